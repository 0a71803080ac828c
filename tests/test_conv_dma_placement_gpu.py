"""The weight-stationary convs and the shifted-fragment weight gradient at the shapes where the placement of their LDS-DMA
pieces can go wrong: the fewest and the most input pieces per wave, dilation classes, a last workgroup / chunk of exactly
one tile (no prefetch at all), and ragged items whose tiles lie wholly outside the staging descriptors' range.
Forward and data gradient: bit-identical to the register-staged generic kernel.  Weight gradient: against float64, and
bit-identical from run to run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

C128 = 128
WS_T = 32801        # 2 x 257 = 514 tiles of 128 rows (>= 512: weight-stationary), 3 per workgroup: the last one gets 1 tile
WG_T = 32929        # 2 x 258 = 516 tiles in chunks of 5: the last chunk has 1 tile
WS_GEOMS = [(5, 1), (5, 3), (7, 1), (7, 7), (9, 1), (9, 7), (7, 9), (9, 27)]   # rows_pad 132 .. 184; dilation >= 8: classes
WG_GEOMS = [(3, 1), (5, 3), (7, 7), (9, 7), (7, 9), (9, 27)]


def _ws_pair(k, dil, epi, lens_list):
    """(names, outputs) of the generic and of the weight-stationary kernel on the same inputs."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(300 + 10 * k + dil)
    b, t, c = 2, WS_T, C128
    big = torch.randn(b, t, 256, device="cuda", generator=g).to(torch.bfloat16)
    x = big[:, :, 128:256]                                   # channel slice: row pitch 256
    w = torch.randn(c, c, k, device="cuda", generator=g) / (c * k) ** 0.5
    bias = torch.randn(c, device="cuda", generator=g)
    res = torch.randn(b, t, c, device="cuda", generator=g).to(torch.bfloat16)
    u_src = torch.relu(torch.randn(b, t, c, device="cuda", generator=g)).to(torch.bfloat16)
    lens = torch.tensor(lens_list, device="cuda", dtype=torch.int32)
    pad = (k - 1) * dil // 2
    outs, names = [], []
    for dma in (False, True):
        y = torch.zeros(b, t, c, device="cuda", dtype=torch.bfloat16)
        u = torch.zeros_like(y)
        wp = C._pack_fwd(w, torch.bfloat16, dma)
        d = C._base_desc(x, None if epi == "actout-only" else y, lens, c, c, k, 1, dil, pad, t, t_y=t)
        d.w, d.bias = C._p(wp), C._p(bias)
        if dma:
            C._use_dma(d, wp)
        d.lens_out = C._p(lens)
        if epi == "res+actgrad":
            d.res, d.bs_res, d.ld_res = C._geom(res)
            C._set_act_grad(d, u_src, 1.111)
        else:
            C._set_act_out(d, u, [C.dropout_key(3, 5)], 6554, 1.0 / 0.9, c)
        names.append(C._kernel_of(d))
        C._launch(d, "t")
        torch.cuda.synchronize()
        outs.append((y, u))
    return names, outs


def _check_ws(k, dil, epi, lens_list):
    names, outs = _ws_pair(k, dil, epi, lens_list)
    assert names == ["conv_gemm", "conv_ws_pipe" if epi == "actout-only" else "conv_ws"]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert (outs[0][1] if epi == "actout-only" else outs[0][0]).float().abs().sum() > 0


@pytest.mark.parametrize("k,dil", WS_GEOMS)
@pytest.mark.parametrize("epi", ["actout-only", "res+actgrad"])
def test_weight_stationary_kernels_match_generic_kernel_at_the_placement_edges(k, dil, epi):
    """K2 forward (pipelined kernel) and K2 data gradient (MODE 2) with a ragged second item: whole tiles of it read out of
    range, and the last workgroup runs a single tile."""
    _check_ws(k, dil, epi, [WS_T, 12345])


@pytest.mark.parametrize("epi", ["actout-only", "res+actgrad"])
def test_weight_stationary_kernels_match_generic_kernel_on_a_one_row_item(epi):
    _check_ws(7, 7, epi, [WS_T, 1])


def _wgrad(k, dil, lens_list, seed):
    """(dw, db, x, dy, lens, pad) of the shift weight gradient on channel slices of wider tensors."""
    from smt_amd import convops as C
    import ctypes
    g = torch.Generator(device="cuda").manual_seed(seed)
    b, t, c = 2, WG_T, C128
    xb = torch.randn(b, t, 256, device="cuda", generator=g).to(torch.bfloat16)
    dyb = torch.randn(b, t, 384, device="cuda", generator=g).to(torch.bfloat16)
    x, dy = xb[:, :, 128:256], dyb[:, :, 128:256]
    lens = torch.tensor(lens_list, device="cuda", dtype=torch.int32)
    pad = (k - 1) * dil // 2

    def run():
        dw, db = torch.empty(c, c, k, device="cuda"), torch.empty(c, device="cuda")
        d = C._base_desc(x, dy, lens, c, c, k, 1, dil, pad, t)
        d.zero_page = C._p(C._zero_page(dw.device))
        assert C.N.lib().smt_conv1d_wgrad_kernel_name(ctypes.byref(d)).decode() == "conv_wgrad_shift"
        C._wgrad(d, dw, c * k, k, 1, list(range(k)), db)
        torch.cuda.synchronize()
        return dw, db

    return run, x, dy, lens, pad


def _check_wgrad_float64(k, dil, lens_list):
    run, x, dy, lens, pad = _wgrad(k, dil, lens_list, 400 + 10 * k + dil)
    dw, db = run()
    b, t = x.shape[0], x.shape[1]
    mask = (torch.arange(t, device="cuda")[None, :] < lens[:, None])[:, :, None]
    xm = torch.where(mask, x, torch.zeros_like(x)).double()
    xp = torch.nn.functional.pad(xm, (0, 0, pad, pad))
    ref = torch.stack([torch.einsum("bto,bti->oi", dy.double(), xp[:, s * dil:s * dil + t]) for s in range(k)], dim=2)
    tol = 2e-6 * float(ref.abs().max()) * (b * t) ** 0.5 + 1e-4     # fp32 accumulation over b*t rows
    err = float((dw.double() - ref).abs().max())
    dbr = dy.double().sum((0, 1))
    tol_b = 2e-6 * float(dbr.abs().max()) * (b * t) ** 0.5 + 1e-3
    err_b = float((db.double() - dbr).abs().max())
    print(f"k={k} dil={dil} lens={lens_list}: dw err {err:.3e} (tol {tol:.3e}), db err {err_b:.3e} (tol {tol_b:.3e})")
    assert float(ref.abs().max()) > 0
    assert err <= tol
    assert err_b <= tol_b


@pytest.mark.parametrize("k,dil", WG_GEOMS)
def test_shift_wgrad_matches_float64_at_the_placement_edges(k, dil):
    """Ragged second item (whole tiles of x out of the descriptor's range) and a last chunk of one tile."""
    _check_wgrad_float64(k, dil, [WG_T, 12345])


def test_shift_wgrad_matches_float64_when_nearly_every_row_is_out_of_range():
    """First item of length 1: nearly every x row of it is out of range of its descriptor."""
    _check_wgrad_float64(7, 9, [1, 12345])


@pytest.mark.parametrize("k,dil", [(5, 3), (9, 27)])
def test_shift_wgrad_is_bit_identical_from_run_to_run(k, dil):
    run, *_ = _wgrad(k, dil, [WG_T, 12345], 500 + k)
    dw0, db0 = run()
    dw1, db1 = run()
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
