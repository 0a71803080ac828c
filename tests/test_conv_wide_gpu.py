"""The 256-channel conv paths of the width-128 level of GatedHiFiBlock -- conv_gemm_dma_kernel with two channel chunks per
tile and grid.y = 2, its dilation classes, its 256-row instantiation, and conv_wgrad_shift_kernel with 2 x 4 blocks --
against the float64 reference and the derived bound of tests/conv_ref_helpers.py (twice the bound is allowed).

Operands are the channel slices [:, :, 256:512] of 1024-wide bf16 tensors, as in the model; the untouched channels of the
outputs hold a sentinel and must keep it.  Epilogues as the model uses them: "actout-only" (K2 forward, y null), "res" (K3
forward), "actgrad" (K3 data gradient), "res+actgrad" (K2 data gradient).  The conv a descriptor performs has the weights
wc [co][ci][tap]: forward descriptors pack wc with _pack_fwd, data-gradient descriptors pack the torch-layout weight whose
data gradient that conv is (wc flipped along the taps, channels transposed) with _pack_bwd -- one reference serves both.
Every test asserts the kernel's name and plan (tile rows, row classes) before it compares anything.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_ref_helpers as R
from oracle import vqvae_oracle as orc

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
WIDE, SENTINEL = 1024, 7.0
SEED, SITE, P_DROP, THRESH = 3, 5, 0.1, 6554
DROP_SCALE = float(np.float32(1.0) / np.float32(0.9))
K2 = [(3, 1), (5, 3), (7, 9), (9, 27)]
FORWARD = ("actout-only", "res")
B_A, T_A = 5, 6950
LENS_A = (6950, 6949, 3457, 26, 0)       # full; one short; 27 * 128 + 1: a tile edge in the class domain; class 26 empty; empty item
B_B, T_B = 2, 65700
LENS_B = (65700, 40001)


def _slice(c):
    return slice(256, 256 + c)


@functools.lru_cache(maxsize=1)
def _operands(b, t):
    g = torch.Generator(device="cuda").manual_seed(100003 * b + t)

    def wide():
        return torch.randn(b, t, WIDE, device="cuda", generator=g)

    return {"x": wide().to(BF), "res": wide().to(BF), "u_src": torch.relu(wide()).to(BF)}


@functools.lru_cache(maxsize=None)
def _weights(c, k):
    """wc (fp32, what the forward descriptor packs), its data-gradient twin, the bias."""
    g = torch.Generator(device="cuda").manual_seed(31 * c + k)
    wc = torch.randn(c, c, k, device="cuda", generator=g) / (c * k) ** 0.5
    bias = torch.randn(c, device="cuda", generator=g)
    return wc, wc.flip(2).transpose(0, 1).contiguous(), bias


def _lens(lens):
    return None if lens is None else torch.tensor(lens, device="cuda", dtype=torch.int32)


@functools.lru_cache(maxsize=2)
def _reference(b, t, t_cut, c, k, dil, pad, lens):
    """(a, mag) of the bias-free conv of the first t_cut rows of the (b, t) operands: computed once, never modified."""
    x = _operands(b, t)["x"][:, :t_cut, _slice(c)]
    return R.conv_ref(x, _weights(c, k)[0].to(BF), None, dil, pad, _lens(lens))


@pytest.fixture(scope="module", autouse=True)
def _release_caches():
    yield
    for f in (_operands, _weights, _reference):
        f.cache_clear()
    torch.cuda.empty_cache()


def _run(b, t, t_cut, c, k, dil, pad, epi, lens, dma=True):
    """One launch; returns (y_big, u_big, kernel name, plan)."""
    from smt_amd import convops as C
    ops, sl = _operands(b, t), _slice(c)
    x = ops["x"][:, :t_cut, sl]
    t_out = t_cut + 2 * pad - dil * (k - 1)
    wc, wt, bias = _weights(c, k)
    lens32 = _lens(lens)
    y_big = torch.full((b, t_out, WIDE), SENTINEL, device="cuda", dtype=BF)
    u_big = torch.full((b, t_out, WIDE), SENTINEL, device="cuda", dtype=BF)
    y, u = y_big[:, :, sl], u_big[:, :, sl]
    if epi in FORWARD:
        wp = C._pack_fwd(wc, BF, dma)
        d = C._base_desc(x, None if epi == "actout-only" else y, lens32, c, c, k, 1, dil, pad, t_out, t_y=t_out)
        d.w, d.bias = C._p(wp), C._p(bias)
    else:
        wp = C._pack_bwd(wt, BF, dma)
        d = C._dgrad_stride1(x, wp, y, k, dil, (k - 1) * dil - pad)
        d.lens_in = C._p(lens32)
    if dma:
        C._use_dma(d, wp)
    d.lens_out = C._p(lens32)
    if "res" in epi:
        d.res, d.bs_res, d.ld_res = C._geom(ops["res"][:, :t_out, sl])
    if "actgrad" in epi:
        C._set_act_grad(d, ops["u_src"][:, :t_out, sl], DROP_SCALE)
    if epi == "actout-only":
        C._set_act_out(d, u, [C.dropout_key(SEED, SITE)], THRESH, DROP_SCALE, c)
    name, plan = C._kernel_of(d), C._dma_plan_of(d)
    if dma:
        assert name == "conv_gemm_dma", name
    C._launch(d, "t")
    torch.cuda.synchronize()
    return y_big, u_big, name, plan


def _compare(b, t, t_cut, c, k, dil, pad, epi, lens, y_big, u_big):
    """Every row of both outputs against float64 within the bound; masked rows, sentinels, kept fraction."""
    ops, sl = _operands(b, t), _slice(c)
    t_out = t_cut + 2 * pad - dil * (k - 1)
    a, mag = _reference(b, t, t_cut, c, k, dil, pad, lens)
    lens32 = _lens(lens)
    res = ops["res"][:, :t_out, sl]
    kw = {"lens_out": lens32}
    if epi in FORWARD:
        bias = _weights(c, k)[2].double()
        a, mag = a + bias, mag + bias.abs()
    if "res" in epi:
        kw["res"] = res
    if "actgrad" in epi:
        kw.update(act_grad_src=ops["u_src"][:, :t_out, sl], scale=DROP_SCALE)
    keep = None
    if epi == "actout-only":
        keep = R.keep_mask(SEED, SITE, b, t_out, c, P_DROP, "cuda")
        kw.update(keep=keep, drop_scale=DROP_SCALE)
    ref = R.epilogue_ref(a, mag, c * k, **kw)
    valid = R.row_mask(lens32, t_out) if lens32 is not None else torch.ones(b, t_out, 1, dtype=torch.bool, device="cuda")
    y, u = y_big[:, :, sl], u_big[:, :, sl]
    tag = f"k{k} d{dil} {epi} lens={lens} T={t_cut}"
    for big in (y_big, u_big):                                    # channels outside the slice: untouched
        assert bool((big[:, :, :sl.start] == SENTINEL).all()) and bool((big[:, :, sl.stop:] == SENTINEL).all()), tag
    if epi == "actout-only":
        assert bool((y == SENTINEL).all()), tag                   # y is null: nothing written
        R.check(tag + " u", u, ref["u"], ref["u_bound"])
        assert float((u.float() * (~valid)).abs().max()) == 0, tag          # u is exactly 0 on rows >= lens_out
        sure = (ref["y"] > R.SLACK * ref["y_bound"]) & valid                # pre-activations that are positive for certain
        assert int(sure.sum()) > 1000 * b
        assert torch.equal((u != 0)[sure], keep[sure]), tag
        frac = float((u != 0)[sure].float().mean())
        print(f"  {tag}: kept fraction {frac:.4f}")
        assert abs(frac - (1.0 - P_DROP)) < 0.01, tag
    else:
        assert bool((u_big == SENTINEL).all()), tag
        R.check(tag + " y", y, ref["y"], ref["y_bound"])
        want = res if "res" in epi else torch.zeros_like(y)       # rows >= lens_out: the residual bit for bit, or 0
        assert torch.equal(torch.where(valid, want, y), want), tag
    assert float(ref["y"].abs().max()) > 0.5


def _plan_of(k, dil, t, big):
    return (256 if big else 128, dil if dil >= 8 and t // dil >= 128 else 1)


# ---- (a) 128-row tiles, with and without classes ----------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["actout-only", "res+actgrad"])          # innermost: both share one cached reference
@pytest.mark.parametrize("lens", [None, LENS_A], ids=["full", "ragged"])
@pytest.mark.parametrize("k,dil", K2)
def test_k2_at_256_channels_128_row_tiles_matches_float64(k, dil, lens, epi):
    """K2 forward and K2 data gradient at 256 channels, B = 5, T = 6950: two channel chunks, grid.y = 2, for dilation 9
    and 27 the classes with unequal row counts (27: classes 0-10 have 258 rows, 11-26 have 257; the third tile of a class
    holds 2 rows or 1), lens that end on a class tile edge, leave a class empty, and an empty item."""
    pad = (k - 1) * dil // 2
    y_big, u_big, name, plan = _run(B_A, T_A, T_A, 256, k, dil, pad, epi, lens)
    assert plan == _plan_of(k, dil, T_A, False) and plan[1] == (dil if dil >= 9 else 1)
    _compare(B_A, T_A, T_A, 256, k, dil, pad, epi, lens, y_big, u_big)


@pytest.mark.parametrize("epi", ["res", "actgrad"])
@pytest.mark.parametrize("lens", [None, LENS_A], ids=["full", "ragged"])
def test_k3_at_256_channels_matches_float64(lens, epi):
    """K3 forward (residual) and K3 data gradient (activation derivative) at 256 channels: taps == 1 with two chunks."""
    y_big, u_big, name, plan = _run(B_A, T_A, T_A, 256, 1, 1, 0, epi, lens)
    assert plan == (128, 1)
    _compare(B_A, T_A, T_A, 256, 1, 1, 0, epi, lens, y_big, u_big)


@pytest.mark.parametrize("t", [3455, 3456])
def test_both_sides_of_the_class_threshold_match_float64(t):
    """k = 9, dilation 27, B = 2: T = 3455 runs without classes (a 216-row halo per tile), T = 3456 with 27 classes of 128
    rows; the operands of the shorter run are the first 3455 rows of the longer one's."""
    for epi in ("actout-only", "res+actgrad"):
        y_big, u_big, name, plan = _run(2, 3456, t, 256, 9, 27, 108, epi, None)
        assert plan == (128, 27 if t == 3456 else 1)
        _compare(2, 3456, t, 256, 9, 27, 108, epi, None, y_big, u_big)


# ---- (b) 256-row tiles ------------------------------------------------------------------------------------------------
def _big_tile_case(c, k, dil, pad, epi):
    y_big, u_big, name, plan = _run(B_B, T_B, T_B, c, k, dil, pad, epi, LENS_B)
    assert plan == _plan_of(k, dil, T_B, True)
    _compare(B_B, T_B, T_B, c, k, dil, pad, epi, LENS_B, y_big, u_big)
    y_gen, u_gen, name_gen, plan_gen = _run(B_B, T_B, T_B, c, k, dil, pad, epi, LENS_B, dma=False)
    assert name_gen == "conv_gemm" and plan_gen == (0, 0)
    assert torch.equal(y_big, y_gen) and torch.equal(u_big, u_gen)


@pytest.mark.parametrize("epi", ["actout-only", "res+actgrad"])
@pytest.mark.parametrize("k,dil", K2)
def test_k2_at_256_channels_256_row_tiles_matches_float64_and_the_generic_kernel(k, dil, epi):
    """conv_gemm_dma_kernel<4>: B = 2, T = 65,700 (131,400 class rows or more for every geometry), lens [65700, 40001],
    every row against float64.  Against the register-staged generic kernel the outputs are bit-identical: both walk the
    128-channel chunks outermost, the taps inside and the 16-channel MFMA steps innermost, on the same MFMA, and share the
    epilogue's arithmetic, so every fp32 sum sees the same terms in the same order."""
    _big_tile_case(256, k, dil, (k - 1) * dil // 2, epi)


@pytest.mark.parametrize("epi", ["actout-only", "res+actgrad"])
def test_single_chunk_256_row_tile_matches_float64_and_the_generic_kernel(epi):
    """c = 128 with an even tap count (k = 4, padding 1: one output row fewer), which the weight-stationary kernels do
    not take: conv_gemm_dma_kernel<4> with one channel chunk.  Bit-identical to the generic kernel, as above."""
    _big_tile_case(128, 4, 1, 1, epi)


# ---- (c) the shift weight gradient at 256 channels --------------------------------------------------------------------
@pytest.mark.parametrize("lens", [None, LENS_A], ids=["full", "ragged"])
@pytest.mark.parametrize("k,dil", K2)
def test_shift_wgrad_at_256_channels_matches_float64(k, dil, lens):
    """conv_wgrad_shift_kernel with nblk_ci = 2, nblk_co = 4 on the operands of (a) (270 or more 128-row tiles for every
    geometry): dW and db against float64 with the fp32-accumulation bound; a one-hot dy picks out the shifted input rows
    exactly, zero where the row is beyond lens or outside the item."""
    from smt_amd import convops as C
    ops, sl = _operands(B_A, T_A), _slice(256)
    x, dy = ops["x"][:, :, sl], ops["res"][:, :, sl]
    lens32 = _lens(lens)
    pad = (k - 1) * dil // 2

    def wgrad(dout):
        dw = torch.full((256, 256, k), 9.0, device="cuda")
        db = torch.full((256,), 9.0, device="cuda")
        d = C._base_desc(x, dout, lens32, 256, 256, k, 1, dil, pad, T_A)
        C._wgrad(d, dw, 256 * k, k, 1, list(range(k)), db)
        torch.cuda.synchronize()
        assert C.N.lib().smt_conv1d_wgrad_kernel_name(ctypes.byref(d)).decode() == "conv_wgrad_shift"
        return dw, db

    dw, db = wgrad(dy)
    dw_ref, db_ref = R.wgrad_ref(x, dy, k, dil, pad, lens32)
    tol_w, tol_b = R.wgrad_bounds(dw_ref, db_ref, B_A * T_A)
    err_w, err_b = float((dw.double() - dw_ref).abs().max()), float((db.double() - db_ref).abs().max())
    print(f"  k{k} d{dil} lens={lens}: dW err {err_w:.3e} (bound {tol_w:.3e}), db err {err_b:.3e} (bound {tol_b:.3e})")
    assert err_w <= tol_w and err_b <= tol_b
    for item, m in ((1, 6940), (2, 3456)):               # near the end of an item; the class tile edge at 27 * 128
        hot_big = torch.zeros(B_A, T_A, WIDE, device="cuda", dtype=BF)
        hot_big[item, m, 256 + 5] = 1
        dwh, dbh = wgrad(hot_big[:, :, sl])
        limit = T_A if lens is None else lens[item]
        for s in range(k):
            r = m + s * dil - pad
            want = x[item, r].float() if 0 <= r < limit else torch.zeros(256, device="cuda")
            assert torch.equal(dwh[5, :, s], want), (item, m, s)
        assert float(dwh[:5].abs().max()) == 0 and float(dwh[6:].abs().max()) == 0 and float(dbh.sum()) == 1.0


# ---- (d) the width-128 block ------------------------------------------------------------------------------------------
def test_gated_hifi_w128_unfolded_wiring_train_mode_vs_oracle():
    """GatedHiFiBlock(128, 4) in bf16, train mode: the wiring of the wide level -- the h1 residual, four unfused K3
    launches, the 1024-wide K1 with four dropout sites, the generic K1 backward -- against the oracle with the block
    tolerances of test_fastpath_parity_gpu.py (relative L2: 1e-2 forward, 7e-2 gradients)."""
    from models.vqvae.resnet import GatedHiFiBlock
    from smt_amd import profiler
    torch.manual_seed(13)
    w, depth, site_base, seed, p_drop = 128, 4, 16, 11, 0.1
    b, t = 3, 3470
    blk = GatedHiFiBlock(w, depth, dilation_growth_rate=3, kernel_size_growth_rate=2, zero_out=False, dropout=p_drop,
                         site_base=site_base).cuda()
    blk.train()
    g = torch.Generator().manual_seed(6)
    x_nct = torch.randn(b, w, t, generator=g).to(BF).float()
    dy_nct = torch.randn(b, w, t, generator=g).to(BF).float()
    lens = torch.tensor([3470, 2001, 129])
    xa = x_nct.permute(0, 2, 1).contiguous().cuda().to(BF).requires_grad_(True)
    profiler.reset(); profiler.enable(True)
    try:
        y = blk(xa, lens.cuda().to(torch.int32), drop_seed=seed)
        y.backward(dy_nct.permute(0, 2, 1).contiguous().cuda().to(BF))
        names = {r["name"] for r in profiler.summary()}
    finally:
        profiler.enable(False); profiler.reset()
    assert {"conv_gemm_dma:fwd", "conv_gemm_dma:dgrad"} <= names, sorted(names)
    assert not any(n.startswith(("conv_k1act", "conv_k3gate", "conv1x1_fold", "conv1x1_c64", "conv_ws")) for n in names), sorted(names)
    # the unfused pieces: K1 and its backward on the generic kernel, the gate mix on its own, no fused backward kernels
    assert {"conv_gemm:fwd", "conv_gemm:dgrad", "gate_mix_fwd", "gate_mix_bwd"} <= names, sorted(names)
    assert not any(n.startswith(("conv1x1_bwd", "conv_k1_bwd", "conv_gate_bwd")) for n in names), sorted(names)

    sd = {k: v.detach().cpu() for k, v in blk.state_dict().items()}
    prm = {"b." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ids = {f"b.blocks.{d}.1.drop{s}": site_base + 2 * d + s for d in range(depth) for s in (0, 1)}
    drop = orc.make_counter_dropout(seed, p_drop, ids)
    xr = x_nct.clone().requires_grad_(True)
    mask = orc.sequence_mask(lens, t).unsqueeze(1).float()
    yr = orc.gated_hifi_block(xr, mask, prm, "b", orc.VQVAEConfig(width=w, multipliers=(1, 1, 1)), drop)
    yr.backward(dy_nct)

    def rel_l2(got, want):
        got, want = got.detach().float().cpu(), want.detach().float().cpu()
        return ((got - want).norm() / (want.norm() + 1e-30)).item()

    errs = {"y": rel_l2(y.permute(0, 2, 1), yr), "dx": rel_l2(xa.grad.permute(0, 2, 1), xr.grad)}
    for name, q in blk.named_parameters():
        errs[name] = rel_l2(q.grad, prm["b." + name].grad)
    print("\n" + "\n".join(f"  {k:32s} {v:.3e}" for k, v in errs.items()))
    assert errs["y"] <= 1e-2, errs
    bad = {k: v for k, v in errs.items() if k != "y" and v > 7e-2}
    assert not bad, bad
