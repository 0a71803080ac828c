"""The WaveNet gate kernels and the fused tail on the GPU, every element against the bounds of tests/wavenet_helpers.py
(derived in DESIGN.md section 20): all widths and row counts at which the kernels take another path (one row, a tile of 32 or
128 rows and its neighbours, more than one block), a full, a ragged and an empty batch item, pitches larger than the width;
rows at or past lens[b] are not read (NaN poison) and come out as exact zeros; equal inputs give equal bits; the op
``wavenet_tail`` on its fused and unfused paths."""
import pytest
import torch

import wavenet_helpers as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
TS = (1, 2, 127, 128, 129, 257)
F32, BF16 = torch.float32, torch.bfloat16


def lens_of(t):
    """A full, a ragged and an empty item."""
    return torch.tensor([t, (t + 1) // 2, 0], dtype=torch.int32)


def pitched(shape, dtype, pad, fill):
    """A [B, T, C] view with row pitch C + pad into a buffer filled with `fill` (what lies between the rows must never matter
    and never change)."""
    b, t, c = shape
    buf = torch.full((b, t, c + pad), fill, dtype=dtype, device=DEV)
    return buf, buf[:, :, :c]


def z_values(t, hidden, dtype, seed):
    """z over the stated domain [-8, 8], with the values at which the gate function changes its form: 0, the series
    threshold 1/16 and its neighbours, tiny and extreme arguments."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.rand(B, t, 2 * hidden, generator=g) * 2 - 1) * W.GATE_DOMAIN
    special = torch.tensor([0.0, -0.0, 0.0625, -0.0625, 0.0624, 0.0626, 1e-3, -1e-3, 1e-6, 8.0, -8.0, 3e-5])
    n = min(special.numel(), 2 * hidden)
    z[:, 0, :n] = special[:n]
    z[:, -1, 2 * hidden - n:] = special[:n]
    return z.to(dtype)


def valid_rows(lens, t):
    return (torch.arange(t)[None, :] < lens[:, None].long())


def run_gate(z, lens, pad=8, poison=False, da=None):
    """(a, dz or None) from the two kernels on pitched tensors; with `poison`, rows at or past lens hold NaN in z and da and
    the outputs are pre-filled with garbage."""
    from smt_amd import convops
    b, t, c = z.shape
    h = c // 2
    valid = valid_rows(lens, t).to(DEV)
    zbuf, zv = pitched((b, t, c), z.dtype, pad, 7.0)
    zv.copy_(z)
    if poison:
        zv[~valid] = float("nan")
    abuf, av = pitched((b, t, h), z.dtype, pad, 123.0)
    convops._wavenet_gate_fwd(zv, av, lens.to(DEV))
    assert bool((abuf[:, :, h:] == 123.0).all())                   # nothing is written between the rows
    dzv = None
    if da is not None:
        dabuf, dav = pitched((b, t, h), z.dtype, pad, 5.0)
        dav.copy_(da)
        if poison:
            dav[~valid] = float("nan")
        dzbuf, dzv = pitched((b, t, c), z.dtype, pad, -77.0)
        convops._wavenet_gate_bwd(zv, dav, dzv, lens.to(DEV))
        assert bool((dzbuf[:, :, c:] == -77.0).all())
    torch.cuda.synchronize()
    return av.cpu(), (None if dzv is None else dzv.cpu())


@pytest.mark.parametrize("dtype,hidden", [(F32, 8), (F32, 24), (F32, 64), (F32, 136), (BF16, 16), (BF16, 64), (BF16, 128)])
def test_gate_against_float64(dtype, hidden):
    worst_f = worst_b = 0.0
    for t in TS:
        lens = lens_of(t)
        valid = valid_rows(lens, t)
        z = z_values(t, hidden, dtype, seed=t + hidden)
        da = torch.randn(B, t, hidden, generator=torch.Generator().manual_seed(t)).to(dtype)
        a, dz = run_gate(z.to(DEV), lens, da=da.to(DEV))
        a64, dz64 = W.gate64(z), W.gate_grad64(z, da)                 # z, da as the device reads them
        if dtype == F32:
            bound_f = torch.full_like(a64, W.E_F)
            bound_b = W.E_B * da.double().abs().repeat(1, 1, 2)
        else:
            bound_f = W.BF16_GATE_REL * a64.abs()
            bound_b = W.BF16_OUT_REL * dz64.abs() + W.E_B * da.double().abs().repeat(1, 1, 2)
        err_f, err_b = (a.double() - a64).abs(), (dz.double() - dz64).abs()
        worst_f = max(worst_f, (err_f[valid] / bound_f[valid].clamp_min(1e-300)).max().item() if valid.any() else 0.0)
        worst_b = max(worst_b, (err_b[valid] / bound_b[valid].clamp_min(1e-300)).max().item() if valid.any() else 0.0)
        assert bool((err_f[valid] <= bound_f[valid]).all()), (t, "forward")
        assert bool((err_b[valid] <= bound_b[valid]).all()), (t, "backward")
        assert bool((a[~valid] == 0).all()) and bool((dz[~valid] == 0).all()), (t, "rows past lens are zero")
    print(f"gate {dtype} H={hidden}: worst error / bound forward {worst_f:.3f}, backward {worst_b:.3f}")


@pytest.mark.parametrize("dtype,hidden", [(F32, 24), (BF16, 64)])
def test_gate_reads_no_padded_row_and_is_reproducible(dtype, hidden):
    for t in (2, 129):
        lens = lens_of(t)
        valid = valid_rows(lens, t)
        z = z_values(t, hidden, dtype, seed=3).to(DEV)
        da = torch.randn(B, t, hidden, device=DEV).to(dtype)
        a, dz = run_gate(z, lens, da=da)
        a2, dz2 = run_gate(z, lens, da=da)
        assert torch.equal(a, a2) and torch.equal(dz, dz2)                                  # two calls, equal bits
        ap, dzp = run_gate(z, lens, da=da, poison=True)
        assert torch.equal(ap[valid], a[valid]) and torch.equal(dzp[valid], dz[valid])
        assert bool((ap[~valid] == 0).all()) and bool((dzp[~valid] == 0).all())
        # no lens: every row is valid
        from smt_amd import convops
        full = torch.empty(B, t, hidden, dtype=dtype, device=DEV)
        convops._wavenet_gate_fwd(z, full, None)
        assert torch.equal(full.cpu()[valid], a[valid]) and bool(torch.isfinite(full.float()).all())


# ---- the fused tail -------------------------------------------------------------------------------------------------------
def tail_inputs(t, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    z = z_values(t, hidden, BF16, seed)
    x = torch.randn(B, t, hidden, generator=g).to(BF16)
    weight = ((torch.rand(hidden, hidden, 1, generator=g) * 2 - 1) / hidden ** 0.5)
    bias = 0.1 * torch.randn(hidden, generator=g)
    return z, x, weight, bias


def run_tail(z, x, weight, bias, lens, pad=8, poison=False):
    """y of smt_wavenet_tail_fwd on pitched tensors (through the packed-weight cache, as the op calls it)."""
    import ctypes
    from smt_amd import convops, native
    b, t, h = x.shape
    valid = valid_rows(lens, t).to(DEV)
    zbuf, zv = pitched((b, t, 2 * h), BF16, pad, 7.0)
    xbuf, xv = pitched((b, t, h), BF16, 2 * pad, 9.0)
    ybuf, yv = pitched((b, t, h), BF16, pad, 123.0)
    zv.copy_(z)
    xv.copy_(x)
    if poison:
        zv[~valid] = float("nan")
        xv[~valid] = float("nan")
    wp = convops._pack_fwd(weight.to(DEV), BF16)
    bias_d, lens_d = bias.to(DEV), lens.to(DEV)
    (pz, bsz, ldz), (px, bsx, ldx), (py, bsy, ldy) = convops._geom(zv), convops._geom(xv), convops._geom(yv)
    native.check(native.lib().smt_wavenet_tail_fwd(pz, bsz, ldz, px, bsx, ldx, ctypes.c_void_p(wp.data_ptr()),
                                                   ctypes.c_void_p(bias_d.data_ptr()), py, bsy, ldy,
                                                   ctypes.c_void_p(lens_d.data_ptr()), b, t, h, native.stream_ptr()),
                 "smt_wavenet_tail_fwd")
    torch.cuda.synchronize()
    assert bool((ybuf[:, :, h:] == 123.0).all())
    return yv.cpu()


@pytest.mark.parametrize("hidden", [64, 128])
def test_tail_against_float64(hidden):
    worst = 0.0
    for t in TS:
        lens = lens_of(t)
        valid = valid_rows(lens, t)
        z, x, weight, bias = tail_inputs(t, hidden, seed=10 * t + hidden)
        y = run_tail(z.to(DEV), x.to(DEV), weight, bias, lens)
        y64, s = W.tail64(z, x, weight.to(BF16), bias)               # on the bf16-rounded z, x, W_g
        bound = W.tail_bound(y64, s, hidden)
        err = (y.double() - y64).abs()
        if valid.any():
            worst = max(worst, (err[valid] / bound[valid]).max().item())
        assert bool((err[valid] <= bound[valid]).all()), t
        assert bool((y[~valid] == 0).all()), t
    print(f"tail H={hidden}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("hidden", [64, 128])
def test_tail_reads_no_padded_row_and_is_reproducible(hidden):
    for t in (2, 129):
        lens = lens_of(t)
        valid = valid_rows(lens, t)
        z, x, weight, bias = tail_inputs(t, hidden, seed=5)
        y = run_tail(z.to(DEV), x.to(DEV), weight, bias, lens)
        assert torch.equal(run_tail(z.to(DEV), x.to(DEV), weight, bias, lens), y)
        yp = run_tail(z.to(DEV), x.to(DEV), weight, bias, lens, poison=True)
        assert torch.equal(yp[valid], y[valid]) and bool((yp[~valid] == 0).all())


def test_tail_lane_map_with_exact_integers():
    """Small integers and an ASYMMETRIC weight: every product and sum is exact in bf16 / fp32, so a transposed or permuted
    fragment shows as a wrong integer.  The gate is pinned to 1 * 1/2 ... by z = (large, 0): tanh = 1, sigmoid = 1/2."""
    for hidden in (64, 128):
        t = 40
        z = torch.zeros(B, t, 2 * hidden)                              # tanh(30) = 1 in fp32, sigmoid(0) = 1/2
        sel = torch.zeros(B, t, hidden)
        sel[torch.arange(B)[:, None], torch.arange(t)[None, :], (torch.arange(t)[None, :] * 7 + torch.arange(B)[:, None]) % hidden] = 1
        z[..., :hidden] = torch.where(sel.bool(), 30.0, 0.0)           # one live input channel per row: a = 1/2 there, 0 elsewhere
        o, i = torch.arange(hidden)[:, None], torch.arange(hidden)[None, :]
        weight = ((2 * ((3 * o + 5 * i) % 17) - 16).float()).unsqueeze(-1)           # even integers in [-16, 16], asymmetric
        x = ((torch.arange(t)[None, :, None] + torch.arange(hidden)[None, None, :]) % 5).float().expand(B, t, hidden)
        bias = torch.arange(hidden).float() % 3
        lens = torch.tensor([t, 33, 0], dtype=torch.int32)
        y = run_tail(z.to(BF16).to(DEV), x.to(BF16).to(DEV), weight, bias, lens)
        y64, _ = W.tail64(z, x, weight, bias)
        valid = valid_rows(lens, t)
        assert torch.equal(y.double()[valid], y64[valid])


# ---- the op on both paths ---------------------------------------------------------------------------------------------------
def _op(hidden, fused, t=129, lens=(129, 65, 7)):
    from smt_amd import convops, profiler
    z0, x0, w0, b0 = tail_inputs(t, hidden, seed=21)
    z, x = z0.to(DEV).requires_grad_(True), x0.to(DEV).requires_grad_(True)
    weight, bias = w0.to(DEV).requires_grad_(True), b0.to(DEV).requires_grad_(True)
    lens = torch.tensor(lens, dtype=torch.int32)
    valid = valid_rows(lens, t)
    r = torch.randn(B, t, hidden, generator=torch.Generator().manual_seed(2)) * valid[..., None]
    old = (convops._WN_TAIL, convops._WN_TAIL_WIDTHS)
    convops._WN_TAIL, convops._WN_TAIL_WIDTHS = fused, (64, 128)
    profiler.enable(True)
    profiler.reset()
    try:
        y = convops.wavenet_tail(z, x, weight, bias, lens.to(DEV))
        fwd_names = set(profiler._records)
        saved = [tuple(s.shape) for s in y.grad_fn.saved_tensors] if fused else None
        (y.float() * r.to(DEV)).sum().backward()
        names = set(profiler._records)
    finally:
        profiler.enable(False)
        profiler.reset()
        convops._WN_TAIL, convops._WN_TAIL_WIDTHS = old
    torch.cuda.synchronize()
    grads = {"dz": z.grad.cpu(), "dx": x.grad.cpu(), "dw": weight.grad.cpu(), "db": bias.grad.cpu()}
    return dict(y=y.detach().cpu(), grads=grads, fwd_names=fwd_names, names=names, saved=saved, inputs=(z0, x0, w0, b0), valid=valid, r=r)


@pytest.mark.parametrize("hidden", [64, 128])
def test_op_fused_and_unfused(hidden):
    on, off = _op(hidden, True), _op(hidden, False)
    # the region names prove which path ran
    assert "wavenet_tail" in on["fwd_names"] and "wavenet_gate_fwd" not in on["fwd_names"]
    assert {"wavenet_gate_fwd", "wavenet_gate_bwd"} <= on["names"]                        # backward recomputes a, then the gate's backward
    assert "wavenet_tail" not in off["names"] and {"wavenet_gate_fwd", "wavenet_gate_bwd"} <= off["names"]
    assert any(n.startswith("conv") for n in off["fwd_names"])
    # the fused forward keeps z, the weight and lens: no [B, T, H] tensor
    t = on["y"].shape[1]
    assert sorted(on["saved"]) == sorted([(B, t, 2 * hidden), (hidden, hidden, 1), (B,)])
    assert (B, t, hidden) not in on["saved"]
    # both satisfy the forward bound on valid rows; the fused path writes zeros on the others
    z0, x0, w0, b0 = on["inputs"]
    valid = on["valid"]
    y64, s = W.tail64(z0, x0, w0.to(BF16), b0)
    bound = W.tail_bound(y64, s, hidden)
    for run in (on, off):
        assert bool(((run["y"].double() - y64).abs()[valid] <= bound[valid]).all())
    assert bool((on["y"][~valid] == 0).all())
    # gradients: against float64 autograd and against each other, at the project's bf16 block tolerance
    p = [v.double().requires_grad_(True) for v in (z0, x0, w0, b0)]
    (W.tail64(*p)[0] * on["r"].double()).sum().backward()
    ref = dict(zip(("dz", "dx", "dw", "db"), (v.grad for v in p)))
    for name in ref:
        m = valid[..., None] if name in ("dz", "dx") else 1
        e_on, e_off = W.rel_l2(on["grads"][name] * m, ref[name] * m), W.rel_l2(off["grads"][name] * m, ref[name] * m)
        e_pair = W.rel_l2(on["grads"][name] * m, off["grads"][name] * m)
        print(f"H={hidden} {name}: fused {e_on:.2e}, unfused {e_off:.2e}, fused vs unfused {e_pair:.2e}")
        assert e_on <= 7e-2 and e_off <= 7e-2 and e_pair <= 7e-2, name
    # under no_grad nothing is kept
    from smt_amd import convops
    old = (convops._WN_TAIL, convops._WN_TAIL_WIDTHS)
    convops._WN_TAIL, convops._WN_TAIL_WIDTHS = True, (64, 128)
    try:
        with torch.no_grad():
            y = convops.wavenet_tail(z0.to(DEV), x0.to(DEV), w0.to(DEV), b0.to(DEV), torch.tensor([129, 65, 7], device=DEV))
    finally:
        convops._WN_TAIL, convops._WN_TAIL_WIDTHS = old
    assert y.grad_fn is None and torch.equal(y.cpu()[valid], on["y"][valid])
