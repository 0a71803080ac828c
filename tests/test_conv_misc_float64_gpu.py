"""conv_in, conv_out and gate_mix (csrc/conv_misc.hip) against the float64 references and derived bounds of
tests/conv_edge_helpers.py, through the C entries (outputs pre-filled with NaN: an unwritten element fails) and through the
smt_amd.convops autograd ops, at the sizes where the kernels take another path: one row, fewer rows than a workgroup covers, a
grid that wraps (the incremental (b, t) advance of conv_in_fwd, the later trips of gate_mix_bwd with dead lanes in the shuffles),
the slab split of the weight gradients with an empty last workgroup, every admitted width, 1 / 4 / 8 taps, empty items.

Which gate_mix backward kernel runs is not reported by the binding; smt_gate_mix_bwd picks it from the geometry alone, with
vpr = width / (8 for bf16, 4 for fp32) channel vectors per row:
  * depth and vpr powers of two and vpr * depth a divisor of 64: the lane-per-branch shuffle kernel -- specialised (DPP row
    rotation and swizzle) at bf16 (64, 4), generic (__shfl_xor) otherwise: bf16 (128, 4), (16, 1), (64, 8); fp32 (64, 4), (16, 1);
  * anything else -- depth 3 or 5, or more than 64 lanes per row as fp32 (128, 4) and (64, 8): the lane-per-channel-vector kernel."""
import ctypes

import pytest
import torch

import conv_edge_helpers as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dt(dtype):
    from smt_amd import convops as C
    return C._DT[dtype]


def _call(name, *args):
    from smt_amd import native as N
    N.check(getattr(N.lib(), name)(*args, N.stream_ptr()), name)


def gen(*key):
    return torch.Generator(device=DEV).manual_seed(1 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def finite(*ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts)


# ------------------------------------------------------------------------------------------------ conv_in
def raw_conv_in_fwd(x, w, bias, lens, stride, pad, dtype):
    b, t_in = x.shape
    c, _, taps = w.shape
    t_out = E.conv_in_t_out(t_in, taps, stride, pad)
    y = torch.full((b, t_out, c), NAN, dtype=dtype, device=DEV)
    _call("smt_conv_in_fwd", _p(x), _p(w), _p(bias), _p(lens), _p(y), _dt(dtype), b, t_in, t_out, c, taps, stride, pad)
    return y


def raw_conv_in_wgrad(x, dy, lens, taps, stride, pad, short=0):
    from smt_amd import native as N
    b, t_in = x.shape
    _, t_out, c = dy.shape
    dw = torch.full((c, 1, taps), NAN, device=DEV)
    db = torch.full((c,), NAN, device=DEV)
    nbytes = N.lib().smt_conv_in_wgrad_workspace_bytes(b, t_out, c)
    ws = torch.full((nbytes // 4,), NAN, device=DEV)
    _call("smt_conv_in_wgrad", _p(x), _p(dy), _p(lens), _p(dw), _p(db), _dt(dy.dtype), b, t_in, t_out, c, taps, stride, pad, _p(ws),
          nbytes - short)
    return dw, db


def conv_in_case(taps, stride, pad, c, b, t_in, dtype):
    g = gen(taps, c, b, t_in)
    x = torch.rand(b, t_in, device=DEV, generator=g) * 2 - 1
    w = torch.randn(c, 1, taps, device=DEV, generator=g) * 0.5
    bias = torch.randn(c, device=DEV, generator=g)
    dy = torch.randn(b, E.conv_in_t_out(t_in, taps, stride, pad), c, device=DEV, generator=g).to(dtype)
    return x, w, bias, dy, E.edge_lens(b, t_in, DEV)


def check_conv_in(taps, stride, pad, c, b, t_in, dtype, forward=True, wgrad=True, op=True):
    from smt_amd import convops as C
    x, w, bias, dy, lens = conv_in_case(taps, stride, pad, c, b, t_in, dtype)
    tag = f"conv_in {'bf16' if dtype == BF else 'f32'} k{taps}s{stride}p{pad} c={c} ({b}, {t_in})"
    t_out = dy.shape[1]
    if t_out == 0:                                       # an input shorter than the kernel: nothing to launch, gradients are zero
        wa, ba = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        y = C.conv_in(x, wa, ba, stride=stride, padding=pad, lens=lens, out_dtype=dtype)
        assert y.shape == (b, 0, c)
        y.backward(dy)
        assert float(wa.grad.abs().max()) == 0.0 and float(ba.grad.abs().max()) == 0.0
        return
    if forward:
        y = raw_conv_in_fwd(x, w, bias, lens, stride, pad, dtype)
        E.check(tag, y, *E.conv_in_ref(x, w, bias, lens, stride, pad, dtype == BF))
    if wgrad:
        dw, db = raw_conv_in_wgrad(x, dy, lens, taps, stride, pad)
        dw_r, dw_b, db_r, db_b = E.conv_in_wgrad_ref(x, dy, lens, taps, stride, pad)
        E.check(tag + " dW", dw, dw_r, dw_b)
        E.check(tag + " db", db, db_r, db_b)
    if op and forward and wgrad:                         # the autograd op runs the same launches
        wa, ba = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        yo = C.conv_in(x, wa, ba, stride=stride, padding=pad, lens=lens, out_dtype=dtype)
        yo.backward(dy)
        assert torch.equal(yo.detach(), y) and torch.equal(wa.grad, dw) and torch.equal(ba.grad, db)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", E.CONV_IN_WIDTHS)
@pytest.mark.parametrize("taps,stride,pad", E.CONV_IN_GEOMS)
def test_conv_in_forward_and_weight_gradient(taps, stride, pad, c, dtype):
    for b, t_in in E.edge_rows(taps):
        check_conv_in(taps, stride, pad, c, b, t_in, dtype)


@pytest.mark.parametrize("taps,stride,pad", E.CONV_IN_GEOMS)
def test_conv_in_forward_at_128_lanes_per_row(taps, stride, pad):
    for b, t_in in E.edge_rows(taps):
        check_conv_in(taps, stride, pad, 512, b, t_in, F32, wgrad=False)


def test_conv_in_forward_when_the_grid_wraps():
    """80000 rows x 16 lanes on 4096 x 256 threads: the second trip advances (b, t) by (1, 25536) and wraps t."""
    check_conv_in(4, 2, 1, 64, 2, 80000, F32)


def test_conv_in_weight_gradient_split_with_an_empty_last_workgroup():
    """524289 rows: 1024 workgroups of 513 rows, the last one starts past the end and must still write zeros to its slab."""
    check_conv_in(4, 2, 1, 8, 1, 2 * 524289, BF, forward=False)


# ------------------------------------------------------------------------------------------------ conv_out
def raw_conv_out(x, w, bias, lens, dy, short=0):
    from smt_amd import native as N
    b, t, c = x.shape
    y = torch.full((b, t), NAN, device=DEV)
    _call("smt_conv_out_fwd", _p(x), _p(w), _p(bias), _p(lens), _p(y), _dt(x.dtype), b, t, c)
    dx = torch.full((b, t, c), NAN, dtype=x.dtype, device=DEV)
    dw = torch.full((1, c, 1), NAN, device=DEV)
    db = torch.full((1,), NAN, device=DEV)
    nbytes = N.lib().smt_conv_out_bwd_workspace_bytes(b, t, c)
    ws = torch.full((nbytes // 4,), NAN, device=DEV)
    _call("smt_conv_out_bwd", _p(x), _p(w), _p(lens), _p(dy), _p(dx), _p(dw), _p(db), _dt(x.dtype), b, t, c, _p(ws), nbytes - short)
    return y, dx, dw, db


def conv_out_case(c, b, t, dtype):
    g = gen(c, b, t, 9)
    x = torch.randn(b, t, c, device=DEV, generator=g).to(dtype)
    w = torch.randn(1, c, 1, device=DEV, generator=g) * 0.1
    bias = torch.randn(1, device=DEV, generator=g)
    dy = torch.randn(b, t, device=DEV, generator=g)
    return x, w, bias, dy, E.edge_lens(b, t, DEV)


def check_conv_out(c, b, t, dtype):
    from smt_amd import convops as C
    x, w, bias, dy, lens = conv_out_case(c, b, t, dtype)
    tag = f"conv_out {'bf16' if dtype == BF else 'f32'} c={c} ({b}, {t})"
    y, dx, dw, db = raw_conv_out(x, w, bias, lens, dy)
    E.check(tag, y, *E.conv_out_ref(x, w, bias, lens))
    dx_r, dx_b, dw_r, dw_b, db_r, db_b = E.conv_out_bwd_ref(x, w, dy, lens, dtype == BF)
    E.check(tag + " dx", dx, dx_r, dx_b)
    E.check(tag + " dw", dw, dw_r, dw_b)
    E.check(tag + " db", db, db_r, db_b)
    padded = ~E.row_mask(lens, t)[:, :, 0]
    assert bool((y[padded] == bias).all()), "padded rows give the bias alone"
    assert bool((dx[padded] == 0).all()), "padded rows give dx = 0 exactly"
    xa, wa, ba = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    yo = C.conv_out(xa, wa, ba, lens=lens)
    yo.backward(dy)
    assert torch.equal(yo.detach(), y) and torch.equal(xa.grad, dx) and torch.equal(wa.grad, dw) and torch.equal(ba.grad, db)


@pytest.mark.parametrize("dtype,c", [(F32, c) for c in E.CONV_OUT_WIDTHS["f32"]] + [(BF, c) for c in E.CONV_OUT_WIDTHS["bf16"]])
def test_conv_out_forward_and_backward(dtype, c):
    for b, t in E.edge_rows(4):
        check_conv_out(c, b, t, dtype)


def test_conv_out_backward_split_across_an_item_boundary():
    """600000 rows on 1024 workgroups of 586 rows: workgroup 511 holds the last rows of item 0 and the first of item 1."""
    check_conv_out(8, 2, 300000, BF)


# ------------------------------------------------------------------------------------------------ gate_mix
def raw_gate_mix(z, dg, depth, w, g_out, dz_out):
    """The C entries on [rows, *] views whose rows may be pitched."""
    rows = z.shape[0]
    _call("smt_gate_mix_fwd", _p(z), _p(g_out), _dt(z.dtype), rows, w, depth, z.stride(0), g_out.stride(0))
    _call("smt_gate_mix_bwd", _p(z), _p(dg), _p(dz_out), _dt(z.dtype), rows, w, depth, z.stride(0), dg.stride(0), dz_out.stride(0))


def gate_mix_case(w, depth, rows, scale, dtype):
    g = gen(w, depth, rows)
    z = (scale * torch.randn(rows, depth * 2 * w, device=DEV, generator=g)).to(dtype)
    dg = torch.randn(rows, w, device=DEV, generator=g).to(dtype)
    return z, dg


def check_gate_mix(tag, g, dz, z, dg, depth):
    """Print the figure GATE_MIX_K is measured by, then hold the results against the bound."""
    assert finite(g, dz), tag + ": not finite"
    ref = E.gate_mix_ref(z, depth, dg)
    k = max(E.gate_mix_measure(g, ref["g"], ref["g_form"], z.dtype), E.gate_mix_measure(dz, ref["dz"], ref["dz_form"], z.dtype))
    print(f"  {tag}: GATE_MIX_K measure {'bf16' if z.dtype == BF else 'f32'} = {k:.3f}")
    E.check(tag, g, ref["g"], E.gate_mix_bound(ref["g"], ref["g_form"], z.dtype))
    E.check(tag + " dz", dz, ref["dz"], E.gate_mix_bound(ref["dz"], ref["dz_form"], z.dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", E.GATE_MIX_SCALES)
@pytest.mark.parametrize("w,depth", E.GATE_MIX_GEOMS)
def test_gate_mix_forward_and_backward(w, depth, scale, dtype):
    """2 randn; 1e-3 randn, the cancellation range of gate_tanh; 30 randn, saturated tanh and a one-hot softmax (nothing may
    become NaN).  40000 rows: at bf16 (64, 4) more than one trip of the shuffle kernel, the last one part dead."""
    from smt_amd import convops as C
    for rows in E.GATE_MIX_ROWS:
        z, dg = gate_mix_case(w, depth, rows, scale, dtype)
        g = torch.full((rows, w), NAN, dtype=dtype, device=DEV)
        dz = torch.full_like(z, NAN)
        raw_gate_mix(z, dg, depth, w, g, dz)
        check_gate_mix(f"gate_mix w={w} d={depth} rows={rows} x{scale}", g, dz, z, dg, depth)
        if rows == 157:                                  # the autograd op runs the same launches
            za = z.view(1, rows, -1).clone().requires_grad_(True)
            go = C.gate_mix(za, depth)
            go.backward(dg.view(1, rows, w))
            assert torch.equal(go.detach()[0], g) and torch.equal(za.grad[0], dz)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w,depth", [(64, 4), (32, 3), (128, 4)])
def test_gate_mix_on_pitched_operands(w, depth, dtype):
    """z, dz and g as column slices of wider NaN-filled tensors: the columns outside the slices still hold NaN afterwards."""
    rows, n = 157, depth * 2 * w
    z, dg = gate_mix_case(w, depth, rows, 2.0, dtype)
    zw = torch.full((rows, n + 24), NAN, dtype=dtype, device=DEV)
    dzw = torch.full((rows, n + 40), NAN, dtype=dtype, device=DEV)
    gw = torch.full((rows, w + 16), NAN, dtype=dtype, device=DEV)
    dgw = torch.full((rows, w + 32), NAN, dtype=dtype, device=DEV)
    zw[:, 8:8 + n] = z
    dgw[:, 24:24 + w] = dg
    raw_gate_mix(zw[:, 8:8 + n], dgw[:, 24:24 + w], depth, w, gw[:, 8:8 + w], dzw[:, 16:16 + n])
    check_gate_mix(f"gate_mix pitched w={w} d={depth}", gw[:, 8:8 + w], dzw[:, 16:16 + n], z, dg, depth)
    for wide, lo, width in ((gw, 8, w), (dzw, 16, n), (zw, 8, n), (dgw, 24, w)):
        assert bool(torch.isnan(wide[:, :lo]).all()) and bool(torch.isnan(wide[:, lo + width:]).all())
    gd = torch.full((rows, w), NAN, dtype=dtype, device=DEV)
    dzd = torch.full_like(z, NAN)
    raw_gate_mix(z, dg, depth, w, gd, dzd)
    assert torch.equal(gd, gw[:, 8:8 + w]) and torch.equal(dzd, dzw[:, 16:16 + n])


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_are_reported_by_message_before_any_launch():
    x, w, bias, dy, lens = conv_in_case(4, 2, 1, 8, 1, 64, F32)
    t_out = dy.shape[1]
    y = torch.full((1, t_out, 8), NAN, device=DEV)
    with pytest.raises(RuntimeError, match="smt_conv_in_fwd: null pointer"):
        _call("smt_conv_in_fwd", _p(x), None, _p(bias), _p(lens), _p(y), _dt(F32), 1, 64, t_out, 8, 4, 2, 1)
    with pytest.raises(RuntimeError, match="smt_conv_in_fwd: bad geometry"):
        _call("smt_conv_in_fwd", _p(x), _p(w), _p(bias), _p(lens), _p(y), _dt(F32), 1, 64, t_out, 8, 9, 2, 1)
    assert bool(torch.isnan(y).all())
    with pytest.raises(RuntimeError, match="smt_conv_in_wgrad: null pointer"):
        _call("smt_conv_in_wgrad", _p(x), _p(dy), _p(lens), None, _p(bias), _dt(F32), 1, 64, t_out, 8, 4, 2, 1, _p(y), 1 << 20)
    dy128 = torch.zeros(1, t_out, 128, device=DEV)
    with pytest.raises(RuntimeError, match="smt_conv_in_wgrad: c_out must be a power-of-two multiple of the vector width, <= 64"):
        _call("smt_conv_in_wgrad", _p(x), _p(dy128), _p(lens), _p(y), _p(bias), _dt(F32), 1, 64, t_out, 128, 4, 2, 1, _p(y), 1 << 20)
    with pytest.raises(RuntimeError, match="smt_conv_in_wgrad: workspace too small"):
        raw_conv_in_wgrad(x, dy, lens, 4, 2, 1, short=1)
    xo, wo, bo, dyo, lens_o = conv_out_case(8, 1, 64, F32)
    yo = torch.full((1, 64), NAN, device=DEV)
    with pytest.raises(RuntimeError, match="smt_conv_out_fwd: null pointer"):
        _call("smt_conv_out_fwd", _p(xo), _p(wo), None, _p(lens_o), _p(yo), _dt(F32), 1, 64, 8)
    for bad in (24, 6, 512):                             # not a power of two of vectors, no multiple of the vector, 128 lanes per row
        with pytest.raises(RuntimeError, match=f"smt_conv_out_fwd: bad c_in={bad}"):
            _call("smt_conv_out_fwd", _p(xo), _p(wo), _p(bo), _p(lens_o), _p(yo), _dt(F32), 1, 64, bad)
        with pytest.raises(RuntimeError, match=f"smt_conv_out_bwd: bad c_in={bad}"):
            _call("smt_conv_out_bwd", _p(xo), _p(wo), _p(lens_o), _p(dyo), _p(xo), _p(wo), _p(bo), _dt(F32), 1, 64, bad, _p(yo), 1 << 20)
    assert bool(torch.isnan(yo).all())
    with pytest.raises(RuntimeError, match="smt_conv_out_bwd: null pointer"):
        _call("smt_conv_out_bwd", _p(xo), _p(wo), _p(lens_o), _p(dyo), _p(xo), _p(wo), _p(bo), _dt(F32), 1, 64, 8, None, 1 << 20)
    with pytest.raises(RuntimeError, match="smt_conv_out_bwd: workspace too small"):
        raw_conv_out(xo, wo, bo, lens_o, dyo, short=1)
    z, dg = gate_mix_case(8, 2, 4, 2.0, F32)
    with pytest.raises(RuntimeError, match="smt_gate_mix_fwd: null pointer"):
        _call("smt_gate_mix_fwd", _p(z), None, _dt(F32), 4, 8, 2, 32, 8)
    with pytest.raises(RuntimeError, match="smt_gate_mix_bwd: null pointer"):
        _call("smt_gate_mix_bwd", _p(z), _p(dg), None, _dt(F32), 4, 8, 2, 32, 8, 32)
    with pytest.raises(RuntimeError, match="smt_gate_mix_bwd: bad geometry"):
        _call("smt_gate_mix_bwd", _p(z), _p(dg), _p(z), _dt(F32), 4, 8, 9, 32, 8, 32)
