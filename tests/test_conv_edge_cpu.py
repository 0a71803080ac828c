"""tests/conv_edge_helpers.py without a GPU: (1) every float64 reference equals the matching torch functional and its autograd in
float64, on random and on ragged inputs; (2) an fp32 emulation of each kernel's arithmetic (fp32 torch ops on the rounded operands,
then the stated roundings) stays inside the bound at the shapes of tests/test_conv_misc_float64_gpu.py and
tests/test_conv_resample_float64_gpu.py -- the check that the reference alone satisfies the cap; (3) the bounds have teeth: a
dropped tap, swapped phases, lens off by one row, a dropped 8-channel vector, a dropped bias, permuted gate_mix branches and a
truncating bf16 store each exceed SLACK times the bound."""
import pytest
import torch
import torch.nn.functional as F

import conv_edge_helpers as E

BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]


def gen(*key):
    return torch.Generator().manual_seed(1 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def mask(lens, t):
    return E.row_mask(lens, t).double()


def same(a, b):
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    assert a.shape == b.shape and float((a - b).abs().max() if b.numel() else 0.0) <= 1e-12 * scale


# ------------------------------------------------------------------------------------------------ (1) pins
@pytest.mark.parametrize("b,t_in,c_in,c_out,ragged", [(2, 8, 8, 16, False), (4, 258, 16, 8, True), (3, 3, 8, 8, True),
                                                      (3, 255, 8, 8, True), (4, 2, 8, 8, True)])
def test_strided_reference_is_conv1d_in_float64(b, t_in, c_in, c_out, ragged):
    g = gen(b, t_in, c_in)
    x = torch.randn(b, t_in, c_in, generator=g, dtype=torch.float64)
    w = torch.randn(c_out, c_in, 4, generator=g, dtype=torch.float64).requires_grad_(True)
    bias = torch.randn(c_out, generator=g, dtype=torch.float64).requires_grad_(True)
    lens = E.edge_lens(b, t_in) if ragged else None
    xm = x if lens is None else x * mask(lens, t_in)
    want = F.conv1d(xm.transpose(1, 2), w, bias, stride=2, padding=1).transpose(1, 2)
    got, bound = E.strided_conv_ref(x, w.detach(), bias.detach(), lens)
    same(got, want.detach())
    assert bool((bound > 0).all())
    dy = torch.randn(want.shape, generator=g, dtype=torch.float64)
    want.backward(dy)
    dw, _, db, _ = E.strided_wgrad_ref(x, dy, lens)
    same(dw, w.grad)
    same(db, bias.grad)
    lens_out = E.edge_lens(b, want.shape[1])
    got_m, bound_m = E.strided_conv_ref(x, w.detach(), bias.detach(), lens, lens_out)
    same(got_m, want.detach() * mask(lens_out, want.shape[1]))
    assert float(bound_m[b - 1, int(lens_out[b - 1]):].abs().sum()) == 0.0


@pytest.mark.parametrize("b,t_in,c_in,c_out,ragged", [(2, 8, 8, 16, False), (4, 129, 8, 16, True), (4, 1, 8, 8, True), (3, 2, 16, 8, True)])
def test_transposed_reference_is_conv_transpose1d_in_float64(b, t_in, c_in, c_out, ragged):
    g = gen(b, t_in, c_in, 5)
    x = torch.randn(b, t_in, c_in, generator=g, dtype=torch.float64)
    w = torch.randn(c_in, c_out, 4, generator=g, dtype=torch.float64).requires_grad_(True)
    bias = torch.randn(c_out, generator=g, dtype=torch.float64).requires_grad_(True)
    lens = E.edge_lens(b, t_in) if ragged else None
    xm = x if lens is None else x * mask(lens, t_in)
    want = F.conv_transpose1d(xm.transpose(1, 2), w, bias, stride=2, padding=1).transpose(1, 2)
    got, _ = E.transposed_conv_ref(x, w.detach(), bias.detach(), lens)
    same(got, want.detach())
    dy = torch.randn(want.shape, generator=g, dtype=torch.float64)
    want.backward(dy)
    dw, _, db, _ = E.transposed_wgrad_ref(x, dy, lens)
    same(dw, w.grad)
    same(db, bias.grad)
    lens_out = E.edge_lens(b, 2 * t_in)
    got_m, _ = E.transposed_conv_ref(x, w.detach(), bias.detach(), lens, lens_out)
    same(got_m, want.detach() * mask(lens_out, 2 * t_in))


def test_the_data_gradient_of_each_resampling_conv_is_the_other_one():
    """What the streaming kernels are used for: dx of the strided conv is the transposed reference on dy with the same weight
    tensor read in ConvTranspose1d layout and lens as lens_out, and the reverse."""
    g = gen(11)
    b, t = 4, 9
    lens2, lens1 = E.edge_lens(b, 2 * t), E.edge_lens(b, t)
    w = torch.randn(8, 16, 4, generator=g, dtype=torch.float64)
    x = torch.randn(b, 2 * t, 16, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv1d((x * mask(lens2, 2 * t)).transpose(1, 2), w, None, stride=2, padding=1).transpose(1, 2)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    same(E.transposed_conv_ref(dy, w, None, None, lens2)[0], x.grad)
    xt = torch.randn(b, t, 8, generator=g, dtype=torch.float64, requires_grad=True)
    yt = F.conv_transpose1d((xt * mask(lens1, t)).transpose(1, 2), w, None, stride=2, padding=1).transpose(1, 2)
    dyt = torch.randn(yt.shape, generator=g, dtype=torch.float64)
    yt.backward(dyt)
    same(E.strided_conv_ref(dyt, w, None, None, lens1)[0], xt.grad)


@pytest.mark.parametrize("taps,stride,pad", E.CONV_IN_GEOMS)
@pytest.mark.parametrize("b,t_in", [(1, 8), (3, 50), (4, 66)])
def test_conv_in_reference_is_conv1d_in_float64(taps, stride, pad, b, t_in):
    g = gen(taps, b, t_in)
    x = torch.randn(b, t_in, generator=g, dtype=torch.float64)
    w = torch.randn(8, 1, taps, generator=g, dtype=torch.float64).requires_grad_(True)
    bias = torch.randn(8, generator=g, dtype=torch.float64).requires_grad_(True)
    lens = E.edge_lens(b, t_in)
    want = F.conv1d((x * mask(lens, t_in)[:, :, 0])[:, None], w, bias, stride=stride, padding=pad).transpose(1, 2)
    got, _ = E.conv_in_ref(x, w.detach(), bias.detach(), lens, stride, pad, False)
    same(got, want.detach())
    dy = torch.randn(want.shape, generator=g, dtype=torch.float64)
    want.backward(dy)
    dw, _, db, _ = E.conv_in_wgrad_ref(x, dy, lens, taps, stride, pad)
    same(dw, w.grad)
    same(db, bias.grad)


def test_conv_in_reference_of_an_input_shorter_than_the_kernel_is_empty():
    x, w, bias = torch.randn(1, 2), torch.randn(8, 1, 8), torch.randn(8)
    y, bound = E.conv_in_ref(x, w, bias, None, 4, 2, False)
    assert y.shape == bound.shape == (1, 0, 8)
    dw, _, db, _ = E.conv_in_wgrad_ref(x, torch.zeros(1, 0, 8), None, 8, 4, 2)
    assert dw.shape == (8, 1, 8) and float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0


@pytest.mark.parametrize("b,t,c", [(1, 2, 8), (3, 50, 16), (4, 66, 64)])
def test_conv_out_reference_is_conv1d_in_float64(b, t, c):
    g = gen(b, t, c, 3)
    x = torch.randn(b, t, c, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(1, c, 1, generator=g, dtype=torch.float64).requires_grad_(True)
    bias = torch.randn(1, generator=g, dtype=torch.float64).requires_grad_(True)
    lens = E.edge_lens(b, t)
    want = F.conv1d((x * mask(lens, t)).transpose(1, 2), w, bias)[:, 0]
    got, _ = E.conv_out_ref(x.detach(), w.detach(), bias.detach(), lens)
    same(got, want.detach())
    dy = torch.randn(want.shape, generator=g, dtype=torch.float64)
    want.backward(dy)
    dx, dx_b, dw, _, db, _ = E.conv_out_bwd_ref(x.detach(), w.detach(), dy, lens, False)
    same(dx, x.grad)
    same(dw, w.grad)
    same(db, bias.grad)
    pad_rows = mask(lens, t)[:, :, 0] == 0
    assert bool((got[pad_rows] == bias.detach()).all()) and float(dx_b[pad_rows].abs().max() if pad_rows.any() else 0.0) == 0.0


@pytest.mark.parametrize("w,depth", [(8, 1), (8, 3), (16, 4), (8, 8)])
@pytest.mark.parametrize("scale", E.GATE_MIX_SCALES)
def test_gate_mix_reference_is_tanh_times_softmax_in_float64(w, depth, scale):
    g = gen(w, depth)
    rows = 13
    z = (scale * torch.randn(rows, depth * 2 * w, generator=g, dtype=torch.float64)).requires_grad_(True)
    zz = z.view(rows, depth, 2, w)
    want = (torch.tanh(zz[:, :, 0]) * torch.softmax(zz[:, :, 1], dim=1)).sum(1)
    dg = torch.randn(rows, w, generator=g, dtype=torch.float64)
    want.backward(dg)
    ref = E.gate_mix_ref(z.detach(), depth, dg)
    same(ref["g"], want.detach())
    same(ref["dz"], z.grad)
    assert bool((ref["g_form"] > 0).all()) and bool((ref["dz_form"] > 0).all())
    assert bool(torch.isfinite(ref["g"]).all()) and bool(torch.isfinite(ref["dz"]).all())


# ------------------------------------------------------------------------------------------------ (2) emulations, (3) teeth
def resample_case(kind, c_wide, t, b=4, dtype=BF):
    """Operands of one resampling layer: 'conv' x [b, 2t, c_wide] -> [b, t, 64]; 'convt' x [b, t, 64] -> [b, 2t, c_wide]."""
    g = gen(c_wide, t, b, kind == "conv")
    t_in, c_in = (2 * t, c_wide) if kind == "conv" else (t, 64)
    x = torch.randn(b, t_in, c_in, generator=g).to(dtype)
    w = (torch.randn(64, c_wide, 4, generator=g) / (2 * c_in) ** 0.5).to(dtype)
    bias = torch.randn(64 if kind == "conv" else c_wide, generator=g)
    return x, w, bias


def resample_uses(kind, b, t):
    """(lens_in, lens_out) of the forward use, the data-gradient use and the both-set use, at every length of the case."""
    t_in, t_out = (2 * t, t) if kind == "conv" else (t, 2 * t)
    big_in, big_out = ([255, 256, 257], [127, 128, 129]) if kind == "conv" else ([127, 128, 129], [255, 256, 257])
    uses = []
    for li in E.resample_lens(t_in, big_in):
        uses.append((torch.tensor([li, li - 1, 1, 0][:b], dtype=torch.int32), None))
    for lo in E.resample_lens(t_out, big_out):
        uses.append((None, torch.tensor([lo, lo - 1, 1, 0][:b], dtype=torch.int32)))
    uses.append((uses[0][0], uses[len(uses) // 2][1]))
    return uses


RS = {"conv": (E.strided_conv_ref, E.emulate_strided), "convt": (E.transposed_conv_ref, E.emulate_transposed)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c_wide", [64, 128])
@pytest.mark.parametrize("t", E.RESAMPLE_T)
@pytest.mark.parametrize("kind", ["conv", "convt"])
def test_resampling_emulation_stays_inside_the_bound(kind, t, c_wide, dtype):
    ref_fn, emu_fn = RS[kind]
    x, w, bias = resample_case(kind, c_wide, t, dtype=dtype)
    for lens_in, lens_out in resample_uses(kind, 4, t):
        bs = bias if lens_in is not None else None
        ref, bound = ref_fn(x, w, bs, lens_in, lens_out, rounded=dtype == BF)
        E.check(f"{kind} t={t} c={c_wide}", emu_fn(x, w, bs, lens_in, lens_out, dtype), ref, bound)


@pytest.mark.parametrize("kind", ["conv", "convt"])
def test_resampling_emulation_stays_inside_the_bound_on_two_tiles_per_workgroup(kind):
    ref_fn, emu_fn = RS[kind]
    x, w, bias = resample_case(kind, 128, 11100, b=3)
    lens = torch.tensor([x.shape[1], x.shape[1] - 1, 1], dtype=torch.int32)
    ref, bound = ref_fn(x, w, bias, lens, None)
    E.check(f"{kind} t=11100", emu_fn(x, w, bias, lens, None, BF), ref, bound)


@pytest.mark.parametrize("t", E.RESAMPLE_WGRAD_T)
def test_resampling_weight_gradient_emulation_stays_inside_the_bound(t):
    for kind, ref_fn in (("conv", E.strided_wgrad_ref), ("convt", E.transposed_wgrad_ref)):
        x, _, _ = resample_case(kind, 64, t)
        g = gen(t, 17)
        dy = torch.randn(4, t if kind == "conv" else 2 * t, 64, generator=g).to(BF)
        lens = E.edge_lens(4, x.shape[1])
        dw, dw_b, db, db_b = ref_fn(x, dy, lens)
        dw32, _, db32, _ = ref_fn(x.float(), dy.float(), lens)         # the same sums; rounded to fp32 below
        E.check(f"{kind} dW t={t}", dw32.float(), dw, dw_b)
        E.check(f"{kind} db t={t}", db32.float(), db, db_b)


RS_MUTATIONS = {"conv": ["tap", "lens", "vector", "bias", "truncate"], "convt": ["tap", "phases", "lens", "vector", "bias", "truncate"]}


@pytest.mark.parametrize("kind,drop", [(k, d) for k, ds in RS_MUTATIONS.items() for d in ds])
def test_resampling_bound_has_teeth(kind, drop):
    ref_fn, emu_fn = RS[kind]
    x, w, bias = resample_case(kind, 64, 129)
    lens_in = E.edge_lens(4, x.shape[1])
    ref, bound = ref_fn(x, w, bias, lens_in, None)
    assert E.worst(emu_fn(x, w, bias, lens_in, None, BF), ref, bound) <= E.SLACK
    assert E.worst(emu_fn(x, w, bias, lens_in, None, BF, drop=drop), ref, bound) > E.SLACK
    if drop == "lens":                                                   # the output mask off by one row as well
        lens_out = E.edge_lens(4, ref.shape[1])
        ref, bound = ref_fn(x, w, None, None, lens_out)
        assert E.worst(emu_fn(x, w, None, None, lens_out, BF, drop=drop), ref, bound) > E.SLACK


def conv_in_case(taps, stride, pad, c, b, t_in):
    g = gen(taps, c, b, t_in)
    x = torch.rand(b, t_in, generator=g) * 2 - 1
    w = torch.randn(c, 1, taps, generator=g) * 0.5
    bias = torch.randn(c, generator=g)
    dy = torch.randn(b, E.conv_in_t_out(t_in, taps, stride, pad), c, generator=g)
    return x, w, bias, dy


def conv_in_emulated(taps, stride, pad, c, b, t_in, dtype):
    x, w, bias, dy = conv_in_case(taps, stride, pad, c, b, t_in)
    lens = E.edge_lens(b, t_in)
    tag = f"conv_in k{taps}s{stride} c={c} ({b}, {t_in})"
    E.check(tag, E.emulate_conv_in(x, w, bias, lens, stride, pad, dtype), *E.conv_in_ref(x, w, bias, lens, stride, pad, dtype == BF))
    dyr = dy.to(dtype)
    dw, dw_b, db, db_b = E.conv_in_wgrad_ref(x, dyr, lens, taps, stride, pad)
    xs = E._conv_in_rows(x, lens, taps, stride, pad, dy.shape[1])
    dw32 = torch.stack([torch.einsum("bto,bt->o", dyr.float(), r.float()) for r in xs], dim=1)[:, None, :]
    E.check(tag + " dW", dw32, dw, dw_b)
    E.check(tag + " db", dyr.float().sum((0, 1)), db, db_b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", E.CONV_IN_WIDTHS)
@pytest.mark.parametrize("taps,stride,pad", E.CONV_IN_GEOMS)
def test_conv_in_emulation_stays_inside_the_bound(taps, stride, pad, c, dtype):
    for b, t_in in E.edge_rows(taps):
        conv_in_emulated(taps, stride, pad, c, b, t_in, dtype)


def test_conv_in_emulation_stays_inside_the_bound_at_the_wide_and_long_cases():
    x, w, bias, _ = conv_in_case(4, 2, 1, 512, 3, 1000)
    lens = E.edge_lens(3, 1000)
    E.check("conv_in c=512", E.emulate_conv_in(x, w, bias, lens, 2, 1, F32), *E.conv_in_ref(x, w, bias, lens, 2, 1, False))
    conv_in_emulated(4, 2, 1, 64, 2, 80000, F32)                        # t_out = 40000: the grid wraps
    conv_in_emulated(4, 2, 1, 8, 1, 2 * 524289, BF)                     # t_out = 524289: the split weight gradient


@pytest.mark.parametrize("drop", ["tap", "lens", "bias", "truncate"])
def test_conv_in_bound_has_teeth(drop):
    x, w, bias, _ = conv_in_case(4, 2, 1, 32, 4, 66)
    lens = E.edge_lens(4, 66)
    ref, bound = E.conv_in_ref(x, w, bias, lens, 2, 1, True)
    assert E.worst(E.emulate_conv_in(x, w, bias, lens, 2, 1, BF), ref, bound) <= E.SLACK
    assert E.worst(E.emulate_conv_in(x, w, bias, lens, 2, 1, BF, drop=drop), ref, bound) > E.SLACK


def conv_out_case(c, b, t, dtype):
    g = gen(c, b, t, 9)
    x = torch.randn(b, t, c, generator=g).to(dtype)
    w = torch.randn(1, c, 1, generator=g) * 0.1
    bias = torch.randn(1, generator=g)
    dy = torch.randn(b, t, generator=g)
    return x, w, bias, dy


def conv_out_emulated(c, b, t, dtype):
    x, w, bias, dy = conv_out_case(c, b, t, dtype)
    lens = E.edge_lens(b, t)
    tag = f"conv_out c={c} ({b}, {t})"
    E.check(tag, E.emulate_conv_out(x, w, bias, lens), *E.conv_out_ref(x, w, bias, lens))
    dx, dx_b, dw, dw_b, db, db_b = E.conv_out_bwd_ref(x, w, dy, lens, dtype == BF)
    E.check(tag + " dx", E.emulate_conv_out_dx(x, w, dy, lens), dx, dx_b)
    xm = x.float() * E.row_mask(lens, t)
    E.check(tag + " dw", torch.einsum("bt,btc->c", dy, xm).reshape(1, c, 1), dw, dw_b)
    E.check(tag + " db", dy.sum().reshape(1), db, db_b)


@pytest.mark.parametrize("dtype,c", [(F32, c) for c in E.CONV_OUT_WIDTHS["f32"]] + [(BF, c) for c in E.CONV_OUT_WIDTHS["bf16"]])
def test_conv_out_emulation_stays_inside_the_bound(dtype, c):
    for b, t in E.edge_rows(4):
        conv_out_emulated(c, b, t, dtype)


def test_conv_out_emulation_stays_inside_the_bound_at_the_split_case():
    conv_out_emulated(8, 2, 300000, BF)


@pytest.mark.parametrize("drop", ["lens", "vector", "bias", "truncate"])
def test_conv_out_bound_has_teeth(drop):
    x, w, bias, dy = conv_out_case(128, 4, 66, BF)
    lens = E.edge_lens(4, 66)
    if drop != "truncate":
        ref, bound = E.conv_out_ref(x, w, bias, lens)
        assert E.worst(E.emulate_conv_out(x, w, bias, lens), ref, bound) <= E.SLACK
        assert E.worst(E.emulate_conv_out(x, w, bias, lens, drop=drop), ref, bound) > E.SLACK
    if drop != "bias":
        dx, dx_b = E.conv_out_bwd_ref(x, w, dy, lens, True)[:2]
        assert E.worst(E.emulate_conv_out_dx(x, w, dy, lens), dx, dx_b) <= E.SLACK
        assert E.worst(E.emulate_conv_out_dx(x, w, dy, lens, drop=drop), dx, dx_b) > E.SLACK


def gate_mix_case(w, depth, rows, scale, dtype):
    g = gen(w, depth, rows)
    z = (scale * torch.randn(rows, depth * 2 * w, generator=g)).to(dtype)
    dg = torch.randn(rows, w, generator=g).to(dtype)
    return z, dg


def gate_mix_emulated(w, depth, rows, scale, dtype):
    z, dg = gate_mix_case(w, depth, rows, scale, dtype)
    ref = E.gate_mix_ref(z, depth, dg)
    g, dz = E.emulate_gate_mix(z, depth, dg)
    assert bool(torch.isfinite(g.float()).all()) and bool(torch.isfinite(dz.float()).all())
    tag = f"gate_mix w={w} d={depth} rows={rows} x{scale}"
    E.check(tag, g, ref["g"], E.gate_mix_bound(ref["g"], ref["g_form"], dtype))
    E.check(tag + " dz", dz, ref["dz"], E.gate_mix_bound(ref["dz"], ref["dz_form"], dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", E.GATE_MIX_SCALES)
@pytest.mark.parametrize("w,depth", E.GATE_MIX_GEOMS)
def test_gate_mix_emulation_stays_inside_the_bound(w, depth, scale, dtype):
    """Rows do not enter the arithmetic of an element; the 40000-row case runs once, at the geometry whose kernel it is about."""
    for rows in [r for r in E.GATE_MIX_ROWS if r < 40000 or (w, depth, dtype) == (64, 4, BF)]:
        gate_mix_emulated(w, depth, rows, scale, dtype)


@pytest.mark.parametrize("drop", ["branches", "truncate"])
def test_gate_mix_bound_has_teeth(drop):
    z, dg = gate_mix_case(64, 4, 157, 2.0, BF)
    ref = E.gate_mix_ref(z, 4, dg)
    g, dz = E.emulate_gate_mix(z, 4, dg, drop=drop)
    assert E.worst(g, ref["g"], E.gate_mix_bound(ref["g"], ref["g_form"], BF)) > E.SLACK
    assert E.worst(dz, ref["dz"], E.gate_mix_bound(ref["dz"], ref["dz_form"], BF)) > E.SLACK
