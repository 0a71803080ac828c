"""The k = 4 / stride 2 / padding 1 resampling convs against the float64 references and derived bounds of
tests/conv_edge_helpers.py: the streaming kernels smt_conv4s2 / smt_convt4s2 (csrc/conv_resample.hip) through
convops._resample and the C entries, and the generic kernel's stride-2 and phase-split launches (csrc/conv.hip) through the
autograd ops, in fp32 and -- with convops._RESAMPLE off -- in bf16.  Where both kernels run, their results are bit-identical (the
existing contract) AND each is inside the float64 bound, so a mistake the two share, or a rewrite that changes the summation
order, is still caught.

One layer gives both uses of both kernels: the forward of the strided conv is smt_conv4s2 with lens_in, its data gradient is
smt_convt4s2 on dy with lens_out and the same weight tensor read in ConvTranspose1d layout; the transposed conv is the reverse
(tests/test_conv_edge_cpu.py pins that identity).  Lengths: one output row, a single partial tile, the 128-row tile edge from
both sides, three tiles, and masked lengths inside the two-row halo and the first DMA piece of the second tile; items of length
1 and 0.  bf16 operands of the streaming kernels are channel slices of wider NaN-filled tensors, y a NaN-filled slice of a
NaN-filled wider tensor: nothing outside the slice may be written and no NaN may be read."""
import ctypes

import pytest
import torch

import conv_edge_helpers as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
BF, F32 = torch.bfloat16, torch.float32
BIG_IN = {"conv": [255, 256, 257], "convt": [127, 128, 129]}       # masked input lengths at the halo / first piece of tile two
REF = {"conv": E.strided_conv_ref, "convt": E.transposed_conv_ref}
WREF = {"conv": E.strided_wgrad_ref, "convt": E.transposed_wgrad_ref}
OTHER = {"conv": "convt", "convt": "conv"}


def gen(*key):
    return torch.Generator(device=DEV).manual_seed(1 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def lens_of(length, b):
    return torch.tensor([length, length - 1, 1, 0][:b], dtype=torch.int32, device=DEV)


def in_slice(t, lo=8, extra=16):
    """t as a channel slice of a wider NaN-filled tensor."""
    wide = torch.full(t.shape[:2] + (t.shape[2] + extra,), NAN, dtype=t.dtype, device=DEV)
    wide[:, :, lo:lo + t.shape[2]] = t
    return wide[:, :, lo:lo + t.shape[2]]


def pack(kind, w):
    """The weight tensor w [64, c_wide, 4] as the operand of the kernel: Conv1d layout [C_out, C_in, k] for 'conv',
    ConvTranspose1d layout [C_in, C_out, k] for 'convt' (as _Conv1d / _ConvTranspose1d pack them, forward and data gradient)."""
    from smt_amd import convops as C
    c_wide = w.shape[1]
    return C._pack_fwd(w, BF) if kind == "conv" else C._pack(w, BF, c_wide, 64, 4, c_wide * 4, 1, list(range(4)))


def run_stream(kind, x, w, bias, lens_in, lens_out, raw=False):
    """One streaming launch on sliced operands; returns y (a view into its wider tensor) after checking the surroundings."""
    from smt_amd import convops as C
    from smt_amd import native as N
    b, t_in, _ = x.shape
    c_wide = w.shape[1]
    t_y, c_y = (t_in // 2, 64) if kind == "conv" else (2 * t_in, c_wide)
    y_wide = torch.full((b, t_y, c_y + 24), NAN, dtype=BF, device=DEV)
    y = y_wide[:, :, 16:16 + c_y]
    xs, wp = in_slice(x), pack(kind, w)
    if raw:
        fn = N.lib().smt_conv4s2 if kind == "conv" else N.lib().smt_convt4s2
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
        N.check(fn(p(xs), xs.stride(0), xs.stride(1), p(wp), p(bias), p(y), y.stride(0), y.stride(1), p(lens_in), p(lens_out), b, t_in,
                   c_wide, p(C._zero_page(x.device)), N.stream_ptr()), "smt_conv4s2" if kind == "conv" else "smt_convt4s2")
    else:
        C._resample(kind, "fwd" if lens_out is None else "dgrad", xs, wp, bias, y, lens_in, lens_out, c_wide)
    assert bool(torch.isnan(y_wide[:, :, :16]).all()) and bool(torch.isnan(y_wide[:, :, 16 + c_y:]).all()), "written outside the slice"
    return y


def run_layer(kind, x, w, bias, lens, dy, resample, streams=None):
    """(y, dx, dW, db) of the autograd op with the streaming kernels on or off; which kernels ran is asserted (`streams`:
    whether the streaming kernels are expected, by default whenever they are on)."""
    from smt_amd import convops as C
    from smt_amd import profiler
    xa, wa, ba = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    C._RESAMPLE = resample
    try:
        profiler.reset(); profiler.enable(True)
        if kind == "conv":
            y = C.conv1d(xa, wa, ba, stride=2, padding=1, lens=lens)
        else:
            y = C.conv_transpose1d(xa, wa, ba, stride=2, padding=1, lens=lens)
        y.backward(dy)
        names = {r["name"] for r in profiler.summary()}
    finally:
        profiler.enable(False); profiler.reset()
        C._RESAMPLE = True
    streamed = {n for n in names if n.startswith(("conv4s2:", "convt4s2:"))}
    want = {f"{'conv4s2' if kind == 'conv' else 'convt4s2'}:fwd", f"{'convt4s2' if kind == 'conv' else 'conv4s2'}:dgrad"}
    assert streamed == (want if (resample if streams is None else streams) else set()), sorted(names)
    return y.detach(), xa.grad, wa.grad, ba.grad


def layer_case(kind, c_wide, t, b, c_narrow=64):
    """fp32 masters of one layer: 'conv' x [b, 2t, c_wide] -> [b, t, c_narrow]; 'convt' x [b, t, c_narrow] -> [b, 2t, c_wide].
    w is [c_narrow, c_wide, 4] in both."""
    g = gen(c_wide, t, b, kind == "conv")
    t_in, c_in = (2 * t, c_wide) if kind == "conv" else (t, c_narrow)
    t_y, c_y = (t, c_narrow) if kind == "conv" else (2 * t, c_wide)
    x = torch.randn(b, t_in, c_in, device=DEV, generator=g)
    w = torch.randn(c_narrow, c_wide, 4, device=DEV, generator=g) / (2 * c_in) ** 0.5
    bias = torch.randn(c_y, device=DEV, generator=g)
    dy = torch.randn(b, t_y, c_y, device=DEV, generator=g)
    return x, w, bias, dy


def dgrad_ref(kind, dy, w, lens, t_in, rounded):
    """dx of layer `kind` in float64: the other conv on dy, masked by lens; an odd t_in (strided conv only) has one more row
    than twice the output, which a zero row appended to dy supplies."""
    if kind == "conv" and t_in != 2 * dy.shape[1]:
        dy = torch.nn.functional.pad(dy, (0, 0, 0, 1))
    ref, bound = REF[OTHER[kind]](dy, w, None, None, lens, rounded=rounded)
    return ref[:, :t_in], bound[:, :t_in]


def check_layer(tag, kind, got, x, w, bias, lens, dy, dtype, wgrad):
    """y, dx (and dW, db) of one layer run against float64; x, w, dy are the fp32 masters."""
    y, dx, dw, db = got
    xr, wr, dyr = E.as_read(x, dtype), E.as_read(w, dtype), E.as_read(dy, dtype)
    E.check(f"{tag} y", y, *REF[kind](xr, wr, bias, lens, None, rounded=dtype == BF))
    E.check(f"{tag} dx", dx, *dgrad_ref(kind, dyr, wr, lens, x.shape[1], dtype == BF))
    if wgrad:
        dw_r, dw_b, db_r, db_b = WREF[kind](xr, dyr, lens)
        E.check(f"{tag} dW", dw, dw_r, dw_b)
        E.check(f"{tag} db", db, db_r, db_b)


def check_streamed_layer(kind, c_wide, t, b, wgrad):
    x, w, bias, dy = layer_case(kind, c_wide, t, b)
    xb, dyb = x.to(BF), dy.to(BF)
    t_in = x.shape[1]
    for length in E.resample_lens(t_in, BIG_IN[kind]):
        lens = lens_of(length, b)
        tag = f"{kind} c={c_wide} t={t} L={length}"
        y_s = run_stream(kind, xb, w, bias, lens, None)                              # the forward use: lens_in, bias
        dx_s = run_stream(OTHER[kind], dyb, w, None, None, lens)                     # the data-gradient use: lens_out, no bias
        generic = run_layer(kind, xb, w, bias, lens, dyb, resample=False)
        check_layer(tag + " generic bf16", kind, generic, x, w, bias, lens, dy, BF, wgrad)
        check_layer(tag + " stream", kind, (y_s, dx_s, None, None), x, w, bias, lens, dy, BF, False)
        assert torch.equal(y_s, generic[0]) and torch.equal(dx_s, generic[1]), tag + ": streaming and generic kernels differ"
        streamed = run_layer(kind, xb, w, bias, lens, dyb, resample=True)            # the op itself takes the streaming kernels
        assert all(torch.equal(a, c) for a, c in zip(streamed, generic)), tag + ": op differs with the streaming kernels on"
        check_layer(tag + " generic f32", kind, run_layer(kind, x, w, bias, lens, dy, True, streams=False), x, w, bias, lens, dy, F32,
                    wgrad)
    # both masks in one launch, through the C entry
    lens_in, lens_out = lens_of(t_in, b), lens_of(dy.shape[1], b)
    y_b = run_stream(kind, xb, w, bias, lens_in, lens_out, raw=True)
    E.check(f"{kind} c={c_wide} t={t} both lens", y_b, *REF[kind](E.as_read(x, BF), E.as_read(w, BF), bias, lens_in, lens_out))
    assert bool((y_b[~E.row_mask(lens_out, y_b.shape[1]).expand_as(y_b)] == 0).all()), "rows past lens_out are exact zeros"


@pytest.mark.parametrize("c_wide", [64, 128])
@pytest.mark.parametrize("t", E.RESAMPLE_T)
@pytest.mark.parametrize("kind", ["conv", "convt"])
def test_resampling_kernels_at_the_tile_edges(kind, t, c_wide):
    check_streamed_layer(kind, c_wide, t, 4, wgrad=t in E.RESAMPLE_WGRAD_T)


@pytest.mark.parametrize("c_wide", [64, 128])
@pytest.mark.parametrize("kind", ["conv", "convt"])
def test_resampling_kernels_with_two_tiles_of_two_items_in_one_workgroup(kind, c_wide):
    """b = 3, T = 11100: 87 tiles per item, 261 tiles on 256 workgroups; tiles 86 and 87 (the last of item 0, the first of
    item 1) share a workgroup's run."""
    check_streamed_layer(kind, c_wide, 11100, 3, wgrad=False)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("t_in", [3, 255])
def test_strided_conv_of_an_odd_length_on_the_generic_kernel(t_in, dtype):
    """Odd input lengths go to the generic kernel alone: stride-2 forward, phase-split data gradient of unequal phases."""
    b, c_wide = 4, 64
    x, w, bias, _ = layer_case("conv", c_wide, (t_in + 1) // 2, b)
    x = x[:, :t_in].contiguous()
    t_out = (t_in - 2) // 2 + 1
    dy = torch.randn(b, t_out, 64, device=DEV, generator=gen(t_in))
    lens = lens_of(t_in, b)
    got = run_layer("conv", x.to(dtype), w, bias, lens, dy.to(dtype), True, streams=False)
    assert got[0].shape == (b, t_out, 64) and got[1].shape == (b, t_in, c_wide)
    check_layer(f"conv odd t_in={t_in}", "conv", got, x, w, bias, lens, dy, dtype, True)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("t", E.RESAMPLE_WGRAD_T)
def test_phase_split_transposed_conv_at_16_to_32_channels(t, dtype):
    b = 4
    x, w, bias, dy = layer_case("convt", 32, t, b, c_narrow=16)
    lens = lens_of(t, b)
    got = run_layer("convt", x.to(dtype), w, bias, lens, dy.to(dtype), True, streams=False)
    assert got[0].shape == (b, 2 * t, 32)
    check_layer(f"convt 16->32 t={t}", "convt", got, x, w, bias, lens, dy, dtype, True)
