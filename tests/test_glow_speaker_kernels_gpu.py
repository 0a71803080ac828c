"""The speaker-conditioning kernels of GlowTTS (csrc/glow.hip: smt_glow_gate_cond_fwd / _bwd, smt_glow_bcast_concat,
smt_glow_item_colsum; smt_amd/glow.py: wn_gate_cond, gate_cond_backward, bcast_concat) one by one against float64 restatements
written here, with the tolerances and helpers of tests/test_glow_kernels_gpu.py.

The shapes straddle what the kernels tile by: the per-item reductions work in chunks of 64 rows (T = 63, 64, 65, 130: below,
at, past one chunk, and a third partial chunk) and tiles of 64 columns (H = 1, 3, 64, 192), a workgroup never spans two items
(B = 1, 2, 3 with ragged lens including 0 and T).  d cond is the quantity that was once written out of bounds (DESIGN.md
section 17: a dense [B, 2H] destination passed with the stride of cond's view): it is checked THROUGH AUTOGRAD from the grad of
the wider cond tensor after slicing, for B > 1, and once more through a directly strided destination; every destination that
the test allocates itself has guard elements behind it, and the other layers' slices hold a sentinel.

Tolerances: forward and da are a handful of fp32 operations per element (F32_TOL = 1e-5 of the tensor's max magnitude, as for
the unconditioned gate).  d cond and d g sum at most 130 rows per item here: about 130 roundings of 6e-8 relative to partial
sums no larger than the result's scale, i.e. below 1e-5 of the max magnitude as well -- the rule of test_glow_kernels_gpu.py
(SUM_TOL only past 1000 rows) gives F32_TOL too."""
import ctypes

import pytest
import torch

from test_glow_kernels_gpu import F32_TOL, close, drop_keep, make_drop

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 777.0
GUARD = 64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def lens_for(b, t):
    """Ragged, with one item of length 0 and one of length T where the batch has room for both."""
    return {1: [(t + 1) // 2], 2: [0, t], 3: [t, 0, (t + 1) // 2]}[b]


def valid(lens, t):
    return (torch.arange(t)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1)


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def gate_ref(a64, cond64, keep, h):
    ad = a64 * keep + cond64[:, None, :]
    return torch.tanh(ad[..., :h]) * torch.sigmoid(ad[..., h:])


GATE_CASES = [  # B, T, H, L (layers in the cond tensor; the middle one is used), p
    (1, 1, 1, 1, 0.0), (1, 1, 3, 3, 0.05), (2, 63, 1, 3, 0.0), (2, 64, 3, 1, 0.05),
    (3, 65, 64, 3, 0.0), (3, 130, 192, 3, 0.05), (3, 130, 192, 1, 0.0), (1, 130, 64, 3, 0.05),
    (2, 65, 192, 3, 0.0), (3, 1, 64, 3, 0.05), (3, 64, 64, 1, 0.0), (2, 130, 3, 3, 0.05),
    (1, 63, 192, 3, 0.0), (3, 63, 3, 1, 0.05), (2, 1, 192, 3, 0.0), (3, 65, 1, 3, 0.05),
]


def _gate_inputs(b, t, h, n_layers, p):
    g = gen(1000 * b + 10 * t + h)
    a, dacts = 2 * torch.randn(b, t, 2 * h, generator=g), torch.randn(b, t, h, generator=g)      # dacts non-zero past lens too
    cond = torch.randn(b, 2 * h, generator=g)
    lens = lens_for(b, t)
    keep = drop_keep(11, 3, b * t * 2 * h, p).view(b, t, 2 * h) if p > 0 else torch.ones(b, t, 2 * h, dtype=torch.float64)
    a64, c64 = a.double().requires_grad_(True), cond.double().requires_grad_(True)
    ref = gate_ref(a64, c64, keep, h)
    (da_ref,) = torch.autograd.grad(ref, a64, dacts.double(), retain_graph=True)                # every row
    (dc_ref,) = torch.autograd.grad(ref, c64, dacts.double() * valid(lens, t))                  # the rows t < lens[b] only
    i = n_layers // 2
    cond_all = torch.full((b, 2 * h * n_layers), SENTINEL)
    cond_all[:, 2 * h * i:2 * h * (i + 1)] = cond
    return a, dacts, cond_all, i, lens, ref.detach(), da_ref, dc_ref


@pytest.mark.parametrize("b,t,h,n_layers,p", GATE_CASES)
def test_gate_cond_forward_da_and_dcond_through_autograd(b, t, h, n_layers, p):
    from smt_amd import glow
    a, dacts, cond_all, i, lens, ref, da_ref, dc_ref = _gate_inputs(b, t, h, n_layers, p)
    drop = make_drop(p)
    ad = a.to(DEV).requires_grad_(True)
    cd = cond_all.to(DEV).requires_grad_(True)
    before = cd.detach().clone()
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    view = cd[:, 2 * h * i:2 * h * (i + 1)]
    assert n_layers == 1 or b == 1 or view.stride(0) == 2 * h * n_layers               # the strided view, not a copy
    acts = glow.wn_gate_cond(ad, view, lens_d, drop)
    acts.backward(dacts.to(DEV))
    torch.cuda.synchronize()
    close(acts, ref, F32_TOL, "acts")
    close(ad.grad, da_ref, F32_TOL, "da")
    assert torch.equal(cd.detach(), before), "the forward or backward wrote into cond"
    grad = cd.grad.cpu()
    close(grad[:, 2 * h * i:2 * h * (i + 1)], dc_ref, F32_TOL, "d cond (through autograd)")
    other = torch.ones(2 * h * n_layers, dtype=torch.bool)
    other[2 * h * i:2 * h * (i + 1)] = False
    assert (grad[:, other] == 0).all(), "the other layers' slices of d cond must be exactly zero"
    for item, n in enumerate(lens):
        if n == 0:
            assert (grad[item] == 0).all(), "an item without valid rows has d cond = 0"


@pytest.mark.parametrize("b,t,h,n_layers,p", GATE_CASES)
def test_gate_cond_backward_into_guarded_destinations(b, t, h, n_layers, p):
    """The same d cond written (a) into a slice of a [B, 2H L] buffer -- the strided destination -- and (b) into a dense
    [B, 2H] one, each with guard elements behind it: the neighbouring slices and the guards keep their sentinel."""
    from smt_amd import glow
    a, dacts, cond_all, i, lens, _, da_ref, dc_ref = _gate_inputs(b, t, h, n_layers, p)
    drop = make_drop(p)
    ad, gd, cd = a.to(DEV), dacts.to(DEV), cond_all.to(DEV)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    view = cd[:, 2 * h * i:2 * h * (i + 1)]
    wide = 2 * h * n_layers
    buf = torch.full((b * wide + GUARD,), SENTINEL, device=DEV)
    dest = buf[:b * wide].view(b, wide)[:, 2 * h * i:2 * h * (i + 1)]
    da, out = glow.gate_cond_backward(ad, gd, view, lens_d, drop, dcond=dest)
    dense_buf = torch.full((b * 2 * h + GUARD,), SENTINEL, device=DEV)
    dense = dense_buf[:b * 2 * h].view(b, 2 * h)
    glow.gate_cond_backward(ad, gd, view, lens_d, drop, dcond=dense)
    torch.cuda.synchronize()
    assert out.data_ptr() == dest.data_ptr()
    close(da, da_ref, F32_TOL, "da")
    close(dest, dc_ref, F32_TOL, "d cond (strided destination)")
    close(dense, dc_ref, F32_TOL, "d cond (dense destination)")
    assert torch.equal(bits(dest), bits(dense)), "the destination's layout changed the sums"
    keep = torch.ones(b, wide, dtype=torch.bool)
    keep[:, 2 * h * i:2 * h * (i + 1)] = False
    host = buf.cpu()
    assert (host[:b * wide].view(b, wide)[keep] == SENTINEL).all(), "a neighbouring slice of the strided destination was written"
    assert (host[b * wide:] == SENTINEL).all() and (dense_buf.cpu()[b * 2 * h:] == SENTINEL).all(), "guard elements were written"


def test_the_earlier_bug_is_refused_before_the_launch():
    """A dense [B, 2H] destination can only ever be passed with its own stride; a stride taken from cond's view does not fit the
    destination's storage, and the extent check says so before anything runs."""
    from smt_amd import glow
    b, h, n_layers = 3, 8, 3
    dense = torch.zeros(b, 2 * h, device=DEV)
    with pytest.raises(ValueError, match="d cond"):
        glow.check_extent(dense, b, 2 * h * n_layers, 2 * h, "d cond")
    with pytest.raises(AssertionError, match="dense"):
        glow._item_rows(torch.zeros(2 * h, b, device=DEV).t(), 2 * h, "cond")          # columns apart: not rows of floats


@pytest.mark.parametrize("p", [0.0, 0.05])
def test_zero_condition_is_the_unconditioned_gate_bit_for_bit(p):
    from smt_amd import glow
    b, t, h = 3, 130, 192
    a = (2 * torch.randn(b, t, 2 * h, generator=gen(7))).to(DEV)
    a[0, 0, :4] = torch.tensor([-0.0, 0.0, -1e-30, 1e-30], device=DEV)
    drop = make_drop(p)
    plain = glow.wn_gate(a, drop)
    cond = glow.wn_gate_cond(a, torch.zeros(b, 2 * h, device=DEV), torch.tensor([t, 0, 5], dtype=torch.int32, device=DEV), drop)
    assert torch.equal(bits(plain), bits(cond))


def test_gate_cond_backward_is_bitwise_reproducible():
    from smt_amd import glow
    b, t, h = 3, 130, 192
    g = gen(8)
    a, dacts = (2 * torch.randn(b, t, 2 * h, generator=g)).to(DEV), torch.randn(b, t, h, generator=g).to(DEV)
    cond = torch.randn(b, 2 * h * 3, generator=g).to(DEV)[:, 2 * h:4 * h]
    lens = torch.tensor([130, 77, 1], dtype=torch.int32, device=DEV)
    runs = [glow.gate_cond_backward(a, dacts, cond, lens, make_drop(0.05)) for _ in range(2)]
    assert torch.equal(bits(runs[0][1]), bits(runs[1][1])) and torch.equal(bits(runs[0][0]), bits(runs[1][0]))


CONCAT_CASES = [(1, 1, 8, 8, 16), (3, 65, 64, 16, 128), (2, 130, 192, 64, 256)]      # B, T, H, gin, W


@pytest.mark.parametrize("b,t,h,gin,w", CONCAT_CASES)
def test_bcast_concat_and_its_gradient(b, t, h, gin, w):
    from smt_amd import glow
    g = gen(9 + t)
    x, dout = torch.randn(b, t, h, generator=g), torch.randn(b, t, w, generator=g) + 0.5     # dout non-zero everywhere
    emb = torch.randn(b, gin + 5, generator=g)
    lens = {1: [1], 2: [0, t], 3: [t, 0, 33]}[b]
    m = valid(lens, t)
    ref = torch.zeros(b, t, w, dtype=torch.float64)
    ref[..., :h] = x.double() * m
    ref[..., h:h + gin] = emb[:, 3:3 + gin].double()[:, None, :] * m
    dg_ref = (dout.double() * m)[..., h:h + gin].sum(1)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        ed = emb.to(DEV).requires_grad_(True)
        out = glow.bcast_concat(x.to(DEV), ed[:, 3:3 + gin], lens_d, w)                   # g as a strided view of a wider tensor
        out.backward(dout.to(DEV))
        outs.append((out.detach(), ed.grad))
    out, demb = outs[0]
    assert out.shape == (b, t, w) and torch.equal(out.cpu().double(), ref), "bcast_concat copies: it must be exact"
    assert (out.cpu()[..., h + gin:] == 0).all() and (out.cpu() * ~m == 0).all()
    close(demb[:, 3:3 + gin], dg_ref, F32_TOL, "d g")
    assert (demb.cpu()[:, :3] == 0).all() and (demb.cpu()[:, 3 + gin:] == 0).all()
    assert torch.equal(bits(outs[0][1]), bits(outs[1][1])), "d g differs between two runs"
    with pytest.raises(AssertionError):
        glow.bcast_concat(x.to(DEV).requires_grad_(True), emb.to(DEV)[:, :gin], lens_d, w)   # x enters detached


def test_item_colsum_into_a_guarded_strided_destination():
    from smt_amd import glow, native as N
    b, t, w, col0, ncol, stride = 3, 130, 128, 64, 16, 40
    dout = (torch.randn(b, t, w, generator=gen(12)) + 0.5).to(DEV)
    lens = [130, 0, 65]
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    buf = torch.full((b * stride + GUARD,), SENTINEL, device=DEV)
    dest = buf[:b * stride].view(b, stride)[:, 7:7 + ncol]
    ptr, st = glow._item_rows(dest, ncol, "d g")
    assert st == stride
    lib = N.lib()
    ws = N.workspace.get(max(lib.smt_glow_gate_cond_workspace_bytes(b, t, ncol), 16), dout.device)
    N.check(lib.smt_glow_item_colsum(N.ptr(dout), N.ptr(lens_d), ptr, st, b, t, w, col0, ncol, N.ptr(ws), ws.numel(), N.stream_ptr()),
            "smt_glow_item_colsum")
    torch.cuda.synchronize()
    close(dest, (dout.double().cpu() * valid(lens, t))[..., col0:col0 + ncol].sum(1), F32_TOL, "column sums")
    keep = torch.ones(b, stride, dtype=torch.bool)
    keep[:, 7:7 + ncol] = False
    host = buf.cpu()
    assert (host[:b * stride].view(b, stride)[keep] == SENTINEL).all() and (host[b * stride:] == SENTINEL).all()


def test_argument_checks_return_an_error_without_launching():
    """cond_stride < 2H, dcond_stride < 2H, W < H + gin and a workspace that is too small come back through N.check as errors;
    the outputs keep their sentinel and the device stays usable."""
    from smt_amd import native as N
    lib = N.lib()
    b, t, h, gin = 2, 5, 8, 4
    a, dacts = torch.randn(b, t, 2 * h, device=DEV), torch.randn(b, t, h, device=DEV)
    cond = torch.randn(b, 2 * h, device=DEV)
    acts = torch.full((b, t, h), SENTINEL, device=DEV)
    da, dcond = torch.full((b, t, 2 * h), SENTINEL, device=DEV), torch.full((b, 2 * h), SENTINEL, device=DEV)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    p = N.ptr
    with pytest.raises(RuntimeError, match="cond_stride"):
        N.check(lib.smt_glow_gate_cond_fwd(p(a), p(cond), 2 * h - 1, p(acts), b, t, h, 0, None, 0, 1.0, N.stream_ptr()), "gate_cond_fwd")
    with pytest.raises(RuntimeError, match="cond_stride"):
        N.check(lib.smt_glow_gate_cond_bwd(p(a), p(dacts), p(cond), 2 * h - 1, None, p(da), p(dcond), 2 * h, b, t, h, 0, None, 0, 1.0,
                                           p(ws), ws.numel(), N.stream_ptr()), "gate_cond_bwd")
    with pytest.raises(RuntimeError, match="dcond_stride"):
        N.check(lib.smt_glow_gate_cond_bwd(p(a), p(dacts), p(cond), 2 * h, None, p(da), p(dcond), 2 * h - 1, b, t, h, 0, None, 0, 1.0,
                                           p(ws), ws.numel(), N.stream_ptr()), "gate_cond_bwd")
    with pytest.raises(RuntimeError, match="workspace"):
        N.check(lib.smt_glow_gate_cond_bwd(p(a), p(dacts), p(cond), 2 * h, None, p(da), p(dcond), 2 * h, b, t, h, 0, None, 0, 1.0,
                                           p(ws), 2 * 2 * h * 4 - 1, N.stream_ptr()), "gate_cond_bwd")
    x, g = torch.randn(b, t, h, device=DEV), torch.randn(b, gin, device=DEV)
    out = torch.full((b, t, 16), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="width"):
        N.check(lib.smt_glow_bcast_concat(p(x), p(g), gin, None, p(out), b, t, h, gin, h + gin - 1, N.stream_ptr()), "bcast_concat")
    dg = torch.full((b, gin), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="width"):
        N.check(lib.smt_glow_item_colsum(p(out), None, p(dg), gin, b, t, h + gin - 1, h, gin, p(ws), ws.numel(), N.stream_ptr()), "item_colsum")
    torch.cuda.synchronize()
    for name, v in (("acts", acts), ("da", da), ("d cond", dcond), ("out", out), ("d g", dg)):
        assert (v == SENTINEL).all(), f"{name} was written by a refused call"
    assert isinstance(ctypes.c_void_p(a.data_ptr()).value, int) and float((a * 0).sum()) == 0.0
