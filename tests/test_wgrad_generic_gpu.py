"""conv_wgrad_kernel, the generic weight-gradient kernel (csrc/conv_wgrad.hip): register prefetch of the next tile, two
fragment requests in flight in the bf16 k-loop, residue planes for the strided bf16 x tile.  Every case calls
smt_conv1d_wgrad directly, asserts that the plan names `conv_wgrad`, and checks dw / db against float64 sums of the same
bf16 / fp32 operands, run-to-run bit-identity, and a one-hot dy that picks single input rows out exactly."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# name: dtype, c_in, c_out, taps, stride, dil, pad, out_stride, out_offset, zero_page
KINDS = {
    "down64": ("bf16", 64, 64, 4, 2, 1, 1, 1, 0, True),       # k = 4, stride 2: residue planes, 5 accumulator planes
    "down128": ("bf16", 64, 128, 4, 2, 1, 1, 1, 0, True),     # two blocks of output channels
    "up0": ("bf16", 64, 64, 2, 1, 1, 1, 2, 0, True),          # the two 2-tap phases of the transposed conv: dy rows 2m, 2m + 1
    "up1": ("bf16", 64, 64, 2, 1, 1, 0, 2, 1, True),
    # taps in planes (0, 2, 1, 0) at rows (0, 0, 1, 2): the general residue rule; 388 staged rows, 100 beyond the prefetch
    "s3d2": ("bf16", 64, 64, 4, 3, 2, 2, 1, 0, True),
    "k5d3_128": ("bf16", 128, 128, 5, 1, 3, 6, 1, 0, False),  # the 128-channel instance (8 waves per workgroup)
    "f32k3": ("f32", 32, 64, 3, 1, 1, 1, 1, 0, False),        # fp32, half a channel block
    "f32s2": ("f32", 64, 64, 4, 2, 1, 1, 1, 0, False),        # fp32 keeps its scalar strided reads
}

CASES = (
    [(k, 3, t, None) for k in ("down64", "down128", "up0", "up1") for t in (1, 127, 129, 385)]
    # 4 tiles per chunk, a partial last tile and a partial last chunk: the prefetch runs through a buffer reuse and drains
    + [(k, 2, 100000, None) for k in ("down64", "up0", "up1")]
    + [("down64", 3, 129, 259)]                               # odd t_in
    + [("s3d2", 3, 300, None), ("s3d2", 2, 5000, None)]
    + [("k5d3_128", 3, 1000, None), ("k5d3_128", 2, 40000, None)]
    + [("f32k3", 3, 300, None), ("f32k3", 2, 40000, None), ("f32s2", 3, 385, None)]
)


@pytest.mark.parametrize("kind,b,t_out,t_in", CASES)
def test_generic_wgrad_matches_float64(kind, b, t_out, t_in):
    from smt_amd import convops as C
    dt_name, c_in, c_out, taps, stride, dil, pad, os_, oo, zero_page = KINDS[kind]
    dt = torch.bfloat16 if dt_name == "bf16" else torch.float32
    if t_in is None:
        t_in = stride * t_out if stride > 1 else t_out
    t_y = t_out * os_
    g = torch.Generator(device="cuda").manual_seed(11 * t_out + c_out + taps)
    x = torch.randn(b, t_in, c_in, device="cuda", generator=g).to(dt)
    dy = torch.randn(b, t_y, c_out, device="cuda", generator=g).to(dt)
    lens = torch.tensor([t_in, max(1, t_in // 3), 1][:b], device="cuda", dtype=torch.int32)   # ragged, a length of 1
    lib = C.N.lib()

    def run(dout):
        dw = torch.full((c_out, c_in, taps), 9.0, device="cuda")
        db = torch.full((c_out,), 9.0, device="cuda")
        d = C._base_desc(x, dout, lens, c_in, c_out, taps, stride, dil, pad, t_out, t_y=t_y, out_stride=os_, out_offset=oo)
        if zero_page:
            d.zero_page = C._p(C._zero_page(x.device))
        name = lib.smt_conv1d_wgrad_kernel_name(ctypes.byref(d)).decode()
        ws = torch.empty(max(16, lib.smt_conv1d_wgrad_workspace_bytes(ctypes.byref(d))), dtype=torch.uint8, device="cuda")
        arr = (ctypes.c_int * taps)(*range(taps))
        C.N.check(lib.smt_conv1d_wgrad(ctypes.byref(d), C._p(dw), c_in * taps, taps, 1, arr, C._p(db), C._p(ws), ws.numel(),
                                       C.N.stream_ptr()), "smt_conv1d_wgrad")
        torch.cuda.synchronize()
        return name, dw, db

    name, dw, db = run(dy)
    assert name == "conv_wgrad"
    _, dw2, db2 = run(dy)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)                  # fixed summation order: bit-identical

    # float64 reference
    xm = x.double()
    xm = xm * (torch.arange(t_in, device="cuda")[None, :] < lens[:, None]).double()[:, :, None]
    dyr = dy.double()[:, oo::os_][:, :t_out]
    ref = torch.zeros(c_out, c_in, taps, dtype=torch.float64, device="cuda")
    for j in range(taps):
        rows = stride * torch.arange(t_out, device="cuda") - pad + j * dil
        ok = (rows >= 0) & (rows < t_in)
        xs = torch.zeros(b, t_out, c_in, dtype=torch.float64, device="cuda")
        xs[:, ok] = xm[:, rows[ok]]
        ref[:, :, j] = torch.einsum("bto,bti->oi", dyr, xs)
    dbr = dyr.sum((0, 1))
    err_w = float((dw.double() - ref).abs().max())
    err_b = float((db.double() - dbr).abs().max())
    tol_w = 2e-6 * float(ref.abs().max()) * (b * t_out) ** 0.5 + 1e-4
    tol_b = 2e-6 * float(dbr.abs().max()) * (b * t_out) ** 0.5 + 1e-3
    print(f"{kind} b {b} t_out {t_out}: dw err {err_w:.3e} (tol {tol_w:.3e})  db err {err_b:.3e} (tol {tol_b:.3e})")
    assert err_w <= tol_w
    assert err_b <= tol_b

    # one-hot dy: the gradient IS the shifted input rows (the last output row of item 0, a row inside item 1)
    hot = torch.zeros_like(dy)
    picks = [(0, t_out - 1, 5), (1, t_out // 4, 9)]
    for bi, m, co in picks:
        hot[bi, m * os_ + oo, co] = 1
    _, dwh, dbh = run(hot)
    for bi, m, co in picks:
        for j in range(taps):
            r = stride * m - pad + j * dil
            want = x[bi, r].float() if 0 <= r < int(lens[bi]) else torch.zeros(c_in, device="cuda")
            assert torch.equal(dwh[co, :, j], want), (bi, m, j)
    rest = torch.ones(c_out, dtype=torch.bool, device="cuda")
    rest[[5, 9]] = False
    assert float(dwh[rest].abs().max()) == 0 and float(dbh.sum()) == 2.0
