"""Conv-stack kernels (libsmt_hip.so via smt_amd.convops) against a plain PyTorch fp32 reference of
the same op on the GPU.  fp32 path: exact-fp32 MFMA fma chains -> tight tolerance; bf16 path: bf16
operands / fp32 accumulate -> tolerance relative to the tensor's max magnitude."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vqvae_oracle as orc

pytestmark = pytest.mark.gpu


def tol(dtype):
    return dict(f=2e-5, g=2e-4) if dtype == torch.float32 else dict(f=1.5e-2, g=3e-2)


def close(a, b, rel):
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() <= rel * b.abs().max().item() + 1e-6


def ref_mask(lens, t):
    return (torch.arange(t, device=lens.device)[None, :] < lens[:, None]).float().unsqueeze(-1)


GEOMS = [  # cin, cout, k, dil, stride, pad
    (64, 128, 1, 1, 1, 0), (128, 128, 3, 1, 1, 1), (128, 128, 5, 3, 1, 6), (128, 128, 7, 9, 1, 27),
    (128, 128, 9, 27, 1, 108), (64, 64, 4, 1, 2, 1), (128, 64, 4, 1, 2, 1), (64, 128, 3, 1, 1, 1),
    (16, 32, 3, 1, 1, 1), (32, 32, 9, 27, 1, 108), (32, 16, 4, 1, 2, 1), (512, 64, 1, 1, 1, 0),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geom", GEOMS)
def test_conv1d_forward_backward(geom, dtype):
    from smt_amd import convops
    cin, cout, k, dil, stride, pad = geom
    g = torch.Generator(device="cuda").manual_seed(hash(geom) % 1000)
    b, t = 3, 2 * 173 if stride == 2 else 333
    x = torch.randn(b, t, cin, device="cuda", generator=g)
    w = torch.randn(cout, cin, k, device="cuda", generator=g) / (cin * k) ** 0.5
    bias = torch.randn(cout, device="cuda", generator=g)
    lens = torch.tensor([t, t - 37, 5], device="cuda", dtype=torch.int32)
    t_out = (t + 2 * pad - dil * (k - 1) - 1) // stride + 1
    res = torch.randn(b, t_out, cout, device="cuda", generator=g)
    xq, resq = x.to(dtype), res.to(dtype)

    xa = xq.clone().requires_grad_(True); wa = w.clone().requires_grad_(True); ba = bias.clone().requires_grad_(True)
    ra = resq.clone().requires_grad_(True)
    y = convops.conv1d(xa, wa, ba, stride=stride, padding=pad, dilation=dil, lens=lens, residual=ra)
    dy = torch.randn(b, t_out, cout, device="cuda", generator=g).to(dtype)
    y.backward(dy)

    xr = xq.float().clone().requires_grad_(True); wr = w.to(dtype).float().clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True); rr = resq.float().clone().requires_grad_(True)
    yr = F.conv1d((xr * ref_mask(lens, t)).transpose(1, 2), wr, br, stride=stride, padding=pad, dilation=dil)
    yr = yr.transpose(1, 2) + rr
    yr.backward(dy.float())
    tl = tol(dtype)
    assert y.shape == yr.shape
    assert close(y, yr, tl["f"]), "forward"
    assert close(xa.grad, xr.grad, tl["g"]), "dx"
    assert close(wa.grad, wr.grad, tl["g"]), "dw"
    assert close(ba.grad, br.grad, tl["g"]), "db"
    assert torch.equal(ra.grad, dy)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (16, 32)])
def test_conv_transpose1d(cin, cout, dtype):
    from smt_amd import convops
    g = torch.Generator(device="cuda").manual_seed(3)
    b, t, k, s, pad = 3, 211, 4, 2, 1
    x = torch.randn(b, t, cin, device="cuda", generator=g).to(dtype)
    w = torch.randn(cin, cout, k, device="cuda", generator=g) / (cin * 2) ** 0.5
    bias = torch.randn(cout, device="cuda", generator=g)
    lens = torch.tensor([t, 100, 0], device="cuda", dtype=torch.int32)
    xa = x.clone().requires_grad_(True); wa = w.clone().requires_grad_(True); ba = bias.clone().requires_grad_(True)
    y = convops.conv_transpose1d(xa, wa, ba, stride=s, padding=pad, lens=lens)
    dy = torch.randn_like(y)
    y.backward(dy)
    xr = x.float().clone().requires_grad_(True); wr = w.to(dtype).float().clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    yr = F.conv_transpose1d((xr * ref_mask(lens, t)).transpose(1, 2), wr, br, stride=s, padding=pad).transpose(1, 2)
    yr.backward(dy.float())
    tl = tol(dtype)
    assert y.shape == yr.shape == (b, 2 * t, cout)
    assert close(y, yr, tl["f"]) and close(xa.grad, xr.grad, tl["g"])
    assert close(wa.grad, wr.grad, tl["g"]) and close(ba.grad, br.grad, tl["g"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gate_mix(dtype):
    from smt_amd import convops
    g = torch.Generator(device="cuda").manual_seed(4)
    b, t, w, depth = 2, 157, 64, 4
    z = (2 * torch.randn(b, t, depth * 2 * w, device="cuda", generator=g)).to(dtype)
    za = z.clone().requires_grad_(True)
    out = convops.gate_mix(za, depth)
    dg = torch.randn_like(out)
    out.backward(dg)
    zr = z.float().clone().requires_grad_(True)
    zz = zr.view(b, t, depth, 2, w)
    ref = (torch.tanh(zz[:, :, :, 0]) * torch.softmax(zz[:, :, :, 1], dim=2)).sum(2)
    ref.backward(dg.float())
    tl = tol(dtype)
    assert close(out, ref, max(tl["f"], 1e-5)) and close(za.grad, zr.grad, max(tl["g"], 1e-4))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_in_and_conv_out(dtype):
    from smt_amd import convops
    g = torch.Generator(device="cuda").manual_seed(6)
    b, t, c = 3, 1000, 64
    x = torch.rand(b, t, device="cuda", generator=g) * 2 - 1
    w = torch.randn(c, 1, 4, device="cuda", generator=g) * 0.5
    bias = torch.randn(c, device="cuda", generator=g)
    lens = torch.tensor([t, 640, 128], device="cuda", dtype=torch.int32)
    wa = w.clone().requires_grad_(True); ba = bias.clone().requires_grad_(True)
    y = convops.conv_in(x, wa, ba, stride=2, padding=1, lens=lens, out_dtype=dtype)
    dy = torch.randn_like(y)
    y.backward(dy)
    wr = w.clone().requires_grad_(True); br = bias.clone().requires_grad_(True)
    yr = F.conv1d((x.unsqueeze(-1) * ref_mask(lens, t)).transpose(1, 2), wr, br, stride=2, padding=1).transpose(1, 2)
    yr.backward(dy.float())
    tl = tol(dtype)
    assert close(y, yr, max(tl["f"], 1e-6) if dtype == torch.float32 else 8e-3)
    assert close(wa.grad, wr.grad, 1e-4) and close(ba.grad, br.grad, 1e-4)

    c2 = 128
    h = torch.randn(b, t, c2, device="cuda", generator=g).to(dtype)
    wo = torch.randn(1, c2, 1, device="cuda", generator=g) * 0.1
    bo = torch.randn(1, device="cuda", generator=g)
    ha = h.clone().requires_grad_(True); woa = wo.clone().requires_grad_(True); boa = bo.clone().requires_grad_(True)
    o = convops.conv_out(ha, woa, boa, lens=lens)
    do = torch.randn_like(o)
    o.backward(do)
    hr = h.float().clone().requires_grad_(True); wor = wo.clone().requires_grad_(True); bor = bo.clone().requires_grad_(True)
    oref = F.conv1d((hr * ref_mask(lens, t)).transpose(1, 2), wor, bor)[:, 0]
    oref.backward(do)
    assert o.dtype == torch.float32 and close(o, oref, 1e-5)
    assert close(ha.grad, hr.grad, tl["f"]) and close(woa.grad, wor.grad, 1e-4) and close(boa.grad, bor.grad, 1e-4)


def test_gated_hifi_block_forward_backward_vs_oracle(golden):
    """One GatedHiFiBlock (reference fixture, eval mode) through the product modules: forward against
    the reference output, parameter + input gradients against the oracle's autograd (fp32)."""
    from models.vqvae.resnet import GatedHiFiBlock
    g = golden("gated_hifi")
    blk = GatedHiFiBlock(16, 4, dilation_growth_rate=3, kernel_size_growth_rate=2, zero_out=True).cuda()
    sd = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p.")}
    blk.load_state_dict(sd)
    blk.eval()
    x_nct = torch.from_numpy(g["x"])
    lens = torch.from_numpy(g["lens"])
    xa = x_nct.permute(0, 2, 1).contiguous().cuda().requires_grad_(True)
    y = blk(xa, lens.cuda().to(torch.int32))
    assert torch.allclose(y.detach().cpu().permute(0, 2, 1), torch.from_numpy(g["y"]), atol=2e-5)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(0))
    y.backward(dy.cuda())
    # oracle autograd on CPU
    p = {"b." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x_nct.clone().requires_grad_(True)
    mask = orc.sequence_mask(lens, x_nct.shape[-1]).unsqueeze(1).float()
    yr = orc.gated_hifi_block(xr, mask, p, "b", orc.VQVAEConfig(width=16, multipliers=(1, 1, 1)), orc.no_dropout)
    yr.backward(dy.permute(0, 2, 1))
    # A pre-activation that is ~0 can land on the other side of the ReLU on the GPU (different fp32
    # summation order); one such flip changes a handful of gradient entries by O(1e-2) of the max.
    # So the metric is the relative L2 error of each tensor.
    def check(a, b, name):
        a, b = a.float(), b.float()
        assert (a - b).norm() <= 2e-2 * b.norm() + 1e-7, name
    check(xa.grad.cpu().permute(0, 2, 1), xr.grad, "dx")
    for name, prm in blk.named_parameters():
        check(prm.grad.cpu(), p["b." + name].grad, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gated_hifi_block_train_mode_counter_dropout_vs_oracle(dtype, golden):
    """Train mode: the dropout masks come from the counter-based generator, which the oracle restates
    bit-exactly, so the whole block (forward + every gradient) is checkable with dropout ON."""
    from models.vqvae.resnet import GatedHiFiBlock
    g = golden("gated_hifi")
    site_base, seed, p_drop = 24, 7, 0.1
    blk = GatedHiFiBlock(16, 4, dilation_growth_rate=3, kernel_size_growth_rate=2, zero_out=True, dropout=p_drop,
                         site_base=site_base).cuda()
    sd = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p.")}
    blk.load_state_dict(sd)
    blk.train()
    x_nct = torch.from_numpy(g["x"])
    lens = torch.from_numpy(g["lens"])
    xa = x_nct.permute(0, 2, 1).contiguous().cuda().to(dtype).requires_grad_(True)
    y = blk(xa, lens.cuda().to(torch.int32), drop_seed=seed)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(0))
    y.backward(dy.cuda().to(dtype))
    ids = {f"b.blocks.{d}.1.drop{s}": site_base + 2 * d + s for d in range(4) for s in (0, 1)}
    drop = orc.make_counter_dropout(seed, p_drop, ids)
    prm = {"b." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x_nct.clone().requires_grad_(True)
    mask = orc.sequence_mask(lens, x_nct.shape[-1]).unsqueeze(1).float()
    yr = orc.gated_hifi_block(xr, mask, prm, "b", orc.VQVAEConfig(width=16, multipliers=(1, 1, 1)), drop)
    yr.backward(dy.permute(0, 2, 1))
    rel = 2e-2 if dtype == torch.float32 else 6e-2     # relative L2 (ReLU-boundary flips, see above)
    fwd = 2e-5 if dtype == torch.float32 else 2e-2
    assert (y.detach().float().cpu().permute(0, 2, 1) - yr.detach()).norm() <= fwd * yr.detach().norm()
    assert (xa.grad.float().cpu().permute(0, 2, 1) - xr.grad).norm() <= rel * xr.grad.norm()
    for name, q in blk.named_parameters():
        ref = prm["b." + name].grad
        assert (q.grad.cpu() - ref).norm() <= rel * ref.norm() + 1e-7, name
    # dropout really happened: eval-mode output differs
    blk.eval()
    y_eval = blk(xa.detach(), lens.cuda().to(torch.int32))
    assert (y_eval.float() - y.detach().float()).abs().max() > 1e-3


def test_act_out_epilogue_matches_counter_spec():
    """Kernel level: y_act = relu(dropout(y)) written by the conv epilogue, per-site keys."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(2)
    b, t, cin, cout, sw = 2, 203, 64, 256, 128
    x = torch.randn(b, t, cin, device="cuda", generator=g)
    w = torch.randn(cout, cin, 1, device="cuda", generator=g) / 8
    bias = torch.randn(cout, device="cuda", generator=g)
    y = torch.empty(b, t, cout, device="cuda")
    u = torch.empty_like(y)
    seed, p = 5, 0.1
    keys = [C.dropout_key(seed, 3), C.dropout_key(seed, 11)]
    d = C._base_desc(x, y, None, cin, cout, 1, 1, 1, 0, t)
    wp = C._pack_fwd(w, torch.float32)
    d.w, d.bias = C._p(wp), C._p(bias)
    C._set_act_out(d, u, keys, int(round(p * 65536)), 1.0 / (1.0 - p), sw)
    C._launch(d, "conv_fwd")
    torch.cuda.synchronize()
    yr = torch.nn.functional.conv1d(x.transpose(1, 2), w, bias).transpose(1, 2)
    assert torch.allclose(y, yr, atol=1e-5)
    for s, site in enumerate((3, 11)):
        keep = torch.from_numpy(orc.dropout_keep_ntc(seed, site, b, t, sw, p)).cuda()
        ref = torch.relu(y[:, :, s * sw:(s + 1) * sw]) * keep / (1.0 - p)
        assert torch.allclose(u[:, :, s * sw:(s + 1) * sw], ref, atol=1e-6, rtol=1e-6)
        assert abs(keep.float().mean().item() - 0.9) < 0.01


@pytest.mark.parametrize("k,dil", [(1, 1), (3, 1), (5, 3), (7, 9), (9, 27)])
def test_lds_dma_conv_kernel_matches_generic_kernel(k, dil):
    """The LDS-DMA variant (bf16, C % 128 == 0, XOR-swizzled operands) against the register-staged generic
    kernel on the same inputs: same MFMA, same k order -> bit-identical outputs; ragged lens, residual,
    activation-derivative epilogue and the activated second output included."""
    lds_dma_conv_vs_generic(k, dil, 700)


def test_persistent_1x1_kernel_at_three_tiles_per_workgroup():
    """conv1x1_dma as above at 3 x 44000 rows: 1032 tiles on 512 workgroups, three tiles per workgroup -- the second reuse
    of a staging buffer, which the 700-row case (two tiles per workgroup) does not reach."""
    lds_dma_conv_vs_generic(1, 1, 44000)


def lds_dma_conv_vs_generic(k, dil, t):
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(k)
    b, c = 3, 128
    big = torch.randn(b, t, 512, device="cuda", generator=g).to(torch.bfloat16)
    x = big[:, :, 128:256]                                   # channel slice: row pitch 512
    w = torch.randn(c, c, k, device="cuda", generator=g) / (c * k) ** 0.5
    bias = torch.randn(c, device="cuda", generator=g)
    res = torch.randn(b, t, c, device="cuda", generator=g).to(torch.bfloat16)
    u_src = torch.relu(torch.randn(b, t, c, device="cuda", generator=g)).to(torch.bfloat16)
    lens = torch.tensor([t, 333, 1], device="cuda", dtype=torch.int32)
    pad = (k - 1) * dil // 2
    outs = []
    for dma in (False, True):
        y = torch.zeros(b, t, c, device="cuda", dtype=torch.bfloat16)
        u = torch.zeros_like(y)
        wp = C._pack_fwd(w, torch.bfloat16, dma)
        d = C._base_desc(x, y, lens, c, c, k, 1, dil, pad, t)
        d.w, d.bias = C._p(wp), C._p(bias)
        if dma:
            C._use_dma(d, wp)
        d.res, d.bs_res, d.ld_res = C._geom(res)
        d.lens_out = C._p(lens)
        C._set_act_grad(d, u_src, 1.111)
        C._set_act_out(d, u, [C.dropout_key(3, 5)], 6554, 1.0 / 0.9, c)
        C._launch(d, "t")
        torch.cuda.synchronize()
        outs.append((y, u))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][0].float().abs().sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("k,dil", [(3, 1), (5, 3), (7, 9), (9, 27)])
@pytest.mark.parametrize("epi", ["plain", "res+actgrad+actout", "actout-only", "res+actgrad"])
def test_weight_stationary_conv_kernel_matches_generic_kernel(k, dil, epi):
    """The persistent weight-stationary kernel (weights in registers, double-buffered LDS-DMA activation tiles,
    dilation classes for dil >= 8) against the register-staged generic kernel on enough rows for it to be
    dispatched: same MFMA and accumulation order -> bit-identical outputs, ragged lens included."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(100 + k)
    b, t, c = 3, 50021, 128
    big = torch.randn(b, t, 256, device="cuda", generator=g).to(torch.bfloat16)
    x = big[:, :, 128:256]                                   # channel slice: row pitch 256
    w = torch.randn(c, c, k, device="cuda", generator=g) / (c * k) ** 0.5
    bias = torch.randn(c, device="cuda", generator=g)
    res = torch.randn(b, t, c, device="cuda", generator=g).to(torch.bfloat16)
    u_src = torch.relu(torch.randn(b, t, c, device="cuda", generator=g)).to(torch.bfloat16)
    lens = torch.tensor([t, 33333, 1], device="cuda", dtype=torch.int32)
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
        if epi.startswith("res+actgrad"):
            d.res, d.bs_res, d.ld_res = C._geom(res)
            C._set_act_grad(d, u_src, 1.111)
        if "actout" in epi:
            C._set_act_out(d, u, [C.dropout_key(3, 5)], 6554, 1.0 / 0.9, c)
        names.append(C._kernel_of(d))
        C._launch(d, "t")
        torch.cuda.synchronize()
        outs.append((y, u))
    two_waves = k <= 3 and epi in ("actout-only", "res+actgrad")          # conv_ws2_kernel: two staggered waves per SIMD
    assert names == ["conv_gemm", "conv_ws2" if two_waves else ("conv_ws_pipe" if epi == "actout-only" else "conv_ws")]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert (outs[0][1] if epi == "actout-only" else outs[0][0]).float().abs().sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("b,t", [(3, 700), (2, 33000), (1, 1)])
def test_fused_1x1_backward_matches_separate_kernels(b, t):
    """smt_conv1x1_bwd (one pass over dy and u) against the data-gradient conv + the weight-gradient kernel it
    replaces: the masked data gradient is bit-identical (same MFMA, same order, same rounding), the fp32 weight
    and bias gradients agree to summation-order round-off and match a float64 reference."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(7 * b + t)
    c = 128
    big = torch.randn(b, t, 512, device="cuda", generator=g).to(torch.bfloat16)
    dz = big[:, :, 256:384]                                  # channel slices of wider tensors: row pitch 512
    u_big = torch.relu(torch.randn(b, t, 512, device="cuda", generator=g)).to(torch.bfloat16)
    u2 = u_big[:, :, 128:256]
    w = torch.randn(c, c, 1, device="cuda", generator=g) / c ** 0.5
    scale = 1.0 / 0.9
    wb = C._pack_bwd(w, torch.bfloat16, True)

    def desc(dx):
        d = C._dgrad_stride1(dz, wb, dx, 1, 1, 0)
        C._use_dma(d, wb)
        C._set_act_grad(d, u2, scale)
        return d

    dx_ref = torch.zeros(b, t, c, device="cuda", dtype=torch.bfloat16)
    C._launch(desc(dx_ref), "t")
    dw_ref, db_ref = torch.empty_like(w), torch.empty(c, device="cuda")
    C._wgrad(C._base_desc(u2, dz, None, c, c, 1, 1, 1, 0, t), dw_ref, c, 1, 1, [0], db_ref)

    dx = torch.zeros_like(dx_ref)
    dw, db = torch.empty_like(w), torch.empty(c, device="cuda")
    C._conv1x1_bwd(desc(dx), dw, c, 1, db)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_ref)
    dw64 = torch.einsum("bto,bti->oi", dz.double(), u2.double())
    db64 = dz.double().sum((0, 1))
    tol = 1e-5 * float(dw64.abs().max()) + 1e-6
    assert float((dw[:, :, 0].double() - dw64).abs().max()) <= 20 * tol
    assert float((dw - dw_ref).abs().max()) <= 20 * tol
    assert float((db.double() - db64).abs().max()) <= 1e-5 * float(db64.abs().max()) + 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("b,t", [(3, 700), (2, 20011), (3, 44000)])
def test_folded_1x1_conv_matches_float64(b, t):
    """conv1x1_fold (y = W u + b + W2 x2 + b2, the K3 + recomputed-K1 residual of GatedHiFiBlock) against a float64
    evaluation of the same bf16 operands; x2 rows beyond lens read as 0, u rows are not masked.  (3, 44000): 1032 tiles on
    256 workgroups, five tiles per workgroup -- every staging buffer is reused, the last run is short."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(11 * b + t)
    c, w_in = 128, 64
    u_big = torch.randn(b, t, 512, device="cuda", generator=g).to(torch.bfloat16)
    u = u_big[:, :, 256:384]
    x = torch.randn(b, t, w_in, device="cuda", generator=g).to(torch.bfloat16)
    w3 = torch.randn(c, c, 1, device="cuda", generator=g) / c ** 0.5
    w1 = torch.randn(c, w_in, 1, device="cuda", generator=g) / w_in ** 0.5
    b3, b1 = torch.randn(c, device="cuda", generator=g), torch.randn(c, device="cuda", generator=g)
    lens = torch.tensor([t, t // 3, 1][:b], device="cuda", dtype=torch.int32)
    z_big = torch.zeros(b, t, 512, device="cuda", dtype=torch.bfloat16)
    z = z_big[:, :, 128:256]
    wp3, wp1 = C._pack_fwd(w3, torch.bfloat16, True), C._pack_fwd(w1, torch.bfloat16)
    d = C._base_desc(u, z, None, c, c, 1, 1, 1, 0, t)
    d.bias = C._p(b3)
    C._use_dma(d, wp3)
    d.x2, d.bs_x2, d.ld_x2 = C._geom(x)
    d.w2, d.bias2, d.c_in2, d.lens_in2 = C._p(wp1), C._p(b1), w_in, C._p(lens)
    assert C._kernel_of(d) == "conv1x1_fold"
    C._launch(d, "t")
    torch.cuda.synchronize()
    mask = (torch.arange(t, device="cuda")[None, :] < lens[:, None]).double()[:, :, None]
    ref = (torch.einsum("bti,oi->bto", u.double(), w3[:, :, 0].to(torch.bfloat16).double()) + b3.double()
           + torch.einsum("bti,oi->bto", x.double() * mask, w1[:, :, 0].to(torch.bfloat16).double()) + b1.double())
    err = (z.double() - ref).abs()
    assert float(err.max()) <= 2.0 ** -8 * float(ref.abs().max()) + 1e-3       # one bf16 rounding of the result
    assert float(z_big[:, :, :128].abs().max()) == 0 and float(z_big[:, :, 256:].abs().max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("k,dil", [(3, 1), (5, 3), (7, 9), (9, 27)])
def test_shifted_fragment_wgrad_matches_float64(k, dil):
    """conv_wgrad_shift_kernel (all taps of a dilated conv from one 16-row register window per k-step, dilation
    classes, tile ranges across (batch, class) items) against a float64 evaluation of the same bf16 operands, on
    enough rows for it to be dispatched; ragged lens, operands that are channel slices of wider tensors."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(200 + k)
    b, t, c = 3, 50021, 128
    xb = torch.randn(b, t, 256, device="cuda", generator=g).to(torch.bfloat16)
    dyb = torch.randn(b, t, 384, device="cuda", generator=g).to(torch.bfloat16)
    x, dy = xb[:, :, 128:256], dyb[:, :, 128:256]
    lens = torch.tensor([t, 33333, 1], device="cuda", dtype=torch.int32)
    pad = (k - 1) * dil // 2
    dw, db = torch.empty(c, c, k, device="cuda"), torch.empty(c, device="cuda")
    d = C._base_desc(x, dy, lens, c, c, k, 1, dil, pad, t)
    C._wgrad(d, dw, c * k, k, 1, list(range(k)), db)
    torch.cuda.synchronize()
    mask = (torch.arange(t, device="cuda")[None, :] < lens[:, None])[:, :, None]
    xm = torch.where(mask, x, torch.zeros_like(x)).double()
    xp = torch.nn.functional.pad(xm, (0, 0, pad, pad))
    ref = torch.stack([torch.einsum("bto,bti->oi", dy.double(), xp[:, s * dil:s * dil + t]) for s in range(k)], dim=2)
    tol = 2e-6 * float(ref.abs().max()) * (b * t) ** 0.5 + 1e-4     # fp32 accumulation over b*t rows
    assert float((dw.double() - ref).abs().max()) <= tol
    dbr = dy.double().sum((0, 1))
    assert float((db.double() - dbr).abs().max()) <= 2e-6 * float(dbr.abs().max()) * (b * t) ** 0.5 + 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("b,t,train", [(3, 700, True), (2, 20011, True), (2, 1000, False), (3, 44000, True)])
def test_k1_activated_output_kernel_matches_generic_kernel(b, t, train):
    """conv_k1act (64 -> 512, only u = relu(dropout(W x + b)) written, four dropout sites) against the generic
    kernel on the same inputs: bit-identical, ragged lens included.  (3, 44000): 1032 tiles on 512 workgroups, three tiles
    per workgroup -- the second reuse of a staging buffer."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(13 * b + t)
    w_in, c_out = 64, 512
    x = torch.randn(b, t, w_in, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(c_out, w_in, 1, device="cuda", generator=g) / w_in ** 0.5
    bias = torch.randn(c_out, device="cuda", generator=g)
    lens = torch.tensor([t, t // 3, 1][:b], device="cuda", dtype=torch.int32)
    wp = C._pack_fwd(w, torch.bfloat16)
    keys = [C.dropout_key(5, s) for s in range(4)] if train else [0] * 4
    thresh, scale = (6554, 1.0 / 0.9) if train else (0, 1.0)
    outs, names = [], []
    for fast in (False, True):
        u = torch.zeros(b, t, c_out, device="cuda", dtype=torch.bfloat16)
        d = C._base_desc(x, None, lens, w_in, c_out, 1, 1, 1, 0, t, t_y=t)
        d.w, d.bias = C._p(wp), C._p(bias)
        d.lens_out = C._p(lens)
        C._set_act_out(d, u, keys, thresh, scale, 128)
        if fast:
            d.zero_page = C._p(C._zero_page(x.device))
        names.append(C._kernel_of(d))
        C._launch(d, "t")
        torch.cuda.synchronize()
        outs.append(u)
    assert names == ["conv_gemm", "conv_k1act"]
    assert torch.equal(outs[0], outs[1])
    assert outs[0].float().abs().sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("b,t", [(3, 700), (2, 20011), (1, 1), (2, 128), (3, 44000)])
def test_gate_conv_forward_kernel_matches_generic_kernel(b, t):
    """conv1x1_c64 (the 64 -> 64 gate conv with the block input as residual, out = W g + b + x) against the generic kernel on
    the same inputs: bit-identical, ragged lens and channel-sliced (pitch 256) operands included.  (3, 44000): 2064 tiles on
    1024 workgroups, three tiles per workgroup -- the second reuse of a staging buffer."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(17 * b + t)
    big = torch.randn(b, t, 128, device="cuda", generator=g).to(torch.bfloat16)
    x = big[:, :, 64:128]                                          # channel slice: row pitch 128 elements
    res = torch.randn(b, t, 64, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(64, 64, 1, device="cuda", generator=g) / 8.0
    bias = torch.randn(64, device="cuda", generator=g)
    lens = torch.tensor([t, max(1, t // 3), 1][:b], device="cuda", dtype=torch.int32)
    wp = C._pack_fwd(w, torch.bfloat16)
    outs, names = [], []
    for fast in (False, True):
        y = torch.full((b, t, 64), 7.0, device="cuda", dtype=torch.bfloat16)
        d = C._base_desc(x, y, lens, 64, 64, 1, 1, 1, 0, t)
        d.w, d.bias = C._p(wp), C._p(bias)
        d.res, d.bs_res, d.ld_res = C._geom(res)
        if fast:
            d.zero_page = C._p(C._zero_page(x.device))
        names.append(C._kernel_of(d))
        C._launch(d, "t")
        torch.cuda.synchronize()
        outs.append(y)
    assert names == ["conv_gemm", "conv1x1_c64"]
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[1][0, lens[0]:], res[0, lens[0]:]) or int(lens[0]) == t   # rows beyond lens: the residual alone


@pytest.mark.gpu
@pytest.mark.parametrize("b,t", [(3, 700), (2, 20011), (1, 1)])
def test_fused_k1_backward_matches_separate_kernels(b, t):
    """smt_conv_k1_bwd (one pass over dh) against the data-gradient conv it replaces (within one bf16 rounding step,
    bitwise reproducible run to run) and a float64 reference for dx and the fp32 weight / bias gradients; ragged lens."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(17 * b + t)
    w_in, c_out = 64, 512
    dh = torch.randn(b, t, c_out, device="cuda", generator=g).to(torch.bfloat16)
    x = torch.randn(b, t, w_in, device="cuda", generator=g).to(torch.bfloat16)
    dout = torch.randn(b, t, w_in, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(c_out, w_in, 1, device="cuda", generator=g) / w_in ** 0.5
    lens = torch.tensor([t, t // 3, 1][:b], device="cuda", dtype=torch.int32)
    wb = C._pack_bwd(w, torch.bfloat16)

    dx_ref = torch.zeros(b, t, w_in, device="cuda", dtype=torch.bfloat16)
    d = C._dgrad_stride1(dh, wb, dx_ref, 1, 1, 0)
    d.lens_out = C._p(lens)
    d.res, d.bs_res, d.ld_res = C._geom(dout)
    C._launch(d, "t")
    dx = torch.zeros_like(dx_ref)
    dw, db = torch.empty_like(w), torch.empty(c_out, device="cuda")
    C._conv_k1_bwd(dh, x, wb, dout, dx, lens, dw, db)
    torch.cuda.synchronize()
    # the fused kernel splits the 512-channel contraction over two waves (lower half + upper half, fixed order), so
    # its fp32 sums differ from the one-chain kernel in the last bits: at most one bf16 rounding step apart
    diff = (dx.float() - dx_ref.float()).abs()
    scale_c = dx_ref.float().abs() + dout.float().abs()      # >= |bf16(conv)|, whose rounding step bounds the difference
    assert float((diff - 2.0 ** -6 * scale_c).max()) <= 1e-6
    assert float((diff > 0).float().mean()) < 0.02
    keep = (torch.arange(t, device="cuda")[None, :] < lens[:, None]).double()[:, :, None]
    dx64 = torch.einsum("bto,oi->bti", dh.double(), w[:, :, 0].to(torch.bfloat16).double()) * keep + dout.double()
    assert float(((dx.double() - dx64).abs() - 2.0 ** -6 * (dx64.abs() + dout.double().abs())).max()) <= 1e-2
    dx2 = torch.zeros_like(dx)
    C._conv_k1_bwd(dh, x, wb, dout, dx2, lens, dw, db)
    assert torch.equal(dx, dx2)                      # run-to-run reproducible
    mask = (torch.arange(t, device="cuda")[None, :] < lens[:, None]).double()[:, :, None]
    dw64 = torch.einsum("bto,bti->oi", dh.double(), x.double() * mask)
    db64 = dh.double().sum((0, 1))
    assert float((dw[:, :, 0].double() - dw64).abs().max()) <= 2e-6 * float(dw64.abs().max()) * (b * t) ** 0.5 + 1e-4
    assert float((db.double() - db64).abs().max()) <= 2e-6 * float(db64.abs().max()) * (b * t) ** 0.5 + 1e-3


@pytest.mark.gpu
def test_pack_cache_follows_in_place_weight_updates():
    """Packed operand copies are cached per (weight storage, layout) and repacked in one table-driven launch when a
    weight's version changes: outputs must follow an in-place (optimizer-style) update, forward and backward."""
    from smt_amd import convops as C, packing
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(2, 300, 32, device="cuda", generator=g, requires_grad=True)
    ws = [torch.nn.Parameter(torch.randn(64, 32, 3, device="cuda", generator=g) * 0.1) for _ in range(3)]
    bs = [torch.nn.Parameter(torch.randn(64, device="cuda", generator=g)) for _ in range(3)]

    def run():
        outs = []
        for w, b in zip(ws, bs):
            y = C._Conv1d.apply(x, w, b, None, None, 1, 1, 1)
            (gx,) = torch.autograd.grad(y.square().sum(), x)
            ref = torch.nn.functional.conv1d(x.detach().cpu().transpose(1, 2), w.detach().cpu(), b.detach().cpu(), padding=1)
            assert float((y.detach().cpu() - ref.transpose(1, 2)).abs().max()) <= 2e-5 * float(ref.abs().max()) + 1e-5
            outs.append((y.detach().clone(), gx.clone()))
        return outs

    first = run()
    import gc
    gc.collect()
    packing.prune()                                       # entries of dead parameters (earlier tests) go at the next repack anyway
    n_entries = packing.entry_count()
    again = run()                                         # nothing changed: cache hits, no new entries
    assert packing.entry_count() == n_entries
    assert all(torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]) for a, b_ in zip(first, again))
    with torch.no_grad():
        for w in ws:
            w.mul_(-0.5)                                  # in-place update bumps the version -> batched repack
    changed = run()                                       # run() re-checks against torch with the NEW weights
    assert packing.entry_count() == n_entries
    assert not torch.equal(first[0][0], changed[0][0]) and not torch.equal(first[0][1], changed[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("b,t", [(3, 700), (2, 20011), (1, 1), (3, 44000)])
def test_fused_gate_conv_backward_matches_separate_kernels(b, t):
    """smt_conv_gate_bwd (one pass over dout) against the data-gradient conv it replaces (bit-identical: same MFMA
    chain) and a float64 reference for the fp32 weight / bias gradients; ragged lens included.  (3, 44000): 1032 tiles on
    512 workgroups, three tiles per workgroup (the second reuse of a staging buffer), 168 workgroups without a tile."""
    from smt_amd import convops as C
    g_ = torch.Generator(device="cuda").manual_seed(19 * b + t)
    c = 64
    dout = torch.randn(b, t, c, device="cuda", generator=g_).to(torch.bfloat16)
    gbig = torch.randn(b, t, 128, device="cuda", generator=g_).to(torch.bfloat16)
    g = gbig[:, :, 64:128]                                    # channel slice: row pitch 128
    w = torch.randn(c, c, 1, device="cuda", generator=g_) / c ** 0.5
    lens = torch.tensor([t, t // 3, 1][:b], device="cuda", dtype=torch.int32)
    wb = C._pack_bwd(w, torch.bfloat16)
    dx_ref = torch.zeros(b, t, c, device="cuda", dtype=torch.bfloat16)
    d = C._dgrad_stride1(dout, wb, dx_ref, 1, 1, 0)
    d.lens_out = C._p(lens)
    C._launch(d, "t")
    dx = torch.zeros_like(dx_ref)
    dw, db = torch.empty_like(w), torch.empty(c, device="cuda")
    C._conv_gate_bwd(dout, g, wb, dx, lens, dw, db)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_ref)
    mask = (torch.arange(t, device="cuda")[None, :] < lens[:, None]).double()[:, :, None]
    dw64 = torch.einsum("bto,bti->oi", dout.double(), g.double() * mask)
    db64 = dout.double().sum((0, 1))
    assert float((dw[:, :, 0].double() - dw64).abs().max()) <= 2e-6 * float(dw64.abs().max()) * (b * t) ** 0.5 + 1e-4
    assert float((db.double() - db64).abs().max()) <= 2e-6 * float(db64.abs().max()) * (b * t) ** 0.5 + 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("kind,c_out,b,t", [("down", 64, 3, 2000), ("down", 128, 2, 9002), ("up0", 64, 3, 1500), ("up1", 128, 2, 7001),
                                            ("down", 64, 1, 2)])
def test_weight_gradient_of_the_resampling_convs(kind, c_out, b, t):
    """Weight / bias gradients of the 64-channel k = 4, stride-2 conv ("down": dW[co][ci][j] = sum dy[t][co] x[2t - 1 + j][ci])
    and of the two 2-tap phases of its transpose ("up0": rows x[m - 1], x[m] against dy[2m]; "up1": x[m], x[m + 1] against
    dy[2m + 1]) on the generic kernel, which they run on with or without a zero page, against float64 sums; ragged input
    lengths, one-hot dy picks out the input rows exactly."""
    import ctypes
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(7 * t + c_out)
    bf = torch.bfloat16
    if kind == "down":
        t_in, t_out, taps, stride, pad, os_, oo = 2 * t, t, 4, 2, 1, 1, 0
        t_y = t
    else:
        t_in, t_out, taps, stride, os_ = t, t, 2, 1, 2
        pad, oo = (1, 0) if kind == "up0" else (0, 1)
        t_y = 2 * t
    x = torch.randn(b, t_in, 64, device="cuda", generator=g).to(bf)
    dy = torch.randn(b, t_y, c_out, device="cuda", generator=g).to(bf)
    lens = torch.tensor([t_in, max(1, t_in // 3), 1][:b], device="cuda", dtype=torch.int32)

    def run(zero_page, dout):
        dw = torch.full((c_out, 64, taps), 9.0, device="cuda")
        db = torch.full((c_out,), 9.0, device="cuda")
        d = C._base_desc(x, dout, lens, 64, c_out, taps, stride, 1, pad, t_out, t_y=t_y, out_stride=os_, out_offset=oo)
        lib = C.N.lib()
        if zero_page:
            d.zero_page = C._p(C._zero_page(x.device))
        name = lib.smt_conv1d_wgrad_kernel_name(ctypes.byref(d)).decode()
        ws = torch.empty(max(16, lib.smt_conv1d_wgrad_workspace_bytes(ctypes.byref(d))), dtype=torch.uint8, device="cuda")
        arr = (ctypes.c_int * taps)(*range(taps))
        C.N.check(lib.smt_conv1d_wgrad(ctypes.byref(d), C._p(dw), 64 * taps, taps, 1, arr, C._p(db), C._p(ws), ws.numel(),
                                       C.N.stream_ptr()), "smt_conv1d_wgrad")
        torch.cuda.synchronize()
        return name, dw, db

    n0, dw0, db0 = run(False, dy)
    n1, dw1, db1 = run(True, dy)
    assert (n0, n1) == ("conv_wgrad", "conv_wgrad")
    # float64 reference
    xm = x.double().clone()
    for i in range(b):
        xm[i, int(lens[i]):] = 0
    dyr = dy.double()[:, oo::os_][:, :t_out]
    ref = torch.zeros(c_out, 64, taps, dtype=torch.float64, device="cuda")
    for j in range(taps):
        rows = stride * torch.arange(t_out, device="cuda") - pad + j
        ok = (rows >= 0) & (rows < t_in)
        xs = torch.zeros(b, t_out, 64, dtype=torch.float64, device="cuda")
        xs[:, ok] = xm[:, rows[ok]]
        ref[:, :, j] = torch.einsum("bto,bti->oi", dyr, xs)
    tol = 2e-6 * float(ref.abs().max()) * (b * t_out) ** 0.5 + 1e-4
    assert float((dw1.double() - ref).abs().max()) <= tol and float((dw0.double() - ref).abs().max()) <= tol
    dbr = dyr.sum((0, 1))
    tol_b = 2e-6 * float(dbr.abs().max()) * (b * t_out) ** 0.5 + 1e-3
    assert float((db1.double() - dbr).abs().max()) <= tol_b and float((db0.double() - dbr).abs().max()) <= tol_b
    if t_out >= 1000:                                       # one-hot dy: the gradient IS the shifted input rows
        hot = torch.zeros_like(dy)
        m = 777
        hot[1, m * os_ + oo, 5] = 1
        _, dwh, dbh = run(True, hot)
        for j in range(taps):
            r = stride * m - pad + j
            want = x[1, r].float() if r < int(lens[1]) else torch.zeros(64, device="cuda")
            assert torch.equal(dwh[5, :, j], want)
        assert float(dwh[:5].abs().max()) == 0 and float(dbh.sum()) == 1.0


WGRAD_DMA_CASES = [
    # b, t, c_in, c_out, k, dil, pad, lens
    (3, 700, 128, 128, 3, 1, 1, [700, 233, 1]),            # single-tile chunks; a partial last tile
    (3, 700, 128, 128, 9, 27, 108, [700, 233, 1]),         # two tap groups (5 + 4); halo wider than item 2's valid length
    (3, 50021, 128, 128, 4, 1, 1, [50021, 33333, 1]),      # three tiles per chunk: steady-state prefetch, last-tile drain
    (2, 3000, 256, 192, 3, 1, 1, None),                    # 2 x 3 blocks of (ci, co); the bias plane only in ci0 == 0
    (1, 1, 128, 128, 3, 1, 1, None),                       # one row
]


@pytest.mark.gpu
@pytest.mark.parametrize("b,t,c_in,c_out,k,dil,pad,lens", WGRAD_DMA_CASES)
def test_lds_dma_wgrad_matches_float64(b, t, c_in, c_out, k, dil, pad, lens):
    """conv_wgrad_dma_kernel (double-buffered LDS-DMA staging through range-checked descriptors, swizzled transposed
    fragments, tap groups of <= 5) against a float64 evaluation of the same bf16 operands.  Where lens are given the
    operands are channel slices of wider tensors.  An even tap count (k = 4, one output row fewer) keeps the long case off
    the shift kernel."""
    import ctypes
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(300 + 7 * k + t)
    t_out = t + 2 * pad - dil * (k - 1)
    if lens is not None:
        xb = torch.randn(b, t, c_in + 128, device="cuda", generator=g).to(torch.bfloat16)
        dyb = torch.randn(b, t_out, c_out + 256, device="cuda", generator=g).to(torch.bfloat16)
        x, dy = xb[:, :, 128:128 + c_in], dyb[:, :, 128:128 + c_out]
        lens = torch.tensor(lens, device="cuda", dtype=torch.int32)
    else:
        x = torch.randn(b, t, c_in, device="cuda", generator=g).to(torch.bfloat16)
        dy = torch.randn(b, t_out, c_out, device="cuda", generator=g).to(torch.bfloat16)
    dw, db = torch.empty(c_out, c_in, k, device="cuda"), torch.empty(c_out, device="cuda")
    d = C._base_desc(x, dy, lens, c_in, c_out, k, 1, dil, pad, t_out)
    C._wgrad(d, dw, c_in * k, k, 1, list(range(k)), db)      # sets the zero page
    torch.cuda.synchronize()
    assert C.N.lib().smt_conv1d_wgrad_kernel_name(ctypes.byref(d)).decode() == "conv_wgrad_dma"
    xm = x.double()
    if lens is not None:
        mask = (torch.arange(t, device="cuda")[None, :] < lens[:, None])[:, :, None]
        xm = torch.where(mask, xm, torch.zeros_like(xm))
    xp = torch.nn.functional.pad(xm, (0, 0, pad, pad))
    ref = torch.stack([torch.einsum("bto,bti->oi", dy.double(), xp[:, s * dil:s * dil + t_out]) for s in range(k)], dim=2)
    tol = 2e-6 * float(ref.abs().max()) * (b * t) ** 0.5 + 1e-4     # fp32 accumulation over b*t rows
    assert float((dw.double() - ref).abs().max()) <= tol
    dbr = dy.double().sum((0, 1))
    assert float((db.double() - dbr).abs().max()) <= 2e-6 * float(dbr.abs().max()) * (b * t) ** 0.5 + 1e-3


@pytest.mark.gpu
def test_full_size_linearity_of_the_dilated_conv_kernels():
    """BASELINE.json's full size of the top level (B = 32, T = 72,704, 128 channels, k = 9, dilation 27): scaling the
    input by a power of two scales a bias-free bf16 convolution and its weight gradient exactly (bit-for-bit), zero
    input gives exactly the bias, and the weight gradient of a one-hot-row dy picks out the shifted input rows."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(99)
    b, t, c, k, dil = 32, 72704, 128, 9, 27
    pad = (k - 1) * dil // 2
    x = torch.randn(b, t, c, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(c, c, k, device="cuda", generator=g) / (c * k) ** 0.5
    bias = torch.randn(c, device="cuda", generator=g)
    wp = C._pack_fwd(w, torch.bfloat16, True)

    def conv(inp, with_bias):
        y = torch.empty(b, t, c, device="cuda", dtype=torch.bfloat16)
        d = C._base_desc(inp, y, None, c, c, k, 1, dil, pad, t)
        C._use_dma(d, wp)
        d.bias = C._p(bias) if with_bias else None
        assert C._kernel_of(d) == "conv_ws"
        C._launch(d, "t")
        return y

    y1 = conv(x, False)
    y2 = conv(x * 2, False)
    assert torch.equal(y2, y1 * 2)                                     # exact: every product and sum doubles
    y0 = conv(torch.zeros_like(x), True)
    assert torch.equal(y0, bias.to(torch.bfloat16).expand(b, t, c))
    del y0, y2

    dy = torch.randn(b, t, c, device="cuda", generator=g).to(torch.bfloat16)

    def wgrad(inp, dout):
        dw, db = torch.empty(c, c, k, device="cuda"), torch.empty(c, device="cuda")
        C._wgrad(C._base_desc(inp, dout, None, c, c, k, 1, dil, pad, t), dw, c * k, k, 1, list(range(k)), db)
        return dw, db

    dw1, db1 = wgrad(x, dy)
    dw2, db2 = wgrad(x * 2, dy)
    assert torch.equal(dw2, dw1 * 2) and torch.equal(db2, db1)         # fp32 sums double exactly, db does not see x
    # one-hot dy (row t0 of batch 3, channel 5 = 1): dW[5, :, s] = x[3, t0 + s*dil - pad, :]
    t0 = 40000
    hot = torch.zeros_like(dy)
    hot[3, t0, 5] = 1
    dwh, dbh = wgrad(x, hot)
    torch.cuda.synchronize()
    for s in range(k):
        assert torch.equal(dwh[5, :, s], x[3, t0 + s * dil - pad].float())
    assert float(dwh[:5].abs().max()) == 0 and float(dwh[6:].abs().max()) == 0 and float(dbh.sum()) == 1.0


@pytest.mark.gpu
def test_full_size_properties_of_the_fused_backward_kernels():
    """Full top-level size (B = 32, T = 72,704): the fused K3 / K1 / gate backward kernels are linear in dy (a power-of-two
    scale goes through bit-for-bit), zero dy gives zero weight gradients and passes the residual through unchanged."""
    from smt_amd import convops as C
    g = torch.Generator(device="cuda").manual_seed(123)
    b, t = 32, 72704
    bf = torch.bfloat16
    # K3: 128 -> 128 behind relu+dropout
    dz = torch.randn(b, t, 128, device="cuda", generator=g).to(bf)
    u2 = torch.relu(torch.randn(b, t, 128, device="cuda", generator=g)).to(bf)
    w3 = torch.randn(128, 128, 1, device="cuda", generator=g) / 128 ** 0.5
    wb3 = C._pack_bwd(w3, bf, True)

    def k3(dzz):
        dx = torch.empty(b, t, 128, device="cuda", dtype=bf)
        d = C._dgrad_stride1(dzz, wb3, dx, 1, 1, 0)
        C._use_dma(d, wb3)
        C._set_act_grad(d, u2, 1.0)
        dw, db = torch.empty_like(w3), torch.empty(128, device="cuda")
        C._conv1x1_bwd(d, dw, 128, 1, db)
        return dx, dw, db

    dx1, dw1, db1 = k3(dz)
    dx2, dw2, db2 = k3(dz * 4)
    assert torch.equal(dx2, dx1 * 4) and torch.equal(dw2, dw1 * 4) and torch.equal(db2, db1 * 4)
    assert float((dx1.float().abs() * (u2 == 0)).max()) == 0                     # masked where the activation was off
    del dx1, dx2, dz
    # K1: 64 -> 512 with the block residual
    dh = torch.randn(b, t, 512, device="cuda", generator=g).to(bf)
    x = torch.randn(b, t, 64, device="cuda", generator=g).to(bf)
    res = torch.randn(b, t, 64, device="cuda", generator=g).to(bf)
    w1 = torch.randn(512, 64, 1, device="cuda", generator=g) / 8
    wb1 = C._pack_bwd(w1, bf)

    def k1(dhh):
        dx = torch.empty_like(x)
        dw, db = torch.empty_like(w1), torch.empty(512, device="cuda")
        C._conv_k1_bwd(dhh, x, wb1, res, dx, None, dw, db)
        return dx, dw, db

    dxa, dwa, dba = k1(dh)
    dxb, dwb, dbb = k1(dh * 2)
    assert torch.equal(dwb, dwa * 2) and torch.equal(dbb, dba * 2)
    dx0, dw0, db0 = k1(torch.zeros_like(dh))
    assert torch.equal(dx0, res) and float(dw0.abs().max()) == 0 and float(db0.abs().max()) == 0
    # gate: 64 -> 64
    dout = torch.randn(b, t, 64, device="cuda", generator=g).to(bf)
    gg = torch.randn(b, t, 64, device="cuda", generator=g).to(bf)
    wg = torch.randn(64, 64, 1, device="cuda", generator=g) / 8
    wbg = C._pack_bwd(wg, bf)

    def gate(dd):
        dx = torch.empty_like(gg)
        dw, db = torch.empty_like(wg), torch.empty(64, device="cuda")
        C._conv_gate_bwd(dd, gg, wbg, dx, None, dw, db)
        return dx, dw, db

    a, bq = gate(dout), gate(dout * 2)
    torch.cuda.synchronize()
    assert torch.equal(bq[0], a[0] * 2) and torch.equal(bq[1], a[1] * 2) and torch.equal(bq[2], a[2] * 2)


@pytest.mark.gpu
@pytest.mark.parametrize("c_wide", [64, 128])
def test_resampling_stream_kernels_match_the_generic_kernel(c_wide):
    """smt_conv4s2 / smt_convt4s2 (k = 4, stride 2, padding 1, width 64) against the generic implicit-GEMM launches they
    replace: forward and data gradient of the strided conv (c_wide -> 64) and of the transposed conv (64 -> c_wide),
    ragged lens, a length that is not a multiple of the 128-row tile, bias, bit-identical outputs."""
    resampling_stream_vs_generic(c_wide, 2 * 1237)


@pytest.mark.gpu
@pytest.mark.parametrize("c_wide", [64, 128])
def test_resampling_stream_kernels_at_three_tiles_per_workgroup(c_wide):
    """As above on 2 x 22001 input rows: 516 tiles on 256 workgroups, three tiles per workgroup -- the second reuse of a
    staging buffer, which the short case (one tile per workgroup) does not reach."""
    resampling_stream_vs_generic(c_wide, 2 * 22001)


def resampling_stream_vs_generic(c_wide, t):
    from smt_amd import convops as C
    from smt_amd import profiler
    g = torch.Generator(device="cuda").manual_seed(c_wide)
    b = 3
    lens = torch.tensor([t, t - 501, 64], device="cuda", dtype=torch.int32)
    x = torch.randn(b, t, c_wide, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(64, c_wide, 4, device="cuda", generator=g) / (c_wide * 4) ** 0.5
    bias = torch.randn(64, device="cuda", generator=g)
    xt = torch.randn(b, t // 2, 64, device="cuda", generator=g).to(torch.bfloat16)
    wt = torch.randn(64, c_wide, 4, device="cuda", generator=g) / 16
    bt = torch.randn(c_wide, device="cuda", generator=g)
    res = []
    for fast in (True, False):
        C._RESAMPLE = fast
        try:
            profiler.reset(); profiler.enable(True)
            xa, wa, ba = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
            y = C.conv1d(xa, wa, ba, stride=2, padding=1, lens=lens)
            y.backward(torch.ones_like(y) * 0.5 + y.detach() * 0.25)
            xb, wb, bb = xt.clone().requires_grad_(True), wt.clone().requires_grad_(True), bt.clone().requires_grad_(True)
            z = C.conv_transpose1d(xb, wb, bb, stride=2, padding=1, lens=(lens + 1) // 2)
            z.backward(torch.ones_like(z) * 0.5 + z.detach() * 0.25)
            names = {r["name"] for r in profiler.summary()}
            profiler.enable(False); profiler.reset()
        finally:
            C._RESAMPLE = True
        assert ({"conv4s2:fwd", "convt4s2:dgrad", "convt4s2:fwd", "conv4s2:dgrad"} <= names) == fast, sorted(names)
        res.append((y.detach(), xa.grad, wa.grad, z.detach(), xb.grad, wb.grad))
    for a, c in zip(*res):
        assert torch.equal(a, c)
