"""gate_mix (sum over the branches of tanh(t_d) softmax_d(s_d), GatedHiFiBlock) at branch counts and widths whose backward
cannot exchange its softmax statistics between lanes -- a depth that is no power of two (VQTTS runs three branches), or
more than 64 lanes per row -- and therefore runs the kernel that holds all branches in one lane.  Same reference and
tolerances as tests/test_conv_gpu.py::test_gate_mix, which covers the four-branch geometry."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def tol(dtype):
    return dict(f=2e-5, g=2e-4) if dtype == torch.float32 else dict(f=1.5e-2, g=3e-2)


def close(a, b, rel):
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() <= rel * b.abs().max().item() + 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("w,depth", [(64, 3), (32, 3), (8, 5), (128, 4), (16, 1), (64, 8)])
def test_gate_mix_any_depth(w, depth, dtype):
    from smt_amd import convops
    g = torch.Generator(device="cuda").manual_seed(10 * w + depth)
    b, t = 2, 157
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
    assert bool(torch.isfinite(za.grad).all())
