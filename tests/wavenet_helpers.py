"""Float64 restatement of the WaveNet block (reference models/vqvae/resnet.py:123-181), written from its formulas, and the
error bounds of the device kernels (derived in DESIGN.md section 20, not fitted).  Channels-last [B, T, C] throughout.

    x = conv_in(x * mask)                                   1x1, n_in -> H
    for d:  z = convs[d](x * mask)                          k = 3, dilation = padding = dil_d, H -> 2H
            a = tanh(z[..., :H]) * sigmoid(z[..., H:])
            x = x + gates[d](a * mask)                      1x1, H -> H
    x = conv_out(x * mask)                                  1x1, H -> n_in
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

# ---- bounds -------------------------------------------------------------------------------------------------------------
# fp32 gate over z in [-8, 8]: v_exp_f32 and v_rcp_f32 are 1 ulp (2^-23 relative) each, every fp32
# operation rounds by 2^-24 relative.  Forward: 1.2 (argument and exp of E through tanh) + 0.6 (the same of S through sigmoid)
# + 5 roundings + 2 (one reciprocal) = 8.8 units of 2^-24 on a value of at most 1, stated as 16.  Backward: 20 units, stated
# as 32.  The issue's condition: neither may exceed 2^-18.
E_F = 16 * 2.0 ** -24
E_B = 32 * 2.0 ** -24
assert E_F <= 2.0 ** -18 and E_B <= 2.0 ** -18
GATE_DOMAIN = 8.0
BF16_OUT_REL = 2.0 ** -8           # a value rounded once to bf16: half an ulp (2^-8 of its binade) is at most 2^-8 of the value
BF16_GATE_REL = 2.0 ** -7          # that rounding plus one bf16 ulp for the functions and a double rounding
# bf16 gate backward: |dz - dz64| <= BF16_OUT_REL |dz64| + E_B |da|.  The fp32 value is within 20 * 2^-24 |da| of dz64 (above);
# rounding it to bf16 adds at most 2^-8 of |dz64| + 20 * 2^-24 |da|; the sum stays below 2^-8 |dz64| + 32 * 2^-24 |da|.
# A purely relative bound cannot hold here: 1 - tanh^2 cancels for large |t|, so the fp32 error is absolute.


def det_uniform(name, shape):
    """float32 array of `shape`, uniform in (-b, b), a closed-form function of (name, index): splitmix64 of the index offset by
    crc32(name).  b = 1 / sqrt(fan_in) for a convolution weight (half of it for a WaveNet gate, so that the residual stack
    stays O(1)), 0.05 for every other tensor.  Both the fixture generator and the test evaluate it; no file carries the values."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64(zlib.crc32(name.encode()) << 32) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    u = (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    bound = 0.05
    if len(shape) == 3:
        bound = (0.5 if ".gates." in name else 1.0) / np.sqrt(shape[1] * shape[2])
    return ((2.0 * u - 1.0) * bound).astype(np.float32).reshape(shape)


def row_mask(lens, t):
    """[B, T, 1] float64 prefix mask t < lens[b]."""
    return (torch.arange(t)[None, :] < torch.as_tensor(lens)[:, None]).double().unsqueeze(-1)


# ---- gate, its derivative, the tail ---------------------------------------------------------------------------------------
def gate64(z):
    h = z.shape[-1] // 2
    z = z.double()
    return torch.tanh(z[..., :h]) * torch.sigmoid(z[..., h:])


def gate_grad64(z, da):
    h = z.shape[-1] // 2
    z, da = z.double(), da.double()
    th, sg = torch.tanh(z[..., :h]), torch.sigmoid(z[..., h:])
    return torch.cat([da * sg * (1 - th * th), da * th * sg * (1 - sg)], dim=-1)


def tail64(z, x, weight, bias):
    """(y, s): y = x + bias + W_g . gate(z), s = sum_i |W_g[o, i]| |a_i| (the scale of the tail's operand and accumulation
    error).  weight is [H, H, 1] or [H, H]."""
    w = weight.double().reshape(weight.shape[0], weight.shape[1])
    a = gate64(z)
    y = x.double() + a @ w.t()
    if bias is not None:
        y = y + bias.double()
    return y, a.abs() @ w.abs().t()


def tail_bound(y64, s, hidden):
    """|y - y64| <= 2^-8 |y64| + (2^-7 + H 2^-24) sum_i |W_g,i| |a64,i|: output rounding, the bf16 operand a, fp32 accumulation."""
    return BF16_OUT_REL * y64.abs() + (BF16_GATE_REL + hidden * 2.0 ** -24) * s


# ---- the block ----------------------------------------------------------------------------------------------------------------
def conv64(x, weight, bias, dilation=1, padding=0):
    return F.conv1d(x.transpose(1, 2), weight, bias, dilation=dilation, padding=padding).transpose(1, 2)


def block64(x, lens, params, dilations):
    """x [B, T, n_in] float64; params: the block's state dict (float64 tensors, torch layouts).  Every convolution reads its
    input times the mask, so rows at or past lens[b] hold biases, as in the reference; callers compare valid rows."""
    m = row_mask(lens, x.shape[1])
    x = conv64(x * m, params["conv_in.weight"], params["conv_in.bias"])
    for d, dil in enumerate(dilations):
        z = conv64(x * m, params[f"convs.{d}.weight"], params[f"convs.{d}.bias"], dil, dil)
        x = x + conv64(gate64(z) * m, params[f"gates.{d}.weight"], params[f"gates.{d}.bias"])
    return conv64(x * m, params["conv_out.weight"], params["conv_out.bias"])


def block_dilations(n_depth, growth, cycle):
    return [growth ** (d if cycle is None else d % cycle) for d in range(n_depth)]


def rel_l2(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()
