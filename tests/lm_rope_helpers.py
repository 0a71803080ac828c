"""Shared by tests/test_lm_rope_cpu.py, tests/test_lm_rope_kernels_gpu.py and tests/test_lm_rope_model_gpu.py: rotary positions
(model.position: rotary; include/smt_hip.h "Rotary positions") restated in float64 -- the rotation, the encoder layer and the
model with it -- plus the inputs and the assertion of the kernel tests, so that the CPU tests can show on those very inputs that
the assertion fails for each of the `mutate` variants.

    pair i of a head = channels (2i, 2i+1) of the q and k thirds of qkv [.., 3 H dh]; theta_i = base^(-2i/dh); a = p theta_i
    y[2i] = x[2i] cos a - x[2i+1] sin a,  y[2i+1] = x[2i] sin a + x[2i+1] cos a          (inverse: sin negated); v untouched

Error bound of the device rotation against this helper (u = 2^-24): a table entry is off by at most u/2, each of the two
products rounds once and the sum rounds once, so |y - y64| <= 4 u (|x[2i]| + |x[2i+1]|).
"""
import math

import torch
import torch.nn.functional as F

import lm_prenorm_helpers as H
from oracle import lm_oracle as lmo

U = 2.0 ** -24
MUTATIONS = ("half_split", "neg_sine", "pos_off_by_one", "theta_d_model", "v_rotated")
# the kernel tests' shapes: batch 2, 2 heads, rope_rows = pos0 + L exactly
KERNEL_B, KERNEL_H = 2, 2
KERNEL_CASES = [(L, dh, pos0) for dh in (32, 64) for L in (1, 5, 33) for pos0 in (0, 37)]


def angles64(positions, dh, base=10000.0, theta_dim=None):
    """a[p, i] = p * base^(-2i / dh) in float64; `theta_dim` replaces dh in the exponent (a mutation)."""
    i = torch.arange(dh // 2, dtype=torch.float64)
    theta = torch.pow(torch.tensor(float(base), dtype=torch.float64), -2.0 * i / (theta_dim or dh))
    return positions.double()[:, None] * theta[None, :]


def table64(rows, dh, base=10000.0):
    """What smt_amd.lm.rope_table must equal once rounded to fp32: (cos a, sin a) [rows, dh/2, 2] in float64."""
    a = angles64(torch.arange(rows), dh, base)
    return torch.stack([torch.cos(a), torch.sin(a)], dim=-1)


def rope64(qkv, heads, positions, base=10000.0, inverse=False, mutate=None):
    """qkv [..., L, 3 H dh] (any float dtype; computed in float64) with row l at position positions[l] -> rotated, float64."""
    assert mutate is None or mutate in MUTATIONS
    x = qkv.double()
    lead, l, d3 = x.shape[:-2], x.shape[-2], x.shape[-1]
    dh = d3 // (3 * heads)
    assert d3 == 3 * heads * dh and positions.shape == (l,)
    if mutate == "pos_off_by_one":
        positions = positions + 1
    a = angles64(positions, dh, base, theta_dim=heads * dh if mutate == "theta_d_model" else None)      # [L, dh/2]
    cos, sin = torch.cos(a)[:, None, None, :], torch.sin(a)[:, None, None, :]                              # over [L, 3, H, dh/2]
    if inverse != (mutate == "neg_sine"):
        sin = -sin
    x = x.reshape(*lead, l, 3, heads, dh)
    if mutate == "half_split":
        x0, x1 = x[..., :dh // 2], x[..., dh // 2:]
    else:
        x0, x1 = x[..., 0::2], x[..., 1::2]
    y0, y1 = x0 * cos - x1 * sin, x0 * sin + x1 * cos
    y = torch.cat([y0, y1], dim=-1) if mutate == "half_split" else torch.stack([y0, y1], dim=-1).reshape(x.shape)
    if mutate != "v_rotated":
        y = torch.cat([y[..., :2, :, :], x[..., 2:, :, :]], dim=-3)
    return y.reshape(*lead, l, d3)


def rope_bound(x, heads):
    """4 u (|x[2i]| + |x[2i+1]|) at both channels of every pair of the q and k thirds (float64, shape of x); 0 on the v third."""
    d3 = x.shape[-1]
    pairs = x.double().abs().reshape(*x.shape[:-1], d3 // 2, 2).sum(-1, keepdim=True).expand(*x.shape[:-1], d3 // 2, 2)
    bound = 4.0 * U * pairs.reshape(x.shape).clone()
    bound[..., 2 * d3 // 3:] = 0.0
    return bound


def assert_rope(got, x, heads, positions, base=10000.0, inverse=False):
    """THE assertion of the kernel tests: `got` (fp32) against rope64(x) within `rope_bound` on the q and k thirds, the v third
    equal to x's bit for bit.  Returns the worst |err| / bound."""
    d3 = x.shape[-1]
    want = rope64(x, heads, positions, base, inverse)
    err = (got.double() - want).abs()
    bound = rope_bound(x, heads)
    qk = slice(0, 2 * d3 // 3)
    ratio = float((err[..., qk] / bound[..., qk].clamp_min(1e-300)).max())
    assert bool((err[..., qk] <= bound[..., qk]).all()), f"rotation outside 4u(|x0| + |x1|): worst ratio {ratio:.3g}"
    assert torch.equal(got[..., 2 * d3 // 3:].float(), x[..., 2 * d3 // 3:].float()), "the v third changed"
    return ratio


def kernel_case(L, dh, pos0):
    """(x [2, L, 3 * 2 * dh] fp32, positions) of one kernel test case."""
    g = torch.Generator().manual_seed(1000 * L + 10 * dh + pos0)
    x = torch.randn(KERNEL_B, L, 3 * KERNEL_H * dh, generator=g)
    return x, torch.arange(pos0, pos0 + L)


# ------------------------------------------------------------------------------------------------ the model in float64
def encoder_layer(x, p, pre, lens, heads, causal, drop, site0, norm_first, activation, base, linear=F.linear, mutate=None, eps=1e-5):
    """lm_prenorm_helpers.encoder_layer with q and k rotated right after the in-projection, row l at position l."""
    d = x.shape[-1:]
    act = H.activation_fn(activation)
    positions = torch.arange(x.shape[1])

    def norm(t, which):
        return F.layer_norm(t, d, p[pre + which + ".weight"], p[pre + which + ".bias"], eps)

    def sa(t):
        qkv = linear(t, p[pre + "self_attn.in_proj_weight"], p[pre + "self_attn.in_proj_bias"])
        qkv = rope64(qkv, heads, positions, base, mutate=mutate).to(qkv.dtype)
        a = lmo.attention_core(qkv, lens, heads, causal, drop, site0)
        return drop(site0 + 1, linear(a, p[pre + "self_attn.out_proj.weight"], p[pre + "self_attn.out_proj.bias"]))

    def ff(t):
        f = drop(site0 + 2, act(linear(t, p[pre + "linear1.weight"], p[pre + "linear1.bias"])))
        return drop(site0 + 3, linear(f, p[pre + "linear2.weight"], p[pre + "linear2.bias"]))

    if norm_first:
        x = x + sa(norm(x, "norm1"))
        return x + ff(norm(x, "norm2"))
    x = norm(x + sa(x), "norm1")
    return norm(x + ff(x), "norm2")


def lm_logits(x, lens, p, heads, num_layers, norm_first=False, activation="relu", base=10000.0, final_eps=1e-5, causal=True, drop=None,
              linear=F.linear, mutate=None):
    """tokens [B, L] -> logits [B, L, vocab] of the rotary model: nothing is added to the scaled embedding."""
    drop = drop or lmo.CounterDropout()
    emb = p["embedding.weight"]
    d = emb.shape[1]
    h = drop(0, F.embedding(x, emb) * math.sqrt(d))
    for i in range(num_layers):
        h = encoder_layer(h, p, f"transformer.layers.{i}.", lens, heads, causal, drop, 1 + 4 * i, norm_first, activation, base, linear, mutate)
    h = F.layer_norm(h, (d,), p["transformer.norm.weight"], p["transformer.norm.bias"], final_eps)
    return linear(h, p["classifier.weight"], p["classifier.bias"])


def step64(x, lens, params, heads, num_layers, norm_first, activation, base=10000.0, drop=None, linear=F.linear):
    """(loss, accuracy, logits, {name: grad}) of the float64 rotary helper on float64 leaves made from `params`."""
    p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    logits = lm_logits(x, lens, p64, heads, num_layers, norm_first, activation, base, drop=drop, linear=linear)
    loss, acc = lmo.lm_loss(x, logits)
    loss.backward()
    return loss.detach(), acc.detach(), logits.detach(), {k: v.grad for k, v in p64.items()}
