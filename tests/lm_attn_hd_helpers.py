"""Shared by tests/test_lm_attn_hd64_*.py and tests/test_lm_hd64_model_gpu.py: `attention_exact`, `bounds` and `RoundedAttention`
of tests/lm_attn_bf16_helpers.py with the head dim read from the tensors (dh = d / heads) instead of that module's DH = 32.

The formulas, the rounding points and the derivation of the bound are that module's docstring with c = 1 / sqrt(dh): nothing in
the derivation uses the number of channels (every output element is still a contraction with ONE rounded factor per term, and
the scores are exact products accumulated in fp32 whether they have 32 or 64 terms).  The pieces that never depended on the
head dim are imported from there; tests/test_lm_attn_hd64_cpu.py shows that at dh = 32 `attention_exact` here is that module's.
"""
import contextlib
import math

import torch

import lm_attn_bf16_helpers as A32
from lm_attn_bf16_helpers import LOG2E, MUTATIONS, _softmax, bf16, heads_of, keep_scale, rows_of, split_qkv, visible   # noqa: F401
from oracle import lm_oracle as lmo


def head_dim(qkv, heads):
    d3 = qkv.shape[-1]
    assert d3 % (3 * heads) == 0
    return d3 // (3 * heads)


def attention_exact(qkv, lens, heads, causal, ks=None, dctx=None, dctx_delta=None, mutate=None, ks_other=None):
    """lm_attn_bf16_helpers.attention_exact at head dim qkv.shape[-1] / (3 heads); the dict also holds "dh"."""
    assert mutate is None or mutate in MUTATIONS
    qkv = qkv.double()
    b, l, _ = qkv.shape
    dh = head_dim(qkv, heads)
    q, k, v = split_qkv(qkv, heads)
    c = 1.0 / math.sqrt(dh)
    vis = visible(b, l, lens, causal, shift=1 if mutate == "causal_off_by_one" else 0)
    if mutate == "other_key":
        ks = ks_other
    if mutate == "v_shifted":
        v = torch.roll(v, 1, dims=2)
    ks = torch.ones(b, heads, l, l, dtype=torch.float64) if ks is None else ks.double()
    pt, m, z = _softmax(c * (q @ k.transpose(-1, -2)), vis)
    any_vis = z > 0
    p = pt / z.clamp_min(1e-300)
    w = p * ks
    ctx = w @ v
    lse = torch.where(any_vis, (m + torch.log(z.clamp_min(1e-300))) * LOG2E, torch.zeros_like(m)).squeeze(-1)
    out = dict(ctx=rows_of(ctx), lse=lse, p=p, w=w, q=q, k=k, v=v, dh=dh)
    if dctx is None:
        return out
    g = heads_of(dctx.double(), heads)
    gd = g if dctx_delta is None else heads_of(dctx_delta.double(), heads)
    delta = (gd * ctx).sum(-1, keepdim=True)
    ds = p * (ks * (g @ v.transpose(-1, -2)) - delta)
    cs = 1.0 if mutate == "unscaled_ds" else c
    dq, dk, dv = cs * (ds @ k), cs * (ds.transpose(-1, -2) @ q), w.transpose(-1, -2) @ g
    out.update(dqkv=torch.cat([rows_of(dq), rows_of(dk), rows_of(dv)], dim=-1), ds=ds, g=g)
    return out


def bounds(exact):
    """The a-priori bounds of lm_attn_bf16_helpers' docstring, c = 1 / sqrt(dh): ctx [B, L, d], dqkv [B, L, 3 d]."""
    p, w, ds, q, k, v, g = (exact[n] for n in ("p", "w", "ds", "q", "k", "v", "g"))
    c, u = 1.0 / math.sqrt(exact["dh"]), 2.0 ** -8
    b_ctx = u * (w.abs() @ v.abs())
    b_dv = u * (w.abs().transpose(-1, -2) @ g.abs())
    big_d = (g.abs() * b_ctx).sum(-1, keepdim=True)                     # D_i, [B, H, L, 1]
    pd = p * big_d
    b_dq = c * (u * (ds.abs() @ k.abs()) + pd @ k.abs())
    b_dk = c * (u * (ds.abs().transpose(-1, -2) @ q.abs()) + pd.transpose(-1, -2) @ q.abs())
    return rows_of(b_ctx), torch.cat([rows_of(b_dq), rows_of(b_dk), rows_of(b_dv)], dim=-1)


class RoundedAttention(torch.autograd.Function):
    """lm_attn_bf16_helpers.RoundedAttention at head dim qkv.shape[-1] / (3 heads), in the dtype of its input."""

    @staticmethod
    def forward(ctx, qkv, lens, heads, causal, ks):
        b, l, _ = qkv.shape
        dh = head_dim(qkv, heads)
        q, k, v = (bf16(t) for t in split_qkv(qkv, heads))
        ks = torch.ones(b, heads, l, l, dtype=qkv.dtype) if ks is None else ks.to(qkv.dtype)
        pt, _, z = _softmax((q @ k.transpose(-1, -2)) / math.sqrt(dh), visible(b, l, lens, causal))
        zc = z.clamp_min(1e-300)
        out = (bf16(pt * ks) @ v) / zc
        ctx.save_for_backward(q, k, v, pt / zc, ks, out)
        ctx.heads, ctx.dh = heads, dh
        return rows_of(out)

    @staticmethod
    def backward(ctx, dout):
        q, k, v, p, ks, out = ctx.saved_tensors
        g = heads_of(dout, ctx.heads)
        gb = bf16(g)
        delta = (g * out).sum(-1, keepdim=True)
        ds = bf16(p * (ks * (gb @ v.transpose(-1, -2)) - delta))
        c = 1.0 / math.sqrt(ctx.dh)
        dq, dk, dv = c * (ds @ k), c * (ds.transpose(-1, -2) @ q), bf16(p * ks).transpose(-1, -2) @ gb
        return torch.cat([rows_of(dq), rows_of(dk), rows_of(dv)], dim=-1), None, None, None, None


def rounded_core(qkv, lens, heads, causal, drop, site):
    """oracle.lm_oracle.attention_core with the rounding points of the bf16 kernels, at any head dim."""
    b, l, _ = qkv.shape
    return RoundedAttention.apply(qkv, lens, heads, causal, keep_scale(drop, site, b, heads, l, qkv.dtype))


@contextlib.contextmanager
def oracle_attention(rounded):
    """Inside the block oracle.lm_oracle.attention_core is `rounded_core` (restored on the way out)."""
    old = lmo.attention_core
    if rounded:
        lmo.attention_core = rounded_core
    try:
        yield
    finally:
        lmo.attention_core = old
