"""Shared by tests/test_lm_attn_bf16_*.py: the attention core of the TransformerLM in float64, written out from the formulas of
include/smt_hip.h (smt_lm_attention_bf16_*), forward and backward, in two forms, and the a-priori error bound of the kernel tests.

With x^ = x rounded to bf16 (nearest even), ks = keep * drop_scale (1 without dropout), c = 1 / sqrt(32):

  exact     s = c q.k   P = softmax(s) over the visible keys   W = P ks   ctx = W v   lse = log2 sum_j 2^(s log2 e)
            dv = W^T dctx   dP = dctx v^T   delta = rowsum(dctx * ctx)   dS = P (ks dP - delta)   dq = c dS k   dk = c dS^T q
  rounded   s = c q^.k^   p~ = exp(s - rowmax)   z = sum_j p~ (unrounded)   ctx = (bf16(p~ ks) v^) / z
            P = p~ / z   dv = bf16(P ks)^T dctx^   dP = dctx^ v^^T   delta = rowsum(dctx * ctx) (unrounded dctx)
            dS = bf16(P (ks dP - delta))   dq = c dS k^   dk = c dS^T q^

`attention_exact` is the first (with `mutate`, broken on purpose in one of four ways), `RoundedAttention` the second as an
autograd.Function, and `oracle_attention` swaps it in for oracle.lm_oracle.attention_core the way
lm_bf16_helpers.oracle_linear swaps the oracle's linear.  The masks are oracle.lm_oracle.CounterDropout's.

The bound (`bounds`).  On bf16-representable q, k, v and dctx the operand roundings of the loads do nothing, the scores are
exact up to fp32 accumulation, and every output element is a contraction sum_j a_j b_j in which a_j (a weight p ks, or dS) is
rounded ONCE to bf16 and b_j (a value, key, query or dctx channel) is exact.  bf16 keeps 8 significant bits, so one rounding to
nearest moves a_j by 2^-10 .. 2^-9 of |a_j| on average and by at most 2^-8 / (1 + 2^-8) |a_j| (just above a power of two,
half way between two neighbours).  The bound is 2^-8 sum_j |a_j b_j|: at least twice the typical size of the rounding term,
and above its worst case by the factor 1 + 2^-8, i.e. by 2^-16 sum_j |a_j b_j|, which is what is left for the fp32 accumulation,
the fp32 rescales and the hardware exp2 (relative 2^-22 or so on p) when every rounding of an element falls on its worst case:
an element with ONE visible term (the last key of a causal row in dv, the first query in ctx) can therefore come within a
fraction of a percent of the bound, and elements with many terms stay well inside it.

  ctx_ic <= 2^-8 sum_j |W_ij v_jc|            dv_jc <= 2^-8 sum_i |W_ij dctx_ic|

dS carries one more error than its own rounding: delta_i = sum_c dctx_ic ctx_ic is formed from the DEVICE's context, which is off
by up to the context's own bound, so delta is off by up to D_i = sum_c |dctx_ic| bound_ctx_ic, dS_ij by P_ij D_i, and

  dq_ic <= c (2^-8 sum_j |dS_ij k_jc| + sum_j P_ij D_i |k_jc|)        dk_jc <= c (2^-8 sum_i |dS_ij q_ic| + sum_i P_ij D_i |q_ic|)

Everything on the right is computed from the exact form.  tests/test_lm_attn_bf16_cpu.py shows that the rounded form sits inside
the bound and that each mutation leaves it by more than a factor 10.
"""
import contextlib
import math

import torch

from oracle import lm_oracle as lmo

DH = 32
MUTATIONS = ("other_key", "v_shifted", "causal_off_by_one", "unscaled_ds")
LOG2E = 1.0 / math.log(2.0)


def bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def heads_of(t, heads):
    """[B, L, H * 32] -> [B, H, L, 32]"""
    b, l, d = t.shape
    return t.reshape(b, l, heads, d // heads).permute(0, 2, 1, 3)


def rows_of(t):
    """[B, H, L, 32] -> [B, L, H * 32]"""
    b, h, l, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, l, h * dh)


def split_qkv(qkv, heads):
    return tuple(heads_of(t, heads) for t in qkv.split(qkv.shape[-1] // 3, dim=-1))


def visible(batch, length, lens, causal, shift=0):
    """[B, 1, L, L] bool: key j visible to query i iff (j <= i + shift or not causal) and j < lens[b]."""
    i = torch.arange(length)
    vis = torch.ones(batch, 1, length, length, dtype=torch.bool)
    if causal:
        vis = vis & (i[None, :] <= i[:, None] + shift)[None, None]
    if lens is not None:
        vis = vis & (i[None, :] < lens.clamp(0, length)[:, None])[:, None, None, :]
    return vis


def keep_scale(drop, site, batch, heads, length, dtype=torch.float64):
    """keep * drop_scale of the attention-weight site as [B, H, L, L] (CounterDropout indexes the tensor row-major: element
    ((b H + h) L + i) L + j), or None for the identity."""
    if drop is None or drop.p <= 0.0:
        return None
    return drop(site, torch.ones(batch, heads, length, length, dtype=dtype))


def _softmax(s, vis):
    """(P, rowmax m, z): P = exp(s - m) / z over the visible keys, all-zero rows where nothing is visible."""
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    pt = torch.exp(s - m)
    z = pt.sum(-1, keepdim=True)
    return pt, m, z


def attention_exact(qkv, lens, heads, causal, ks=None, dctx=None, dctx_delta=None, mutate=None, ks_other=None):
    """Float64, no rounding.  Returns a dict: ctx [B, L, d], lse [B, H, L] in base 2 (0 where no key is visible), and with
    `dctx` also dqkv [B, L, 3 d] and the intermediates the bound needs.  `dctx_delta` (default dctx) is the gradient delta is
    formed from: the kernels take it from the unrounded dctx.  `mutate` breaks the result on purpose (`ks_other`: the
    keep * scale of another key, for "other_key")."""
    assert mutate is None or mutate in MUTATIONS
    qkv = qkv.double()
    b, l, _ = qkv.shape
    q, k, v = split_qkv(qkv, heads)
    c = 1.0 / math.sqrt(DH)
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
    out = dict(ctx=rows_of(ctx), lse=lse, p=p, w=w, q=q, k=k, v=v)
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
    """The a-priori bounds of the module docstring from the dict of `attention_exact` (with dctx): ctx [B, L, d], dqkv [B, L, 3 d]."""
    p, w, ds, q, k, v, g = (exact[n] for n in ("p", "w", "ds", "q", "k", "v", "g"))
    c, u = 1.0 / math.sqrt(DH), 2.0 ** -8
    b_ctx = u * (w.abs() @ v.abs())
    b_dv = u * (w.abs().transpose(-1, -2) @ g.abs())
    big_d = (g.abs() * b_ctx).sum(-1, keepdim=True)                     # D_i, [B, H, L, 1]
    pd = p * big_d
    b_dq = c * (u * (ds.abs() @ k.abs()) + pd @ k.abs())
    b_dk = c * (u * (ds.abs().transpose(-1, -2) @ q.abs()) + pd.transpose(-1, -2) @ q.abs())
    return rows_of(b_ctx), torch.cat([rows_of(b_dq), rows_of(b_dk), rows_of(b_dv)], dim=-1)


class RoundedAttention(torch.autograd.Function):
    """The rounded form of the module docstring, in the dtype of its input (float64 in the tests)."""

    @staticmethod
    def forward(ctx, qkv, lens, heads, causal, ks):
        b, l, _ = qkv.shape
        q, k, v = (bf16(t) for t in split_qkv(qkv, heads))
        ks = torch.ones(b, heads, l, l, dtype=qkv.dtype) if ks is None else ks.to(qkv.dtype)
        pt, _, z = _softmax((q @ k.transpose(-1, -2)) / math.sqrt(DH), visible(b, l, lens, causal))
        zc = z.clamp_min(1e-300)
        out = (bf16(pt * ks) @ v) / zc
        ctx.save_for_backward(q, k, v, pt / zc, ks, out)
        ctx.heads = heads
        return rows_of(out)

    @staticmethod
    def backward(ctx, dout):
        q, k, v, p, ks, out = ctx.saved_tensors
        g = heads_of(dout, ctx.heads)
        gb = bf16(g)
        delta = (g * out).sum(-1, keepdim=True)
        ds = bf16(p * (ks * (gb @ v.transpose(-1, -2)) - delta))
        c = 1.0 / math.sqrt(DH)
        dq, dk, dv = c * (ds @ k), c * (ds.transpose(-1, -2) @ q), bf16(p * ks).transpose(-1, -2) @ gb
        return torch.cat([rows_of(dq), rows_of(dk), rows_of(dv)], dim=-1), None, None, None, None


def rounded_core(qkv, lens, heads, causal, drop, site):
    """oracle.lm_oracle.attention_core with the rounding points of the bf16 kernels."""
    b, l, _ = qkv.shape
    return RoundedAttention.apply(qkv, lens, heads, causal, keep_scale(drop, site, b, heads, l, qkv.dtype))


@contextlib.contextmanager
def oracle_attention(rounded):
    """Inside the block oracle.lm_oracle.attention_core (which tests/lm_prenorm_helpers.py calls too) is `rounded_core`."""
    old = lmo.attention_core
    if rounded:
        lmo.attention_core = rounded_core
    try:
        yield
    finally:
        lmo.attention_core = old
