"""Autograd bindings of the TransformerLM kernels (csrc/lm.hip, include/smt_hip.h "TransformerLM").

Everything between the dense projections of the reference's nn.TransformerEncoder stack
(models/transformer_lm/transformer_lm.py:54-66) runs in these kernels; the projections themselves go through ``linear``
below: library GEMMs (torch.nn.functional.linear -> hipBLASLt) in fp32, csrc/lm_linear.hip with bf16 operands.  Activations are [batch, len, dim] fp32; dropout masks come from the
counter-based generator (smt_hip.h "dropout") keyed per (step seed, site), so backward recomputes them instead of
storing a mask per site.  The post-norm ReLU stack of the reference uses ``add_layer_norm`` and ``bias_relu_dropout_``;
``residual_layer_norm`` (a residual add fused with the LayerNorm that follows it) and ``bias_gelu_dropout`` serve
``norm_first`` and ``activation="gelu"`` of nn.TransformerEncoderLayer.
"""
import math

import ctypes

import torch
import torch.nn.functional as F

from . import native as N
from . import packing
from . import profiler
from .convops import dropout_key


class Drop:
    """(key, thresh16, scale) of one dropout site; p = 0 or eval -> identity.  ``keys_dev`` (a device uint32/int32 tensor
    of per-site keys written by ``make_keys``) makes the kernels read the key from device memory instead of taking it by
    value: what a captured graph needs, since replays cannot change by-value arguments."""
    __slots__ = ("key", "thresh", "scale", "key_dev")

    def __init__(self, p=0.0, training=False, seed=0, site=0, keys_dev=None):
        self.key_dev = None
        if training and p > 0.0:
            self.key, self.thresh, self.scale = dropout_key(seed, site), int(round(p * 65536.0)), 1.0 / (1.0 - p)
            if keys_dev is not None:
                self.key_dev = keys_dev[site:site + 1]
        else:
            self.key, self.thresh, self.scale = 0, 0, 1.0


def make_keys(seed_dev, keys_dev):
    """keys_dev[s] = dropout_key(seed_dev[0], s) computed on the device (smt_lm_make_keys)."""
    assert seed_dev.is_cuda and keys_dev.is_cuda and seed_dev.dtype == torch.int32 and keys_dev.dtype == torch.int32
    N.check(N.lib().smt_lm_make_keys(N.ptr(seed_dev), N.ptr(keys_dev), keys_dev.numel(), N.stream_ptr()), "smt_lm_make_keys")


NO_DROP = Drop()


def _f32(t):
    assert t.dtype == torch.float32 and t.is_cuda, "TransformerLM kernels take fp32 device tensors"
    return t.contiguous()


class _Embed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tokens, weight, pe, mul, drop, padding_idx):
        b, l = tokens.shape
        d = weight.shape[1]
        tokens = tokens.contiguous()
        out = torch.empty(b, l, d, device=weight.device, dtype=torch.float32)
        N.check(N.lib().smt_lm_embed_fwd(N.ptr(tokens), N.ptr(_f32(weight)), N.ptr(_f32(pe)), N.ptr(out), b, l, d, mul, drop.key, N.ptr(drop.key_dev),
                                         drop.thresh, drop.scale, N.stream_ptr()), "smt_lm_embed_fwd")
        ctx.save_for_backward(tokens)
        ctx.meta = (weight.shape[0], d, mul, drop, padding_idx)
        return out

    @staticmethod
    def backward(ctx, dout):
        (tokens,) = ctx.saved_tensors
        rows, d, mul, drop, padding_idx = ctx.meta
        b, l = tokens.shape
        demb = torch.empty(rows, d, device=dout.device, dtype=torch.float32)
        N.check(N.lib().smt_lm_embed_bwd(N.ptr(tokens), N.ptr(_f32(dout)), N.ptr(demb), b, l, d, rows, mul, drop.key, N.ptr(drop.key_dev), drop.thresh,
                                         drop.scale, padding_idx, N.stream_ptr()), "smt_lm_embed_bwd")
        return None, demb, None, None, None, None


def embed(tokens, weight, pe, drop=NO_DROP, padding_idx=0):
    """dropout(weight[tokens] * sqrt(dim) + pe[:len])  (transformer_lm.py:114-116, :27-29); tokens [batch, len] int64."""
    assert tokens.dtype == torch.int64 and pe.shape[0] >= tokens.shape[1] and pe.shape[-1] == weight.shape[1]
    return _Embed.apply(tokens, weight, pe, math.sqrt(weight.shape[1]), drop, padding_idx)


def _attn_flops(b, heads, l, causal, matmuls, head_dim=32):
    """Algorithmic FLOPs of `matmuls` head_dim-channel products over the visible (query, key) pairs (full lengths):
    forward 2 (scores, context), backward 5 (scores, dP, dq, dk, dv; the two backward kernels each recompute scores and
    dP, which is not counted)."""
    pairs = l * (l + 1) // 2 if causal else l * l
    return b * heads * pairs * 2 * head_dim * matmuls


HEAD_DIMS = (32, 64)          # what the attention kernels (csrc/lm.hip, csrc/lm_decode.hip) are built for


def _head_dim(dim, heads):
    dh = dim // heads if heads > 0 else 0
    assert dh in HEAD_DIMS and dim == heads * dh, \
        f"the attention kernels are built for head dim 32 or 64 (got {dim / heads if heads > 0 else dim:g})"
    return dh


# compute_dtype of `attention` -> (bf16 flag of smt_lm_attention_hd_fwd / _bwd, profiler region, profiler dtype)
_ATTN_ENTRIES = {torch.float32: (0, "lm_attention", "f32"), torch.bfloat16: (1, "lm_attention_bf16", "bf16")}


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, lens, heads, causal, drop, compute_dtype=torch.float32):
        bf16, region, dtype = _ATTN_ENTRIES[compute_dtype]
        b, l, d3 = qkv.shape
        d = d3 // 3
        dh = _head_dim(d, heads)
        qkv = _f32(qkv)
        out = torch.empty(b, l, d, device=qkv.device, dtype=torch.float32)
        lse = torch.empty(b, heads, l, device=qkv.device, dtype=torch.float32)
        with profiler.region(region + ":fwd", flops=_attn_flops(b, heads, l, causal, 2, dh), bound="mfma", dtype=dtype):
            N.check(N.lib().smt_lm_attention_hd_fwd(N.ptr(qkv), N.ptr(lens), N.ptr(out), N.ptr(lse), b, l, heads, int(causal),
                                                    drop.key, N.ptr(drop.key_dev), drop.thresh, drop.scale, dh, bf16, N.stream_ptr()),
                    "smt_lm_attention_hd_fwd")
        ctx.save_for_backward(qkv, lens, out, lse)
        ctx.meta = (heads, int(causal), drop, compute_dtype, dh)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, lens, out, lse = ctx.saved_tensors
        heads, causal, drop, compute_dtype, dh = ctx.meta
        bf16, region, dtype = _ATTN_ENTRIES[compute_dtype]
        b, l, _ = qkv.shape
        dqkv = torch.empty_like(qkv)
        delta = torch.empty_like(lse)
        dout = _f32(dout)
        with profiler.region(region + ":bwd", flops=_attn_flops(b, heads, l, causal, 5, dh), bound="mfma", dtype=dtype):
            N.check(N.lib().smt_lm_attention_hd_bwd(N.ptr(qkv), N.ptr(lens), N.ptr(out), N.ptr(lse), N.ptr(dout), N.ptr(dqkv),
                                                    N.ptr(delta), b, l, heads, causal, drop.key, N.ptr(drop.key_dev), drop.thresh,
                                                    drop.scale, dh, bf16, N.stream_ptr()), "smt_lm_attention_hd_bwd")
        return dqkv, None, None, None, None, None


def attention(qkv, lens, heads, causal=True, drop=NO_DROP, *, compute_dtype=torch.float32):
    """Self-attention core: qkv [batch, len, 3 dim] -> [batch, len, dim], head dim dim / heads = 32 or 64 (anything else
    is an AssertionError); lens [batch] int32 (keys >= lens[b] masked) or None; causal adds the triu(-inf, 1) mask of the reference's forward (:111).  compute_dtype is the operand type of the
    products: torch.float32, or torch.bfloat16 for the kernels on bf16 MFMAs (smt_lm_attention_hd_*, bf16 = 1: tensors stay fp32,
    the rounding points are listed in include/smt_hip.h)."""
    if compute_dtype not in _ATTN_ENTRIES:
        raise ValueError(f"attention: compute_dtype must be torch.float32 or torch.bfloat16 (got {compute_dtype!r})")
    if lens is not None:
        assert lens.dtype == torch.int32 and lens.is_cuda
    return _Attention.apply(qkv, lens, heads, causal, drop, compute_dtype)


# ------------------------------------------------------------------------------------------------ rotary positions
# csrc/lm_rope.hip, include/smt_hip.h "Rotary positions".
def rope_table(rows, head_dim, base=10000.0, device="cpu"):
    """The (cos a, sin a) table [rows, head_dim / 2, 2] fp32 of the rotary rotation: a = p * theta_i, theta_i = base^(-2 i / head_dim),
    for positions p = 0..rows-1 and pairs i = 0..head_dim/2-1, computed on the host in float64 and rounded once."""
    assert head_dim in HEAD_DIMS, f"the attention kernels are built for head dim 32 or 64 (got {head_dim})"
    base = float(base)
    if not (math.isfinite(base) and base > 1.0):
        raise ValueError(f"rope_table: base must be a finite number > 1 (got {base!r})")
    i = torch.arange(head_dim // 2, dtype=torch.float64)
    theta = torch.pow(torch.tensor(base, dtype=torch.float64), -2.0 * i / head_dim)
    a = torch.arange(rows, dtype=torch.float64)[:, None] * theta[None, :]
    return torch.stack([torch.cos(a), torch.sin(a)], dim=-1).to(torch.float32).to(device)


def _rope_launch(qkv, table, heads, pos0, inverse):
    b, l, d3 = qkv.shape
    dh = _head_dim(d3 // 3, heads)
    assert d3 == 3 * heads * dh and table.dim() == 3 and table.shape[1:] == (dh // 2, 2), \
        f"rope: the table must be [rows, {dh // 2}, 2] for head dim {dh} (got {tuple(table.shape)})"
    assert table.dtype == torch.float32 and table.is_cuda and table.is_contiguous()
    with profiler.region("lm_rope:bwd" if inverse else "lm_rope:fwd", nbytes=2 * b * l * 2 * heads * dh * 4, bound="hbm"):
        N.check(N.lib().smt_lm_rope(N.ptr(qkv), N.ptr(table), b, l, heads, dh, table.shape[0], int(pos0), int(inverse), N.stream_ptr()),
                "smt_lm_rope")


class _Rope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, table, heads, pos0):
        assert qkv.dtype == torch.float32 and qkv.is_cuda and qkv.dim() == 3 and qkv.is_contiguous(), \
            "rope rotates a contiguous fp32 device tensor [batch, len, 3 dim] in place"
        _rope_launch(qkv, table, heads, pos0, False)
        ctx.mark_dirty(qkv)
        ctx.save_for_backward(table)
        ctx.meta = (heads, pos0)
        return qkv

    @staticmethod
    def backward(ctx, dout):
        (table,) = ctx.saved_tensors
        heads, pos0 = ctx.meta
        # an incoming gradient is not ours to modify: the inverse rotation runs in place on a copy, whose v third is the pass-through
        dqkv = dout.clone(memory_format=torch.contiguous_format)
        _rope_launch(dqkv, table, heads, pos0, True)
        return dqkv, None, None, None


def rope(qkv, table, heads, pos0=0):
    """Rotary positions, IN PLACE: the q and k thirds of qkv [batch, len, 3 dim] (contiguous fp32, the output of the
    in-projection) rotated pair by pair -- channels (2i, 2i+1) of every head by the angle of `table` row pos0 + l (`rope_table`);
    the v third is not touched.  Returns qkv.  Backward: the inverse rotation of the gradient's q and k thirds, v passed through.
    The projection that produced qkv must not need its own output for its backward (F.linear and `linear` below do not)."""
    return _Rope.apply(qkv, table, heads, pos0)


class _AddLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h, h_bias, gamma, beta, eps, drop):
        src = x if x is not None else h
        d = src.shape[-1]
        rows = src.numel() // d
        x = _f32(x) if x is not None else None
        h = _f32(h) if h is not None else None
        y = torch.empty_like(src, memory_format=torch.contiguous_format)
        stats = torch.empty(rows, 2, device=src.device, dtype=torch.float32)
        n_in = (x is not None) + (h is not None)
        with profiler.region("lm_add_ln:fwd", nbytes=(n_in + 1) * rows * d * 4, bound="hbm"):
            N.check(N.lib().smt_lm_add_ln_fwd(N.ptr(x), N.ptr(h), N.ptr(h_bias), N.ptr(_f32(gamma)), N.ptr(_f32(beta)), N.ptr(y),
                                              N.ptr(stats), rows, d, eps, drop.key, N.ptr(drop.key_dev), drop.thresh, drop.scale, N.stream_ptr()),
                    "smt_lm_add_ln_fwd")
        ctx.save_for_backward(x, h, h_bias, gamma, stats)
        ctx.meta = (rows, d, drop)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h, h_bias, gamma, stats = ctx.saved_tensors
        rows, d, drop = ctx.meta
        lib = N.lib()
        dy = _f32(dy)
        dx = torch.empty_like(dy) if x is not None and ctx.needs_input_grad[0] else None
        dh = torch.empty_like(dy) if h is not None and ctx.needs_input_grad[1] else None
        dparams = torch.empty(3, d, device=dy.device, dtype=torch.float32)
        ws_bytes = lib.smt_lm_add_ln_bwd_workspace_bytes(rows, d)
        ws = torch.empty(ws_bytes, device=dy.device, dtype=torch.uint8)
        n_io = 1 + (x is not None) + (h is not None) + (dx is not None) + (dh is not None)
        with profiler.region("lm_add_ln:bwd", nbytes=n_io * rows * d * 4, bound="hbm"):
            N.check(lib.smt_lm_add_ln_bwd(N.ptr(x), N.ptr(h), N.ptr(h_bias), N.ptr(dy), N.ptr(_f32(gamma)), N.ptr(stats), N.ptr(dx),
                                          N.ptr(dh), N.ptr(dparams), rows, d, drop.key, N.ptr(drop.key_dev), drop.thresh, drop.scale, N.ptr(ws),
                                          ws_bytes, N.stream_ptr()), "smt_lm_add_ln_bwd")
        return dx, dh, (dparams[2] if h_bias is not None else None), dparams[0], dparams[1], None, None


def add_layer_norm(x, h, gamma, beta, eps=1e-5, drop=NO_DROP, h_bias=None):
    """LayerNorm(x + dropout(h + h_bias)) (post-norm sub-layer of nn.TransformerEncoderLayer; h_bias = the bias of the
    projection that produced h, whose gradient then comes out of this op's backward); h = None -> LayerNorm(x)."""
    assert h_bias is None or (h is not None and h_bias.dtype == torch.float32 and h_bias.is_contiguous())
    return _AddLayerNorm.apply(x, h, h_bias, gamma, beta, eps, drop)


class _ResidualLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h, h_bias, gamma, beta, eps, drop):
        d = x.shape[-1]
        rows = x.numel() // d
        x, h = _f32(x), _f32(h)
        s = torch.empty_like(x)
        y = torch.empty_like(x)
        stats = torch.empty(rows, 2, device=x.device, dtype=torch.float32)
        with profiler.region("lm_res_ln:fwd", nbytes=4 * rows * d * 4, bound="hbm"):
            N.check(N.lib().smt_lm_res_ln_fwd(N.ptr(x), N.ptr(h), N.ptr(h_bias), N.ptr(_f32(gamma)), N.ptr(_f32(beta)), N.ptr(s), N.ptr(y),
                                              N.ptr(stats), rows, d, eps, drop.key, N.ptr(drop.key_dev), drop.thresh, drop.scale, N.stream_ptr()),
                    "smt_lm_res_ln_fwd")
        ctx.save_for_backward(s, gamma, stats)
        ctx.meta = (rows, d, drop, h_bias is not None)
        ctx.set_materialize_grads(False)                        # an unused output's gradient arrives as None, not as zeros
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        s, gamma, stats = ctx.saved_tensors
        rows, d, drop, with_bias = ctx.meta
        lib = N.lib()
        ds = _f32(ds) if ds is not None else None
        dy = _f32(dy) if dy is not None else None
        dx = torch.empty_like(s) if ctx.needs_input_grad[0] else None
        dh = torch.empty_like(s) if ctx.needs_input_grad[1] else None
        dparams = torch.empty(3, d, device=s.device, dtype=torch.float32)
        ws_bytes = lib.smt_lm_res_ln_bwd_workspace_bytes(rows, d)
        ws = torch.empty(ws_bytes, device=s.device, dtype=torch.uint8)
        n_io = (ds is not None) + 2 * (dy is not None) + (dx is not None) + (dh is not None)
        with profiler.region("lm_res_ln:bwd", nbytes=n_io * rows * d * 4, bound="hbm"):
            N.check(lib.smt_lm_res_ln_bwd(N.ptr(s), N.ptr(ds), N.ptr(dy), N.ptr(_f32(gamma)), N.ptr(stats), N.ptr(dx), N.ptr(dh),
                                          N.ptr(dparams), rows, d, drop.key, N.ptr(drop.key_dev), drop.thresh, drop.scale, N.ptr(ws),
                                          ws_bytes, N.stream_ptr()), "smt_lm_res_ln_bwd")
        return dx, dh, (dparams[2] if with_bias else None), dparams[0], dparams[1], None, None


def residual_layer_norm(x, h, gamma, beta, eps=1e-5, drop=NO_DROP, h_bias=None):
    """The residual step of a pre-norm layer: (s, y) with s = x + dropout(h + h_bias), the new residual stream, and
    y = LayerNorm(s) * gamma + beta, the input of the next projection (gamma / beta / eps of the NEXT norm: the layer's norm2,
    the next layer's norm1 or the encoder's final norm).  h_bias as in `add_layer_norm`.  Either output may go unused: its
    gradient then counts as zero."""
    assert x.shape == h.shape and (h_bias is None or (h_bias.dtype == torch.float32 and h_bias.is_contiguous()))
    return _ResidualLayerNorm.apply(x, h, h_bias, gamma, beta, eps, drop)


class _BiasGeluDrop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, bias, drop):
        d = h.shape[-1]
        rows = h.numel() // d
        h, bias = _f32(h), _f32(bias)
        a = torch.empty_like(h)
        with profiler.region("lm_bias_gelu:fwd", nbytes=2 * rows * d * 4, bound="hbm"):
            N.check(N.lib().smt_lm_bias_gelu_fwd(N.ptr(h), N.ptr(bias), N.ptr(a), rows, d, drop.key, N.ptr(drop.key_dev), drop.thresh,
                                                 drop.scale, N.stream_ptr()), "smt_lm_bias_gelu_fwd")
        ctx.save_for_backward(h, bias)
        ctx.meta = (rows, d, drop)
        return a

    @staticmethod
    def backward(ctx, da):
        h, bias = ctx.saved_tensors
        rows, d, drop = ctx.meta
        lib = N.lib()
        da = _f32(da)
        dh = torch.empty_like(h)
        dbias = torch.empty(d, device=h.device, dtype=torch.float32)
        ws_bytes = lib.smt_lm_bias_gelu_bwd_workspace_bytes(rows, d)
        ws = torch.empty(ws_bytes, device=h.device, dtype=torch.uint8)
        with profiler.region("lm_bias_gelu:bwd", nbytes=3 * rows * d * 4, bound="hbm"):
            N.check(lib.smt_lm_bias_gelu_bwd(N.ptr(h), N.ptr(bias), N.ptr(da), N.ptr(dh), N.ptr(dbias), rows, d, drop.key,
                                             N.ptr(drop.key_dev), drop.thresh, drop.scale, N.ptr(ws), ws_bytes, N.stream_ptr()),
                    "smt_lm_bias_gelu_bwd")
        return dh, dbias, None


def bias_gelu_dropout(h, bias, drop=NO_DROP):
    """dropout(gelu(h + bias)), the exact (erf) GELU, on the (bias-free) output of linear1.  Not in place: h stays as it is
    and is kept for the backward, which needs the pre-activation."""
    return _BiasGeluDrop.apply(h, bias, drop)


class _BiasReluDrop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, bias, drop):
        d = h.shape[-1]
        rows = h.numel() // d
        h = _f32(h)
        with profiler.region("lm_bias_relu:fwd", nbytes=2 * rows * d * 4, bound="hbm"):
            N.check(N.lib().smt_lm_bias_relu_fwd(N.ptr(h), N.ptr(_f32(bias)), rows, d, drop.key, N.ptr(drop.key_dev), drop.thresh, drop.scale,
                                                 N.stream_ptr()), "smt_lm_bias_relu_fwd")
        ctx.mark_dirty(h)
        ctx.save_for_backward(h)
        ctx.meta = (rows, d, drop)
        return h

    @staticmethod
    def backward(ctx, da):
        (a,) = ctx.saved_tensors
        rows, d, drop = ctx.meta
        lib = N.lib()
        da = _f32(da)
        dh = torch.empty_like(da)
        dbias = torch.empty(d, device=a.device, dtype=torch.float32)
        ws_bytes = lib.smt_lm_bias_relu_bwd_workspace_bytes(rows, d)
        ws = torch.empty(ws_bytes, device=a.device, dtype=torch.uint8)
        with profiler.region("lm_bias_relu:bwd", nbytes=3 * rows * d * 4, bound="hbm"):
            N.check(lib.smt_lm_bias_relu_bwd(N.ptr(a), N.ptr(da), N.ptr(dh), N.ptr(dbias), rows, d, drop.key, N.ptr(drop.key_dev), drop.thresh, drop.scale,
                                             N.ptr(ws), ws_bytes, N.stream_ptr()), "smt_lm_bias_relu_bwd")
        return dh, dbias, None


def bias_relu_dropout_(h, bias, drop=NO_DROP):
    """In place: dropout(relu(h + bias)) on the (bias-free) output of linear1 (feed-forward of the encoder layer)."""
    return _BiasReluDrop.apply(h, bias, drop)


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        v = logits.shape[-1]
        rows = logits.numel() // v
        logits = _f32(logits)
        target = target.contiguous()
        row_out = torch.empty(rows, 2, device=logits.device, dtype=torch.float32)
        lse = torch.empty(rows, device=logits.device, dtype=torch.float32)
        N.check(N.lib().smt_lm_ce_fwd(N.ptr(logits), N.ptr(target), N.ptr(row_out), N.ptr(lse), rows, v, N.stream_ptr()),
                "smt_lm_ce_fwd")
        count = (target >= 0).sum().to(torch.float32)
        sums = row_out.sum(0)
        ctx.save_for_backward(logits, target, lse, count)
        ctx.mark_non_differentiable(count)
        loss, acc = sums[0] / count, sums[1] / count
        ctx.mark_non_differentiable(acc)
        return loss, acc, count

    @staticmethod
    def backward(ctx, dloss, _dacc, _dcount):
        logits, target, lse, count = ctx.saved_tensors
        v = logits.shape[-1]
        rows = logits.numel() // v
        coef = (dloss.to(torch.float32) / count).reshape(1).contiguous()
        dlogits = torch.empty_like(logits)
        N.check(N.lib().smt_lm_ce_bwd(N.ptr(logits), N.ptr(target), N.ptr(lse), N.ptr(coef), N.ptr(dlogits), rows, v,
                                      N.stream_ptr()), "smt_lm_ce_bwd")
        return dlogits, None


def cross_entropy(logits, target):
    """(mean CE over rows with target >= 0, accuracy over the same rows, their number) -- transformer_lm.py:121-128 with
    the reference's boolean row selection turned into target = -1 on the rows it drops."""
    assert target.dtype == torch.int64
    return _CrossEntropy.apply(logits, target)


class _FocalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, gamma):
        v = logits.shape[-1]
        rows = logits.numel() // v
        logits = _f32(logits)
        target = target.contiguous()
        row_out = torch.empty(rows, 2, device=logits.device, dtype=torch.float32)
        lse = torch.empty(rows, device=logits.device, dtype=torch.float32)
        row_coef = torch.empty(rows, device=logits.device, dtype=torch.float32)
        N.check(N.lib().smt_lm_focal_fwd(N.ptr(logits), N.ptr(target), N.ptr(row_out), N.ptr(lse), N.ptr(row_coef), rows, v, gamma,
                                         N.stream_ptr()), "smt_lm_focal_fwd")
        count = (target >= 0).sum().to(torch.float32)
        sums = row_out.sum(0)
        ctx.save_for_backward(logits, target, lse, row_coef, count)
        # no scored row: 0 like FocalLoss (the row sums are 0 then), where the mean of the cross entropy is nan
        loss, acc = sums[0] / count.clamp_min(1.0), sums[1] / count
        ctx.mark_non_differentiable(acc, count)                   # one call: a second one would replace the first
        return loss, acc, count

    @staticmethod
    def backward(ctx, dloss, _dacc, _dcount):
        logits, target, lse, row_coef, count = ctx.saved_tensors
        v = logits.shape[-1]
        rows = logits.numel() // v
        coef = (dloss.to(torch.float32) / count.clamp_min(1.0)).reshape(1).contiguous()
        dlogits = torch.empty_like(logits)
        N.check(N.lib().smt_lm_focal_bwd(N.ptr(logits), N.ptr(target), N.ptr(lse), N.ptr(row_coef), N.ptr(coef), N.ptr(dlogits), rows, v,
                                         N.stream_ptr()), "smt_lm_focal_bwd")
        return dlogits, None, None


def focal_loss(logits, target, gamma):
    """(mean of (1 - p_t)^gamma * CE over rows with target >= 0, accuracy over the same rows, their number): FocalLoss of
    models/transformer_lm/losses.py without class weights, on the device (smt_lm_focal_fwd / _bwd) and with the convention of
    `cross_entropy`: target = -1 on the rows that are not scored.  gamma = 0 or >= 1 (else RuntimeError).  No scored row: loss 0
    (as FocalLoss), accuracy nan."""
    assert target.dtype == torch.int64
    return _FocalLoss.apply(logits, target, float(gamma))


class _MMILoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        v = logits.shape[-1]
        rows = logits.numel() // v
        logits = _f32(logits)
        target = target.contiguous()
        lib = N.lib()
        dev = logits.device
        row_out = torch.empty(rows, 2, device=dev, dtype=torch.float32)
        lse = torch.empty(rows, device=dev, dtype=torch.float32)
        logm = torch.empty(v, device=dev, dtype=torch.float32)
        ent = torch.full((1,), float("nan"), device=dev, dtype=torch.float32)     # rows = 0 launches nothing
        count = (target >= 0).sum().to(torch.float32)
        ws_bytes = lib.smt_lm_mmi_workspace_bytes(rows, v)
        ws = N.workspace.get(max(int(ws_bytes), 16), dev)          # consumed inside this call: nothing of it is kept for backward
        N.check(lib.smt_lm_mmi_fwd(N.ptr(logits), N.ptr(target), N.ptr(count.reshape(1)), N.ptr(row_out), N.ptr(lse), N.ptr(logm),
                                   N.ptr(ent), rows, v, N.ptr(ws), ws.numel(), N.stream_ptr()), "smt_lm_mmi_fwd")
        sums = row_out.sum(0)
        ctx.save_for_backward(logits, target, lse, logm, count)
        # the constant is formed in double and rounded once, when it meets the fp32 tensor
        loss, acc = math.log(math.e + v - 1) - sums[0] / count + ent[0], sums[1] / count
        ctx.mark_non_differentiable(acc, count)
        return loss, acc, count

    @staticmethod
    def backward(ctx, dloss, _dacc, _dcount):
        logits, target, lse, logm, count = ctx.saved_tensors
        v = logits.shape[-1]
        rows = logits.numel() // v
        coef = (dloss.to(torch.float32) / count).reshape(1).contiguous()
        dlogits = torch.empty_like(logits)
        N.check(N.lib().smt_lm_mmi_bwd(N.ptr(logits), N.ptr(target), N.ptr(lse), N.ptr(logm), N.ptr(coef), N.ptr(dlogits), rows, v,
                                       N.stream_ptr()), "smt_lm_mmi_bwd")
        return dlogits, None


def mmi_loss(logits, target):
    """(MaximumMutualInformationLoss over the rows with target >= 0, accuracy over the same rows, their number) on the device
    (smt_lm_mmi_fwd / _bwd), target = -1 on the rows that are not scored.  The marginal is that of the rows of this call (one
    rank's own rows under data parallelism, as in the reference).  No scored row: loss and accuracy nan."""
    assert target.dtype == torch.int64
    return _MMILoss.apply(logits, target)


# ------------------------------------------------------------------------------------------------ dense projections
# csrc/lm_linear.hip, include/smt_hip.h "The dense projections with bf16 operands".
def _rows(t, width):
    """(tensor whose storage the kernel reads, row pitch in elements) of t [..., width]: t itself when its last axis is dense,
    its leading axes collapse to one row index, and pitch and address suit the kernels' 16-byte accesses (a column slice of a
    wider contiguous tensor does); a contiguous copy otherwise."""
    if t.dim() >= 2 and t.stride(-1) == 1 and t.numel() > 0:
        pitch = t.stride(-2)
        ok = pitch >= width and pitch % 4 == 0 and t.data_ptr() % 16 == 0
        for i in range(t.dim() - 2):
            ok = ok and (t.shape[i] == 1 or t.stride(i) == t.stride(i + 1) * t.shape[i + 1])
        if ok:
            return t, pitch
    return t.contiguous(), width


def _addr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _packed_bf16(weight, transposed):
    """The bf16 operand copy of weight [n_out, n_in]: as it stands (forward) or as [n_in][n_out] (data gradient).  A Parameter's
    copy lives in the pack cache and is refreshed once per optimizer step with all the others (smt_amd.packing)."""
    n_out, n_in = weight.shape
    if not weight.is_contiguous():
        weight = weight.contiguous()
    if transposed:
        return packing.pack([packing.Part.dense(weight, n_in, n_out, 1, n_in, 1, (0,))], torch.bfloat16, (1, n_in, n_out))
    return packing.pack([packing.Part.dense(weight, n_out, n_in, n_in, 1, 1, (0,))], torch.bfloat16, (1, n_out, n_in))


class _LinearBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        n_out, n_in = weight.shape
        assert x.shape[-1] == n_in and (bias is None or bias.shape == (n_out,))
        for t in (x, weight, bias):
            assert t is None or (t.dtype == torch.float32 and t.is_cuda), "lm.linear in bf16 takes fp32 device tensors"
        xs, ld_x = _rows(x, n_in)
        rows = x.numel() // n_in
        y = torch.empty(*x.shape[:-1], n_out, device=x.device, dtype=torch.float32)
        ctx.save_for_backward(x, weight)
        ctx.with_bias = bias is not None
        if rows == 0:
            return y
        wp = _packed_bf16(weight, False)
        with profiler.region("lm_linear_fwd", flops=2 * rows * n_in * n_out, bound="mfma", dtype="bf16"):
            N.check(N.lib().smt_lm_linear_fwd(_addr(xs), ld_x, N.ptr(wp), N.ptr(None if bias is None else bias.contiguous()), N.ptr(y),
                                              n_out, rows, n_in, n_out, N.stream_ptr()), "smt_lm_linear_fwd")
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        n_out, n_in = weight.shape
        rows = x.numel() // n_in
        lib = N.lib()
        if rows == 0:                                                   # no row: an empty dx, the sums over nothing
            return (torch.empty_like(x), torch.zeros_like(weight),
                    torch.zeros(n_out, device=x.device, dtype=torch.float32) if ctx.with_bias else None)
        dys, ld_dy = _rows(dy, n_out)
        dx = dweight = dbias = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(*x.shape[:-1], n_in, device=x.device, dtype=torch.float32)
            wt = _packed_bf16(weight, True)
            with profiler.region("lm_linear_dgrad", flops=2 * rows * n_in * n_out, bound="mfma", dtype="bf16"):
                N.check(lib.smt_lm_linear_dgrad(_addr(dys), ld_dy, N.ptr(wt), N.ptr(dx), n_in, rows, n_in, n_out, N.stream_ptr()),
                        "smt_lm_linear_dgrad")
        if ctx.needs_input_grad[1] or (ctx.with_bias and ctx.needs_input_grad[2]):
            xs, ld_x = _rows(x, n_in)
            dweight = torch.empty(n_out, n_in, device=x.device, dtype=torch.float32)
            dbias = torch.empty(n_out, device=x.device, dtype=torch.float32) if ctx.with_bias else None
            ws_bytes = lib.smt_lm_linear_wgrad_workspace_bytes(rows, n_in, n_out)
            ws = N.workspace.get(max(int(ws_bytes), 16), x.device)      # consumed inside this call
            with profiler.region("lm_linear_wgrad", flops=2 * rows * n_in * n_out, bound="mfma", dtype="bf16"):
                N.check(lib.smt_lm_linear_wgrad(_addr(xs), ld_x, _addr(dys), ld_dy, N.ptr(dweight), N.ptr(dbias), rows, n_in, n_out,
                                                N.ptr(ws), ws.numel(), N.stream_ptr()), "smt_lm_linear_wgrad")
        return dx, dweight, dbias


def linear(x, weight, bias=None, *, compute_dtype=torch.float32):
    """x [..., n_in] @ weight [n_out, n_in]^T (+ bias).  compute_dtype fp32: torch.nn.functional.linear (the library GEMM), the
    very call the model made before it had a choice.  bf16: the native GEMMs of csrc/lm_linear.hip -- x, dy and the weight
    are rounded to bf16 as operands, sums and the bias add are fp32, every tensor in memory stays fp32; n_in a multiple of 32,
    n_out of 16.  x is read in place when its last axis is dense and its leading axes are contiguous (a column slice of a
    wider tensor is); backward keeps x and the weight, as F.linear does."""
    if compute_dtype == torch.float32:
        return F.linear(x, weight, bias)
    if compute_dtype != torch.bfloat16:
        raise ValueError(f"lm.linear: compute_dtype must be torch.float32 or torch.bfloat16 (got {compute_dtype!r})")
    return _LinearBF16.apply(x, weight, bias)


# ------------------------------------------------------------------------------------------------ incremental decoding
# csrc/lm_decode.hip, include/smt_hip.h "Incremental decoding": eval mode, fp32, no autograd.  Every op writes into a buffer the
# caller owns (DecodeState) and takes the position by value (`pos`) or from device memory (`pos_dev`, which overrides it).
def _pos_args(pos, pos_dev):
    if pos_dev is not None:
        assert pos_dev.is_cuda and pos_dev.dtype == torch.int32 and pos_dev.numel() == 1
    return int(pos), N.ptr(pos_dev)


def decode_embed(tokens, weight, pe, out, pos=0, pos_dev=None):
    """out[b] = weight[tokens[b, pos]] * sqrt(dim) + pe[pos]; tokens [batch, tok_len] int64, out [batch, dim]."""
    b, l = tokens.shape
    d = weight.shape[1]
    assert tokens.dtype == torch.int64 and pe.shape[-1] == d and out.shape == (b, d) and out.dtype == torch.float32
    p, pd = _pos_args(pos, pos_dev)
    N.check(N.lib().smt_lm_decode_embed(N.ptr(tokens), N.ptr(_f32(weight)), N.ptr(_f32(pe)), N.ptr(out), b, l, d, weight.shape[0],
                                        pe.shape[0], math.sqrt(d), p, pd, N.stream_ptr()), "smt_lm_decode_embed")
    return out


ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


def decode_linear(x, weight, bias=None, out=None, relu=False, act=None):
    """out [batch, n] = act(x [batch, k] @ weight [n, k]^T (+ bias)); act: 0 none, 1 ReLU, 2 exact GELU (`relu=True` is act=1);
    batch <= 32, k % 64 == 0 (else RuntimeError)."""
    b, k = x.shape
    n = weight.shape[0]
    assert weight.shape == (n, k) and (bias is None or bias.shape == (n,))
    if act is None:
        act = ACT_RELU if relu else ACT_NONE
    elif relu and act != ACT_RELU:
        raise ValueError(f"decode_linear: relu=True and act={act!r} contradict each other")
    if out is None:
        out = torch.empty(b, n, device=x.device, dtype=torch.float32)
    assert out.shape == (b, n) and out.dtype == torch.float32
    N.check(N.lib().smt_lm_decode_linear(N.ptr(_f32(x)), N.ptr(_f32(weight)), N.ptr(None if bias is None else _f32(bias)), N.ptr(out),
                                         b, k, n, int(act), N.stream_ptr()), "smt_lm_decode_linear")
    return out


def decode_attention_workspace(batch, heads, l_max, device, head_dim=32):
    """The partial-softmax buffer of `decode_attention` for caches of l_max rows (None when none is needed)."""
    assert head_dim in HEAD_DIMS, f"the attention kernels are built for head dim 32 or 64 (got {head_dim})"
    nbytes = N.lib().smt_lm_decode_attention_hd_workspace_bytes(batch, heads, l_max, head_dim)
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def decode_attention(qkv, k_cache, v_cache, ctx, workspace=None, pos=0, pos_dev=None, rope=None):
    """qkv [batch, 3 * heads * dh] of the token at `pos`; k_cache / v_cache [batch, heads, l_max, dh] get its k / v rows at row
    pos; ctx [batch, heads * dh] = softmax(q K[0..pos]^T / sqrt(dh)) V[0..pos].  dh, read from the caches, is 32 or 64.
    rope (a `rope_table` [rows, dh / 2, 2], or None): q and the step's k are rotated at position pos inside the same launch, so
    the cache holds rotated keys; None is the launch without it."""
    b, h, l_max, dh = k_cache.shape
    assert dh in HEAD_DIMS, f"the attention kernels are built for head dim 32 or 64 (got {dh})"
    assert v_cache.shape == k_cache.shape and qkv.shape == (b, 3 * h * dh) and ctx.shape == (b, h * dh)
    assert k_cache.dtype == v_cache.dtype == ctx.dtype == torch.float32
    p, pd = _pos_args(pos, pos_dev)
    ws_bytes = 0 if workspace is None else workspace.numel()
    if rope is None:
        N.check(N.lib().smt_lm_decode_attention_hd(N.ptr(_f32(qkv)), N.ptr(k_cache), N.ptr(v_cache), N.ptr(ctx), N.ptr(workspace),
                                                   ws_bytes, b, h, l_max, dh, p, pd, N.stream_ptr()), "smt_lm_decode_attention_hd")
        return ctx
    assert rope.dim() == 3 and rope.shape[1:] == (dh // 2, 2) and rope.dtype == torch.float32 and rope.is_cuda and rope.is_contiguous(), \
        f"decode_attention: the rope table must be a contiguous fp32 device tensor [rows, {dh // 2}, 2]"
    N.check(N.lib().smt_lm_decode_attention_rope(N.ptr(_f32(qkv)), N.ptr(k_cache), N.ptr(v_cache), N.ptr(ctx), N.ptr(workspace), ws_bytes,
                                                 b, h, l_max, dh, N.ptr(rope), rope.shape[0], p, pd, N.stream_ptr()),
            "smt_lm_decode_attention_rope")
    return ctx


def decode_sample(logits, uniforms, tokens, codes, sigma=1.0, pos=0, pos_dev=None, token_offset=2):
    """Inverse-CDF draw from softmax(logits / sigma) with uniforms[pos, b]: tokens[b, pos + 1] = k + token_offset,
    codes[b, pos] = k.  logits [batch, vocab], uniforms [n_steps, batch] f32, tokens [batch, tok_len] / codes [batch, n_steps] int64."""
    b, v = logits.shape
    n_steps = uniforms.shape[0]
    assert uniforms.shape == (n_steps, b) and uniforms.dtype == torch.float32 and tokens.shape[0] == b and codes.shape == (b, n_steps)
    assert tokens.dtype == codes.dtype == torch.int64
    p, pd = _pos_args(pos, pos_dev)
    N.check(N.lib().smt_lm_decode_sample(N.ptr(_f32(logits)), N.ptr(uniforms), N.ptr(tokens), N.ptr(codes), b, v, tokens.shape[1], n_steps,
                                         1.0 / sigma, token_offset, p, pd, N.stream_ptr()), "smt_lm_decode_sample")


def decode_sample_filtered(logits, uniforms, tokens, codes, sigma=1.0, top_k=None, top_p=None, kept=None, pos=0, pos_dev=None,
                           token_offset=2):
    """`decode_sample` over the top-k / nucleus prefix of the codes ordered by logit (descending, ties by index): the first
    min(top_k, vocab) codes are the candidates, of which the shortest prefix holding top_p of THEIR mass is kept (None = off);
    kept [n_steps, batch] int32 (optional) gets the size of the kept set at row pos.  Both off: the codes of `decode_sample`."""
    b, v = logits.shape
    n_steps = uniforms.shape[0]
    assert uniforms.shape == (n_steps, b) and uniforms.dtype == torch.float32 and tokens.shape[0] == b and codes.shape == (b, n_steps)
    assert tokens.dtype == codes.dtype == torch.int64
    assert kept is None or (kept.shape == (n_steps, b) and kept.dtype == torch.int32 and kept.is_cuda and kept.is_contiguous())
    p, pd = _pos_args(pos, pos_dev)
    N.check(N.lib().smt_lm_decode_sample_filtered(N.ptr(_f32(logits)), N.ptr(uniforms), N.ptr(tokens), N.ptr(codes), b, v, tokens.shape[1],
                                                  n_steps, 1.0 / sigma, token_offset, 0 if top_k is None else int(top_k),
                                                  1.0 if top_p is None else float(top_p), N.ptr(kept), p, pd, N.stream_ptr()),
            "smt_lm_decode_sample_filtered")


def decode_prefill_kv(qkv, k_cache, v_cache):
    """The k and v thirds of qkv [batch, len, 3 * heads * dh] (the batched in-projection of a prompt) into rows 0..len-1 of
    k_cache / v_cache [batch, heads, l_max, dh]; rows from len on are left alone.  dh, read from the caches, is 32 or 64."""
    b, h, l_max, dh = k_cache.shape
    assert dh in HEAD_DIMS, f"the attention kernels are built for head dim 32 or 64 (got {dh})"
    assert v_cache.shape == k_cache.shape and qkv.dim() == 3 and qkv.shape[0] == b and qkv.shape[2] == 3 * h * dh
    assert k_cache.dtype == v_cache.dtype == torch.float32 and k_cache.is_contiguous() and v_cache.is_contiguous()
    N.check(N.lib().smt_lm_decode_prefill_kv_hd(N.ptr(_f32(qkv)), N.ptr(k_cache), N.ptr(v_cache), b, qkv.shape[1], h, l_max, dh,
                                                N.stream_ptr()), "smt_lm_decode_prefill_kv_hd")


def decode_advance(pos_dev):
    """pos_dev += 1 on the device."""
    assert pos_dev.is_cuda and pos_dev.dtype == torch.int32 and pos_dev.numel() == 1
    N.check(N.lib().smt_lm_decode_advance(N.ptr(pos_dev), N.stream_ptr()), "smt_lm_decode_advance")


def decode_layer_norm(x, h, h_bias, gamma, beta, eps, out, stats):
    """smt_lm_add_ln_fwd on `rows = batch` without dropout, into caller-owned `out` / `stats`."""
    rows, d = x.shape
    N.check(N.lib().smt_lm_add_ln_fwd(N.ptr(x), N.ptr(h), N.ptr(h_bias), N.ptr(_f32(gamma)), N.ptr(_f32(beta)), N.ptr(out), N.ptr(stats),
                                      rows, d, eps, 0, None, 0, 1.0, N.stream_ptr()), "smt_lm_add_ln_fwd")
    return out


def decode_residual_layer_norm(x, h, h_bias, gamma, beta, eps, s_out, out, stats):
    """smt_lm_res_ln_fwd on `rows = batch` without dropout: s_out = x + h + h_bias (the new stream), out = LayerNorm(s_out), both
    caller-owned and distinct from x and h."""
    rows, d = x.shape
    N.check(N.lib().smt_lm_res_ln_fwd(N.ptr(x), N.ptr(h), N.ptr(h_bias), N.ptr(_f32(gamma)), N.ptr(_f32(beta)), N.ptr(s_out), N.ptr(out),
                                      N.ptr(stats), rows, d, eps, 0, None, 0, 1.0, N.stream_ptr()), "smt_lm_res_ln_fwd")
    return s_out, out


class DecodeState:
    """Every buffer of an incremental decoding loop (TransformerLM.sample(causal=True) / step_logits): the key/value cache
    [layers, 2, batch, heads, l_max, dh] (dh = dim / heads, 32 or 64), the token [batch, n_steps + 1] and code [batch, n_steps] buffers, the position
    (``pos_dev`` on the device, mirrored by ``pos`` on the host), the uniforms [n_steps, batch], the kept-set sizes of the
    filtered sampler [n_steps, batch] int32 and the activations of one step.
    Nothing here comes from the grow-only workspace of smt_amd.native: captured launches keep pointing at these tensors."""

    def __init__(self, batch, n_steps, dim, heads, dim_ff, vocab, layers, device, first_token=1, uniforms=None):
        dh = _head_dim(dim, heads)
        f32 = dict(device=device, dtype=torch.float32)
        self.batch, self.n_steps = batch, n_steps
        self.kv = torch.empty(layers, 2, batch, heads, n_steps, dh, **f32)           # rows beyond pos are never read
        self.tokens = torch.zeros(batch, n_steps + 1, device=device, dtype=torch.int64)
        self.tokens[:, 0] = first_token
        self.codes = torch.zeros(batch, n_steps, device=device, dtype=torch.int64)
        self.pos_dev = torch.zeros(1, device=device, dtype=torch.int32)
        self.pos = 0
        self.uniforms = torch.zeros(n_steps, batch, **f32) if uniforms is None else uniforms.to(**f32).contiguous()
        assert self.uniforms.shape == (n_steps, batch)
        self.kept = torch.zeros(n_steps, batch, device=device, dtype=torch.int32)
        self.h, self.h1, self.ctx, self.a = (torch.empty(batch, dim, **f32) for _ in range(4))
        self.s = torch.empty(batch, dim, **f32)        # pre-norm layers: the residual stream between a layer's two sub-layers
        self.qkv = torch.empty(batch, 3 * dim, **f32)
        self.f = torch.empty(batch, dim_ff, **f32)
        self.stats = torch.empty(batch, 2, **f32)
        self.logits = torch.empty(batch, vocab, **f32)
        self.attn_ws = decode_attention_workspace(batch, heads, n_steps, device, dh)
        self.pe = None        # set by a model with rotary positions: the [n_steps, dim] zeros its decode_embed adds

    def advance(self):
        """pos += 1, on the device and in the host mirror."""
        decode_advance(self.pos_dev)
        self.pos += 1

    def prefill_done(self, n):
        """The position after a prefill of n prompt tokens (their keys / values are in cache rows 0..n-1): pos = n on the
        device and in the host mirror, so the next step processes tokens[:, n]."""
        if self.pos != 0 or not 1 <= n <= self.n_steps:
            raise ValueError(f"DecodeState.prefill_done: needs a state at position 0 and 1 <= n <= {self.n_steps} (pos {self.pos}, n {n})")
        self.pos_dev.fill_(n)
        self.pos = n

    def push(self, tokens):
        """Force the next token (teacher forcing): tokens [batch] int64 -> tokens[:, pos + 1], then advance."""
        if self.pos + 1 > self.n_steps:
            raise ValueError(f"DecodeState.push: the token buffer holds {self.n_steps + 1} tokens")
        self.tokens[:, self.pos + 1] = tokens.to(self.tokens.device, torch.int64)
        self.advance()
