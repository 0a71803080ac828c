"""Causal TransformerLM over VQ codes (reference models/transformer_lm/transformer_lm.py:32-155).

Same constructor keys, parameter names (a reference state_dict loads as is), ``forward`` / ``sample`` /
``reconstruct`` / ``load_vqvae`` surface and loss definition as the reference, which builds the stack from
``torch.nn.TransformerEncoder``.  Here a layer is its dense projections (``smt_amd.lm.linear``: library GEMMs in fp32, or with
``model.compute_dtype: bf16`` the native bf16-operand GEMMs of csrc/lm_linear.hip) with everything between them in the HIP kernels
of csrc/lm.hip (attention core -- with ``model.attention_dtype: bf16`` its products on bf16 MFMAs --, add + dropout + LayerNorm, bias + ReLU + dropout, embedding, the three losses); activations
are batch-major [B, L, d] instead of the reference's [L, B, d].  ``model.norm_first`` and ``model.activation`` are
nn.TransformerEncoderLayer's arguments of those names: pre-norm layers run their residual adds fused with the NEXT LayerNorm
(``smt_amd.lm.residual_layer_norm``), ``gelu`` is the exact form (``smt_amd.lm.bias_gelu_dropout``).  Dropout uses the
counter-based generator keyed by (step counter, site): site 0 = positional-encoding dropout, 1 + 4 i + {0, 1, 2, 3} = layer
i's attention-weight, attention-output, feed-forward-inner and feed-forward-output dropouts.
"""
import copy
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from models.base import TokenToWaveformModel
from smt_amd import lm as K
from smt_amd import packing

COMPUTE_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
ACTIVATIONS = {"relu": K.ACT_RELU, "gelu": K.ACT_GELU}
POSITIONS = ("sinusoidal", "rotary")


class PositionalEncoding(nn.Module):
    """Sinusoidal table ``pe`` [max_len, 1, d_model] (transformer_lm.py:14-29); applied inside the embedding kernel."""

    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.p = dropout
        position = torch.arange(max_len, dtype=torch.float32)[:, None]
        div_term = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, 1, d_model)
        pe[:, 0, 0::2] = torch.sin(position * div_term)
        pe[:, 0, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe)

    def table(self):
        return self.pe.view(self.pe.shape[0], self.pe.shape[2])


class _SelfAttention(nn.Module):
    """Parameter holder with nn.MultiheadAttention's names and initialisation."""

    def __init__(self, d_model, nhead):
        super().__init__()
        assert d_model % nhead == 0
        self.num_heads = nhead
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d_model, d_model))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d_model))
        self.out_proj = nn.Linear(d_model, d_model)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)


class _EncoderLayer(nn.Module):
    """Encoder layer with nn.TransformerEncoderLayer's parameter names; post-norm (`forward`, `prefill`) or pre-norm
    (`forward_pre`, `prefill_pre`: the encoder calls the pair that matches its norm_first), ReLU or exact-GELU feed-forward."""

    def __init__(self, d_model, nhead, dim_feedforward, dropout, layer_norm_eps=1e-5, compute_dtype=torch.float32, activation="relu",
                 attention_dtype=torch.float32):
        super().__init__()
        self.compute_dtype = compute_dtype      # of the four projections' operands (smt_amd.lm.linear)
        self.attention_dtype = attention_dtype  # of the attention core's products (smt_amd.lm.attention)
        self.act = ACTIVATIONS[activation]
        self.self_attn = _SelfAttention(d_model, nhead)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.norm2 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.p = dropout

    def _ff_inner(self, x, drop=K.NO_DROP):
        """dropout(activation(linear1(x))): the bias, the activation and the dropout in one kernel after the bias-free GEMM."""
        h = K.linear(x, self.linear1.weight, compute_dtype=self.compute_dtype)
        if self.act == K.ACT_GELU:
            return K.bias_gelu_dropout(h, self.linear1.bias, drop)
        return K.bias_relu_dropout_(h, self.linear1.bias, drop)

    def _in_proj(self, x, rope):
        """The in-projection; with a rotary table its q and k thirds are rotated in place, row l at position l."""
        sa = self.self_attn
        qkv = K.linear(x, sa.in_proj_weight, sa.in_proj_bias, compute_dtype=self.compute_dtype)
        return qkv if rope is None else K.rope(qkv, rope, sa.num_heads)

    def forward(self, x, lens, causal, seed, site0, kd=None, rope=None):
        sa, tr, p, cd = self.self_attn, self.training, self.p, self.compute_dtype
        qkv = self._in_proj(x, rope)
        ctx = K.attention(qkv, lens, sa.num_heads, causal, K.Drop(p, tr, seed, site0, kd), compute_dtype=self.attention_dtype)
        a = K.linear(ctx, sa.out_proj.weight, compute_dtype=cd)    # its bias is added (and differentiated) inside add_layer_norm
        x = K.add_layer_norm(x, a, self.norm1.weight, self.norm1.bias, self.norm1.eps, K.Drop(p, tr, seed, site0 + 1, kd),
                             h_bias=sa.out_proj.bias)
        f = self._ff_inner(x, K.Drop(p, tr, seed, site0 + 2, kd))
        f = K.linear(f, self.linear2.weight, compute_dtype=cd)
        return K.add_layer_norm(x, f, self.norm2.weight, self.norm2.bias, self.norm2.eps, K.Drop(p, tr, seed, site0 + 3, kd),
                                h_bias=self.linear2.bias)

    def forward_pre(self, s, y, nxt, lens, causal, seed, site0, kd=None, rope=None):
        """Pre-norm layer: s [B, L, d] is the residual stream, y = norm1(s) already formed by whoever produced s, `nxt` the
        LayerNorm that follows this layer (the next layer's norm1 or the encoder's final norm).  Returns (s', nxt(s')): each
        residual add runs fused with the norm after it, so a layer is the same four launches as the post-norm one."""
        sa, tr, p, cd = self.self_attn, self.training, self.p, self.compute_dtype
        qkv = self._in_proj(y, rope)
        ctx = K.attention(qkv, lens, sa.num_heads, causal, K.Drop(p, tr, seed, site0, kd), compute_dtype=self.attention_dtype)
        a = K.linear(ctx, sa.out_proj.weight, compute_dtype=cd)    # its bias is added (and differentiated) inside residual_layer_norm
        s, y = K.residual_layer_norm(s, a, self.norm2.weight, self.norm2.bias, self.norm2.eps, K.Drop(p, tr, seed, site0 + 1, kd),
                                     h_bias=sa.out_proj.bias)
        f = self._ff_inner(y, K.Drop(p, tr, seed, site0 + 2, kd))
        f = K.linear(f, self.linear2.weight, compute_dtype=cd)
        return K.residual_layer_norm(s, f, nxt.weight, nxt.bias, nxt.eps, K.Drop(p, tr, seed, site0 + 3, kd), h_bias=self.linear2.bias)

    def prefill(self, x, k_cache, v_cache, last, rope=None):
        """Eval-mode `forward` over a prompt x [B, P, d] (causal, no lengths, no dropout) that also writes the P key / value
        rows into the decoding cache; the last layer stops there (nothing reads its output: the next decoding step attends
        to the cache only) and returns None."""
        sa, cd = self.self_attn, self.compute_dtype
        qkv = self._in_proj(x, rope)                               # rotated before the copy: the cache holds rotated keys
        K.decode_prefill_kv(qkv, k_cache, v_cache)
        if last:
            return None
        ctx = K.attention(qkv, None, sa.num_heads, True, compute_dtype=self.attention_dtype)
        a = K.linear(ctx, sa.out_proj.weight, compute_dtype=cd)
        x = K.add_layer_norm(x, a, self.norm1.weight, self.norm1.bias, self.norm1.eps, h_bias=sa.out_proj.bias)
        f = self._ff_inner(x)
        f = K.linear(f, self.linear2.weight, compute_dtype=cd)
        return K.add_layer_norm(x, f, self.norm2.weight, self.norm2.bias, self.norm2.eps, h_bias=self.linear2.bias)

    def prefill_pre(self, s, y, nxt, k_cache, v_cache, last, rope=None):
        """`prefill` of a pre-norm layer, on the (s, y) pair of `forward_pre`; returns the next pair, or None from the last layer."""
        sa, cd = self.self_attn, self.compute_dtype
        qkv = self._in_proj(y, rope)
        K.decode_prefill_kv(qkv, k_cache, v_cache)
        if last:
            return None
        ctx = K.attention(qkv, None, sa.num_heads, True, compute_dtype=self.attention_dtype)
        a = K.linear(ctx, sa.out_proj.weight, compute_dtype=cd)
        s, y = K.residual_layer_norm(s, a, self.norm2.weight, self.norm2.bias, self.norm2.eps, h_bias=sa.out_proj.bias)
        f = K.linear(self._ff_inner(y), self.linear2.weight, compute_dtype=cd)
        return K.residual_layer_norm(s, f, nxt.weight, nxt.bias, nxt.eps, h_bias=self.linear2.bias)


class _Encoder(nn.Module):
    """``layers`` + final ``norm`` as in nn.TransformerEncoder, which deep-copies ONE initialised layer: every layer
    starts from the same weights, and so do these."""

    def __init__(self, layer, num_layers, norm):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(num_layers)])
        self.norm = norm


class TransformerLM(TokenToWaveformModel):

    PAD = 0     # <pad> token
    BOS = 1     # <bos> token
    OFFSET = 2  # number of special tokens the original vocabulary is shifted by

    def __init__(self, config):
        super().__init__()
        m = config.model
        assert m.embed_dim == m.d_model, "the embedding feeds the encoder directly"
        # nn.TransformerEncoderLayer's arguments of the same names; absent = the reference's construction (post-norm, ReLU)
        self.norm_first = m.get("norm_first", False)
        if not isinstance(self.norm_first, bool):
            raise ValueError(f"model.norm_first must be true or false (got {self.norm_first!r})")
        activation = m.get("activation", "relu")
        if activation not in ACTIVATIONS:
            raise ValueError(f"model.activation must be relu or gelu (got {activation!r})")
        # operands of the six dense projections: fp32 = library GEMMs, bf16 = csrc/lm_linear.hip (everything else stays fp32,
        # the incremental decoding path included: it reads the fp32 master weights)
        name = m.get("compute_dtype", "fp32")
        if name not in COMPUTE_DTYPES:
            raise ValueError(f"model.compute_dtype must be fp32 or bf16 (got {name!r})")
        self.compute_dtype = COMPUTE_DTYPES[name]
        if self.compute_dtype == torch.bfloat16:
            for key, mult in (("d_model", 32), ("dim_feedforward", 32), ("vocab_size", 16)):
                if m[key] % mult:
                    raise ValueError(f"model.compute_dtype bf16: {key}={m[key]} must be a multiple of {mult} (the GEMM kernels' limit)")
        # operands of the attention core's products, independent of compute_dtype: fp32 = f32-input MFMAs, bf16 = bf16 MFMAs
        # (smt_lm_attention_bf16_*); the one-token decoding attention stays fp32 either way
        name = m.get("attention_dtype", "fp32")
        if name not in COMPUTE_DTYPES:
            raise ValueError(f"model.attention_dtype must be fp32 or bf16 (got {name!r})")
        self.attention_dtype = COMPUTE_DTYPES[name]
        # where positions enter: sinusoidal = the reference's table added to the embedding; rotary = q and k rotated inside every
        # layer (smt_amd.lm.rope, csrc/lm_rope.hip), nothing added to the embedding
        self.position = m.get("position", "sinusoidal")
        if self.position not in POSITIONS:
            raise ValueError(f"model.position must be sinusoidal or rotary (got {self.position!r})")
        self.rope_base = m.get("rope_base", 10000.0)
        if isinstance(self.rope_base, bool) or not isinstance(self.rope_base, (int, float)) or not (math.isfinite(self.rope_base) and self.rope_base > 1):
            raise ValueError(f"model.rope_base must be a finite number > 1 (got {self.rope_base!r})")
        self.d_model = m.d_model
        self.embedding = nn.Embedding(m.vocab_size + TransformerLM.OFFSET, m.embed_dim, padding_idx=TransformerLM.PAD)
        self.pos_encoding = PositionalEncoding(m.d_model, m.dropout, m.max_len)
        # the reference's layers keep nn.TransformerEncoderLayer's default eps; only the final norm takes the config's
        layer = _EncoderLayer(m.d_model, m.nhead, m.dim_feedforward, m.dropout, compute_dtype=self.compute_dtype, activation=activation,
                              attention_dtype=self.attention_dtype)
        self.transformer = _Encoder(layer, m.num_layers, nn.LayerNorm(m.d_model, eps=float(m.layer_norm_eps)))
        self.classifier = nn.Linear(m.d_model, m.vocab_size)
        # rotary: the (cos, sin) table of every position is derived from the config, so it stays out of the state dict -- whose
        # keys and shapes (pos_encoding.pe included) are the same for both settings
        self.register_buffer("rope", K.rope_table(m.max_len, m.d_model // m.nhead, self.rope_base) if self.position == "rotary" else None,
                             persistent=False)
        self._zero_pe = None                            # rotary: the table the embedding kernel adds (all zeros), grown on demand
        self.vqvae = TransformerLM.load_vqvae(m.vqvae.log_dir, m.vqvae.ckpt_num)
        self.loss_type = m.loss_type
        # all three losses run in the native loss kernels (smt_amd.lm.cross_entropy / mmi_loss / focal_loss); `self.loss`
        # holds the torch form of the other two for callers that want it, `forward` does not call it
        self.focal_gamma = float(m.get("focal_gamma", 10.0))    # the reference hard-codes 10
        if m.loss_type == "ce":
            self.loss = None
        elif m.loss_type == "mmi":
            from models.transformer_lm.losses import MaximumMutualInformationLoss
            self.loss = MaximumMutualInformationLoss(num_classes=m.vocab_size)
        elif m.loss_type == "focal":
            from models.transformer_lm.losses import FocalLoss
            self.loss = FocalLoss(gamma=self.focal_gamma, reduction="mean")
        else:
            raise ValueError(f"Loss function {m.loss_type} not supported")
        self._drop_seed = 0
        self._seed_dev = self._keys_dev = None          # device-resident dropout keys (enable_device_keys)

    def enable_device_keys(self, flag=True):
        """Keep the dropout step counter and the per-site keys in device memory (smt_lm_make_keys) instead of passing keys
        by value: a captured hipGraph of the train step then draws fresh masks on every replay (smt_amd/graph.py).  The
        masks are the same either way -- the host counter `_drop_seed` and the device one advance together."""
        if not flag:
            self._seed_dev = self._keys_dev = None
            return
        dev = self.embedding.weight.device
        self._seed_dev = torch.tensor([self._drop_seed & 0x7FFFFFFF], dtype=torch.int32, device=dev)
        self._keys_dev = torch.zeros(1 + 4 * len(self.transformer.layers), dtype=torch.int32, device=dev)
        K.make_keys(self._seed_dev, self._keys_dev)

    def _embed_table(self, rows):
        """The table the embedding kernels add, with at least `rows` rows: the sinusoidal one, or zeros with rotary positions
        (x + 0 is exact; the kernels keep refusing a null table).  The zeros are kept and grown to the longest sequence seen."""
        if self.position != "rotary":
            return self.pos_encoding.table()
        dev = self.embedding.weight.device
        if self._zero_pe is None or self._zero_pe.shape[0] < rows or self._zero_pe.device != dev:
            self._zero_pe = torch.zeros(rows, self.d_model, device=dev, dtype=torch.float32)
        return self._zero_pe

    @staticmethod
    def load_vqvae(log_dir, ckpt_num):
        """Frozen-architecture VQ-VAE pieces for audio reconstruction (transformer_lm.py:84-98): the run's config.yaml
        and ckpts/ckpt.<n>.pt -> {"bottleneck": level block, "decoder": decoder} (they stay trainable parameters of
        this model, as in the reference)."""
        from models.vqvae.vqvae import VQVAE
        from utils import config as cfglib
        config = cfglib.load(os.path.join(log_dir, "config.yaml"))
        ckpt = torch.load(os.path.join(log_dir, "ckpts", f"ckpt.{ckpt_num}.pt"), map_location="cpu", weights_only=True)
        vqvae = VQVAE(config)
        vqvae.load_state_dict(ckpt["model"])
        block = vqvae.bottleneck.level_blocks[vqvae.LEVEL]
        holder = nn.ModuleDict({"bottleneck": block, "decoder": vqvae.decoders[vqvae.LEVEL]})
        holder.compute_dtype = vqvae.compute_dtype
        return holder

    def reconstruct(self, q, mask):
        """codes q [B, T'] (no special-token offset), mask [B, 1, T'] (a length prefix) -> audio [B, T]."""
        lens = mask.reshape(mask.shape[0], -1).to(torch.int32).sum(-1).to(torch.int32)
        with torch.no_grad():
            xq = self.vqvae["bottleneck"].decode(q)
            keep = (torch.arange(q.shape[1], device=q.device)[None, :] < lens[:, None]).unsqueeze(-1)
            y, y_lens = self.vqvae["decoder"]((xq * keep).to(self.vqvae.compute_dtype), lens)
            keep_t = torch.arange(y.shape[1], device=y.device)[None, :] < y_lens[:, None]
        return (y * keep_t).float()

    @packing.forward_scope
    def logits(self, x, lens, causal=True):
        """tokens [B, L] int64 (+ int32 lengths or None) -> next-token logits [B, L, vocab]."""
        seed, tr, kd = self._drop_seed, self.training, self._keys_dev
        h = K.embed(x, self.embedding.weight, self._embed_table(x.shape[1]), K.Drop(self.pos_encoding.p, tr, seed, 0, kd),
                    TransformerLM.PAD)
        rope = self.rope
        layers, norm = self.transformer.layers, self.transformer.norm
        if self.norm_first:
            # layer 0's norm1 is the only LayerNorm on its own; every other one runs inside the residual add before it, the
            # final norm inside the last layer's second add
            n1 = layers[0].norm1
            y = K.add_layer_norm(h, None, n1.weight, n1.bias, n1.eps)
            for i, layer in enumerate(layers):
                h, y = layer.forward_pre(h, y, layers[i + 1].norm1 if i + 1 < len(layers) else norm, lens, causal, seed, 1 + 4 * i, kd, rope)
            return K.linear(y, self.classifier.weight, self.classifier.bias, compute_dtype=self.compute_dtype)
        for i, layer in enumerate(layers):
            h = layer(h, lens, causal, seed, 1 + 4 * i, kd, rope)
        h = K.add_layer_norm(h, None, norm.weight, norm.bias, norm.eps)
        return K.linear(h, self.classifier.weight, self.classifier.bias, compute_dtype=self.compute_dtype)

    @packing.forward_scope
    def forward(self, x, x_lengths, y, y_lengths, speaker=None):
        l = x.shape[1]
        lens = x_lengths.to(device=x.device, dtype=torch.int32)
        if self.training:
            self._drop_seed += 1                                # one fresh set of dropout masks per training step
            if self._keys_dev is not None:                      # the same counter on the device, and the keys derived from it
                self._seed_dev.add_(1)
                K.make_keys(self._seed_dev, self._keys_dev)
        xh = self.logits(x, lens, causal=True)
        # next-token targets (transformer_lm.py:121-126): position t predicts x[t + 1]; pads / specials are not scored
        nxt = x[:, 1:]
        target = torch.full_like(x, -1)
        target[:, :-1] = torch.where(nxt >= TransformerLM.OFFSET, nxt - TransformerLM.OFFSET, -1)
        if self.loss_type == "ce":
            loss, accuracy, _ = K.cross_entropy(xh, target)
        elif self.loss_type == "mmi":
            loss, accuracy, _ = K.mmi_loss(xh, target)
        else:
            loss, accuracy, _ = K.focal_loss(xh, target, self.focal_gamma)
        if not self.training:
            keep = torch.arange(l - 1, device=x.device)[None, :] < lens[:, None]
            yh = self.reconstruct(xh[:, :-1, :].argmax(-1), keep[:, None, :])
        else:
            yh = None
        return {"loss": loss, "yh": yh}, {"accuracy": accuracy}

    # ------------------------------------------------------------------------------------------ incremental decoding
    def new_decode_state(self, batch_size, n_steps, device="cuda", uniforms=None):
        """A `smt_amd.lm.DecodeState` for `n_steps` tokens after <bos> (key/value cache of n_steps rows per layer)."""
        if not 1 <= batch_size <= 32:
            raise ValueError(f"incremental decoding runs batches of 1..32 (got {batch_size})")
        if n_steps < 1 or n_steps + 1 > self.pos_encoding.pe.shape[0]:
            raise ValueError(f"n_steps must be in 1..max_len - 1 = {self.pos_encoding.pe.shape[0] - 1} (got {n_steps})")
        layer = self.transformer.layers[0]
        st = K.DecodeState(batch_size, n_steps, self.d_model, layer.self_attn.num_heads, layer.linear1.out_features,
                           self.classifier.out_features, len(self.transformer.layers), device, TransformerLM.BOS, uniforms)
        if self.position == "rotary":
            # what decode_embed adds instead of the sinusoidal table: zeros, one row per position the state can reach, owned
            # by the state (captured launches keep pointing at them)
            st.pe = torch.zeros(n_steps, self.d_model, device=device, dtype=torch.float32)
        return st

    def _decode_logits(self, st):
        """The launches of one decoding step up to the classifier: the token at the state's position -> st.logits.  Fixed
        arguments only (the position is read from st.pos_dev), no allocation, no host synchronisation."""
        pd = st.pos_dev
        K.decode_embed(st.tokens, self.embedding.weight, st.pe if self.position == "rotary" else self.pos_encoding.table(), st.h, 0, pd)
        if self.norm_first:
            return self._decode_logits_pre(st)
        rope = self.rope
        for i, layer in enumerate(self.transformer.layers):
            sa, n1, n2 = layer.self_attn, layer.norm1, layer.norm2
            K.decode_linear(st.h, sa.in_proj_weight, sa.in_proj_bias, st.qkv)
            K.decode_attention(st.qkv, st.kv[i, 0], st.kv[i, 1], st.ctx, st.attn_ws, 0, pd, rope)
            K.decode_linear(st.ctx, sa.out_proj.weight, None, st.a)     # its bias goes through the LayerNorm kernel, as in forward
            K.decode_layer_norm(st.h, st.a, sa.out_proj.bias, n1.weight, n1.bias, n1.eps, st.h1, st.stats)
            K.decode_linear(st.h1, layer.linear1.weight, layer.linear1.bias, st.f, act=layer.act)
            K.decode_linear(st.f, layer.linear2.weight, None, st.a)
            K.decode_layer_norm(st.h1, st.a, layer.linear2.bias, n2.weight, n2.bias, n2.eps, st.h, st.stats)
        norm = self.transformer.norm
        K.decode_layer_norm(st.h, None, None, norm.weight, norm.bias, norm.eps, st.h1, st.stats)
        K.decode_linear(st.h1, self.classifier.weight, self.classifier.bias, st.logits)

    def _decode_logits_pre(self, st):
        """`_decode_logits` after the embedding for pre-norm layers, launch for launch the post-norm sequence: the stream
        alternates between st.h (a layer's input) and st.s (between its sub-layers), the normed rows are always st.h1."""
        pd = st.pos_dev
        layers, norm = self.transformer.layers, self.transformer.norm
        n1 = layers[0].norm1
        K.decode_layer_norm(st.h, None, None, n1.weight, n1.bias, n1.eps, st.h1, st.stats)
        for i, layer in enumerate(layers):
            sa, n2 = layer.self_attn, layer.norm2
            nxt = layers[i + 1].norm1 if i + 1 < len(layers) else norm
            K.decode_linear(st.h1, sa.in_proj_weight, sa.in_proj_bias, st.qkv)
            K.decode_attention(st.qkv, st.kv[i, 0], st.kv[i, 1], st.ctx, st.attn_ws, 0, pd, self.rope)
            K.decode_linear(st.ctx, sa.out_proj.weight, None, st.a)     # its bias goes through the LayerNorm kernel, as in forward
            K.decode_residual_layer_norm(st.h, st.a, sa.out_proj.bias, n2.weight, n2.bias, n2.eps, st.s, st.h1, st.stats)
            K.decode_linear(st.h1, layer.linear1.weight, layer.linear1.bias, st.f, act=layer.act)
            K.decode_linear(st.f, layer.linear2.weight, None, st.a)
            K.decode_residual_layer_norm(st.s, st.a, layer.linear2.bias, nxt.weight, nxt.bias, nxt.eps, st.h, st.h1, st.stats)
        K.decode_linear(st.h1, self.classifier.weight, self.classifier.bias, st.logits)

    def _decode_step(self, st, sigma, top_k=None, top_p=None):
        self._decode_logits(st)
        if top_k is None and top_p is None:
            K.decode_sample(st.logits, st.uniforms, st.tokens, st.codes, sigma, 0, st.pos_dev, TransformerLM.OFFSET)
        else:
            K.decode_sample_filtered(st.logits, st.uniforms, st.tokens, st.codes, sigma, top_k, top_p, st.kept, 0, st.pos_dev,
                                     TransformerLM.OFFSET)
        st.advance()

    def _check_prompt(self, codes, batch):
        """codes int64 [B, P] or [P] (broadcast over the batch), values in [0, vocab), P >= 1 -> [B, P]."""
        vocab = self.classifier.out_features
        if not torch.is_tensor(codes) or codes.dtype != torch.int64 or codes.dim() not in (1, 2):
            raise ValueError("prompt: an int64 tensor of codes, [batch, P] or [P]")
        if codes.dim() == 1:
            codes = codes[None, :].expand(batch, -1)
        if codes.shape[0] != batch or codes.shape[1] < 1:
            raise ValueError(f"prompt: shape [{batch}, P >= 1] or [P] expected (got {tuple(codes.shape)})")
        if int(codes.min()) < 0 or int(codes.max()) >= vocab:
            raise ValueError(f"prompt: codes must lie in [0, {vocab}) (no special-token offset)")
        return codes

    @torch.no_grad()
    def prefill(self, state, codes):
        """Hand a prompt of P codes (int64 [B, P] or [P], values in [0, vocab), the same length for every row) to a fresh
        decoding state in ONE batched pass: tokens[:, 1:P + 1] = codes + OFFSET, codes[:, :P] = codes, and tokens 0..P-1
        (<bos> and the first P - 1 codes) go through the kernels of `logits` in eval mode, every layer's keys and values
        landing in cache rows 0..P-1.  The last layer stops after its in-projection; the final norm and the classifier do
        not run.  Leaves the state at position P: the next `step_logits` / decoding step processes tokens[:, P], the last
        prompt code, and yields the logits of the first new code."""
        if self.training:
            raise ValueError("prefill: incremental decoding runs in eval mode (no dropout)")
        if state.pos != 0:
            raise ValueError(f"prefill: needs a state at position 0 (it is at {state.pos})")
        codes = self._check_prompt(codes, state.batch).to(state.tokens.device)
        p = codes.shape[1]
        if p > state.n_steps:
            raise ValueError(f"prefill: the state holds {state.n_steps + 1} tokens, <bos> and {p} prompt codes do not fit")
        state.tokens[:, 1:p + 1] = codes + TransformerLM.OFFSET
        state.codes[:, :p] = codes
        h = K.embed(state.tokens[:, :p].contiguous(), self.embedding.weight, self._embed_table(p), K.NO_DROP, TransformerLM.PAD)
        layers, rope = self.transformer.layers, self.rope
        if self.norm_first:
            n1 = layers[0].norm1
            pair = (h, K.add_layer_norm(h, None, n1.weight, n1.bias, n1.eps))
            for i, layer in enumerate(layers):
                last = i + 1 == len(layers)
                pair = layer.prefill_pre(*pair, None if last else layers[i + 1].norm1, state.kv[i, 0], state.kv[i, 1], last, rope)
        else:
            for i, layer in enumerate(layers):
                h = layer.prefill(h, state.kv[i, 0], state.kv[i, 1], i + 1 == len(layers), rope)
        state.prefill_done(p)

    @torch.no_grad()
    def step_logits(self, state):
        """Next-token logits [B, vocab] of the token at the state's position, given the cached keys / values of the positions
        before it: what `logits(x, None, causal=True)[:, pos]` computes from the whole prefix.  Neither samples nor advances;
        continue with `state.push(tokens)`."""
        if self.training:
            raise ValueError("step_logits: incremental decoding runs in eval mode (no dropout)")
        if state.pos >= state.n_steps:
            raise ValueError(f"step_logits: the state holds {state.n_steps} positions and all are used")
        self._decode_logits(state)
        return state.logits.clone()

    def _sample_causal(self, batch_size, n_steps, device, sigma, uniforms, generator, graph, prompt=None, top_k=None, top_p=None):
        if self.training:
            raise ValueError("sample(causal=True) runs in eval mode (no dropout)")
        if not sigma > 0:
            raise ValueError("Temperature scalar must be positive")
        if not 1 <= batch_size <= 32:
            raise ValueError(f"sample(causal=True) runs batches of 1..32 (got {batch_size})")
        if n_steps < 1 or n_steps + 1 > self.pos_encoding.pe.shape[0]:
            raise ValueError(f"n_steps must be in 1..max_len - 1 = {self.pos_encoding.pe.shape[0] - 1} (got {n_steps})")
        if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= self.classifier.out_features):
            raise ValueError(f"top_k must be an int in 1..vocab = {self.classifier.out_features} (got {top_k!r})")
        if top_p is not None and not 0.0 < top_p <= 1.0:
            raise ValueError(f"top_p must lie in (0, 1] (got {top_p!r})")
        n_prompt = 0
        if prompt is not None:
            prompt = self._check_prompt(prompt, batch_size)
            n_prompt = prompt.shape[1]
            if n_prompt + n_steps + 1 > self.pos_encoding.pe.shape[0]:
                raise ValueError(f"prompt ({n_prompt}) + n_steps ({n_steps}) + 1 exceeds max_len = {self.pos_encoding.pe.shape[0]}")
        if uniforms is None:
            uniforms = torch.rand(n_steps, batch_size, generator=generator, device=device if generator is None else generator.device)
        else:
            if generator is not None:
                raise ValueError("pass either uniforms or a generator")
            if not torch.is_tensor(uniforms) or uniforms.dtype != torch.float32 or tuple(uniforms.shape) != (n_steps, batch_size):
                raise ValueError(f"uniforms must be a float32 tensor of shape ({n_steps}, {batch_size})")
            if not bool(((uniforms >= 0) & (uniforms < 1)).all()):
                raise ValueError("uniforms must lie in [0, 1)")
        if n_prompt:                                            # position t draws with row t: the caller's rows follow the prompt's
            uniforms = torch.cat([torch.zeros(n_prompt, batch_size, dtype=torch.float32, device=device), uniforms.to(device)])
        st = self.new_decode_state(batch_size, n_prompt + n_steps, device, uniforms)
        if n_prompt:
            self.prefill(st, prompt)                            # eager, before any capture: the step below holds DecodeState buffers only
        eager = min(2, n_steps) if graph else n_steps           # a graphed run warms up with its first two steps
        for _ in range(eager):
            self._decode_step(st, sigma, top_k, top_p)
        if n_steps > eager:
            step = torch.cuda.CUDAGraph()
            with torch.cuda.graph(step):                        # one linear chain of launches on the capture stream
                self._decode_step(st, sigma, top_k, top_p)
            for _ in range(n_steps - eager):
                step.replay()
            st.pos = n_prompt + n_steps                         # the host mirror of what the replays did on the device
            torch.cuda.current_stream().synchronize()           # after the loop: the graph must outlive its last replay
        q = st.codes
        return self.reconstruct(q, torch.ones_like(q).unsqueeze(1)), q

    @torch.no_grad()
    def sample(self, batch_size, n_steps, device="cuda", sigma=1.0, *, causal=False, uniforms=None, generator=None, graph=False,
               prompt=None, top_k=None, top_p=None):
        """Ancestral sampling (transformer_lm.py:137-155).  As in the reference every step re-runs the whole prefix WITHOUT
        the causal mask (mask=None there), so a key/value cache cannot reproduce it; the step is one pass of `logits`.

        causal=True samples from the model as it was trained instead: every position sees only the positions before it, so a
        step is ONE new token against a key/value cache (csrc/lm_decode.hip) and the loop never synchronises with the host.
        The draws are inverse-CDF with `uniforms` [n_steps, batch_size] in [0, 1) (float32; drawn with torch.rand from
        `generator` or the global one when not given); graph=True replays one captured step instead of issuing the launches.
        `prompt` (int64 codes [batch_size, P] or [P], no special-token offset) is continued instead of starting at <bos>: it
        goes through `prefill` in one batched pass, P + n_steps + 1 <= max_len, and the returned codes [batch_size, P + n_steps]
        and audio hold the prompt followed by the n_steps new codes.  `top_k` (1..vocab) keeps the top_k most likely codes,
        `top_p` (0 < top_p <= 1) the shortest most-likely-first prefix of them that holds top_p of their mass; the draw is
        from the kept codes, renormalised (smt_lm_decode_sample_filtered in include/smt_hip.h has the exact rule).
        Returns (audio, codes) like the other path."""
        if causal:
            return self._sample_causal(batch_size, n_steps, device, sigma, uniforms, generator, graph, prompt, top_k, top_p)
        if uniforms is not None or generator is not None or graph or prompt is not None or top_k is not None or top_p is not None:
            raise ValueError("uniforms, generator, graph, prompt, top_k and top_p belong to sample(causal=True)")
        assert sigma > 0, "Temperature scalar must be positive"
        q = torch.full((batch_size, 1), TransformerLM.BOS, dtype=torch.long, device=device)
        for _ in range(n_steps):
            probs = F.softmax(self.logits(q, None, causal=False)[:, -1, :] / sigma, dim=-1)
            q = torch.cat([q, torch.multinomial(probs, 1)], dim=-1)
        q = q[:, 1:]
        return self.reconstruct(q, torch.ones_like(q).unsqueeze(1)), q
