"""Shared by tests/test_lm_prenorm_cpu.py and tests/test_lm_prenorm_gpu.py: the TransformerLM forward written out on the CPU
with the two switches of nn.TransformerEncoderLayer that oracle/lm_oracle.py does not have -- `norm_first` and `activation` --
and the product's dropout sites injected (oracle.lm_oracle.CounterDropout: site 0 the embedding, 1 + 4 i + {0, 1, 2, 3} layer
i's attention weights, attention output, feed-forward inner, feed-forward output).  Plain torch in any float dtype; gradients
come from autograd over it.  tests/test_lm_prenorm_cpu.py pins it on torch.nn.TransformerEncoder itself in float64, for all
four combinations, and shows that each of the `mutate` variants moves the logits far outside what the device tests allow.

Also the small-model plumbing of tests/test_lm_gpu.py (a throw-away VQ-VAE run directory, a config, a model on the device).
"""
import math
import os

import torch
import torch.nn.functional as F

from oracle import lm_oracle as lmo

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-masters-thesis_amd")
DEV = "cuda:0"
# the small size of the model tests: 3 layers so that a pre-norm stack has a first, a middle and a last layer
SMALL = dict(vocab_size=16, embed_dim=64, max_len=64, num_layers=3, d_model=64, nhead=2, dim_feedforward=128, dropout=0.0)
COMBOS = [(False, "relu"), (False, "gelu"), (True, "relu"), (True, "gelu")]
NEW_COMBOS = COMBOS[1:]
MUTATIONS = ("other_norm_order", "tanh_gelu", "no_final_norm", "norm1_for_norm2")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def activation_fn(name, mutate=None):
    if name == "relu":
        return F.relu
    if name == "gelu":
        return (lambda u: F.gelu(u, approximate="tanh")) if mutate == "tanh_gelu" else F.gelu
    raise ValueError(name)


def encoder_layer(x, p, pre, lens, heads, causal, drop, site0, norm_first, activation, linear=F.linear, mutate=None, eps=1e-5):
    """nn.TransformerEncoderLayer.forward, both norm orders (torch/nn/modules/transformer.py: `x = x + _sa_block(norm1(x))`,
    `x = x + _ff_block(norm2(x))` when norm_first, else `x = norm1(x + _sa_block(x))`, `x = norm2(x + _ff_block(x))`)."""
    d = x.shape[-1:]
    act = activation_fn(activation, mutate)

    def norm(t, which):
        if mutate == "norm1_for_norm2":
            which = "norm1"
        return F.layer_norm(t, d, p[pre + which + ".weight"], p[pre + which + ".bias"], eps)

    def sa(t):
        qkv = linear(t, p[pre + "self_attn.in_proj_weight"], p[pre + "self_attn.in_proj_bias"])
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


def lm_logits(x, lens, p, heads, num_layers, norm_first=False, activation="relu", final_eps=1e-5, causal=True, drop=None,
              linear=F.linear, mutate=None):
    """tokens [B, L] -> logits [B, L, vocab]; `mutate` (one of MUTATIONS) breaks it on purpose."""
    assert mutate is None or mutate in MUTATIONS
    drop = drop or lmo.CounterDropout()
    if mutate == "other_norm_order":
        norm_first = not norm_first
    emb = p["embedding.weight"]
    d = emb.shape[1]
    pe = lmo.positional_table(x.shape[1], d).to(emb.dtype)
    h = drop(0, F.embedding(x, emb) * math.sqrt(d) + pe[None])
    for i in range(num_layers):
        h = encoder_layer(h, p, f"transformer.layers.{i}.", lens, heads, causal, drop, 1 + 4 * i, norm_first, activation, linear, mutate)
    if mutate != "no_final_norm":
        h = F.layer_norm(h, (d,), p["transformer.norm.weight"], p["transformer.norm.bias"], final_eps)
    return linear(h, p["classifier.weight"], p["classifier.bias"])


def step64(x, lens, params, heads, num_layers, norm_first, activation, drop=None, linear=F.linear):
    """(loss, accuracy, logits, {name: grad}) of the float64 helper on float64 leaves made from `params`."""
    p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    logits = lm_logits(x, lens, p64, heads, num_layers, norm_first, activation, drop=drop, linear=linear)
    loss, acc = lmo.lm_loss(x, logits)
    loss.backward()
    return loss.detach(), acc.detach(), logits.detach(), {k: v.grad for k, v in p64.items()}


def torch_encoder(params, d_model, heads, ff, num_layers, norm_first, activation, dtype=torch.float64):
    """torch's own stack with `params` loaded: (nn.TransformerEncoder in train mode with dropout 0, its state-dict names
    mapped to ours).  batch_first, so that it takes the helper's [B, L, d] rows."""
    import torch.nn as nn
    layer = nn.TransformerEncoderLayer(d_model, heads, ff, dropout=0.0, activation=activation, layer_norm_eps=1e-5, batch_first=True,
                                       norm_first=norm_first, dtype=dtype)
    enc = nn.TransformerEncoder(layer, num_layers, norm=nn.LayerNorm(d_model, eps=1e-5, dtype=dtype), enable_nested_tensor=False)
    names = {k: "transformer." + k for k in enc.state_dict()}
    enc.load_state_dict({k: params[v].to(dtype) for k, v in names.items()})
    return enc.train(), names


def unpadded(lens, length):
    return torch.arange(length)[None, :] < lens[:, None]


# ------------------------------------------------------------------------------------------------ models on the device
def vqvae_run(tmp_path, l_bins=16):
    """A small VQ-VAE run directory (config.yaml + ckpts/ckpt.3.pt) for TransformerLM.load_vqvae."""
    from utils import config as C
    from utils.commons import get_model, get_optimizer, setup_logdir
    from utils.train_utils import save_checkpoint
    log_dir = str(tmp_path / "vqvae")
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/vqvae.yaml")),
                  C.load(os.path.join(PKG, "configs/datasets/synthetic_ljspeech.yaml")),
                  C.create({"train": {"batch_size": 2, "n_gpus": 1, "ema": False, "log_dir": log_dir, "num_workers": 0, "total_epochs": 1}}))
    cfg.model.update(C.create(dict(width=16, emb_width=32, l_bins=l_bins, multipliers=[1, 1, 1])))
    torch.manual_seed(0)
    setup_logdir(cfg)
    model, ema = get_model(cfg, DEV)
    opt, sched = get_optimizer(cfg, model)
    model.bottleneck.level_blocks[0].k.copy_(torch.randn(l_bins, 32, generator=torch.Generator().manual_seed(1)).to(DEV) * 0.3)
    save_checkpoint(cfg, 3, 0, model, ema, opt, sched)
    return log_dir, model


def lm_config(log_dir, base="transformer_lm.yaml", drop_keys=(), **over):
    from utils import config as C
    cfg = C.load(os.path.join(PKG, "configs/models", base))
    cfg.model.update(C.create(over))
    for key in drop_keys:
        del cfg.model[key]
    cfg.model.vqvae.log_dir, cfg.model.vqvae.ckpt_num = log_dir, 3
    return cfg


def build(tmp_path, params=None, log_dir=None, drop_keys=(), **over):
    """A TransformerLM on the device; `log_dir` reuses a VQ-VAE run written earlier, `drop_keys` removes keys from the config."""
    from models.transformer_lm.transformer_lm import TransformerLM
    if log_dir is None:
        log_dir, _ = vqvae_run(tmp_path, l_bins=over.get("vocab_size", 512))
    torch.manual_seed(0)
    model = TransformerLM(lm_config(log_dir, drop_keys=drop_keys, **over)).to(DEV)
    if params is not None:
        missing, unexpected = model.load_state_dict(dict(params), strict=False)
        assert not unexpected and all(k.startswith("vqvae.") or k == "pos_encoding.pe" for k in missing), (missing, unexpected)
    return model, log_dir


def named_grads(model):
    return {n: p.grad for n, p in model.named_parameters() if not n.startswith("vqvae.")}
