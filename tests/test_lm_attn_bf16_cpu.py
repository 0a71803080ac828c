"""`model.attention_dtype: bf16` without a GPU: the float64 forms of tests/lm_attn_bf16_helpers.py and the a-priori bound the
kernel tests use (the rounded form sits inside it, four wrong answers leave it by more than a factor 10), the constructor's
refusals, the shipped config, and the two new C entries under the unchanged ABI version."""
import ctypes
import os

import pytest
import torch

import lm_attn_bf16_helpers as A
from oracle import lm_oracle as lmo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "speech-masters-thesis_amd")
OUTPUTS = ("ctx", "dq", "dk", "dv")


def _case(seed=0, b=2, heads=2, l=45, representable=True):
    g = torch.Generator().manual_seed(seed)
    d = heads * A.DH
    qkv = torch.randn(b, l, 3 * d, generator=g, dtype=torch.float64)
    dctx = torch.randn(b, l, d, generator=g, dtype=torch.float64)
    if representable:
        qkv, dctx = A.bf16(qkv), A.bf16(dctx)
    lens = torch.tensor([l, l - 7][:b])
    return qkv, dctx, lens


def _ratios(got_ctx, got_dqkv, exact):
    """Worst |error| / bound per output."""
    b_ctx, b_dqkv = A.bounds(exact)
    d = got_ctx.shape[-1]
    out = {"ctx": float(((got_ctx - exact["ctx"]).abs() / b_ctx.clamp_min(1e-300)).max())}
    r = (got_dqkv - exact["dqkv"]).abs() / b_dqkv.clamp_min(1e-300)
    out.update(dq=float(r[..., :d].max()), dk=float(r[..., d:2 * d].max()), dv=float(r[..., 2 * d:].max()))
    return out


def _rounded(qkv, dctx, lens, heads, causal, ks):
    leaf = qkv.clone().requires_grad_(True)
    ctx = A.RoundedAttention.apply(leaf, lens, heads, causal, ks)
    ctx.backward(dctx)
    return ctx.detach(), leaf.grad


@pytest.mark.parametrize("causal", [True, False])
def test_the_rounded_form_is_inside_the_bound(causal):
    qkv, dctx, lens = _case()
    ks = A.keep_scale(lmo.CounterDropout(seed=5, p=0.1), 1, 2, 2, 45)
    exact = A.attention_exact(qkv, lens, 2, causal, ks, dctx)
    ratios = _ratios(*_rounded(qkv, dctx, lens, 2, causal, ks), exact)
    print("  worst |rounded - exact| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert all(ratios[k] > 0.01 for k in OUTPUTS), ratios        # and the bound is not slack by orders of magnitude


@pytest.mark.parametrize("mutate", A.MUTATIONS)
def test_a_wrong_answer_leaves_the_bound_tenfold(mutate):
    """Another dropout key, V shifted by one row, the causal mask off by one, dq / dk without dS's 1 / sqrt(32)."""
    qkv, dctx, lens = _case()
    ks = A.keep_scale(lmo.CounterDropout(seed=5, p=0.1), 1, 2, 2, 45)
    other = A.keep_scale(lmo.CounterDropout(seed=6, p=0.1), 1, 2, 2, 45)
    exact = A.attention_exact(qkv, lens, 2, True, ks, dctx)
    wrong = A.attention_exact(qkv, lens, 2, True, ks, dctx, mutate=mutate, ks_other=other)
    ratios = _ratios(wrong["ctx"], wrong["dqkv"], exact)
    print(f"  {mutate}: worst |wrong - exact| / bound: " + ", ".join(f"{k} {v:.1f}" for k, v in ratios.items()))
    assert max(ratios.values()) > 10.0, ratios


def test_exact_form_is_the_oracles_attention_and_its_autograd():
    qkv, dctx, lens = _case(representable=False)
    drop = lmo.CounterDropout(seed=5, p=0.1)
    lens[1] = 38
    exact = A.attention_exact(qkv, lens, 2, True, A.keep_scale(drop, 3, 2, 2, 45), dctx)
    leaf = qkv.clone().requires_grad_(True)
    ctx = lmo.attention_core(leaf, lens, 2, True, drop, 3)
    ctx.backward(dctx)
    assert float((exact["ctx"] - ctx.detach()).abs().max()) < 1e-12
    assert float((exact["dqkv"] - leaf.grad).abs().max()) < 1e-12
    s = (exact["q"] @ exact["k"].transpose(-1, -2)) / A.DH ** 0.5
    s = s.masked_fill(~A.visible(2, 45, lens, True), float("-inf"))
    assert float((exact["lse"] - torch.logsumexp(s, -1) * A.LOG2E).abs().max()) < 1e-12


def test_rounded_form_differs_from_the_exact_one_by_its_roundings_only():
    """Dropout 0, bf16-representable inputs: the operand roundings do nothing, so replacing the three remaining roundings
    (p~, P and dS) by the identity must give the exact form; with them in place the two differ."""
    qkv, dctx, lens = _case(seed=3)
    exact = A.attention_exact(qkv, lens, 2, True, None, dctx)
    ctx_r, dqkv_r = _rounded(qkv, dctx, lens, 2, True, None)
    assert float((ctx_r - exact["ctx"]).abs().max()) > 1e-5 and float((dqkv_r - exact["dqkv"]).abs().max()) > 1e-5
    old = A.bf16
    A.bf16 = lambda t: t
    try:
        ctx_i, dqkv_i = _rounded(qkv, dctx, lens, 2, True, None)
    finally:
        A.bf16 = old
    assert float((ctx_i - exact["ctx"]).abs().max()) < 1e-12 and float((dqkv_i - exact["dqkv"]).abs().max()) < 1e-12
    # and the operand roundings are there: on plain inputs the rounded form is the rounded form of the rounded inputs
    qkv2, dctx2, _ = _case(seed=4, representable=False)
    a = _rounded(qkv2, dctx2, lens, 2, True, None)
    bq = A.bf16(qkv2)
    leaf = bq.clone().requires_grad_(True)
    ctx_b = A.RoundedAttention.apply(leaf, lens, 2, True, None)
    assert torch.equal(a[0], ctx_b.detach()) and not torch.equal(bq, qkv2)


def test_oracle_attention_swaps_the_core_and_restores_it():
    p = lmo.init_params(16, 64, 2, 128, 2, seed=1, dtype=torch.float64)
    x, lens = lmo.synthetic_tokens(2, 17, 16, seed=2)
    plain = lmo.lm_logits(x, lens, p, heads=2, num_layers=2)
    core = lmo.attention_core
    with A.oracle_attention(True):
        rounded = lmo.lm_logits(x, lens, p, heads=2, num_layers=2)
    with A.oracle_attention(False):
        same = lmo.lm_logits(x, lens, p, heads=2, num_layers=2)
    assert lmo.attention_core is core
    assert torch.equal(plain, same) and not torch.equal(plain, rounded)
    assert float((plain - rounded).abs().max()) < 0.5


def _config(**over):
    from utils import config as C
    cfg = C.load(os.path.join(PKG, "configs/models/transformer_lm.yaml"))
    cfg.model.update(C.create(dict(vocab_size=16, embed_dim=64, max_len=64, num_layers=2, d_model=64, nhead=2, dim_feedforward=128)))
    cfg.model.update(C.create(over))
    return cfg


def test_constructor_reads_attention_dtype_and_refuses_anything_else(monkeypatch):
    import torch.nn as nn
    from models.transformer_lm.transformer_lm import TransformerLM
    monkeypatch.setattr(TransformerLM, "load_vqvae", staticmethod(lambda log_dir, ckpt_num: nn.ModuleDict()))
    for over, want in (({}, torch.float32), (dict(attention_dtype="fp32"), torch.float32), (dict(attention_dtype="bf16"), torch.bfloat16),
                       (dict(attention_dtype="bf16", compute_dtype="bf16", norm_first=True, activation="gelu"), torch.bfloat16)):
        model = TransformerLM(_config(**over))
        assert model.attention_dtype == want
        assert all(layer.attention_dtype == want for layer in model.transformer.layers)
        assert model.compute_dtype == (torch.bfloat16 if over.get("compute_dtype") == "bf16" else torch.float32)
    for bad in ("fp16", "float32", True, 16):
        with pytest.raises(ValueError, match="attention_dtype"):
            TransformerLM(_config(attention_dtype=bad))


def test_binding_refuses_other_dtypes_before_touching_the_device():
    from smt_amd import lm as K
    qkv = torch.zeros(1, 4, 96)
    for bad in (torch.float16, torch.float64, "bf16", None):
        with pytest.raises(ValueError, match="compute_dtype"):
            K.attention(qkv, None, 1, True, compute_dtype=bad)


def test_shipped_config_is_the_bf16_config_plus_the_key():
    from utils import config as C
    base = C.load(os.path.join(PKG, "configs/models/transformer_lm_bf16.yaml")).to_dict()
    attn = C.load(os.path.join(PKG, "configs/models/transformer_lm_bf16_attn.yaml")).to_dict()
    assert attn["model"].pop("attention_dtype") == "bf16"
    assert attn == base and "attention_dtype" not in base["model"]


def test_header_and_library_export_the_two_entries_under_abi_10():
    from smt_amd import native
    with open(os.path.join(REPO, "include", "smt_hip.h")) as f:
        header = f.read()
    handle = ctypes.CDLL(native.LIB_PATH)
    for name in ("smt_lm_attention_bf16_fwd", "smt_lm_attention_bf16_bwd"):
        assert f"int {name}(" in header
        assert hasattr(handle, name) and name in native.exported_symbols()
    assert native.ABI_VERSION == 10 and handle.smt_abi_version() == 10
