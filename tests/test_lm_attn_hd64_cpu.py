"""Head dim 64 without a GPU: the head-dim-parametrised float64 forms of tests/lm_attn_hd_helpers.py (at 32 they are
tests/lm_attn_bf16_helpers.py's, at 64 the oracle's attention and its autograd; the rounded form sits inside the a-priori
bound and four wrong answers leave it tenfold), the binding's refusal of other head dims, the shipped config and the new C
entries under the unchanged ABI version."""
import ctypes
import os

import pytest
import torch

import lm_attn_bf16_helpers as A32
import lm_attn_hd_helpers as A
from oracle import lm_oracle as lmo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "speech-masters-thesis_amd")
OUTPUTS = ("ctx", "dq", "dk", "dv")
NEW_ENTRIES = ("smt_lm_attention_hd_fwd", "smt_lm_attention_hd_bwd", "smt_lm_decode_attention_hd",
               "smt_lm_decode_attention_hd_workspace_bytes", "smt_lm_decode_prefill_kv_hd")


def _case(dh, seed=0, b=2, heads=2, l=45, representable=True):
    g = torch.Generator().manual_seed(seed)
    d = heads * dh
    qkv = torch.randn(b, l, 3 * d, generator=g, dtype=torch.float64)
    dctx = torch.randn(b, l, d, generator=g, dtype=torch.float64)
    if representable:
        qkv, dctx = A.bf16(qkv), A.bf16(dctx)
    return qkv, dctx, torch.tensor([l, l - 7][:b])


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


def test_at_head_dim_32_the_parametrised_forms_are_the_old_modules():
    qkv, dctx, lens = _case(32, representable=False)
    ks = A.keep_scale(lmo.CounterDropout(seed=5, p=0.1), 1, 2, 2, 45)
    other = A.keep_scale(lmo.CounterDropout(seed=6, p=0.1), 1, 2, 2, 45)
    for causal, mutate in [(True, None), (False, None)] + [(True, m) for m in A.MUTATIONS]:
        old = A32.attention_exact(qkv, lens, 2, causal, ks, dctx, mutate=mutate, ks_other=other)
        new = A.attention_exact(qkv, lens, 2, causal, ks, dctx, mutate=mutate, ks_other=other)
        assert new.pop("dh") == 32 and set(new) == set(old)
        assert all(torch.equal(new[n], old[n]) for n in old), (causal, mutate)
        if mutate is None:
            new["dh"] = 32
            assert all(torch.equal(x, y) for x, y in zip(A.bounds(new), A32.bounds(old)))
    leaf = qkv.clone().requires_grad_(True)
    ctx = A32.RoundedAttention.apply(leaf, lens, 2, True, ks)
    ctx.backward(dctx)
    mine = _rounded(qkv, dctx, lens, 2, True, ks)
    assert torch.equal(mine[0], ctx.detach()) and torch.equal(mine[1], leaf.grad)


def test_at_head_dim_64_the_exact_form_is_the_oracles_attention_and_its_autograd():
    qkv, dctx, lens = _case(64, representable=False)
    drop = lmo.CounterDropout(seed=5, p=0.1)
    lens[1] = 38
    exact = A.attention_exact(qkv, lens, 2, True, A.keep_scale(drop, 3, 2, 2, 45), dctx)
    assert exact["dh"] == 64 and exact["q"].shape == (2, 2, 45, 64)
    leaf = qkv.clone().requires_grad_(True)
    ctx = lmo.attention_core(leaf, lens, 2, True, drop, 3)
    ctx.backward(dctx)
    assert float((exact["ctx"] - ctx.detach()).abs().max()) < 1e-12
    assert float((exact["dqkv"] - leaf.grad).abs().max()) < 1e-12
    s = (exact["q"] @ exact["k"].transpose(-1, -2)) / 8.0
    s = s.masked_fill(~A.visible(2, 45, lens, True), float("-inf"))
    assert float((exact["lse"] - torch.logsumexp(s, -1) * A.LOG2E).abs().max()) < 1e-12


@pytest.mark.parametrize("causal", [True, False])
def test_at_head_dim_64_the_rounded_form_is_inside_the_bound(causal):
    qkv, dctx, lens = _case(64)
    ks = A.keep_scale(lmo.CounterDropout(seed=5, p=0.1), 1, 2, 2, 45)
    exact = A.attention_exact(qkv, lens, 2, causal, ks, dctx)
    ratios = _ratios(*_rounded(qkv, dctx, lens, 2, causal, ks), exact)
    print("  worst |rounded - exact| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert all(ratios[k] > 0.01 for k in OUTPUTS), ratios        # and the bound is not slack by orders of magnitude


@pytest.mark.parametrize("mutate", A.MUTATIONS)
def test_at_head_dim_64_a_wrong_answer_leaves_the_bound_tenfold(mutate):
    """Another dropout key, V shifted by one row, the causal mask off by one, dq / dk without dS's 1 / sqrt(64)."""
    qkv, dctx, lens = _case(64)
    ks = A.keep_scale(lmo.CounterDropout(seed=5, p=0.1), 1, 2, 2, 45)
    other = A.keep_scale(lmo.CounterDropout(seed=6, p=0.1), 1, 2, 2, 45)
    exact = A.attention_exact(qkv, lens, 2, True, ks, dctx)
    wrong = A.attention_exact(qkv, lens, 2, True, ks, dctx, mutate=mutate, ks_other=other)
    ratios = _ratios(wrong["ctx"], wrong["dqkv"], exact)
    print(f"  {mutate}: worst |wrong - exact| / bound: " + ", ".join(f"{k} {v:.1f}" for k, v in ratios.items()))
    assert max(ratios.values()) > 10.0, ratios


def test_oracle_attention_swaps_the_core_at_head_dim_64_and_restores_it():
    p = lmo.init_params(16, 128, 2, 128, 2, seed=1, dtype=torch.float64)
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


def test_binding_refuses_other_head_dims_before_touching_the_device():
    from smt_amd import lm as K
    assert K.HEAD_DIMS == (32, 64)
    for d, heads in ((48, 1), (128, 1), (96, 2), (16, 1), (100, 3)):
        with pytest.raises(AssertionError, match="head dim 32 or 64"):
            K.attention(torch.zeros(1, 4, 3 * d), None, heads)
        with pytest.raises(AssertionError, match="head dim 32"):
            K.DecodeState(1, 4, d, heads, 64, 16, 1, "cpu")
    for dh in (48, 128):
        cache = torch.zeros(1, 1, 4, dh)
        with pytest.raises(AssertionError, match="head dim 32 or 64"):
            K.decode_attention(torch.zeros(1, 3 * dh), cache, cache.clone(), torch.zeros(1, dh))
        with pytest.raises(AssertionError, match="head dim 32 or 64"):
            K.decode_prefill_kv(torch.zeros(1, 2, 3 * dh), cache, cache.clone())
        with pytest.raises(AssertionError, match="head dim 32 or 64"):
            K.decode_attention_workspace(1, 1, 600, "cpu", head_dim=dh)
    assert K._attn_flops(2, 3, 10, True, 2) == 2 * 3 * 55 * 64 * 2 == K._attn_flops(2, 3, 10, True, 2, 32)
    assert K._attn_flops(2, 3, 10, False, 5, 64) == 2 * 3 * 100 * 128 * 5


def test_constructor_accepts_what_it_accepted_and_eight_heads(monkeypatch):
    """The head-dim check stays at the call: d_model 48 with 3 heads still constructs, and so does d_model 128 with 2."""
    import torch.nn as nn
    from models.transformer_lm.transformer_lm import TransformerLM
    from utils import config as C
    monkeypatch.setattr(TransformerLM, "load_vqvae", staticmethod(lambda log_dir, ckpt_num: nn.ModuleDict()))
    for d, heads in ((48, 3), (128, 2), (64, 2)):
        cfg = C.load(os.path.join(PKG, "configs/models/transformer_lm_h8.yaml"))
        cfg.model.update(C.create(dict(vocab_size=16, embed_dim=d, max_len=64, num_layers=2, d_model=d, nhead=heads, dim_feedforward=128)))
        model = TransformerLM(cfg)
        assert all(layer.self_attn.num_heads == heads for layer in model.transformer.layers)


def test_shipped_config_is_the_base_config_with_eight_heads():
    from utils import config as C
    base = C.load(os.path.join(PKG, "configs/models/transformer_lm.yaml")).to_dict()
    h8 = C.load(os.path.join(PKG, "configs/models/transformer_lm_h8.yaml")).to_dict()
    assert base["model"]["nhead"] == 16 and h8["model"]["nhead"] == 8 and h8["model"]["d_model"] == 512
    h8["model"]["nhead"] = 16
    assert h8 == base


def test_header_and_library_export_the_new_entries_under_abi_10():
    from smt_amd import native
    with open(os.path.join(REPO, "include", "smt_hip.h")) as f:
        header = f.read()
    handle = ctypes.CDLL(native.LIB_PATH)
    for name in NEW_ENTRIES:
        assert f" {name}(" in header
        assert hasattr(handle, name) and name in native.exported_symbols()
    assert native.ABI_VERSION == 10 and handle.smt_abi_version() == 10
    ws = native.lib().smt_lm_decode_attention_hd_workspace_bytes
    assert ws(3, 2, 600, 64) == 3 * 2 * 3 * 68 * 4 and ws(3, 2, 600, 32) == native.lib().smt_lm_decode_attention_workspace_bytes(3, 2, 600)
    assert ws(3, 2, 256, 64) == 0 and ws(3, 2, 600, 48) == 0
