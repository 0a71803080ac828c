"""The CPU yardstick of the pre-norm / GELU TransformerLM (tests/lm_prenorm_helpers.py) against torch's own
nn.TransformerEncoder, and the proof that the device tests of tests/test_lm_prenorm_gpu.py can fail: every deliberate mistake
the helper can make moves the checked quantity at least ten times further than the device tests allow.  No GPU."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import lm_prenorm_helpers as H
from oracle import lm_oracle as lmo

PKG = H.PKG
LOGITS_ATOL = 1e-4                  # tests/test_lm_prenorm_gpu.py: model logits against the float64 helper
GELU_BOUND_CEILING = 1e-5           # the same file: the bias_gelu_dropout bound, |err| <= c * max(1, |u|), may never exceed this c


def _torch_logits(x, lens, p64, enc, names, d):
    """The model around torch's stack: embedding * sqrt(d) + positions, causal + key-padding masks, classifier."""
    l = x.shape[1]
    h = F.embedding(x, p64["embedding.weight"]) * math.sqrt(d) + lmo.positional_table(l, d).double()[None]
    causal = torch.triu(torch.ones(l, l, dtype=torch.bool), diagonal=1)
    h = enc(h, mask=causal, src_key_padding_mask=~H.unpadded(lens, l))
    return F.linear(h, p64["classifier.weight"], p64["classifier.bias"])


@pytest.mark.parametrize("norm_first,activation", H.COMBOS)
def test_helper_is_torchs_transformer_encoder_in_float64(norm_first, activation):
    """d 64, 2 heads, ff 128, 3 layers, 3 x 21 ragged: logits on the unpadded positions and every parameter gradient of the
    next-token loss equal torch.nn.TransformerEncoder(norm_first, activation, enable_nested_tensor=False) in train mode with
    dropout 0, to 1e-10 (float64 both sides; the two differ in the order of a few sums only)."""
    d, heads, ff, layers, vocab = 64, 2, 128, 3, 16
    params = lmo.init_params(vocab, d, heads, ff, layers, seed=11, dtype=torch.float64)
    x, lens = lmo.synthetic_tokens(3, 21, vocab, seed=12)
    loss, _, logits, grads = H.step64(x, lens, params, heads, layers, norm_first, activation)

    enc, names = H.torch_encoder(params, d, heads, ff, layers, norm_first, activation)
    p64 = {k: v.clone().requires_grad_(True) for k, v in params.items() if not k.startswith("transformer.")}
    want = _torch_logits(x, lens, p64, enc, names, d)
    want_loss, _ = lmo.lm_loss(x, want)
    want_loss.backward()
    want_loss = want_loss.detach()
    keep = H.unpadded(lens, 21)
    err = float((logits - want.detach())[keep].abs().max())
    print(f"  norm_first={norm_first} {activation}: max |dlogits| {err:.3e}, |dloss| {abs(float(loss) - float(want_loss)):.3e}")
    assert err <= 1e-10 and abs(float(loss) - float(want_loss)) <= 1e-10
    want_grads = {k: v.grad for k, v in p64.items()}
    want_grads.update({names[k]: v.grad for k, v in enc.named_parameters()})
    assert set(want_grads) == set(grads)
    for name, g in grads.items():
        assert float((g - want_grads[name]).abs().max()) <= 1e-10, name


def _small_case():
    params = lmo.init_params(16, 64, 2, 128, 3, seed=21, dtype=torch.float64)
    x, lens = lmo.synthetic_tokens(4, 33, 16, seed=22)
    return params, x, lens


@pytest.mark.parametrize("mutate", ["other_norm_order", "no_final_norm", "norm1_for_norm2"])
@pytest.mark.parametrize("norm_first,activation", H.NEW_COMBOS)
def test_a_wrong_norm_moves_the_logits_ten_tolerances(norm_first, activation, mutate):
    """At the size and weights of the device's model test, the wrong norm order, a dropped final norm and norm1's parameters
    where norm2's belong each move some unpadded logit by >= 10 x the 1e-4 that test allows."""
    params, x, lens = _small_case()
    keep = H.unpadded(lens, 33)
    with torch.no_grad():
        good = H.lm_logits(x, lens, params, 2, 3, norm_first, activation)
        bad = H.lm_logits(x, lens, params, 2, 3, norm_first, activation, mutate=mutate)
    moved = float((good - bad)[keep].abs().max())
    print(f"  norm_first={norm_first} {activation} {mutate}: max |dlogits| {moved:.3e}")
    assert moved >= 10 * LOGITS_ATOL


def test_the_tanh_gelu_is_caught_by_the_kernel_bound_not_by_the_logits():
    """The tanh approximation moves the small model's logits by about the model tolerance itself (printed below), so the
    model tests cannot tell the two forms apart and do not claim to.  The quantity that pins the form is the activation: over
    u in [-6, 6] the tanh form is >= 10 x further from the erf form than the largest bound the kernel test may ever use
    (1e-5 * max(1, |u|); it uses 1e-6 unless the float32 erf needs more)."""
    u = torch.linspace(-6, 6, 240001, dtype=torch.float64)
    gap = ((H.activation_fn("gelu", "tanh_gelu")(u) - F.gelu(u)).abs() / u.abs().clamp_min(1.0)).max()
    params, x, lens = _small_case()
    keep = H.unpadded(lens, 33)
    with torch.no_grad():
        for norm_first in (False, True):
            moved = (H.lm_logits(x, lens, params, 2, 3, norm_first, "gelu") - H.lm_logits(x, lens, params, 2, 3, norm_first, "gelu", mutate="tanh_gelu"))
            print(f"  norm_first={norm_first}: tanh-GELU moves the logits by {float(moved[keep].abs().max()):.3e}")
    print(f"  max |tanh gelu - erf gelu| / max(1, |u|) = {float(gap):.3e}")
    assert float(gap) >= 10 * GELU_BOUND_CEILING


def test_relu_post_norm_helper_is_the_pinned_oracle():
    """With both switches at their defaults the helper is oracle.lm_oracle.lm_logits, which the reference's fixture pins."""
    params, x, lens = _small_case()
    drop = lmo.CounterDropout(seed=3, p=0.1)
    with torch.no_grad():
        assert torch.equal(H.lm_logits(x, lens, params, 2, 3, drop=drop), lmo.lm_logits(x, lens, params, heads=2, num_layers=3, drop=drop))


def test_prenorm_config_is_the_shipped_model_with_the_two_keys_set():
    from utils import config as C
    base = C.load(os.path.join(PKG, "configs/models/transformer_lm.yaml")).to_dict()
    pre = C.load(os.path.join(PKG, "configs/models/transformer_lm_prenorm.yaml")).to_dict()
    assert base["model"]["norm_first"] is False and base["model"]["activation"] == "relu"
    assert pre["model"].pop("norm_first") is True and pre["model"].pop("activation") == "gelu"
    base["model"].pop("norm_first"), base["model"].pop("activation")
    assert pre == base
