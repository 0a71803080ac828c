"""Pre-norm layers and GELU of the TransformerLM on the device (model.norm_first / model.activation; csrc/lm.hip
smt_lm_res_ln_* and smt_lm_bias_gelu_*, smt_lm_decode_linear act = 2) against float64: the two kernel pairs alone, the decoder
variant, the model in the three new combinations against tests/lm_prenorm_helpers.py (pinned on torch's own
nn.TransformerEncoder by tests/test_lm_prenorm_cpu.py, which also shows that each of these comparisons can fail), incremental
decoding, the bf16 option and train.py with the shipped pre-norm config.

Tolerances are the project's for the neighbouring kernels (tests/test_lm_gpu.py) and are stated at each assert."""
import os

import pytest
import torch
import torch.nn.functional as F

import lm_bf16_helpers as B
import lm_prenorm_helpers as H
from oracle import lm_oracle as lmo

pytestmark = pytest.mark.gpu
DEV = H.DEV
PRE_GELU = dict(norm_first=True, activation="gelu")


# ------------------------------------------------------------------------------------------------ residual add + LayerNorm
def _res_ln_case(rows, dim, p, with_bias, seed=9, site=2):
    g = torch.Generator().manual_seed(rows * 7 + dim)
    x, h = torch.randn(rows, dim, generator=g), torch.randn(rows, dim, generator=g) * 2
    hb = torch.randn(dim, generator=g) if with_bias else None
    gamma, beta = 1 + 0.2 * torch.randn(dim, generator=g), 0.2 * torch.randn(dim, generator=g)
    gamma[3] = 0.0                                                  # a dead scale: its xhat must still reach dgamma
    ds, dy = torch.randn(rows, dim, generator=g), torch.randn(rows, dim, generator=g)
    return (x, h, gamma, beta, hb), ds, dy


def _res_ln_ref(tensors, p, ds, dy, seed=9, site=2):
    """float64: (s, y, [gradients of x, h, gamma, beta, h_bias]; None where the tensor is absent, zeros where no gradient arrives)."""
    leaves = [t.double().requires_grad_(True) if t is not None else None for t in tensors]
    x, h, gamma, beta, hb = leaves
    s = x + lmo.CounterDropout(seed=seed, p=p)(site, h + (hb if hb is not None else 0))
    y = F.layer_norm(s, (x.shape[-1],), gamma, beta, 1e-5)
    total = (s * ds.double()).sum() if ds is not None else 0
    total = total + ((y * dy.double()).sum() if dy is not None else 0)
    total.backward()
    grads = [None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t)) for t in leaves]
    return s.detach(), y.detach(), grads


def _res_ln_dev(tensors, p, ds, dy, seed=9, site=2):
    from smt_amd import lm as K
    dev = [t.to(DEV).requires_grad_(True) if t is not None else None for t in tensors]
    s, y = K.residual_layer_norm(dev[0], dev[1], dev[2], dev[3], 1e-5, K.Drop(p, True, seed, site), h_bias=dev[4])
    outs = [o for o, go in ((s, ds), (y, dy)) if go is not None]
    torch.autograd.backward(outs, [go.to(DEV) for go in (ds, dy) if go is not None])
    return s.detach(), y.detach(), [None if t is None else t.grad for t in dev]


@pytest.mark.parametrize("with_bias,p", [(True, 0.1), (True, 0.0), (False, 0.1), (False, 0.0)])
@pytest.mark.parametrize("rows,dim", [(37, 64), (130, 512), (5, 768), (3, 2048)])
def test_residual_layer_norm_kernel(rows, dim, with_bias, p):
    """Forward and backward against float64 with both incoming gradients, the stream's only and the normed output's only.
    add_layer_norm's tolerances: outputs atol 2e-5, gradients atol 1e-4 / rtol 1e-4; the stream itself is one add and one
    multiply away from its inputs: atol 1e-6.  37 rows leave a workgroup three-quarters empty, 768 is PER = 12."""
    tensors, ds, dy = _res_ln_case(rows, dim, p, with_bias)
    for name, gs, gy in (("both", ds, dy), ("ds only", ds, None), ("dy only", None, dy)):
        s64, y64, want = _res_ln_ref(tensors, p, gs, gy)
        s, y, got = _res_ln_dev(tensors, p, gs, gy)
        assert torch.allclose(s.cpu(), s64.float(), atol=1e-6, rtol=0), (name, float((s.cpu() - s64.float()).abs().max()))
        assert torch.allclose(y.cpu(), y64.float(), atol=2e-5, rtol=0), (name, float((y.cpu() - y64.float()).abs().max()))
        for which, mine, ref in zip(("x", "h", "gamma", "beta", "h_bias"), got, want):
            assert (mine is None) == (ref is None), (name, which)
            if mine is not None:
                assert torch.allclose(mine.cpu(), ref.float(), atol=1e-4, rtol=1e-4), (name, which, float((mine.cpu() - ref.float()).abs().max()))


def test_residual_layer_norm_is_bit_reproducible_and_leaves_its_inputs_alone():
    tensors, ds, dy = _res_ln_case(130, 512, 0.1, True)
    first, second = _res_ln_dev(tensors, 0.1, ds, dy), _res_ln_dev(tensors, 0.1, ds, dy)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    for a, b in zip(first[2], second[2]):
        assert torch.equal(a, b)
    other = _res_ln_dev(tensors, 0.1, ds, dy, seed=10)             # another key: another mask
    assert not torch.equal(first[0], other[0])


def test_residual_layer_norm_empty_and_unbuilt_width():
    from smt_amd import lm as K
    from smt_amd import native as N
    e = torch.empty(0, 64, device=DEV, requires_grad=True)
    gamma, beta, hb = (torch.ones(64, device=DEV, requires_grad=True), torch.zeros(64, device=DEV, requires_grad=True),
                       torch.zeros(64, device=DEV, requires_grad=True))
    s, y = K.residual_layer_norm(e, e * 1.0, gamma, beta, 1e-5, K.NO_DROP, h_bias=hb)
    assert s.shape == y.shape == (0, 64)
    (s.sum() + y.sum()).backward()
    for t in (gamma, beta, hb):                                     # rows = 0: no launch, the parameter gradients are zeroed
        assert t.grad.shape == (64,) and float(t.grad.abs().max()) == 0.0
    assert N.lib().smt_lm_res_ln_bwd_workspace_bytes(0, 512) == 0
    x = torch.randn(4, 320, device=DEV)
    with pytest.raises(RuntimeError, match="res_ln: dim 320 not built"):
        K.residual_layer_norm(x, x.clone(), torch.ones(320, device=DEV), torch.zeros(320, device=DEV))


# ------------------------------------------------------------------------------------------------ bias + GELU + dropout
GELU_BOUND = 1e-6       # |err| <= GELU_BOUND * max(1, |u|): bias_relu's 1e-6 scaled by magnitude, 8 * 2^-23 of max(|u|, 1)


def _gelu_case(rows, dim):
    """u = h + bias spread over [-6, 6], with exact zeros of both signs among them."""
    g = torch.Generator().manual_seed(rows + dim)
    u = torch.rand(rows, dim, generator=g) * 12 - 6
    bias = torch.randn(dim, generator=g) * 0.3
    bias[0], bias[1] = 0.0, -0.0
    h = u - bias
    h[0, :] = -bias                                                 # u = +0 along a row
    h[1, 0], h[1, 1], h[2, 0], h[2, 1] = 0.0, -0.0, -0.0, 0.0       # +0 + +0, -0 + -0 = -0, -0 + +0, +0 + -0
    da = torch.randn(rows, dim, generator=g)
    return h, bias, da


@pytest.mark.parametrize("rows,dim,p", [(50, 128, 0.1), (7, 256, 0.0), (2064, 2048, 0.1)])
def test_bias_gelu_dropout_kernel(rows, dim, p):
    """The exact (erf) GELU against float64.  Forward |err| <= 1e-6 max(1, |u|); backward dh to the same bound times |da|;
    dbias atol 1e-3 / rtol 1e-5 as for bias_relu; h is not modified.  (The tanh form is 4.7e-4 away.)"""
    from smt_amd import lm as K
    h, bias, da = _gelu_case(rows, dim)
    h64, b64 = h.double().requires_grad_(True), bias.double().requires_grad_(True)
    u = (h64 + b64).detach()
    ref = lmo.CounterDropout(seed=4, p=p)(6, F.gelu(h64 + b64))
    ref.backward(da.double())
    hg, bg = h.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    out = K.bias_gelu_dropout(hg, bg, K.Drop(p, True, 4, 6))
    out.backward(da.to(DEV))
    assert out.data_ptr() != hg.data_ptr() and torch.equal(hg.detach().cpu(), h)        # not in place
    scale = u.abs().clamp_min(1.0)
    fwd = float(((out.detach().cpu().double() - ref.detach()).abs() / scale).max())
    bwd = float(((hg.grad.cpu().double() - h64.grad).abs() / (scale * da.double().abs().clamp_min(1e-30))).max())
    cpu32 = float(((F.gelu(h + bias).double() - F.gelu(u)).abs() / scale).max())
    print(f"  ({rows}, {dim}, p {p}): forward {fwd:.3e}, backward {bwd:.3e} of max(1, |u|) (float32 CPU F.gelu: {cpu32:.3e})")
    assert fwd <= GELU_BOUND and bwd <= GELU_BOUND
    assert torch.allclose(bg.grad.cpu(), b64.grad.float(), atol=1e-3, rtol=1e-5)
    if p > 0:
        gone = (ref.detach() == 0) & (u != 0)                       # what the mask dropped (float64 GELU is 0 only at u = 0)
        assert 0.08 < float(gone.float().mean()) < 0.12 and float(out.detach().cpu()[gone].abs().max()) == 0.0
        assert float(hg.grad.cpu()[gone].abs().max()) == 0.0        # dropped elements: exactly zero, value and gradient
    again = K.bias_gelu_dropout(hg.detach(), bg.detach(), K.Drop(p, True, 4, 6))
    assert torch.equal(again, out.detach())
    assert K.bias_gelu_dropout(torch.empty(0, dim, device=DEV), bg.detach()).shape == (0, dim)


# ------------------------------------------------------------------------------------------------ decoder
@pytest.mark.parametrize("b,k,n", [(3, 64, 128), (32, 512, 2048)])
def test_decode_linear_with_gelu(b, k, n):
    """act = 2 against float64: the pre-activation carries the fp32 dot-product bound of tests/test_lm_decode_gpu.py,
    K 2^-23 max|x| max|W|, which the GELU (slope <= 1.13) passes on at most 1.13-fold, plus the activation's own
    1e-6 max(1, |u|).  act = 0 / 1 are the launches of relu = False / True, bit for bit."""
    from smt_amd import lm as K
    g = torch.Generator().manual_seed(1000 * b + k + n)
    x, w, bias = torch.randn(b, k, generator=g), torch.randn(n, k, generator=g) * k ** -0.5, torch.randn(n, generator=g)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    u = x.double() @ w.double().t() + bias.double()
    got = K.decode_linear(xd, wd, bd, act=2).cpu().double()
    bound = 1.13 * k * 2.0 ** -23 * float(x.abs().max()) * float(w.abs().max()) + GELU_BOUND * u.abs().clamp_min(1.0)
    assert bool(((got - F.gelu(u)).abs() <= bound).all()), float((got - F.gelu(u)).abs().max())
    assert float((got - F.gelu(u, approximate="tanh")).abs().max()) > 1e-4             # and it is not the tanh form
    assert torch.equal(K.decode_linear(xd, wd, bd, act=0), K.decode_linear(xd, wd, bd, relu=False))
    assert torch.equal(K.decode_linear(xd, wd, bd, act=1), K.decode_linear(xd, wd, bd, relu=True))
    assert torch.equal(K.decode_linear(xd, wd, None, act=K.ACT_GELU), K.decode_linear(xd, wd, None, act=2))
    with pytest.raises(RuntimeError, match="act must be"):
        K.decode_linear(xd, wd, bd, act=3)
    with pytest.raises(ValueError, match="contradict"):
        K.decode_linear(xd, wd, bd, relu=True, act=2)


# ------------------------------------------------------------------------------------------------ model, small size
@pytest.fixture(scope="module")
def small_case():
    """Weights and batch of the small model tests, and the float64 helper's results per combination, computed once."""
    p32 = lmo.init_params(16, 64, 2, 128, 3, seed=21)
    x, lens = lmo.synthetic_tokens(4, 33, 16, seed=22)
    cache = {}

    def ref(norm_first, activation, p):
        key = (norm_first, activation, p)
        if key not in cache:
            cache[key] = H.step64(x, lens, p32, 2, 3, norm_first, activation, drop=lmo.CounterDropout(seed=41, p=p))
        return cache[key]

    return p32, x, lens, ref


@pytest.mark.parametrize("norm_first,activation", H.NEW_COMBOS)
def test_small_model_matches_the_float64_helper(tmp_path, small_case, norm_first, activation):
    """The test that needs the feature: the constructor refused both keys before.  Train mode, dropout 0.1 at every site
    with the masks restated by the helper: loss 2e-5, accuracy 1e-6, every parameter gradient 1e-3 rel-L2 (the figures of the
    post-norm dropout test).  Dropout 0: logits atol 1e-4 on the unpadded positions."""
    p32, x, lens, ref = small_case
    model, log_dir = H.build(tmp_path, p32, **dict(H.SMALL, dropout=0.1, norm_first=norm_first, activation=activation))
    assert model.norm_first is norm_first
    model.train()
    model._drop_seed = 40
    loss_dict, metrics = model(x.to(DEV), lens.to(DEV), None, None)
    loss_dict["loss"].backward()
    loss, acc, _, grads = ref(norm_first, activation, 0.1)          # forward bumped the seed to 41
    print(f"  loss {float(loss_dict['loss'].detach()):.7f} vs {float(loss):.7f}")
    assert abs(float(loss_dict["loss"]) - float(loss)) < 2e-5 and abs(float(metrics["accuracy"]) - float(acc)) < 1e-6
    for name, grad in H.named_grads(model).items():
        assert H.rel(grad, grads[name]) < 1e-3, (name, H.rel(grad, grads[name]))

    plain, _ = H.build(tmp_path, p32, log_dir=log_dir, **dict(H.SMALL, norm_first=norm_first, activation=activation))
    plain.train()
    with torch.no_grad():
        logits = plain.logits(x.to(DEV), lens.to(DEV, torch.int32))
    _, _, logits64, _ = ref(norm_first, activation, 0.0)
    keep = H.unpadded(lens, 33)
    err = float((logits.cpu().double() - logits64)[keep].abs().max())
    print(f"  logits max |err| {err:.3e}")
    assert err <= 1e-4


def test_torch_prenorm_gelu_state_dict_loads_and_computes_the_same(tmp_path):
    """The state dict of nn.TransformerEncoder(norm_first=True, activation="gelu") under `transformer.`: no unexpected key,
    nothing of the stack missing, and the logits are the helper's on those weights (which is torch's own forward)."""
    p32 = lmo.init_params(16, 64, 2, 128, 3, seed=5)
    enc, names = H.torch_encoder(p32, 64, 2, 128, 3, True, "gelu", dtype=torch.float32)
    sd = {"transformer." + k: v for k, v in enc.state_dict().items()}
    model, _ = H.build(tmp_path, **dict(H.SMALL, **PRE_GELU))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith("transformer.")], (missing, unexpected)
    model.load_state_dict({k: v for k, v in p32.items() if not k.startswith("transformer.")}, strict=False)
    x, lens = lmo.synthetic_tokens(3, 21, 16, seed=6)
    model.eval()
    with torch.no_grad():
        got = model.logits(x.to(DEV), lens.to(DEV, torch.int32))
    want = H.lm_logits(x, lens, {k: v.double() for k, v in p32.items()}, 2, 3, True, "gelu")
    assert float((got.cpu().double() - want)[H.unpadded(lens, 21)].abs().max()) <= 1e-4


def test_other_activations_are_refused_by_name(tmp_path):
    with pytest.raises(ValueError, match="model.activation"):
        H.build(tmp_path, **dict(H.SMALL, activation="tanh"))
    with pytest.raises(ValueError, match="model.norm_first"):
        H.build(tmp_path, log_dir=str(tmp_path / "vqvae"), **dict(H.SMALL, norm_first="yes"))


def test_absent_keys_are_the_post_norm_relu_path_bit_for_bit(tmp_path):
    """A config without the two keys and one that spells out norm_first: false, activation: relu: the same logits and the same
    gradients, bit for bit, in train mode with dropout.  (Each code appears twice in the batch: the embedding gradient adds
    colliding rows with atomics, and a sum of two terms does not depend on their order.)"""
    p32 = lmo.init_params(16, 64, 2, 128, 3, seed=21)
    g = torch.Generator().manual_seed(3)
    x = torch.stack([torch.cat([torch.tensor([lmo.BOS]), torch.randperm(16, generator=g) + lmo.OFFSET]) for _ in range(2)])
    lens = torch.tensor([17, 17])
    results, log_dir = [], None
    for drop_keys, over in ((("norm_first", "activation"), {}), ((), dict(norm_first=False, activation="relu"))):
        model, log_dir = H.build(tmp_path, p32, log_dir=log_dir, drop_keys=drop_keys, **dict(H.SMALL, dropout=0.1, **over))
        assert model.norm_first is False
        model.train()
        model._drop_seed = 7
        logits = model.logits(x.to(DEV), lens.to(DEV, torch.int32)).detach().clone()
        loss_dict, _ = model(x.to(DEV), lens.to(DEV), None, None)
        loss_dict["loss"].backward()
        results.append((logits, loss_dict["loss"].detach(), H.named_grads(model)))
    (la, lossa, ga), (lb, lossb, gb) = results
    assert torch.equal(la, lb) and torch.equal(lossa, lossb) and set(ga) == set(gb)
    for name in ga:
        assert torch.equal(ga[name], gb[name]), name


# ------------------------------------------------------------------------------------------------ decoding, pre-norm + GELU
@pytest.fixture()
def decoder(tmp_path):
    model, _ = H.build(tmp_path, lmo.init_params(16, 64, 2, 128, 3, seed=71), **dict(H.SMALL, **PRE_GELU))
    return model.eval()


def test_step_logits_and_prefill_equal_the_full_prefix_pass(decoder):
    """step_logits at every position of a 20-token sequence, and prefill of 7 codes followed by step_logits, against
    logits(x, None, causal=True)[:, pos]: atol 2e-5 (fp32 both ways, different summation orders)."""
    model = decoder
    x, _ = lmo.synthetic_tokens(3, 20, 16, seed=72, ragged=False)
    xd = x.to(DEV)
    with torch.no_grad():
        full = model.logits(xd, None, causal=True)
    st = model.new_decode_state(3, 20, DEV)
    for t in range(20):
        got = model.step_logits(st)
        assert float((got - full[:, t]).abs().max()) <= 2e-5, t
        if t + 1 < 20:
            st.push(x[:, t + 1])
    st = model.new_decode_state(3, 20, DEV)
    model.prefill(st, x[:, 1:8] - lmo.OFFSET)                       # <bos> and 6 codes go through the batched pass
    assert st.pos == 7
    for t in range(7, 20):
        got = model.step_logits(st)
        assert float((got - full[:, t]).abs().max()) <= 2e-5, t
        if t + 1 < 20:
            st.push(x[:, t + 1])


def test_causal_sample_is_the_hand_replay_of_its_uniforms(decoder):
    from smt_amd import lm as K
    model = decoder
    u = torch.rand(12, 3, generator=torch.Generator().manual_seed(8)).to(DEV)
    audio, q = model.sample(3, 12, DEV, sigma=0.9, causal=True, uniforms=u)
    st = model.new_decode_state(3, 12, DEV, u)
    for _ in range(12):
        logits = model.step_logits(st)
        K.decode_sample(logits, st.uniforms, st.tokens, st.codes, 0.9, pos=st.pos, token_offset=lmo.OFFSET)
        st.advance()
    assert torch.equal(q, st.codes) and audio.shape == (3, 12 * 128) and bool(torch.isfinite(audio).all())
    _, q2 = model.sample(3, 12, DEV, sigma=0.9, causal=True, uniforms=u, prompt=q[:, :5], top_k=8, top_p=0.9)
    assert q2.shape == (3, 17) and torch.equal(q2[:, :5], q[:, :5])
    torch.manual_seed(0)
    _, q3 = model.sample(2, 4, DEV)                                 # the reference's un-causal loop
    assert q3.shape == (2, 4) and int(q3.min()) >= 0 and int(q3.max()) < 16


# ------------------------------------------------------------------------------------------------ bf16, train.py
def test_bf16_composes_with_prenorm_gelu(tmp_path, small_case):
    """compute_dtype bf16 with pre-norm + GELU: finite loss and gradients, and the loss within twice the distance between the
    float64 helper with rounded operands (tests/lm_bf16_helpers.RoundedLinear) and the exact float64 helper."""
    p32, x, lens, ref = small_case
    exact, _, _, _ = ref(True, "gelu", 0.1)
    rounded, _, _, _ = H.step64(x, lens, p32, 2, 3, True, "gelu", drop=lmo.CounterDropout(seed=41, p=0.1),
                                linear=lambda t, w, b=None: B.RoundedLinear.apply(t, w, b))
    model, _ = H.build(tmp_path, p32, **dict(H.SMALL, dropout=0.1, compute_dtype="bf16", **PRE_GELU))
    assert model.compute_dtype == torch.bfloat16
    model.train()
    model._drop_seed = 40
    loss_dict, _ = model(x.to(DEV), lens.to(DEV), None, None)
    loss_dict["loss"].backward()
    loss = float(loss_dict["loss"])
    yard = abs(float(rounded) - float(exact))
    print(f"  loss |err|: yardstick {yard:.3e}, device {abs(loss - float(exact)):.3e} (allowed 2 x yardstick)")
    assert torch.isfinite(loss_dict["loss"]) and all(bool(torch.isfinite(g).all()) for g in H.named_grads(model).values())
    assert abs(loss - float(exact)) <= 2.0 * yard


def test_train_py_with_the_prenorm_config(tmp_path, monkeypatch):
    """`train.py --model transformer_lm_prenorm --dataset vqlatent` at a small size on generated codes: a finite loss and a
    checkpoint whose config carries both keys."""
    import json
    import math
    import train
    from scripts import generate_vq_dataset as G
    from utils import config as C
    log_vq, _ = H.vqvae_run(tmp_path, l_bins=16)
    dump_dir = str(tmp_path / "VQ-Latent")
    ds_cfg = C.load(os.path.join(log_vq, "config.yaml"))
    ds_cfg.dataset.update(C.create(dict(num_clips=6, ragged=True)))
    C.save(ds_cfg, os.path.join(log_vq, "config.yaml"))
    G.main(["--log_dir", log_vq, "--ckpt_num", "3", "--dump_dir", dump_dir, "--batch_size", "3", "--n_processes", "1", "--n_workers", "0"])
    monkeypatch.chdir(H.PKG)
    cfg = H.lm_config(log_vq, base="transformer_lm_prenorm.yaml", **H.SMALL)
    assert cfg.model.norm_first is True and cfg.model.activation == "gelu"
    C.save(cfg, "configs/models/_test_lm_prenorm.yaml")
    vql = C.load("configs/datasets/vqlatent.yaml")
    vql.dataset.update(C.create(dict(dataset_path=dump_dir, segment_length=24)))
    C.save(vql, "configs/datasets/_test_vql_prenorm.yaml")
    try:
        log_dir = str(tmp_path / "run")
        argv = ["--model", "_test_lm_prenorm", "--dataset", "_test_vql_prenorm", "--batch_size", "3", "--num_workers", "0",
                "--total_epochs", "1", "--log_every_n_steps", "1", "--ckpt_every_n_steps", "2", "--eval_every_n_epochs", "1",
                "--log_dir", log_dir, "--n_gpus", "1"]
        train.main(argv)
        last = torch.load(os.path.join(log_dir, "ckpts", "ckpt.last.pt"), weights_only=True)
        assert last["step"] == 2 and "transformer.layers.2.norm2.weight" in last["model"]
        assert all(bool(torch.isfinite(v).all()) for k, v in last["model"].items() if k.startswith("transformer."))
        saved = C.load(os.path.join(log_dir, "config.yaml")).model
        assert saved.norm_first is True and saved.activation == "gelu"
        scal = os.path.join(log_dir, "scalars.jsonl")
        if os.path.exists(scal):
            losses = [json.loads(line) for line in open(scal)]
            losses = [r["value"] for r in losses if r["tag"] == "loss/train_loss"]
            assert losses and all(math.isfinite(v) for v in losses)
    finally:
        os.remove("configs/models/_test_lm_prenorm.yaml")
        os.remove("configs/datasets/_test_vql_prenorm.yaml")
