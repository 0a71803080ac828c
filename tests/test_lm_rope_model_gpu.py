"""The TransformerLM with rotary positions (model.position: rotary) on the device against the float64 helper of
tests/lm_rope_helpers.py: logits, loss and gradients in both norm orders and at both head dims, the bf16 options, incremental
decoding (step_logits, prefill, sample, the captured step), the launch counts, checkpoints, the config keys and train.py.

Small models as in tests/lm_prenorm_helpers.py: vocab 16, 2 layers, L = 21 with ragged lengths; d_model 64 with 2 heads (head dim
32) and d_model 128 with 2 heads (head dim 64).  Tolerances are the neighbouring tests' and are stated at each assert."""
import json
import math
import os

import pytest
import torch

import lm_attn_bf16_helpers as A
import lm_bf16_helpers as B
import lm_prenorm_helpers as H
import lm_rope_helpers as R
from oracle import lm_oracle as lmo

pytestmark = pytest.mark.gpu
DEV = H.DEV
LAYERS, LEN = 2, 21
SMALL = {32: dict(H.SMALL, num_layers=LAYERS, position="rotary"),
         64: dict(H.SMALL, num_layers=LAYERS, position="rotary", embed_dim=128, d_model=128)}
# (norm_first, activation, head dim): both norm orders at head dim 32, one case at 64
CASES = [(False, "relu", 32), (True, "gelu", 32), (False, "relu", 64)]


def _params(dh, seed):
    return lmo.init_params(16, 2 * dh, 2, 128, LAYERS, seed=seed)


@pytest.fixture(scope="module")
def vq_dir(tmp_path_factory):
    """One throw-away VQ-VAE run directory for every model of this module."""
    return H.vqvae_run(tmp_path_factory.mktemp("rope"), l_bins=16)[0]


@pytest.fixture(scope="module")
def batch():
    return lmo.synthetic_tokens(3, LEN, 16, seed=52)


@pytest.fixture(scope="module")
def ref(batch):
    """The float64 helper's (loss, accuracy, logits, gradients) per case and dropout rate, computed once."""
    x, lens = batch
    cache = {}

    def get(norm_first, activation, dh, p, **kwargs):
        key = (norm_first, activation, dh, p, tuple(sorted(kwargs)))
        if key not in cache:
            cache[key] = R.step64(x, lens, _params(dh, 51), 2, LAYERS, norm_first, activation, drop=lmo.CounterDropout(seed=41, p=p), **kwargs)
        return cache[key]

    return get


def _build(tmp_path, vq_dir, dh, params=None, **over):
    model, _ = H.build(tmp_path, params, log_dir=vq_dir, **dict(SMALL[dh], **over))
    return model


@pytest.mark.parametrize("norm_first,activation,dh", CASES)
def test_small_model_matches_the_float64_helper(tmp_path, vq_dir, batch, ref, norm_first, activation, dh):
    """Train mode, dropout 0.1 at every site with the masks restated by the helper: loss 2e-5, accuracy 1e-6, every parameter
    gradient 1e-3 rel-L2 (test_lm_prenorm_gpu's figures).  Dropout 0: logits atol 1e-4 on the unpadded positions."""
    x, lens = batch
    p32 = _params(dh, 51)
    model = _build(tmp_path, vq_dir, dh, p32, dropout=0.1, norm_first=norm_first, activation=activation)
    assert model.position == "rotary" and model.rope.shape == (64, dh // 2, 2)
    model.train()
    model._drop_seed = 40
    loss_dict, metrics = model(x.to(DEV), lens.to(DEV), None, None)
    loss_dict["loss"].backward()
    loss, acc, _, grads = ref(norm_first, activation, dh, 0.1)      # forward bumped the seed to 41
    print(f"  loss {float(loss_dict['loss'].detach()):.7f} vs {float(loss):.7f}")
    assert abs(float(loss_dict["loss"]) - float(loss)) < 2e-5 and abs(float(metrics["accuracy"]) - float(acc)) < 1e-6
    for name, grad in H.named_grads(model).items():
        assert H.rel(grad, grads[name]) < 1e-3, (name, H.rel(grad, grads[name]))

    plain = _build(tmp_path, vq_dir, dh, p32, norm_first=norm_first, activation=activation)
    plain.train()
    with torch.no_grad():
        logits = plain.logits(x.to(DEV), lens.to(DEV, torch.int32))
    _, _, logits64, _ = ref(norm_first, activation, dh, 0.0)
    err = float((logits.cpu().double() - logits64)[H.unpadded(lens, LEN)].abs().max())
    print(f"  logits max |err| {err:.3e}")
    assert err <= 1e-4


def test_rotary_logits_differ_from_the_sinusoidal_model_on_the_same_weights(tmp_path, vq_dir, batch, ref):
    """The test that needs the feature: a constructor that ignores the key builds the sinusoidal model twice."""
    x, lens = batch
    p32 = _params(32, 51)
    rotary = _build(tmp_path, vq_dir, 32, p32).eval()
    sinus = _build(tmp_path, vq_dir, 32, p32, position="sinusoidal").eval()
    assert rotary.position == "rotary" and sinus.position == "sinusoidal" and sinus.rope is None
    with torch.no_grad():
        a, b = rotary.logits(x.to(DEV), lens.to(DEV, torch.int32)), sinus.logits(x.to(DEV), lens.to(DEV, torch.int32))
    keep = H.unpadded(lens, LEN)
    assert float((a - b).cpu()[keep].abs().max()) > 1e-2
    want = H.lm_logits(x, lens, {k: v.double() for k, v in p32.items()}, 2, LAYERS)
    assert float((b.cpu().double() - want)[keep].abs().max()) <= 1e-4          # the sinusoidal one is still the sinusoidal helper's
    # un-causal (what sample(causal=False) runs) goes through the same rotation
    with torch.no_grad():
        c = rotary.logits(x.to(DEV), lens.to(DEV, torch.int32), causal=False)
    want = R.lm_logits(x, lens, {k: v.double() for k, v in p32.items()}, 2, LAYERS, causal=False)
    assert float((c.cpu().double() - want)[keep].abs().max()) <= 1e-4


def test_bf16_projections_compose_with_rotary_positions(tmp_path, vq_dir, batch, ref):
    """compute_dtype bf16, pre-norm + GELU: finite loss and gradients, the loss within twice the distance between the float64
    helper with rounded operands (tests/lm_bf16_helpers.RoundedLinear) and the exact one (test_lm_prenorm_gpu's bf16 yardstick)."""
    x, lens = batch
    exact = ref(True, "gelu", 32, 0.1)[0]
    rounded = ref(True, "gelu", 32, 0.1, linear=lambda t, w, b=None: B.RoundedLinear.apply(t, w, b))[0]
    model = _build(tmp_path, vq_dir, 32, _params(32, 51), dropout=0.1, compute_dtype="bf16", norm_first=True, activation="gelu")
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


def test_bf16_attention_composes_with_rotary_positions(tmp_path, vq_dir, batch):
    """attention_dtype bf16 (head dim 32): logits within twice the rounded-attention helper's own distance from the exact one
    (+ 1e-6), the rule of tests/test_lm_attn_bf16_model_gpu.py; the rotation itself stays fp32 in front of the rounding."""
    x, lens = batch
    p64 = {k: v.double() for k, v in _params(32, 51).items()}
    exact = R.lm_logits(x, lens, p64, 2, LAYERS)
    with A.oracle_attention(True):
        rounded = R.lm_logits(x, lens, p64, 2, LAYERS)
    model = _build(tmp_path, vq_dir, 32, _params(32, 51), attention_dtype="bf16").eval()
    with torch.no_grad():
        logits = model.logits(x.to(DEV), lens.to(DEV, torch.int32))
    keep = H.unpadded(lens, LEN)
    yard, err = float((rounded - exact)[keep].abs().max()), float((logits.cpu().double() - exact)[keep].abs().max())
    print(f"  logits max |err|: yardstick {yard:.3e}, device {err:.3e} (allowed 2 x yardstick + 1e-6)")
    assert err <= 2.0 * yard + 1e-6


# ------------------------------------------------------------------------------------------------ decoding
@pytest.fixture(params=[(False, "relu", 32), (True, "gelu", 64)], ids=["post-relu-dh32", "pre-gelu-dh64"])
def decoder(request, tmp_path, vq_dir):
    norm_first, activation, dh = request.param
    return _build(tmp_path, vq_dir, dh, _params(dh, 71), norm_first=norm_first, activation=activation).eval()


def test_step_logits_and_prefill_equal_the_full_prefix_pass(decoder):
    """step_logits at every position of a 20-token sequence, and prefill of P = 1 and 5 codes followed by step_logits up to 20,
    against logits(x, None, causal=True)[:, t]: atol 2e-5 (fp32 both ways, different summation orders)."""
    model = decoder
    x, _ = lmo.synthetic_tokens(3, 20, 16, seed=72, ragged=False)
    with torch.no_grad():
        full = model.logits(x.to(DEV), None, causal=True)
    worst = 0.0
    for n_prompt in (0, 1, 5):
        st = model.new_decode_state(3, 20, DEV)
        if n_prompt:
            model.prefill(st, x[:, 1:n_prompt + 1] - lmo.OFFSET)
            assert st.pos == n_prompt
        for t in range(n_prompt, 20):
            got = model.step_logits(st)
            err = float((got - full[:, t]).abs().max())
            worst = max(worst, err)
            assert err <= 2e-5, (n_prompt, t, err)
            if t + 1 < 20:
                st.push(x[:, t + 1])
    print(f"  worst |step - full| = {worst:.3e}")


def test_causal_sample_is_the_hand_replay_of_its_uniforms_and_the_graph_is_the_eager_loop(decoder):
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
    u6 = u[:6].contiguous()
    audio_e, q_e = model.sample(3, 6, DEV, sigma=0.9, causal=True, uniforms=u6)
    audio_g, q_g = model.sample(3, 6, DEV, sigma=0.9, causal=True, uniforms=u6, graph=True)
    assert torch.equal(q_e, q_g) and torch.equal(audio_e, audio_g) and torch.equal(q_e, q[:, :6])
    torch.manual_seed(0)
    _, q3 = model.sample(2, 4, DEV)                                 # the reference's un-causal loop, through `logits`
    assert q3.shape == (2, 4) and int(q3.min()) >= 0 and int(q3.max()) < 16


# ------------------------------------------------------------------------------------------------ launch counts
class _CountingLib:
    """The ctypes handle with every entry that launches counted by name (size queries and the error string are not)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.endswith("_workspace_bytes") or name in ("smt_last_error", "smt_abi_version"):
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)

        return counted


def _count(monkeypatch, fn):
    from smt_amd import native as N
    lib = _CountingLib(N.lib())
    with monkeypatch.context() as m:
        m.setattr(N, "lib", lambda: lib)
        fn()
    return lib.calls


@pytest.mark.parametrize("norm_first", [False, True])
def test_launch_counts_at_the_binding_layer(tmp_path, vq_dir, batch, monkeypatch, norm_first):
    """A rotary decoding step issues exactly the entries of a sinusoidal one (the rotation rides in the attention launch); a
    rotary training forward issues one more per layer (smt_lm_rope), and its backward one more per layer."""
    x, lens = batch
    p32 = _params(32, 51)
    calls = {}
    for position in ("sinusoidal", "rotary"):
        model = _build(tmp_path, vq_dir, 32, p32, position=position, norm_first=norm_first)
        model.eval()
        st = model.new_decode_state(3, 8, DEV)
        model._decode_step(st, 1.0)                                 # warm: nothing lazy is left for the counted step
        step = _count(monkeypatch, lambda: model._decode_step(st, 1.0))
        model.train()
        out = []
        fwd = _count(monkeypatch, lambda: out.append(model.logits(x.to(DEV), lens.to(DEV, torch.int32))))
        bwd = _count(monkeypatch, lambda: out[0].sum().backward())
        calls[position] = (step, fwd, bwd)
    (step_s, fwd_s, bwd_s), (step_r, fwd_r, bwd_r) = calls["sinusoidal"], calls["rotary"]
    print(f"  decoding step: {len(step_s)} entries; training forward: {len(fwd_s)} -> {len(fwd_r)}; backward: {len(bwd_s)} -> {len(bwd_r)}")
    assert len(step_r) == len(step_s)
    assert [n.replace("smt_lm_decode_attention_rope", "smt_lm_decode_attention_hd") for n in step_r] == step_s
    assert step_r.count("smt_lm_decode_attention_rope") == LAYERS and "smt_lm_rope" not in step_r
    assert len(fwd_r) == len(fwd_s) + LAYERS and fwd_r.count("smt_lm_rope") == LAYERS and "smt_lm_rope" not in fwd_s
    assert [n for n in fwd_r if n != "smt_lm_rope"] == fwd_s
    assert len(bwd_r) == len(bwd_s) + LAYERS and bwd_r.count("smt_lm_rope") == LAYERS


# ------------------------------------------------------------------------------------------------ checkpoints, config, train.py
def test_a_sinusoidal_checkpoint_loads_into_a_rotary_model_and_back(tmp_path, vq_dir):
    sinus = _build(tmp_path, vq_dir, 32, _params(32, 5), position="sinusoidal")
    rotary = _build(tmp_path, vq_dir, 32, _params(32, 6))
    sd_s, sd_r = sinus.state_dict(), rotary.state_dict()
    assert list(sd_s) == list(sd_r) and all(sd_s[k].shape == sd_r[k].shape for k in sd_s)
    assert "pos_encoding.pe" in sd_r and not any("rope" in k for k in sd_r)
    table = rotary.rope.clone()
    rotary.load_state_dict(sd_s, strict=True)
    assert torch.equal(rotary.rope, table)
    assert torch.equal(rotary.transformer.layers[1].linear1.weight, sinus.transformer.layers[1].linear1.weight)
    sinus.load_state_dict({k: v.clone() for k, v in sd_r.items()}, strict=True)
    absent = _build(tmp_path, vq_dir, 32, position="sinusoidal", drop_keys=("position",))
    assert absent.position == "sinusoidal" and absent.rope is None


def test_position_and_rope_base_are_validated_by_name(tmp_path, vq_dir):
    from smt_amd import lm as K
    for bad in ("learned", "rope", True, 1):
        with pytest.raises(ValueError, match="model.position.*" + repr(bad).replace("'", ".")):
            _build(tmp_path, vq_dir, 32, position=bad)
    for bad in (1.0, 0.5, -10000.0, float("inf"), float("nan"), "10000", True):
        with pytest.raises(ValueError, match="model.rope_base"):
            _build(tmp_path, vq_dir, 32, rope_base=bad)
    model = _build(tmp_path, vq_dir, 32, rope_base=500)
    assert torch.equal(model.rope.cpu(), K.rope_table(64, 32, 500.0))
    assert not model.rope.requires_grad and "rope" not in dict(model.named_parameters())
    assert _build(tmp_path, vq_dir, 32, position="sinusoidal", rope_base=500).rope is None      # read with rotary only


def test_train_py_with_the_rotary_config(tmp_path, monkeypatch):
    """`train.py --model transformer_lm_rope --dataset vqlatent` at a small size on generated codes (the tiny run directory of the
    pre-norm test): two steps, finite losses, a checkpoint whose config carries the key."""
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
    cfg = H.lm_config(log_vq, base="transformer_lm_rope.yaml", **H.SMALL)
    assert cfg.model.position == "rotary"
    C.save(cfg, "configs/models/_test_lm_rope.yaml")
    vql = C.load("configs/datasets/vqlatent.yaml")
    vql.dataset.update(C.create(dict(dataset_path=dump_dir, segment_length=24)))
    C.save(vql, "configs/datasets/_test_vql_rope.yaml")
    try:
        log_dir = str(tmp_path / "run")
        argv = ["--model", "_test_lm_rope", "--dataset", "_test_vql_rope", "--batch_size", "3", "--num_workers", "0",
                "--total_epochs", "1", "--log_every_n_steps", "1", "--ckpt_every_n_steps", "2", "--eval_every_n_epochs", "1",
                "--log_dir", log_dir, "--n_gpus", "1"]
        train.main(argv)
        last = torch.load(os.path.join(log_dir, "ckpts", "ckpt.last.pt"), weights_only=True)
        assert last["step"] == 2 and "pos_encoding.pe" in last["model"] and not any("rope" in k for k in last["model"])
        assert all(bool(torch.isfinite(v).all()) for k, v in last["model"].items() if k.startswith("transformer."))
        assert C.load(os.path.join(log_dir, "config.yaml")).model.position == "rotary"
        scal = os.path.join(log_dir, "scalars.jsonl")
        if os.path.exists(scal):
            losses = [json.loads(line) for line in open(scal)]
            losses = [r["value"] for r in losses if r["tag"] == "loss/train_loss"]
            assert losses and all(math.isfinite(v) for v in losses)
    finally:
        os.remove("configs/models/_test_lm_rope.yaml")
        os.remove("configs/datasets/_test_vql_rope.yaml")
