"""Multi-speaker GlowTTS (n_speakers > 1) on the GPU: against the reference's own multi-speaker run
(tests/golden/glow_tts_speakers.npz and glow_tts_speakers_grads.npz, written by tests/golden/make_golden_glow_speakers.py with the
two repairs the reference needs), the model API (forward / infer / infer_step with speakers and every
refusal), the single-speaker model left as it was, and train.py + scripts.synthesize end to end on the multi-speaker corpus.

Tolerances against the fixture are those of test_glow_tts_matches_the_reference_golden: losses rtol 1e-5, every gradient's
relative L2 <= 2e-3 with the same floor, eval yh atol 2e-4.  The fixture's parameters are float16-representable and stored
without loss; its gradients are stored as float16 of grad / max|grad| (about 1.5e-4 relative L2 of their own), and the 2e-3
bound is applied to the stored values as it stands.  The stored run is the reference in float64: in float32 the reference's
own rounding of one exactly-zero gradient (a key bias; 8.6e-8 against the floor of 1e-6 x 42.6) is a relative error of 2.02e-3,
so a product that computed the exact value would have missed the 2e-3 bound against it (make_golden_glow_speakers.py asserts
that the two runs agree)."""
import os

import numpy as np
import pytest
import torch

from oracle import glow_oracle as go

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-masters-thesis_amd")
DEV = "cuda"
INFER_TOL = 1e-5      # MODEL_TOL of tests/test_glow_infer_gpu.py (max-abs / max)


def _config(n_speakers, gin, extra=None):
    from utils import config as C
    tree = {"model": dict(n_speakers=n_speakers, gin_channels=gin, encoder=dict(go.GOLDEN_CFG["encoder"]), decoder=dict(go.GOLDEN_CFG["decoder"])),
            "dataset": dict(n_mels=8, intersperse_blanks=False, cmudict_path="")}
    tree.update(extra or {})
    return C.create(tree)


def _params(g):
    return {k[len("param."):]: torch.from_numpy(g[k]).float() for k in g if k.startswith("param.")}


@pytest.fixture(scope="module")
def fixture_model(golden):
    """The fixture's model (4 speakers, gin 16) with the fixture's parameters, and the fixture."""
    from models.glow_tts.glow_tts import GlowTTS
    g = golden("glow_tts_speakers")
    model = GlowTTS(_config(4, 16)).to(DEV)
    params = _params(g)
    assert set(model.state_dict()) == set(params)                      # the reference's state-dict names, all of them
    model.load_state_dict(params, strict=True)
    model.encoder.pre.p_dropout = 0.0           # the prenet's dropout is 0.1 whatever the config says; the fixture switched it off
    return model, g


def _batch(g):
    return [torch.from_numpy(g[k]).to(DEV) for k in ("tokens", "x_lens", "y", "y_lens")]


def test_multi_speaker_glow_tts_matches_the_reference(fixture_model, golden):
    model, g = fixture_model
    gg = golden("glow_tts_speakers_grads")
    assert g["param.emb_g.weight"].shape == (4, 16) and g["param.encoder.proj_w.conv_1.weight"].shape == (128, 80, 3)
    assert model.encoder.dp_width == 128                                    # 80 input channels run as 128: 48 zero columns
    tokens, x_lens, y, y_lens = _batch(g)
    speaker = torch.from_numpy(g["speaker"]).to(DEV)
    assert speaker.tolist() == [2, 0, 2]
    model.train()
    model.zero_grad()
    loss_dict, metrics = model.supervised_step([tokens, x_lens, y, y_lens, None, None, speaker])
    assert metrics == {} and loss_dict["yh"] is None
    loss_dict["loss"].backward()
    model.check_speaker_ids()                                               # ids in range: nothing to report
    print(f"\n[glow_tts speakers] loss_mle {loss_dict['loss_mle'].item():.6f} (ref {float(g['loss_mle']):.6f}), "
          f"loss_length {loss_dict['loss_length'].item():.6f} (ref {float(g['loss_length']):.6f})")
    worst = (0.0, "")
    refs = {k[len("grad."):]: torch.from_numpy(gg[k]).double() * float(gg["gscale." + k[len("grad."):]]) for k in gg if k.startswith("grad.")}
    assert set(refs) == {n for n, _ in model.named_parameters()}
    gmax = max(float(v.norm()) for v in refs.values())
    errs = {}
    for name, prm in model.named_parameters():
        assert prm.grad is not None, name
        errs[name] = float((prm.grad.double().cpu() - refs[name]).norm() / (refs[name].norm() + 1e-6 * gmax))
        worst = max(worst, (errs[name], name))
    print(f"  worst gradient rel-L2 {worst}; emb_g {errs['emb_g.weight']:.2e}; "
          f"cond_layer {max(v for k, v in errs.items() if 'cond_layer' in k):.2e}; proj_w.conv_1 {errs['encoder.proj_w.conv_1.weight']:.2e}")
    assert np.isclose(loss_dict["loss_mle"].item(), float(g["loss_mle"]), rtol=1e-5)
    assert np.isclose(loss_dict["loss_length"].item(), float(g["loss_length"]), rtol=1e-5)
    for name, e in errs.items():
        assert e <= 2e-3, (name, e)
    eg = model.emb_g.weight.grad.cpu()
    assert (eg[[1, 3]] == 0).all() and (eg[[0, 2]].abs().sum(1) > 0).all()         # only the speakers present have a gradient

    model.eval()
    noise = torch.from_numpy(g["eval_noise"]).to(DEV)
    with torch.no_grad():
        ev, _ = model(tokens, x_lens, y, y_lens, speaker=speaker, noise=noise)
        ev2, _ = model(tokens, x_lens, y, y_lens, speaker=torch.from_numpy(g["speaker_2"]).to(DEV), noise=noise)
    ref, ref2 = torch.from_numpy(g["eval_yh"]), torch.from_numpy(g["eval_yh_2"])
    print(f"  eval yh max-abs error {float((ev['yh'].cpu() - ref).abs().max()):.2e} / second speaker vector "
          f"{float((ev2['yh'].cpu() - ref2).abs().max()):.2e}")
    assert ev["yh"].shape == ref.shape and torch.allclose(ev["yh"].cpu(), ref, atol=2e-4)
    assert ev2["yh"].shape == ref2.shape and torch.allclose(ev2["yh"].cpu(), ref2, atol=2e-4)
    assert float((ev["yh"] - ev2["yh"]).abs().max()) > 1e-2                      # another voice, another spectrogram
    assert np.isclose(ev["loss_mle"].item(), float(g["loss_mle"]), rtol=1e-5)
    assert np.isclose(ev2["loss_mle"].item(), float(g["eval_loss_mle_2"]), rtol=1e-5)


def test_infer_with_speakers(fixture_model):
    """infer(x, speaker=s) with given noise is the decoder's reverse pass, conditioned on s, of the z that the encoder (whose
    duration predictor reads s) and the duration kernels give; an int speaker is the tensor filled with it; the voice matters;
    items do not depend on their neighbours in the batch."""
    from smt_amd import glow
    model, g = fixture_model
    model.eval()
    tokens, x_lens = torch.from_numpy(g["tokens"]), torch.from_numpy(g["x_lens"])
    s = torch.tensor([3, 1, 3])
    _, y_len = model.infer(tokens, x_lens, speaker=s)
    t_out = int(y_len.max())
    assert t_out > 0
    noise = torch.randn(3, 8, t_out, generator=torch.Generator().manual_seed(5))
    yh, y_len2 = model.infer(tokens, x_lens, speaker=s, noise=noise)
    assert torch.equal(y_len, y_len2) and yh.shape == (3, 8, t_out)
    with torch.no_grad():
        emb = model.emb_g.weight[s.to(DEV)]
        x_m, x_logs, logw, lens32 = model.encoder(tokens.to(DEV), x_lens.to(DEV), speaker_embeddings=emb)
        _, z_lens, cum = glow.durations(logw, lens32, 1.0, 2)
        idx = glow.duration_index(cum, lens32, z_lens, t_out)
        z = model._prior_sample(glow.align_gather(x_m, idx), glow.align_gather(x_logs, idx), noise.to(DEV).transpose(1, 2), z_lens, t_out)
        rows, _ = model.decoder(z, z_lens, speaker_embeddings=emb, reverse=True)
    assert z_lens.tolist() == y_len.tolist()
    ref = rows.transpose(1, 2).double().cpu()
    err = float((yh.double().cpu() - ref).abs().max())
    assert err <= INFER_TOL * float(ref.abs().max()), err
    for i in range(3):
        assert torch.equal(yh[i, :, int(y_len[i]):].cpu(), torch.zeros(8, t_out - int(y_len[i])))
    # one int for all items = the tensor filled with it
    torch.manual_seed(9)
    a, la = model.infer(tokens, x_lens, speaker=2)
    torch.manual_seed(9)
    b, lb = model.infer(tokens, x_lens, speaker=torch.full((3,), 2))
    assert torch.equal(la, lb) and torch.equal(a, b)
    torch.manual_seed(9)
    c, _ = model.infer(tokens, x_lens, speaker=torch.full((3,), 2, device=DEV))      # ids on the device: the same
    assert torch.equal(a, c)
    # the voice matters, to the durations' input and to the decoder
    with torch.no_grad():
        other_emb = model.emb_g.weight[torch.tensor([0, 1, 3], device=DEV)]
        _, _, logw_other, _ = model.encoder(tokens.to(DEV), x_lens.to(DEV), speaker_embeddings=other_emb)
        rows_other, _ = model.decoder(z, z_lens, speaker_embeddings=other_emb, reverse=True)
    n0, n1, f1 = int(x_lens[0]), int(x_lens[1]), int(z_lens[1])
    assert float((logw_other[0, :n0] - logw[0, :n0]).abs().max()) > 1e-4 and torch.equal(logw_other[1, :n1], logw[1, :n1])
    assert float((rows_other[0] - rows[0]).abs().max()) > 1e-3 and torch.equal(rows_other[1, :f1], rows[1, :f1])
    # an item alone gives what it gives in the batch
    n1 = int(y_len[1])
    alone, l1 = model.infer(tokens[1:2, :int(x_lens[1])], x_lens[1:2], speaker=s[1:2], noise=noise[1:2, :, :n1])
    assert int(l1[0]) == n1
    err = float((alone[0].double() - yh[1, :, :n1].double()).abs().max())
    assert err <= INFER_TOL * float(yh[1].abs().max()), err
    # infer_step passes the speaker on
    ids = tokens[0, :int(x_lens[0])].tolist()
    torch.manual_seed(11)
    one = model.infer_step(ids, speaker=3)
    torch.manual_seed(11)
    two, _ = model.infer(torch.tensor([ids]), speaker=torch.tensor([3]))
    assert torch.equal(one, two)


def test_speaker_refusals(fixture_model, golden):
    from models.glow_tts.glow_tts import GlowTTS
    model, g = fixture_model
    tokens, x_lens, y, y_lens = _batch(g)
    with pytest.raises(ValueError, match="gin_channels"):
        GlowTTS(_config(4, 0))
    model.eval()
    for call in (lambda: model(tokens, x_lens, y, y_lens),                                            # no speaker
                 lambda: model(tokens, x_lens, y, y_lens, speaker=torch.tensor([0, 1, 4], device=DEV)),   # eval: checked at once
                 lambda: model(tokens, x_lens, y, y_lens, speaker=torch.tensor([0, -1, 2])),
                 lambda: model(tokens, x_lens, y, y_lens, speaker=torch.tensor([0, 1], device=DEV)),
                 lambda: model(tokens, x_lens, y, y_lens, speaker=torch.tensor([0.0, 1.0, 2.0], device=DEV)),
                 lambda: model.infer(tokens, x_lens),
                 lambda: model.infer(tokens, x_lens, speaker=4),
                 lambda: model.infer(tokens, x_lens, speaker=torch.tensor([0, 1, 4], device=DEV)),
                 lambda: model.infer_step(tokens[0, :3].tolist()),
                 lambda: model.infer_step(tokens[0, :3].tolist(), speaker=-1)):
        with pytest.raises(ValueError, match="speaker"):
            call()
    # a training step does not wait for the device: ids already there are clamped for the lookup and compared on the device; the
    # item gets a NaN embedding, and check_speaker_ids (which train.py calls when its NaN guard fires) names the cause
    model.train()
    with pytest.raises(ValueError, match="speaker"):
        model(tokens, x_lens, y, y_lens, speaker=torch.tensor([0, 1, 4]))                             # on the host: at once
    model.check_speaker_ids()
    loss_dict, _ = model(tokens, x_lens, y, y_lens, speaker=torch.tensor([0, 1, 4], device=DEV))
    assert torch.isnan(loss_dict["loss"])
    with pytest.raises(ValueError, match="speaker"):
        model.check_speaker_ids()
    model.check_speaker_ids()                                                                         # reported once
    loss_dict, _ = model(tokens, x_lens, y, y_lens, speaker=torch.tensor([0, 1, 3], device=DEV))
    assert torch.isfinite(loss_dict["loss"])
    model.check_speaker_ids()
    model.eval()
    # a single-speaker model takes no speaker
    single = GlowTTS(_config(1, 0)).to(DEV).eval()
    for call in (lambda: single(tokens, x_lens, y, y_lens, speaker=torch.tensor([0, 0, 0], device=DEV)),
                 lambda: single.infer(tokens, x_lens, speaker=0),
                 lambda: single.infer_step(tokens[0, :3].tolist(), speaker=torch.tensor([0]))):
        with pytest.raises(ValueError, match="speaker"):
            call()
    yh, _ = single.infer(tokens, x_lens)                                                              # and still works without
    assert torch.isfinite(yh).all()


def test_single_speaker_model_is_unchanged(golden):
    """Same parameters and state dict as the single-speaker fixture of the reference, same dropout sites as before: the
    multi-speaker model adds parameters and no site."""
    from models.glow_tts.glow_tts import GlowTTS
    single, multi = GlowTTS(_config(1, 0)), GlowTTS(_config(4, 16))
    g = golden("glow_tts")
    assert set(single.state_dict()) == {k[len("param."):] for k in g if k.startswith("param.")}
    for k, v in single.state_dict().items():
        assert tuple(v.shape) == g["param." + k].shape, k
    assert not hasattr(single, "emb_g") and not any("cond_layer" in k for k in single.state_dict())
    sites = single.dropout_sites()
    assert multi.dropout_sites() == sites
    enc, dec = go.GOLDEN_CFG["encoder"], go.GOLDEN_CFG["decoder"]
    expect = (3 if enc["prenet"] else 0) + 4 * enc["n_layers"] + 2 + dec["n_blocks"] * dec["n_layers"]
    assert len(sites) == expect and sorted(sites.values()) == list(range(expect))
    assert sum(".wn.drop." in n for n in sites) == dec["n_blocks"] * dec["n_layers"]


def test_train_py_and_synthesize_with_speakers(tmp_path, monkeypatch):
    """`train.py --model glow_tts_speakers --dataset synthetic_tts_speakers` on reduced copies of the two configurations, two
    epochs: finite losses, the validation loss (no dropout, the same clips) goes down, the checkpoint holds the speaker
    parameters; then `scripts.synthesize --speaker 1` from that checkpoint, and its refusals."""
    import train
    from scripts import synthesize
    from utils import config as C
    monkeypatch.chdir(PKG)
    m = C.load("configs/models/glow_tts_speakers.yaml")
    m.model.encoder.update(C.create(dict(hidden_channels=64, filter_channels=128, n_layers=2)))
    m.model.decoder.update(C.create(dict(hidden_channels=64, n_blocks=3, n_layers=2)))
    m.model.gin_channels = 16                                   # 64 + 16 = 80 input channels: run as 128
    m.scheduler.warmup_steps = 50
    C.save(m, "configs/models/_test_glow_spk.yaml")
    ds = C.load("configs/datasets/synthetic_tts_speakers.yaml")
    ds.dataset.update(C.create(dict(num_clips=8, max_tokens=24)))
    C.save(ds, "configs/datasets/_test_tts_spk.yaml")
    seen = []
    log_stats = train.log_stats
    monkeypatch.setattr(train, "log_stats", lambda step, writer, losses, metrics, prefix="train":
                        (seen.append((prefix, step, dict(losses))), log_stats(step, writer, losses, metrics, prefix=prefix))[1])
    try:
        log_dir = str(tmp_path / "run")
        train.main(["--model", "_test_glow_spk", "--dataset", "_test_tts_spk", "--batch_size", "4", "--num_workers", "0", "--total_epochs", "2",
                    "--log_every_n_steps", "1", "--eval_every_n_epochs", "1", "--ckpt_every_n_steps", "4", "--log_dir", log_dir, "--n_gpus", "1"])
    finally:
        os.remove("configs/models/_test_glow_spk.yaml")
        os.remove("configs/datasets/_test_tts_spk.yaml")
    last = torch.load(os.path.join(log_dir, "ckpts", "ckpt.4.pt"), weights_only=True)
    assert last["step"] == 4 and last["model"]["emb_g.weight"].shape == (8, 16)
    assert "decoder.flows.2.wn.cond_layer.weight_g" in last["model"] and last["model"]["encoder.proj_w.conv_1.weight"].shape[1] == 80
    tr = [l for p, _, l in seen if p == "train"]
    val = [float(l["loss"]) for p, _, l in seen if p == "val"]
    assert len(tr) == 4 and len(val) == 2
    assert all(np.isfinite(float(v)) for l in tr for v in l.values()) and all(np.isfinite(v) for v in val)
    assert {"loss", "loss_mle", "loss_length"} <= set(tr[0])
    print(f"\n[train.py speakers] train loss {[round(float(l['loss']), 4) for l in tr]}, val loss {val}")
    assert val[1] < val[0], val

    (tmp_path / "tokens.txt").write_text("1 5 9 2 7 3\n4 4 8 1\n")
    common = ["--log_dir", log_dir, "--ckpt_num", "4", "--tokens", str(tmp_path / "tokens.txt"), "--dump_dir", str(tmp_path / "out")]
    out = synthesize.main(common + ["--speaker", "1", "--seed", "3"])
    mels = [np.load(os.path.join(out, f"mel_{i}.npy")) for i in range(2)]
    assert all(mel.dtype == np.float32 and mel.shape[0] == 80 and mel.shape[1] > 0 and np.isfinite(mel).all() for mel in mels)
    with pytest.raises(ValueError, match="speaker"):
        synthesize.main(common)
    with pytest.raises(ValueError, match="speaker"):
        synthesize.main(common + ["--speaker", "8"])
