"""The assembled VQTTS on the GPU at the test configuration of tests/vqtts_model_helpers.py (fp32 compute): losses, yh and
every parameter gradient against a float64 restatement with the discrete results teacher-forced; the wiring of the discrete
stages bit for bit; eval and training mode; ``infer``; train.py and scripts.synthesize end to end.

One training step (dropout 0) and its float64 reference are computed once and shared by the first three tests."""
import os
import wave

import numpy as np
import pytest
import torch

import vqtts_model_helpers as H

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-masters-thesis_amd")
DEV = "cuda"
LOSSES = ("loss", "loss_recon", "loss_stft", "loss_commit", "loss_dur", "loss_align", "loss_ce")
VQ_KEYS = {"fit", "entropy", "used_curr", "usage", "dk"}


def _model(dropout=0.0, p_dropout=0.0, seed=0, codebook=True):
    """The model with seeded parameters (zero-initialised tensors included) and, unless ``codebook`` is off, a random,
    initialised codebook."""
    from models.vqtts import VQTTS
    from utils import config as C
    torch.manual_seed(seed)
    model = VQTTS(C.create(H.config_dict(dropout=dropout, p_dropout=p_dropout))).to(DEV)
    H.randomize_zero_init(model)
    if dropout == 0.0 and p_dropout == 0.0:
        model.text_encoder.pre.p_dropout = 0.0       # the prenet's dropout is 0.1 whatever the config says (modules.py:62)
    blk = model.quant_bottleneck
    if not codebook:
        return model
    blk.k.copy_(0.5 * torch.randn(blk.k.shape, generator=torch.Generator().manual_seed(seed + 1)))
    blk.restore_k(threshold=blk.threshold)           # init set, k_sum / k_elem from k
    return model


def _batch():
    return [t.to(DEV) for t in H.batch()]


@pytest.fixture(scope="module")
def run():
    model = _model()
    x, x_lens, y, y_lens = _batch()
    k0 = model.quant_bottleneck.k.detach().clone()
    state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train()
    out, metrics, parts = model(x, x_lens, y, y_lens, return_parts=True)
    out["loss"].backward()
    grads = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}
    k1 = model.quant_bottleneck.k.detach().clone()
    # float64 on the CPU, teacher-forced with the device's alignment and codes
    p64 = {n: p.detach().double().cpu().requires_grad_(True) for n, p in model.named_parameters()}
    ref = H.forward64(p64, k0.double().cpu(), x.cpu(), x_lens.cpu(), y.double().cpu(), y_lens.cpu(), parts["align_idx"].cpu(),
                      parts["q_rel"].cpu(), H.config_dict())
    ref["loss"].backward()
    return dict(model=model, batch=(x, x_lens, y, y_lens), k0=k0, k1=k1, state0=state0, out=out, metrics=metrics, parts=parts,
                grads=grads, p64=p64, ref=ref)


def test_parts_and_outputs_have_the_stated_form(run):
    from models.vqtts.vqtts import PARTS
    out, metrics, parts = run["out"], run["metrics"], run["parts"]
    assert set(out) == set(LOSSES) | {"yh"} and out["yh"].shape == (H.B, H.T)
    assert set(metrics) == {"q_acc"} | VQ_KEYS
    assert tuple(parts) == PARTS and len(parts) == 10
    assert parts["q_lens"].tolist() == list(H.Q_LENS) and parts["x_lens"].tolist() == list(H.X_LENS)
    assert parts["y_enc"].shape == (H.B, H.T // H.STRIDE, H.EMB) and parts["x_enc"].shape == (H.B, H.TX, H.EMB)
    assert parts["align_idx"].dtype == torch.int32 and parts["pred"].shape == (H.B, H.T // H.STRIDE)
    idx = parts["align_idx"].cpu()
    for b in range(H.B):                                          # a monotonic path over all tokens inside the lengths
        row = idx[b, :H.Q_LENS[b]]
        assert row[0] == 0 and row[-1] == H.X_LENS[b] - 1 and bool(((row[1:] - row[:-1]) >= 0).all()) and bool(((row[1:] - row[:-1]) <= 1).all())
        assert bool((idx[b, H.Q_LENS[b]:] == -1).all())


def test_losses_and_yh_against_float64(run):
    """Each of the six loss terms, the reported loss_align and the total within rtol 2e-4, yh within atol 1e-4 (the
    end-to-end criteria of tests/test_model_gpu.py)."""
    out, ref = run["out"], run["ref"]
    for k in LOSSES:
        got, want = out[k].item(), float(ref[k].detach())
        print(f"[vqtts model] {k}: device {got:.8g}  float64 {want:.8g}  rel {abs(got - want) / abs(want):.2e}")
    err = (out["yh"].detach().double().cpu() - ref["yh"].detach()).abs().max().item()
    print(f"[vqtts model] yh: max-abs error {err:.3e} (max |yh| {ref['yh'].detach().abs().max().item():.3e}); "
          f"q_acc device {run['metrics']['q_acc'].item():.4f} float64 {float(ref['q_acc']):.4f}")
    for k in LOSSES:
        assert np.isclose(out[k].item(), float(ref[k].detach()), rtol=2e-4, atol=0.0), k
    assert err <= 1e-4
    assert abs(run["metrics"]["q_acc"].item() - float(ref["q_acc"])) <= 1.0 / sum(H.Q_LENS) + 1e-6      # at most one near-tie


def test_gradients_against_float64(run):
    """Global relative L2 of the concatenated gradient <= 2e-2 and every tensor within 0.5 of its norm (the criterion of
    tests/test_model_gpu.py)."""
    num = den = 0.0
    worst = (0.0, "")
    for name, got in run["grads"].items():
        ref = run["p64"][name].grad
        # (an attention layer's key bias has an exactly zero gradient: softmax ignores a constant added to every score)
        assert ref is not None and (float(ref.norm()) > 1e-12 or name.endswith("conv_k.bias")), f"{name}: the reference gradient is vacuous"
        diff, norm = (got - ref).norm().item(), ref.norm().item()
        worst = max(worst, (diff / (norm + 1e-30), name))
        assert diff <= 0.5 * norm + 1e-6, (name, diff, norm)
        num += diff ** 2
        den += norm ** 2
    print(f"[vqtts model] gradients: global rel-L2 {(num / den) ** 0.5:.3e}; worst tensor {worst[1]} at {worst[0]:.3e}")
    assert len(run["grads"]) == len(run["p64"]) > 300
    assert (num / den) ** 0.5 <= 2e-2


def test_loss_ce_reaches_the_predictor_alone():
    model = _model()
    x, x_lens, y, y_lens = _batch()
    model.train()
    out, _ = model(x, x_lens, y, y_lens)
    out["loss_ce"].backward()
    seen = set()
    for name, p in model.named_parameters():
        top = name.split(".")[0]
        seen.add(top)
        if top in ("text_encoder", "audio_encoder", "audio_decoder"):
            assert p.grad is None or not bool(p.grad.any()), f"loss_ce reached {name}"
        else:
            assert top in ("quant_decoder", "quant_proj")
            assert p.grad is not None and bool(p.grad.any()) and bool(torch.isfinite(p.grad).all()), f"loss_ce did not reach {name}"
    assert seen == {"text_encoder", "audio_encoder", "audio_decoder", "quant_decoder", "quant_proj"}


def test_discrete_stages_are_wired_bit_for_bit(run):
    from models.vqtts import Bottleneck
    from smt_amd import vqtts
    model, parts = run["model"], run["parts"]
    x = run["batch"][0]
    idx, dur = vqtts.align(parts["x_enc"].detach(), parts["y_enc"].detach(), parts["x_lens"], parts["q_lens"])
    assert torch.equal(idx, parts["align_idx"]) and torch.equal(dur, parts["durations"])
    fresh = Bottleneck(H.N_VOCAB + 1, H.L_BINS, H.EMB, 0.99, 1.0).to(DEV)
    fresh.k.copy_(run["k0"])
    q_rel, q_abs = fresh.encode(parts["y_enc"].detach(), x, parts["align_idx"])
    assert torch.equal(q_rel, parts["q_rel"])
    has = parts["align_idx"] >= 0
    assert torch.equal(parts["y_d"].detach()[has], run["k0"][q_abs[has]]) and bool((parts["y_d"].detach()[~has] == 0).all())
    assert not torch.equal(run["k1"], run["k0"])                  # the training step did update the codebook afterwards
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            pred = model.predictor(parts["x_enc"].detach(), parts["align_idx"], parts["q_lens"])
    finally:
        model.train(was)
    assert torch.equal(pred, parts["pred"])


def test_eval_mode(run):
    """Eval mode of a model built WITH dropout in its configuration: yh decodes the predicted codes, the losses are the
    quantiser path's, nothing is dropped and the codebook stays."""
    model = _model(dropout=0.1, p_dropout=0.1)
    model.load_state_dict(run["state0"], strict=True)
    model.quant_bottleneck.restore_k(threshold=1.0)
    model.eval()
    x, x_lens, y, y_lens = run["batch"]
    with torch.no_grad():
        out, metrics, parts = model(x, x_lens, y, y_lens, return_parts=True)
        out2, _ = model(x, x_lens, y, y_lens)
    assert set(metrics) == {"q_acc"}
    assert torch.equal(model.quant_bottleneck.k, run["k0"]) and model._drop_seed == 2
    assert all(torch.equal(out[k], out2[k]) for k in LOSSES + ("yh",))                      # no dropout: equal bits
    # yh: the torch chain on the predicted codes
    keep = torch.arange(parts["pred"].shape[1], device=DEV)[None, :] < parts["q_lens"][:, None]
    with torch.no_grad():
        q = model.predictor.synthesize_codes(parts["pred"], x, parts["align_idx"])
        yh, _ = model.audio_decoder(model.quant_bottleneck.decode(q) * keep[..., None], parts["q_lens"])
    assert torch.equal(out["yh"], yh)
    assert not torch.equal(parts["pred"].long(), parts["q_rel"]), "an untrained predictor that agrees with the quantiser everywhere"
    # the losses are the training-mode formulae on the quantiser's path: the float64 reference of the shared step applies
    # (same parameters, same codebook; the discrete results must then be the same too)
    assert torch.equal(parts["align_idx"], run["parts"]["align_idx"]) and torch.equal(parts["q_rel"], run["parts"]["q_rel"])
    for k in LOSSES:
        assert np.isclose(out[k].item(), float(run["ref"][k].detach()), rtol=2e-4, atol=0.0), k


def test_training_mode_with_dropout():
    model = _model(dropout=0.1, p_dropout=0.1, codebook=False)     # as built: the first training forward draws the codebook
    blk = model.quant_bottleneck
    x, x_lens, y, y_lens = _batch()
    model.train()
    assert not blk.init and not bool(blk.k.any())
    out, metrics = model(x, x_lens, y, y_lens)
    assert blk.init and bool(blk.k.any()) and VQ_KEYS <= set(metrics) and "q_acc" in metrics
    k1 = blk.k.detach().clone()
    out["loss"].backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert all(bool(torch.isfinite(out[k])) for k in LOSSES) and bool(torch.isfinite(out["yh"]).all())
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in metrics.values())
    out2, _ = model(x, x_lens, y, y_lens)
    assert model._drop_seed == 2 and not torch.equal(blk.k, k1)
    assert out2["loss_recon"].item() != out["loss_recon"].item()                           # the masks advance with _drop_seed


def _infer_chain(model, x, lens, length_scale=1.0):
    """VQTTS.infer's steps with the torch chain in place of the emission kernel: (wave, wave_lengths, z_lens)."""
    from smt_amd import glow
    valid = torch.arange(x.shape[1])[None, :] < lens[:, None]
    x_dev = torch.where(valid, x, 0).to(DEV)
    x_enc, _, logw, lens32 = model.text_encoder(x_dev, lens.to(DEV))
    _, z_lens, cum = glow.durations(logw, lens32, length_scale, 1)
    t_out = int(z_lens.max())
    idx = glow.duration_index(cum, lens32, z_lens, t_out)
    pred = model.predictor(x_enc, idx, z_lens)
    keep = torch.arange(t_out, device=DEV)[None, :] < z_lens[:, None]
    y_d = model.quant_bottleneck.decode(model.predictor.synthesize_codes(pred, x_dev, idx)) * keep[..., None]
    wave, _ = model.audio_decoder(y_d, z_lens)
    wave_lengths = z_lens.long() * model.stride
    return wave * (torch.arange(wave.shape[1], device=DEV)[None, :] < wave_lengths[:, None]), wave_lengths, z_lens


def test_infer():
    model = _model().eval()
    x, x_lens, _, _ = H.batch()
    wave, wave_lengths = model.infer(x, x_lens)
    with torch.no_grad():
        want, want_lengths, z_lens = _infer_chain(model, x, x_lens)
    assert wave.dtype == torch.float32 and wave_lengths.dtype == torch.int64 and wave_lengths.shape == (H.B,)
    assert wave.shape == (H.B, int(z_lens.max()) * H.STRIDE) and torch.equal(wave_lengths, z_lens.long() * H.STRIDE)
    assert bool((z_lens.cpu() >= x_lens).all())                                           # at least a frame per token
    for b, n in enumerate(wave_lengths.tolist()):
        assert bool((wave[b, n:] == 0).all()) and bool(wave[b, :n].any())
    assert torch.equal(wave, want) and torch.equal(wave_lengths, want_lengths)            # the kernel against the torch chain
    wave2, lengths2 = model.infer(x, x_lens)
    assert torch.equal(wave2, wave) and torch.equal(lengths2, wave_lengths)
    # padding ids are never read: garbage past the lengths changes nothing
    junk = x.clone()
    junk[1, H.X_LENS[1]:] = 10 ** 6
    assert torch.equal(model.infer(junk, x_lens)[0], wave)
    # length_scale = 2: ceil(2 e) per token lies in [2 ceil(e) - 1, 2 ceil(e)]
    _, doubled = model.infer(x, x_lens, length_scale=2.0)
    frames, frames2 = wave_lengths.cpu() // H.STRIDE, doubled.cpu() // H.STRIDE
    assert bool((frames2 <= 2 * frames).all()) and bool((frames2 >= 2 * frames - x_lens).all())
    # one utterance
    one = model.infer_step(x[2, :H.X_LENS[2]].tolist())
    alone, alone_length = model.infer(x[2:3, :H.X_LENS[2]])
    assert one.shape == (1, int(alone_length[0])) and torch.equal(one, alone)
    # refusals
    bad = x.clone()
    bad[0, 3] = H.N_VOCAB + 1
    with pytest.raises(ValueError, match=r"item 0, token 3: id 12 is outside \[0, 12\)"):
        model.infer(bad, x_lens)
    with pytest.raises(ValueError, match="item 1 has 0 tokens"):
        model.infer(x, torch.tensor([12, 0, 5]))
    for scale in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="length_scale"):
            model.infer(x, x_lens, length_scale=scale)
    with pytest.raises(NotImplementedError):
        model.infer_step("a string")
    with pytest.raises(ValueError, match="speaker"):
        model.infer_step([1, 2, 3], speaker=0)
    model.train()
    with pytest.raises(RuntimeError, match="evaluation mode"):
        model.infer(x, x_lens)


def test_train_py_and_synthesize(tmp_path, monkeypatch):
    """`train.py --model vqtts --dataset synthetic_vqtts` end to end on reduced copies of the two configurations (8 clips,
    batch 4, two epochs), then `scripts.synthesize` on the checkpoint it wrote."""
    import train
    from scripts import synthesize
    from utils import config as C
    from utils.commons import get_model
    monkeypatch.chdir(PKG)
    rows = []

    class Recorder:                                                # the writer's surface, whatever scalar back end is installed
        _tb = None

        def __init__(self, log_dir):
            pass

        def add_scalar(self, tag, value, step):
            rows.append({"tag": tag, "value": float(value), "step": int(step)})

        def close(self):
            pass
    monkeypatch.setattr(train, "ScalarWriter", Recorder)
    m = C.load("configs/models/vqtts.yaml")
    small = H.config_dict(dropout=0.1, p_dropout=0.1)["model"]
    m.model.update(C.create({k: small[k] for k in ("width", "depth", "multipliers", "emb_width", "l_bins")}))
    m.model.encoder.update(C.create(dict(out_channels=H.EMB, hidden_channels=64, filter_channels=128, n_layers=2)))
    m.model.loss.linf_topk = 256
    C.save(m, "configs/models/_test_vqtts.yaml")
    ds = C.load("configs/datasets/synthetic_vqtts.yaml")
    ds.dataset.update(C.create(dict(num_clips=8, clip_length=16384, max_tokens=16)))
    C.save(ds, "configs/datasets/_test_vqtts_data.yaml")
    try:
        log_dir = str(tmp_path / "run")
        train.main(["--model", "_test_vqtts", "--dataset", "_test_vqtts_data", "--batch_size", "4", "--num_workers", "0",
                    "--total_epochs", "2", "--log_every_n_steps", "1", "--eval_every_n_epochs", "1", "--ckpt_every_n_steps", "4",
                    "--log_dir", log_dir, "--n_gpus", "1"])
    finally:
        os.remove("configs/models/_test_vqtts.yaml")
        os.remove("configs/datasets/_test_vqtts_data.yaml")
    last = torch.load(os.path.join(log_dir, "ckpts", "ckpt.last.pt"), weights_only=True)
    assert last["step"] == 4 and {"quant_proj.weight", "audio_decoder.out.weight", "quant_bottleneck.k"} <= set(last["model"])
    assert "quant_bottleneck" in last["extra"] and last["extra"]["drop_seed"] > 0
    assert {"loss/train_loss_ce", "loss/train_loss_align", "loss/train_loss_dur", "loss/val_loss"} <= {r["tag"] for r in rows}
    assert all(np.isfinite(r["value"]) for r in rows)
    assert os.path.exists(os.path.join(log_dir, "audio", "val_audio_2_pred.wav"))
    # synthesis from the numbered checkpoint of the same step
    tokens = tmp_path / "utterances.txt"
    tokens.write_text("5 17 0 99 3 148\n\n7 7 1\n")
    common = ["--log_dir", log_dir, "--ckpt_num", "4", "--tokens", str(tokens), "--dump_dir", str(tmp_path / "out"), "--batch_size", "1"]
    with pytest.raises(ValueError, match="noise_scale"):
        synthesize.main(common + ["--noise_scale", "0.5"])
    dump = synthesize.main(common)
    assert os.path.basename(dump) == "VQTTS@4" and os.path.exists(os.path.join(dump, "mel_spectrograms.png"))
    cfg = C.load(os.path.join(log_dir, "config.yaml"))
    model, _ = get_model(cfg, DEV)
    model.load_state_dict(torch.load(os.path.join(log_dir, "ckpts", "ckpt.4.pt"), weights_only=True)["model"])
    model.eval()
    for i, ids in enumerate(([5, 17, 0, 99, 3, 148], [7, 7, 1])):
        wav, lengths = model.infer(torch.tensor([ids]))
        with wave.open(os.path.join(dump, f"wav_{i}.wav"), "rb") as f:
            assert f.getframerate() == 22050 and f.getnchannels() == 1 and f.getsampwidth() == 2
            assert f.getnframes() == int(lengths[0]) >= 256 * len(ids)
            pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
        want = (np.clip(wav[0].double().cpu().numpy(), -1.0, 1.0) * 32767.0).astype("<i2")
        assert np.array_equal(pcm, want)
