"""smt_mel_invert and smt_griffin_lim on the device against the float64 restatements of tests/griffin_lim_helpers.py, and the
layers above them (datasets.transforms.GriffinLim, scripts.synthesize --vocoder, the validation dumps of train.py).  Every
tolerance is the E32 rule of tests/spectral_ref_helpers.py: max(4 E32, floor) with the floors named there and in the helper.
The tests print every figure before they assert; DESIGN.md section 19 has the measured ones."""
import os

import numpy as np
import pytest
import torch

import griffin_lim_helpers as G
import spectral_ref_helpers as H

pytestmark = pytest.mark.gpu


def run_mel_invert(mel, lens, front, n_iter, log_input):
    from smt_amd import spectral
    cfg, n_mels, f_max = G.MEL_FRONT_ENDS[front]
    module = H.mel_module(cfg, n_mels, f_max).cuda()
    return spectral.mel_invert(mel.cuda(), torch.tensor(lens), module.mel_basis, module.band, n_iter=n_iter, log_input=log_input).cpu()


def run_griffin_lim(mag, phase, lens, cfg, n_iter, momentum=G.MOMENTUM, seed=0):
    from smt_amd import spectral
    wave, lengths = spectral.griffin_lim(mag.cuda(), torch.tensor(lens), cfg[0], cfg[1], cfg[2], n_iter=n_iter, momentum=momentum,
                                         seed=seed, phase0=None if phase is None else phase.cuda())
    assert lengths.tolist() == [G.samples_of(cfg, n) for n in lens] and not lengths.is_cuda
    assert wave.shape == (len(lens), G.samples_of(cfg, mag.shape[2]))
    return wave.cpu()


# ------------------------------------------------------------------------------------------------ mel inversion

@pytest.mark.parametrize("log_input", [True, False])
@pytest.mark.parametrize("front", range(len(G.MEL_FRONT_ENDS)))
def test_mel_invert_against_float64(front, log_input):
    """Every frame count x iteration count of the table; padded columns and uncovered bins exactly zero; bit-equal twice."""
    worst = 0.0
    for frames in G.MEL_FRAMES:
        mel, lens, basis = G.mel_case(front, frames, log_input)
        uncovered = basis.sum(0) == 0
        assert uncovered.any() and torch.isnan(mel[1, :, lens[1]:]).all()
        for n_iter in G.MEL_ITERS:
            ref, e32 = G.mel_reference(front, frames, log_input, n_iter)
            got = run_mel_invert(mel, lens, front, n_iter, log_input)
            err, bound = H.max_abs(got, ref), H.bound_magnitude(e32, ref)
            print(f"mel_invert front {front} log {int(log_input)} frames {frames} n_iter {n_iter}: max|ref| {float(ref.max()):.4g} "
                  f"err {err:.3g} E32 {e32:.3g} bound {bound:.3g}")
            assert got.shape == ref.shape and torch.isfinite(got).all()
            assert err <= bound, (front, log_input, frames, n_iter, err, e32)
            worst = max(worst, err / bound)
            for b, n in enumerate(lens):
                assert (got[b, :, n:] == 0).all(), (frames, n_iter, b, "padded columns")
            assert (got[:, uncovered] == 0).all() and float(got.min()) >= 0
            if n_iter == 8:
                assert torch.equal(got, run_mel_invert(mel, lens, front, n_iter, log_input))
    print(f"mel_invert front {front} log {int(log_input)}: worst err / bound {worst:.3g}")


def test_mel_invert_c_entry_without_lens():
    """lens = NULL means `frames` for every item: bit-equal to the op with full lengths."""
    from smt_amd import native as N
    from smt_amd import spectral
    cfg, n_mels, f_max = G.MEL_FRONT_ENDS[1]
    module = H.mel_module(cfg, n_mels, f_max).cuda()
    mel = G.mel_case(1, 65, True)[0][:1].cuda().contiguous()
    want = spectral.mel_invert(mel, torch.tensor([65]), module.mel_basis, module.band, n_iter=8)
    got = torch.full_like(want, float("nan"))
    N.check(N.lib().smt_mel_invert(N.ptr(mel), None, N.ptr(module.mel_basis), N.ptr(module.band), N.ptr(got), 1, cfg[0], n_mels, 65, 8, 1,
                                   N.stream_ptr()), "smt_mel_invert")
    assert torch.equal(got, want) and float(got.max()) > 0


# --------------------------------------------------------------------------------------------------- Griffin-Lim

def check_waves(cfg, lens, seed0, got, n_iter, momentum):
    worst = 0.0
    for b, n in enumerate(lens):
        t = G.samples_of(cfg, n)
        assert (got[b, t:] == 0).all(), (cfg, lens, b, "samples at or past T_b")
        if n == 0:
            continue
        ref, e32 = G.item_reference(cfg, n, seed0 + b, n_iter, momentum)
        err, bound = H.max_abs(got[b, :t], ref), H.bound_inverse(e32, ref)
        print(f"griffin_lim {cfg} lens {lens} item {b} ({n} frames) n_iter {n_iter} momentum {momentum}: max|ref| "
              f"{float(ref.abs().max()):.4g} err {err:.3g} E32 {e32:.3g} bound {bound:.3g}")
        assert err <= bound, (cfg, lens, b, n_iter, momentum, err, e32)
        worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize("n_iter", [0, 1, 2])
@pytest.mark.parametrize("cfg", G.CONFIGS)
def test_griffin_lim_per_element(cfg, n_iter):
    """Explicit start phases, per element against float64.  n_iter = 2 is the first that reads t; there momentum 0 runs too."""
    worst = 0.0
    for lens, seed0 in G.calls(cfg):
        mag, phase = G.batch(cfg, lens, seed0=seed0)
        for momentum in ([G.MOMENTUM, 0.0] if n_iter == 2 else [G.MOMENTUM]):
            worst = max(worst, check_waves(cfg, lens, seed0, run_griffin_lim(mag, phase, lens, cfg, n_iter, momentum), n_iter, momentum))
    print(f"griffin_lim {cfg} n_iter {n_iter}: worst err / bound {worst:.3g}")


@pytest.mark.parametrize("cfg", G.CONFIGS)
def test_griffin_lim_32_iterations(cfg):
    """Spectral convergence of the waveform returned against the float64 run's, relative; bit-equal on a second call; zeros
    at or past T_b.  MI355X: median 1.8e-6 over the 58 items of the table, largest 4.6e-5 ((2048, 240, 1200), four frames) against
    the floor of 5.3e-5."""
    for lens, seed0 in G.calls(cfg):
        mag, phase = G.batch(cfg, lens, seed0=seed0)
        got = run_griffin_lim(mag, phase, lens, cfg, G.N_ITER_LONG)
        assert torch.equal(got, run_griffin_lim(mag, phase, lens, cfg, G.N_ITER_LONG))
        assert torch.isfinite(got).all()
        for b, n in enumerate(lens):
            t = G.samples_of(cfg, n)
            assert (got[b, t:] == 0).all()
            if n == 0:
                continue
            sc64, e32 = G.sc_reference(cfg, n, seed0 + b)
            sc = G.spectral_convergence(got[b, :t], G.item(cfg, n, seed0 + b)[0], cfg)
            err = abs(sc - sc64) / sc64
            print(f"griffin_lim {cfg} lens {lens} item {b} ({n} frames) n_iter {G.N_ITER_LONG}: sc {sc:.6g} sc64 {sc64:.6g} "
                  f"rel {err:.3g} E32 {e32:.3g} bound {G.bound_sc(e32):.3g}")
            assert err <= G.bound_sc(e32), (cfg, lens, b, sc, sc64, e32)


@pytest.mark.parametrize("cfg", [G.CONFIGS[0], G.CONFIGS[2], G.CONFIGS[4]])
def test_an_item_does_not_depend_on_its_batch(cfg):
    """Bit for bit: alone, at another position among other items, and in a batch with more frames and NaN past its own."""
    n_iter = 3
    for n in (G.f_min(cfg), 5):
        S, phi = G.item(cfg, n, 0)
        t = G.samples_of(cfg, n)
        alone = run_griffin_lim(S[None], phi[None], [n], cfg, n_iter)[0]
        assert alone.shape == (t,) and float(alone.abs().max()) > 0
        lens = [9, n, 0, 4 if 4 >= G.f_min(cfg) else 9]
        mag, phase = G.batch(cfg, lens, frames=11, seed0=50)            # frames above every item's: NaN columns everywhere
        mag[1, :, :n], phase[1, :, :n] = S, phi
        moved = run_griffin_lim(mag, phase, lens, cfg, n_iter)
        assert torch.equal(moved[1, :t], alone) and (moved[1, t:] == 0).all(), (cfg, n)
        assert torch.isfinite(moved).all()
        # generated phases: the draw depends on (seed_b, f, k), not on the position or on `frames`
        a = run_griffin_lim(S[None], None, [n], cfg, n_iter, seed=[7])[0]
        m = run_griffin_lim(mag, None, lens, cfg, n_iter, seed=[1, 7, 2, 3])
        assert torch.equal(m[1, :t], a), (cfg, n)


def test_generated_phases():
    """Equal seeds give equal bits, other seeds differ on most samples, an int seed is (seed + b) per item, and one iteration
    from the generated phases is the float64 helper's from its own hash-derived phases."""
    for cfg in (G.CONFIGS[0], G.CONFIGS[3]):
        lens = G.ragged_lens(cfg)
        mag, _ = G.batch(cfg, lens)
        a = run_griffin_lim(mag, None, lens, cfg, 1, seed=11)
        assert torch.equal(a, run_griffin_lim(mag, None, lens, cfg, 1, seed=11))
        assert torch.equal(a, run_griffin_lim(mag, None, lens, cfg, 1, seed=[11 + b for b in range(len(lens))]))
        other = run_griffin_lim(mag, None, lens, cfg, 1, seed=12)
        for b, n in enumerate(lens):
            t = G.samples_of(cfg, n)
            if n == 0:
                continue
            assert float((a[b, :t] != other[b, :t]).float().mean()) > 0.9
            S = G.item(cfg, n, b)[0]
            phi = G.hash_phases(11 + b, n, S.shape[0])
            ref = G.griffin_lim_ref(S, phi, cfg, 1, G.MOMENTUM)
            e32 = H.max_abs(G.griffin_lim_ref(S, phi, cfg, 1, G.MOMENTUM, torch.float32), ref)
            err = H.max_abs(a[b, :t], ref)
            print(f"generated phases {cfg} item {b} ({n} frames): err {err:.3g} E32 {e32:.3g} bound {H.bound_inverse(e32, ref):.3g}")
            assert err <= H.bound_inverse(e32, ref), (cfg, b, err, e32)


def test_c_entry_writes_zeros_for_an_item_too_short_to_transform():
    """One frame at (1024, 256) is 256 samples against a reflect padding of 384: the Python op refuses it, the C entry writes
    zeros for it and transforms its neighbours; lens = NULL means `frames` for every item."""
    from smt_amd import native as N
    from smt_amd import spectral
    cfg = G.CONFIGS[0]
    lens = [5, 1, 3]
    mag, phase = G.batch(cfg, [5, 5, 3], frames=5, poison=1.0)
    mag, phase = mag.cuda(), phase.cuda()
    window, tw = spectral._get_tables(cfg[0], cfg[2], mag.device)
    t_max = G.samples_of(cfg, 5)

    def call(lens32):
        wave = torch.full((3, t_max), float("nan"), device="cuda")
        ws = torch.empty(N.lib().smt_griffin_lim_workspace_bytes(3, cfg[0], cfg[1], 5), dtype=torch.uint8, device="cuda")
        N.check(N.lib().smt_griffin_lim(N.ptr(mag), N.ptr(lens32), N.ptr(phase), None, N.ptr(window), N.ptr(tw), N.ptr(wave), 3, cfg[0],
                                        cfg[1], 5, 2, G.MOMENTUM, N.ptr(ws), ws.numel(), N.stream_ptr()), "smt_griffin_lim")
        return wave.cpu()

    got = call(torch.tensor(lens, dtype=torch.int32).cuda())
    assert (got[1] == 0).all() and (got[2, G.samples_of(cfg, 3):] == 0).all()
    for b in (0, 2):
        ref, e32 = G.item_reference(cfg, lens[b], b, 2)
        assert H.max_abs(got[b, :ref.shape[0]], ref) <= H.bound_inverse(e32, ref)
    full = call(None)
    assert torch.equal(full[0], got[0]) and float(full[1].abs().max()) > 0
    with pytest.raises(ValueError, match="item 1 has 1 frames"):
        spectral.griffin_lim(mag, torch.tensor(lens), *cfg)


# ------------------------------------------------------------------------------------------------------- module

def test_round_trip_through_the_module():
    """signal -> MelSpectrogram -> GriffinLim -> MelSpectrogram: the mean |log-mel error| is the float64 pipeline's own (0.1
    to 0.2 on these signals: a property of the algorithm) within max(4 E32, floor)."""
    from datasets.transforms import GriffinLim
    cfg, n_mels, f_max = G.ROUNDTRIP_FRONT
    vocoder = GriffinLim(sample_rate=H.SAMPLE_RATE, n_fft=cfg[0], win_length=cfg[2], hop_length=cfg[1], n_mels=n_mels, f_min=0.0,
                         f_max=f_max).cuda()
    assert torch.equal(vocoder.mel_basis.cpu(), H.mel_module(cfg, n_mels, f_max).mel_basis.cpu())
    front = H.mel_module(cfg, n_mels, f_max).cuda()
    for seed in G.ROUNDTRIP_SEEDS:
        x = G.roundtrip_signal(seed).cuda()
        mel = front(x)
        frames = mel.shape[2]
        wave, lengths = vocoder(mel, torch.tensor([frames]), n_iter=G.ROUNDTRIP_ITERS, nnls_iter=G.ROUNDTRIP_ITERS, seed=seed)
        assert lengths.tolist() == [frames * cfg[1]] == [x.shape[1]]
        again = front(wave.clamp(-1, 1))
        err = float((again - mel).abs().double().mean())
        ref, e32 = G.roundtrip_reference(seed), G.roundtrip_e32(seed)
        print(f"round trip seed {seed}: mean |log-mel error| {err:.6g} float64 {ref:.6g} diff {abs(err - ref):.3g} E32 {e32:.3g} "
              f"bound {G.bound_roundtrip(e32):.3g}")
        assert abs(err - ref) <= G.bound_roundtrip(e32), (seed, err, ref, e32)


# ---------------------------------------------------------------------------------------------- train.py, the CLI

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-masters-thesis_amd")


def wav_samples(path):
    import wave
    with wave.open(path, "rb") as f:
        assert f.getnchannels() == 1 and f.getsampwidth() == 2
        return f.getnframes()


@pytest.fixture(scope="module")
def trained_run(tmp_path_factory):
    """`train.py --model glow_tts --dataset synthetic_tts` on reduced copies of the two configurations, two epochs, once for
    the tests below: (log_dir, the validation dumps it left)."""
    import train
    from utils import config as C
    root = tmp_path_factory.mktemp("gl_run")
    cwd = os.getcwd()
    os.chdir(PKG)
    m = C.load("configs/models/glow_tts.yaml")
    m.model.encoder.update(C.create(dict(hidden_channels=64, filter_channels=128, n_layers=2)))
    m.model.decoder.update(C.create(dict(hidden_channels=64, n_blocks=3, n_layers=2)))
    m.scheduler.warmup_steps = 50
    C.save(m, "configs/models/_test_gl_glow.yaml")
    ds = C.load("configs/datasets/synthetic_tts.yaml")
    ds.dataset.update(C.create(dict(num_clips=8, max_tokens=24)))
    C.save(ds, "configs/datasets/_test_gl_tts.yaml")
    try:
        log_dir = str(root / "run")
        train.main(["--model", "_test_gl_glow", "--dataset", "_test_gl_tts", "--batch_size", "4", "--num_workers", "0", "--total_epochs", "2",
                    "--log_every_n_steps", "1", "--eval_every_n_epochs", "1", "--ckpt_every_n_steps", "4", "--log_dir", log_dir, "--n_gpus", "1"])
    finally:
        os.remove("configs/models/_test_gl_glow.yaml")
        os.remove("configs/datasets/_test_gl_tts.yaml")
        os.chdir(cwd)
    return log_dir, root


def test_train_py_leaves_spectrogram_and_audio_dumps(trained_run):
    log_dir, _ = trained_run
    spect, audio = sorted(os.listdir(os.path.join(log_dir, "spect"))), sorted(os.listdir(os.path.join(log_dir, "audio")))
    steps = sorted({int(name.split("_")[2].split(".")[0]) for name in spect})
    assert len(steps) == 2 and spect == [f"val_spect_{e}.png" for e in steps]
    assert audio == sorted(f"val_audio_{e}_{kind}.wav" for e in steps for kind in ("gt", "syn"))
    for name in spect:
        with open(os.path.join(log_dir, "spect", name), "rb") as f:
            assert f.read(8) == b"\x89PNG\r\n\x1a\n"
    for name in audio:
        n = wav_samples(os.path.join(log_dir, "audio", name))
        assert n > 0 and n % 256 == 0, (name, n)


def test_synthesize_with_the_vocoder(trained_run):
    """wav_<i>.wav of frames * hop samples beside the spectrograms; byte-equal on a second run and at another --batch_size
    (utterance i starts from seed --seed + i; --noise_scale 0 makes the spectrograms themselves independent of the batch);
    without the flag the directory holds what it held before the flag existed."""
    from scripts import synthesize
    log_dir, root = trained_run
    (root / "tokens.txt").write_text("1 5 9 2 7 3\n4 4 8 1\n2 6 6 9 3 1 5 7\n")
    common = ["--log_dir", log_dir, "--ckpt_num", "4", "--tokens", str(root / "tokens.txt"), "--seed", "3", "--noise_scale", "0"]

    def run(name, *extra):
        out = synthesize.main(common + ["--dump_dir", str(root / name)] + list(extra))
        return out, {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}

    _, plain = run("plain")
    assert sorted(plain) == ["mel_0.npy", "mel_1.npy", "mel_2.npy", "mel_spectrograms.png"]
    out, a = run("a", "--vocoder", "griffin_lim", "--gl_iters", "8")
    assert sorted(a) == sorted(list(plain) + ["wav_0.wav", "wav_1.wav", "wav_2.wav"])
    assert all(a[f] == plain[f] for f in plain)
    for i in range(3):
        mel = np.load(os.path.join(out, f"mel_{i}.npy"))
        assert wav_samples(os.path.join(out, f"wav_{i}.wav")) == mel.shape[1] * 256 > 0
        pcm = np.frombuffer(a[f"wav_{i}.wav"][44:], dtype="<i2")
        assert np.abs(pcm).max() > 0
    _, again = run("again", "--vocoder", "griffin_lim", "--gl_iters", "8")
    assert again == a
    _, other = run("other", "--vocoder", "griffin_lim", "--gl_iters", "8", "--batch_size", "2")
    assert all(other[f"mel_{i}.npy"] == a[f"mel_{i}.npy"] for i in range(3)), "the spectrograms themselves depend on the batch"
    assert all(other[f"wav_{i}.wav"] == a[f"wav_{i}.wav"] for i in range(3))
    _, seeded = run("seeded", "--vocoder", "griffin_lim", "--gl_iters", "8", "--seed", "4")
    assert seeded["wav_1.wav"] != a["wav_1.wav"] and seeded["mel_1.npy"] == a["mel_1.npy"]
    with pytest.raises(ValueError, match="--gl_iters must be >= 0"):
        synthesize.main(common + ["--vocoder", "griffin_lim", "--gl_iters", "-2"])
