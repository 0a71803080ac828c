"""Host side of the mel inversion and Griffin-Lim (smt_mel_invert / smt_griffin_lim, smt_amd.spectral.mel_invert / griffin_lim,
scripts.synthesize --vocoder): export, every argument error, the phase hash, the float64 restatements of
tests/griffin_lim_helpers.py against the existing references, and the refusals.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import griffin_lim_helpers as G
import spectral_ref_helpers as H

DUMMY = ctypes.c_void_p(0x1000)      # a non-null pointer for calls that must fail before they launch anything
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_exported_declared_and_bound_under_abi_10():
    from smt_amd import native as N
    lib = N.lib()
    assert lib.smt_abi_version() == N.ABI_VERSION == 10
    with open(os.path.join(REPO, "include", "smt_hip.h")) as f:
        header = f.read()
    for name in ("smt_mel_invert", "smt_griffin_lim_workspace_bytes", "smt_griffin_lim"):
        assert name in N.exported_symbols() and hasattr(lib, name)
        assert re.search(r"\b(int|size_t) " + name + r"\(", header), name
    # the declared argument counts are the bound ones
    for name in ("smt_mel_invert", "smt_griffin_lim"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(N._SIGNATURES[name][1]), name


def test_mel_invert_checks_its_arguments():
    from smt_amd import native as N
    lib = N.lib()

    def call(mel=DUMMY, lens=DUMMY, basis=DUMMY, band=DUMMY, mag=DUMMY, batch=2, n_fft=1024, n_mels=80, frames=16, n_iter=32):
        return lib.smt_mel_invert(mel, lens, basis, band, mag, batch, n_fft, n_mels, frames, n_iter, 1, None)

    bad = [(dict(mel=None), "null pointer"), (dict(basis=None), "null pointer"), (dict(band=None), "null pointer"),
           (dict(mag=None), "null pointer"), (dict(n_fft=1000), "n_fft=1000 unsupported (256, 512, 1024, 2048)"),
           (dict(n_fft=4096), "n_fft=4096 unsupported"), (dict(n_mels=0), "n_mels=0 outside [1, 1024]"),
           (dict(n_mels=1025), "n_mels=1025 outside [1, 1024]"), (dict(n_iter=-1), "n_iter=-1, need >= 0"),
           (dict(batch=-1), "batch=-1 outside [0, 65535]"), (dict(batch=65536), "batch=65536 outside [0, 65535]"),
           (dict(frames=-1), "frames=-1, need >= 0")]
    for change, message in bad:
        assert call(**change) == 1, change
        got = lib.smt_last_error().decode()
        assert got.startswith("smt_mel_invert: ") and message in got, (change, got)
    assert call(batch=0) == 0 and call(frames=0) == 0 and call(batch=0, lens=None) == 0     # lens may be NULL
    assert call(batch=0, n_fft=1000) == 1 and call(frames=0, n_iter=-1) == 1               # only after the checks


def test_griffin_lim_checks_its_arguments():
    from smt_amd import native as N
    lib = N.lib()
    need = lib.smt_griffin_lim_workspace_bytes(2, 1024, 256, 16)
    bins, t_max = 513, 15 * 256 + 256
    parts = [2 * 16 * bins * 8, 2 * 16 * bins * 4, 2 * 16 * 1024 * 4, 2 * t_max * 4]
    assert need == sum((p + 255) // 256 * 256 for p in parts)
    assert lib.smt_griffin_lim_workspace_bytes(0, 1024, 256, 16) == 0 and lib.smt_griffin_lim_workspace_bytes(2, 1024, 256, 0) == 0

    def call(mag=DUMMY, lens=DUMMY, phase0=DUMMY, seeds=None, window=DUMMY, tw=DUMMY, wave=DUMMY, batch=2, n_fft=1024, hop=256,
             frames=16, n_iter=32, momentum=0.99, ws=DUMMY, ws_bytes=need):
        return lib.smt_griffin_lim(mag, lens, phase0, seeds, window, tw, wave, batch, n_fft, hop, frames, n_iter, momentum, ws,
                                   ws_bytes, None)

    bad = [(dict(mag=None), "null pointer"), (dict(window=None), "null pointer"), (dict(tw=None), "null pointer"),
           (dict(wave=None), "null pointer"),
           (dict(seeds=DUMMY), "exactly one of phase0 and seeds must be given, got both"),
           (dict(phase0=None), "exactly one of phase0 and seeds must be given, got neither"),
           (dict(n_fft=1000), "n_fft=1000 unsupported (256, 512, 1024, 2048)"), (dict(n_fft=128), "n_fft=128 unsupported"),
           (dict(hop=0), "hop=0 outside [1, n_fft=1024]"), (dict(hop=1025), "hop=1025 outside [1, n_fft=1024]"),
           (dict(n_iter=-1), "n_iter=-1, need >= 0"), (dict(momentum=1.0), "momentum=1 outside [0, 1)"),
           (dict(momentum=-0.5), "momentum=-0.5 outside [0, 1)"), (dict(momentum=float("nan")), "outside [0, 1)"),
           (dict(batch=-1), "batch=-1 outside [0, 65535]"), (dict(batch=65536), "batch=65536 outside [0, 65535]"),
           (dict(frames=-1), "frames=-1, need >= 0"), (dict(frames=1 << 23), "above 2^30"),
           (dict(ws_bytes=need - 1), "workspace too small"), (dict(ws=None), "workspace too small")]
    for change, message in bad:
        assert call(**change) == 1, change
        got = lib.smt_last_error().decode()
        assert got.startswith("smt_griffin_lim: ") and message in got, (change, got)
    assert call(batch=0) == 0 and call(frames=0) == 0 and call(batch=0, ws=None, ws_bytes=0, lens=None) == 0
    assert call(batch=0, n_fft=1000) == 1 and call(frames=0, momentum=1.0) == 1


def test_uniform_draw_is_exact_and_inside_the_open_interval():
    rng = np.random.default_rng(0)
    bits = np.concatenate([np.array([0, 2 ** 32 - 1, 511, 512], dtype=np.uint64), rng.integers(0, 2 ** 32, 4096, dtype=np.uint64)])
    u32 = G.uniform_from_bits(bits)
    assert u32.dtype == np.float32
    exact = ((bits >> 9).astype(np.float64) + 0.5) * 2.0 ** -23           # 24 significant bits: representable
    assert np.array_equal(u32.astype(np.float64), exact)
    assert u32.min() > 0.0 and u32.max() < 1.0
    assert float(u32[0]) == 2.0 ** -24 and float(u32[1]) == 1.0 - 2.0 ** -24
    # the hash itself: fmix32 of MurmurHash3 (0 is its fixed point; the avalanche of 1 is a published value)
    assert int(G.fmix32(0)) == 0 and int(G.fmix32(1)) == 0x514E28B7
    a, b = G.hash_phases(3, 5, 129), G.hash_phases(3, 9, 129)
    assert a.dtype == torch.float32 and torch.equal(a, b[:, :5])          # a draw depends on (seed, f, k) only
    assert not torch.equal(a, G.hash_phases(4, 5, 129))
    assert float(a.min()) > 0 and float(a.max()) < 2 * np.pi


@pytest.mark.parametrize("cfg", G.CONFIGS)
def test_reference_without_iterations_is_the_inverse_stft(cfg):
    for frames in G.frame_counts(cfg):
        S, phi = G.item(cfg, frames, 0)
        assert S.shape == (cfg[0] // 2 + 1, frames) and float(S.max(0).values.min()) > 1e-3        # no frame silent
        got = G.griffin_lim_ref(S, phi, cfg, 0, G.MOMENTUM)
        want = H.stft_inverse64(S[None], phi[None], cfg)[0, 0]
        assert got.shape == want.shape == (G.samples_of(cfg, frames),)
        assert H.num_frames(got.shape[0], cfg[0], cfg[1]) == frames
        assert H.max_abs(got, want) <= 1e-12 * float(want.abs().max())
        # the fp32 restatement's own transforms are the float64 ones to fp32 rounding
        x = got.float()
        r64 = G.stft(x, cfg)
        assert float((G.stft(x, cfg, torch.float32).to(torch.complex128) - r64).abs().max()) <= 1e-5 * float(r64.abs().max())


def test_case_table_frame_counts():
    assert [G.f_min(c) for c in G.CONFIGS] == [2, 2, 3, 5, 4]
    assert G.frame_counts((1024, 256, 1024)) == [2, 3, 4, 5, 9] and G.frame_counts((512, 50, 240)) == [5, 9]
    assert G.ragged_lens((1024, 256, 1024)) == [9, 4, 0, 5, 2] and G.ragged_lens((512, 50, 240)) == [9, 5, 0, 5, 5]


@pytest.mark.parametrize("front", range(len(G.MEL_FRONT_ENDS)))
def test_nnls_residual_falls_with_the_iteration_count(front):
    for log_input in (True, False):
        mel, lens, basis = G.mel_case(front, 65, log_input)
        res = [G.nnls_residual(G.mel_invert_ref(mel, lens, basis, n, log_input)[0], mel[0], basis, log_input) for n in G.MEL_ITERS]
        print(front, log_input, res)
        assert all(a > b for a, b in zip(res, res[1:])), res
        ref = G.mel_invert_ref(mel, lens, basis, 32, log_input)
        assert float(ref.min()) >= 0 and (ref[1][:, lens[1]:] == 0).all() and (ref[2] == 0).all()
        uncovered = basis.sum(0) == 0
        assert uncovered.any() and (ref[:, uncovered] == 0).all()


def test_scalar_floors_are_four_times_the_largest_host_e32():
    """SC_FLOOR and ROUNDTRIP_FLOOR are written down in the helper; here they are recomputed from the two host restatements.
    The iteration amplifies rounding differences, so another CPU's FFT gives another figure of the same size: within 4x."""
    sc, rt = G.sc_floor(), G.roundtrip_floor()
    print(f"sc floor {sc:.3g} (written {G.SC_FLOOR:.3g}); round-trip floor {rt:.3g} (written {G.ROUNDTRIP_FLOOR:.3g})")
    assert G.SC_FLOOR / 4 <= sc <= G.SC_FLOOR * 4
    assert G.ROUNDTRIP_FLOOR / 4 <= rt <= G.ROUNDTRIP_FLOOR * 4


def _mel_args():
    return torch.zeros(80, 513), torch.zeros(80, 2, dtype=torch.int32)


def test_python_ops_refuse_on_the_host():
    from smt_amd import spectral
    basis, band = _mel_args()
    mel, mag = torch.zeros(2, 80, 16), torch.zeros(2, 513, 16)
    good = torch.tensor([16, 8])
    bad_lens = [(torch.tensor([16, 17]), "item 1 has 17 frames, outside \\[0, frames=16\\]"), (torch.tensor([-1, 4]), "item 0 has -1 frames"),
                (torch.tensor([16]), "2 lengths"), (torch.tensor([16.0, 1.0]), "integer tensor on the CPU"),
                ([16, 16], "integer tensor on the CPU")]
    for lens, message in bad_lens:
        with pytest.raises(ValueError, match="mel_invert: .*" + message):
            spectral.mel_invert(mel, lens, basis, band)
        with pytest.raises(ValueError, match="griffin_lim: .*" + message):
            spectral.griffin_lim(mag, lens, 1024, 256, 1024)
    with pytest.raises(ValueError, match="n_iter=-1"):
        spectral.mel_invert(mel, good, basis, band, n_iter=-1)
    with pytest.raises(ValueError, match="n_mels=80"):
        spectral.mel_invert(torch.zeros(2, 40, 16), good, basis, band)
    gl = [(dict(lens=torch.tensor([16, 1])), "item 1 has 1 frames = 256 samples, not more than the reflect padding 384"),
          (dict(n_fft=1000), "n_fft=1000 unsupported"), (dict(hop=0), "hop=0 outside"), (dict(n_iter=-1), "n_iter=-1"),
          (dict(momentum=1.0), "momentum=1.0 outside"), (dict(mag=torch.zeros(2, 512, 16)), "n_fft/2\\+1=513"),
          (dict(seed=3, phase0=torch.zeros(2, 513, 16)), "either seed or phase0, not both"),
          (dict(phase0=torch.zeros(2, 513, 15)), "phase0 must have mag's shape"),
          (dict(seed=[1, 2, 3]), "seed must be an int or 2 ints"), (dict(seed=[1, -2]), "seed must be an int or 2 ints")]
    for change, message in gl:
        kw = dict(mag=mag, lens=good, n_fft=1024, hop=256, n_iter=32, momentum=0.99, seed=0, phase0=None)
        kw.update(change)
        with pytest.raises(ValueError, match=message):
            spectral.griffin_lim(kw["mag"], kw["lens"], kw["n_fft"], kw["hop"], 1024, n_iter=kw["n_iter"], momentum=kw["momentum"],
                                 seed=kw["seed"], phase0=kw["phase0"])
    assert [spectral.inverse_samples(f, 1024, 256) for f in (0, 1, 2, 16)] == [0, 256, 512, 4096]
    assert [spectral.invertible(f, 1024, 256) for f in (1, 2)] == [False, True]
    assert [spectral.invertible(f, 512, 50) for f in (4, 5)] == [False, True]


def test_lens_on_the_device_are_refused():
    """A tensor that says it is on the device (no GPU needed to build one: the check reads .is_cuda alone)."""
    from smt_amd import spectral

    class OnDevice(torch.Tensor):
        is_cuda = True

    lens = torch.tensor([16, 8]).as_subclass(OnDevice)
    basis, band = _mel_args()
    with pytest.raises(ValueError, match="integer tensor on the CPU"):
        spectral.mel_invert(torch.zeros(2, 80, 16), lens, basis, band)
    with pytest.raises(ValueError, match="integer tensor on the CPU"):
        spectral.griffin_lim(torch.zeros(2, 513, 16), lens, 1024, 256, 1024)


def test_synthesize_refuses_bad_vocoder_flags(tmp_path):
    from scripts import synthesize
    base = ["--log_dir", str(tmp_path), "--ckpt_num", "1", "--tokens", str(tmp_path / "t.txt")]
    assert synthesize.parse_args(base).vocoder is None and synthesize.parse_args(base).gl_iters == 32
    with pytest.raises(SystemExit):
        synthesize.parse_args(base + ["--vocoder", "wavenet"])
    with pytest.raises(ValueError, match="--gl_iters must be >= 0"):
        synthesize.main(base + ["--vocoder", "griffin_lim", "--gl_iters", "-1"])
    with pytest.raises(ValueError, match="--gl_iters applies to --vocoder griffin_lim"):
        synthesize.main(base + ["--gl_iters", "8"])

    class Waveform:
        pass

    with pytest.raises(ValueError, match="--vocoder applies to a token-to-spectrogram model; Waveform makes waveforms itself"):
        synthesize.refuse_vocoder_for(Waveform())
