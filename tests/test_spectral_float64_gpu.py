"""The STFT loss (forward and backward), STFT magnitude, log-mel and inverse STFT kernels of csrc/spectral.hip against the
plain float64 references of tests/spectral_ref_helpers.py (pinned to the upstream fixtures by tests/test_spectral_ref_cpu.py),
on a fixed table of small cases: six (n_fft, hop, win) configurations -- all four transform sizes, one with n_fft - hop odd --
at three lengths each: pad + 1 (every frame reflects on both sides), n_fft + hop + 3 and 3 n_fft + 17 (odd: items 1 and 2 start
off 16-byte alignment; left-edge, interior and right-edge frames); frame counts 1 .. 31 with every remainder modulo the four
frames of a workgroup; lens that put the mask boundary exactly on a frame's centre tap and one sample behind it, lens 0 and 1;
mel filterbanks of 20, 80 and 128 filters, four of them empty at n_fft 256; inverses of 1, 2 and 7 frames.

Both implementations of the frame kernels run the loss, magnitude and mel cases: the one-wave form in this process, the
whole-workgroup form (SMT_FFT_NT=256, read once per process) in ONE child process per module run.

Tolerances.  E32 is the error of the oracle's fp32 formulation of the same operation (DFT as conv1d, fp32 autograd) against the
float64 reference, computed per case; the kernels get 4 x E32 (an FFT and a DFT matmul have different error constants at the
same precision), with the bounds tests/test_spectral_gpu.py already uses for the same quantities as floors:
magnitudes max abs <= max(4 E32, 2e-6 max|ref|); loss relative <= max(4 E32, 2e-5); mel abs <= max(4 E32, 2e-5); inverse
max abs <= max(4 E32, 1e-5 max|ref|); gradient, relative L2 and max abs / max|ref| over the live items,
<= max(4 E32, 2e-4) with the log term and <= max(4 E32, 2e-5) without.  Exact: the gradient is 0.0 on items without a live
frame and wherever the float64 gradient is exactly 0 (samples no kept frame reaches, zero window taps); the backward is
bit-identical run to run; permuting the batch permutes dyh bit for bit; an identical-silence item gets gradient 0.0 and leaves
the others' bits alone.

Measured on an MI355X, worst case per configuration over its lengths and lens sets, "kernel error / E32" (every case is within its
bound; the two maxima of a cell may come from different cases):

  config         form       loss (rel)         grad log, rel-L2   grad log, max/max  grad lin, rel-L2   grad lin, max/max  magnitude / max    mel (abs)
  2048-240-1200  one-wave   1.3e-07 / 2.4e-07  2.6e-05 / 8.8e-05  2.7e-05 / 8.2e-05  9.8e-07 / 2.9e-06  1.0e-06 / 3.8e-06  1.7e-07 / 2.2e-06  9.0e-07 / 2.0e-06
  2048-240-1200  workgroup  5.9e-08 / 2.4e-07  2.6e-05 / 8.8e-05  2.5e-05 / 8.2e-05  4.5e-07 / 2.9e-06  5.4e-07 / 3.8e-06  1.3e-07 / 2.2e-06  7.7e-07 / 2.0e-06
  1024-120-600   one-wave   7.3e-07 / 4.4e-07  4.8e-05 / 9.2e-05  4.9e-05 / 9.4e-05  8.9e-07 / 2.1e-06  9.4e-07 / 2.3e-06  1.6e-07 / 8.6e-07  1.2e-06 / 1.3e-06
  1024-120-600   workgroup  8.2e-07 / 4.4e-07  5.3e-05 / 9.2e-05  5.5e-05 / 9.4e-05  4.7e-07 / 2.1e-06  6.1e-07 / 2.3e-06  1.8e-07 / 8.6e-07  9.3e-07 / 1.3e-06
  1024-256-1024  one-wave   3.4e-07 / 2.6e-07  5.0e-05 / 1.1e-04  5.5e-05 / 1.2e-04  1.2e-06 / 4.4e-06  1.2e-06 / 4.4e-06  1.5e-07 / 9.6e-07  8.6e-07 / 1.1e-06
  1024-256-1024  workgroup  1.6e-07 / 2.6e-07  2.1e-05 / 1.1e-04  1.9e-05 / 1.2e-04  7.0e-07 / 4.4e-06  8.3e-07 / 4.4e-06  1.8e-07 / 9.6e-07  5.4e-07 / 1.1e-06
  512-50-240     one-wave   4.5e-07 / 2.7e-07  6.0e-05 / 4.6e-05  5.7e-05 / 4.3e-05  7.1e-07 / 1.2e-06  7.2e-07 / 1.2e-06  1.3e-07 / 6.8e-07  2.4e-06 / 1.8e-06
  512-50-240     workgroup  3.5e-07 / 2.7e-07  6.0e-05 / 4.6e-05  5.7e-05 / 4.3e-05  3.8e-07 / 1.2e-06  4.0e-07 / 1.2e-06  1.5e-07 / 6.8e-07  2.9e-06 / 1.8e-06
  512-75-300     one-wave   5.4e-07 / 4.0e-07  1.5e-04 / 1.1e-04  1.5e-04 / 1.1e-04  7.7e-07 / 1.7e-06  8.0e-07 / 1.5e-06  1.6e-07 / 7.3e-07  2.4e-06 / 8.8e-06
  512-75-300     workgroup  4.0e-07 / 4.0e-07  1.5e-04 / 1.1e-04  1.5e-04 / 1.1e-04  4.9e-07 / 1.7e-06  4.4e-07 / 1.5e-06  1.4e-07 / 7.3e-07  3.6e-06 / 8.8e-06
  256-64-256     one-wave   6.3e-07 / 1.2e-06  3.2e-05 / 7.7e-06  2.5e-05 / 7.9e-06  1.5e-06 / 2.3e-06  1.4e-06 / 2.3e-06  1.5e-07 / 5.8e-07  2.2e-06 / 2.5e-06
  256-64-256     workgroup  2.1e-07 / 1.2e-06  8.6e-06 / 7.7e-06  7.1e-06 / 7.9e-06  5.5e-07 / 2.3e-06  8.4e-07 / 2.3e-06  1.2e-07 / 5.8e-07  2.1e-06 / 2.5e-06
  inverse (error / max|ref|): 2048-240-1200 1.8e-07 / 3.9e-07, 512-50-240 1.9e-07 / 4.0e-07, 256-64-256 1.6e-07 / 5.9e-07,
  1024-256-1024 1.7e-07 / 9.3e-07.  Multi-resolution loss: 7.7e-08 / 6.0e-08, gradient rel-L2 2.2e-05 / 2.0e-05.

The log gradient at (512, 75, 300), T 590 (1.5e-4 in both forms, E32 1.1e-4) is the largest: its smallest live bin is 6.4e-3, and
the log term's 1 / |Yh|^2 turns the ~1e-7 fp32 noise of that bin into a few 1e-5 of its own gradient row.

Single-line mutations of spectral.hip, each tried on a scratch copy: the keep test of the one-wave forward `<` -> `<=`, the `-i`
candidate of stft_overlap_gather_kernel dropped, the right-hand branch of reflect_index off by one -- each fails all 18 cases
of test_stft_loss_and_gradient_match_float64[*-one-wave] (the third also all of test_magnitude_and_log_mel_match_float64).
"""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import spectral_ref_helpers as H

pytestmark = pytest.mark.gpu

FORMS = ["one-wave", "workgroup"]
CASES = [(cfg, t) for cfg in H.CONFIGS for t in H.lengths(cfg)]
TESTS = os.path.dirname(os.path.abspath(__file__))
_child = {}


def workgroup_results():
    """The whole table through the whole-workgroup form: one fresh child process per module run (the library reads SMT_FFT_NT
    once per process).  A non-zero exit or a timeout fails every test that asks; it is not tried again."""
    if not _child:
        repo = os.path.dirname(TESTS)
        code = (f"import sys; sys.path[:0] = [{TESTS!r}, {os.path.join(repo, 'speech-masters-thesis_amd')!r}, {repo!r}]; "
                "import spectral_ref_helpers as H; H.run_all_cases(sys.argv[1])")
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "nt256.pt")
            try:
                r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, SMT_FFT_NT="256"), timeout=300,
                                   capture_output=True, text=True)
                if r.returncode == 0:
                    _child["results"] = torch.load(path, weights_only=True)
                else:
                    _child["error"] = f"child exited with {r.returncode}: {r.stderr[-2000:]}"
            except subprocess.TimeoutExpired:
                _child["error"] = "child timed out"
    if "error" in _child:
        pytest.fail(_child["error"])
    return _child["results"]


def ident(v):
    return "-".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cfg,t", CASES, ids=ident)
def test_stft_loss_and_gradient_match_float64(cfg, t, form):
    for use_log in (True, False):
        for i, lens in enumerate(H.lens_sets(cfg, t)):
            key = H.loss_key(cfg, t, use_log, i)
            if form == "workgroup":
                H.check_loss_case(key, *workgroup_results()[key], form=form)
                continue
            y, yh = H.make_signals(cfg, t)
            loss, grad = H.run_loss(y, yh, lens, cfg, use_log)
            H.check_loss_case(key, loss, grad, form=form)
            loss2, grad2 = H.run_loss(y, yh, lens, cfg, use_log)
            assert torch.equal(loss, loss2) and torch.equal(grad, grad2), (key, "not bit-identical run to run")
            perm = [2, 0, 1]
            _, grad_p = H.run_loss(y[perm], yh[perm], [lens[p] for p in perm], cfg, use_log)
            assert torch.equal(grad_p, grad[perm]), (key, "a permuted batch does not permute dyh bit for bit")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cfg,t", CASES, ids=ident)
def test_magnitude_and_log_mel_match_float64(cfg, t, form):
    x = H.make_signals(cfg, t)[0]
    mag = workgroup_results()[H.mag_key(cfg, t)] if form == "workgroup" else H.run_magnitude(x, cfg)
    H.check_magnitude_case(cfg, t, mag, form=form)
    if form == "one-wave":                                   # the [B, 1, T] input form of the module
        assert torch.equal(H.run_magnitude(x.unsqueeze(1), cfg), mag)
    mels = [c for c in H.MEL_CASES if c[0] == cfg]
    assert mels
    for _, n_mels, f_max in mels:
        key = H.mel_key(cfg, n_mels, t)
        mel = workgroup_results()[key] if form == "workgroup" else H.run_mel(x, cfg, n_mels, f_max)
        H.check_mel_case(cfg, n_mels, f_max, t, mel, form=form)
        if form == "one-wave":                               # a 1-D input adds a batch dimension
            one = H.run_mel(x[1], cfg, n_mels, f_max)
            assert one.shape == (1,) + mel.shape[1:] and torch.equal(one[0], mel[1])


def test_multi_resolution_loss_equals_the_sum_of_the_per_resolution_references():
    from models.vqvae.losses import MultiResolutionSpectralLoss
    t = 3 * 512 + 17                        # accepted by all three resolutions (2048 needs more than 904 samples)
    lens = [t, 700, 0]
    y, yh = H.make_signals((0, 0, 0), t)
    n_ffts, hops, wins = (list(v) for v in zip(*H.MODEL_RESOLUTIONS))
    mod = MultiResolutionSpectralLoss(n_ffts=n_ffts, hop_lengths=hops, win_lengths=wins, window="hann", log=True)
    yhd = yh.cuda().requires_grad_(True)
    loss = mod(y.cuda(), yhd, torch.tensor(lens, dtype=torch.int32).cuda())
    grad, = torch.autograd.grad(loss * H.UPSTREAM, yhd)
    grad = grad.double().cpu()
    refs = [H.stft_loss64(y, yh, lens, cfg, True, upstream=H.UPSTREAM / 3) for cfg in H.MODEL_RESOLUTIONS]
    r32 = [H.stft_loss32(y, yh, lens, cfg, True, upstream=H.UPSTREAM / 3) for cfg in H.MODEL_RESOLUTIONS]
    assert min(r["min_live_bin"] for r in refs) >= 1e-3
    loss64, grad64 = sum(r["loss"] for r in refs) / 3, sum(r["grad"] for r in refs)
    loss32, grad32 = sum(r[0] for r in r32) / 3, sum(r[1] for r in r32)
    e32 = (abs(loss32 - loss64) / loss64, H.rel_l2(grad32[:2], grad64[:2]), H.rel_max(grad32[:2], grad64[:2]))
    err = (abs(loss.item() - loss64) / loss64, H.rel_l2(grad[:2], grad64[:2]), H.rel_max(grad[:2], grad64[:2]))
    print("multi-resolution: loss, grad rel-L2, grad max/max: err", err, "E32", e32)
    assert err[0] <= H.bound_loss(e32[0])
    assert err[1] <= H.bound_grad(e32[1], True) and err[2] <= H.bound_grad(e32[2], True)
    assert (grad[2] == 0.0).all() and (grad[grad64 == 0.0] == 0.0).all() and torch.isfinite(grad).all()


@pytest.mark.parametrize("cfg", H.CONFIGS, ids=ident)
def test_identical_silence_item_gets_zero_gradient_and_leaves_the_others_alone(cfg):
    """y == yh == 0 on item 1: its sums are exactly 0, where d sqrt(S) / dS is infinite -- the kernels define the gradient as 0.
    The other items' gradients are those of the batch without it, bit for bit: the upstream factors 3.0 (three items) and 2.0
    (two) make g / (2 B), the only place the batch size enters, the same number."""
    t = cfg[0] + cfg[1] + 3
    y, yh = H.make_signals(cfg, t)
    y[1], yh[1] = 0.0, 0.0
    lens = [t, t, t]
    for use_log in (True, False):
        loss, grad = H.run_loss(y, yh, lens, cfg, use_log, upstream=3.0)
        ref = H.stft_loss64(y, yh, lens, cfg, use_log, upstream=3.0)
        loss32, grad32 = H.stft_loss32(y, yh, lens, cfg, use_log, upstream=3.0)
        assert torch.isfinite(loss) and torch.isfinite(grad).all()
        assert (grad[1] == 0.0).all() and (ref["grad"][1] == 0.0).all()
        assert abs(loss.item() - ref["loss"]) / ref["loss"] <= H.bound_loss(abs(loss32 - ref["loss"]) / ref["loss"])
        # E32 over the other two items: the oracle's sqrt(re^2 + im^2) has no finite fp32 autograd at a zero spectrum
        others = [0, 2]
        assert H.rel_l2(grad[others], ref["grad"][others]) <= H.bound_grad(H.rel_l2(grad32[others], ref["grad"][others]), use_log)
        _, grad2 = H.run_loss(y[[0, 2]], yh[[0, 2]], [t, t], cfg, use_log, upstream=2.0)
        assert torch.equal(grad[[0, 2]], grad2)


@pytest.mark.parametrize("frames,phase_scale", [(1, 1.0), (2, 1.0), (7, 1.0), (7, 100 / 3.141592653589793)],
                         ids=["1", "2", "7", "7-phases-to-100-rad"])
@pytest.mark.parametrize("cfg", [H.CONFIGS[0], H.CONFIGS[2], H.CONFIGS[3], H.CONFIGS[4]], ids=ident)
def test_stft_inverse_matches_float64(cfg, frames, phase_scale):
    from datasets.transforms import STFT
    mag, phase, ref, e32 = H.inverse_reference(cfg, frames, phase_scale)
    out = STFT(n_fft=cfg[0], hop_length=cfg[1], win_length=cfg[2], window="hann").inverse(mag.cuda(), phase.cuda()).cpu()
    assert out.shape == ref.shape
    err = H.max_abs(out, ref)
    print(f"inverse {ident(cfg)} frames {frames} |phase| <= {float(phase.abs().max()):.4g}: max|ref| {float(ref.abs().max()):.4g} "
          f"err {err:.3g} E32 {e32:.3g}")
    assert err <= H.bound_inverse(e32, ref)
