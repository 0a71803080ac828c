"""Shared by the float64 tests of the spectral kernels (csrc/spectral.hip behind smt_amd.spectral, datasets.transforms.STFT /
MelSpectrogram and models.vqvae.losses.MultiResolutionSpectralLoss): a plain float64 reference of every operation, the error
of the oracle's fp32 formulation of the same operation against it (E32, the yardstick of the tolerances), the fixed case
table, and the functions that run the kernels on a case (in the test process, or in a child started with SMT_FFT_NT=256).

The references are written from the formulas, not from the kernels:
  magnitude  reflect-pad by pad = (n_fft - hop) // 2, frames every hop (unfold), times the window, rfft, abs.  The window is
             the table the kernels read: the fp32 values of oracle.vqvae_oracle.stft_window, cast to double.
  loss       frame f of item b is kept iff n_fft // 2 - pad + f * hop < lens[b]; mean_b sqrt(sum ((|Y| - |Yh|) m)^2), plus the
             same on log(clamp(., 1e-5)) with use_log.  An item whose sum is exactly 0 (no kept frame, or y == yh) contributes 0
             with ZERO gradient: torch's autograd of sqrt gives inf * 0 = nan there, the kernels define it as 0, and so does
             zero_safe_sqrt below (the only place where the reference departs from the literal upstream expression).
  gradient   float64 autograd of the above.
  log-mel    log(clamp(basis @ magnitude, 1e-5)) with the fp32 filterbank the kernel reads, cast to double.
  inverse    irfft of mag * exp(i phase) per frame (the imaginary parts of bins 0 and n_fft / 2 dropped: they meet zero rows
             of the upstream pseudo-inverse basis), times the window, overlap-add, divided by the window sum-square where it
             exceeds float32 tiny, pad trimmed on both sides.
tests/test_spectral_ref_cpu.py pins all of them to the committed upstream fixtures.

Every reference is computed once per case and cached; callers must not modify what they get.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vqvae_oracle as orc

# (n_fft, hop, win): the three model resolutions, the smallest transform, the mel front end, and one with n_fft - hop odd
CONFIGS = [(2048, 240, 1200), (1024, 120, 600), (512, 50, 240), (256, 64, 256), (1024, 256, 1024), (512, 75, 300)]
MODEL_RESOLUTIONS = CONFIGS[:3]
BATCH = 3
UPSTREAM = 3.0                    # the backward runs through (loss * 3.0).backward()
SAMPLE_RATE = 22050
CLAMP = 1e-5
SEED = 1          # with it every live bin of |Y| and |Yh| in the table is >= 1e-3 (asserted per case): nothing near the clamp
FLOAT32_TINY = float(np.finfo(np.float32).tiny)


def pad_of(n_fft, hop):
    return (n_fft - hop) // 2


def num_frames(t, n_fft, hop):
    return (t + 2 * pad_of(n_fft, hop) - n_fft) // hop + 1


def lengths(cfg):
    """Per configuration: pad + 1 (the shortest accepted clip: every frame reflects on both sides), n_fft + hop + 3, and
    3 n_fft + 17 (odd, so items 1 and 2 start off 16-byte alignment; left-edge, interior and right-edge frames).  A fourth
    is not needed: over the table frames % 4 -- four frames share a workgroup in the one-wave form -- takes 0, 1, 2 and 3
    (frame counts 3, 9, 25 / 3, 9, 25 / 4, 11, 31 / 1, 5, 12 / 1, 5, 12 / 2, 7, 20;
    tests/test_spectral_ref_cpu.py::test_case_table_covers_every_frame_remainder)."""
    n_fft, hop, _ = cfg
    return [pad_of(n_fft, hop) + 1, n_fft + hop + 3, 3 * n_fft + 17]


def centre_tap(cfg, k):
    """Sample under the centre tap of frame k: the frame is kept iff it is < lens[b]."""
    n_fft, hop, _ = cfg
    return n_fft // 2 - pad_of(n_fft, hop) + k * hop


def lens_sets(cfg, t):
    """[T, c_k, 0] and [c_k + 1, 1, T] for the frame k in the middle: with lens == c_k frame k is the first one dropped, with
    c_k + 1 the last one kept; lens 0 and 1 leave no live frame (frame 0's centre tap is at n_fft // 2 - pad >= 32)."""
    c = centre_tap(cfg, num_frames(t, cfg[0], cfg[1]) // 2)
    assert 1 < c < t
    return [t, c, 0], [c + 1, 1, t]


def make_signals(cfg, t, batch=BATCH):
    """y uniform noise of amplitude 0.5, yh = y + 0.05 randn, fp32 [batch, t]."""
    g = torch.Generator().manual_seed(SEED + cfg[0] * 131 + cfg[1] * 7 + t)
    y = (torch.rand(batch, t, generator=g) * 2 - 1) * 0.5
    yh = y + 0.05 * torch.randn(batch, t, generator=g)
    return y.contiguous(), yh.contiguous()


# ---------------------------------------------------------------------------------------------- float64 references

@functools.lru_cache(maxsize=None)
def window64(n_fft, win):
    return torch.from_numpy(orc.stft_window(n_fft, win)).double()


@functools.lru_cache(maxsize=None)
def basis32(n_fft, win):
    return orc.stft_forward_basis(n_fft, win)


def spectrum64(x, cfg):
    """x [B, T] -> complex128 [B, frames, n_fft / 2 + 1]."""
    n_fft, hop, win = cfg
    pad = pad_of(n_fft, hop)
    xp = F.pad(x.double().unsqueeze(1), (pad, pad), mode="reflect")[:, 0]
    return torch.fft.rfft(xp.unfold(-1, n_fft, hop) * window64(n_fft, win), dim=-1)


def magnitude64(x, cfg):
    """x [B, T] -> |STFT| float64 [B, n_fft / 2 + 1, frames] (the layout of STFT.forward)."""
    return spectrum64(x, cfg).abs().transpose(1, 2)


def keep_mask(lens, cfg, frames):
    """bool [B, frames]."""
    centre = centre_tap(cfg, torch.arange(frames))
    return centre[None, :] < torch.as_tensor(lens)[:, None]


def zero_safe_sqrt(s):
    """sqrt(s) with value 0 and gradient 0 where s == 0 (see the module docstring)."""
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def loss_from_magnitudes(my, mh, keep, use_log):
    """my, mh [B, bins, frames] (any float dtype), keep bool [B, frames] -> scalar."""
    m = keep[:, None, :].to(my.dtype)
    loss = zero_safe_sqrt((((my - mh) * m) ** 2).sum((1, 2))).mean()
    if use_log:
        dl = torch.log(my.clamp(min=CLAMP)) - torch.log(mh.clamp(min=CLAMP))
        loss = loss + zero_safe_sqrt(((dl * m) ** 2).sum((1, 2))).mean()
    return loss


def stft_loss64(y, yh, lens, cfg, use_log, upstream=UPSTREAM):
    """float64: dict(loss, grad = d(upstream * loss)/dyh [B, T], keep [B, frames], live [B], min_live_bin)."""
    yh64 = yh.double().requires_grad_(True)
    my, mh = magnitude64(y, cfg), magnitude64(yh64, cfg)
    keep = keep_mask(lens, cfg, my.shape[-1])
    loss = loss_from_magnitudes(my, mh, keep, use_log)
    grad, = torch.autograd.grad(loss * upstream, yh64)
    live_bins = torch.minimum(my, mh.detach()).transpose(1, 2)[keep]
    return dict(loss=float(loss.detach()), grad=grad, keep=keep, live=keep.any(1),
                min_live_bin=float(live_bins.min()) if live_bins.numel() else float("inf"))


def stft_loss32(y, yh, lens, cfg, use_log, upstream=UPSTREAM):
    """The same loss on the oracle's fp32 magnitudes (DFT as conv1d, oracle.vqvae_oracle.stft_magnitude), fp32 autograd."""
    n_fft, hop, win = cfg
    yh32 = yh.float().clone().requires_grad_(True)
    basis = basis32(n_fft, win)
    my, mh = orc.stft_magnitude(y.float(), n_fft, hop, win, basis), orc.stft_magnitude(yh32, n_fft, hop, win, basis)
    loss = loss_from_magnitudes(my, mh, keep_mask(lens, cfg, my.shape[-1]), use_log)
    grad, = torch.autograd.grad(loss * upstream, yh32)
    return float(loss.detach()), grad


def log_mel64(x, cfg, basis):
    """basis fp32 [n_mels, bins] as the kernel reads it -> dict(mel [B, n_mels, frames], sums = basis @ magnitude)."""
    sums = torch.matmul(basis.double(), magnitude64(x, cfg))
    return dict(mel=torch.log(sums.clamp(min=CLAMP)), sums=sums)


def stft_inverse64(mag, phase, cfg):
    """mag, phase [B, bins, frames] -> float64 [B, 1, (frames - 1) hop + n_fft - 2 pad]."""
    n_fft, hop, win = cfg
    pad, frames = pad_of(n_fft, hop), mag.shape[-1]
    w = window64(n_fft, win)
    spec = torch.polar(mag.double(), phase.double()).transpose(1, 2).clone()
    spec[..., 0] = spec[..., 0].real + 0j
    spec[..., -1] = spec[..., -1].real + 0j
    rows = torch.fft.irfft(spec, n=n_fft, dim=-1) * w
    total = n_fft + hop * (frames - 1)
    out = torch.zeros(mag.shape[0], total, dtype=torch.float64)
    wss = torch.zeros(total, dtype=torch.float64)
    for f in range(frames):
        out[:, f * hop:f * hop + n_fft] += rows[:, f]
        wss[f * hop:f * hop + n_fft] += w * w
    nz = wss > FLOAT32_TINY
    out[:, nz] /= wss[nz]
    return out[:, pad:total - pad].unsqueeze(1)


# ------------------------------------------------------------------------------------- metrics, E32 and the bounds

def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rel_max(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def max_abs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


# Floors: the bounds tests/test_spectral_gpu.py already uses for the same quantities.  The factor 4 on E32 covers the different
# error constants of an FFT and a DFT matmul at the same precision.
def bound_magnitude(e32, ref):
    return max(4 * e32, 2e-6 * float(ref.abs().max()))


def bound_loss(e32):
    return max(4 * e32, 2e-5)


def bound_mel(e32):
    return max(4 * e32, 2e-5)


def bound_inverse(e32, ref):
    return max(4 * e32, 1e-5 * float(ref.abs().max()))


def bound_grad(e32, use_log):
    return max(4 * e32, 2e-4 if use_log else 2e-5)


# ------------------------------------------------------------------------------------------------------ case table

def loss_cases():
    """[(key, cfg, t, use_log, lens)] -- every configuration x length x use_log x lens set."""
    out = []
    for cfg in CONFIGS:
        for t in lengths(cfg):
            for use_log in (True, False):
                for i, lens in enumerate(lens_sets(cfg, t)):
                    out.append((loss_key(cfg, t, use_log, i), cfg, t, use_log, lens))
    return out


def loss_key(cfg, t, use_log, i):
    return f"loss/{cfg[0]}-{cfg[1]}-{cfg[2]}/T{t}/log{int(use_log)}/lens{i}"


# (cfg, n_mels, f_max): 80 filters at n_fft 256 leave four EMPTY (their band lies between two bins); 128 and 80 are above the 64
# lanes that walk the filters, 20 below
MEL_CASES = [((256, 64, 256), 80, 8000.0), ((512, 50, 240), 80, 8000.0), ((512, 75, 300), 80, 8000.0),
             ((1024, 120, 600), 80, 8000.0), ((1024, 256, 1024), 80, 8000.0), ((1024, 256, 1024), 20, 8000.0),
             ((2048, 240, 1200), 128, None)]


def mel_key(cfg, n_mels, t):
    return f"mel/{cfg[0]}-{cfg[1]}-{cfg[2]}/m{n_mels}/T{t}"


def mag_key(cfg, t):
    return f"mag/{cfg[0]}-{cfg[1]}-{cfg[2]}/T{t}"


@functools.lru_cache(maxsize=None)
def loss_reference(cfg, t, use_log, i):
    """(y, yh, lens, ref64 dict, loss32, grad32) of one loss case; computed once, shared, read-only."""
    y, yh = make_signals(cfg, t)
    lens = lens_sets(cfg, t)[i]
    return (y, yh, lens, stft_loss64(y, yh, lens, cfg, use_log)) + stft_loss32(y, yh, lens, cfg, use_log)


@functools.lru_cache(maxsize=None)
def magnitude_reference(cfg, t):
    """(x, mag64, E32)."""
    x, _ = make_signals(cfg, t)
    ref = magnitude64(x, cfg)
    n_fft, hop, win = cfg
    return x, ref, max_abs(orc.stft_magnitude(x, n_fft, hop, win, basis32(n_fft, win)), ref)


@functools.lru_cache(maxsize=None)
def mel_module(cfg, n_mels, f_max):
    from datasets.transforms import MelSpectrogram
    n_fft, hop, win = cfg
    return MelSpectrogram(sample_rate=SAMPLE_RATE, n_fft=n_fft, win_length=win, hop_length=hop, n_mels=n_mels, f_min=0.0,
                          f_max=f_max)


@functools.lru_cache(maxsize=None)
def mel_reference(cfg, n_mels, f_max, t):
    """(x, dict(mel, sums) float64, E32, empty [n_mels] bool)."""
    x, _ = make_signals(cfg, t)
    basis = mel_module(cfg, n_mels, f_max).mel_basis.cpu()
    ref = log_mel64(x, cfg, basis)
    return x, ref, max_abs(orc.mel_spectrogram(x, basis, *cfg), ref["mel"]), (basis > 0).sum(1) == 0


def inverse_case(cfg, frames, phase_scale=1.0, batch=2):
    """Magnitudes uniform in [0, 3), phases uniform in (-pi, pi) times phase_scale, fp32 [batch, bins, frames]."""
    g = torch.Generator().manual_seed(cfg[0] + 17 * frames + int(phase_scale))
    bins = cfg[0] // 2 + 1
    mag = torch.rand(batch, bins, frames, generator=g) * 3
    phase = (torch.rand(batch, bins, frames, generator=g) * 2 - 1) * (np.pi * (1 - 1e-6)) * phase_scale
    return mag, phase


@functools.lru_cache(maxsize=None)
def inverse_reference(cfg, frames, phase_scale=1.0):
    """(mag, phase, y64, E32)."""
    mag, phase = inverse_case(cfg, frames, phase_scale)
    ref = stft_inverse64(mag, phase, cfg)
    return mag, phase, ref, max_abs(orc.stft_inverse(mag, phase, *cfg), ref)


# ------------------------------------------------------------------------------------------------ running the kernels

def run_loss(y, yh, lens, cfg, use_log, upstream=UPSTREAM):
    """smt_amd.spectral.stft_loss forward and backward on the device: (loss fp32 scalar, dyh [B, T]) on the host."""
    from smt_amd import spectral
    yd = y.cuda()
    yhd = yh.cuda().requires_grad_(True)
    loss = spectral.stft_loss(yd, yhd, torch.as_tensor(lens, dtype=torch.int32).cuda(), cfg[0], cfg[1], cfg[2], use_log)
    grad, = torch.autograd.grad(loss * upstream, yhd)
    return loss.detach().cpu(), grad.cpu()


def run_magnitude(x, cfg):
    from datasets.transforms import STFT
    return STFT(n_fft=cfg[0], hop_length=cfg[1], win_length=cfg[2], window="hann")(x.cuda()).cpu()


def run_mel(x, cfg, n_mels, f_max):
    return mel_module(cfg, n_mels, f_max).cuda()(x.cuda()).cpu()


def run_all_cases(path):
    """Every loss, magnitude and mel case of the table through the kernels of THIS process, results saved to `path` by key.
    The library reads SMT_FFT_NT once per process: the GPU test starts one child with SMT_FFT_NT=256 on this function."""
    out = {}
    for key, cfg, t, use_log, lens in loss_cases():
        y, yh = make_signals(cfg, t)
        out[key] = run_loss(y, yh, lens, cfg, use_log)
    for cfg in CONFIGS:
        for t in lengths(cfg):
            out[mag_key(cfg, t)] = run_magnitude(make_signals(cfg, t)[0], cfg)
    for cfg, n_mels, f_max in MEL_CASES:
        for t in lengths(cfg):
            out[mel_key(cfg, n_mels, t)] = run_mel(make_signals(cfg, t)[0], cfg, n_mels, f_max)
    torch.save(out, path)


# --------------------------------------------------------------------------------------------------------- checks

def check_loss_case(key, loss, grad, form=""):
    """The assertions on one loss case (forward value and dyh) against its float64 reference; prints every figure first."""
    _, cfg, t, use_log, i = parse_loss_key(key)
    y, yh, lens, ref, loss32, grad32 = loss_reference(cfg, t, use_log, i)
    assert ref["min_live_bin"] >= 1e-3, (key, ref["min_live_bin"])          # nothing near the 1e-5 clamp
    live, g64 = ref["live"], ref["grad"]
    grad = grad.double()
    e32_loss = abs(loss32 - ref["loss"]) / abs(ref["loss"])
    err_loss = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
    e32_l2, e32_max = rel_l2(grad32[live], g64[live]), rel_max(grad32[live], g64[live])
    err_l2, err_max = rel_l2(grad[live], g64[live]), rel_max(grad[live], g64[live])
    print(f"{key} {form}: frames {ref['keep'].shape[1]} lens {lens} min live bin {ref['min_live_bin']:.3g}; "
          f"loss {float(loss):.9g} ref {ref['loss']:.12g} err {err_loss:.3g} E32 {e32_loss:.3g}; "
          f"grad rel-L2 {err_l2:.3g} E32 {e32_l2:.3g}, max/max {err_max:.3g} E32 {e32_max:.3g}")
    assert torch.isfinite(grad).all(), key
    assert err_loss <= bound_loss(e32_loss), (key, form, err_loss, e32_loss)
    assert err_l2 <= bound_grad(e32_l2, use_log), (key, form, err_l2, e32_l2)
    assert err_max <= bound_grad(e32_max, use_log), (key, form, err_max, e32_max)
    assert live.tolist() == [n > centre_tap(cfg, 0) for n in lens]
    assert (grad[~live] == 0.0).all(), (key, form, "gradient on an item without a live frame")
    # samples no kept frame reaches, and samples only zero window taps reach
    zero = g64 == 0.0
    assert (grad[zero] == 0.0).all(), (key, form, int((grad[zero] != 0).sum()))
    return err_loss, err_l2, err_max, e32_loss, e32_l2, e32_max


def parse_loss_key(key):
    _, c, t, lg, ln = key.split("/")
    return key, tuple(int(v) for v in c.split("-")), int(t[1:]), bool(int(lg[3:])), int(ln[4:])


def check_magnitude_case(cfg, t, mag, form=""):
    x, ref, e32 = magnitude_reference(cfg, t)
    assert mag.shape == ref.shape, (cfg, t, mag.shape, ref.shape)
    err = max_abs(mag, ref)
    print(f"{mag_key(cfg, t)} {form}: frames {ref.shape[-1]} max|ref| {float(ref.max()):.4g} err {err:.3g} E32 {e32:.3g}")
    assert err <= bound_magnitude(e32, ref), (cfg, t, form, err, e32)
    return err, e32


def check_mel_case(cfg, n_mels, f_max, t, mel, form=""):
    x, ref, e32, empty = mel_reference(cfg, n_mels, f_max, t)
    assert mel.shape == ref["mel"].shape
    assert float(ref["sums"][:, ~empty].min()) >= 1e-4                      # nothing but the empty filters near the clamp
    err = max_abs(mel, ref["mel"])
    print(f"{mel_key(cfg, n_mels, t)} {form}: frames {mel.shape[-1]} empty filters {int(empty.sum())} "
          f"min non-empty sum {float(ref['sums'][:, ~empty].min()):.3g} err {err:.3g} E32 {e32:.3g}")
    assert err <= bound_mel(e32), (cfg, n_mels, t, form, err, e32)
    if empty.any():                                                         # both sides: log(1e-5), whatever the signal
        assert (ref["mel"][:, empty] == float(np.log(CLAMP))).all()
        assert float((mel[:, empty].double() - np.log(CLAMP)).abs().max()) <= 1e-6     # logf(1e-5f), to its rounding
    return err, e32
