"""Spectral front end and spectral loss on the HIP library (include/smt_hip.h, "spectral"):
in-LDS FFT instead of the reference's DFT-as-conv1d (datasets/transforms.py:86-123).

Window and twiddle tables are computed once per (n_fft, win_length) in float64 and cached on
the device; the kernels never evaluate sin/cos.
"""
import math

import torch

from . import native as N
from . import profiler

_tables = {}


_consts = {}


def _const(values, device):
    """A small fp32 constant on the device, uploaded once per (values, device): a fresh torch.tensor(..., device=cuda) in
    every backward is a pageable host-to-device copy -- a launch more, and not capturable in a hipGraph."""
    key = (tuple(float(v) for v in values), str(device))
    if key not in _consts:
        _consts[key] = torch.tensor(key[0], dtype=torch.float32, device=device)
    return _consts[key]


def _get_tables(n_fft, win_length, device):
    key = (n_fft, win_length, str(device))
    if key not in _tables:
        m = torch.arange(win_length, dtype=torch.float64)
        hann = 0.5 - 0.5 * torch.cos(2.0 * math.pi * m / win_length)       # periodic Hann (fftbins=True)
        window = torch.zeros(n_fft, dtype=torch.float64)
        lpad = (n_fft - win_length) // 2                                      # librosa.util.pad_center
        window[lpad:lpad + win_length] = hann
        k = torch.arange(n_fft // 2, dtype=torch.float64)
        ang = -2.0 * math.pi * k / n_fft
        tw = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)
        _tables[key] = (window.to(torch.float32).to(device), tw.to(torch.float32).contiguous().to(device))
    return _tables[key]


def num_frames(t, n_fft, hop):
    return (t + 2 * ((n_fft - hop) // 2) - n_fft) // hop + 1


def _check_length(what, t, n_fft, hop):
    """The library's own argument check (SMT_CHECK_STFT_LENGTH, csrc/spectral.hip), made before the outputs are sized:
    num_frames() is 0 or negative for such a signal, and a negative size would fail in torch.empty with another message."""
    pad = (n_fft - hop) // 2
    if t <= pad:
        raise RuntimeError(f"{what} failed (status 1): {what}: signal shorter than the reflect padding")
    if t + 2 * pad < n_fft:
        raise RuntimeError(f"{what} failed (status 1): {what}: signal shorter than one frame "
                           f"(t={t} + 2 * pad={pad} < n_fft={n_fft}, hop={hop})")


@torch.no_grad()
def stft_magnitude(x, n_fft, hop, win_length):
    """x [B, T] fp32 -> |STFT| [B, n_fft/2+1, frames] (STFT.forward, transforms.py:108-123)."""
    x = x.contiguous().float()
    b, t = x.shape
    _check_length("smt_stft_magnitude", t, n_fft, hop)
    window, tw = _get_tables(n_fft, win_length, x.device)
    frames = num_frames(t, n_fft, hop)
    mag = torch.empty(b, n_fft // 2 + 1, frames, dtype=torch.float32, device=x.device)
    with profiler.region("stft_mag", nbytes=x.numel() * 4 + mag.numel() * 4, bound="hbm"):
        N.check(N.lib().smt_stft_magnitude(N.ptr(x), N.ptr(window), N.ptr(tw), N.ptr(mag), b, t, n_fft, hop,
                                           N.stream_ptr()), "smt_stft_magnitude")
    return mag


@torch.no_grad()
def stft_inverse(magnitude, phase, n_fft, hop, win_length):
    """magnitude, phase [B, n_fft/2+1, frames] -> audio [B, 1, T'] (STFT.inverse, transforms.py:125-156)."""
    magnitude, phase = magnitude.contiguous().float(), phase.contiguous().float()
    b, bins, frames = magnitude.shape
    assert bins == n_fft // 2 + 1 and phase.shape == magnitude.shape
    window, tw = _get_tables(n_fft, win_length, magnitude.device)
    pad = (n_fft - hop) // 2
    out = torch.empty(b, (frames - 1) * hop + n_fft - 2 * pad, dtype=torch.float32, device=magnitude.device)
    with profiler.region("stft_inverse", nbytes=2 * magnitude.numel() * 4 + out.numel() * 4, bound="hbm"):
        N.check(N.lib().smt_stft_inverse(N.ptr(magnitude), N.ptr(phase), N.ptr(window), N.ptr(tw), N.ptr(out), b, n_fft, hop,
                                         frames, N.stream_ptr()), "smt_stft_inverse")
    return out.unsqueeze(1)


@torch.no_grad()
def log_mel(x, mel_basis, band, n_fft, hop, win_length):
    """x [B, T] -> log-mel [B, n_mels, frames] in one kernel (5.25 B/sample algorithmic)."""
    x = x.contiguous().float()
    b, t = x.shape
    _check_length("smt_melspec", t, n_fft, hop)
    window, tw = _get_tables(n_fft, win_length, x.device)
    frames = num_frames(t, n_fft, hop)
    n_mels = mel_basis.shape[0]
    mel = torch.empty(b, n_mels, frames, dtype=torch.float32, device=x.device)
    with profiler.region("melspec", nbytes=x.numel() * 4 + mel.numel() * 4, bound="hbm"):
        N.check(N.lib().smt_melspec(N.ptr(x), N.ptr(window), N.ptr(tw), N.ptr(mel_basis), N.ptr(band), N.ptr(mel), b, t,
                                    n_fft, hop, n_mels, N.stream_ptr()), "smt_melspec")
    return mel


def clip_frames(length, n_fft, hop):
    """Frames of a clip of `length` samples transformed alone: num_frames(), or 0 for a clip `log_mel` refuses (not longer than
    the reflect padding, or shorter than one frame after it).  The device computes the same in smt_melspec_ragged."""
    pad = (n_fft - hop) // 2
    return num_frames(length, n_fft, hop) if length > pad and length + 2 * pad >= n_fft else 0


@torch.no_grad()
def log_mel_ragged(x, lens, mel_basis, band, n_fft, hop, win_length, fill):
    """x [B, T] on the device, lens int64 [B] ON THE CPU (what collate produced) -> (mel [B, n_mels, F], frames int64 [B] on the
    CPU), F = max_b frames[b], in ONE launch.  Item b's first frames[b] = clip_frames(lens[b]) columns are log_mel(x[b:b+1,
    :lens[b]]) bit for bit -- the clip is reflected about its own end, not the batch's -- and the rest hold `fill`; x at or
    past lens[b] is never read.  Every check is made on the host copy of lens (ValueError), so the call does not wait for the
    device; an item too short for one frame is not an error here: it is all `fill` and has frames[b] = 0."""
    if not isinstance(lens, torch.Tensor) or lens.is_cuda or lens.is_floating_point() or lens.is_complex() \
            or lens.dtype == torch.bool:
        raise ValueError("log_mel_ragged: lens must be an integer tensor on the CPU (the lengths the collate produced)")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"log_mel_ragged: x must be [B, T] with B, T >= 1, got shape {tuple(x.shape)}")
    b, t = x.shape
    if lens.shape != (b,):
        raise ValueError(f"log_mel_ragged: lens must hold {b} lengths, got shape {tuple(lens.shape)}")
    host = [int(v) for v in lens.tolist()]
    for i, n in enumerate(host):
        if not 0 <= n <= t:
            raise ValueError(f"log_mel_ragged: item {i} has length {n}, outside [0, T={t}]")
    if n_fft not in (256, 512, 1024, 2048):
        raise ValueError(f"log_mel_ragged: n_fft={n_fft} unsupported (256, 512, 1024, 2048)")
    if not 1 <= hop <= n_fft:
        raise ValueError(f"log_mel_ragged: hop={hop} outside [1, n_fft={n_fft}]")
    x = x.contiguous().float()
    frames = [clip_frames(n, n_fft, hop) for n in host]
    frames_out = max(frames)
    window, tw = _get_tables(n_fft, win_length, x.device)
    n_mels = mel_basis.shape[0]
    mel = torch.empty(b, n_mels, frames_out, dtype=torch.float32, device=x.device)
    lens32 = torch.tensor(host, dtype=torch.int32).to(x.device, non_blocking=True)
    if frames_out > 0:
        with profiler.region("melspec_ragged", nbytes=sum(host) * 4 + mel.numel() * 4, bound="hbm"):
            N.check(N.lib().smt_melspec_ragged(N.ptr(x), N.ptr(lens32), N.ptr(window), N.ptr(tw), N.ptr(mel_basis), N.ptr(band),
                                               N.ptr(mel), b, t, n_fft, hop, n_mels, frames_out, float(fill), N.stream_ptr()),
                    "smt_melspec_ragged")
    return mel, torch.tensor(frames, dtype=torch.int64)


def _host_lens(what, lens, batch, frames):
    """The per-item frame counts of a ragged spectrogram batch as Python ints, checked on the host copy (no device wait)."""
    if not isinstance(lens, torch.Tensor) or lens.is_cuda or lens.is_floating_point() or lens.is_complex() \
            or lens.dtype == torch.bool:
        raise ValueError(f"{what}: lens must be an integer tensor on the CPU (frames per item)")
    if lens.shape != (batch,):
        raise ValueError(f"{what}: lens must hold {batch} lengths, got shape {tuple(lens.shape)}")
    host = [int(v) for v in lens.tolist()]
    for i, n in enumerate(host):
        if not 0 <= n <= frames:
            raise ValueError(f"{what}: item {i} has {n} frames, outside [0, frames={frames}]")
    return host


@torch.no_grad()
def mel_invert(mel, lens, mel_basis, band, n_iter=32, log_input=True):
    """mel [B, n_mels, F] (log-mel as MelSpectrogram makes it, or mel magnitudes with log_input=False), lens integer [B] ON THE
    CPU -> linear magnitudes [B, K, F], K = mel_basis.shape[1]: the non-negative least-squares inverse of `mel_basis @ |STFT|`
    by n_iter multiplicative updates in ONE launch (smt_mel_invert).  Columns at or past lens[b] are exact
    zeros and mel is not read there."""
    if mel.dim() != 3 or mel.shape[1] != mel_basis.shape[0]:
        raise ValueError(f"mel_invert: mel must be [B, n_mels={mel_basis.shape[0]}, frames], got shape {tuple(mel.shape)}")
    if n_iter < 0:
        raise ValueError(f"mel_invert: n_iter={n_iter}, need >= 0")
    b, n_mels, frames = mel.shape
    host = _host_lens("mel_invert", lens, b, frames)
    bins = mel_basis.shape[1]
    mel = mel.contiguous().float()
    mag = torch.empty(b, bins, frames, dtype=torch.float32, device=mel.device)
    if b == 0 or frames == 0:
        return mag
    lens32 = torch.tensor(host, dtype=torch.int32).to(mel.device, non_blocking=True)
    with profiler.region("mel_invert", nbytes=sum(host) * (n_mels + bins) * 4, bound="hbm"):
        N.check(N.lib().smt_mel_invert(N.ptr(mel), N.ptr(lens32), N.ptr(mel_basis), N.ptr(band), N.ptr(mag), b, 2 * (bins - 1),
                                       n_mels, frames, int(n_iter), int(bool(log_input)), N.stream_ptr()), "smt_mel_invert")
    return mag


def inverse_samples(frames, n_fft, hop):
    """Samples STFT.inverse makes of `frames` frames: (frames - 1) hop + n_fft - 2 pad, so num_frames() of it is `frames`."""
    return (frames - 1) * hop + n_fft - 2 * ((n_fft - hop) // 2) if frames > 0 else 0


def invertible(frames, n_fft, hop):
    """Whether an item of `frames` frames can be transformed back and forth: its samples must outnumber the reflect padding."""
    return inverse_samples(frames, n_fft, hop) > (n_fft - hop) // 2


@torch.no_grad()
def griffin_lim(mag, lens, n_fft, hop, win_length, n_iter=32, momentum=0.99, seed=0, phase0=None):
    """mag [B, n_fft/2+1, F] on the device, lens integer [B] ON THE CPU (frames per item) -> (wave [B, T_max] with T_max =
    inverse_samples(F), wave_lengths int64 [B] on the CPU): fast Griffin-Lim, all n_iter iterations queued by one call
    (smt_griffin_lim).  The start phases are phase0 [B, n_fft/2+1, F] or generated on the device from
    `seed`: an int (item b uses (seed + b) mod 2^31) or one int per item.  Item b's samples depend on its own lens[b] frames
    only -- not on its neighbours, its position or F -- and are exact zeros at or past wave_lengths[b]."""
    what = "griffin_lim"
    if n_fft not in (256, 512, 1024, 2048):
        raise ValueError(f"{what}: n_fft={n_fft} unsupported (256, 512, 1024, 2048)")
    if not 1 <= hop <= n_fft:
        raise ValueError(f"{what}: hop={hop} outside [1, n_fft={n_fft}]")
    if mag.dim() != 3 or mag.shape[1] != n_fft // 2 + 1:
        raise ValueError(f"{what}: mag must be [B, n_fft/2+1={n_fft // 2 + 1}, frames], got shape {tuple(mag.shape)}")
    if n_iter < 0:
        raise ValueError(f"{what}: n_iter={n_iter}, need >= 0")
    if not 0.0 <= momentum < 1.0:
        raise ValueError(f"{what}: momentum={momentum} outside [0, 1)")
    b, bins, frames = mag.shape
    host = _host_lens(what, lens, b, frames)
    for i, n in enumerate(host):
        if n > 0 and not invertible(n, n_fft, hop):
            raise ValueError(f"{what}: item {i} has {n} frames = {inverse_samples(n, n_fft, hop)} samples, not more than the "
                             f"reflect padding {(n_fft - hop) // 2}: too short to transform")
    seeds = None
    if phase0 is not None:
        if not (isinstance(seed, int) and seed == 0):
            raise ValueError(f"{what}: give either seed or phase0, not both")
        if phase0.shape != mag.shape:
            raise ValueError(f"{what}: phase0 must have mag's shape {tuple(mag.shape)}, got {tuple(phase0.shape)}")
        phase0 = phase0.contiguous().float()
    else:
        per_item = [(seed + i) % (1 << 31) for i in range(b)] if isinstance(seed, int) else [int(s) for s in seed]
        if len(per_item) != b or any(not 0 <= s < (1 << 31) for s in per_item):
            raise ValueError(f"{what}: seed must be an int or {b} ints in [0, 2^31)")
        seeds = torch.tensor(per_item, dtype=torch.int32).to(mag.device, non_blocking=True)
    mag = mag.contiguous().float()
    t_max = inverse_samples(frames, n_fft, hop)
    wave = torch.empty(b, t_max, dtype=torch.float32, device=mag.device)
    lengths = torch.tensor([inverse_samples(n, n_fft, hop) for n in host], dtype=torch.int64)
    if b == 0 or frames == 0:
        return wave, lengths
    window, tw = _get_tables(n_fft, win_length, mag.device)
    lens32 = torch.tensor(host, dtype=torch.int32).to(mag.device, non_blocking=True)
    ws_bytes = int(N.lib().smt_griffin_lim_workspace_bytes(b, n_fft, hop, frames))
    ws = N.workspace.get(ws_bytes, mag.device)
    # per iteration: x written and read as frames (n_fft / hop times, mostly from L2), t read and written, S read, rows written
    # and read
    per_iter = sum(host) * (bins * (8 + 8 + 4) + 2 * n_fft * 4) + 2 * int(lengths.sum()) * 4
    with profiler.region("griffin_lim", nbytes=2 * mag.numel() * 4 + n_iter * per_iter + wave.numel() * 4, bound="hbm"):
        N.check(N.lib().smt_griffin_lim(N.ptr(mag), N.ptr(lens32), N.ptr(phase0), N.ptr(seeds), N.ptr(window), N.ptr(tw),
                                        N.ptr(wave), b, n_fft, hop, frames, int(n_iter), float(momentum), N.ptr(ws), ws.numel(),
                                        N.stream_ptr()), "smt_griffin_lim")
    return wave, lengths


class _StftLoss(torch.autograd.Function):
    """mean_b sqrt(sum ((|Y|-|Yh|) m)^2) [+ the same on clamped log magnitudes] for ONE resolution."""

    @staticmethod
    def forward(ctx, y, yh, lens, n_fft, hop, win_length, use_log):
        y, yh = y.contiguous().float(), yh.contiguous().float()
        b, t = y.shape
        _check_length("smt_stft_loss_fwd", t, n_fft, hop)
        window, tw = _get_tables(n_fft, win_length, y.device)
        frames = num_frames(t, n_fft, hop)
        part = torch.empty(b, frames, 2, dtype=torch.float32, device=y.device)
        lens32 = None if lens is None else lens.to(torch.int32)
        with profiler.region("stft_loss_fwd", nbytes=2 * y.numel() * 4, bound="hbm"):
            N.check(N.lib().smt_stft_loss_fwd(N.ptr(y), N.ptr(yh), N.ptr(lens32), N.ptr(window), N.ptr(tw),
                                              N.ptr(part), b, t, n_fft, hop, N.stream_ptr()), "smt_stft_loss_fwd")
        sums = part.sum(dim=1)                       # [B, 2]; fixed-order reduction of tiny tensors
        root = sums.sqrt()
        loss = root[:, 0].mean() + (root[:, 1].mean() if use_log else 0.0)
        ctx.save_for_backward(y, yh, lens32 if lens32 is not None else torch.empty(0), root)
        ctx.cfg = (n_fft, hop, win_length, use_log, lens is not None)
        return loss

    @staticmethod
    def backward(ctx, g):
        y, yh, lens32, root = ctx.saved_tensors
        n_fft, hop, win_length, use_log, has_lens = ctx.cfg
        lens32 = lens32 if has_lens else None
        b, t = y.shape
        window, tw = _get_tables(n_fft, win_length, y.device)
        coef = (g / (2.0 * b)) / root.clamp(min=1e-30)          # d sqrt(S)/dS = 1/(2 sqrt(S)), mean over B
        if not use_log:
            coef = coef * _const([1.0, 0.0], coef.device)
        coef = coef.contiguous().float()
        dyh = torch.empty_like(yh)
        ws_bytes = N.lib().smt_stft_loss_bwd_workspace_bytes(b, t, n_fft, hop)
        ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=y.device)     # per-frame gradient rows
        with profiler.region("stft_loss_bwd", nbytes=3 * y.numel() * 4, bound="hbm"):
            N.check(N.lib().smt_stft_loss_bwd(N.ptr(y), N.ptr(yh), N.ptr(lens32), N.ptr(window), N.ptr(tw),
                                              N.ptr(coef), N.ptr(dyh), b, t, n_fft, hop, N.ptr(ws), ws.numel(),
                                              N.stream_ptr()), "smt_stft_loss_bwd")
        return None, dyh, None, None, None, None, None


def stft_loss(y, yh, lens, n_fft, hop, win_length, use_log):
    return _StftLoss.apply(y, yh, lens, n_fft, hop, win_length, use_log)


class _ReconLoss(torch.autograd.Function):
    """l1 * mean|d| + l2 * mean d^2 + linf * sum_j mean_b topk_j(d^2) on masked [B, T] signals (losses.py:73-80)."""

    @staticmethod
    def forward(ctx, y, yh, lens, l1, l2, linf, topk):
        y, yh = y.contiguous().float(), yh.contiguous().float()
        b, t = y.shape
        lens32 = None if lens is None else lens.to(torch.int32)
        stats = torch.empty(b, 8, dtype=torch.float32, device=y.device)
        with profiler.region("recon_loss_fwd", nbytes=5 * 2 * y.numel() * 4, bound="hbm"):
            N.check(N.lib().smt_recon_loss_fwd(N.ptr(y), N.ptr(yh), N.ptr(lens32), b, t, int(topk), N.ptr(stats),
                                               N.stream_ptr()), "smt_recon_loss_fwd")
        sums = stats[:, :3].sum(dim=0)                 # fixed-order reduction over the batch
        loss = l2 * sums[0] / (b * t) + linf * sums[2] / b
        if l1:
            loss = loss + l1 * sums[1] / (b * t)
        ctx.save_for_backward(y, yh, lens32 if lens32 is not None else torch.empty(0), stats)
        ctx.cfg = (l1, l2, linf, int(topk), lens is not None)
        return loss

    @staticmethod
    def backward(ctx, g):
        y, yh, lens32, stats = ctx.saved_tensors
        l1, l2, linf, topk, has_lens = ctx.cfg
        lens32 = lens32 if has_lens else None
        b, t = y.shape
        scale = _const([l1 / (b * t), 2.0 * l2 / (b * t), 2.0 * linf / b], y.device)
        coef = (g.reshape(1).float() * scale).contiguous()
        dyh = torch.empty_like(yh)
        with profiler.region("recon_loss_bwd", nbytes=3 * y.numel() * 4, bound="hbm"):
            N.check(N.lib().smt_recon_loss_bwd(N.ptr(y), N.ptr(yh), N.ptr(lens32), N.ptr(stats), N.ptr(coef), b, t, topk,
                                               N.ptr(dyh), N.stream_ptr()), "smt_recon_loss_bwd")
        return None, dyh, None, None, None, None, None


def recon_loss(y, yh, lens, l1, l2, linf, topk):
    return _ReconLoss.apply(y, yh, lens, float(l1), float(l2), float(linf), int(topk))
