"""Shared by tests/test_griffin_lim_cpu.py and tests/test_griffin_lim_gpu.py: float64 restatements of the mel inversion and of
fast Griffin-Lim (smt_mel_invert / smt_griffin_lim), the fp32 host restatements that give E32, the case
tables and the bounds.  Everything here is written from the formulas, with torch.fft and dense matrices, not from the kernels:

  mel inversion   m = exp(mel) (log_input) or mel; c = B 1; num = B^T m; S = num / (B^T c) where that is > 0, else 0 for good;
                  n_iter times: r = B S, S <- S num / max(B^T r, 1e-30).  Columns at or past lens[b] are zero.
  Griffin-Lim     alpha = momentum / (1 + momentum); c = S e^{i phi0}, t = 0; n_iter times: x = istft(c), R = stft(x),
                  a = R - alpha t, t = R, c = S a / (|a| + 1e-16); wave = istft(c).  istft is spectral_ref_helpers.stft_inverse64
                  (test_griffin_lim_cpu.py pins the n_iter = 0 case to it), stft is spectral_ref_helpers.spectrum64 of the
                  item's own samples.  Every item is computed ALONE: that is the batch-independence contract.
  phases          key = fmix32(fmix32(seed) + f 0x9E3779B1), bits = fmix32(key + k 0x85EBCA77), u = ((bits >> 9) + 0.5) 2^-23,
                  phi0 = fp32(2 pi) * u in fp32.
  sc              ||  |stft(wave)| - S || / || S ||  in float64 from the waveform returned (spectral convergence).

Tolerances are the project's E32 rule (spectral_ref_helpers): the device gets max(4 E32, floor), E32 being the error of the
fp32 restatement below against the float64 one on the same inputs; the floors are bound_magnitude (mel inversion) and
bound_inverse (waveforms).  For the two scalar criteria (sc, and the round trip's mean |log-mel error|) the floor is 4 x the
largest E32 over the case table, computed by sc_floor() / roundtrip_floor() from the two HOST restatements alone and written
down here; test_griffin_lim_cpu.py recomputes them.  Nothing in this file was fitted to a device result.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import spectral_ref_helpers as H

# (n_fft, hop, win): the mel front end, the smallest transform, n_fft - hop odd, the two narrow model resolutions
CONFIGS = [(1024, 256, 1024), (256, 64, 256), (512, 75, 300), (512, 50, 240), (2048, 240, 1200)]
MOMENTUM = 0.99
N_ITER_LONG = 32
# 4 x the largest E32 of sc / of the round trip's error over the tables below (sc_floor(), roundtrip_floor()), measured with the
# two host restatements: 4 x 1.33e-5 (relative) and 4 x 7.7e-6 (absolute, in log-mel units)
SC_FLOOR = 5.3e-5
ROUNDTRIP_FLOOR = 3.1e-5


def pad_of(cfg):
    return (cfg[0] - cfg[1]) // 2


def samples_of(cfg, frames):
    return (frames - 1) * cfg[1] + cfg[0] - 2 * pad_of(cfg) if frames > 0 else 0


def f_min(cfg):
    """Fewest frames an item can be transformed with: its samples must outnumber the reflect padding."""
    f = 1
    while samples_of(cfg, f) <= pad_of(cfg):
        f += 1
    return f


def frame_counts(cfg):
    """F_min, 3, 4, 5, 9 (those an item can have): below, at and above the four frames of a workgroup."""
    return sorted({f for f in (f_min(cfg), 3, 4, 5, 9) if f >= f_min(cfg)})


def ragged_lens(cfg):
    """[9, 4, 0, 5, F_min] with the counts below F_min raised to it."""
    m = f_min(cfg)
    return [9, max(4, m), 0, max(5, m), m]


# ------------------------------------------------------------------------------------------------------- phases

def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def uniform_from_bits(bits):
    """u = ((bits >> 9) + 0.5) 2^-23 computed in fp32, as the device does."""
    return ((np.asarray(bits, dtype=np.uint64) >> 9).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def hash_phases(seed, frames, bins):
    """phi0 fp32 [bins, frames] of one item."""
    f = np.arange(frames, dtype=np.uint64)[None, :]
    k = np.arange(bins, dtype=np.uint64)[:, None]
    key = fmix32((fmix32(seed) + f * 0x9E3779B1) & 0xFFFFFFFF)
    bits = fmix32((key + k * 0x85EBCA77) & 0xFFFFFFFF)
    phi = np.float32(2.0 * math.pi) * uniform_from_bits(bits)
    assert phi.dtype == np.float32
    return torch.from_numpy(phi)


# ------------------------------------------------------------------------------------------------ mel inversion

def mel_invert_ref(mel, lens, basis, n_iter, log_input, dtype=torch.float64):
    """mel [B, n_mels, F] fp32, basis fp32 [n_mels, K] -> [B, K, F] in `dtype` (float64: the reference; float32: E32)."""
    B = basis.to(dtype)
    out = torch.zeros(mel.shape[0], B.shape[1], mel.shape[2], dtype=dtype)
    c = B.sum(1)
    d0 = B.t() @ c
    covered = d0 > 0
    for b, n in enumerate(lens):
        if n == 0:
            continue
        m = mel[b, :, :n].to(dtype)
        m = torch.exp(m) if log_input else m
        num = B.t() @ m
        S = torch.where(covered[:, None], num / torch.where(covered, d0, torch.ones_like(d0))[:, None], torch.zeros_like(num))
        for _ in range(n_iter):
            den = B.t() @ (B @ S)
            S = torch.where(covered[:, None], S * num / den.clamp(min=1e-30), torch.zeros_like(S))
        out[b, :, :n] = S
    return out


def nnls_residual(S, mel, basis, log_input):
    """|| B S - m || / || m || in float64, one item."""
    m = torch.exp(mel.double()) if log_input else mel.double()
    return float((basis.double() @ S.double() - m).norm() / m.norm())


# the three front ends of the issue: 80 filters to 8 kHz at 22,050 Hz; at n_fft 256 four filters are empty, and every bin above
# 8 kHz is uncovered at all three
MEL_FRONT_ENDS = [((1024, 256, 1024), 80, 8000.0), ((512, 50, 240), 80, 8000.0), ((256, 64, 256), 80, 8000.0)]
MEL_FRAMES = [1, 3, 4, 5, 65, 130]
MEL_ITERS = [0, 1, 8, 32]


def mel_lens(frames):
    """`frames`, a length inside a run of eight, none."""
    return [frames, frames // 2, 0]


@functools.lru_cache(maxsize=None)
def mel_case(front, frames, log_input):
    """(mel fp32 [3, n_mels, frames] with NaN past lens, lens, basis fp32): mels of the magnitudes of a noisy signal."""
    cfg, n_mels, f_max = MEL_FRONT_ENDS[front]
    basis = H.mel_module(cfg, n_mels, f_max).mel_basis.cpu()
    lens = mel_lens(frames)
    g = torch.Generator().manual_seed(1000 * front + frames)
    mag = torch.rand(len(lens), cfg[0] // 2 + 1, frames, generator=g, dtype=torch.float64) ** 2 * 3
    m = torch.matmul(basis.double(), mag)
    mel = (torch.log(m.clamp(min=H.CLAMP)) if log_input else m).float()
    for b, n in enumerate(lens):
        mel[b, :, n:] = float("nan")
    return mel, lens, basis


@functools.lru_cache(maxsize=None)
def mel_reference(front, frames, log_input, n_iter):
    """(ref64, E32)."""
    mel, lens, basis = mel_case(front, frames, log_input)
    ref = mel_invert_ref(mel, lens, basis, n_iter, log_input)
    return ref, H.max_abs(mel_invert_ref(mel, lens, basis, n_iter, log_input, torch.float32), ref)


# -------------------------------------------------------------------------------------------------- Griffin-Lim

def istft(c, cfg, dtype=torch.float64):
    """c complex [K, F] -> [T]: irfft per frame (imaginary parts of bins 0 and N/2 dropped), window, overlap-add, division by
    the window sum-square above float32 tiny, pad trimmed."""
    n_fft, hop, win = cfg
    pad, frames = pad_of(cfg), c.shape[1]
    w = H.window64(n_fft, win).to(dtype)
    spec = c.t().clone()
    spec[:, 0] = spec[:, 0].real + 0j
    spec[:, -1] = spec[:, -1].real + 0j
    rows = torch.fft.irfft(spec, n=n_fft, dim=-1) * w
    total = n_fft + hop * (frames - 1)
    out = torch.zeros(total, dtype=dtype)
    wss = torch.zeros(total, dtype=dtype)
    for f in range(frames):
        out[f * hop:f * hop + n_fft] += rows[f]
        wss[f * hop:f * hop + n_fft] += w * w
    nz = wss > H.FLOAT32_TINY
    out[nz] /= wss[nz]
    return out[pad:total - pad]


def stft(x, cfg, dtype=torch.float64):
    """x [T] -> complex [K, F], reflected about its own ends."""
    if dtype == torch.float64:
        return H.spectrum64(x[None], cfg)[0].t()
    n_fft, hop, win = cfg
    pad = pad_of(cfg)
    xp = F.pad(x.to(dtype)[None, None], (pad, pad), mode="reflect")[0, 0]
    return torch.fft.rfft(xp.unfold(-1, n_fft, hop) * H.window64(n_fft, win).to(dtype), dim=-1).t()


def griffin_lim_ref(S, phi, cfg, n_iter, momentum, dtype=torch.float64):
    """One item: S, phi fp32 [K, F] -> wave [T] in `dtype`."""
    alpha = momentum / (1.0 + momentum)
    S = S.to(dtype)
    c = torch.polar(S, phi.to(dtype))
    t = torch.zeros_like(c)
    for _ in range(n_iter):
        R = stft(istft(c, cfg, dtype), cfg, dtype)
        a = R - alpha * t
        t = R
        c = S * a / (a.abs() + 1e-16)
    return istft(c, cfg, dtype)


def spectral_convergence(wave, S, cfg):
    S = S.double()
    return float((stft(wave.double(), cfg).abs() - S).norm() / S.norm())


@functools.lru_cache(maxsize=None)
def item(cfg, frames, seed):
    """(S fp32 [K, F], phi fp32 [K, F]): S is the magnitude of a seeded sum of sinusoids plus noise (no frame silent)."""
    t = samples_of(cfg, frames)
    g = torch.Generator().manual_seed(7919 * seed + 31 * frames + cfg[0] + cfg[1])
    n = torch.arange(t, dtype=torch.float64)
    x = torch.zeros(t, dtype=torch.float64)
    for _ in range(5):
        freq = 0.01 + 0.4 * float(torch.rand(1, generator=g))
        x += (0.1 + 0.2 * float(torch.rand(1, generator=g))) * torch.sin(2 * math.pi * freq * n + 6.28 * float(torch.rand(1, generator=g)))
    x += 0.05 * torch.randn(t, generator=g, dtype=torch.float64)
    S = stft(x, cfg).abs().float()
    phi = ((torch.rand(S.shape, generator=g) * 2 - 1) * (math.pi * (1 - 1e-6))).float()
    return S.contiguous(), phi.contiguous()


def batch(cfg, lens, frames=None, seed0=0, poison=float("nan")):
    """(mag, phase0) fp32 [B, K, frames]: item b is item(cfg, lens[b], seed0 + b), `poison` past its frames."""
    frames = max(lens) if frames is None else frames
    mag = torch.full((len(lens), cfg[0] // 2 + 1, frames), poison)
    phase = torch.full_like(mag, poison)
    for b, n in enumerate(lens):
        if n:
            mag[b, :, :n], phase[b, :, :n] = item(cfg, n, seed0 + b)
    return mag, phase


@functools.lru_cache(maxsize=None)
def item_reference(cfg, frames, seed, n_iter, momentum=MOMENTUM):
    """(wave64 [T], E32) of item(cfg, frames, seed) with its explicit phases."""
    S, phi = item(cfg, frames, seed)
    ref = griffin_lim_ref(S, phi, cfg, n_iter, momentum)
    return ref, H.max_abs(griffin_lim_ref(S, phi, cfg, n_iter, momentum, torch.float32), ref)


@functools.lru_cache(maxsize=None)
def sc_reference(cfg, frames, seed):
    """(sc64, E32_sc) after N_ITER_LONG iterations."""
    S, phi = item(cfg, frames, seed)
    sc64 = spectral_convergence(griffin_lim_ref(S, phi, cfg, N_ITER_LONG, MOMENTUM), S, cfg)
    sc32 = spectral_convergence(griffin_lim_ref(S, phi, cfg, N_ITER_LONG, MOMENTUM, torch.float32), S, cfg)
    return sc64, abs(sc32 - sc64) / sc64


def calls(cfg):
    """[(lens, seed0)] -- the calls the device tests make per configuration: the ragged batch, and every frame count alone as
    a batch of two full items.  Item b of a call is item(cfg, lens[b], seed0 + b)."""
    return [(ragged_lens(cfg), 0)] + [([n, n], 100) for n in frame_counts(cfg)]


def sc_table():
    """[(cfg, frames, seed)]: every live item of every call."""
    return [(cfg, n, seed0 + b) for cfg in CONFIGS for lens, seed0 in calls(cfg) for b, n in enumerate(lens) if n]


def sc_floor():
    return 4 * max(sc_reference(*case)[1] for case in sc_table())


def bound_sc(e32):
    return max(4 * e32, SC_FLOOR)


# --------------------------------------------------------------------------------------------------- round trip

ROUNDTRIP_FRONT = ((1024, 256, 1024), 80, 8000.0)
ROUNDTRIP_SEEDS = [0, 1, 2]
ROUNDTRIP_SAMPLES = 40 * 256
ROUNDTRIP_ITERS = 32


def roundtrip_signal(seed):
    g = torch.Generator().manual_seed(4242 + seed)
    n = torch.arange(ROUNDTRIP_SAMPLES, dtype=torch.float64)
    x = torch.zeros_like(n)
    for _ in range(6):
        freq = 0.005 + 0.2 * float(torch.rand(1, generator=g))
        x += 0.1 * torch.sin(2 * math.pi * freq * n + 6.28 * float(torch.rand(1, generator=g)))
    x += 0.02 * torch.randn(n.shape, generator=g, dtype=torch.float64)
    return x.float()[None]


@functools.lru_cache(maxsize=None)
def roundtrip_reference(seed, dtype=torch.float64):
    """Mean |log-mel(GL(invert(log-mel(x)))) - log-mel(x)| of the host pipeline in `dtype`, with the hash phases of `seed`."""
    cfg, n_mels, f_max = ROUNDTRIP_FRONT
    basis = H.mel_module(cfg, n_mels, f_max).mel_basis.cpu()
    x = roundtrip_signal(seed)

    def log_mel(sig):
        return torch.log((basis.to(dtype) @ stft(sig, cfg, dtype).abs()).clamp(min=H.CLAMP))

    mel = log_mel(x[0]).float()                         # what MelSpectrogram hands over: fp32
    frames = mel.shape[1]
    S = mel_invert_ref(mel[None], [frames], basis, ROUNDTRIP_ITERS, True, dtype)[0]
    phi = hash_phases(seed, frames, S.shape[0])
    wave = griffin_lim_ref(S.float(), phi, cfg, ROUNDTRIP_ITERS, MOMENTUM, dtype)
    return float((log_mel(wave.clamp(-1, 1)) - mel.to(dtype)).abs().mean())


def roundtrip_e32(seed):
    r64 = roundtrip_reference(seed)
    return abs(roundtrip_reference(seed, torch.float32) - r64)


def roundtrip_floor():
    return 4 * max(roundtrip_e32(s) for s in ROUNDTRIP_SEEDS)


def bound_roundtrip(e32):
    return max(4 * e32, ROUNDTRIP_FLOOR)
