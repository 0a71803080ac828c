"""Timing of the device vocoder at the GlowTTS bench's output sizes: B = 32 spectrograms of 607 frames
(its mean) and B = 1 of 848, n_fft 1024, hop 256, 80 mels to 8 kHz, 32 NNLS updates and 32 iterations of fast Griffin-Lim.

  mel_invert    spectral.mel_invert: one launch (smt_mel_invert);
  griffin_lim   spectral.griffin_lim: 2 + 2 n_iter launches queued by one call (smt_griffin_lim); the time per iteration is
                (t(n_iter) - t(0)) / n_iter, and the device time of the step and the gather kernels apart comes from one
                call under the torch profiler;
  pinv_clamp    the unfused inversion on the same device: clamp(pinv(B) @ exp(mel), 0) with torch (pinv computed once, outside
                the timed window), and its NNLS residual beside mel_invert's;
  torch_loop    the unfused Griffin-Lim on the same device: torch.istft / torch.stft (center=True, reflect) in a Python loop
                with the same update.  It frames the signal as torch does, not as STFT.forward / inverse do, so it is a cost
                comparison of the same amount of work, not a bit-for-bit alternative.

Each figure is the time of one whole call from a host clock around `iters` calls that end in a device synchronise; the
variants alternate over `rounds` rounds; minimum, median and maximum round are printed.  Bytes moved are the algorithmic ones
of spectral.griffin_lim's profiler region (per iteration: t read and written, S read, the rows written and read, x written and
read once).  Appends to --out (profiles/griffin_lim_micro.txt)."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-masters-thesis_amd"))
from datasets.transforms import MelSpectrogram  # noqa: E402
from smt_amd import spectral  # noqa: E402

N_FFT, HOP, WIN, N_MELS = 1024, 256, 1024, 80


def wall_us(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def kernel_times(fn):
    """{kernel name: (launches, total device us)} of one call."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            n, us = out.get(e.name, (0, 0.0))
            out[e.name] = (n + 1, us + e.device_time_total)
    return out


def fmt(v):
    return f"min {min(v):10.1f}  median {statistics.median(v):10.1f}  max {max(v):10.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="32x607,1x848", help="batch x frames, comma separated")
    ap.add_argument("--n_iter", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "griffin_lim_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_griffin_lim measures on the GPU; none is visible")
    front = MelSpectrogram(n_fft=N_FFT, hop_length=HOP, win_length=WIN, n_mels=N_MELS, sample_rate=22050, f_min=0.0, f_max=8000.0).cuda()
    basis = front.mel_basis
    pinv = torch.linalg.pinv(basis.double()).float()
    window = torch.hann_window(WIN, periodic=True, device="cuda")
    alpha = 0.99 / 1.99
    lines = []
    for shape in args.shapes.split(","):
        b, frames = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(args.seed)
        x = (torch.rand(b, frames * HOP, device="cuda", generator=g) - 0.5) * 0.8
        mel = front(x)
        assert mel.shape == (b, N_MELS, frames)
        lens = torch.full((b,), frames, dtype=torch.int64)
        mag = spectral.mel_invert(mel, lens, basis, front.band, n_iter=args.n_iter)

        def mel_invert():
            return spectral.mel_invert(mel, lens, basis, front.band, n_iter=args.n_iter)

        def pinv_clamp():
            return torch.clamp(torch.matmul(pinv, torch.exp(mel)), min=0.0)

        def griffin_lim(n_iter=args.n_iter):
            return spectral.griffin_lim(mag, lens, N_FFT, HOP, WIN, n_iter=n_iter, momentum=0.99, seed=args.seed)[0]

        def griffin_lim_0():
            return griffin_lim(0)

        phase0 = torch.rand(mag.shape, device="cuda", generator=g) * (2 * math.pi)

        def torch_loop():
            c = torch.polar(mag, phase0)
            t = torch.zeros_like(c)
            for _ in range(args.n_iter):
                wave = torch.istft(c, N_FFT, HOP, WIN, window, center=True, length=frames * HOP)
                r = torch.stft(wave, N_FFT, HOP, WIN, window, center=True, pad_mode="reflect", return_complex=True)[..., :frames]
                a = r - alpha * t
                t = r
                c = mag * a / (a.abs() + 1e-16)
            return torch.istft(c, N_FFT, HOP, WIN, window, center=True, length=frames * HOP)

        m = torch.exp(mel.double())
        res = {k: float((torch.matmul(basis.double(), fn().double()) - m).norm() / m.norm()) for k, fn in
               (("mel_invert", mel_invert), ("pinv_clamp", pinv_clamp))}
        variants = {"mel_invert": mel_invert, "pinv_clamp": pinv_clamp, "griffin_lim": griffin_lim, "griffin_lim_0": griffin_lim_0,
                    "torch_loop": torch_loop}
        for fn in variants.values():
            for _ in range(2):
                fn()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(wall_us(fn, args.iters))
        kern = kernel_times(griffin_lim)
        bins, t_max = N_FFT // 2 + 1, frames * HOP
        per_iter_bytes = b * frames * (bins * (8 + 8 + 4) + 2 * N_FFT * 4) + 2 * b * t_max * 4
        med = {k: statistics.median(v) for k, v in times.items()}
        per_iter = (med["griffin_lim"] - med["griffin_lim_0"]) / args.n_iter
        lines += [f"# bench_griffin_lim: B = {b} x {frames} frames ({t_max} samples each), n_fft {N_FFT} hop {HOP} {N_MELS} mels, "
                  f"n_iter {args.n_iter}, {args.rounds} rounds x {args.iters} calls, seed {args.seed}, {torch.cuda.get_device_name(0)}"]
        for k in variants:
            lines.append(f"{k:14s} us/call  {fmt(times[k])}")
        lines.append(f"griffin_lim per iteration (medians, (t({args.n_iter}) - t(0)) / {args.n_iter}): {per_iter:.1f} us; "
                     f"{per_iter_bytes / 1e6:.1f} MB algorithmic per iteration = {per_iter_bytes / max(per_iter, 1e-9) * 1e-3:.0f} GB/s")
        for name, (n, us) in sorted(kern.items(), key=lambda kv: -kv[1][1]):
            if "smt" in name:
                lines.append(f"  device time of one call: {name[:60]:60s} launches {n:4d}  total {us:10.1f} us  each {us / n:8.1f} us")
        lines.append(f"torch_loop / griffin_lim (medians): {med['torch_loop'] / med['griffin_lim']:.2f};  pinv_clamp / mel_invert: "
                     f"{med['pinv_clamp'] / med['mel_invert']:.2f};  NNLS residual ||B S - m|| / ||m||: mel_invert {res['mel_invert']:.3g}, "
                     f"pinv_clamp {res['pinv_clamp']:.3g}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
