"""Timing of the ragged log-mel front end at the `ragged` bench shape: B = 32 clips with lengths ~ U[24,064, 222,720] cut to a
multiple of 512, zero-padded to the longest; n_fft 1024, hop 256, 80 mels.  Three ways to get the batch's log-mels:

  ragged    spectral.log_mel_ragged: ONE launch (smt_melspec_ragged), every clip reflected about its own end;
  per_clip  the correct alternative without it: B calls of spectral.log_mel on the truncated clips, padded with log(1e-7) and
            stacked;
  padded    spectral.log_mel on the zero-padded batch: one launch, WRONG in the last frames of every shorter clip -- the cost
            floor, not an alternative.

Each figure is the time of one whole call (host side included: the per-clip form is 3 B launches issued from Python) from a
host clock around `iters` calls that end in a device synchronise; the variants alternate over `rounds` rounds, and the
minimum, median and maximum round are printed.  Before timing, `ragged` is compared bit for bit with `per_clip`.  Appends to
--out (profiles/mel_ragged_micro.txt)."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-masters-thesis_amd"))
from datasets.transforms import BatchLogMel  # noqa: E402
from smt_amd import spectral  # noqa: E402

N_FFT, HOP, WIN = 1024, 256, 1024


def wall_us(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "mel_ragged_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_mel_ragged measures on the GPU; none is visible")
    rng = np.random.default_rng(args.seed)
    lens = [int(v) // 512 * 512 for v in rng.integers(24064, 222721, args.batch)]
    t = max(lens)
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    x = torch.rand(args.batch, t, device="cuda", generator=g) - 0.5
    for b, n in enumerate(lens):
        x[b, n:] = 0.0
    lens_cpu = torch.tensor(lens, dtype=torch.int64)
    mel = BatchLogMel(n_fft=N_FFT, hop_length=HOP, win_length=WIN, n_mels=80, sample_rate=22050, f_min=0.0, f_max=8000.0).cuda()
    fill = BatchLogMel.FILL
    frames = [spectral.clip_frames(n, N_FFT, HOP) for n in lens]

    def ragged():
        return spectral.log_mel_ragged(x, lens_cpu, mel.mel_basis, mel.band, N_FFT, HOP, WIN, fill)[0]

    def per_clip():
        parts = [spectral.log_mel(x[b:b + 1, :n], mel.mel_basis, mel.band, N_FFT, HOP, WIN)[0] for b, n in enumerate(lens)]
        return torch.stack([F.pad(p, (0, max(frames) - p.shape[-1]), value=fill) for p in parts])

    def padded():
        return spectral.log_mel(x, mel.mel_basis, mel.band, N_FFT, HOP, WIN)

    a, c, p = ragged(), per_clip(), padded()
    same = torch.equal(a.view(torch.int32), c.view(torch.int32))
    wrong = int(((p != a) & (torch.arange(p.shape[-1], device="cuda")[None, None, :] < torch.tensor(frames, device="cuda")[:, None, None])).any(1).sum())
    variants = {"ragged": ragged, "per_clip": per_clip, "padded": padded}
    for fn in variants.values():               # warm every shape of the timed window
        for _ in range(5):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(wall_us(fn, args.iters))
    samples, total_frames = sum(lens), sum(frames)
    nbytes = samples * 4 + args.batch * 80 * max(frames) * 4
    lines = [f"# bench_mel_ragged: batch {args.batch}, lengths {min(lens)}..{max(lens)} (sum {samples}), frames {total_frames} valid of "
             f"{args.batch * max(frames)} written, seed {args.seed}, {args.rounds} rounds x {args.iters} calls, {torch.cuda.get_device_name(0)}",
             f"# ragged bit-equal to per_clip: {same}; valid frames where the padded-batch transform differs: {wrong}"]
    for k in variants:
        v = times[k]
        extra = f"  {nbytes / statistics.median(v) * 1e-3:7.0f} GB/s of input + output bytes" if k == "ragged" else ""
        lines.append(f"{k:9s} us/call  min {min(v):9.1f}  median {statistics.median(v):9.1f}  max {max(v):9.1f}{extra}")
    lines.append(f"per_clip / ragged (medians): {statistics.median(times['per_clip']) / statistics.median(times['ragged']):.2f};  "
                 f"ragged / padded (medians): {statistics.median(times['ragged']) / statistics.median(times['padded']):.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a", encoding="utf-8") as f:
        f.write(text)
    assert same, "log_mel_ragged differs from the per-clip log_mel"
    assert math.isfinite(sum(sum(v) for v in times.values()))


if __name__ == "__main__":
    main()
