"""Micro-benchmark of the VQTTS code head (HIP events on the launch stream, 5 warm-up calls and a timed window of about
0.4 s -- at least 20 calls -- per line, everything in ONE process).

C = 128 channels, V = 512 bins, a tenth of the rows unscored, at two sizes:
  * N = 581,632 rows (B = 32 items of 18,176 frames: the 145,408-sample clip at stride 8, the largest shape the head is sized for);
  * N = 36,352 rows (two such items).
The fused ``vqtts.code_head`` (forward, and forward + backward to h, weight and bias) beside the unfused path on the same
device, ``F.linear`` followed by ``smt_amd.lm.cross_entropy``, which writes the [N, V] logits and their gradient.  It
prints ms per call, the achieved rate against the algorithmic 2 N C V FLOP of one product (forward 1, forward + backward
3 products; the fused path executes 3 bf16 MFMAs per product and recomputes the logits twice in the backward), and the
peak device memory each path allocates above its inputs (its gradients included).

Sampling lines (``--lines sample`` for these alone): the fused draw ``vqtts.code_head_sample`` at N = 18,176 (32 items of 568
frames, the configuration's shape) and N = 581,632, without truncation (one sweep) and with min_p = 0.05 (two sweeps), beside
(a) the argmax form ``vqtts.code_head_predict`` and (b) the unfused draw on the same device: ``F.linear``, Gumbel noise from
torch's generator, ``argmax``, which writes the [N, V] logits and the noise.  The four are timed in ALTERNATING windows (five
rounds of about 0.2 s per line, after warming every line up); a line reports the median over the rounds and the spread
(min .. max), and the peak memory above the inputs.

    python tools/bench_code_head.py [--out FILE] [--lines all|head|sample]
"""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-masters-thesis_amd"))
sys.path.insert(0, REPO)
from smt_amd import lm, vqtts  # noqa: E402

C, V = 128, 512


def _window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms


def timeit(fn, warmup=5, window_ms=400.0):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    iters = max(20, int(window_ms / _window(fn, 5)))          # a window of ~0.4 s whatever the call takes
    return _window(fn, iters)


def peak(fn, reset):
    fn()
    torch.cuda.synchronize()
    reset()                                   # the gradients of the call above are not part of the next call's base
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def alternate(fns, rounds=5, window_ms=200.0, warmup=5):
    """{name: ms per call, one per round}: every line warmed up first, then `rounds` rounds in which the lines take turns."""
    iters = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        iters[name] = max(10, int(window_ms / _window(fn, 5)))
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(_window(fn, iters[name]))
    return times


def sample_lines(emit, gen, w, b, split):
    w, b = w.detach(), b.detach()
    for n, t_q in ((18176, 568), (581632, 18176)):
        h = torch.randn(n, C, generator=gen).cuda()
        seeds = torch.arange(n // t_q, dtype=torch.int32).cuda()
        gflop = 2.0 * n * C * V / 1e9
        emit(f"--- sampling, N={n} ({n // t_q} items of {t_q} frames): one product is {gflop:.1f} GFLOP; fp32 logits would be "
             f"{4 * n * V / 2 ** 20:.0f} MiB")

        def unfused(min_p):
            def fn():
                with torch.no_grad():
                    logits = F.linear(h, w, b)
                    u = torch.rand_like(logits).clamp_(min=2.0 ** -24)
                    if min_p > 0:
                        logits = logits.masked_fill(logits < logits.max(-1, keepdim=True).values + math.log(min_p), float("-inf"))
                    return (logits - torch.log(-torch.log(u))).argmax(-1)
            return fn

        fns = {"fused    argmax (code_head_predict)": lambda: vqtts.code_head_predict(h, w, b, split=split),
               "fused    draw, no truncation": lambda: vqtts.code_head_sample(h, w, b, seeds, t_q, 1.0, 0.0, split=split),
               "fused    draw, min_p 0.05": lambda: vqtts.code_head_sample(h, w, b, seeds, t_q, 1.0, 0.05, split=split),
               "unfused  draw, no truncation": unfused(0.0), "unfused  draw, min_p 0.05": unfused(0.05)}
        times = alternate(fns)
        med = {}
        for name, fn in fns.items():
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            sweeps = 2 if name.startswith("fused") and "min_p" in name else 1
            emit(f"{name:36s}: {med[name]:9.3f} ms  (min {t[0]:.3f} .. max {t[-1]:.3f} over {len(t)} alternating windows)  "
                 f"{sweeps * gflop / med[name]:7.1f} algorithmic TFLOP/s  peak {peak(fn, lambda: None):8.1f} MiB")
        g = med["fused    argmax (code_head_predict)"]
        emit(f"draw / argmax: {med['fused    draw, no truncation'] / g:.2f} without truncation, {med['fused    draw, min_p 0.05'] / g:.2f} with "
             f"min_p; unfused / fused: {med['unfused  draw, no truncation'] / med['fused    draw, no truncation']:.2f} without, "
             f"{med['unfused  draw, min_p 0.05'] / med['fused    draw, min_p 0.05']:.2f} with min_p")
        del h
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--lines", default="all", choices=("all", "head", "sample"), help="which lines to measure")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit(f"VQTTS code head, C={C} V={V}, a tenth of the rows unscored; {torch.cuda.get_device_name(0)}")
    w = ((torch.rand(V, C, generator=gen) * 2 - 1) / C ** 0.5).cuda().requires_grad_(True)
    b = ((torch.rand(V, generator=gen) * 2 - 1) / C ** 0.5).cuda().requires_grad_(True)
    split = vqtts.WeightSplit()
    for n in (581632, 36352) if args.lines != "sample" else ():
        h = torch.randn(n, C, generator=gen).cuda().requires_grad_(True)
        t = torch.randint(0, V, (n,), generator=gen)
        t[torch.rand(n, generator=gen) < 0.1] = -1
        t = t.cuda()
        gflop = 2.0 * n * C * V / 1e9
        emit(f"--- N={n}: one product is {gflop:.1f} GFLOP; fp32 logits would be {4 * n * V / 2 ** 20:.0f} MiB")

        def reset():
            h.grad = w.grad = b.grad = None

        def fused_fwd():
            with torch.no_grad():
                return vqtts.code_head(h, w, b, t, split=split)[0]

        def fused_fb():
            reset()
            vqtts.code_head(h, w, b, t, split=split)[0].backward()

        def unfused_fwd():
            with torch.no_grad():
                return lm.cross_entropy(F.linear(h, w, b), t)[0]

        def unfused_fb():
            reset()
            lm.cross_entropy(F.linear(h, w, b), t)[0].backward()

        res = {}
        for name, fn, products in (("fused    forward", fused_fwd, 1), ("fused    forward + backward", fused_fb, 3),
                                   ("unfused  forward", unfused_fwd, 1), ("unfused  forward + backward", unfused_fb, 3)):
            ms, mib = timeit(fn), peak(fn, reset)
            res[name] = ms
            emit(f"{name:30s}: {ms:9.3f} ms  {products * gflop / ms:7.1f} algorithmic TFLOP/s  peak {mib:8.1f} MiB")
        lf, lu = fused_fwd().item(), unfused_fwd().item()
        emit(f"unfused / fused: forward {res['unfused  forward'] / res['fused    forward']:.2f}, forward + backward "
             f"{res['unfused  forward + backward'] / res['fused    forward + backward']:.2f}; loss fused {lf:.6f} unfused {lu:.6f}")
        del h, t
        torch.cuda.empty_cache()
    if args.lines != "head":
        sample_lines(emit, gen, w, b, split)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
