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

    python tools/bench_code_head.py [--out FILE]
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
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
    for n in (581632, 36352):
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
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
