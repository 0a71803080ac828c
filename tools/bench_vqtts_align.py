"""Micro-benchmark of the VQTTS text-audio alignment (HIP events on the launch stream, 10 warm-up and 50 timed calls,
everything in ONE process).

Two shapes with ragged lengths, D = 128, B = 32:
  * large  Tx 200, Tq 18,176 (the 145,408-sample clip at stride 8, the largest lattice the search is sized for): the fused ``vqtts.align``, and as the CPU leg
    the numpy search of oracle/mas_oracle.py on ONE item's distance matrix (what the reference runs per item on the host);
  * small  Tx 150, Tq 800 (a GlowTTS-sized lattice): the fused ``vqtts.align`` beside the dense chain on the same device,
    ``vqtts.distance`` + ``smt_maximum_path`` + ``glow.align_index``.
It prints us per call and ns per column step (us / the longest q_len: the items run side by side, one workgroup each).

    python tools/bench_vqtts_align.py [--out FILE]
"""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-masters-thesis_amd"))
sys.path.insert(0, REPO)
from models.glow_tts.submodules import maximum_path  # noqa: E402
from smt_amd import glow, vqtts  # noqa: E402

B, D = 32, 128


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def make(tx, tq, gen):
    x_lens = torch.randint(tx // 2, tx + 1, (B,), generator=gen)
    q_lens = torch.randint(tq // 2, tq + 1, (B,), generator=gen)
    x_lens[0], q_lens[0] = tx, tq
    x = torch.randn(B, tx, D, generator=gen) + 1.5 * torch.randn(B, tx, 1, generator=gen)
    y = torch.randn(B, tq, D, generator=gen)
    for i in range(B):
        tok = (torch.arange(tq) * int(x_lens[i]) // int(q_lens[i])).clamp(max=tx - 1)
        y[i] += 0.7 * x[i, tok]
    return x.cuda(), y.cuda(), x_lens.to(torch.int32).cuda(), q_lens.to(torch.int32).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit(f"VQTTS alignment, B={B} D={D}, ragged lengths (item 0 full); {torch.cuda.get_device_name(0)}")
    for name, tx, tq in (("large", 200, 18176), ("small", 150, 800)):
        x, y, x_lens, q_lens = make(tx, tq, gen)
        emit(f"--- {name}: Tx={tx} Tq={tq} (mean x_len {x_lens.float().mean().item():.0f}, mean q_len {q_lens.float().mean().item():.0f}); "
             f"a dense fp32 distance matrix would be {4 * B * tx * tq / 1e6:.1f} MB")
        us = timeit(lambda: vqtts.align(x, y, x_lens, q_lens))
        idx, dur = vqtts.align(x, y, x_lens, q_lens)
        emit(f"fused align                       : {us:10.1f} us  {1e3 * us / tq:8.1f} ns / column step")
        if name == "small":
            mask = ((torch.arange(tx, device="cuda")[None, :, None] < x_lens[:, None, None]) &
                    (torch.arange(tq, device="cuda")[None, None, :] < q_lens[:, None, None])).float()

            def dense():
                return glow.align_index(maximum_path(-vqtts.distance(x, y), mask))
            us_d = timeit(dense)
            us_dist = timeit(lambda: vqtts.distance(x, y))
            didx, ddur = dense()
            emit(f"dense distance + search + index   : {us_d:10.1f} us  {1e3 * us_d / tq:8.1f} ns / column step  "
                 f"(distance alone {us_dist:.1f} us; dense / fused = {us_d / us:.2f}; same bits: "
                 f"{bool(torch.equal(idx, didx) and torch.equal(dur, ddur))})")
        else:
            from oracle import mas_oracle
            dist0 = vqtts.distance(x[:1], y[:1]).cpu().numpy()
            t0 = time.perf_counter()
            path = mas_oracle.maximum_path(-dist0, torch.ones(1, tx, tq).numpy())
            cpu_us = (time.perf_counter() - t0) * 1e6
            same = bool((torch.from_numpy(path[0].argmax(0)).to(torch.int32) == idx[0].cpu()).all())
            emit(f"numpy search, ONE item, host      : {cpu_us:10.1f} us  {1e3 * cpu_us / tq:8.1f} ns / column step  "
                 f"(+ {4 * tx * tq / 1e6:.1f} MB device -> host per item; same path: {same})")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
