"""Micro-benchmark of the grouped (text-conditioned) VQ kernels at the reference's VQTTS sizes: G = 149 tokens, L = 512
codes per token, D = 128 (HIP events on the launch stream, warm-up, many iterations, everything in ONE process).

Per row count N and group usage it prints the grouped search, the large-table EMA accumulate and apply, and two
comparison rows on the same data: this repository's flat search at K = 512 (all rows against one token's codes) and the
reference's formulation (gather k[x_id] + bmm + min, bottleneck.py:39-52) written with torch ops on the device.

    python tools/bench_vq_grouped.py [--out FILE]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-masters-thesis_amd"))
from smt_amd import vq  # noqa: E402

G, L, D = 149, 512, 128


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


def reference_formulation(x, group, k3):
    """bottleneck.py:39-52 on the device: the [N, L, D] gather, bmm, min."""
    k = k3[group]
    dist = (x.unsqueeze(1) ** 2).sum(-1) - 2 * torch.bmm(x.unsqueeze(1), k.transpose(1, 2)).squeeze(1) + (k ** 2).sum(-1)
    return torch.min(dist, dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    centre = 2.0 * torch.randn(G, 1, D, generator=gen) + 3.0 * torch.randn(1, 1, D, generator=gen)
    cb = (torch.randn(G, L, D, generator=gen) + centre).reshape(G * L, D).cuda()
    prep = vq.grouped_prepare(cb, G, L)
    emit(f"grouped VQ, G={G} L={L} D={D} ({G * L} codes, {4 * G * L * D / 1e6:.1f} MB table); "
         f"grouped_prepare {timeit(lambda: vq.grouped_prepare(cb, G, L, prep)):.1f} us")
    for n in (4544, 36352):
        for usage in ("uniform", "zipf"):
            if usage == "uniform":
                group = torch.randint(0, G, (n,), generator=gen)
            else:
                w = 1.0 / torch.arange(1, G + 1, dtype=torch.float64)
                group = torch.multinomial(w / w.sum(), n, replacement=True, generator=gen)
            x = (torch.randn(n, D, generator=gen) + centre[group, 0]).cuda()
            group = group.to(torch.int32).cuda()
            emit(f"--- N={n} groups {usage} (largest group {int(torch.bincount(group.long()).max())} rows)")
            us = timeit(lambda: vq.grouped_forward_raw(x, group, cb, G, L, prep=prep))
            out = vq.grouped_forward_raw(x, group, cb, G, L, prep=prep)
            used = int(torch.unique(group).numel())
            alg = n * (4 * D + 4 + 16 + 4 + 4 * D) + 4 * used * L * D
            emit(f"grouped search        : {us:9.1f} us  {alg / us / 1e6:7.3f} TB/s alg  {3 * 2.0 * n * L * D / us / 1e6:7.2f} TFLOP/s "
                 f"bf16-MFMA  queued={int(out[4][3].item())}")
            # (ii) the flat search at K = 512 on the same rows (one token's codes for every row)
            cb0 = cb[:L].contiguous()
            prep0 = vq.prepare(cb0)
            us_flat = timeit(lambda: vq.vq_forward_raw(x, cb0, prep=prep0))
            emit(f"flat search K={L}     : {us_flat:9.1f} us  (grouped / flat = {us / us_flat:.2f})")
            # (i) the reference's formulation with torch ops; the gather alone is n * L * D * 4 bytes
            k3 = cb.view(G, L, D)
            try:
                us_ref = timeit(lambda: reference_formulation(x, group.long(), k3), iters=10, warmup=3)
                q_ref = reference_formulation(x, group.long(), k3)[1]
                agree = float((q_ref == out[0]).float().mean())
                emit(f"torch gather+bmm+min  : {us_ref:9.1f} us  (torch / grouped = {us_ref / us:.1f}; gather {n * L * D * 4 / 1e9:.2f} GB; "
                     f"fp32 indices agree on {100 * agree:.2f}% of rows)")
            except torch.cuda.OutOfMemoryError:
                emit(f"torch gather+bmm+min  : out of memory (gather {n * L * D * 4 / 1e9:.2f} GB)")
            torch.cuda.empty_cache()
            # EMA statistics over the whole table, beside the existing path at K = 1024 on the same rows
            q_abs = out[1]
            stats = torch.empty(vq.ema_stats_numel(G * L, D), device="cuda")
            us_acc = timeit(lambda: vq.ema_accumulate(x, q_abs, None, G * L, stats))
            emit(f"ema_accumulate K={G * L}: {us_acc:9.1f} us  {(n * (4 * D + 8) + 4 * G * L * (D + 1)) / us_acc / 1e6:7.3f} TB/s alg")
            idx1k = q_abs % 1024
            stats1k = torch.empty(vq.ema_stats_numel(1024, D), device="cuda")
            us_1k = timeit(lambda: vq.ema_accumulate(x, idx1k, None, 1024, stats1k))
            emit(f"ema_accumulate K=1024 : {us_1k:9.1f} us  (existing path, same rows)")
            cbw, ks, ke = cb.clone(), cb.clone(), torch.ones(G * L, device="cuda")
            prepw = vq.grouped_prepare(cbw, G, L)
            us_app = timeit(lambda: vq.grouped_ema_apply(cbw, ks, ke, stats, cb, 0.99, 1.0, G, L, prepw))
            emit(f"grouped_ema_apply (+ prep refresh): {us_app:9.1f} us  {(4 * (5 * G * L * D + 3 * G * L) + 4 * G * L * D) / us_app / 1e6:7.3f} TB/s alg")
            del stats, cbw, ks, ke, prepw
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
