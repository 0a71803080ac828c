"""Stand-alone timing of GlowTTS's speaker conditioning at the shape of BASELINE.json configs[4] (configs/models/glow_tts.yaml:
hidden 192; batch 32, T = 435 squeezed frames -- 870 mel frames, n_sqz 2; dropout 0.05):

  * the WN gate: `smt_amd.glow.wn_gate` (unconditioned) beside `wn_gate_cond` with the middle slice of a [B, 2H * 4] condition,
    forward and backward each, the four alternating in one loop, HIP events around `--iters` back-to-back calls; median and
    spread over `--reps` rounds.  A call is a few launches of ~10 us each, so this is the pace at which a train step issues
    them (host work included), not kernel time: for the kernels alone run the tool with `--no_step` under
    `rocprofv3 --kernel-trace --stats` (tools/kstats.py prints the table).
    Algorithmic bytes: forward 3 B T H floats (a read, acts written), backward 5 B T H (a and dacts read, da written); the
    condition adds B * 2H floats to either;
  * one train step (forward + backward + AdamW + Noam) of configs/models/glow_tts_speakers.yaml on
    configs/datasets/synthetic_tts_speakers.yaml beside the single-speaker step of configs/models/glow_tts.yaml on
    configs/datasets/synthetic_tts.yaml, batch `--batch`, the way `bench.py --workload glow_tts` steps, alternating in
    blocks of steps.

Writes the report to --out (default profiles/glow_speaker_micro.txt) and prints one JSON line.  No pass/fail threshold."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "speech-masters-thesis_amd")
sys.path.insert(0, PKG)
from smt_amd import glow  # noqa: E402
from smt_amd.lm import Drop  # noqa: E402
from utils import config as C  # noqa: E402
from utils.commons import get_model, get_optimizer  # noqa: E402


def timed(fn, iters):
    """ms per call by HIP events around `iters` calls."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def bench_gate(b, t, h, n_layers, p, iters, reps, seed):
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    a, dacts = (2 * torch.randn(b, t, 2 * h, generator=g)).to(dev), torch.randn(b, t, h, generator=g).to(dev)
    cond_all = torch.randn(b, 2 * h * n_layers, generator=g).to(dev)
    i = n_layers // 2
    cond = cond_all[:, 2 * h * i:2 * h * (i + 1)]
    lens = torch.randint(t // 2, t + 1, (b,), generator=g).to(torch.int32).to(dev)
    drop = Drop(p, True, 11, 3)
    ctx = types.SimpleNamespace(saved_tensors=(a,), drop=drop)      # what _Gate.backward reads from its context: the backward alone
    fns = {"gate fwd": lambda: glow.wn_gate(a, drop),
           "gate_cond fwd": lambda: glow.wn_gate_cond(a, cond, lens, drop),
           "gate bwd": lambda: glow._Gate.backward(ctx, dacts),
           "gate_cond bwd": lambda: glow.gate_cond_backward(a, dacts, cond, lens, drop)}
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn, iters))
    nbytes = {"gate fwd": 3 * b * t * h * 4, "gate_cond fwd": (3 * b * t * h + 2 * b * h) * 4, "gate bwd": 5 * b * t * h * 4,
              "gate_cond bwd": (5 * b * t * h + 4 * b * h) * 4}
    return {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "alg_bytes": nbytes[k],
                "gb_per_s": nbytes[k] / (statistics.median(v) * 1e-3) * 1e-9} for k, v in ms.items()}


def make_step(model_cfg, data_cfg, batch, seed):
    import train as trainlib
    from utils.commons import _resolve
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models", model_cfg)), C.load(os.path.join(PKG, "configs/datasets", data_cfg)),
                  C.create({"train": {"batch_size": batch, "n_gpus": 1, "ema": False, "grad_clip_norm": None, "seed": seed,
                                      "log_dir": "/tmp/smt_bench_glow_speaker"}}))
    torch.manual_seed(seed)
    device = torch.device("cuda")
    model, ema = get_model(cfg, device)
    optimizer, scheduler = get_optimizer(cfg, model)
    cls = _resolve(cfg.dataset["_import_"])
    ds = cls(cfg, "train")
    pool = []
    for bi in range(4):
        items = [ds[bi * batch + i] for i in range(batch)]
        pool.append([v.to(device) if torch.is_tensor(v) else v for v in cls.collate(items)])
    model.train()
    count = [0]

    def step():
        count[0] += 1
        return trainlib.train_step(global_step=count[0], batch=pool[count[0] % len(pool)], config=cfg, model=model, ema=ema,
                                   optimizer=optimizer, scheduler=scheduler, device=device)
    frames = sum(int(p[3].sum()) for p in pool) / len(pool)
    return step, frames


def bench_step(batch, warmup, steps, reps, seed):
    import time
    single, f1 = make_step("glow_tts.yaml", "synthetic_tts.yaml", batch, seed)
    multi, f2 = make_step("glow_tts_speakers.yaml", "synthetic_tts_speakers.yaml", batch, seed)
    for _ in range(warmup):
        single(); multi()
    torch.cuda.synchronize()
    ms = {"single": [], "multi": []}
    for _ in range(reps):
        for name, fn in (("single", single), ("multi", multi)):
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    return {k: {"ms_per_step_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ms.items()}, (f1, f2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--t", type=int, default=435)
    ap.add_argument("--hidden", type=int, default=192)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--step_reps", type=int, default=3)
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "glow_speaker_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_glow_speaker times kernels on MI355X; no GPU is visible")
    gate = bench_gate(args.batch, args.t, args.hidden, 4, 0.05, args.iters, args.reps, args.seed)
    lines = [f"GlowTTS speaker conditioning, {torch.cuda.get_device_name(0)}",
             f"WN gate, B = {args.batch}, T = {args.t}, H = {args.hidden}, dropout 0.05, cond = slice 2 of 4 of a [B, 2H * 4] tensor; "
             f"{args.iters} calls per timing, median [min, max] of {args.reps} alternating rounds",
             f"{'':16s}{'ms':>10s}{'min':>10s}{'max':>10s}{'alg MB':>10s}{'GB/s':>10s}"]
    for k, v in gate.items():
        lines.append(f"{k:16s}{v['ms_median']:10.4f}{v['ms_min']:10.4f}{v['ms_max']:10.4f}{v['alg_bytes'] / 1e6:10.2f}{v['gb_per_s']:10.1f}")
    lines.append(f"gate_cond / gate: fwd {gate['gate_cond fwd']['ms_median'] / gate['gate fwd']['ms_median']:.3f}, "
                 f"bwd {gate['gate_cond bwd']['ms_median'] / gate['gate bwd']['ms_median']:.3f}")
    out = {"tool": "bench_glow_speaker", "gate": gate}
    if not args.no_step:
        step, frames = bench_step(args.batch, args.warmup, args.steps, args.step_reps, args.seed)
        out["step"] = step
        lines += ["", f"train step (forward + backward + AdamW), batch {args.batch}, fp32, dropout on; {args.steps} steps per timing after "
                      f"{args.warmup} warm-up steps each, median [min, max] of {args.step_reps} alternating rounds; "
                      f"mean mel frames per batch {frames[0]:.0f} / {frames[1]:.0f}",
                  f"{'single-speaker (glow_tts.yaml)':44s}{step['single']['ms_per_step_median']:10.2f} ms  "
                  f"[{step['single']['ms_min']:.2f}, {step['single']['ms_max']:.2f}]",
                  f"{'8 speakers, gin 64 (glow_tts_speakers.yaml)':44s}{step['multi']['ms_per_step_median']:10.2f} ms  "
                  f"[{step['multi']['ms_min']:.2f}, {step['multi']['ms_max']:.2f}]",
                  f"multi / single: {step['multi']['ms_per_step_median'] / step['single']['ms_per_step_median']:.3f}"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
