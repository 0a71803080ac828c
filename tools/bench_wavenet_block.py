"""Micro-benchmark of the WaveNet block (one process, HIP events on the launch stream, every line warmed up, then timed in
ALTERNATING windows: five rounds of about 0.2 s per line; a line reports the median over the rounds and the spread min .. max).

bf16, N = B * T rows at two sizes (2 and 32 items of 18,176 frames: the 145,408-sample clip at stride 8), H in {64, 128}:
  (a) ``convops.wavenet_tail`` fused (smt_wavenet_tail_fwd): 4 H elements of traffic per row;
  (b) the unfused path, ``wavenet_gate`` + ``conv1d(residual=)``: 6 H elements per row;
  (c) the gate alone, forward (3 H) and backward (5 H).
Each line: ms per call, GB/s on those algorithmic bytes and the fraction of the 8 TB/s HBM peak.
Then one full block (W = 64, depth 4, growth 3) forward + backward with ``_WN_TAIL`` on and off, and the train step
(forward + backward + optimizer) of configs/models/vqvae_k1024.yaml (bf16, batch 32 x 145,408 samples) at
``block_type: wavenet`` beside ``gated_hifi``.  No pass/fail threshold.

    python tools/bench_wavenet_block.py [--out profiles/wavenet_block_micro.txt] [--skip-step]
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "speech-masters-thesis_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, REPO)
from smt_amd import convops, profiler  # noqa: E402

DEV = "cuda:0"
ITEM_T = 18176
PEAK = profiler.HBM_PEAK_GBS


def _window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms


def alternate(fns, rounds=5, window_ms=200.0, warmup=5):
    """{name: [ms per call, one per round]}: every line warmed up first, then `rounds` rounds in which the lines take turns."""
    iters = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        iters[name] = max(10, int(window_ms / max(_window(fn, 5), 1e-3)))
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(_window(fn, iters[name]))
    return times


def fmt(name, ms, nbytes=None):
    med = statistics.median(ms)
    line = f"{name:<44s}: {med:9.4f} ms  (min {min(ms):.4f} .. max {max(ms):.4f} over {len(ms)} alternating windows)"
    if nbytes:
        gbs = nbytes / med * 1e-6
        line += f"  {gbs:8.1f} GB/s  {gbs / PEAK:6.1%} of {PEAK / 1000:.0f} TB/s"
    return line


def with_tail(flag, fn):
    def run():
        old = (convops._WN_TAIL, convops._WN_TAIL_WIDTHS)
        convops._WN_TAIL, convops._WN_TAIL_WIDTHS = flag, (64, 128)
        try:
            return fn()
        finally:
            convops._WN_TAIL, convops._WN_TAIL_WIDTHS = old
    return run


def micro(emit, hidden, items):
    g = torch.Generator().manual_seed(hidden + items)
    n = items * ITEM_T
    z = ((torch.rand(items, ITEM_T, 2 * hidden, generator=g) * 2 - 1) * 4).to(torch.bfloat16).to(DEV)
    x = torch.randn(items, ITEM_T, hidden, generator=g).to(torch.bfloat16).to(DEV)
    da = torch.randn(items, ITEM_T, hidden, generator=g).to(torch.bfloat16).to(DEV)
    weight = torch.nn.Parameter(((torch.rand(hidden, hidden, 1, generator=g) * 2 - 1) / hidden ** 0.5).to(DEV))
    bias = torch.nn.Parameter(torch.zeros(hidden, device=DEV))
    lens = torch.full((items,), ITEM_T, dtype=torch.int32, device=DEV)
    a, dz = torch.empty_like(x), torch.empty_like(z)

    def tail():
        with torch.no_grad():
            return convops.wavenet_tail(z, x, weight, bias, lens)
    fns = {"(a) wavenet_tail fused": with_tail(True, tail), "(b) gate + conv1d(residual=)": with_tail(False, tail),
           "(c) gate forward": lambda: convops._wavenet_gate_fwd(z, a, lens),
           "(c) gate backward": lambda: convops._wavenet_gate_bwd(z, da, dz, lens)}
    per_row = {"(a) wavenet_tail fused": 4, "(b) gate + conv1d(residual=)": 6, "(c) gate forward": 3, "(c) gate backward": 5}
    times = alternate(fns)
    emit(f"--- H={hidden}, N={n} rows ({items} items of {ITEM_T} frames), bf16")
    for name, ms in times.items():
        emit(fmt(name, ms, per_row[name] * hidden * 2.0 * n))
    ta, tb = statistics.median(times["(a) wavenet_tail fused"]), statistics.median(times["(b) gate + conv1d(residual=)"])
    emit(f"(b) / (a) = {tb / ta:.2f}")
    return ta < tb


def block(emit):
    from models.vqvae.resnet import WaveNetBlock
    torch.manual_seed(0)
    blk = WaveNetBlock(64, 4, dilation_growth_rate=3, zero_out=False).to(DEV).train()
    items = 32
    x = torch.randn(items, ITEM_T, 64, device=DEV).to(torch.bfloat16).requires_grad_(True)
    r = torch.randn(items, ITEM_T, 64, device=DEV).to(torch.bfloat16)
    lens = torch.full((items,), ITEM_T, dtype=torch.int32, device=DEV)

    def fwd():
        with torch.no_grad():
            blk(x, lens)

    def fb():
        blk.zero_grad(set_to_none=True)
        x.grad = None
        blk(x, lens).backward(r)
    times = alternate({"block forward,   _WN_TAIL on": with_tail(True, fwd), "block forward,   _WN_TAIL off": with_tail(False, fwd),
                       "block fwd + bwd, _WN_TAIL on": with_tail(True, fb), "block fwd + bwd, _WN_TAIL off": with_tail(False, fb)},
                      window_ms=300.0)
    emit(f"--- one WaveNetBlock(64, depth 4, growth 3), bf16, {items} x {ITEM_T} rows; wall time of the launch stream (host included)")
    for name, ms in times.items():
        emit(fmt(name, ms))
    # the same step as the sum of its kernels' own durations (an event pair around every launch: smt_amd.profiler)
    for flag in (True, False):
        run = with_tail(flag, fb)
        run()
        profiler.enable(True)
        profiler.reset()
        for _ in range(5):
            run()
        rows = profiler.summary()
        profiler.enable(False)
        profiler.reset()
        emit(f"kernels of fwd + bwd, _WN_TAIL {'on ' if flag else 'off'}: {sum(r_['total_ms'] for r_ in rows) / 5:.4f} ms in "
             f"{sum(r_['launches'] for r_ in rows) // 5} launches: " +
             ", ".join(f"{r_['name']} {r_['launches'] // 5} x {r_['avg_us']:.1f} us" for r_ in rows))


def make_step(cfg, pool, warmup):
    from utils.commons import get_model, get_optimizer
    torch.manual_seed(0)
    model, _ = get_model(cfg, DEV)
    opt, sched = get_optimizer(cfg, model)
    model.train()
    it = [0]

    def step():
        opt.zero_grad(set_to_none=True)
        loss_dict, _ = model.supervised_step(pool[it[0] % len(pool)])
        loss_dict["loss"].backward()
        opt.step()
        sched.step()
        it[0] += 1
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    return step, sum(p.numel() for p in model.parameters())


def train_step(emit, steps, warmup):
    import bench
    args = bench.parse(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)])
    pool = bench.synthetic_batches(2, args.batch, args.clip_len, 0, DEV)
    emit(f"--- train step of {args.model} (bf16, batch {args.batch} x {args.clip_len} samples): forward + backward + optimizer")
    steps_of, n_params = {}, {}
    for block_type in ("gated_hifi", "wavenet"):
        cfg = bench.make_config(args)
        cfg.model.block_type = block_type
        steps_of[block_type], n_params[block_type] = make_step(cfg, pool, warmup)
    times = {k: [] for k in steps_of}
    for _ in range(3):
        for k, step in steps_of.items():
            times[k].append(_window(step, steps))
    for k, ms in times.items():
        emit(fmt(f"block_type: {k} ({n_params[k]:,} parameters)", ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--skip-step", action="store_true", help="leave the model train step out")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("# python tools/bench_wavenet_block.py --out profiles/wavenet_block_micro.txt, one MI355X")
    emit(f"WaveNet block; {torch.cuda.get_device_name(0)}")
    faster = {}
    for hidden in (64, 128):
        faster[hidden] = all([micro(emit, hidden, items) for items in (2, 32)])
    for hidden, ok in faster.items():
        emit(f"H={hidden}: fused tail faster than gate + conv1d at both N: {ok}  ->  _WN_TAIL default {'on' if ok else 'off'} at this width")
    block(emit)
    if not args.skip_step:
        train_step(emit, args.steps, args.warmup)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
