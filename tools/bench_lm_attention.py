#!/usr/bin/env python3
"""The attention core of the TransformerLM on bf16 MFMAs (smt_lm_attention_bf16_fwd / _bwd, model.attention_dtype: bf16)
against the fp32 kernels (smt_lm_attention_fwd / _bwd) in ONE process at the shipped configuration's shape, batch 8 x 16 heads
x 258 tokens, causal, with attention dropout 0.1 and 0, and the eager train step of the three shipped configurations
(transformer_lm, transformer_lm_bf16, transformer_lm_bf16_attn).

HIP events; every figure is the median of five windows, the windows of the two arms alternate, and the spread of each arm's
windows (min .. max) stands next to it: a difference inside the spread is no difference.  The calls are the C entries
themselves on preallocated buffers (ctypes, no autograd, no allocation), so a window is a run of back-to-back launches; the
backward call is two kernels (dq, then dk/dv).  Random operands.  Reads nothing outside the repository.  Kernel times per kernel
come from a kernel trace of `--trace-workload` (rocprofv3 --kernel-trace, in a run of its own) given back with --kernel-trace.

    python tools/bench_lm_attention.py [--out profiles/lm_attention_micro.txt] [--reps 200] [--steps 10]

--head_dim 64 measures the head-dim-64 instantiations (smt_lm_attention_hd_fwd / _bwd, nhead = d_model / 64) instead: batch 8 x 8
heads x 258 tokens, the same d_model, tokens and algorithmic FLOPs as 8 x 16 x 258 at head dim 32, which is timed in the same
windows as the yardstick; the train step compares transformer_lm.yaml with transformer_lm_h8.yaml.

    python tools/bench_lm_attention.py --head_dim 64 [--out profiles/lm_attention_hd64_micro.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "speech-masters-thesis_amd"))

import torch  # noqa: E402

BATCH, HEADS, LEN = 8, 16, 258
WINDOWS = 5
DEV = "cuda:0"
ENTRIES = {"fp32": ("smt_lm_attention_fwd", "smt_lm_attention_bwd"), "bf16": ("smt_lm_attention_bf16_fwd", "smt_lm_attention_bf16_bwd")}
CONFIGS = {"fp32": "transformer_lm.yaml", "bf16": "transformer_lm_bf16.yaml", "bf16_attn": "transformer_lm_bf16_attn.yaml"}
HD64_HEADS = HEADS // 2                       # head dim 64 at the same d_model
HD64_CONFIGS = {"h16": "transformer_lm.yaml", "h8": "transformer_lm_h8.yaml"}


def window_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def alternate(arms, reps):
    """{name: (median, min, max) ms per call} over WINDOWS windows per arm, the arms taking turns."""
    for fn in arms.values():
        window_ms(fn, max(3, reps // 5))
    times = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, fn in arms.items():
            times[name].append(window_ms(fn, reps))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def attention_arms(p, dtypes=("fp32", "bf16"), heads=HEADS, head_dim=32):
    """{"fwd": {dtype: fn}, "bwd": {dtype: fn}}: the C entries on one set of buffers per dtype (head dim 32: the four entries
    without a head-dim argument; 64: smt_lm_attention_hd_fwd / _bwd)."""
    from smt_amd import lm as K
    from smt_amd import native as N
    g = torch.Generator().manual_seed(0)
    d = heads * head_dim
    qkv = torch.randn(BATCH, LEN, 3 * d, generator=g).to(DEV)
    dctx = torch.randn(BATCH, LEN, d, generator=g).to(DEV)
    lens = torch.full((BATCH,), LEN - 1, dtype=torch.int32, device=DEV)
    drop = K.Drop(p, True, 1, 1)
    lib, stream = N.lib(), N.stream_ptr()
    arms = {"fwd": {}, "bwd": {}}
    for name in dtypes:
        if head_dim == 32:
            fwd, bwd = (getattr(lib, e) for e in ENTRIES[name])
            tail = (stream,)
        else:
            fwd, bwd = lib.smt_lm_attention_hd_fwd, lib.smt_lm_attention_hd_bwd
            tail = (head_dim, int(name == "bf16"), stream)
        ctx, lse = torch.empty(BATCH, LEN, d, device=DEV), torch.empty(BATCH, heads, LEN, device=DEV)
        dqkv, delta = torch.empty_like(qkv), torch.empty_like(lse)
        fargs = (N.ptr(qkv), N.ptr(lens), N.ptr(ctx), N.ptr(lse), BATCH, LEN, heads, 1, drop.key, None, drop.thresh, drop.scale) + tail
        bargs = (N.ptr(qkv), N.ptr(lens), N.ptr(ctx), N.ptr(lse), N.ptr(dctx), N.ptr(dqkv), N.ptr(delta), BATCH, LEN, heads, 1, drop.key, None,
                 drop.thresh, drop.scale) + tail
        N.check(fwd(*fargs), ENTRIES[name][0])                           # the backward arm reads this forward's ctx and lse
        arms["fwd"][name] = lambda fwd=fwd, fargs=fargs, keep=(ctx, lse): fwd(*fargs)
        arms["bwd"][name] = lambda bwd=bwd, bargs=bargs, keep=(dqkv, delta): bwd(*bargs)
    arms["keep"] = (qkv, dctx, lens)
    return arms


def kernel_table(trace_csv):
    """Median kernel time per attention kernel from a rocprofv3 --kernel-trace CSV of `--trace-workload`."""
    import csv
    got = {}
    for r in csv.DictReader(open(trace_csv)):
        name = r["Kernel_Name"]
        if "lm_attn_" in name:
            short = name[name.index("lm_attn_"):].split("(")[0]
            got.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return [f"  {name:<34}{statistics.median(t):>8.1f} us   ({len(t)} launches, min {min(t):.1f}, max {max(t):.1f})" for name, t in sorted(got.items())]


def bench_step(steps, configs=CONFIGS):
    from tools.bench_lm import build
    from utils import config as C
    from utils.commons import get_optimizer
    from models.transformer_lm.transformer_lm import TransformerLM
    g = torch.Generator().manual_seed(1)
    x = torch.randint(2, 514, (BATCH, LEN), generator=g)
    x[:, 0] = 1
    x[:, -1] = 0
    lens = torch.full((BATCH,), LEN - 1)
    x, lens = x.to(DEV), lens.to(DEV)
    arms, keep = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        build(tmp)                                                       # writes the throw-away VQ-VAE run the LM configs point at
        for name, base in configs.items():
            cfg = C.load(os.path.join(ROOT, "speech-masters-thesis_amd", "configs/models", base))
            cfg.model.vqvae.log_dir, cfg.model.vqvae.ckpt_num = os.path.join(tmp, "vqvae"), 1
            torch.manual_seed(0)
            model = TransformerLM(cfg).to(DEV).train()
            opt, sched = get_optimizer(cfg, model)
            keep.append((model, opt, sched))

            def fn(model=model, opt=opt, sched=sched):
                opt.zero_grad(set_to_none=True)
                model(x, lens, None, None)[0]["loss"].backward()
                opt.step()
                sched.step()
            arms[name] = fn
    return alternate(arms, steps)


def resources(head_dim=32):
    """VGPR / AGPR / LDS / occupancy of the six attention kernels of one head dim as the compiler reports them (a compile of
    csrc/lm.hip with -Rpass-analysis=kernel-resource-usage, nothing kept); empty where there is no hipcc."""
    import re
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "speech-masters-thesis_amd", "csrc", "lm.hip")
    if not os.path.exists(hipcc):
        return []
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=on", "-Rpass-analysis=kernel-resource-usage",
                              "-c", src, "-o", os.path.join(tmp, "x.o")], capture_output=True, text=True).stderr
    lines, cur = [], None
    keys = r"Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]"
    for m in re.finditer(r"remark: +(" + keys + r"): (\S+)", err):
        key, val = m.groups()
        if key == "Function Name":
            cur = [val] if "lm_attn_" in val and f"ELi{head_dim // 32}E" in val else None     # <BF, NC>: NC = head_dim / 32
            if cur:
                lines.append(cur)
        elif cur is not None:
            cur.append(f"{key} {val}")
    return ["  " + ", ".join(c) for c in lines]


def main_hd64(args):
    """Head dim 64 at 8 x 8 x 258 against head dim 32 at 8 x 16 x 258, entry by entry, in the same alternating windows."""
    from smt_amd.lm import _attn_flops
    if args.trace_workload:
        for arms in (attention_arms(0.1), attention_arms(0.1, heads=HD64_HEADS, head_dim=64)):
            for phase in ("fwd", "bwd"):
                for fn in arms[phase].values():
                    for _ in range(20):
                        fn()
        torch.cuda.synchronize()
        return
    assert _attn_flops(BATCH, HEADS, LEN, True, 1) == _attn_flops(BATCH, HD64_HEADS, LEN, True, 1, 64)
    lines = [f"tools/bench_lm_attention.py --head_dim 64: {BATCH} x {HD64_HEADS} heads x {LEN} tokens at head dim 64 (dh64) against {BATCH} x {HEADS} "
             f"heads x {LEN} tokens at head dim 32 (dh32), the same d_model, tokens and algorithmic FLOPs",
             f"causal, lens {LEN - 1}; HIP events, median (min .. max) of {WINDOWS} alternating windows of {args.reps} calls, one process; bwd = dq + dk/dv kernels",
             f"{torch.cuda.get_device_name(0)}; the C entries on preallocated buffers; GF = algorithmic GFLOP/s of the dh64 arm (2 products forward, 5 backward)",
             "", f"{'dropout':<9}{'dtype':<6}{'phase':<6}{'dh32 us':>9}{'(min .. max)':>18}{'dh64 us':>9}{'(min .. max)':>18}{'dh64/dh32':>11}{'dh64 GF':>10}"]
    for p in (0.1, 0.0):
        a32, a64 = attention_arms(p), attention_arms(p, heads=HD64_HEADS, head_dim=64)
        for phase, products in (("fwd", 2), ("bwd", 5)):
            t = alternate({f"{dt}/{dh}": arms[phase][dt] for dt in ("fp32", "bf16") for dh, arms in ((32, a32), (64, a64))}, args.reps)
            for dt in ("fp32", "bf16"):
                (f, fl, fh), (b, bl, bh) = t[f"{dt}/32"], t[f"{dt}/64"]
                gf = _attn_flops(BATCH, HD64_HEADS, LEN, True, products, 64) / (b * 1e-3) * 1e-9
                lines.append(f"{p:<9}{dt:<6}{phase:<6}{f * 1e3:>9.1f}{f'({fl * 1e3:.1f} .. {fh * 1e3:.1f})':>18}{b * 1e3:>9.1f}"
                             f"{f'({bl * 1e3:.1f} .. {bh * 1e3:.1f})':>18}{b / f:>11.3f}{gf:>10.0f}")
                print(lines[-1], flush=True)
    if not args.no_step:
        t = bench_step(args.steps, HD64_CONFIGS)
        lines += ["", f"eager train step, batch {BATCH} x {LEN} (forward + backward + optimizer), median (min .. max) of {WINDOWS} windows of "
                  f"{args.steps} steps:"]
        lines += [f"  {name:<10}{HD64_CONFIGS[name]:<32}{m:>7.2f} ms  ({lo:.2f} .. {hi:.2f})" for name, (m, lo, hi) in t.items()]
        print("\n".join(lines[-3:]), flush=True)
    if args.kernel_trace:
        lines += ["", "kernel times (rocprofv3 --kernel-trace of `--head_dim 64 --trace-workload`, a run of its own; dropout 0.1; <BF, NC>: "
                  "BF = bf16 operands, NC = head dim / 32):"] + kernel_table(args.kernel_trace)
    res_lines = [] if args.no_resources else resources(64)
    if res_lines:
        lines += ["", "kernel resources of the head-dim-64 instantiations (hipcc -Rpass-analysis=kernel-resource-usage on csrc/lm.hip; "
                  "ILb0ELi2E = fp32, ILb1ELi2E = bf16):"] + res_lines
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head_dim", type=int, choices=(32, 64), default=32, help="64: the head-dim-64 kernels at 8 x 8 x 258 against head dim 32 at 8 x 16 x 258")
    ap.add_argument("--out", default=None, help="default profiles/lm_attention_micro.txt, with --head_dim 64 profiles/lm_attention_hd64_micro.txt")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--kernel-trace", help="a rocprofv3 --kernel-trace CSV of --trace-workload: add the kernel-time table to the output")
    ap.add_argument("--trace-workload", action="store_true", help="only issue 20 calls of every entry, dropout 0.1 (for a kernel trace)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "lm_attention_micro.txt" if args.head_dim == 32 else "lm_attention_hd64_micro.txt")
    if args.head_dim == 64:
        return main_hd64(args)
    if args.trace_workload:
        arms = attention_arms(0.1)
        for phase in ("fwd", "bwd"):
            for fn in arms[phase].values():
                for _ in range(20):
                    fn()
        torch.cuda.synchronize()
        return
    from smt_amd.lm import _attn_flops
    lines = [f"tools/bench_lm_attention.py: {BATCH} x {HEADS} heads x {LEN} tokens, causal, lens {LEN - 1}; HIP events, median (min .. max) of "
             f"{WINDOWS} alternating windows of {args.reps} calls, one process",
             f"{torch.cuda.get_device_name(0)}; the C entries on preallocated buffers; GF = algorithmic GFLOP/s of the bf16 arm (2 products forward, 5 backward)",
             "", f"{'dropout':<9}{'phase':<6}{'fp32 us':>9}{'(min .. max)':>18}{'bf16 us':>9}{'(min .. max)':>18}{'bf16/fp32':>11}{'bf16 GF':>10}"]
    for p in (0.1, 0.0):
        arms = attention_arms(p)
        for phase, products in (("fwd", 2), ("bwd", 5)):
            t = alternate(arms[phase], args.reps)
            (f, fl, fh), (b, bl, bh) = t["fp32"], t["bf16"]
            gf = _attn_flops(BATCH, HEADS, LEN, True, products) / (b * 1e-3) * 1e-9
            lines.append(f"{p:<9}{phase:<6}{f * 1e3:>9.1f}{f'({fl * 1e3:.1f} .. {fh * 1e3:.1f})':>18}{b * 1e3:>9.1f}{f'({bl * 1e3:.1f} .. {bh * 1e3:.1f})':>18}"
                         f"{b / f:>11.3f}{gf:>10.0f}")
            print(lines[-1], flush=True)
    if not args.no_step:
        t = bench_step(args.steps)
        lines += ["", f"eager train step, shipped configurations, batch {BATCH} x {LEN} (forward + backward + optimizer), median (min .. max) of "
                  f"{WINDOWS} windows of {args.steps} steps:"]
        lines += [f"  {name:<10}{CONFIGS[name]:<32}{m:>7.2f} ms  ({lo:.2f} .. {hi:.2f})" for name, (m, lo, hi) in t.items()]
        print("\n".join(lines[-4:]), flush=True)
    if args.kernel_trace:
        lines += ["", "kernel times (rocprofv3 --kernel-trace of `--trace-workload`, a run of its own; dropout 0.1):"] + kernel_table(args.kernel_trace)
    res_lines = [] if args.no_resources else resources()
    if res_lines:
        lines += ["", "kernel resources (hipcc -Rpass-analysis=kernel-resource-usage on csrc/lm.hip; <false> = fp32, <true> = bf16):"] + res_lines
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
