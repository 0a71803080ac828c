#!/usr/bin/env python3
"""The bf16 projections of the TransformerLM (smt_amd.lm.linear, csrc/lm_linear.hip) against the library's fp32 GEMM
(torch.nn.functional.linear and its autograd: the path of compute_dtype fp32) in ONE process, on the five product shapes of
the shipped configuration at rows = 8 x 258 = 2064, and the eager train step of that configuration in both dtypes.

HIP events; every figure is the median of five windows, and the windows of the two arms alternate.  Random operands.  Reads
nothing outside the repository.  The per-shape figures are CALL times: device events around a run of eager calls, so where the
kernel is shorter than the host takes to issue it (Python, ctypes, the pack-cache lookup) they show the host.  Kernel times
come from a kernel trace of `--trace-workload` (rocprofv3 --kernel-trace, in a run of its own).

    python tools/bench_lm_linear.py [--out profiles/lm_linear_micro.txt] [--reps 50] [--steps 10]
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

ROWS = 2064
SHAPES = [("in_proj", 512, 1536), ("out_proj", 512, 512), ("linear1", 512, 2048), ("linear2", 2048, 512), ("classifier", 512, 512)]
PEAK_BF16_TFLOPS = 2500.0
WINDOWS = 5
DEV = "cuda:0"


def window_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def alternate(arms, reps):
    """{name: median ms per call} over WINDOWS windows per arm, the arms taking turns."""
    for fn in arms.values():
        window_ms(fn, max(3, reps // 5))                  # warm-up: packs, workspaces, library heuristics
    times = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, fn in arms.items():
            times[name].append(window_ms(fn, reps))
    return {name: statistics.median(t) for name, t in times.items()}


def bench_shape(n_in, n_out, reps, dtypes=("fp32", "bf16")):
    from smt_amd import lm as K
    g = torch.Generator().manual_seed(n_in + n_out)
    x = torch.randn(ROWS, n_in, generator=g).to(DEV)
    dy = torch.randn(ROWS, n_out, generator=g).to(DEV)
    w = torch.nn.Parameter((torch.randn(n_out, n_in, generator=g) * n_in ** -0.5).to(DEV))
    w_frozen = torch.nn.Parameter(w.detach(), requires_grad=False)
    bias = torch.nn.Parameter(torch.zeros(n_out, device=DEV))
    out = {}
    for phase in ("fwd", "dgrad", "wgrad"):
        arms = {}
        for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            if name not in dtypes:
                continue
            if phase == "fwd":
                def fn(dtype=dtype):
                    with torch.no_grad():
                        K.linear(x, w, bias, compute_dtype=dtype)
            else:
                # one of the two products alone: autograd runs only what the requested gradient needs
                # (the weight stays a Parameter, as in the model: its packed copies come from the cache; a custom autograd
                # function computes every gradient its inputs ask for, so the data-gradient arm takes a frozen Parameter)
                xg = x.clone().requires_grad_(phase == "dgrad")
                wg = w if phase == "wgrad" else w_frozen
                bg = bias if phase == "wgrad" else None
                y = K.linear(xg, wg, bg, compute_dtype=dtype)
                wanted = [xg] if phase == "dgrad" else [wg, bg]

                def fn(y=y, wanted=wanted):
                    torch.autograd.grad(y, wanted, dy, retain_graph=True)
            arms[name] = fn
        out[phase] = alternate(arms, reps)
    return out


def kernel_table(trace_csv):
    """Kernel times per shape and phase from a rocprofv3 --kernel-trace CSV of `--trace-workload`: the lm_linear kernels in
    start order are, per shape, 23 forward launches, 1 more (the graph of the data-gradient arm), 23 data gradients, 1 forward,
    and 23 weight gradients with their reduce launches."""
    import csv
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    ks = [("nt" if "nt_kernel" in r["Kernel_Name"] else "wgrad" if "wgrad" in r["Kernel_Name"] else "reduce",
           (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r["Grid_Size_X"]) // 256, int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"]))
          for r in rows if "lm_linear" in r["Kernel_Name"]]
    med = statistics.median
    lines = [f"{'shape':<11}{'n_in':>5}{'n_out':>6}  {'fwd us':>7}{'TF':>5}  {'dgrad us':>8}{'TF':>5}  {'wgrad us':>8}{'+ reduces':>10}{'TF':>5}   workgroups fwd / dgrad / wgrad"]
    i = 0
    for name, n_in, n_out in SHAPES:
        got = {"nt": [], "wgrad": [], "reduce": []}
        while i < len(ks) and (len(got["nt"]) < 48 or ks[i][0] != "nt"):
            got[ks[i][0]].append(ks[i])
            i += 1
        nt, wg, rd = got["nt"], got["wgrad"], got["reduce"]
        flops = 2.0 * ROWS * n_in * n_out
        f, d, w = med(k[1] for k in nt[:23]), med(k[1] for k in nt[24:47]), med(k[1] for k in wg)
        r = sum(k[1] for k in rd) / max(1, len(wg))
        lines.append(f"{name:<11}{n_in:>5}{n_out:>6}  {f:>7.1f}{flops / f * 1e-6:>5.0f}  {d:>8.1f}{flops / d * 1e-6:>5.0f}  {w:>8.1f}{r:>10.1f}{flops / (w + r) * 1e-6:>5.0f}"
                     f"   {nt[0][2]}x{nt[0][3]} / {nt[30][2]}x{nt[30][3]} / {wg[0][2]}x{wg[0][3]}x{wg[0][4]}")
    return lines


def bench_step(steps):
    from tools.bench_lm import build
    from utils import config as C
    from utils.commons import get_optimizer
    from models.transformer_lm.transformer_lm import TransformerLM
    g = torch.Generator().manual_seed(1)
    x = torch.randint(2, 514, (8, 258), generator=g)
    x[:, 0] = 1
    x[:, -1] = 0
    lens = torch.full((8,), 257)
    x, lens = x.to(DEV), lens.to(DEV)
    arms = {}
    keep = []
    with tempfile.TemporaryDirectory() as tmp:
        build(tmp)                                                       # writes the throw-away VQ-VAE run the LM configs point at
        for name in ("fp32", "bf16"):
            cfg = C.load(os.path.join(ROOT, "speech-masters-thesis_amd", "configs/models",
                                      "transformer_lm.yaml" if name == "fp32" else "transformer_lm_bf16.yaml"))
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


def resources():
    """VGPR / AGPR / LDS figures of the kernels as the compiler reports them (a compile of csrc/lm_linear.hip with
    -Rpass-analysis=kernel-resource-usage, nothing kept); empty where there is no hipcc."""
    import re
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "speech-masters-thesis_amd", "csrc", "lm_linear.hip")
    if not os.path.exists(hipcc):
        return []
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=on", "-Rpass-analysis=kernel-resource-usage",
                              "-c", src, "-o", os.path.join(tmp, "x.o")], capture_output=True, text=True).stderr
    lines, cur = [], None
    for m in re.finditer(r"remark: +(Function Name|VGPRs|AGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", err):
        key, val = m.groups()
        if key == "Function Name":
            cur = [val]
            lines.append(cur)
        elif cur is not None:
            cur.append(f"{key} {val}")
    return ["  " + ", ".join(c) for c in lines]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_linear_micro.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--kernel-trace", help="a rocprofv3 --kernel-trace CSV of --trace-workload: add the kernel-time table to the output")
    ap.add_argument("--trace-workload", action="store_true", help="only issue 20 calls of every shape and phase in bf16 (for a kernel trace)")
    args = ap.parse_args()
    if args.trace_workload:
        for _, n_in, n_out in SHAPES:
            bench_shape(n_in, n_out, 4, dtypes=("bf16",))
        torch.cuda.synchronize()
        return
    lines = [f"tools/bench_lm_linear.py: rows = {ROWS}, HIP events, median of {WINDOWS} alternating windows of {args.reps} calls, one process",
             f"{torch.cuda.get_device_name(0)}; bf16 = smt_amd.lm.linear (csrc/lm_linear.hip), fp32 = torch.nn.functional.linear and its autograd",
             "", "call times (device events around eager calls; they include the host's issue rate where the kernel is shorter):",
             f"{'shape':<11}{'n_in':>5}{'n_out':>6}  {'phase':<6}{'fp32 us':>9}{'bf16 us':>9}{'bf16/fp32':>10}{'bf16 TFLOP/s':>13}{'of 2.5 PF':>10}"]
    for name, n_in, n_out in SHAPES:
        res = bench_shape(n_in, n_out, args.reps)
        flops = 2.0 * ROWS * n_in * n_out
        for phase, t in res.items():
            tf = flops / (t["bf16"] * 1e-3) * 1e-12
            lines.append(f"{name:<11}{n_in:>5}{n_out:>6}  {phase:<6}{t['fp32'] * 1e3:>9.1f}{t['bf16'] * 1e3:>9.1f}{t['bf16'] / t['fp32']:>10.2f}"
                         f"{tf:>13.1f}{100 * tf / PEAK_BF16_TFLOPS:>9.1f}%")
        print("\n".join(lines[-3:]), flush=True)
    if not args.no_step:
        t = bench_step(args.steps)
        lines += ["", f"eager train step, shipped configuration, batch 8 x 258 (forward + backward + optimizer), median of {WINDOWS} windows of {args.steps} steps:",
                  f"  fp32 {t['fp32']:.2f} ms   bf16 {t['bf16']:.2f} ms   bf16 / fp32 = {t['bf16'] / t['fp32']:.3f}"]
        print("\n".join(lines[-2:]), flush=True)
    if args.kernel_trace:
        lines += ["", "kernel times (rocprofv3 --kernel-trace of `--trace-workload`, a run of its own; median of 23 launches; TF = TFLOP/s):"]
        lines += kernel_table(args.kernel_trace)
    res_lines = resources()
    if res_lines:
        lines += ["", "kernel resources (hipcc -Rpass-analysis=kernel-resource-usage on csrc/lm_linear.hip):"] + res_lines
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
