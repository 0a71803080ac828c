#!/usr/bin/env python3
"""The pre-norm / GELU options of the TransformerLM (model.norm_first, model.activation) in ONE process: the eager train step
of the shipped configuration (12 layers, d 512, batch 8 x 258) in the four combinations, and the call times of the two kernel
pairs the options add (smt_amd.lm.residual_layer_norm, bias_gelu_dropout) beside the ones they stand in for (add_layer_norm,
bias_relu_dropout_) at rows = 8 x 258 = 2064, dropout 0.1.

HIP events; every figure is the median of five windows, and the windows of the arms alternate.  Random operands.  Reads
nothing outside the repository.  The post-norm + ReLU arm issues exactly the launches the model issued before it had the two
keys, so the ratios to it are ratios to that step, from the same run.  The per-kernel figures are CALL times: device events
around a run of eager calls, so where the kernel is shorter than the host takes to issue it they show the host.

    python tools/bench_lm_prenorm.py [--out profiles/lm_prenorm_micro.txt] [--reps 50] [--steps 10]
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "speech-masters-thesis_amd"))

import torch  # noqa: E402

from tools.bench_lm_linear import DEV, ROWS, WINDOWS, alternate  # noqa: E402

COMBOS = [("post-norm relu", False, "relu"), ("post-norm gelu", False, "gelu"), ("pre-norm relu", True, "relu"), ("pre-norm gelu", True, "gelu")]
D_MODEL, D_FF, P = 512, 2048, 0.1


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
    arms, keep = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        build(tmp)                                                       # writes the throw-away VQ-VAE run the LM configs point at
        for name, norm_first, activation in COMBOS:
            cfg = C.load(os.path.join(ROOT, "speech-masters-thesis_amd", "configs/models", "transformer_lm.yaml"))
            cfg.model.norm_first, cfg.model.activation = norm_first, activation
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


def bench_kernels(reps):
    """{pair: {phase: {arm: ms}}}: forward calls under no_grad, backward calls through autograd on a kept graph."""
    from smt_amd import lm as K
    g = torch.Generator().manual_seed(2)
    drop = K.Drop(P, True, 3, 5)
    out = {}

    x, h = torch.randn(ROWS, D_MODEL, generator=g).to(DEV), torch.randn(ROWS, D_MODEL, generator=g).to(DEV)
    dy, ds = torch.randn(ROWS, D_MODEL, generator=g).to(DEV), torch.randn(ROWS, D_MODEL, generator=g).to(DEV)
    gamma, beta, hb = (torch.nn.Parameter(torch.ones(D_MODEL, device=DEV)), torch.nn.Parameter(torch.zeros(D_MODEL, device=DEV)),
                       torch.nn.Parameter(torch.zeros(D_MODEL, device=DEV)))

    def add_ln_fwd():
        with torch.no_grad():
            K.add_layer_norm(x, h, gamma, beta, 1e-5, drop, h_bias=hb)

    def res_ln_fwd():
        with torch.no_grad():
            K.residual_layer_norm(x, h, gamma, beta, 1e-5, drop, h_bias=hb)

    xg, hg = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    y0 = K.add_layer_norm(xg, hg, gamma, beta, 1e-5, drop, h_bias=hb)
    s1, y1 = K.residual_layer_norm(xg, hg, gamma, beta, 1e-5, drop, h_bias=hb)
    wanted = [xg, hg, gamma, beta, hb]
    out["add + LayerNorm [2064, 512]"] = {
        "fwd": alternate({"add_ln": add_ln_fwd, "res_ln": res_ln_fwd}, reps),
        "bwd": alternate({"add_ln": lambda: torch.autograd.grad(y0, wanted, dy, retain_graph=True),
                          "res_ln": lambda: torch.autograd.grad([s1, y1], wanted, [ds, dy], retain_graph=True)}, reps)}

    f = torch.randn(ROWS, D_FF, generator=g).to(DEV)
    da = torch.randn(ROWS, D_FF, generator=g).to(DEV)
    bias = torch.nn.Parameter(torch.zeros(D_FF, device=DEV))
    scratch = f.clone()

    def relu_fwd():                                                       # in place: on a scratch copy that is never reset (same traffic)
        with torch.no_grad():
            K.bias_relu_dropout_(scratch, bias, drop)

    def gelu_fwd():
        with torch.no_grad():
            K.bias_gelu_dropout(f, bias, drop)

    fg = f.clone().requires_grad_(True)
    a0 = K.bias_relu_dropout_(fg * 1.0, bias, drop)
    a1 = K.bias_gelu_dropout(fg, bias, drop)
    out["bias + activation + dropout [2064, 2048]"] = {
        "fwd": alternate({"bias_relu": relu_fwd, "bias_gelu": gelu_fwd}, reps),
        "bwd": alternate({"bias_relu": lambda: torch.autograd.grad(a0, [fg, bias], da, retain_graph=True),
                          "bias_gelu": lambda: torch.autograd.grad(a1, [fg, bias], da, retain_graph=True)}, reps)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_prenorm_micro.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    lines = [f"tools/bench_lm_prenorm.py: HIP events, median of {WINDOWS} alternating windows, one process",
             f"{torch.cuda.get_device_name(0)}", "",
             f"call times at rows = {ROWS}, dropout {P} ({args.reps} eager calls per window; they include the host's issue rate where the kernel is shorter):",
             f"{'kernel pair':<44}{'phase':<6}{'existing us':>12}{'new us':>9}{'new / existing':>16}"]
    for pair, phases in bench_kernels(args.reps).items():
        for phase, t in phases.items():
            (old_name, old), (new_name, new) = t.items()
            lines.append(f"{pair:<44}{phase:<6}{old * 1e3:>12.1f}{new * 1e3:>9.1f}{new / old:>16.2f}   ({old_name} -> {new_name})")
    print("\n".join(lines), flush=True)
    t = bench_step(args.steps)
    base = t[COMBOS[0][0]]
    lines += ["", f"eager train step, shipped configuration, batch 8 x 258 (forward + backward + optimizer), {args.steps} steps per window:",
              f"{'layers':<18}{'ms':>8}{'/ post-norm relu':>18}"]
    lines += [f"{name:<18}{ms:>8.2f}{ms / base:>18.3f}" for name, ms in t.items()]
    print("\n".join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
