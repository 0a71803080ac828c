#!/usr/bin/env python3
"""Rotary positions of the TransformerLM (model.position: rotary) in ONE process:

  * the rope kernel (smt_amd.lm.rope -> smt_lm_rope) at batch 8 x 258 with 16 x 32 and 8 x 64 heads (d 512), in us and as a
    fraction of the copy rate: a device copy of the same bytes (the q and k thirds, 2 * B * L * 2 d * 4 bytes of traffic), timed
    in the same run;
  * the fused one-token attention (decode_attention(rope=table)) beside the entry without the rotation, at the same shapes and
    positions: the launches of one decoding step, which must not get more;
  * the eager train step of the shipped configuration (12 layers, d 512, batch 8 x 258) with and without the key.

HIP events; every figure is the median of five windows, and the windows of the arms alternate.  Random operands.  Reads nothing
outside the repository.  The arm without the key issues exactly the launches the model issued before it had the key, so the
ratios to it are ratios to that code, from the same run.  The per-kernel figures are CALL times: device events around a run of
eager calls, so where the kernel is shorter than the host takes to issue it they show the host.

    python tools/bench_lm_rope.py [--out profiles/lm_rope_micro.txt] [--reps 200] [--steps 10]
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "speech-masters-thesis_amd"))

import torch  # noqa: E402

from tools.bench_lm_linear import DEV, WINDOWS, alternate  # noqa: E402

BATCH, LEN, D_MODEL = 8, 258, 512
HEADS = [(16, 32), (8, 64)]
DECODE_BATCH, DECODE_LMAX = 8, 2048
DECODE_POS = [0, 257, 2047]


def bench_rope(reps):
    """{(heads, dh): {arm: ms}}: the in-place rotation, its inverse, and a copy of the same bytes."""
    from smt_amd import lm as K
    from smt_amd import native as N
    out = {}
    for heads, dh in HEADS:
        g = torch.Generator().manual_seed(heads)
        qkv = torch.randn(BATCH, LEN, 3 * D_MODEL, generator=g).to(DEV)
        table = K.rope_table(LEN, dh, device=DEV)
        src, dst = torch.randn(BATCH * LEN, 2 * D_MODEL, generator=g).to(DEV), torch.empty(BATCH * LEN, 2 * D_MODEL, device=DEV)

        def fwd(qkv=qkv, table=table, heads=heads):
            with torch.no_grad():
                K.rope(qkv, table, heads)

        def inv(qkv=qkv, table=table, heads=heads, dh=dh):
            N.check(N.lib().smt_lm_rope(N.ptr(qkv), N.ptr(table), BATCH, LEN, heads, dh, LEN, 0, 1, N.stream_ptr()), "smt_lm_rope")

        out[(heads, dh)] = alternate({"rope": fwd, "inverse": inv, "copy": lambda src=src, dst=dst: dst.copy_(src)}, reps)
    return out


def bench_decode(reps):
    """{(heads, dh, pos): {arm: ms}}: one layer's one-token attention with and without the rotation."""
    from smt_amd import lm as K
    out = {}
    for heads, dh in HEADS:
        g = torch.Generator().manual_seed(100 + heads)
        qkv = torch.randn(DECODE_BATCH, 3 * D_MODEL, generator=g).to(DEV)
        kc = torch.randn(DECODE_BATCH, heads, DECODE_LMAX, dh, generator=g).to(DEV)
        vc = torch.randn(DECODE_BATCH, heads, DECODE_LMAX, dh, generator=g).to(DEV)
        ctx = torch.empty(DECODE_BATCH, D_MODEL, device=DEV)
        ws = K.decode_attention_workspace(DECODE_BATCH, heads, DECODE_LMAX, DEV, head_dim=dh)
        table = K.rope_table(DECODE_LMAX, dh, device=DEV)
        for pos in DECODE_POS:
            pos_dev = torch.tensor([pos], dtype=torch.int32, device=DEV)       # the decoding loop's form: the position on the device
            arms = {"hd": lambda pos_dev=pos_dev: K.decode_attention(qkv, kc, vc, ctx, ws, 0, pos_dev),
                    "rope": lambda pos_dev=pos_dev: K.decode_attention(qkv, kc, vc, ctx, ws, 0, pos_dev, rope=table)}
            out[(heads, dh, pos)] = alternate(arms, reps)
    return out


def bench_step(steps):
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
        for name, base in (("sinusoidal (no key)", "transformer_lm.yaml"), ("rotary", "transformer_lm_rope.yaml")):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_rope_micro.txt"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    nbytes = 2 * BATCH * LEN * 2 * D_MODEL * 4
    lines = [f"tools/bench_lm_rope.py: HIP events, median of {WINDOWS} alternating windows, one process",
             f"{torch.cuda.get_device_name(0)}", "",
             f"smt_lm_rope at {BATCH} x {LEN} x 3 * {D_MODEL}, in place on the q and k thirds: {nbytes / 1e6:.1f} MB of traffic per call "
             f"(arithmetic: 2 * B * L * 2 d * 4 bytes); call times, {args.reps} eager calls per window",
             f"{'heads x dh':<12}{'rope us':>9}{'inverse us':>12}{'copy us':>9}{'copy / rope':>13}"]
    for (heads, dh), t in bench_rope(args.reps).items():
        lines.append(f"{f'{heads} x {dh}':<12}{t['rope'] * 1e3:>9.1f}{t['inverse'] * 1e3:>12.1f}{t['copy'] * 1e3:>9.1f}{t['copy'] / t['rope']:>13.2f}")
    lines += ["", f"one-token attention, batch {DECODE_BATCH}, cache of {DECODE_LMAX} rows, position on the device; call times, {args.reps} eager calls per window",
              f"{'heads x dh':<12}{'pos':>6}{'_hd us':>9}{'_rope us':>10}{'rope / hd':>11}"]
    for (heads, dh, pos), t in bench_decode(args.reps).items():
        lines.append(f"{f'{heads} x {dh}':<12}{pos:>6}{t['hd'] * 1e3:>9.1f}{t['rope'] * 1e3:>10.1f}{t['rope'] / t['hd']:>11.3f}")
    print("\n".join(lines), flush=True)
    t = bench_step(args.steps)
    base = next(iter(t.values()))
    lines += ["", f"eager train step, shipped configuration, batch {BATCH} x {LEN} (forward + backward + optimizer), {args.steps} steps per window:",
              f"{'position':<22}{'ms':>8}{'/ sinusoidal':>14}"]
    lines += [f"{name:<22}{ms:>8.2f}{ms / base:>14.3f}" for name, ms in t.items()]
    print("\n".join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
