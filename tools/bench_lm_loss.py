"""Micro-benchmark of the TransformerLM's three training losses (loss_type ce | focal | mmi): forward + backward of the
native op (smt_amd.lm.cross_entropy / focal_loss / mmi_loss) beside the torch chain the model ran for focal and mmi before
these ops existed -- a boolean row selection, the loss class of models/transformer_lm/losses.py (F.cross_entropy for ce) on
the copy, a second argmax for the accuracy -- on the same device and the same logits.

Two shapes: [2064, 512] (the reference's batch: 8 x 258 tokens, vocabulary 512) and [16512, 512]; the last position of every
sequence and a tenth of the others are unscored.  HIP events on the launch stream; every line is warmed up, then the lines
of a shape take turns in ALTERNATING windows (five rounds of about 0.1 s per line); a line reports the median over the rounds
with the spread (min .. max) and the peak device memory it allocates above its inputs (its gradient included).  The torch
chain synchronises with the host inside every call (the selection's shape), which the windows include.

    python tools/bench_lm_loss.py [--out FILE]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-masters-thesis_amd"))
sys.path.insert(0, REPO)
from models.transformer_lm.losses import FocalLoss, MaximumMutualInformationLoss  # noqa: E402
from smt_amd import lm  # noqa: E402
from tools.bench_code_head import alternate, peak  # noqa: E402

V, GAMMA = 512, 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit(f"TransformerLM losses, forward + backward, V={V}, focal gamma {GAMMA:g}; {torch.cuda.get_device_name(0)}")
    modules = {"ce": F.cross_entropy, "focal": FocalLoss(gamma=GAMMA), "mmi": MaximumMutualInformationLoss(V)}
    natives = {"ce": lm.cross_entropy, "focal": lambda x, t: lm.focal_loss(x, t, GAMMA), "mmi": lm.mmi_loss}
    for rows in (2064, 16512):
        logits = (torch.randn(rows, V, generator=gen) * 3).cuda().requires_grad_(True)
        target = torch.randint(0, V, (rows,), generator=gen)
        target[torch.rand(rows, generator=gen) < 0.1] = -1
        target[257::258] = -1
        target = target.cuda()
        emit(f"--- [{rows}, {V}]: {int((target >= 0).sum())} scored rows; the logits are {4 * rows * V / 2 ** 20:.1f} MiB")

        def reset():
            logits.grad = None

        def native(kind):
            def fn():
                reset()
                loss, acc, _ = natives[kind](logits, target)
                loss.backward()
                return loss.detach(), acc
            return fn

        def chain(kind):
            def fn():
                reset()
                keep = target >= 0
                scored, tgt = logits[keep], target[keep]
                loss = modules[kind](scored, tgt)
                acc = (scored.argmax(1) == tgt).sum().float() / keep.sum()
                loss.backward()
                return loss.detach(), acc
            return fn

        fns = {}
        for kind in ("ce", "focal", "mmi"):
            fns[f"{kind:5s} native"] = native(kind)
            fns[f"{kind:5s} torch chain"] = chain(kind)
        times = alternate(fns, rounds=5, window_ms=100.0)
        med = {}
        for name, fn in fns.items():
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            emit(f"{name:18s}: {med[name]:8.4f} ms  (min {t[0]:.4f} .. max {t[-1]:.4f} over {len(t)} alternating windows)  "
                 f"peak {peak(fn, reset):7.2f} MiB")
        for kind in ("ce", "focal", "mmi"):
            (ln, an), (lt, at) = fns[f"{kind:5s} native"](), fns[f"{kind:5s} torch chain"]()
            emit(f"{kind:5s} torch chain / native: {med[f'{kind:5s} torch chain'] / med[f'{kind:5s} native']:.2f}; loss native {float(ln):.6f} "
                 f"chain {float(lt):.6f}, accuracy native {float(an):.6f} chain {float(at):.6f}")
        del logits, target
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
