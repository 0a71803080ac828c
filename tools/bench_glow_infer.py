"""Stand-alone timing of GlowTTS synthesis (`GlowTTS.infer`) at the configs/models/glow_tts.yaml widths (hidden 192, 6 encoder
layers, 12 flow blocks of 4 WN layers, 80 mels), batch 1 and batch 32, with the token lengths of configs/datasets/synthetic_tts.yaml
(uniform in [max_tokens / 2, max_tokens]) and a duration-predictor bias that gives about frames_per_token frames per token.
Prints one JSON line: ms per call (HIP events over `iters` calls, the one host read of the lengths included), mel frames per
second, and the device launches of one call (torch profiler), split into libsmt_hip.so kernels and the rest."""
import argparse
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "speech-masters-thesis_amd")
sys.path.insert(0, PKG)
from utils import config as C  # noqa: E402
from utils.commons import get_model  # noqa: E402


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(dev), sum(1 for e in dev if "smt" in e.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    device = torch.device("cuda")
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/glow_tts.yaml")), C.load(os.path.join(PKG, "configs/datasets/synthetic_tts.yaml")),
                  C.create({"train": {"batch_size": 1, "n_gpus": 1}}))
    torch.manual_seed(args.seed)
    model, _ = get_model(cfg, device)
    ds = cfg.dataset
    with torch.no_grad():
        model.encoder.proj_w.proj.bias.fill_(math.log(ds.frames_per_token - 0.5))
    model.eval()
    g = torch.Generator().manual_seed(args.seed)
    n_vocab = model.encoder.emb.num_embeddings
    out = {"tool": "bench_glow_infer", "config": "configs/models/glow_tts.yaml", "iters": args.iters, "runs": []}
    for b in args.batches:
        lens = torch.randint(ds.max_tokens // 2, ds.max_tokens + 1, (b,), generator=g)
        x = torch.randint(1, n_vocab, (b, int(lens.max())), generator=g).to(device)
        lens_d = lens.to(device)

        def call():
            return model.infer(x, lens_d)
        for _ in range(3):
            yh, y_len = call()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            call()
        end.record()
        torch.cuda.synchronize()
        ms = start.elapsed_time(end) / args.iters
        frames = int(y_len.sum())
        total, native = launches(call)
        out["runs"].append({"batch": b, "tokens": int(lens.sum()), "frames": frames, "t_out": int(yh.shape[2]), "ms_per_call": round(ms, 3),
                            "mel_frames_per_s": round(frames / (ms / 1e3), 1), "launches_per_call": total,
                            "native_launches_per_call": native})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
