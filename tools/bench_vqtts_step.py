"""Stand-alone timing of the assembled VQTTS at the shape of configs/models/vqtts.yaml + configs/datasets/synthetic_vqtts.yaml
(batch 32, 145,408 samples = 568 frames per clip, at most 160 tokens, synthetic token + audio pairs):

  * the train step (forward + backward + AdamW) in ms, HIP events over `--steps` steps after `--warmup`, and, in a separate
    pass with smt_amd.profiler on, the forward split by stage (the `vqtts:*` regions of VQTTS.forward);
  * `VQTTS.infer` on the batch's token ids (the one host read of the lengths included);
  * `smt_amd.vqtts.emit_codes` against the torch chain it replaces (synthesize_codes -> F.embedding -> length mask) at
    B * Tq = 32 * 568 and 32 * 18,176, D = 128, the two alternating in one loop; algorithmic bytes = 2 * B * Tq * D * 4.

Writes the report to --out (default profiles/vqtts_step.txt) and prints one JSON line.  No pass/fail threshold."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "speech-masters-thesis_amd")
sys.path.insert(0, PKG)
from smt_amd import profiler, vqtts  # noqa: E402
from utils import config as C  # noqa: E402
from utils.commons import get_model, get_optimizer, to_device  # noqa: E402


def timed(fn, iters):
    """ms per call by HIP events around `iters` calls."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def bench_emit(batch, tq, d, n_vocab, l_bins, iters, seed):
    from models.vqtts import Bottleneck, CodePredictor
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    bott = Bottleneck(n_vocab, l_bins, d, 0.99, 1.0).to(dev)
    bott.k.copy_(torch.randn(n_vocab * l_bins, d, generator=g))
    head = CodePredictor(d, l_bins)
    tx = 160
    x_id = torch.randint(0, n_vocab, (batch, tx), generator=g).to(dev)
    idx = torch.sort(torch.randint(0, tx, (batch, tq), generator=g), dim=1)[0].to(torch.int32).to(dev)      # monotonic, as a path is
    pred = torch.randint(0, l_bins, (batch, tq), generator=g, dtype=torch.int32).to(dev)
    q_lens = torch.randint(tq // 2, tq + 1, (batch,), generator=g, dtype=torch.int32).to(dev)

    def kernel():
        return vqtts.emit_codes(pred, x_id, idx, q_lens, bott.k, n_vocab, l_bins)[0]

    def chain():
        keep = torch.arange(tq, device=dev)[None, :] < q_lens[:, None]
        return bott.decode(head.synthesize_codes(pred, x_id, idx)) * keep[..., None]
    assert torch.equal(kernel(), chain())                          # the same result before either is timed
    for _ in range(5):
        kernel(); chain()
    torch.cuda.synchronize()
    ms = {"kernel": [], "chain": []}
    for _ in range(5):                                             # alternate, five windows each: the spread is part of the result
        ms["kernel"].append(timed(kernel, iters))
        ms["chain"].append(timed(chain, iters))
    nbytes = 2.0 * batch * tq * d * 4
    return {"batch": batch, "t_q": tq, "dim": d, "alg_bytes": nbytes,
            "kernel_us": [round(v * 1e3, 2) for v in ms["kernel"]], "chain_us": [round(v * 1e3, 2) for v in ms["chain"]],
            "kernel_gbs": round(nbytes / (min(ms["kernel"]) * 1e-3) * 1e-9, 1), "chain_gbs": round(nbytes / (min(ms["chain"]) * 1e-3) * 1e-9, 1),
            "speedup_min_over_min": round(min(ms["chain"]) / min(ms["kernel"]), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--emit_iters", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip_step", action="store_true", help="only the emission micro-benchmark")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "vqtts_step.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_vqtts_step measures on MI355X; no GPU is visible")
    device = torch.device("cuda")
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/vqtts.yaml")), C.load(os.path.join(PKG, "configs/datasets/synthetic_vqtts.yaml")),
                  C.create({"train": {"batch_size": args.batch_size, "n_gpus": 1, "ema": False}}))
    out = {"tool": "bench_vqtts_step", "config": "configs/models/vqtts.yaml + configs/datasets/synthetic_vqtts.yaml",
           "batch_size": args.batch_size, "steps": args.steps, "warmup": args.warmup}
    lines = []
    if not args.skip_step:
        torch.manual_seed(args.seed)
        model, _ = get_model(cfg, device)
        opt, sched = get_optimizer(cfg, model)
        from datasets.synthetic import SyntheticTTSAudio
        data = SyntheticTTSAudio(cfg, "train")
        batch = to_device(SyntheticTTSAudio.collate([data[i] for i in range(args.batch_size)]), device)
        out.update(samples=int(batch[4].shape[-1]), frames=int(batch[4].shape[-1]) // model.stride, t_x=int(batch[0].shape[1]),
                   tokens=int(batch[1].sum()), parameters=sum(p.numel() for p in model.parameters()),
                   codebook_rows=int(model.quant_bottleneck.k.shape[0]))

        def step():
            opt.zero_grad()
            loss_dict, _ = model.supervised_step(batch)
            loss_dict["loss"].backward()
            opt.step(); sched.step()
            return loss_dict
        model.train()
        for _ in range(args.warmup):
            loss_dict = step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss_dict["loss"])), "the warm-up step's loss is not finite"
        windows = [timed(step, args.steps) for _ in range(3)]
        out["train_step_ms"] = [round(v, 2) for v in windows]
        out["loss_after"] = round(float(step()["loss"]), 4)
        # the forward by stage, in a pass of its own (the events serialise nothing, but they are not free)
        profiler.reset(); profiler.enable(True)
        for _ in range(args.steps):
            step()
        rows = [r for r in profiler.summary() if r["name"].startswith("vqtts:")]
        profiler.enable(False); profiler.reset()
        out["forward_stages_ms"] = {r["name"][len("vqtts:"):]: round(r["avg_us"] * 1e-3, 3) for r in rows}
        # synthesis
        model.eval()
        x, x_lens = batch[0], batch[1]
        for _ in range(args.warmup):
            wave, wave_lengths = model.infer(x, x_lens)
        torch.cuda.synchronize()
        infer = [timed(lambda: model.infer(x, x_lens), args.steps) for _ in range(3)]
        out["infer_ms"] = [round(v, 2) for v in infer]
        out["infer_frames"] = int(wave_lengths.sum()) // model.stride
        out["infer_t_out"] = int(wave.shape[1]) // model.stride
        lines += [f"train step (fwd + bwd + AdamW), B = {args.batch_size}, {out['samples']} samples = {out['frames']} frames, Tx = {out['t_x']} "
                  f"({out['tokens']} tokens), {out['parameters'] / 1e6:.2f} M parameters, codebook {out['codebook_rows']} x {cfg.model.emb_width}:",
                  f"  ms per step, three windows of {args.steps} steps after {args.warmup} warm-up steps: {out['train_step_ms']}",
                  "forward by stage (smt_amd.profiler regions, ms, mean over the profiled steps):"]
        lines += [f"  {k:<14} {v:9.3f}" for k, v in out["forward_stages_ms"].items()]
        lines += [f"  {'sum':<14} {sum(out['forward_stages_ms'].values()):9.3f}",
                  f"infer (untrained duration predictor: {out['infer_frames']} frames in all, T_out = {out['infer_t_out']}), ms per call, three windows: "
                  f"{out['infer_ms']}"]
    out["emit"] = [bench_emit(32, tq, 128, 149, 512, args.emit_iters, args.seed) for tq in (568, 18176)]
    lines.append("emit_codes against the torch chain it replaces (us per call, five alternating windows each; GB/s = 2 B Tq D 4 bytes over the best window):")
    for r in out["emit"]:
        lines += [f"  B * Tq = {r['batch']} * {r['t_q']}, D = {r['dim']} ({r['alg_bytes'] / 1e6:.1f} MB):",
                  f"    smt_vqtts_emit {r['kernel_us']}  -> {r['kernel_gbs']} GB/s",
                  f"    torch chain    {r['chain_us']}  -> {r['chain_gbs']} GB/s   (chain / kernel, best over best: {r['speedup_min_over_min']})"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
