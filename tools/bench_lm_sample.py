#!/usr/bin/env python3
"""Stand-alone timing of `TransformerLM.sample` at the configs/models/transformer_lm.yaml widths (12 layers, d 512, 16 heads,
ff 2048, vocab 512; random-init weights), batch 4 and 32, 256 and 1024 codes, three ways:

    full     sample(causal=False): the whole prefix through all layers for every new token (the reference's loop)
    cached   sample(causal=True): one token per step against the key/value cache (csrc/lm_decode.hip), launches issued by the host
    graphed  sample(causal=True, graph=True): the same step captured once and replayed

Every call ends with the VQ-VAE decoder (`reconstruct`), as a user's call does.  Per variant: seconds per call (host clock
around calls that end in a device synchronise; one warm-up call, `--iters` timed ones, the median and the spread) and codes
per second.  For the cached paths also the bytes a step cannot avoid -- the 12 layers' projection weights, the classifier
weight, and the keys and values of the positions so far, 2 * layers * batch * d * 4 * (t + 1), averaged over t -- and what
fraction of the copy rate this project quotes for the device (0.79 of 8 TB/s) moving that floor in the measured step time comes to.
A second table times the two streaming kernels alone.  A third compares handing over a prompt of P codes by `prefill` (one
batched pass, keys / values copied into the cache) with P `push`es (one decoding step per prompt token), a fourth the graphed
`sample` and the sampler launch alone with and without the top-k / top-p filter.  Prints the tables and one JSON line.

    python tools/bench_lm_sample.py [--iters 3] [--full_iters 2] [--batches 4 32] [--steps 256 1024]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "speech-masters-thesis_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

COPY_RATE = 0.79 * 8e12          # bytes/s: the device copy rate VERDICT.md item 10 quotes


def timed(fn, iters):
    fn()                                                       # warm-up: code objects, allocator, library heuristics
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def step_floor_bytes(model, batch, n_steps):
    """Bytes one cached step must move, averaged over the steps of a call: weights once, cache rows 0..t once."""
    layers = model.transformer.layers
    weights = sum(p.numel() for layer in layers for p in (layer.self_attn.in_proj_weight, layer.self_attn.out_proj.weight,
                                                          layer.linear1.weight, layer.linear2.weight)) * 4
    weights += model.classifier.weight.numel() * 4
    kv = 2 * len(layers) * batch * model.d_model * 4 * (n_steps + 1) / 2.0
    return weights + kv


def kernel_table(model, batches, l_max=1024, reps=20):
    """The two streaming kernels alone, cycling over the 12 layers' own weights / caches as a decoding step does (HIP events
    over `reps` replays of one captured pass, the gaps between its launches included): us per launch and bytes per second of the weight matrix resp. the visible cache rows."""
    from smt_amd import lm as K
    layers = model.transformer.layers
    rows = []

    def events(fn):
        fn()                                                   # warm-up, then one pass over the layers captured as a graph:
        torch.cuda.synchronize()                               # the host's launch cost (several us per call) stays out
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        graph.replay()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            graph.replay()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) * 1e-3 / (reps * len(layers))

    print(f"{'kernel':>28} {'batch':>5} {'us/launch':>10} {'GB/s':>8}")
    for b in batches:
        st = model.new_decode_state(b, l_max, "cuda")
        st.kv.normal_()
        st.qkv.normal_()
        st.h.normal_()
        st.f.normal_()
        cases = [("in_proj 512->1536", lambda l: K.decode_linear(st.h, l.self_attn.in_proj_weight, l.self_attn.in_proj_bias, st.qkv), 1536 * 512 * 4),
                 ("out_proj 512->512", lambda l: K.decode_linear(st.h, l.self_attn.out_proj.weight, None, st.a), 512 * 512 * 4),
                 ("linear1 512->2048", lambda l: K.decode_linear(st.h, l.linear1.weight, l.linear1.bias, st.f, relu=True), 2048 * 512 * 4),
                 ("linear2 2048->512", lambda l: K.decode_linear(st.f, l.linear2.weight, None, st.a), 2048 * 512 * 4)]
        for name, call, nbytes in cases:
            t = events(lambda: [call(l) for l in layers])
            rows.append({"kernel": name, "batch": b, "us": t * 1e6, "bytes": nbytes, "bytes_per_s": nbytes / t})
            print(f"{name:>28} {b:>5} {t * 1e6:10.2f} {nbytes / t / 1e9:8.0f}", flush=True)
        for pos in (255, l_max - 1):
            nbytes = 2 * (pos + 1) * 128 * b * layers[0].self_attn.num_heads
            t = events(lambda: [K.decode_attention(st.qkv, st.kv[i, 0], st.kv[i, 1], st.ctx, st.attn_ws, pos=pos) for i in range(len(layers))])
            rows.append({"kernel": f"attention pos {pos}", "batch": b, "us": t * 1e6, "bytes": nbytes, "bytes_per_s": nbytes / t})
            print(f"{'attention, pos ' + str(pos):>28} {b:>5} {t * 1e6:10.2f} {nbytes / t / 1e9:8.0f}", flush=True)
    return rows


def prefill_table(model, batches, prompts=(64, 256), iters=5):
    """`prefill` of P codes against P steps of `_decode_logits` + `push` (what `step_logits` / `push` issue), host clock around
    calls that end in a device synchronise; the state is made once and rewound between calls."""
    rows = []
    vocab = model.classifier.out_features
    print(f"{'batch':>5} {'prompt':>6} {'prefill ms':>11} {'pushes ms':>10} {'ratio':>7}")
    for b in batches:
        for p in prompts:
            codes = torch.randint(0, vocab, (b, p), generator=torch.Generator().manual_seed(p + b)).cuda()
            st = model.new_decode_state(b, p + 1, "cuda")

            def rewind():
                st.pos = 0
                st.pos_dev.zero_()

            def by_prefill():
                rewind()
                model.prefill(st, codes)

            def by_pushes():
                rewind()
                for t in range(p):
                    model._decode_logits(st)
                    st.push(codes[:, t] + model.OFFSET)

            t_pre, t_push = statistics.median(timed(by_prefill, iters)), statistics.median(timed(by_pushes, iters))
            rows.append({"batch": b, "prompt": p, "prefill_s": t_pre, "pushes_s": t_push})
            print(f"{b:>5} {p:>6} {t_pre * 1e3:11.3f} {t_push * 1e3:10.3f} {t_push / t_pre:7.1f}", flush=True)
    return rows


def filter_table(model, batches, n_steps=256, iters=3, reps=20, launches=50):
    """Graphed `sample` of n_steps codes, and `launches` sampler launches captured as one graph (HIP events over `reps` replays),
    without a filter and with top_k = 64, top_p = 0.95 and both."""
    from smt_amd import lm as K
    rows = []
    filters = [("none", None, None), ("top_k 64", 64, None), ("top_p 0.95", None, 0.95), ("top_k 64, top_p 0.95", 64, 0.95)]
    print(f"{'batch':>5} {'filter':>22} {'us/step (graphed)':>18} {'us/sampler launch':>18}")
    for b in batches:
        u = torch.rand(n_steps, b, generator=torch.Generator().manual_seed(b)).cuda()
        st = model.new_decode_state(b, n_steps, "cuda", u)
        st.logits.normal_()
        for name, top_k, top_p in filters:
            ts = timed(lambda: model.sample(b, n_steps, "cuda", causal=True, uniforms=u, graph=True, top_k=top_k, top_p=top_p), iters)

            def draw():
                for _ in range(launches):
                    if top_k is None and top_p is None:
                        K.decode_sample(st.logits, st.uniforms, st.tokens, st.codes, 1.0, pos=0)
                    else:
                        K.decode_sample_filtered(st.logits, st.uniforms, st.tokens, st.codes, 1.0, top_k, top_p, st.kept, pos=0)

            draw()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                draw()
            graph.replay()
            torch.cuda.synchronize()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                graph.replay()
            end.record()
            torch.cuda.synchronize()
            t_launch = start.elapsed_time(end) * 1e-3 / (reps * launches)
            rows.append({"batch": b, "filter": name, "n_steps": n_steps, "us_per_step": statistics.median(ts) / n_steps * 1e6,
                         "sampler_us": t_launch * 1e6})
            print(f"{b:>5} {name:>22} {rows[-1]['us_per_step']:18.1f} {rows[-1]['sampler_us']:18.2f}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--full_iters", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--steps", type=int, nargs="+", default=[256, 1024])
    args = ap.parse_args()
    from bench_lm import build
    with tempfile.TemporaryDirectory() as tmp:
        model, _, _ = build(tmp)
    model.eval()
    runs = []
    print(f"{'batch':>5} {'codes':>5} {'variant':>8} {'s/call':>9} {'spread':>7} {'codes/s':>10} {'us/step':>9} {'floor MB':>9} {'of copy rate':>12}")
    for b in args.batches:
        for n in args.steps:
            u = torch.rand(n, b, generator=torch.Generator().manual_seed(n + b)).cuda()
            variants = (("full", args.full_iters, lambda: model.sample(b, n, "cuda")),
                        ("cached", args.iters, lambda: model.sample(b, n, "cuda", causal=True, uniforms=u)),
                        ("graphed", args.iters, lambda: model.sample(b, n, "cuda", causal=True, uniforms=u, graph=True)))
            for name, iters, fn in variants:
                torch.manual_seed(0)
                ts = timed(fn, iters)
                med = statistics.median(ts)
                row = {"batch": b, "n_steps": n, "variant": name, "s_per_call": med, "min_s": min(ts), "max_s": max(ts), "calls": iters,
                       "codes_per_s": b * n / med, "us_per_step": med / n * 1e6}
                floor, frac = "", ""
                if name != "full":
                    row["floor_bytes_per_step"] = step_floor_bytes(model, b, n)
                    row["fraction_of_copy_rate"] = row["floor_bytes_per_step"] / (med / n) / COPY_RATE
                    floor, frac = f"{row['floor_bytes_per_step'] / 1e6:9.1f}", f"{row['fraction_of_copy_rate']:12.3f}"
                runs.append(row)
                print(f"{b:>5} {n:>5} {name:>8} {med:9.4f} {(max(ts) - min(ts)) / med:7.1%} {row['codes_per_s']:10.0f} {row['us_per_step']:9.1f} "
                      f"{floor:>9} {frac:>12}", flush=True)
    with torch.no_grad():
        kernels = kernel_table(model, args.batches)
        prefill = prefill_table(model, args.batches)
        filtered = filter_table(model, args.batches)
    print(json.dumps({"tool": "bench_lm_sample", "config": "transformer_lm.yaml (12 x d512 h16 ff2048, vocab 512), random init",
                      "copy_rate_bytes_per_s": COPY_RATE, "runs": runs, "kernels": kernels, "prefill": prefill, "filtered": filtered}))


if __name__ == "__main__":
    main()
