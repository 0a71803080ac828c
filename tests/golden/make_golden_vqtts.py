#!/usr/bin/env python3
"""Generate tests/golden/vqtts_bottleneck.npz by running THE REFERENCE's own grouped quantiser,
`models.vqtts.bottleneck.Bottleneck` (bottleneck.py:7-77 on top of models/vqvae/bottleneck.py:20-90), on CPU for three
training steps and one eval step.  The harness of make_golden.py is reused (its import sets up the paths, the working
directory and the stand-ins).  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vqtts.py

Nothing of the reference is changed.  It is called the way its own code needs: y_enc channels-first [B, C, Ty], x_id as
[B, 1, Tx] (what its `matmul(x_id, attn)` needs), attn a dense 0/1 path [B, Tx, Ty].  Its random draws are recorded, not
replaced: `_tile` and `torch.randperm` are wrapped so that the rows it selects (`y[randperm][:k_bins]`) can be replayed as
k_rand_init (init_k, from ALL rows) and k_rand (update_k, from the unmasked rows).

Stored per training step s (arrays channels-last, the layout of this repository): s{s}_y_enc [B, T, D], s{s}_x_id [B, Tx],
s{s}_attn [B, Tx, T], s{s}_align_idx [B, T] int32 (-1 = no token), s{s}_k_rand, s{s}_q_rel, s{s}_y_d, s{s}_commit,
s{s}_dy_enc = d(y_d.sum() + 3 commit)/d y_enc, s{s}_m_{fit,entropy,used_curr,usage,dk}, s{s}_k / k_sum / k_elem after the
step; s0_k_rand_init; the eval step as e_*.  The script ASSERTS that on every row of every step the reference's fp32 argmin
equals the float64 argmin over the group's codes, so index comparisons against this fixture leave out no row."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402  (REF first on sys.path, cwd = REF, stand-ins)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_VOCAB, L_BINS, D, B, TX, T = 6, 32, 64, 3, 7, 48
X_LENS, Y_LENS = (7, 5, 4), (48, 40, 29)
MU, THRESHOLD = 0.99, 1.0


def make_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    # the same per-channel +-3 offset at every step: encoder outputs share a large common component
    offset = 3.0 * (torch.randint(0, 2, (D,), generator=torch.Generator().manual_seed(99)).float() * 2 - 1)
    y_enc = 0.5 * torch.randn(B, T, D, generator=g) + offset
    x_id = torch.randint(0, N_VOCAB, (B, TX), generator=g)
    attn = torch.zeros(B, TX, T)
    align = torch.full((B, T), -1, dtype=torch.int32)
    for b in range(B):
        # random monotonic alignment: every token gets at least one frame
        cuts = torch.sort(torch.randperm(Y_LENS[b] - 1, generator=g)[:X_LENS[b] - 1] + 1).values.tolist()
        edges = [0] + cuts + [Y_LENS[b]]
        for i in range(X_LENS[b]):
            attn[b, i, edges[i]:edges[i + 1]] = 1.0
            align[b, edges[i]:edges[i + 1]] = i
    return y_enc, x_id, attn, align


def exact_q_rel(y_enc, x_id, align, k):
    """float64 argmin over the group's codes, lowest index on ties; masked rows search group 0."""
    rows = y_enc.reshape(-1, D).double().numpy()
    al = align.reshape(-1).numpy()
    tok = x_id.numpy()
    kk = k.double().numpy().reshape(N_VOCAB, L_BINS, D)
    out = np.zeros(rows.shape[0], dtype=np.int64)
    gap = np.inf
    for r in range(rows.shape[0]):
        g = tok[r // T, al[r]] if al[r] >= 0 else 0
        dist = ((rows[r][None, :] - kk[g]) ** 2).sum(-1)
        out[r] = int(np.argmin(dist))
        srt = np.sort(dist)
        gap = min(gap, srt[1] - srt[0])
    return out, gap


def main():
    from models.vqtts.bottleneck import Bottleneck
    model = Bottleneck(N_VOCAB, L_BINS, D, MU, THRESHOLD)
    draws = []
    tile = model._tile
    randperm = torch.randperm

    def capture_tile(x):
        y = tile(x)
        draws.append([y.detach().clone(), None])
        return y

    def capture_randperm(n, *a, **k):
        p = randperm(n, *a, **k)
        if draws and draws[-1][1] is None and draws[-1][0].shape[0] == n:
            draws[-1][1] = p.clone()
        return p
    model._tile = capture_tile
    torch.randperm = capture_randperm
    out = dict(mu=np.float32(MU), threshold=np.float32(THRESHOLD), n_vocab=N_VOCAB, l_bins=L_BINS,
               x_lens=np.asarray(X_LENS), y_lens=np.asarray(Y_LENS))
    try:
        torch.manual_seed(1234)
        for s in range(4):
            train = s < 3
            tag = f"s{s}" if train else "e"
            model.train(train)
            y_enc, x_id, attn, align = make_inputs(100 + s)
            y_cf = y_enc.permute(0, 2, 1).contiguous().requires_grad_(True)
            del draws[:]
            k_before = None if (train and not model.init) else model.k.clone()
            q_rel, y_d, commit, metrics = model(y_cf, x_id.reshape(B, 1, TX), attn)
            (y_d.sum() + 3.0 * commit).backward()
            picked = [y[p][:model.k_bins] for y, p in draws]
            if train and s == 0:
                assert len(picked) == 2
                out["s0_k_rand_init"] = picked[0]
                k_before = picked[0]
            assert len(picked) == ((2 if s == 0 else 1) if train else 0)
            exact, gap = exact_q_rel(y_enc, x_id, align, k_before)
            assert np.array_equal(q_rel.reshape(-1).numpy(), exact), f"step {tag}: fp32 argmin != float64 argmin"
            print(f"  step {tag}: {exact.size} rows, reference q_rel == float64 argmin on all; smallest best/runner-up gap {gap:.2e}; "
                  f"commit {commit.item():.5f} fit {metrics['fit'].item():.5f}")
            out.update({f"{tag}_y_enc": y_enc, f"{tag}_x_id": x_id, f"{tag}_attn": attn.to(torch.uint8), f"{tag}_align_idx": align,
                        f"{tag}_q_rel": q_rel, f"{tag}_y_d": y_d.detach().permute(0, 2, 1).contiguous(),
                        f"{tag}_commit": commit.detach(), f"{tag}_dy_enc": y_cf.grad.permute(0, 2, 1).contiguous(),
                        f"{tag}_m_fit": metrics["fit"]})
            if train:
                out[f"{tag}_k_rand"] = picked[-1]
                for mk in ("entropy", "used_curr", "usage", "dk"):
                    out[f"{tag}_m_{mk}"] = torch.as_tensor(metrics[mk]).float()
                out.update({f"{tag}_k": model.k.clone(), f"{tag}_k_sum": model.k_sum.clone(), f"{tag}_k_elem": model.k_elem.clone()})
            else:
                assert set(metrics) == {"fit"}
    finally:
        torch.randperm = randperm
    mg.save("vqtts_bottleneck", **out)
    print("  size:", os.path.getsize(os.path.join(mg.OUT, "vqtts_bottleneck.npz")), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
