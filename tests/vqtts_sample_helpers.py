"""Shared by the tests of the VQTTS code head's sampler (smt_vqtts_code_head_sample): a float64 host restatement of the
noise and the draw as include/smt_hip.h defines them ("VQTTS code head", sample), the derived error bound, and the
acceptance criterion every comparison uses.  numpy only; nothing here imports the product.

The restatement is exact up to the two logarithms of g = -log(-log(u)): the key, the counter hash and u are integer
arithmetic and one exact fp32 product.

Error bound (derived, not fitted).  A device logit is within e_r of the float64 one (section 13:
e_r = 2^-15 S_r + 2^-20 (1 + |lse_r|)).  g passes through two logf of at most 3 ulp each: the outer one leaves a relative
3 * 2^-23 of |g|, the inner one's relative error of -log(u) is an ABSOLUTE error of g of the same size (d log(x) = dx / x);
E_G = 2^-20 covers both with room: e_g = E_G (1 + |g|).  The fused multiply-add rounds once: 2^-23 |score| covers it and the
rounding of inv_T.  Together e_s = e_r * inv_T + e_g + 2^-23 |score|.
"""
import numpy as np

NOISE_ROW = 0x9E3779B1          # the header's multipliers: of the frame index in a row's key, of the bin in a logit's counter
NOISE_BIN = 0x85EBCA77
E_G = 2.0 ** -20                # the ONE place the noise's error constant lives
CHI2_999 = {1: 10.828, 2: 13.816, 3: 16.266, 4: 18.467, 5: 20.515, 6: 22.458, 7: 24.322, 8: 26.124, 9: 27.877, 10: 29.588,
            11: 31.264, 12: 32.909, 13: 34.528, 14: 36.123, 15: 37.697, 16: 39.252, 17: 40.790, 18: 42.312, 19: 43.820,
            20: 45.315, 31: 61.10}     # 99.9 % points of chi-square by degrees of freedom
_M32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    """MurmurHash3's finaliser on uint32 values (held in uint64 so that numpy does not warn on the wrap)."""
    h = np.asarray(h, dtype=np.uint64) & _M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    h ^= h >> np.uint64(16)
    return h


def row_keys(seeds, t_q):
    """key [B * t_q] of row r = b * t_q + j: fmix32(fmix32((uint32) seeds[b]) + (uint32) j * NOISE_ROW)."""
    s = np.asarray(seeds, dtype=np.int64).astype(np.uint64) & _M32
    j = np.arange(t_q, dtype=np.uint64)
    return fmix32((fmix32(s)[:, None] + j[None, :] * np.uint64(NOISE_ROW)) & _M32).reshape(-1)


def uniform(bits):
    """u = ((bits >> 9) + 0.5) * 2^-23 in float64 (every such value is an fp32 number strictly inside (0, 1))."""
    return ((np.asarray(bits, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(keys, bins):
    """g [rows, bins] float64 = -log(-log(u)) with bits = fmix32(key + (uint32) v * NOISE_BIN)."""
    v = np.arange(bins, dtype=np.uint64)
    bits = fmix32((np.asarray(keys, dtype=np.uint64)[:, None] + v[None, :] * np.uint64(NOISE_BIN)) & _M32)
    return -np.log(-np.log(uniform(bits)))


def device_scalars(temperature, min_p):
    """(inv_T, cut) as the fp32 values the device receives, held in float64."""
    cut = temperature * np.log(min_p) if min_p > 0 else -np.inf
    return float(np.float32(1.0 / temperature)), float(np.float32(cut))


def draw64(logits, seeds, t_q, temperature, min_p=0.0):
    """The draw in float64 on float64 logits [rows, bins]: dict of g, score, thr [rows], kept [rows, bins], pred [rows]
    (the kept bin with the highest score, lowest index on ties)."""
    inv_t, cut = device_scalars(temperature, min_p)
    g = gumbel(row_keys(seeds, t_q), logits.shape[1])
    score = logits * inv_t + g
    thr = logits.max(1) + cut
    kept = logits >= thr[:, None]
    pred = np.where(kept, score, -np.inf).argmax(1)
    return dict(g=g, score=score, thr=thr, kept=kept, pred=pred, inv_t=inv_t)


def row_bound(h, w, b, logits):
    """e_r [rows] of DESIGN.md section 13 from float64 arrays."""
    s = (np.abs(h) @ np.abs(w).T + np.abs(b)[None, :]).max(1)
    m = logits.max(1)
    lse = m + np.log(np.exp(logits - m[:, None]).sum(1))
    return 2.0 ** -15 * s + 2.0 ** -20 * (1 + np.abs(lse))


def check_draw(pred, n_kept, logits, e_r, seeds, t_q, temperature, min_p):
    """The acceptance criterion on EVERY row; returns the share of rows on which it pins exactly one admissible bin.
      * the device's k is possibly kept: l_k >= thr - 2 e_r;
      * score_k + e_s,k >= score_v - e_s,v for every surely kept v (l_v >= thr + 2 e_r);
      * n_kept (if given) lies between the surely-kept and the possibly-kept count."""
    d = draw64(logits, seeds, t_q, temperature, min_p)
    pred = np.asarray(pred, dtype=np.int64)
    rows, bins = logits.shape
    assert pred.shape == (rows,) and pred.min() >= 0 and pred.max() < bins, "pred outside [0, bins)"
    e = e_r[:, None]
    possibly = logits >= d["thr"][:, None] - 2 * e
    surely = logits >= d["thr"][:, None] + 2 * e
    e_s = e * d["inv_t"] + E_G * (1 + np.abs(d["g"])) + 2.0 ** -23 * np.abs(d["score"])
    floor = np.where(surely, d["score"] - e_s, -np.inf).max(1)            # what any winner must reach
    admissible = possibly & (d["score"] + e_s >= floor[:, None])
    r = np.arange(rows)
    bad = np.nonzero(~possibly[r, pred])[0]
    assert bad.size == 0, f"rows {bad[:5]}: the drawn bin is not in the kept set"
    bad = np.nonzero(~admissible[r, pred])[0]
    assert bad.size == 0, (f"rows {bad[:5]}: the drawn bin's score is below a surely kept bin's by more than the bound "
                           f"(device {pred[bad[:5]]}, float64 {d['pred'][bad[:5]]})")
    if n_kept is not None:
        n_kept = np.asarray(n_kept, dtype=np.int64)
        lo, hi = surely.sum(1), possibly.sum(1)
        bad = np.nonzero((n_kept < np.maximum(lo, 1)) | (n_kept > hi))[0]
        assert bad.size == 0, f"rows {bad[:5]}: n_kept {n_kept[bad[:5]]} outside [{lo[bad[:5]]}, {hi[bad[:5]]}]"
    return float((admissible.sum(1) == 1).mean())


def chi_square(counts, p):
    """Pearson's statistic of observed counts against probabilities p over the bins with p > 0."""
    counts, p = np.asarray(counts, dtype=np.float64), np.asarray(p, dtype=np.float64)
    live = p > 0
    expect = counts.sum() * p[live]
    return float((((counts[live] - expect) ** 2) / expect).sum())
