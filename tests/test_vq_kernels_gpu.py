"""Flat vector-quantiser kernels (csrc/vq.hip, csrc/vq_common.h, smt_amd/vq.py) one by one against float64 restatements of
the reference's formulas, at every codebook width and at the sizes where a kernel takes another path: a last partial part of
the column sums, the grid-stride loop of the backward, 2..5 column groups per workgroup of the search with a last workgroup
of one live row, the other split counts of the candidate sweep, a null x_d, the share / workgroup boundaries of the EMA
scatter-add, and a NaN row.  Indices are compared bit-exactly with oracle.vqvae_oracle.vq_argmin_exact.

u = 2^-24 is the float32 unit round-off.  Every float tolerance is a count of roundings written at its assert; each test prints
the largest error it saw next to that bound."""
import functools

import numpy as np
import pytest
import torch

from oracle import vqvae_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def bits_equal(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{what}: not bit-identical"


def report(what, err, bound):
    """Largest error / bound ratio of an elementwise check, printed before it is asserted."""
    err, bound = err.double().reshape(-1), bound.double().reshape(-1)
    if err.numel() == 0:
        return
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    i = int(ratio.argmax())
    print(f"\n[{what}] largest error {float(err[i]):.3e} against its bound {float(bound[i]):.3e} (ratio {float(ratio[i]):.3f})")
    assert bool((err <= bound).all()), f"{what}: error {float(err[i]):.3e} > bound {float(bound[i]):.3e}"


def forward_prefilled(x, cb, mask=None, want_xd=True, prep=None):
    """smt_vq_forward through the C entry the way vq.vq_forward_raw calls it, on outputs pre-filled with idx -1, NaN min_dist and
    x_d 777: a row that the kernels leave unwritten shows.  Device tensors in, host tensors out."""
    from smt_amd import native as N
    n, d = x.shape
    k = cb.shape[0]
    lib = N.lib()
    idx = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    md = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    xd = torch.full((n, d), 777.0, dtype=torch.float32, device=DEV) if want_xd else None
    sums = torch.full((4,), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(max(lib.smt_vq_forward_workspace_bytes(n, k, d), 256), dtype=torch.uint8, device=DEV)
    N.check(lib.smt_vq_forward(N.ptr(x), N.ptr(cb), N.ptr(prep), N.ptr(mask), n, k, d, N.ptr(idx), N.ptr(md), N.ptr(xd), N.ptr(sums),
                               N.ptr(ws), ws.numel(), N.stream_ptr()), "smt_vq_forward")
    torch.cuda.synchronize()
    return idx.cpu(), md.cpu(), None if xd is None else xd.cpu(), sums.cpu()


def forward_wrapped(x, cb, mask=None, want_xd=True, prep=None):
    from smt_amd import vq
    idx, md, xd, sums = vq.vq_forward_raw(x, cb, mask, want_xd=want_xd, prep=prep)
    torch.cuda.synchronize()
    return idx.cpu(), md.cpu(), None if xd is None else xd.cpu(), sums.cpu()


def check_forward(out, x, cb, mask, exact, d1):
    """The asserts of test_vq_gpu.test_indices_bit_exact_vs_oracle on host tensors."""
    idx, md, xd, sums = out
    m = np.ones(len(x), np.float32) if mask is None else mask.numpy()
    assert bool((idx >= 0).all()) and bool(torch.isfinite(md).all())          # no row left unwritten
    assert np.array_equal(idx.numpy(), exact)
    assert np.allclose(md.numpy(), d1, rtol=1e-5, atol=1e-6)
    if xd is not None:
        assert np.array_equal(xd.numpy(), cb.numpy()[exact] * m[:, None])
    s = sums.numpy()
    assert np.isclose(s[0], d1.sum(), rtol=1e-5) and np.isclose(s[1], (d1 * (m != 0)).sum(), rtol=1e-5)
    assert s[2] == m.sum()


# ------------------------------------------------------------------------- 1. EMA mix, revival, metrics, prep refresh
def _ema_case(kb, d, mu, thr, seed):
    """k, k_sum, k_elem, stats (float32) with about a third of the codes ending below the threshold on small batch counts, a
    third above it on positive counts, and a third with a zero batch count on either side."""
    g = gen(seed)
    om = float(np.float32(1.0) - np.float32(mu))
    m = float(np.float32(mu))
    cls = torch.randint(0, 3, (kb,), generator=g)                        # 0 below, 1 above, 2 zero count
    side = torch.rand(kb, generator=g) < 0.5
    below = (cls == 0) | ((cls == 2) & side)
    target = (0.1 + 0.8 * torch.rand(kb, generator=g).double()) * thr    # mixed k_elem of a code that ends below
    cmax = torch.clamp(torch.floor(0.8 * target / om), max=3.0)          # keeps the old k_elem positive
    cnt = torch.where(below, torch.floor(torch.rand(kb, generator=g).double() * (cmax + 1.0)),
                      torch.randint(1, 41, (kb,), generator=g).double())
    cnt[cls == 2] = 0.0
    if float(cnt.sum()) == 0.0:
        cnt[0] = 1.0                                                     # an empty batch has no usage histogram (0 / 0)
    k_elem = torch.where(below, (target - om * cnt) / m, (1.2 + 28.8 * torch.rand(kb, generator=g).double()) * thr / m).float()
    k = torch.randn(kb, d, generator=g)
    k_sum = k_elem[:, None] * torch.randn(kb, d, generator=g)
    stats = torch.cat([(cnt.float()[:, None] * torch.randn(kb, d, generator=g)).reshape(-1), cnt.float(),
                       torch.randn(kb * d, generator=g)])
    return k, k_sum, k_elem, stats


EMA_CASES = [  # K, D, mu, threshold
    (1024, 128, 0.99, 1.0), (512, 128, 0.99, 1.0), (256, 128, 0.99, 1.0),                 # the shipped configs
    (1, 32, 0.99, 1.0), (7, 32, 0.99, 1.0), (9, 64, 0.99, 1.0), (250, 64, 0.99, 1.0), (1001, 128, 0.99, 1.0),
    (2050, 32, 0.99, 1.0),
    (250, 64, 0.5, 1.0), (1001, 128, 0.99, 2.5),
]


@pytest.mark.parametrize("kb,d,mu,thr", EMA_CASES)
def test_ema_apply_matches_float64(kb, d, mu, thr):
    from smt_amd import vq
    k, k_sum, k_elem, stats = _ema_case(kb, d, mu, thr, seed=100 + kb + d)
    # float64 reference from the float32 inputs (update_k); mu and 1 - mu as the kernel receives / forms them
    m, om = float(np.float32(mu)), float(np.float32(1.0) - np.float32(mu))
    t = float(np.float32(thr))
    cnt, s_sum, k_rand = stats[kb * d:kb * d + kb].double(), stats[:kb * d].view(kb, d).double(), stats[kb * d + kb:].view(kb, d)
    a, b = m * k_sum.double(), om * s_sum
    ns = a + b
    ne_a, ne_b = m * k_elem.double(), om * cnt
    ne = ne_a + ne_b
    assert bool(((ne - t).abs() >= 1e-3 * t).all()) and bool((ne != 0).all())          # precondition: no code on the edge
    live = ne >= t
    k_ref = torch.where(live[:, None], ns / ne[:, None], k_rand.double())
    prob = cnt / cnt.sum()
    ent_terms = prob * torch.log(torch.clamp(prob, min=1e-5))
    dk_ref = float(torch.sqrt(((k_ref - k.double()) ** 2).sum() / (kb * d)))
    assert 0 < int(live.sum()) or kb < 3
    assert int((~live).sum()) > 0 or kb < 3

    kd, ksd, ked, sd = dev(k.clone()), dev(k_sum.clone()), dev(k_elem.clone()), dev(stats.clone())
    metrics, prep = vq.ema_apply(kd, ksd, ked, sd, sd[kb * d + kb:], mu, thr)
    torch.cuda.synchronize()
    bits_equal(sd, stats, "stats after the call")
    k_new, ks_new, ke_new, met = kd.cpu(), ksd.cpu(), ked.cpu(), metrics.cpu().double()

    # k_sum, k_elem: two products and one sum, each rounded once (or one less under contraction) -> 2 u (|a| + |b|); bound 4 u
    report(f"k_sum K={kb} D={d}", (ks_new.double() - ns).abs(), 4 * U * (a.abs() + b.abs()))
    report(f"k_elem K={kb} D={d}", (ke_new.double() - ne).abs(), 4 * U * (ne_a.abs() + ne_b.abs()))
    # live codes: at most three roundings above the division, three below, the division itself, second-order slack -> 8 u
    kb_bound = 8 * U * (a.abs() + b.abs()) / ne.abs()[:, None]
    report(f"k live K={kb} D={d}", (k_new.double() - k_ref).abs()[live], kb_bound[live])
    # revived codes: usage is exactly 0, so 0 * (k_sum / k_elem) + 1 * k_rand is the k_rand row itself
    assert torch.equal(bits(k_new)[~live], bits(k_rand)[~live]), "revived codes are not their k_rand rows"
    assert float(met[1]) == float((cnt >= t).sum()), "used_curr"
    assert float(met[2]) == float(live.sum()), "usage"
    # dk: the elementwise k bound through the norm, + the rounding of each difference and of the result (<= 2 u dk; bound 4 u dk)
    e_bound = torch.where(live[:, None], kb_bound, torch.zeros_like(kb_bound))
    dk_bound = float(torch.sqrt((e_bound ** 2).sum() / (kb * d))) + 4 * U * dk_ref
    report(f"dk K={kb} D={d}", (met[3] - dk_ref).abs().reshape(1), torch.tensor([dk_bound], dtype=torch.float64))
    # entropy: p, log p and the product rounded in float32 (the log to ~2 u) -> < 10 u |p ln p| per term, + the final rounding
    ent_ref = float(-ent_terms.sum())
    ent_bound = 10 * U * float(ent_terms.abs().sum()) + U * abs(ent_ref)
    report(f"entropy K={kb} D={d}", (met[0] - ent_ref).abs().reshape(1), torch.tensor([ent_bound], dtype=torch.float64))

    # the refreshed prep serves the next search like a fresh one, and like none
    x = dev(torch.randn(500, d, generator=gen(7)))
    i_a = forward_wrapped(x, kd, prep=prep)[0]
    i_b = forward_wrapped(x, kd, prep=vq.prepare(kd))[0]
    i_c = forward_wrapped(x, kd)[0]
    exact, _, _ = orc.vq_argmin_exact(x.cpu().numpy(), k_new.numpy())
    assert torch.equal(i_a, i_b) and torch.equal(i_a, i_c)
    assert np.array_equal(i_a.numpy(), exact)


def test_prepare_reuses_its_buffer_after_an_in_place_change():
    from smt_amd import vq
    g = gen(31)
    kb, d = 250, 64
    k = dev(torch.randn(kb, d, generator=g))
    x = dev(torch.randn(500, d, generator=g))
    old = vq.prepare(k)
    before = forward_wrapped(x, k, prep=old)[0]
    k.mul_(-0.7).add_(dev(0.5 * torch.randn(kb, d, generator=g)))         # same storage, new content
    prep = vq.prepare(k, prep=old)
    assert prep.data_ptr() == old.data_ptr()
    i_a = forward_wrapped(x, k, prep=prep)[0]
    i_b = forward_wrapped(x, k, prep=vq.prepare(k))[0]
    i_c = forward_wrapped(x, k)[0]
    exact, _, _ = orc.vq_argmin_exact(x.cpu().numpy(), k.cpu().numpy())
    assert torch.equal(i_a, i_b) and torch.equal(i_a, i_c)
    assert np.array_equal(i_a.numpy(), exact)
    assert not torch.equal(i_a, before)                                   # the change did move rows to other codes


# ------------------------------------------------------------------------- 2. straight-through backward
def _backward(x, x_d, mask, dy, gc, sums):
    from smt_amd import native as N
    n, d = x.shape
    dx = torch.full((n, d), float("nan"), dtype=torch.float32, device=DEV)
    N.check(N.lib().smt_vq_backward(N.ptr(x), N.ptr(x_d), N.ptr(mask), N.ptr(dy), N.ptr(gc), N.ptr(sums), n, d, N.ptr(dx),
                                    N.stream_ptr()), "smt_vq_backward")
    torch.cuda.synchronize()
    return dx.cpu()


def _backward_ref(x, x_d, mask, dy, gc, sums2):
    """float64: dx = dy mask + [mask != 0] (x - x_d) g_commit 2 / (sums[2] D), absent terms dropped; returns (dx, bound) with
    bound = 4 u (|dy| + |x - x_d| |coef|): the coefficient, the difference, their product and the final sum round once each."""
    n, d = x.shape
    m = torch.ones(n, dtype=torch.float64) if mask is None else mask.double()
    ref = torch.zeros(n, d, dtype=torch.float64)
    bound = torch.zeros(n, d, dtype=torch.float64)
    if dy is not None:
        ref += dy.double() * m[:, None]
        bound += dy.double().abs()
    if gc is not None:
        coef = float(gc.double()) * 2.0 / (float(sums2) * d)
        diff = (x.double() - x_d.double()) * (m != 0)[:, None]
        ref += diff * coef
        bound += diff.abs() * abs(coef)
    return ref, 4 * U * bound


def _backward_case(n, d, has_dy, has_gc, has_mask, seed, all_masked=False):
    g = gen(seed)
    x = torch.randn(n, d, generator=g)
    cb = torch.randn(16, d, generator=g)
    idx = torch.randint(0, 16, (n,), generator=g)
    mask = None
    if has_mask:
        mask = torch.zeros(n) if all_masked else (torch.rand(n, generator=g) > 0.2).float()
    x_d = cb[idx] * (1.0 if mask is None else mask[:, None])
    dy = torch.randn(n, d, generator=g) if has_dy else None
    gc = torch.tensor([1.7]) if has_gc else None
    sums = torch.tensor([0.0, 0.0, float(n if mask is None else mask.sum()), 0.0])
    got = _backward(dev(x), dev(x_d), dev(mask), dev(dy), dev(gc), dev(sums))
    ref, bound = _backward_ref(x, x_d, mask, dy, gc, sums[2])
    what = f"vq_backward n={n} D={d} dy={has_dy} g_commit={has_gc} mask={has_mask}"
    assert bool(torch.isfinite(got).all()), what
    report(what, (got.double() - ref).abs(), bound)
    if mask is not None:
        assert bool((got[mask == 0] == 0).all()), f"{what}: masked rows are not zero"
    if not has_dy and not has_gc:
        assert bool((got == 0).all())


@pytest.mark.parametrize("has_mask", [True, False])
@pytest.mark.parametrize("has_gc", [True, False])
@pytest.mark.parametrize("has_dy", [True, False])
def test_backward_null_branches(has_dy, has_gc, has_mask):
    _backward_case(257, 64, has_dy, has_gc, has_mask, seed=40)


@pytest.mark.parametrize("n,d", [(1, 32), (3, 128), (16500, 128)])      # 16500 x 128 = 528,000 float4s > 2048 x 256: the stride loop
def test_backward_sizes(n, d):
    _backward_case(n, d, True, True, True, seed=41 + n)


@pytest.mark.parametrize("has_dy", [True, False])
def test_backward_every_row_masked(has_dy):
    _backward_case(257, 64, has_dy, False, True, seed=42, all_masked=True)   # sums[2] = 0: the commit term would be 0 / 0


def test_backward_after_the_codebook_was_rewritten_in_place():
    """Production order: forward, update_k (rewrites the codebook in place), backward.  The gradient is the old codebook's."""
    from smt_amd import vq
    g = gen(43)
    kb, d, n = 256, 128, 1000
    x = torch.randn(n, d, generator=g)
    cb = torch.randn(kb, d, generator=g)
    mask = (torch.rand(n, generator=g) > 0.2).float()
    w = torch.randn(n, d, generator=g)
    k = dev(cb.clone())
    prep = vq.prepare(k)
    xg, md = dev(x).requires_grad_(True), dev(mask)
    x_d, idx, commit, fit = vq.vq_straight_through(xg, k, md, prep=prep)
    loss = (x_d * dev(w)).sum() + 3.0 * commit
    exact, _, _ = orc.vq_argmin_exact(x.numpy(), cb.numpy())
    assert np.array_equal(idx.cpu().numpy(), exact)
    stats = torch.empty(vq.ema_stats_numel(kb, d), device=DEV)
    vq.ema_accumulate(xg.detach(), idx, md, kb, stats)
    stats[kb * d + kb:] = dev(torch.randn(kb * d, generator=g))
    k_sum, k_elem = k.clone(), torch.ones(kb, device=DEV)
    vq.ema_apply(k, k_sum, k_elem, stats, stats[kb * d + kb:], 0.99, 1.0, prep=prep)
    torch.cuda.synchronize()
    assert not torch.equal(k.cpu(), cb)
    loss.backward()
    torch.cuda.synchronize()
    x_d_old = cb[torch.from_numpy(exact)] * mask[:, None]
    ref, bound = _backward_ref(x, x_d_old, mask, w, torch.tensor([3.0]), mask.sum())
    report("x.grad after an in-place update_k", (xg.grad.cpu().double() - ref).abs(), bound)


# ------------------------------------------------------------------------- 3. search geometry
@functools.lru_cache(maxsize=None)
def _geometry_case(n, d):
    g = gen(n + d)
    x = torch.randn(n, d, generator=g)
    cb = torch.randn(40, d, generator=g)
    mask = (torch.rand(n, generator=g) > 0.2).float()
    exact, d1, _ = orc.vq_argmin_exact(x.numpy(), cb.numpy())
    return x, cb, mask, exact, d1


GEOMETRY = [(8193, 32), (16417, 64), (24609, 128), (40961, 32)]       # 2, 3, 4, 5 column groups; the last workgroup has one live row


@pytest.mark.parametrize("n,d", GEOMETRY)
def test_search_column_groups_and_a_last_workgroup_of_one_row(n, d):
    x, cb, mask, exact, d1 = _geometry_case(n, d)
    xd_, cbd, md_ = dev(x), dev(cb), dev(mask)
    first = forward_wrapped(xd_, cbd, md_)
    check_forward(first, x, cb, mask, exact, d1)
    again = forward_prefilled(xd_, cbd, md_)                 # idx -1, NaN min_dist, x_d 777 before the call
    check_forward(again, x, cb, mask, exact, d1)
    for a, b, what in zip(first, again, ("idx", "min_dist", "x_d", "sums")):
        assert torch.equal(a, b) if a.dtype == torch.int64 else torch.equal(bits(a), bits(b)), what


# ------------------------------------------------------------------------- 4. queued rows at the other splits and widths
@functools.lru_cache(maxsize=None)
def _near_tie_case(kb, d):
    """The construction of test_vq_gpu.test_near_tie_rows_take_the_fp64_path_and_stay_exact."""
    g = gen(kb + d)
    n = 3000
    base = torch.randn(n, d, generator=g) * 0.3 + 3.0 * torch.randn(1, d, generator=g)
    rows = base.repeat(2, 1) + torch.randn(2 * n, d, generator=g) * 1e-4
    cb = rows[torch.randperm(2 * n, generator=g)][:kb].clone()
    cb[100] = cb[7]
    exact, d1, _ = orc.vq_argmin_exact(base.numpy(), cb.numpy(), chunk=256)     # same arithmetic per row; the [chunk, K] block stays in cache
    return base, cb, exact, d1


NEAR_TIES = [(300, 32), (700, 64), (1030, 128), (1500, 64)]           # kpad 512, 768, 1280, 1536 -> splits 8, 4, 4, 8


@pytest.mark.parametrize("kb,d", NEAR_TIES)
def test_queued_rows_at_every_split_count_and_width(kb, d):
    x, cb, exact, d1 = _near_tie_case(kb, d)
    idx, md, xd, sums = forward_prefilled(dev(x), dev(cb))
    print(f"\n[near ties K={kb} D={d}] {int(sums[3])} of {len(x)} rows re-scored in fp64")
    assert bool((idx >= 0).all()) and bool(torch.isfinite(md).all())
    assert np.array_equal(idx.numpy(), exact)
    assert float(sums[3]) > 0
    assert not bool((idx == 100).any())
    assert np.array_equal(xd.numpy(), cb.numpy()[exact])


# ------------------------------------------------------------------------- 5. want_xd=False
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("case", ["geometry", "near_tie"])
def test_without_x_d_the_other_outputs_keep_their_bits(case, masked):
    if case == "geometry":
        x, cb, mask, exact, _ = _geometry_case(16417, 64)
    else:
        x, cb, exact, _ = _near_tie_case(700, 64)
        mask = (torch.rand(len(x), generator=gen(5)) > 0.2).float()
    mask = mask if masked else None
    xd_, cbd, md_ = dev(x), dev(cb), dev(mask)
    full = forward_wrapped(xd_, cbd, md_, want_xd=True)
    for run in (forward_wrapped, forward_prefilled):
        idx, md, xd, sums = run(xd_, cbd, md_, want_xd=False)
        assert xd is None
        assert torch.equal(idx, full[0]) and np.array_equal(idx.numpy(), exact)
        bits_equal(md, full[1], "min_dist")
        bits_equal(sums, full[3], "sums")
    if case == "near_tie":
        assert float(full[3][3]) > 0


# ------------------------------------------------------------------------- 6. ema_accumulate edges
def _accumulate(x, idx, mask, kb):
    from smt_amd import vq
    d = x.shape[1]
    stats = torch.full((vq.ema_stats_numel(kb, d),), 7.0, device=DEV)
    vq.ema_accumulate(dev(x), dev(idx), dev(mask), kb, stats)
    torch.cuda.synchronize()
    assert bool((stats[kb * d + kb:] == 7.0).all()), "the revival rows' slot was written"
    return stats[:kb * d + kb].cpu()


def _check_accumulate(x, idx, mask, kb, seed=0):
    n, d = x.shape
    got = _accumulate(x, idx, mask, kb)
    sel = torch.ones(n, dtype=torch.bool) if mask is None else mask != 0
    ref_sum = torch.zeros(kb, d, dtype=torch.float64).index_add_(0, idx[sel], x[sel].double())
    ref_cnt = torch.bincount(idx[sel], minlength=kb).double()
    assert torch.equal(got[kb * d:].double(), ref_cnt)
    # each addend is rounded once to the 2^-24 grid (<= 2^-25 each), the sum once to float32
    fullest = float(ref_cnt.max()) if n else 0.0
    bound = fullest * 2.0 ** -25 + U * ref_sum.abs()
    report(f"ema_accumulate n={n} K={kb} D={d}", (got[:kb * d].view(kb, d).double() - ref_sum).abs(), bound + 1e-300)
    perm = torch.randperm(n, generator=gen(seed + 1))
    again = _accumulate(x[perm], idx[perm], None if mask is None else mask[perm], kb)
    bits_equal(again, got, "statistics of a row permutation")
    return got


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025])             # around one share (64 rows) and one workgroup's rows (1024)
def test_ema_accumulate_row_counts_around_a_share_and_a_workgroup(n, masked):
    g = gen(60 + n)
    x = torch.randn(n, 64, generator=g)
    idx = torch.randint(0, 37, (n,), generator=g)
    mask = (torch.rand(n, generator=g) > 0.1).float() if masked else None
    _check_accumulate(x, idx, mask, 37, seed=n)


def test_ema_accumulate_single_code():
    g = gen(61)
    x = torch.randn(200, 32, generator=g)
    mask = (torch.rand(200, generator=g) > 0.1).float()
    _check_accumulate(x, torch.zeros(200, dtype=torch.long), mask, 1)


def test_ema_accumulate_two_codes_per_scan_thread():
    """K = 1500: vq_ema_scan_kernel gives two codes to each of its first 750 threads and none to the rest."""
    g = gen(62)
    n, kb = 5000, 1500
    x = torch.randn(n, 128, generator=g)
    idx = torch.randint(0, kb, (n,), generator=g)
    mask = (torch.rand(n, generator=g) > 0.1).float()
    idx[0], idx[1] = kb - 2, kb - 1
    mask[:2] = 1.0
    got = _check_accumulate(x, idx, mask, kb)
    assert float(got[kb * 128 + kb - 2]) >= 1 and float(got[kb * 128 + kb - 1]) >= 1


def test_ema_accumulate_every_row_masked_and_no_rows():
    g = gen(63)
    x = torch.randn(300, 128, generator=g)
    idx = torch.randint(0, 256, (300,), generator=g)
    got = _check_accumulate(x, idx, torch.zeros(300), 256)
    assert bool((bits(got) == 0).all())
    got = _check_accumulate(torch.zeros(0, 128), torch.zeros(0, dtype=torch.long), None, 256)
    assert bool((bits(got) == 0).all())


# ------------------------------------------------------------------------- 7. NaN rows
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("kb,d", [(64, 32), (300, 128), (320, 128)])
def test_nan_row_gets_code_zero_and_a_defined_x_d(kb, d, masked):
    """A row with a NaN has no finite distance: idx 0, NaN min_dist, x_d = k[0] * mask -- the contract of smt_vq_forward, of the
    grouped quantiser and of the reference's min over a NaN row.  (Before the fix the flat kernel left the row of x_d unwritten.)
    The grouped quantiser takes l_bins that are multiples of 32 only, so the two are compared at K = 64 and K = 320."""
    from smt_amd import vq
    g = gen(70 + kb)
    n = 200
    x = torch.randn(n, d, generator=g)
    cb = torch.randn(kb, d, generator=g)
    other = torch.randn(kb, d, generator=g) + 5.0
    mask = None
    if masked:
        mask = (torch.rand(n, generator=g) > 0.2).float()
        mask[17], mask[150] = 1.0, 0.0
    xn = x.clone()
    xn[17, 5] = float("nan")
    xn[150] = float("nan")
    bad = torch.zeros(n, dtype=torch.bool)
    bad[17] = bad[150] = True
    m = torch.ones(n) if mask is None else mask
    want_bad = cb[0][None, :] * m[bad][:, None]
    xd_, xnd, cbd, md_ = dev(x), dev(xn), dev(cb), dev(mask)
    clean = forward_prefilled(xd_, cbd, md_)
    exact, _, _ = orc.vq_argmin_exact(x.numpy(), cb.numpy())
    assert np.array_equal(clean[0].numpy(), exact)
    forward_wrapped(xd_, dev(other), md_)                                  # leaves another codebook's rows in the freed x_d block
    for run in (forward_wrapped, forward_prefilled):
        idx, md, xd, sums = run(xnd, cbd, md_)
        assert bool((idx[bad] == 0).all()) and bool(torch.isnan(md[bad]).all())
        bits_equal(xd[bad], want_bad, f"x_d of the NaN rows ({run.__name__})")
        assert torch.equal(idx[~bad], clean[0][~bad])
        bits_equal(xd[~bad], clean[2][~bad], "x_d of the other rows")
        bits_equal(md[~bad], clean[1][~bad], "min_dist of the other rows")
        assert float(sums[2]) == float(m.sum()) and float(sums[3]) >= 2
    if kb % 32 == 0:
        q_rel, q_abs, md_g, xd_g, _ = vq.grouped_forward_raw(xnd, torch.zeros(n, dtype=torch.int32, device=DEV), cbd, 1, kb, md_)
        torch.cuda.synchronize()
        assert torch.equal(q_rel.cpu(), idx) and torch.equal(q_abs.cpu(), idx)
        bits_equal(xd_g, xd, "x_d of the grouped quantiser")
        assert bool(torch.isnan(md_g.cpu()[bad]).all())
        assert torch.allclose(md_g.cpu()[~bad], md[~bad], rtol=1e-5, atol=0)      # as test_single_group_equals_flat_search
