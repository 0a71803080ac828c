"""Grouped (text-conditioned) VQ bottleneck of VQTTS: the kernels of csrc/vq_grouped.hip and the large-table EMA path
through smt_amd.vq and models.vqtts.bottleneck, against a float64 oracle written here and against the fixture captured
from the reference (tests/golden/make_golden_vqtts.py).  Index comparisons are BIT-EXACT on every row; float outputs carry
the tolerance written at each assert."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def dev(a):
    return (T(a) if isinstance(a, np.ndarray) else a).cuda().contiguous()


def oracle(x, group, cb, l_bins, full=False):
    """float64 argmin over the codes of each row's group of sum_i (x_i - k_ji)^2 (direct form), lowest index on ties ->
    (q_rel, min_dist).  full=False narrows each row to its 4 best codes by the expanded form in float64 first (error
    ~1e-12 against gaps of 1e-3 and more on random data); full=True scores every code directly (ties, degenerate tables)."""
    n, d = x.shape
    x64 = x.astype(np.float64)
    q_rel = np.zeros(n, dtype=np.int64)
    md = np.zeros(n, dtype=np.float64)
    for g in np.unique(group):
        rows = np.nonzero(group == g)[0]
        k = cb[g * l_bins:(g + 1) * l_bins].astype(np.float64)
        for r0 in range(0, rows.size, 512):
            rr = rows[r0:r0 + 512]
            xr = x64[rr]
            if full:
                cand = np.broadcast_to(np.arange(l_bins), (rr.size, l_bins))
            else:
                approx = (xr ** 2).sum(1)[:, None] - 2.0 * xr @ k.T + (k ** 2).sum(1)[None, :]
                cand = np.sort(np.argpartition(approx, 3, axis=1)[:, :4], axis=1)
            dist = ((xr[:, None, :] - k[cand]) ** 2).sum(-1)
            best = np.argmin(dist, axis=1)                      # first minimum = lowest index (cand is ascending)
            q_rel[rr] = cand[np.arange(rr.size), best]
            md[rr] = dist[np.arange(rr.size), best]
    return q_rel, md


def draw_groups(usage, n, n_groups, gen):
    if usage == "uniform":
        return torch.randint(0, n_groups, (n,), generator=gen).to(torch.int32)
    if usage == "zipf":
        w = 1.0 / torch.arange(1, n_groups + 1, dtype=torch.float64)
        return torch.multinomial(w / w.sum(), max(n, 1), replacement=True, generator=gen)[:n].to(torch.int32)
    return torch.full((n,), n_groups // 2, dtype=torch.int32)   # one group holds every row, every other group is empty


def run_grouped(x, group, cb, n_groups, l_bins, mask=None, prep=None):
    from smt_amd import vq
    q_rel, q_abs, md, xd, sums = vq.grouped_forward_raw(dev(x), dev(group), dev(cb), n_groups, l_bins,
                                                        None if mask is None else dev(mask), prep=prep)
    torch.cuda.synchronize()
    return q_rel.cpu().numpy(), q_abs.cpu().numpy(), md.cpu().numpy(), xd.cpu().numpy(), sums.cpu().numpy()


def scaled(atol, ref):
    """The flat block's absolute tolerances were set on data of order 1: scale by max(1, max|reference array|)."""
    return atol * max(1.0, float(np.abs(np.asarray(ref)).max()))


# ---- 1. the reference's own three training steps and one eval step -------------------------------------------------
def test_fixture_replay_matches_reference(golden):
    """Tolerances are those of tests/test_vq_gpu.py::test_forward_backward_update_k_match_reference for the same
    quantities, the absolute ones scaled by max(1, max|reference array|) (this fixture's rows reach ~4.5).
    Measured on an MI355X (worst step): y_d 1.4e-6 against a bound of 4.7e-6 (0 on the first step: the reference's
    x + (x_d - x) rounding), gradient 1.2e-7 against 1.0e-6, k and k_sum 1.4e-6 against 4.8e-5, k_elem 2.4e-7 against
    1.1e-5; commit and fit agree to 7 digits."""
    from models.vqtts.bottleneck import Bottleneck
    g = golden("vqtts_bottleneck")
    n_vocab, l_bins = int(g["n_vocab"]), int(g["l_bins"])
    d = g["s0_y_enc"].shape[-1]
    m = Bottleneck(n_vocab, l_bins, d, float(g["mu"]), float(g["threshold"])).cuda()
    for tag in ("s0", "s1", "s2", "e"):
        train = tag != "e"
        m.train(train)
        y = dev(g[f"{tag}_y_enc"]).requires_grad_(True)
        # the dense path on one step, the index form on the others
        align = dev(g[f"{tag}_attn"]).float() if tag == "s1" else dev(g[f"{tag}_align_idx"])
        kw = dict(k_rand=dev(g[f"{tag}_k_rand"])) if train else {}
        if tag == "s0":
            kw["k_rand_init"] = dev(g["s0_k_rand_init"])
        q_rel, y_d, commit, metrics = m(y, dev(g[f"{tag}_x_id"]), align, **kw)
        (y_d.sum() + 3.0 * commit).backward()
        torch.cuda.synchronize()
        assert np.array_equal(q_rel.cpu().numpy(), g[f"{tag}_q_rel"]), tag          # every row, bit-identical
        ref = g[f"{tag}_y_d"]
        err = np.abs(y_d.detach().cpu().numpy() - ref).max()
        print(f"\n[{tag}] max|y_d - ref| {err:.3e} (bound {scaled(1e-6, ref):.3e})", end="")
        assert err <= scaled(1e-6, ref), tag
        ref = g[f"{tag}_dy_enc"]
        err = np.abs(y.grad.cpu().numpy() - ref).max()
        print(f"; grad {err:.3e} (bound {scaled(1e-6, ref):.3e})", end="")
        assert err <= scaled(1e-6, ref), tag
        print(f"; commit {commit.item():.7f} vs {float(g[f'{tag}_commit']):.7f}; fit {metrics['fit'].item():.5f} vs "
              f"{float(g[f'{tag}_m_fit']):.5f}", end="")
        assert np.isclose(commit.item(), float(g[f"{tag}_commit"]), rtol=1e-5), tag
        assert np.isclose(metrics["fit"].item(), float(g[f"{tag}_m_fit"]), rtol=2e-5), tag
        if not train:
            assert set(metrics) == {"fit"}
            continue
        for name, tns in (("k", m.k), ("k_sum", m.k_sum), ("k_elem", m.k_elem)):
            ref = g[f"{tag}_{name}"]
            err = np.abs(tns.cpu().numpy() - ref).max()
            print(f"; {name} {err:.3e} (bound {scaled(1e-5, ref):.3e})", end="")
            assert err <= scaled(1e-5, ref), (tag, name)
        for mk in ("entropy", "used_curr", "usage", "dk"):
            assert np.isclose(metrics[mk].item(), float(g[f"{tag}_m_{mk}"]), rtol=1e-4), (tag, mk)


# ---- 2. float64 oracle over the grid -------------------------------------------------------------------------------
@pytest.mark.parametrize("usage", ["uniform", "zipf", "one_group"])
@pytest.mark.parametrize("n_groups", [1, 7, 149])
@pytest.mark.parametrize("l_bins", [32, 512, 1024])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_indices_bit_exact_vs_oracle(d, l_bins, n_groups, usage):
    from smt_amd import vq
    gen = torch.Generator().manual_seed(1000 * d + l_bins + n_groups)
    # every group has its own offset (groups drift apart in training) on top of a common one
    centre = 2.0 * torch.randn(n_groups, 1, d, generator=gen) + 3.0 * torch.randn(1, 1, d, generator=gen)
    cb_t = (torch.randn(n_groups, l_bins, d, generator=gen) + centre).reshape(n_groups * l_bins, d).contiguous()
    cb = cb_t.numpy()
    cb_dev = cb_t.cuda()
    prep = vq.grouped_prepare(cb_dev, n_groups, l_bins)
    for n in (0, 1, 63, 4544):
        group_t = draw_groups(usage, n, n_groups, gen)
        x_t = torch.randn(n, d, generator=gen) + centre[group_t.long(), 0]
        mask_t = (torch.rand(n, generator=gen) > 0.2).float()
        x, group, mask = x_t.numpy(), group_t.numpy(), mask_t.numpy()
        q_rel, q_abs, md, xd, sums = run_grouped(x, group, cb_dev, n_groups, l_bins, mask, prep=prep)
        assert q_rel.shape == (n,) and xd.shape == (n, d)
        if n == 0:
            assert (sums[:3] == 0).all()
            continue
        exact, d1 = oracle(x, group, cb, l_bins)
        assert np.array_equal(q_rel, exact), (n, int((q_rel != exact).sum()))
        assert np.array_equal(q_abs, group.astype(np.int64) * l_bins + exact)
        assert np.allclose(md, d1, rtol=1e-5, atol=1e-6)                    # fp32 direct-form distance
        assert np.array_equal(xd, cb[q_abs] * mask[:, None])
        assert np.isclose(sums[0], d1.sum(), rtol=1e-5) and np.isclose(sums[1], (d1 * mask).sum(), rtol=1e-5)
        assert sums[2] == mask.sum()


# ---- 3. near-ties and degenerate tables ----------------------------------------------------------------------------
def test_near_ties_stay_exact_and_inside_the_group():
    gen = torch.Generator().manual_seed(3)
    n_groups, l_bins, d, n = 5, 64, 128, 700
    cb = (0.3 * torch.randn(n_groups * l_bins, d, generator=gen) + 3.0 * torch.randn(1, d, generator=gen)).numpy().copy()
    group = torch.randint(1, n_groups, (n,), generator=gen).to(torch.int32).numpy()
    a = torch.randint(0, l_bins, (n,), generator=gen).numpy()
    b = (a + 1 + torch.randint(0, l_bins - 1, (n,), generator=gen).numpy()) % l_bins
    ka, kb = cb[group * l_bins + a], cb[group * l_bins + b]
    x = ((ka + kb) * np.float32(0.5)).astype(np.float32)        # equidistant from two codes of the group up to rounding
    x[::3] = np.nextafter(x[::3], ka[::3])                      # ... and one ulp towards one of them, per element
    # a duplicate of a row's own position in ANOTHER group (group 0, lower absolute indices): distance 0, must not win
    cb[:l_bins][np.arange(n) % l_bins] = x
    q_rel, q_abs, md, xd, sums = run_grouped(x, group, cb, n_groups, l_bins)
    exact, d1 = oracle(x, group, cb, l_bins, full=True)
    assert np.array_equal(q_rel, exact)
    assert np.array_equal(q_abs // l_bins, group) and np.array_equal(q_abs % l_bins, q_rel)
    assert sums[3] > 0                                           # the fp64 queue was exercised
    assert np.allclose(md, d1, rtol=1e-5, atol=1e-6)


def test_group_of_equal_codes_lowest_index_wins():
    gen = torch.Generator().manual_seed(4)
    n_groups, l_bins, d, n = 3, 96, 64, 300
    cb = torch.randn(n_groups * l_bins, d, generator=gen).numpy().copy()
    cb[l_bins:2 * l_bins] = cb[l_bins]                           # group 1: all L codes equal
    cb[2 * l_bins + 40] = cb[2 * l_bins + 7]                     # group 2: one exact duplicate
    x = torch.randn(n, d, generator=gen).numpy()
    x[-20:] = cb[2 * l_bins + 7] + 1e-3 * x[-20:]                # rows that sit on the duplicated code
    group = (np.arange(n) % n_groups).astype(np.int32)
    group[-20:] = 2
    q_rel, q_abs, md, xd, sums = run_grouped(x, group, cb, n_groups, l_bins)
    exact, d1 = oracle(x, group, cb, l_bins, full=True)
    assert np.array_equal(q_rel, exact)
    assert (q_rel[group == 1] == 0).all() and not (q_rel[group == 2] == 40).any() and (q_rel[-20:] == 7).all()
    assert sums[3] >= (group == 1).sum() + 20
    assert np.allclose(md, d1, rtol=1e-5, atol=1e-6)


# ---- 4. one group == the flat kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,l_bins,d", [(4544, 512, 128), (1000, 64, 64), (77, 1024, 32)])
def test_single_group_equals_flat_search(n, l_bins, d):
    from smt_amd import vq
    gen = torch.Generator().manual_seed(n)
    x = (torch.randn(n, d, generator=gen) + 2.0).cuda()
    cb = (torch.randn(l_bins, d, generator=gen) + 2.0).cuda()
    mask = (torch.rand(n, generator=gen) > 0.2).float().cuda()
    idx, md_f, xd_f, sums_f = vq.vq_forward_raw(x, cb, mask)
    q_rel, q_abs, md_g, xd_g, sums_g = vq.grouped_forward_raw(x, torch.zeros(n, dtype=torch.int32, device="cuda"), cb, 1, l_bins, mask)
    assert torch.equal(q_rel, idx) and torch.equal(q_abs, idx) and torch.equal(xd_g, xd_f)
    assert torch.allclose(md_g, md_f, rtol=1e-5, atol=0)
    assert torch.allclose(sums_g[:3], sums_f[:3], rtol=1e-5, atol=0)


# ---- 5. large-table EMA --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("usage", ["uniform", "zipf"])
def test_large_table_ema_matches_dense_onehot(usage):
    from smt_amd import vq
    gen = torch.Generator().manual_seed(21)
    n, d, n_groups, l_bins = 36352, 128, 149, 512
    kb = n_groups * l_bins
    x = torch.randn(n, d, generator=gen)
    if usage == "uniform":
        idx = torch.randint(0, kb, (n,), generator=gen)
    else:                                                        # Zipf over tokens AND over the codes of a token
        wg = 1.0 / torch.arange(1, n_groups + 1, dtype=torch.float64)
        wl = 1.0 / torch.arange(1, l_bins + 1, dtype=torch.float64)
        idx = (torch.multinomial(wg / wg.sum(), n, replacement=True, generator=gen) * l_bins
               + torch.multinomial(wl / wl.sum(), n, replacement=True, generator=gen))
    mask = (torch.rand(n, generator=gen) > 0.1).float()
    stats = torch.empty(vq.ema_stats_numel(kb, d), device="cuda")
    vq.ema_accumulate(x.cuda(), idx.cuda(), mask.cuda(), kb, stats)
    sel = mask != 0
    ref_sum = torch.zeros(kb, d, dtype=torch.float64).index_add_(0, idx[sel], x[sel].double())
    ref_cnt = torch.bincount(idx[sel], minlength=kb).double()
    got = stats.cpu().double()
    # 64-bit fixed point (2^-24 units): each addend rounded once by <= 2^-25; the most used code of the Zipf draw has
    # ~1,200 addends -> 4e-5 worst case, then one rounding to f32 (rtol); uniform usage has < 10 addends per code
    assert torch.allclose(got[:kb * d].view(kb, d), ref_sum, atol=4e-6 if usage == "uniform" else 1e-4, rtol=1e-6)
    assert torch.equal(got[kb * d:kb * d + kb], ref_cnt)
    live = kb * d + kb
    again = torch.empty_like(stats)
    vq.ema_accumulate(x.cuda(), idx.cuda(), mask.cuda(), kb, again)
    assert torch.equal(again[:live], stats[:live])               # two runs: identical bits
    perm = torch.randperm(n, generator=gen)
    vq.ema_accumulate(x[perm].cuda(), idx[perm].cuda(), mask[perm].cuda(), kb, again)
    assert torch.equal(again[:live], stats[:live])               # ... for any row order


def test_large_and_small_table_paths_give_the_same_bits():
    """The same rows and codes (all below 16384) at k_bins = 16384 (the LDS-histogram path, unchanged) and at
    k_bins = 16384 + 512 (the global-memory path): the statistics of the shared codes are bit-identical."""
    from smt_amd import vq
    gen = torch.Generator().manual_seed(22)
    n, d, kb = 20000, 64, 16384
    x = torch.randn(n, d, generator=gen).cuda()
    idx = torch.randint(0, kb, (n,), generator=gen).cuda()
    mask = (torch.rand(n, generator=gen) > 0.1).float().cuda()
    small = torch.empty(vq.ema_stats_numel(kb, d), device="cuda")
    large = torch.empty(vq.ema_stats_numel(kb + 512, d), device="cuda")
    vq.ema_accumulate(x, idx, mask, kb, small)
    vq.ema_accumulate(x, idx, mask, kb + 512, large)
    assert torch.equal(small[:kb * d], large[:kb * d])
    assert torch.equal(small[kb * d:kb * d + kb], large[(kb + 512) * d:(kb + 512) * d + kb])
    assert (large[kb * d:(kb + 512) * d] == 0).all() and (large[(kb + 512) * d + kb:(kb + 512) * (d + 1)] == 0).all()


# ---- 6. masked rows ------------------------------------------------------------------------------------------------
def test_masked_rows_are_searched_in_group_zero_and_ignored_elsewhere():
    from models.vqtts.bottleneck import Bottleneck
    gen = torch.Generator().manual_seed(6)
    n_vocab, l_bins, d, b, tx, t = 9, 64, 32, 4, 6, 50
    m = Bottleneck(n_vocab, l_bins, d, 0.9, 1.0).cuda().train()
    k0 = torch.randn(n_vocab * l_bins, d, generator=gen)
    y = torch.randn(b, t, d, generator=gen)
    x_id = torch.randint(1, n_vocab, (b, tx), generator=gen)     # no token 0: only masked rows land in group 0
    align = torch.randint(0, tx, (b, t), generator=gen).to(torch.int32)
    align[:, 37:] = -1
    align[2, 20:] = -1
    yd = y.cuda().requires_grad_(True)
    q_rel, y_d, commit, metrics = m(yd, x_id.cuda(), align.cuda(), k_rand=k0.cuda(), k_rand_init=k0.cuda())
    (y_d.sum() + commit).backward()
    torch.cuda.synchronize()
    mask = (align >= 0).reshape(-1).numpy()
    group = np.where(mask, x_id.numpy()[np.arange(b)[:, None], np.maximum(align.numpy(), 0)].reshape(-1), 0)
    exact, d1 = oracle(y.reshape(-1, d).numpy(), group, k0.numpy(), l_bins)
    assert np.array_equal(q_rel.reshape(-1).cpu().numpy(), exact)                    # masked rows: group 0's argmin
    assert (y_d.detach().reshape(-1, d).cpu().numpy()[~mask] == 0).all()
    assert (yd.grad.reshape(-1, d).cpu().numpy()[~mask] == 0).all()
    assert np.isclose(commit.item(), d1[mask].sum() / (mask.sum() * d), rtol=1e-5)   # unmasked rows only
    assert np.isclose(metrics["fit"].item(), d1.sum() / l_bins, rtol=2e-5)           # ALL rows, the reference's broadcast
    # EMA: k_elem = mu * 1 + (1 - mu) * count over UNMASKED rows only -- group 0 saw no unmasked row
    cnt = np.bincount((group * l_bins + exact)[mask], minlength=n_vocab * l_bins)
    assert np.allclose(m.k_elem.cpu().numpy(), 0.9 + 0.1 * cnt, atol=1e-5)   # two fp32 products of order 1
    assert cnt[:l_bins].sum() == 0


# ---- 7. determinism ------------------------------------------------------------------------------------------------
def test_three_training_steps_twice_bit_identical():
    from models.vqtts.bottleneck import Bottleneck

    def run():
        torch.manual_seed(77)
        gen = torch.Generator().manual_seed(7)
        n_vocab, l_bins, d, b, tx, t = 20, 64, 64, 8, 12, 300
        m = Bottleneck(n_vocab, l_bins, d, 0.99, 1.0).cuda().train()
        out = []
        for _ in range(3):
            y = (torch.randn(b, t, d, generator=gen) + 1.5).cuda().requires_grad_(True)
            x_id = torch.randint(0, n_vocab, (b, tx), generator=gen).cuda()
            align = torch.sort(torch.randint(0, tx, (b, t), generator=gen), dim=1).values.to(torch.int32)
            align[:, 280:] = -1
            q_rel, y_d, commit, metrics = m(y, x_id, align.cuda())
            ((y_d * y_d).sum() + commit).backward()
            out += [q_rel, commit.detach(), y.grad, m.k.clone(), metrics["fit"], metrics["entropy"], metrics["dk"]]
        torch.cuda.synchronize()
        return [o.cpu() for o in out]
    a, b_ = run(), run()
    assert all(torch.equal(u, v) for u, v in zip(a, b_))


# ---- 8. bad arguments ----------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_name_the_argument():
    from models.vqtts.bottleneck import Bottleneck
    from smt_amd import native, vq
    x = torch.zeros(8, 64, device="cuda")
    g = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="l_bins"):
        vq.grouped_forward_raw(x, g, torch.zeros(2 * 48, 64, device="cuda"), 2, 48)
    with pytest.raises(ValueError, match="dim"):
        vq.grouped_forward_raw(torch.zeros(8, 48, device="cuda"), g, torch.zeros(2 * 32, 48, device="cuda"), 2, 32)
    with pytest.raises(ValueError, match="n_groups"):
        vq.grouped_prepare(torch.zeros(300 * 32, 32, device="cuda"), 300, 32)
    with pytest.raises(ValueError, match="x_id"):
        vq.align_groups(torch.tensor([[0, 5, 2]], device="cuda"), torch.zeros(1, 4, dtype=torch.int32, device="cuda"), 5)
    m = Bottleneck(4, 32, 32, 0.99, 1.0).cuda().eval()
    with pytest.raises(ValueError, match="x_id"):
        m(torch.zeros(1, 4, 32, device="cuda"), torch.tensor([[4]], device="cuda"), torch.zeros(1, 4, dtype=torch.int32, device="cuda"))
    # the C entry points refuse the same shapes themselves (status != 0, a message that names the argument, no launch)
    lib = native.lib()
    assert lib.smt_vq_grouped_prep_bytes(2, 48, 64) == 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    rc = lib.smt_vq_grouped_prepare(native.ptr(x), 2, 48, 64, native.ptr(buf), buf.numel(), native.stream_ptr())
    assert rc != 0 and b"l_bins" in lib.smt_last_error()
    rc = lib.smt_vq_grouped_prepare(native.ptr(x), 2, 32, 48, native.ptr(buf), buf.numel(), native.stream_ptr())
    assert rc != 0 and b"dim" in lib.smt_last_error()
    with pytest.raises(RuntimeError, match="k_bins"):
        vq.ema_accumulate(x, g.long(), None, (1 << 18) + 1, torch.zeros(16, device="cuda"))
