"""The VQTTS text-audio alignment on the device (csrc/vqtts_align.hip, smt_amd.vqtts, models.vqtts.align):

1. the dense distance against float64;
2. the fused search against the dense chain distance -> smt_maximum_path -> align_index, bit for bit, at the kernel's own
   constants +- 1 and at degenerate lengths;
3. lattices the dense search refuses (Tq = 20,000 and 32,768) against the numpy oracle and, independently of any product
   arithmetic, against the float64 optimum;
4. the loss on the path and its gradients against float64 autograd;
5. the module feeding the grouped bottleneck, align_gather and length_loss as is;
6. the argument limits.

u = 2^-24 below.  Error bounds: one distance is D subtractions (u each, relative), D fmaf accumulations of non-negative
terms and one square root, so its relative error is within (D + 3) u; sums of n non-negative terms add n u.
"""
import numpy as np
import pytest
import torch

from oracle import mas_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SENTINEL = 1.0e6          # large and finite: its squares summed over 256 channels stay far below fp32's range


def _inputs(b, tx, tq, d, x_lens, q_lens, seed):
    """N(0,1) rows plus a per-token offset; frame j of an item sits near the token a linear ramp gives it, so the best
    path is neither trivial nor arbitrary."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, tx, d, generator=g) + 1.5 * torch.randn(b, tx, 1, generator=g)
    y = torch.randn(b, tq, d, generator=g)
    for i in range(b):
        xl, ql = max(int(x_lens[i]), 1), max(int(q_lens[i]), 1)
        tok = (torch.arange(tq) * xl // ql).clamp(max=tx - 1)
        y[i] += x[i, tok] * 0.7
    return x, y


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _mask(x_lens, q_lens, tx, tq):
    xl, ql = torch.as_tensor(x_lens), torch.as_tensor(q_lens)
    return ((torch.arange(tx)[None, :, None] < xl[:, None, None]) & (torch.arange(tq)[None, None, :] < ql[:, None, None])).float()


def _dist64(x, y):
    return ((x.double()[:, :, None, :] - y.double()[:, None, :, :]) ** 2).sum(-1).sqrt()


# ---- 1. distance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 128, 132, 256])
@pytest.mark.parametrize("tx,tq", [(1, 1), (65, 130), (200, 257)])
def test_distance_against_float64(d, tx, tq):
    from smt_amd import vqtts
    b = 2
    x, y = _inputs(b, tx, tq, d, [tx] * b, [tq] * b, seed=d + tx)
    y[0, tq - 1] = x[0, tx // 2]                       # a duplicated row: the distance there is exactly 0
    y[1, 0] = x[1, 0]
    x, y = x.to(DEV), y.to(DEV)
    got = vqtts.distance(x, y)
    ref = _dist64(x, y)
    err = (got.double() - ref).abs()
    bound = (d + 3) * U * ref + 2.0 ** -75
    worst = float((err / bound).max())
    print(f"\n[vqtts distance D={d} {tx}x{tq}] worst err / bound {worst:.3f}")
    assert got.shape == (b, tx, tq) and bool((err <= bound).all())
    assert got[0, tx // 2, tq - 1].item() == 0.0 and got[1, 0, 0].item() == 0.0


# ---- 2. fused = dense chain ------------------------------------------------------------------------------------------
def _dense_chain(x, y, x_lens, q_lens):
    from models.glow_tts.submodules import maximum_path
    from smt_amd import glow, vqtts
    dist = vqtts.distance(x, y)
    mask = _mask(x_lens, q_lens, x.shape[1], y.shape[1]).to(DEV)
    return glow.align_index(maximum_path(-dist, mask))


def _tq_cases():
    from smt_amd import vqtts
    edges = {1, 2500}
    for c in (vqtts.ALIGN_SLAB, vqtts.ALIGN_WALK, vqtts.ALIGN_CHUNK):      # 32, 64, 512: slab, walk step (= ballot word), chunk
        edges |= {c - 1, c, c + 1}
    return sorted(edges)


@pytest.mark.parametrize("lens", ["a", "b"])
@pytest.mark.parametrize("tx", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("tq", _tq_cases())
def test_fused_search_equals_dense_chain_bit_for_bit(tx, tq, lens):
    """Rows per ballot word 64 -> Tx 63 / 64 / 65; the fused kernel runs one row per thread at every Tx, so it has no
    other row boundary.  Every shape is within the dense search's LDS limit.  Two length sets of B = 5 together hold
    x_len = Tx, 1, 0 and q_len = 0, x_len, x_len - 1.  The fused call sees a large sentinel beyond the lengths, the dense
    chain does not: what lies there cannot move the result."""
    from smt_amd import vqtts
    assert 8 * ((tx + 3) // 4 * 4) + 16 * tq * ((tx + 63) // 64) <= 163776
    d, b = 32, 5
    m = min(tx, tq)
    if lens == "a":
        x_lens, q_lens = [tx, 1, 0, m, m], [tq, tq, tq, m, m - 1]
    else:
        x_lens, q_lens = [tx, tx, 1, max(m // 2, 1), 0], [tq, 0, 1, tq, 0]
    x, y = _inputs(b, tx, tq, d, x_lens, q_lens, seed=1000 * tx + tq)
    ref_idx, ref_dur = _dense_chain(x.to(DEV), y.to(DEV), x_lens, q_lens)
    xs, ys = x.clone(), y.clone()
    for i in range(b):
        xs[i, x_lens[i]:] = SENTINEL
        ys[i, q_lens[i]:] = -SENTINEL
    idx, dur = vqtts.align(xs.to(DEV), ys.to(DEV), _i32(x_lens), _i32(q_lens))
    assert idx.dtype == torch.int32 and idx.shape == (b, tq) and dur.shape == (b, tx)
    assert torch.equal(idx, ref_idx), [int((idx[i] != ref_idx[i]).sum()) for i in range(b)]
    assert torch.equal(dur, ref_dur)
    assert int(dur[0].sum()) == tq                                 # the full item aligns every frame


def test_fused_search_with_x_read_from_l2():
    """Tx = 200 at D = 256 does not fit in LDS beside the rest, so the kernel takes its other path (x_enc from L2)."""
    from smt_amd import vqtts
    b, tx, tq, d = 2, 200, 700, 256
    x_lens, q_lens = [200, 131], [700, 650]
    x, y = _inputs(b, tx, tq, d, x_lens, q_lens, seed=5)
    ref_idx, ref_dur = _dense_chain(x.to(DEV), y.to(DEV), x_lens, q_lens)
    idx, dur = vqtts.align(x.to(DEV), y.to(DEV), _i32(x_lens), _i32(q_lens))
    assert torch.equal(idx, ref_idx) and torch.equal(dur, ref_dur)


# ---- 3. long lattices ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tq", [20000, 32768])
def test_long_lattice_against_the_oracle_and_the_float64_optimum(tq):
    from models.glow_tts.submodules import maximum_path
    from smt_amd import vqtts
    b, tx, d = 2, 130, 128
    x_lens, q_lens = [130, 97], [tq, tq - 1234]
    x, y = _inputs(b, tx, tq, d, x_lens, q_lens, seed=tq)
    xd, yd = x.to(DEV), y.to(DEV)
    dist = vqtts.distance(xd, yd)
    mask = _mask(x_lens, q_lens, tx, tq)
    with pytest.raises(RuntimeError, match="LDS"):                 # the reason the fused search exists
        maximum_path(-dist, mask.to(DEV))
    idx, dur = vqtts.align(xd, yd, _i32(x_lens), _i32(q_lens))
    idx, dur = idx.cpu().numpy(), dur.cpu().numpy()
    # (a) the numpy search on the product's own distance matrix, bit for bit
    path = mas_oracle.maximum_path((-dist).cpu().numpy(), mask.numpy())
    ref_idx = np.where(path.sum(1) > 0, path.argmax(1), -1).astype(np.int32)
    assert np.array_equal(idx, ref_idx) and np.array_equal(dur, path.sum(2))
    del path
    # (b) independent of the product's arithmetic: shape of the path, and its float64 score against the float64 optimum
    d64 = torch.cdist(xd.double(), yd.double(), compute_mode="donot_use_mm_for_euclid_dist").cpu().numpy()
    for i in range(b):
        xl, ql = x_lens[i], q_lens[i]
        p = idx[i, :ql].astype(np.int64)
        assert (idx[i, ql:] == -1).all() and p[0] == 0 and p[-1] == xl - 1
        steps = np.diff(p)
        assert ((steps == 0) | (steps == 1)).all()
        assert (np.bincount(p, minlength=xl) >= 1).all() and dur[i, xl:].sum() == 0
        cost = d64[i, :xl, :ql]
        score = cost[p, np.arange(ql)].sum()
        v = np.full(xl, np.inf)
        v[0] = cost[0, 0]
        for j in range(1, ql):                                     # min-cost monotonic path from (0, 0) to (xl - 1, ql - 1)
            v[1:] = np.minimum(v[1:], v[:-1])
            v += cost[:, j]
        bound = 2 * tq * (tq + d + 3) * U * cost.max()
        print(f"\n[vqtts long Tq={tq} item {i}] score - optimum {score - v[-1]:.3e} (bound {bound:.3e}, optimum {v[-1]:.3f})")
        assert 0 <= score - v[-1] + 1e-9 * v[-1] and score - v[-1] <= bound


# ---- 4. loss and gradients -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,tx,tq,d", [(3, 37, 301, 128), (2, 5, 70, 12)])
def test_loss_and_gradients_against_float64(b, tx, tq, d):
    from smt_amd import vqtts
    g = torch.Generator().manual_seed(d)
    x_lens = [tx, max(tx // 2, 1), tx][:b]
    q_lens = [tq, tq - 17, max(tx // 2, 1)][:b]                    # the last item (b = 3) has fewer frames than tokens
    x, y = _inputs(b, tx, tq, d, x_lens, q_lens, seed=d + 1)
    idx = torch.full((b, tq), -1, dtype=torch.int32)
    for i in range(b):
        ql = q_lens[i]
        idx[i, :ql] = torch.sort(torch.randint(0, x_lens[i], (ql,), generator=g)).values.to(torch.int32)   # some tokens get no frame
    j0 = 11
    y[0, j0] = x[0, idx[0, j0]]                                    # a planted frame at distance exactly 0
    denom = torch.tensor(float(sum(a * c for a, c in zip(x_lens, q_lens))))
    gscale = 1.75

    def run():
        xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
        loss = vqtts.align_loss(xd, yd, idx.to(DEV), denom.to(DEV))
        (gscale * loss).backward()
        return loss.detach(), xd.grad, yd.grad
    loss, dx, dy = run()
    loss2, dx2, dy2 = run()
    assert torch.equal(loss, loss2) and torch.equal(dx, dx2) and torch.equal(dy, dy2)       # fixed order: equal bits
    # float64 autograd of the reference formula restricted to the path, clamp-free sqrt on cells with dist > 0
    x64, y64 = x.double().to(DEV).requires_grad_(True), y.double().to(DEV).requires_grad_(True)
    idl = idx.to(DEV).long()
    xg = torch.gather(x64, 1, idl.clamp(min=0)[:, :, None].expand(-1, -1, d))
    d2 = ((y64 - xg) ** 2).sum(-1)
    valid = (idl >= 0) & (d2 > 0)
    ref = d2[valid].sqrt().sum() / denom.double().to(DEV)
    (gscale * ref).backward()
    n = int(valid.sum())
    coef = gscale / float(denom)
    print(f"\n[vqtts loss D={d}] loss {loss.item():.7f} ref {ref.item():.7f} rel {abs(loss.item() - ref.item()) / ref.item():.2e} "
          f"(bound {(n + d + 3) * U:.2e})")
    assert abs(loss.double().item() - ref.item()) <= (n + d + 3) * U * ref.item()
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dy).all())
    err_y = (dy.double() - y64.grad).abs().max().item()
    print(f"[vqtts loss D={d}] dy worst {err_y:.3e} (bound {(d + 6) * U * coef:.3e})")
    assert err_y <= (d + 6) * U * coef
    n_i = torch.zeros(b, tx, device=DEV, dtype=torch.float64)
    n_i.scatter_add_(1, idl.clamp(min=0), (idl >= 0).double())
    bound_x = ((d + 6 + n_i) * U * n_i * coef)[:, :, None]
    err_x = (dx.double() - x64.grad).abs()
    print(f"[vqtts loss D={d}] dx worst err / bound {(err_x / bound_x.clamp(min=1e-300)).max().item():.3f}")
    assert bool((err_x <= bound_x).all())
    assert bool((dy[0, j0] == 0).all())                            # the planted frame: exactly 0, no NaN
    assert bool((dy[(idx < 0).to(DEV)] == 0).all())                # frames without a token
    # the planted frame adds nothing to its token's gradient either: dx equals the sum over the other frames (checked above
    # against float64, whose sum leaves the frame out)


# ---- 5. module -------------------------------------------------------------------------------------------------------
def test_module_feeds_bottleneck_gather_and_length_loss():
    """The issue names Bottleneck(n_vocab = 5, l_bins = 8, emb_width = 16); the grouped search takes emb_width in
    {32, 64, 128} and l_bins a multiple of 32, so the smallest shape it accepts stands in: l_bins = 32, emb_width = 32."""
    from models.vqtts import Bottleneck, TextAudioAlignment
    from smt_amd import glow
    torch.manual_seed(3)
    b, tx, tq, d, n_vocab = 3, 9, 120, 32, 5
    x_lens_l, q_lens_l = [9, 4, 7], [120, 77, 5]                   # the last item has fewer frames than tokens
    x, y = _inputs(b, tx, tq, d, x_lens_l, q_lens_l, seed=9)
    x_enc, y_enc = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    x_lens, q_lens = _i32(x_lens_l), _i32(q_lens_l)
    align = TextAudioAlignment()
    align_idx, durations, loss_align = align(x_enc, x_lens, y_enc, q_lens)
    assert align_idx.dtype == torch.int32 and align_idx.shape == (b, tq) and durations.shape == (b, tx)
    assert not align_idx.requires_grad and not durations.requires_grad
    assert durations.sum(1).tolist() == [float(q) for q in q_lens_l]          # every frame inside q_len has one token
    dist = ((x_enc.detach()[:, :, None] - y_enc.detach()[:, None]) ** 2).sum(-1).sqrt()
    on_path = torch.gather(dist, 1, align_idx.long().clamp(min=0)[:, None, :])[:, 0] * (align_idx >= 0)
    want = on_path.sum() / sum(a * c for a, c in zip(x_lens_l, q_lens_l))
    assert torch.isclose(loss_align.detach(), want, rtol=1e-5)
    # consumers, without conversion
    m = Bottleneck(n_vocab, 32, d, 0.99, 1.0).cuda().train()
    x_id = torch.randint(0, n_vocab, (b, tx), device=DEV)
    q_rel, y_d, commit, _ = m(y_enc, x_id, align_idx)
    assert q_rel.shape == (b, tq) and y_d.shape == (b, tq, d)
    x_exp = glow.align_gather(x_enc, align_idx)
    assert torch.equal(x_exp.detach()[0, 5], x_enc.detach()[0, align_idx[0, 5]]) and bool((x_exp[1, 77:] == 0).all())
    logw = torch.zeros(b, tx, device=DEV, requires_grad=True)
    l_len = glow.length_loss(logw, durations, x_lens, x_lens.sum().float())
    ref_len = sum(((torch.log(1e-8 + durations[i, :n])) ** 2).sum() for i, n in enumerate(x_lens_l)) / sum(x_lens_l)
    assert torch.isclose(l_len.detach(), ref_len, rtol=1e-5)
    (loss_align + commit + l_len + x_exp.sum() * 0).backward()
    assert x_enc.grad is not None and y_enc.grad is not None
    assert bool(torch.isfinite(x_enc.grad).all()) and bool(torch.isfinite(y_enc.grad).all())
    assert float(x_enc.grad.abs().sum()) > 0 and float(y_enc.grad.abs().sum()) > 0
    assert bool((y_enc.grad[1, 77:] == 0).all()) and bool((x_enc.grad[1, 4:] == 0).all())   # nothing past the lengths


# ---- 6. arguments ----------------------------------------------------------------------------------------------------
def test_limits_raise_and_name_the_limit():
    from smt_amd import vqtts
    lens = _i32([1])

    def call(tx, tq, d):
        return vqtts.align(torch.zeros(1, tx, d, device=DEV), torch.zeros(1, tq, d, device=DEV), lens, lens)
    with pytest.raises(RuntimeError, match=r"dim=6 .*multiple of 4 up to 256"):
        call(4, 4, 6)
    with pytest.raises(RuntimeError, match=r"t_x=513 .*limit of 512"):
        call(513, 4, 8)
    with pytest.raises(RuntimeError, match=r"t_q=32769 .*limit of 32768"):
        call(4, 32769, 8)
    with pytest.raises(RuntimeError, match=r"dim=260"):
        vqtts.distance(torch.zeros(1, 2, 260, device=DEV), torch.zeros(1, 2, 260, device=DEV))
    e = torch.zeros(0, dtype=torch.int32, device=DEV)
    idx, dur = vqtts.align(torch.zeros(0, 7, 8, device=DEV), torch.zeros(0, 11, 8, device=DEV), e, e)
    assert idx.shape == (0, 11) and idx.dtype == torch.int32 and dur.shape == (0, 7)
    assert vqtts.distance(torch.zeros(0, 7, 8, device=DEV), torch.zeros(0, 11, 8, device=DEV)).shape == (0, 7, 11)
