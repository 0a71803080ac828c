"""The VQTTS code head on the device (csrc/vqtts_codes.hip, smt_amd.vqtts.code_head, models.vqtts.CodePredictor) against
float64: ``F.linear`` + ``F.cross_entropy`` in float64 on the same inputs.

The error bound is derived, not fitted.  Per row r, S_r = max_v (sum_c |h_rc||W_vc| + |b_v|) and
e_r = 2^-15 S_r + 2^-20 (1 + |lse_r|), both in float64:
  * the bf16-pair split leaves at most 3 * 2^-18 sum |h||W| per logit (the dropped lo.lo term and two representation residues);
  * fp32 accumulation over C <= 256 adds at most 2^-16 sum |h||W|;
  * the last term covers expf / logf.
A logit is within e_r, so is lse (a maximum and a log-sum-exp are 1-Lipschitz in the sup norm), row_loss = lse - logit[t] within
2 e_r, and p = exp(logit - lse) within a relative 2 e_r.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _inputs(n, c, v, seed, unscored=0.1):
    """h ~ N(0, 1), W and b ~ U(+-1/sqrt(C)) (nothing symmetric under a row/column swap), a tenth of the targets -1."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, c, generator=g)
    w = (torch.rand(v, c, generator=g) * 2 - 1) / c ** 0.5
    b = (torch.rand(v, generator=g) * 2 - 1) / c ** 0.5
    t = torch.randint(0, v, (n,), generator=g)
    t[torch.rand(n, generator=g) < unscored] = -1
    return h.to(DEV), w.to(DEV), b.to(DEV), t.to(DEV)


class Ref:
    """float64 reference of one case and the bound e_r, computed once."""

    def __init__(self, h, w, b, t, grads=False):
        h64, w64, b64 = (x.double().detach().clone().requires_grad_(grads) for x in (h, w, b))
        self.logits = F.linear(h64, w64, b64)
        self.lse = torch.logsumexp(self.logits, -1).detach()
        self.row_loss = F.cross_entropy(self.logits, t, ignore_index=-1, reduction="none").detach()
        self.scored = t >= 0
        self.count = int(self.scored.sum())
        self.loss = self.row_loss.sum() / max(self.count, 1)
        s = (F.linear(h64.detach().abs(), w64.detach().abs(), b64.detach().abs())).max(-1).values
        self.e = 2.0 ** -15 * s + 2.0 ** -20 * (1 + self.lse.abs())
        self.t = t
        if grads:
            (F.cross_entropy(self.logits, t, ignore_index=-1, reduction="sum") / max(self.count, 1)).backward()
            self.dh, self.dw, self.db = h64.grad, w64.grad, b64.grad
            p = torch.softmax(self.logits.detach(), -1)
            onehot = F.one_hot(t.clamp(min=0), w.shape[0]).double()
            self.ghat = (p + onehot) * self.scored[:, None] / max(self.count, 1)
            self.h, self.w = h64.detach(), w64.detach()
        self.logits = self.logits.detach()


def _rows(h, w, b, t):
    """The per-row results of the forward (lse, row_loss, pred, correct) and the three sums (float64)."""
    from smt_amd import vqtts
    with torch.no_grad():
        _, _, _, _, _, lse, row_loss, correct, sums, pred = vqtts._head_fwd(h, w, b, t, True)
    return lse, row_loss, pred, correct, sums[:3]


def _check_pred(pred, ref, limit=0.02):
    top2 = ref.logits.topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * ref.e
    am = ref.logits.argmax(-1)
    assert torch.equal(pred.long()[clear], am[clear]), "pred differs from the float64 argmax on a row with a clear gap"
    got = ref.logits.gather(1, pred.long()[:, None])[:, 0]
    assert bool((got >= top2[:, 0] - 2 * ref.e).all()), "pred is not within 2 e_r of the maximum"
    share = 1.0 - clear.double().mean().item()
    print(f"near-tie rows: {share:.4%}")
    assert share <= limit, f"{share:.3%} of the rows have a float64 top-two gap within 2 e_r"


def _check_forward(h, w, b, t, pred_limit=0.02):
    from smt_amd import vqtts
    ref = Ref(h, w, b, t)
    lse, row_loss, pred, correct, sums = _rows(h, w, b, t)
    loss, acc, count, pred2 = vqtts.code_head(h, w, b, t)
    torch.cuda.synchronize()
    for x in (lse, row_loss, loss, acc):
        assert bool(torch.isfinite(x).all())
    d_lse = ((lse.double() - ref.lse).abs() / ref.e).max().item()
    d_row = ((row_loss.double() - ref.row_loss).abs() / (2 * ref.e)).max().item()
    print(f"n={h.shape[0]} c={h.shape[1]} v={w.shape[0]}: max |lse - lse64| / e_r = {d_lse:.4f}, max |row_loss - ref| / 2 e_r = {d_row:.4f}")
    assert d_lse <= 1.0 and d_row <= 1.0
    assert bool((row_loss[~ref.scored] == 0).all()), "an unscored row has a loss"
    assert int(count) == ref.count and count.dtype == torch.int64 and int(sums[2].item()) == ref.count
    tol = (2 * ref.e).sum().item() / h.shape[0] + 2.0 ** -20 * abs(ref.loss.item())
    print(f"  |loss - loss64| = {abs(loss.item() - ref.loss.item()):.3e} (bound {tol:.3e})")
    assert abs(loss.item() - ref.loss.item()) <= tol
    assert torch.equal(pred, pred2) and pred.dtype == torch.int32
    want_acc = (pred.long() == t)[ref.scored].double().mean().item() if ref.count else 0.0
    assert abs(acc.item() - want_acc) <= 2.0 ** -23 * want_acc
    assert torch.equal(correct, ((pred.long() == t) & ref.scored).float())
    _check_pred(pred, ref, pred_limit)
    assert torch.equal(vqtts.code_head_predict(h, w, b), pred), "the synthesis form gives another argmax"
    return ref


# ---- forward ----------------------------------------------------------------------------------------------------------
# a single near-tie row is more than 2 % of fewer than 50 rows: the seeds below give none at those sizes (a property of the
# float64 reference alone), and the limit is asserted at every size
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 257])
def test_forward_rows(n):
    _check_forward(*_inputs(n, 128, 512, seed=100 + n))


@pytest.mark.parametrize("c,v", [(c, v) for c in (16, 64, 256) for v in (32, 96, 1024)])
def test_forward_widths(c, v):
    _check_forward(*_inputs(257, c, v, seed=c + v))


def test_forward_across_weight_gradient_slices():
    from smt_amd import vqtts
    _check_forward(*_inputs(3 * vqtts.CH_SLICE + 5, 128, 512, seed=5))


@pytest.mark.parametrize("lo,hi", [(3, 4), (4, 8), (37, 300), (0, 511)])
def test_ties_go_to_the_lowest_index(lo, hi):
    """Two identical weight rows with identical biases win on every row: every logit is computed by the same instruction
    sequence whatever its column, so they tie exactly and the lower index is returned -- within a lane's registers, across
    the two lane halves (rows 4..7 of a 32-row chunk sit in the upper half) and across staged tiles."""
    from smt_amd import vqtts
    h, w, b, t = _inputs(65, 128, 512, seed=lo + hi)
    w[hi] = w[lo]
    b[lo] = b[hi] = 30.0
    pred = vqtts.code_head_predict(h, w, b)
    assert bool((pred == lo).all())
    ref = Ref(h, w, b, t)
    lse, row_loss, pred2, _, _ = _rows(h, w, b, t)
    assert torch.equal(pred2, pred)
    assert bool(((lse.double() - ref.lse).abs() <= ref.e).all()) and bool(((row_loss.double() - ref.row_loss).abs() <= 2 * ref.e).all())


def test_large_logits_stay_stable():
    h, w, b, t = _inputs(257, 128, 512, seed=9)
    h *= 60.0 / F.linear(h.double(), w.double()).abs().max().item()
    b[77] += 80.0
    ref = _check_forward(h, w, b, t)
    assert ref.logits.abs().max().item() > 59.0 and ref.lse.max().item() > 20.0


def test_all_rows_unscored():
    from smt_amd import vqtts
    h, w, b, t = _inputs(130, 128, 512, seed=11)
    t.fill_(-1)
    h.requires_grad_(True); w.requires_grad_(True); b.requires_grad_(True)
    loss, acc, count, pred = vqtts.code_head(h, w, b, t)
    assert loss.item() == 0.0 and acc.item() == 0.0 and int(count) == 0
    loss.backward()
    for g in (h.grad, w.grad, b.grad):
        assert bool(torch.isfinite(g).all()) and bool((g == 0).all()), "a gradient of an unscored batch is not zero"
    assert pred.shape == (130,)


# ---- backward ---------------------------------------------------------------------------------------------------------
def _grads(h, w, b, t):
    from smt_amd import vqtts
    hd, wd, bd = (x.detach().clone().requires_grad_(True) for x in (h, w, b))
    loss, _, _, _ = vqtts.code_head(hd, wd, bd, t)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), hd.grad, wd.grad, bd.grad


def _check_backward(n, c, v, seed):
    h, w, b, t = _inputs(n, c, v, seed)
    ref = Ref(h, w, b, t, grads=True)
    loss, dh, dw, db = _grads(h, w, b, t)
    e, emax = ref.e, ref.e.max()
    bh = (2 * e + 2.0 ** -15)[:, None] * (ref.ghat @ ref.w.abs())
    bw = (2 * emax + 2.0 ** -15) * (ref.ghat.t() @ ref.h.abs())
    bb = (2 * emax + 2.0 ** -20) * ref.ghat.sum(0)
    tiny = 1e-300
    r_h = ((dh.double() - ref.dh).abs() / (bh + tiny)).max().item()
    r_w = ((dw.double() - ref.dw).abs() / (bw + tiny)).max().item()
    r_b = ((db.double() - ref.db).abs() / (bb + tiny)).max().item()
    print(f"n={n} c={c} v={v}: error / bound: dh {r_h:.4f}, dW {r_w:.4f}, db {r_b:.4f}")
    assert bool(((dh.double() - ref.dh).abs() <= bh).all()), f"dh: error / bound = {r_h}"
    assert bool(((dw.double() - ref.dw).abs() <= bw).all()), f"dW: error / bound = {r_w}"
    assert bool(((db.double() - ref.db).abs() <= bb).all()), f"db: error / bound = {r_b}"
    assert bool((dh[~ref.scored] == 0).all()), "dh of an unscored row is not exactly 0"
    # determinism: equal inputs, equal bits
    loss2, dh2, dw2, db2 = _grads(h, w, b, t)
    assert torch.equal(loss, loss2) and torch.equal(dh, dh2) and torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 257])
def test_backward_rows(n):
    _check_backward(n, 128, 512, seed=200 + n)


@pytest.mark.parametrize("c,v", [(c, v) for c in (16, 64, 256) for v in (32, 96, 1024)])
def test_backward_widths(c, v):
    _check_backward(257, c, v, seed=2 * c + v)


def test_backward_across_weight_gradient_slices():
    """Three full row slices of the weight-gradient kernel and a ragged tail: four slabs, added in slice order."""
    from smt_amd import vqtts
    _check_backward(3 * vqtts.CH_SLICE + 5, 128, 512, seed=6)


def test_logits_are_never_materialised():
    from smt_amd import vqtts
    n, c, v = 32768, 128, 512
    h, w, b, t = _inputs(n, c, v, seed=12)
    h.requires_grad_(True); w.requires_grad_(True); b.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, _, _, _ = vqtts.code_head(h, w, b, t)
    loss.backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"peak above entry: {extra / 2 ** 20:.1f} MiB (logits would be {n * v * 4 / 2 ** 20:.0f} MiB)")
    assert extra < n * v * 4


def test_backward_past_the_most_slices():
    """Just over CH_MAX_SLICES * CH_SLICE rows the slices grow instead of their number (a multiple of 128 rows each, a ragged
    last one), and the forward's reduce runs with every partial sum in use."""
    from smt_amd import vqtts
    _check_backward(vqtts.CH_MAX_SLICES * vqtts.CH_SLICE + 77, 16, 32, seed=7)


def test_no_rows():
    from smt_amd import vqtts
    h, w, b, t = _inputs(0, 128, 512, seed=13)
    h.requires_grad_(True); w.requires_grad_(True); b.requires_grad_(True)
    loss, acc, count, pred = vqtts.code_head(h, w, b, t)
    assert loss.item() == 0.0 and acc.item() == 0.0 and int(count) == 0 and pred.shape == (0,)
    loss.backward()
    assert h.grad.shape == (0, 128) and not bool(w.grad.any()) and not bool(b.grad.any())
    assert vqtts.code_head_predict(h.detach().reshape(2, 0, 128), w, b).shape == (2, 0)


# ---- the cached weight split follows the weight --------------------------------------------------------------------------
def _check_loss(loss, h, w, b, t):
    ref = Ref(h, w, b, t)
    tol = (2 * ref.e).mean().item() + 2.0 ** -20 * abs(ref.loss.item())
    print(f"|loss - loss64| = {abs(loss.item() - ref.loss.item()):.3e} (bound {tol:.3e})")
    assert abs(loss.item() - ref.loss.item()) <= tol
    return ref


def test_split_follows_an_in_place_write():
    from smt_amd import vqtts
    h, w, b, t = _inputs(257, 128, 512, seed=14)
    split = vqtts.WeightSplit()
    _check_loss(vqtts.code_head(h, w, b, t, split=split)[0], h, w, b, t)
    buf = split.buf
    _check_loss(vqtts.code_head(h, w, b, t, split=split)[0], h, w, b, t)
    assert split.buf is buf
    w.mul_(-1.5)                                                  # moves _version
    ref = _check_loss(vqtts.code_head(h, w, b, t, split=split)[0], h, w, b, t)
    _check_pred(vqtts.code_head_predict(h, w, b, split=split), ref)


def test_split_follows_a_fused_optimizer_step():
    """A fused AdamW step writes the weight without moving its _version: the split is redone all the same."""
    from smt_amd import vqtts
    h, w, b, t = _inputs(257, 128, 512, seed=15)
    w.requires_grad_(True)
    split = vqtts.WeightSplit()
    opt = torch.optim.AdamW([w], lr=0.05, fused=True)
    before = w.detach().clone()
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        vqtts.code_head(h, w, b, t, split=split)[0].backward()
        opt.step()
    assert (w.detach() - before).abs().max().item() > 0.05
    with torch.no_grad():
        ref = _check_loss(vqtts.code_head(h, w, b, t, split=split)[0], h, w.detach(), b, t)
        _check_pred(vqtts.code_head_predict(h, w, b, split=split), ref)


def test_module_eval_after_a_fused_optimizer_step():
    """Training forward, fused AdamW step, eval forward (a validation pass): loss and pred are those of the new weights."""
    m, x_enc, idx, q_lens, target = _module()
    opt = torch.optim.AdamW(m.parameters(), lr=0.05, fused=True)
    m.eval()
    with torch.no_grad():
        m(x_enc, idx, q_lens, target)                             # an eval pass before: the split is cached
    m.train()
    loss, _, _ = m(x_enc, idx, q_lens, target, drop_seed=1)
    loss.backward()
    before = m.quant_proj.weight.detach().clone()
    opt.step()
    assert (m.quant_proj.weight.detach() - before).abs().max().item() > 0.01
    m.eval()
    with torch.no_grad():
        hid, valid = m.hidden(x_enc, idx, q_lens)
        loss, _, pred = m(x_enc, idx, q_lens, target)
        t = torch.where(valid & (idx >= 0), target, torch.full_like(target, -1)).reshape(-1)
        ref = _check_loss(loss, hid.reshape(-1, C), m.quant_proj.weight.reshape(V, C), m.quant_proj.bias, t)
        _check_pred(pred.reshape(-1), ref)
        assert torch.equal(m(x_enc, idx, q_lens), pred)


# ---- limits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,v,what", [(24, 512, "multiple of 16"), (128, 48, "multiple of 32"), (128, 2048, "up to 1024")])
def test_limits_are_named(c, v, what):
    from smt_amd import vqtts
    h = torch.zeros(8, c, device=DEV)
    w, b = torch.zeros(v, c, device=DEV), torch.zeros(v, device=DEV)
    with pytest.raises(RuntimeError, match=what):
        vqtts.code_head_predict(h, w, b)
    with pytest.raises(RuntimeError, match=what):
        vqtts.code_head(h, w, b, torch.zeros(8, dtype=torch.int64, device=DEV))


# ---- module -----------------------------------------------------------------------------------------------------------
B, TX, TQ, C, V = 2, 7, 70, 64, 96
X_LENS, Q_LENS = [7, 5], [70, 53]


def _module(seed=3):
    from models.vqtts import CodePredictor
    torch.manual_seed(seed)
    m = CodePredictor(C, V).to(DEV)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if ".model.5." in name:                               # zero-initialised: give the second conv something to do
                p.copy_(((torch.rand(p.shape, generator=g) * 2 - 1) / (2 * C) ** 0.5).to(DEV))
    x_enc = torch.randn(B, TX, C, generator=g).to(DEV)
    idx = torch.full((B, TQ), -1, dtype=torch.int32)
    for i in range(B):
        idx[i, :Q_LENS[i]] = (torch.arange(Q_LENS[i]) * X_LENS[i] // Q_LENS[i]).to(torch.int32)
    q_lens = torch.tensor(Q_LENS, dtype=torch.int32, device=DEV)
    target = torch.randint(0, V, (B, TQ), generator=g).to(DEV)
    return m, x_enc, idx.to(DEV), q_lens, target


def _stack64(m, x_enc, idx, q_lens):
    """The residual stack restated in float64 with F.conv1d (eval mode: no dropout)."""
    sd = {k: p.detach().double() for k, p in m.state_dict().items()}
    x = torch.where((idx >= 0)[..., None], torch.gather(x_enc.double(), 1, idx.clamp(min=0).long()[..., None].expand(-1, -1, C)), 0.0)
    mask = (torch.arange(TQ, device=DEV)[None, :] < q_lens[:, None])[..., None].double()
    for i, dil in enumerate([27, 9, 3, 1]):
        x = x * mask
        u = F.conv1d(torch.relu(x).transpose(1, 2), sd[f"quant_decoder.model.{i}.model.2.weight"],
                     sd[f"quant_decoder.model.{i}.model.2.bias"], padding=dil, dilation=dil)
        u = torch.relu(u) * mask.transpose(1, 2)
        x = x + F.conv1d(u, sd[f"quant_decoder.model.{i}.model.5.weight"], sd[f"quant_decoder.model.{i}.model.5.bias"]).transpose(1, 2)
    return x * mask


def test_module_eval_against_float64():
    m, x_enc, idx, q_lens, target = _module()
    m.eval()
    with torch.no_grad():
        hid, valid = m.hidden(x_enc, idx, q_lens)
        ref = _stack64(m, x_enc, idx, q_lens)
        err, scale = (hid.double() - ref).abs().max().item(), ref.abs().max().item()
        print(f"stack: max-abs error {err:.3e}, max {scale:.3e}")
        assert err <= 2e-5 * scale + 1e-12                        # the fp32-conv tolerance of tests/test_glow_kernels_gpu.py
        assert bool((hid[~valid] == 0).all())
        loss, acc, pred = m(x_enc, idx, q_lens, target)
        t = torch.where(valid & (idx >= 0), target, torch.full_like(target, -1)).reshape(-1)
        w, b = m.quant_proj.weight.reshape(V, C), m.quant_proj.bias
        r = Ref(hid.reshape(-1, C), w, b, t)                     # the head's bounds on the stack's own output
        assert abs(loss.item() - r.loss.item()) <= (2 * r.e).mean().item() + 2.0 ** -20 * abs(r.loss.item())
        _check_pred(pred.reshape(-1), r)
        assert torch.equal(m(x_enc, idx, q_lens), pred) and pred.shape == (B, TQ)
        assert abs(acc.item() - (pred.reshape(-1).long() == t)[t >= 0].double().mean().item()) < 1e-6


def test_module_training_gradients_and_seeds():
    m, x_enc, idx, q_lens, target = _module()
    m.train()
    x_enc.requires_grad_(True)

    def run(seed):
        m.zero_grad(set_to_none=True)
        loss, _, _ = m(x_enc, idx, q_lens, target, drop_seed=seed)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}

    l1, g1 = run(5)
    assert x_enc.grad is None, "x_enc is detached: no gradient may reach it"
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), f"no gradient reached {k}"
    l2, g2 = run(5)
    assert torch.equal(l1, l2) and all(torch.equal(g1[k], g2[k]) for k in g1), "equal drop_seed, different bits"
    l3, g3 = run(6)
    assert not torch.equal(l1, l3) and any(not torch.equal(g1[k], g3[k]) for k in g1), "another drop_seed, the same result"


def test_synthesize_codes_round_trips_through_the_bottleneck():
    from models.vqtts import Bottleneck, CodePredictor
    g = torch.Generator().manual_seed(8)
    n_vocab, l_bins, d, b, tx, t = 9, 64, 32, 2, 6, 50
    bn = Bottleneck(n_vocab, l_bins, d, 0.99, 1.0).to(DEV).eval()
    with torch.no_grad():
        bn.k.copy_(torch.randn(n_vocab * l_bins, d, generator=g).to(DEV))
    y = torch.randn(b, t, d, generator=g).to(DEV)
    x_id = torch.randint(0, n_vocab, (b, tx), generator=g).to(DEV)
    idx = torch.full((b, t), -1, dtype=torch.int32)
    idx[0] = (torch.arange(t) * tx // t).to(torch.int32)
    idx[1, :31] = (torch.arange(31) * 4 // 31).to(torch.int32)
    idx = idx.to(DEV)
    q_rel, q_abs = bn.encode(y, x_id, idx)
    q = CodePredictor(d, l_bins).synthesize_codes(q_rel, x_id, idx)
    has = idx >= 0
    assert torch.equal(q[has], q_abs.long()[has])
    assert torch.equal(bn.decode(q)[has], bn.k[q_abs.long()[has]])


def test_reference_checkpoint_loads_strictly():
    from models.vqtts import CodePredictor
    g = torch.Generator().manual_seed(4)
    sd = {}
    for i in range(4):
        sd[f"quant_decoder.model.{i}.model.2.weight"] = torch.randn(2 * C, C, 3, generator=g)
        sd[f"quant_decoder.model.{i}.model.2.bias"] = torch.randn(2 * C, generator=g)
        sd[f"quant_decoder.model.{i}.model.5.weight"] = torch.randn(C, 2 * C, 1, generator=g)
        sd[f"quant_decoder.model.{i}.model.5.bias"] = torch.randn(C, generator=g)
    sd["quant_proj.weight"], sd["quant_proj.bias"] = torch.randn(V, C, 1, generator=g), torch.randn(V, generator=g)
    m = CodePredictor(C, V).to(DEV)
    m.load_state_dict(sd, strict=True)
    for k, p in m.state_dict().items():
        assert torch.equal(p.cpu(), sd[k])
