"""The TransformerLM's focal and MMI losses on the device (smt_lm_focal_* / smt_lm_mmi_*, smt_amd.lm.focal_loss / mmi_loss)
against the float64 reference of tests/lm_loss_helpers.py: the kernels alone, the model's train step, and the captured step.

Bounds.  Kernels: those of test_cross_entropy_kernel_masks_rows_and_breaks_ties_low (loss 1e-5 max(1, |loss|), accuracy and
count exact, gradient atol 1e-7 / rtol 1e-4) plus a relative L2 of 1e-4 over the whole gradient
(lm_loss_helpers.check_against_reference).  Model: those of test_small_model_train_mode_with_dropout_matches_the_oracle
(loss 2e-5 max(1, |loss|), accuracy 1e-6, gradients 1e-3 relative L2).  Capture: loss bit for bit, gradients 2e-6 relative."""
import math

import pytest
import torch

import lm_loss_helpers as H
from oracle import lm_oracle as lmo
from test_lm_gpu import DEV, SMALL, _build, rel

pytestmark = pytest.mark.gpu

KINDS = [("focal", g) for g in H.GAMMAS] + [("mmi", None)]
KIND_IDS = [f"focal{g:g}" for g in H.GAMMAS] + ["mmi"]


def _op(kind, logits, target, gamma):
    from smt_amd import lm as K
    return K.focal_loss(logits, target, gamma) if kind == "focal" else K.mmi_loss(logits, target)


def _run(kind, logits, target, gamma):
    """(loss, accuracy, count, d(1.5 loss)/dlogits) of the device op."""
    lg = logits.to(DEV).requires_grad_(True)
    loss, acc, count = _op(kind, lg, target.to(DEV), gamma)
    assert not acc.requires_grad and not count.requires_grad
    (loss * H.UPSTREAM).backward()
    return loss.detach(), acc, count, lg.grad


def _raw(kind, logits, target, gamma, prefill=float("nan")):
    """The C entries themselves on buffers of the test's own, the backward with coef = 1.5 / count into a `prefill`-filled
    dlogits: every output of forward and backward, as a tuple of tensors."""
    from smt_amd import native as N
    lib = N.lib()
    rows, v = logits.shape
    lg, tg = logits.to(DEV).contiguous(), target.to(DEV)
    f32 = dict(device=DEV, dtype=torch.float32)
    row_out, lse = torch.full((rows, 2), prefill, **f32), torch.full((rows,), prefill, **f32)
    count = (tg >= 0).sum().to(torch.float32).reshape(1)
    coef = (H.UPSTREAM / count).contiguous()
    dlogits = torch.full((rows, v), prefill, **f32)
    if kind == "focal":
        row_coef = torch.full((rows,), prefill, **f32)
        N.check(lib.smt_lm_focal_fwd(N.ptr(lg), N.ptr(tg), N.ptr(row_out), N.ptr(lse), N.ptr(row_coef), rows, v, gamma, N.stream_ptr()), "fwd")
        N.check(lib.smt_lm_focal_bwd(N.ptr(lg), N.ptr(tg), N.ptr(lse), N.ptr(row_coef), N.ptr(coef), N.ptr(dlogits), rows, v,
                                     N.stream_ptr()), "bwd")
        return row_out, lse, row_coef, dlogits
    logm, ent = torch.full((v,), prefill, **f32), torch.full((1,), prefill, **f32)
    ws = torch.empty(lib.smt_lm_mmi_workspace_bytes(rows, v), device=DEV, dtype=torch.uint8)
    N.check(lib.smt_lm_mmi_fwd(N.ptr(lg), N.ptr(tg), N.ptr(count), N.ptr(row_out), N.ptr(lse), N.ptr(logm), N.ptr(ent), rows, v,
                               N.ptr(ws), ws.numel(), N.stream_ptr()), "fwd")
    N.check(lib.smt_lm_mmi_bwd(N.ptr(lg), N.ptr(tg), N.ptr(lse), N.ptr(logm), N.ptr(coef), N.ptr(dlogits), rows, v, N.stream_ptr()), "bwd")
    return row_out, lse, logm, ent, dlogits


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("rows,vocab", H.KERNEL_SHAPES)
@pytest.mark.parametrize("kind,gamma", KINDS, ids=KIND_IDS)
def test_loss_kernels_match_float64(kind, gamma, rows, vocab):
    ref = H.case_reference(kind, rows, vocab, gamma)
    logits, target = ref[0], ref[1]
    loss, acc, count, grad = _run(kind, logits, target, gamma)
    H.check_against_reference(loss, acc, count, grad, ref, f"{kind} gamma {gamma} [{rows}, {vocab}]")
    assert float(grad[(target < 0).to(DEV)].abs().sum()) == 0.0


@pytest.mark.parametrize("rows,vocab", [(5, 16), (41, 512), (1030, 64)])
def test_focal_at_gamma_zero_is_the_cross_entropy_kernel(rows, vocab):
    from smt_amd import lm as K
    logits, target = H.make_case(rows, vocab)
    loss, acc, count, grad = _run("focal", logits, target, 0.0)
    lg = logits.to(DEV).requires_grad_(True)
    ce, ce_acc, ce_count = K.cross_entropy(lg, target.to(DEV))
    (ce * H.UPSTREAM).backward()
    ref = (logits, target, float(ce.detach()), float(ce_acc), int(ce_count), lg.grad.double().cpu())
    H.check_against_reference(loss, acc, count, grad, ref, f"focal gamma 0 vs cross_entropy [{rows}, {vocab}]")


@pytest.mark.parametrize("kind,gamma", [("focal", 2.0), ("focal", 10.0), ("mmi", None)], ids=["focal2", "focal10", "mmi"])
def test_logits_scaled_by_30_do_not_overflow_and_empty_columns_weigh_nothing(kind, gamma):
    """Logits of spread 90 at (41, 512), without the planted uniform row (its 1 / vocab would reach every column): most fp32
    probabilities underflow to 0, and so do whole column means.  Everything stays finite; a column whose mean is 0 in fp32
    (float64 mean below 1e-50, far under the smallest fp32 denormal) gets logm = 0 and gradient exactly 0.
    Bounds: the logits reach |x| < 512 where a cross-entropy case stays under 16, so lse -- and with it every log-probability
    -- is held 32 times more coarsely (half an ulp: 2^-16 against 2^-21); the kernel bounds are widened by that factor."""
    ref = H.case_reference(kind, 41, 512, gamma, 30.0, False)
    logits, target, loss64, acc64, count64, grad64 = ref
    assert 256 < float(logits.abs().max()) < 512
    loss, acc, count, grad = _run(kind, logits, target, gamma)
    assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
    g = grad.double().cpu()
    worst = float(((g - grad64).abs() - 32 * (1e-7 + 1e-4 * grad64.abs())).max())
    print(f"{kind} gamma {gamma} x30: loss {float(loss):.9g} ref {loss64:.9g}; grad excess {worst:.3g} rel-L2 {H.rel_l2(g, grad64):.3g}")
    assert abs(float(loss) - loss64) <= 32 * 1e-5 * max(1.0, abs(loss64))
    assert abs(float(acc) - acc64) < 1e-7 and int(count) == count64
    assert worst <= 0.0 and H.rel_l2(g, grad64) <= 32 * 1e-4
    if kind == "mmi":
        keep = target >= 0
        mean64 = torch.softmax(logits.double()[keep], -1).mean(0)
        empty = mean64 < 1e-50
        assert 10 <= int(empty.sum()) < 512
        row_out, lse, logm, ent, dlogits = _raw(kind, logits, target, gamma)
        assert float(logm.cpu()[empty].abs().max()) == 0.0 and math.isfinite(float(ent)) and bool(torch.isfinite(logm).all())
        assert float(grad.cpu()[:, empty].abs().max()) == 0.0 and float(dlogits.cpu()[:, empty].abs().max()) == 0.0


@pytest.mark.parametrize("kind,gamma", [("focal", 2.0), ("mmi", None)], ids=["focal2", "mmi"])
def test_unscored_rows_get_exact_zeros_in_a_nan_prefilled_gradient(kind, gamma):
    logits, target = H.make_case(300, 96)
    out = _raw(kind, logits, target, gamma)
    dlogits, row_out = out[-1].cpu(), out[0].cpu()
    assert bool(torch.isfinite(dlogits).all()) and all(bool(torch.isfinite(t).all()) for t in out)
    off = target < 0
    assert int(off.sum()) == 60 and float(dlogits[off].abs().max()) == 0.0 and float(dlogits[~off].abs().sum()) > 0.0
    assert float(row_out[off].abs().max()) == 0.0
    if kind == "focal":
        assert float(out[2].cpu()[off].abs().max()) == 0.0          # row_coef


@pytest.mark.parametrize("kind,gamma", [("focal", 10.0), ("mmi", None)], ids=["focal10", "mmi"])
def test_no_scored_row(kind, gamma):
    """Focal 0 (FocalLoss on an empty selection), MMI nan (the reference's mean over nothing), accuracy nan, gradient 0."""
    logits, _ = H.make_case(41, 512)
    loss, acc, count, grad = _run(kind, logits, torch.full((41,), -1), gamma)
    assert int(count) == 0 and math.isnan(float(acc))
    assert float(loss) == 0.0 if kind == "focal" else math.isnan(float(loss))
    assert grad.shape == (41, 512) and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize("kind,gamma", [("focal", 10.0), ("mmi", None)], ids=["focal10", "mmi"])
def test_two_calls_are_bit_equal(kind, gamma):
    logits, target = H.make_case(2064, 512)
    a = _raw(kind, logits, target, gamma)
    b = _raw(kind, logits, target, gamma)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    first, second = _run(kind, logits, target, gamma), _run(kind, logits, target, gamma)
    assert all(torch.equal(u, v) for u, v in zip(first, second))


def test_empty_input_and_an_unbuilt_gamma():
    from smt_amd import lm as K
    e, t = torch.empty(0, 16, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV)
    assert float(K.focal_loss(e, t, 2.0)[0]) == 0.0 and math.isnan(float(K.mmi_loss(e, t)[0]))
    with pytest.raises(RuntimeError, match="not built"):
        K.focal_loss(torch.zeros(4, 16, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), 0.5)


# ------------------------------------------------------------------------------------------------ model
def _targets(x):
    """Next-token targets as the model forms them, -1 where the reference's loss_mask drops the position."""
    target = torch.full_like(x, -1)
    nxt = x[:, 1:]
    target[:, :-1] = torch.where(nxt >= lmo.OFFSET, nxt - lmo.OFFSET, -1)
    return target.reshape(-1)


def _boom(self, *args, **kwargs):
    raise AssertionError("the torch loss class was called: the train step left the native path")


@pytest.mark.parametrize("kind,gamma", [("focal", None), ("focal", 2.0), ("mmi", None)], ids=["focal", "focal_gamma2", "mmi"])
def test_small_model_train_step_matches_the_oracle_and_stays_native(kind, gamma, tmp_path, monkeypatch):
    """SMALL with 3 layers and dropout 0.1 in train mode: float64 oracle logits with the same masks, then the helper's loss.
    The torch classes raise while the model steps; focal_gamma (default 10) selects the exponent."""
    from models.transformer_lm.losses import FocalLoss, MaximumMutualInformationLoss
    over = dict(SMALL, dropout=0.1, num_layers=3, loss_type=kind)
    if gamma is not None:
        over["focal_gamma"] = gamma
    model, _ = _build(tmp_path, **over)
    p32 = lmo.init_params(16, 64, 2, 128, 3, seed=21)
    model.load_state_dict(p32, strict=False)
    x, lens = lmo.synthetic_tokens(4, 33, 16, seed=22)
    model.train()
    model._drop_seed = 40
    with monkeypatch.context() as mp:
        mp.setattr(FocalLoss, "forward", _boom)
        mp.setattr(MaximumMutualInformationLoss, "forward", _boom)
        loss_dict, metrics = model(x.to(DEV), lens.to(DEV), None, None)
        loss_dict["loss"].backward()
    p64 = {k: v.double().requires_grad_(True) for k, v in p32.items()}
    logits = lmo.lm_logits(x, lens, p64, heads=2, num_layers=3, drop=lmo.CounterDropout(seed=41, p=0.1))   # forward bumps the seed
    used = 10.0 if gamma is None else gamma
    loss, acc, _ = H.module_loss(kind, logits.reshape(-1, 16), _targets(x), used)
    loss.backward()
    print(f"{kind} gamma {gamma}: loss {float(loss_dict['loss']):.9g} ref {float(loss):.9g}; acc {float(metrics['accuracy']):.9g} ref {float(acc):.9g}")
    assert abs(float(loss_dict["loss"]) - float(loss)) <= 2e-5 * max(1.0, abs(float(loss)))
    assert abs(float(metrics["accuracy"]) - float(acc)) < 1e-6
    for name, prm in model.named_parameters():
        if not name.startswith("vqvae."):
            assert rel(prm.grad, p64[name].grad) < 1e-3, (name, rel(prm.grad, p64[name].grad))
    if kind == "focal":                                               # the other exponent gives another loss
        other, _, _ = H.module_loss(kind, logits.detach().reshape(-1, 16), _targets(x), 2.0 if gamma is None else 10.0)
        assert abs(float(other) - float(loss)) > 1e-3 * abs(float(loss))


# ------------------------------------------------------------------------------------------------ capture
@pytest.mark.parametrize("kind", ["focal", "mmi"])
def test_captured_step_replays_the_eager_step(kind, tmp_path):
    """A GraphedStep around the model's forward + backward, replayed ONCE: the loss of an eager step from the same weights and
    dropout counter, bit for bit; gradients to 2e-6 relative (the embedding gradient's atomics add in arrival order)."""
    from smt_amd.graph import GraphedStep
    x, lens = lmo.synthetic_tokens(4, 60, 16, seed=8)
    xd, ld = x.to(DEV), lens.to(DEV)
    p32 = lmo.init_params(16, 64, 2, 128, 2, seed=81)

    def fresh(seed):
        model, _ = _build(tmp_path, **dict(SMALL, dropout=0.1, loss_type=kind))
        model.load_state_dict(p32, strict=False)
        model.train()
        model._drop_seed = seed
        return model

    model = fresh(100)
    step = GraphedStep(model, lambda a, b: model(a, b, None, None), [xd, ld], lambda: model.zero_grad(set_to_none=True), warmup=2)
    assert model._drop_seed == 102
    loss_dict, metrics = step.replay(xd, ld)
    torch.cuda.synchronize()
    loss_g, acc_g = loss_dict["loss"].clone(), metrics["accuracy"].clone()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert model._drop_seed == 103

    ref = fresh(102)
    out, ref_metrics = ref(xd, ld, None, None)
    out["loss"].backward()
    assert math.isfinite(float(loss_g)) and torch.equal(loss_g, out["loss"].detach()) and torch.equal(acc_g, ref_metrics["accuracy"])
    assert set(grads) == {n for n, p in ref.named_parameters() if p.grad is not None} and len(grads) > 10
    for name, prm in ref.named_parameters():
        if prm.grad is not None:
            assert rel(grads[name], prm.grad) <= 2e-6, (name, rel(grads[name], prm.grad))
