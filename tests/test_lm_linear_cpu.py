"""The yardstick of the bf16 projections (tests/lm_linear_helpers.py) checked on the CPU: its float64 evaluation is
torch.nn.functional.linear on the rounded operands, its bound rejects the mistakes a GEMM kernel makes, the bf16 configuration
is transformer_lm.yaml plus one key, and smt_amd.lm.linear in fp32 is the call the model made before."""
import os

import pytest
import torch
import torch.nn.functional as F

import lm_linear_helpers as H

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-masters-thesis_amd")
TEETH_SHAPES = [(33, 64, 48), (129, 128, 64), (300, 64, 64)]


@pytest.mark.parametrize("rows,n_in,n_out", [(33, 64, 48), (129, 128, 16), (300, 512, 192)])
def test_float64_evaluation_is_f_linear_on_the_rounded_operands(rows, n_in, n_out):
    x, w, bias, dy = H.make_case(rows, n_in, n_out)
    xb, wb, dyb = (H.bf16(t).requires_grad_(True) for t in (x, w, dy))
    assert torch.equal(xb.detach().float().to(torch.bfloat16).double(), xb.detach())          # representable in bf16
    b64 = bias.double().requires_grad_(True)
    ref = F.linear(xb, wb, b64)
    y, _ = H.fwd_ref(x, w, bias)
    assert float((y - ref.detach()).abs().max()) <= 1e-12
    assert float((H.fwd_ref(x, w)[0] - F.linear(xb, wb).detach()).abs().max()) <= 1e-12
    ref.backward(dyb.detach())                                        # the rounded dy through F.linear's own backward
    dx, _ = H.dgrad_ref(dy, w)
    dw, _, db, _ = H.wgrad_ref(x, dy)
    assert float((dx - xb.grad).abs().max()) <= 1e-12 and float((dw - wb.grad).abs().max()) <= 1e-12
    assert float((db - dy.double().sum(0)).abs().max()) == 0.0        # the bias gradient sees the unrounded dy


def test_leading_axes_are_rows():
    x, w, bias, _ = H.make_case(6, 32, 16)
    y2, b2 = H.fwd_ref(x, w, bias)
    y3, b3 = H.fwd_ref(x.reshape(2, 3, 32), w, bias)
    assert torch.equal(y3.reshape(6, 16), y2) and torch.equal(b3.reshape(6, 16), b2)


@pytest.mark.parametrize("rows,n_in,n_out", TEETH_SHAPES)
def test_the_bound_has_teeth(rows, n_in, n_out):
    """Each mistake leaves at least 90 % of the elements outside SLACK times the bound, on the data the GPU tests use."""
    x, w, bias, dy = H.make_case(rows, n_in, n_out)
    y, by = H.fwd_ref(x, w, bias)
    dx, bdx = H.dgrad_ref(dy, w)
    dw, bdw, db, bdb = H.wgrad_ref(x, dy)
    xb, wb, dyb = H.bf16(x), H.bf16(w), H.bf16(dy)

    def trunc(t):                                                     # drop the low 16 bits instead of rounding
        return (t.float().view(torch.int32) & -65536).view(torch.float32).double()

    wrong = {
        "fwd without the bias": (xb @ wb.T, y, by),
        "fwd without one 32-wide slice": (xb[:, 32:] @ wb[:, 32:].T + bias.double(), y, by),
        "dgrad without one 32-wide slice": (dyb[:, :-16] @ wb[:-16], dx, bdx) if n_out > 32 else None,
        "wgrad without 32 rows": (dyb[32:].T @ xb[32:], dw, bdw),
        "dbias without 32 rows": (dy.double()[32:].sum(0), db, bdb),
        "fwd with truncated operands": (trunc(x) @ trunc(w).T + bias.double(), y, by),
        "dgrad with truncated operands": (trunc(dy) @ trunc(w), dx, bdx),
        "wgrad with truncated operands": (trunc(dy).T @ trunc(x), dw, bdw),
    }
    if n_in == n_out:
        wrong["fwd with the weight untransposed"] = (xb @ wb + bias.double(), y, by)
        wrong["dgrad with the weight untransposed"] = (dyb @ wb.T, dx, bdx)
    for name, case in wrong.items():
        if case is None:
            continue
        got, ref, bnd = case
        frac = H.fraction_outside(got, ref, bnd)
        print(f"  {name}: {100 * frac:.1f} % outside")
        assert frac >= 0.9, (name, frac)
    # and the float64 value rounded to fp32, the best a kernel can do, is inside everywhere
    for got, ref, bnd in ((y.float(), y, by), (dx.float(), dx, bdx), (dw.float(), dw, bdw), (db.float(), db, bdb)):
        assert H.worst(got, ref, bnd) <= 1.0


def test_bf16_config_is_the_fp32_config_plus_one_key():
    from utils import config as C
    base = C.load(os.path.join(PKG, "configs/models/transformer_lm.yaml")).to_dict()
    bf = C.load(os.path.join(PKG, "configs/models/transformer_lm_bf16.yaml")).to_dict()
    assert "compute_dtype" not in base["model"] and bf["model"].pop("compute_dtype") == "bf16"
    assert bf == base
    with open(os.path.join(PKG, "configs/models/transformer_lm_bf16.yaml")) as f:
        first = f.readline()
    assert first.startswith("#") and "transformer_lm.yaml" in first and "compute_dtype: bf16" in first


def test_fp32_seam_is_f_linear():
    from smt_amd import lm as K
    x, w, bias, dy = H.make_case(3 * 7, 32, 16)
    x = x.reshape(3, 7, 32)
    assert torch.equal(K.linear(x, w, bias), F.linear(x, w, bias))
    assert torch.equal(K.linear(x, w, compute_dtype=torch.float32), F.linear(x, w))
    xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    K.linear(xa, wa, bias).backward(dy.reshape(3, 7, 16))
    F.linear(xr, wr, bias).backward(dy.reshape(3, 7, 16))
    assert torch.equal(xa.grad, xr.grad) and torch.equal(wa.grad, wr.grad)
    with pytest.raises(ValueError, match="compute_dtype"):
        K.linear(x, w, bias, compute_dtype=torch.float16)
