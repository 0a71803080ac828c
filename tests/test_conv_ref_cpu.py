"""tests/conv_ref_helpers.py, the float64 reference of the conv kernels' GPU tests, pinned on the CPU: the forward against
torch.nn.functional.conv1d in float64, every epilogue against the formula written out here, the weight / bias gradients
against float64 autograd; and the bound itself against an fp32 / bf16 emulation of the kernel's arithmetic, which must sit
inside it while the same emulation with one tap, row or channel chunk dropped must not."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref_helpers as R
from oracle import vqvae_oracle as orc

B, T, C = 3, 40, 16
LENS = [40, 17, 0]
GEOMS = [(3, 1), (5, 3)]
SEED, SITE, P = 3, 5, 0.1
DROP_SCALE = float(np.float32(1.0) / np.float32(0.9))
ACT_SCALE = 1.25
EPILOGUES = ("plain", "actout-only", "res", "actgrad", "res+actgrad", "res+actgrad+actout")


def operands(k, dil):
    g = torch.Generator().manual_seed(10 * k + dil)
    bf = torch.bfloat16
    x = torch.randn(B, T, C, generator=g).to(bf)
    w = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(bf)
    bias = torch.randn(C, generator=g)
    res = torch.randn(B, T, C, generator=g).to(bf)
    u_src = torch.relu(torch.randn(B, T, C, generator=g)).to(bf)
    dy = torch.randn(B, T, C, generator=g).to(bf)
    return x, w, bias, res, u_src, dy, torch.tensor(LENS, dtype=torch.int32)


def epilogue_args(epi, res, u_src, lens, keep):
    kw = {"lens_out": lens}
    if "res" in epi:
        kw["res"] = res
    if "actgrad" in epi:
        kw.update(act_grad_src=u_src, scale=ACT_SCALE)
    if "actout" in epi:
        kw.update(keep=keep, drop_scale=DROP_SCALE)
    return kw


def conv64(x, w, bias, dil, pad, lens):
    xm = x.double() * R.row_mask(lens, T) if lens is not None else x.double()
    return F.conv1d(xm.transpose(1, 2), w.double(), None if bias is None else bias.double(), dilation=dil, padding=pad).transpose(1, 2)


@pytest.mark.parametrize("k,dil", GEOMS)
@pytest.mark.parametrize("ragged", [False, True])
def test_forward_reference_matches_conv1d_in_float64(k, dil, ragged):
    x, w, bias, _, _, _, lens = operands(k, dil)
    lens = lens if ragged else None
    pad = (k - 1) * dil // 2
    a, mag = R.conv_ref(x, w, bias, dil, pad, lens)
    want = conv64(x, w, bias, dil, pad, lens)
    assert a.dtype == torch.float64 and a.shape == want.shape == (B, T, C)
    assert float((a - want).abs().max()) <= 1e-13 * float(want.abs().max())
    want_mag = conv64(x.abs(), w.abs(), bias.abs(), dil, pad, lens)
    assert float((mag - want_mag).abs().max()) <= 1e-13 * float(want_mag.abs().max())
    assert bool((mag >= a.abs() - 1e-12).all())
    if ragged:                                             # an empty item sees the bias alone
        assert torch.equal(a[2], bias.double().expand(T, C))
    a0, mag0 = R.conv_ref(x, w, None, dil, pad, lens)
    assert torch.allclose(a0 + bias.double(), a, rtol=0, atol=1e-13) and torch.allclose(mag0 + bias.abs().double(), mag, rtol=0, atol=1e-13)


def test_forward_reference_without_same_padding_has_fewer_rows():
    x, w, bias, _, _, _, lens = operands(3, 1)
    w4 = torch.cat([w, w[:, :, :1]], dim=2)                # k = 4, padding 1: one output row fewer
    a, _ = R.conv_ref(x, w4, bias, 1, 1, lens)
    want = conv64(x, w4, bias, 1, 1, lens)
    assert a.shape == want.shape == (B, T - 1, C) and float((a - want).abs().max()) <= 1e-13 * float(want.abs().max())


@pytest.mark.parametrize("k,dil", GEOMS)
@pytest.mark.parametrize("epi", EPILOGUES)
def test_epilogue_reference_follows_the_kernels_order(k, dil, epi):
    x, w, bias, res, u_src, _, lens = operands(k, dil)
    pad = (k - 1) * dil // 2
    keep = torch.from_numpy(orc.dropout_keep_ntc(SEED, SITE, B, T, C, P))
    a, mag = R.conv_ref(x, w, bias, dil, pad, lens)
    out = R.epilogue_ref(a, mag, C * k, **epilogue_args(epi, res, u_src, lens, keep))
    # the formula, element by element
    o = conv64(x, w, bias, dil, pad, lens)
    if "actgrad" in epi:
        o = torch.where(u_src != 0, o * ACT_SCALE, torch.zeros_like(o))
    for b in range(B):
        o[b, LENS[b]:] = 0
    if "res" in epi:
        o = o + res.double()
    assert float((out["y"] - o).abs().max()) <= 1e-12
    if "actout" in epi:
        u = torch.where(keep, torch.relu(o) * DROP_SCALE, torch.zeros_like(o))
        assert float((out["u"] - u).abs().max()) <= 1e-12
        assert bool((out["u"][~keep] == 0).all()) and bool((out["u_bound"][~keep] == 0).all())
        assert float(out["u"][2].abs().max()) == 0 or "res" in epi      # item 2 is empty: u = relu(res) there, else 0
    else:
        assert "u" not in out
    # rows beyond lens_out: the residual alone, with only its own store's rounding in the bound; exactly 0 without one
    for b in range(B):
        tail, tail_bound = out["y"][b, LENS[b]:], out["y_bound"][b, LENS[b]:]
        if "res" in epi:
            assert torch.equal(tail, res[b, LENS[b]:].double()) and torch.equal(tail_bound, R.BF16_STEP * tail.abs())
        else:
            assert float(tail.abs().sum()) == 0 and float(tail_bound.abs().sum()) == 0
    if "actgrad" in epi and "res" not in epi:
        off = (u_src == 0)
        assert bool((out["y"][off] == 0).all()) and bool((out["y_bound"][off] == 0).all())
    # the bound's terms at one live element
    live = out["y_bound"] > 0
    assert bool(live.any())
    e_c = C * k * R.F32_STEP * mag + R.BF16_STEP * a.abs()
    if epi == "plain":
        assert torch.equal(out["y_bound"][0], (e_c + R.BF16_STEP * o.abs())[0])


@pytest.mark.parametrize("k,dil", GEOMS)
@pytest.mark.parametrize("ragged", [False, True])
def test_gradient_reference_matches_float64_autograd(k, dil, ragged):
    x, w, bias, _, _, dy, lens = operands(k, dil)
    lens = lens if ragged else None
    pad = (k - 1) * dil // 2
    wd = w.double().requires_grad_(True)
    bd = bias.double().requires_grad_(True)
    xm = x.double() * R.row_mask(lens, T) if ragged else x.double()
    y = F.conv1d(xm.transpose(1, 2), wd, bd, dilation=dil, padding=pad).transpose(1, 2)
    (y * dy.double()).sum().backward()
    dw, db = R.wgrad_ref(x, dy, k, dil, pad, lens)
    assert dw.shape == (C, C, k) and db.shape == (C,)
    assert float((dw - wd.grad).abs().max()) <= 1e-12 * float(wd.grad.abs().max())
    assert float((db - bd.grad).abs().max()) <= 1e-12 * float(bd.grad.abs().max())
    tw, tb = R.wgrad_bounds(dw, db, B * T)
    assert tw == 2e-6 * float(dw.abs().max()) * (B * T) ** 0.5 + 1e-4 and tb == 2e-6 * float(db.abs().max()) * (B * T) ** 0.5 + 1e-3


def emulate(x, w, bias, dil, pad, lens, epi, res, u_src, keep, fault=None):
    """The kernel's arithmetic in fp32 with its bf16 roundings; fault = 'tap' / 'row' / 'chunk' drops one of them."""
    xm = (x.float() * R.row_mask(lens, T)).clone()
    wf = w.float().clone()
    if fault == "tap":
        wf[:, :, 0] = 0
    if fault == "chunk":
        wf[:, C // 2:, :] = 0
    if fault == "row":
        xm[0, 7] = 0
    acc = F.conv1d(xm.transpose(1, 2), wf, bias, dilation=dil, padding=pad).transpose(1, 2)
    o = acc.to(torch.bfloat16).float()
    if "actgrad" in epi:
        o = torch.where(u_src != 0, o * np.float32(ACT_SCALE), torch.zeros_like(o))
    o = o * R.row_mask(lens, T).float()
    if "res" in epi:
        o = o + res.float()
    y = o.to(torch.bfloat16)
    u = torch.where(keep & (o > 0), o * np.float32(DROP_SCALE), torch.zeros_like(o)).to(torch.bfloat16)
    return y, u


@pytest.mark.parametrize("k,dil", GEOMS)
@pytest.mark.parametrize("epi", EPILOGUES)
def test_bound_holds_an_emulated_kernel_and_rejects_a_dropped_tap_row_or_chunk(k, dil, epi):
    x, w, bias, res, u_src, _, lens = operands(k, dil)
    pad = (k - 1) * dil // 2
    keep = torch.from_numpy(orc.dropout_keep_ntc(SEED, SITE, B, T, C, P))
    a, mag = R.conv_ref(x, w, bias, dil, pad, lens)
    out = R.epilogue_ref(a, mag, C * k, **epilogue_args(epi, res, u_src, lens, keep))
    y, u = emulate(x, w, bias, dil, pad, lens, epi, res, u_src, keep)
    assert R.worst(y, out["y"], out["y_bound"]) <= R.SLACK
    if "actout" in epi:
        assert R.worst(u, out["u"], out["u_bound"]) <= R.SLACK
    for fault in ("tap", "row", "chunk"):
        yf, uf = emulate(x, w, bias, dil, pad, lens, epi, res, u_src, keep, fault)
        assert R.worst(yf, out["y"], out["y_bound"]) > 10 * R.SLACK, fault
        if "actout" in epi:
            assert R.worst(uf, out["u"], out["u_bound"]) > 10 * R.SLACK, fault
    with pytest.raises(AssertionError):
        R.check("faulty", yf, out["y"], out["y_bound"])
    # a value where the bound is 0 is an error however small; NaN never passes
    bad = out["y"].clone()
    if bool((out["y_bound"] == 0).any()):
        i = (out["y_bound"] == 0).nonzero()[0]
        bad[tuple(i)] += 1e-30
        assert R.worst(bad, out["y"], out["y_bound"]) == float("inf")
    nan = out["y"].clone()
    nan[0, 0, 0] = float("nan")
    assert not R.worst(nan, out["y"], out["y_bound"]) <= R.SLACK
