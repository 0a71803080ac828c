"""The attention kernels on bf16 MFMAs (csrc/lm.hip, smt_lm_attention_bf16_fwd / _bwd) against float64.

The yardstick is never the fp32 device kernel: it is tests/lm_attn_bf16_helpers.attention_exact, float64 and unrounded, and the
tolerance is the a-priori bound derived in that module's docstring, elementwise (tests/test_lm_attn_bf16_cpu.py shows what the
bound lets through and what it does not).  Inputs are random and bf16-representable unless a test says otherwise; the backward
call is handed the device forward's own ctx and lse, as the autograd function hands them over.

Worst |error| / bound over every case of the float64 test, measured on an MI355X: see DESIGN.md section 23.
"""
import itertools

import pytest
import torch

import lm_attn_bf16_helpers as A
from oracle import lm_oracle as lmo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SITE = 3
LENGTHS = [1, 31, 32, 33, 127, 129, 131, 258]


def run(qkv, lens, heads, causal, p=0.0, seed=5, dctx=None, use_key_dev=False, dtype="bf16"):
    """The C entries themselves: (ctx, lse, dqkv or None) on the CPU.  `use_key_dev` passes a wrong key by value and the right one
    through device memory."""
    from smt_amd import lm as K
    from smt_amd import native as N
    fwd, bwd = ("smt_lm_attention_bf16_fwd", "smt_lm_attention_bf16_bwd") if dtype == "bf16" else ("smt_lm_attention_fwd", "smt_lm_attention_bwd")
    b, l, d3 = qkv.shape
    d = d3 // 3
    drop = K.Drop(p, True, seed, SITE)
    key, key_dev = drop.key, None
    if use_key_dev:
        key_dev = torch.tensor([drop.key - (drop.key >> 31 << 32)], dtype=torch.int32, device=DEV)      # the uint32 key's bits
        key = (drop.key + 12345) & 0xFFFFFFFF
    qd = qkv.to(DEV, torch.float32).contiguous()
    ld = None if lens is None else lens.to(DEV, torch.int32)
    ctx = torch.full((b, l, d), float("nan"), device=DEV)
    lse = torch.full((b, heads, l), float("nan"), device=DEV)
    N.check(getattr(N.lib(), fwd)(N.ptr(qd), N.ptr(ld), N.ptr(ctx), N.ptr(lse), b, l, heads, int(causal), key, N.ptr(key_dev), drop.thresh,
                                  drop.scale, N.stream_ptr()), fwd)
    dqkv = None
    if dctx is not None:
        gd = dctx.to(DEV, torch.float32).contiguous()
        dqkv = torch.full_like(qd, float("nan"))
        delta = torch.empty_like(lse)
        N.check(getattr(N.lib(), bwd)(N.ptr(qd), N.ptr(ld), N.ptr(ctx), N.ptr(lse), N.ptr(gd), N.ptr(dqkv), N.ptr(delta), b, l, heads,
                                      int(causal), key, N.ptr(key_dev), drop.thresh, drop.scale, N.stream_ptr()), bwd)
        dqkv = dqkv.cpu()
    torch.cuda.synchronize()
    return ctx.cpu(), lse.cpu(), dqkv


def inputs(b, l, heads, seed, representable=True):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b, l, 3 * heads * A.DH, generator=g)
    dctx = torch.randn(b, l, heads * A.DH, generator=g)
    return (A.bf16(qkv), A.bf16(dctx)) if representable else (qkv, dctx)


def check_against(exact, ctx, lse, dqkv, worst, what):
    """Elementwise |device - exact| <= bound for ctx, dq, dk, dv, lse within 1e-5; `worst` collects max |err| / bound per output."""
    b_ctx, b_dqkv = A.bounds(exact)
    d = ctx.shape[-1]
    assert float((lse.double() - exact["lse"]).abs().max()) <= 1e-5, (what, "lse")
    errs = {"ctx": ((ctx.double() - exact["ctx"]).abs(), b_ctx)}
    e = (dqkv.double() - exact["dqkv"]).abs()
    for i, name in enumerate(("dq", "dk", "dv")):
        errs[name] = (e[..., i * d:(i + 1) * d], b_dqkv[..., i * d:(i + 1) * d])
    for name, (err, bound) in errs.items():
        assert not torch.isnan(err).any(), (what, name, "the kernel left elements unwritten or wrote NaN")
        ratio = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert bool((err <= bound).all()), (what, name, f"worst |err| / bound {ratio:.3f}", float(err.max()))


def lens_options(b, l):
    """None, and two ragged sets that between them hold 0, L and lengths in between."""
    return [None, torch.tensor([max(1, (2 * l) // 3), 0][:b]), torch.tensor([l, l // 2][:b])]


@pytest.mark.parametrize("l", LENGTHS)
def test_against_exact_float64_within_the_a_priori_bound(l):
    """Block and four-wave boundaries (32, 128), the even-L paired-hash and the odd-L dropout paths; B, H in {1, 2}, causal
    or not, lens None or ragged with 0 and L, dropout 0 / 0.1 / 0.5."""
    worst = {}
    for (b, h), causal, p in itertools.product([(1, 1), (1, 2), (2, 1), (2, 2)], [True, False], [0.0, 0.1, 0.5]):
        qkv, dctx = inputs(b, l, h, seed=1000 * l + 10 * b + h)
        ks = A.keep_scale(lmo.CounterDropout(seed=5, p=p), SITE, b, h, l)
        for lens in lens_options(b, l):
            exact = A.attention_exact(qkv, lens, h, causal, ks, dctx)
            ctx, lse, dqkv = run(qkv, lens, h, causal, p, 5, dctx)
            check_against(exact, ctx, lse, dqkv, worst, (b, h, l, causal, p, None if lens is None else lens.tolist()))
    print(f"  L {l}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("l", [33, 129])
def test_plain_fp32_inputs_are_rounded_to_nearest_even_on_load(l):
    """Inputs that are not bf16-representable, against exact float64 on operands rounded on the host (torch's conversion is
    round to nearest even); delta is formed from the unrounded dctx there too, as the kernel forms it."""
    worst = {}
    for causal, p in itertools.product([True, False], [0.0, 0.1]):
        qkv, dctx = inputs(2, l, 2, seed=77 + l, representable=False)
        assert not torch.equal(A.bf16(qkv), qkv)
        lens = torch.tensor([l, l - 5])
        ks = A.keep_scale(lmo.CounterDropout(seed=5, p=p), SITE, 2, 2, l)
        exact = A.attention_exact(A.bf16(qkv), lens, 2, causal, ks, A.bf16(dctx), dctx_delta=dctx)
        ctx, lse, dqkv = run(qkv, lens, 2, causal, p, 5, dctx)
        check_against(exact, ctx, lse, dqkv, worst, (l, causal, p))
    print(f"  L {l}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("l", [32, 33, 96])
def test_the_dropout_masks_are_the_fp32_kernels(l):
    """B = H = 1, not causal, p = 0.5, V one-hot inside one 32-key window (row j0 + c has its 1 in channel c) and zero elsewhere:
    ctx[i, c] = P[i, j0 + c] * keep * 2, so the zero pattern of ctx is the oracle's keep mask of that window.  Every window."""
    qkv, _ = inputs(1, l, 1, seed=l)
    keep = A.keep_scale(lmo.CounterDropout(seed=5, p=0.5), SITE, 1, 1, l)[0, 0] > 0          # [L, L]
    assert 0.4 < float(keep.float().mean()) < 0.6
    for j0 in range(0, l, 32):
        n = min(32, l - j0)
        v = torch.zeros(l, 32)
        v[j0 + torch.arange(n), torch.arange(n)] = 1.0
        x = qkv.clone()
        x[0, :, 64:] = v
        ctx, _, _ = run(x, None, 1, False, 0.5, 5)
        assert torch.equal(ctx[0, :, :n] != 0, keep[:, j0:j0 + n]), (l, j0)
        assert not ctx[0, :, n:].any()


def test_bit_for_bit_properties():
    b, h, l, t, p = 2, 2, 131, 70, 0.1
    qkv, dctx = inputs(b, l, h, seed=9)
    lens = torch.tensor([l, 90])
    first = run(qkv, lens, h, True, p, 5, dctx)
    # two runs are equal, and the device-resident key is the by-value key
    for other in (run(qkv, lens, h, True, p, 5, dctx), run(qkv, lens, h, True, p, 5, dctx, use_key_dev=True)):
        assert all(torch.equal(a, c) for a, c in zip(first, other))
    # causal: tokens after t change nothing at or before t (with no gradient coming from after t either)
    g0 = dctx.clone()
    g0[:, t + 1:] = 0
    base = run(qkv, None, h, True, p, 5, g0)
    x2 = qkv.clone()
    x2[:, t + 1:] = A.bf16(torch.randn(b, l - t - 1, x2.shape[-1], generator=torch.Generator().manual_seed(1)))
    moved = run(x2, None, h, True, p, 5, g0)
    assert torch.equal(base[0][:, :t + 1], moved[0][:, :t + 1]) and torch.equal(base[1][..., :t + 1], moved[1][..., :t + 1])
    assert torch.equal(base[2][:, :t + 1], moved[2][:, :t + 1])
    assert not torch.equal(base[0][:, t + 1:], moved[0][:, t + 1:])
    # keys at or beyond lens[b] change nothing (their own dk, dv are zero)
    x3 = qkv.clone()
    x3[1, 90:, h * 32:] = 7.0
    padded = run(x3, lens, h, False, p, 5, dctx)
    plain = run(qkv, lens, h, False, p, 5, dctx)
    assert torch.equal(padded[0], plain[0]) and torch.equal(padded[1], plain[1]) and torch.equal(padded[2], plain[2])
    assert not plain[2][1, 90:, h * 32:].any()
    # a row with lens = 0: zero context, zero gradients
    ctx, lse, dqkv = run(qkv, torch.tensor([l, 0]), h, True, p, 5, dctx)
    assert not ctx[1].any() and not dqkv[1].any() and not lse[1].any()
    assert ctx[0].any() and dqkv[0].any()


def test_the_option_changes_the_arithmetic():
    """On inputs that are not bf16-representable the bf16 context differs from the fp32 kernel's (and stays near it)."""
    qkv, dctx = inputs(2, 129, 2, seed=4, representable=False)
    bf = run(qkv, None, 2, True, 0.0, 5, dctx)
    fp = run(qkv, None, 2, True, 0.0, 5, dctx, dtype="fp32")
    diff = float((bf[0] - fp[0]).abs().max())
    print(f"  max |ctx bf16 - ctx fp32| = {diff:.3e}, max |dqkv bf16 - dqkv fp32| = {float((bf[2] - fp[2]).abs().max()):.3e}")
    assert 1e-5 < diff < 0.1


def test_binding_selects_the_entries_and_names_the_regions():
    """smt_amd.lm.attention(compute_dtype=torch.bfloat16) is the bf16 entries (bit for bit), through autograd; the default is
    today's call; the profiler sees lm_attention_bf16:fwd / :bwd with dtype bf16."""
    from smt_amd import lm as K
    from smt_amd import profiler
    qkv, dctx = inputs(2, 70, 2, seed=12, representable=False)
    lens = torch.tensor([70, 41])
    seen = []
    real = profiler.region

    def spy(name, **kw):
        seen.append((name, kw.get("dtype")))
        return real(name, **kw)

    K.profiler.region, old = spy, K.profiler.region
    try:
        outs = {}
        for name, kw in (("bf16", dict(compute_dtype=torch.bfloat16)), ("fp32", dict(compute_dtype=torch.float32)), ("default", {})):
            leaf = qkv.to(DEV).requires_grad_(True)
            out = K.attention(leaf, lens.to(DEV, torch.int32), 2, True, K.Drop(0.1, True, 5, SITE), **kw)
            out.backward(dctx.to(DEV))
            outs[name] = (out.detach().cpu(), leaf.grad.cpu())
    finally:
        K.profiler.region = old
    assert seen == [("lm_attention_bf16:fwd", "bf16"), ("lm_attention_bf16:bwd", "bf16")] + [("lm_attention:fwd", "f32"), ("lm_attention:bwd", "f32")] * 2
    direct = run(qkv, lens, 2, True, 0.1, 5, dctx)
    assert torch.equal(outs["bf16"][0], direct[0]) and torch.equal(outs["bf16"][1], direct[2])
    direct32 = run(qkv, lens, 2, True, 0.1, 5, dctx, dtype="fp32")
    for name in ("fp32", "default"):
        assert torch.equal(outs[name][0], direct32[0]) and torch.equal(outs[name][1], direct32[2])
    with pytest.raises(ValueError, match="compute_dtype"):
        K.attention(qkv.to(DEV), None, 2, True, compute_dtype=torch.float16)
