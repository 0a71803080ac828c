"""The attention kernels at head dim 64 (csrc/lm.hip, smt_lm_attention_hd_fwd / _bwd with head_dim = 64), the C entries
themselves, against float64.

fp32 operands: oracle.lm_oracle.attention_core and its autograd in float64, with the tolerances tests/test_lm_gpu.py uses for
the head-dim-32 kernels on the same input distribution (ctx atol 2e-5, dqkv atol 5e-5): the f32 MFMA's products are exact and
the only term that grows with the head dim is the 64-term score sum.  bf16 operands: tests/lm_attn_hd_helpers.attention_exact
and the a-priori elementwise bound of tests/lm_attn_bf16_helpers.py with c = 1 / sqrt(64), on bf16-representable inputs.  The
backward call is handed the device forward's own ctx and lse, as the autograd function hands them over.

Worst errors over every case, measured on an MI355X: see DESIGN.md section 24.
"""
import itertools

import pytest
import torch

import lm_attn_hd_helpers as A
from oracle import lm_oracle as lmo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SITE = 3
DH = 64
LENGTHS = [1, 31, 32, 33, 127, 129, 131]
SHAPES = [(1, 1), (2, 2)]


def run(qkv, lens, heads, causal, p=0.0, seed=5, dctx=None, use_key_dev=False, dtype="fp32", head_dim=DH, entries="hd"):
    """The C entries themselves: (ctx, lse, dqkv or None) on the CPU.  `use_key_dev` passes a wrong key by value and the right one
    through device memory; entries = "old" calls the four head-dim-32 entries instead."""
    from smt_amd import lm as K
    from smt_amd import native as N
    lib = N.lib()
    b, l, d3 = qkv.shape
    d = d3 // 3
    drop = K.Drop(p, True, seed, SITE)
    key, key_dev = drop.key, None
    if use_key_dev:
        key_dev = torch.tensor([drop.key - (drop.key >> 31 << 32)], dtype=torch.int32, device=DEV)      # the uint32 key's bits
        key = (drop.key + 12345) & 0xFFFFFFFF
    if entries == "hd":
        fwd, bwd, tail = lib.smt_lm_attention_hd_fwd, lib.smt_lm_attention_hd_bwd, (head_dim, int(dtype == "bf16"))
    else:
        assert head_dim == 32
        fwd, bwd = ((lib.smt_lm_attention_bf16_fwd, lib.smt_lm_attention_bf16_bwd) if dtype == "bf16" else
                    (lib.smt_lm_attention_fwd, lib.smt_lm_attention_bwd))
        tail = ()
    qd = qkv.to(DEV, torch.float32).contiguous()
    ld = None if lens is None else lens.to(DEV, torch.int32)
    ctx = torch.full((b, l, d), float("nan"), device=DEV)
    lse = torch.full((b, heads, l), float("nan"), device=DEV)
    N.check(fwd(N.ptr(qd), N.ptr(ld), N.ptr(ctx), N.ptr(lse), b, l, heads, int(causal), key, N.ptr(key_dev), drop.thresh, drop.scale,
                *tail, N.stream_ptr()), "attention forward")
    dqkv = None
    if dctx is not None:
        gd = dctx.to(DEV, torch.float32).contiguous()
        dqkv = torch.full_like(qd, float("nan"))
        delta = torch.empty_like(lse)
        N.check(bwd(N.ptr(qd), N.ptr(ld), N.ptr(ctx), N.ptr(lse), N.ptr(gd), N.ptr(dqkv), N.ptr(delta), b, l, heads, int(causal), key,
                    N.ptr(key_dev), drop.thresh, drop.scale, *tail, N.stream_ptr()), "attention backward")
        dqkv = dqkv.cpu()
    torch.cuda.synchronize()
    return ctx.cpu(), lse.cpu(), dqkv


def inputs(b, l, heads, seed, representable=True, dh=DH):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b, l, 3 * heads * dh, generator=g)
    dctx = torch.randn(b, l, heads * dh, generator=g)
    return (A.bf16(qkv), A.bf16(dctx)) if representable else (qkv, dctx)


def lens_options(b, l):
    """None, [2L/3, 0], [L, L/2]: between them 0, L and lengths in between."""
    return [None, torch.tensor([(2 * l) // 3, 0][:b]), torch.tensor([l, l // 2][:b])]


@pytest.mark.parametrize("l", LENGTHS)
def test_fp32_kernels_against_the_float64_oracle(l):
    """The 32-row block edge, the 128-row four-wave edge, even and odd L (the two dropout hash paths); causal or not, lens
    None / [2L/3, 0] / [L, L/2], dropout 0 and 0.1.  A batch item with lens = 0 has no visible key: the oracle's softmax is
    NaN there (and only there), the kernels write zeros."""
    worst = {"ctx": 0.0, "dqkv": 0.0}
    for (b, h), causal, p in itertools.product(SHAPES, [True, False], [0.0, 0.1]):
        qkv, dctx = inputs(b, l, h, seed=1000 * l + 10 * b + h, representable=False)
        for lens in lens_options(b, l):
            what = (b, h, l, causal, p, None if lens is None else lens.tolist())
            leaf = qkv.double().requires_grad_(True)
            ref = lmo.attention_core(leaf, lens, h, causal, lmo.CounterDropout(seed=5, p=p), SITE)
            ref.backward(dctx.double())
            live = torch.ones(b, dtype=torch.bool) if lens is None else lens > 0
            ctx, _, dqkv = run(qkv, lens, h, causal, p, 5, dctx)
            assert not torch.isnan(ctx).any() and not torch.isnan(dqkv).any(), (what, "unwritten or NaN elements")
            assert not ctx[~live].any() and not dqkv[~live].any(), what
            if not live.any():
                continue
            ref, gref = ref.detach()[live], leaf.grad[live]
            assert not torch.isnan(ref).any() and not torch.isnan(gref).any()
            e_ctx, e_g = float((ctx[live].double() - ref).abs().max()), float((dqkv[live].double() - gref).abs().max())
            worst["ctx"], worst["dqkv"] = max(worst["ctx"], e_ctx), max(worst["dqkv"], e_g)
            assert torch.allclose(ctx[live], ref.float(), atol=2e-5), (what, e_ctx)
            assert torch.allclose(dqkv[live], gref.float(), atol=5e-5), (what, e_g)
    print(f"  L {l}: worst |fp32 kernel - float64|: ctx {worst['ctx']:.3e}, dqkv {worst['dqkv']:.3e}")


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


@pytest.mark.parametrize("l", LENGTHS)
def test_bf16_kernels_against_exact_float64_within_the_a_priori_bound(l):
    """The shapes of the fp32 test plus dropout 0.5, bf16-representable inputs."""
    worst = {}
    for (b, h), causal, p in itertools.product(SHAPES, [True, False], [0.0, 0.1, 0.5]):
        qkv, dctx = inputs(b, l, h, seed=1000 * l + 10 * b + h)
        ks = A.keep_scale(lmo.CounterDropout(seed=5, p=p), SITE, b, h, l)
        for lens in lens_options(b, l):
            exact = A.attention_exact(qkv, lens, h, causal, ks, dctx)
            ctx, lse, dqkv = run(qkv, lens, h, causal, p, 5, dctx, dtype="bf16")
            check_against(exact, ctx, lse, dqkv, worst, (b, h, l, causal, p, None if lens is None else lens.tolist()))
    print(f"  L {l}: worst |bf16 kernel - float64| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_bf16_kernels_round_plain_fp32_inputs_to_nearest_even_on_load():
    """Inputs that are not bf16-representable, against exact float64 on operands rounded on the host; delta is formed from the
    unrounded dctx there too, as the kernel forms it."""
    worst, l = {}, 129
    for causal, p in itertools.product([True, False], [0.0, 0.1]):
        qkv, dctx = inputs(2, l, 2, seed=77 + l, representable=False)
        assert not torch.equal(A.bf16(qkv), qkv)
        lens = torch.tensor([l, l - 5])
        ks = A.keep_scale(lmo.CounterDropout(seed=5, p=p), SITE, 2, 2, l)
        exact = A.attention_exact(A.bf16(qkv), lens, 2, causal, ks, A.bf16(dctx), dctx_delta=dctx)
        ctx, lse, dqkv = run(qkv, lens, 2, causal, p, 5, dctx, dtype="bf16")
        check_against(exact, ctx, lse, dqkv, worst, (l, causal, p))
    print(f"  L {l}, plain inputs: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("l", [32, 33, 96])
def test_the_dropout_masks_are_the_head_dim_32_kernels(l, dtype):
    """B = H = 1, not causal, p = 0.5, V one-hot inside one 32-key window (row j0 + c has its 1 in channel c0 + c) and zero
    elsewhere: ctx[i, c0 + c] = P[i, j0 + c] * keep * 2, so the zero pattern of ctx is the oracle's keep mask of that window --
    the mask of element ((b H + h) L + i) L + j, which does not know the head dim.  Every window, once with the one-hot in the
    lower 32 channels (c0 = 0) and once in the upper (c0 = 32): a swapped or dropped upper chunk shows."""
    qkv, _ = inputs(1, l, 1, seed=l)
    keep = A.keep_scale(lmo.CounterDropout(seed=5, p=0.5), SITE, 1, 1, l)[0, 0] > 0          # [L, L]
    assert 0.4 < float(keep.float().mean()) < 0.6
    for c0, j0 in itertools.product((0, 32), range(0, l, 32)):
        n = min(32, l - j0)
        v = torch.zeros(l, DH)
        v[j0 + torch.arange(n), c0 + torch.arange(n)] = 1.0
        x = qkv.clone()
        x[0, :, 2 * DH:] = v
        ctx, _, _ = run(x, None, 1, False, 0.5, 5, dtype=dtype)
        assert torch.equal(ctx[0, :, c0:c0 + n] != 0, keep[:, j0:j0 + n]), (l, c0, j0)
        rest = torch.ones(DH, dtype=torch.bool)
        rest[c0:c0 + n] = False
        assert not ctx[0][:, rest].any(), (l, c0, j0)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bit_for_bit_properties(dtype):
    b, h, l, t, p = 2, 2, 131, 70, 0.1
    qkv, dctx = inputs(b, l, h, seed=9)
    lens = torch.tensor([l, 90])
    first = run(qkv, lens, h, True, p, 5, dctx, dtype=dtype)
    # two runs are equal, and the device-resident key is the by-value key
    for other in (run(qkv, lens, h, True, p, 5, dctx, dtype=dtype), run(qkv, lens, h, True, p, 5, dctx, use_key_dev=True, dtype=dtype)):
        assert all(torch.equal(a, c) for a, c in zip(first, other))
    # causal: tokens after t change nothing at or before t (with no gradient coming from after t either)
    g0 = dctx.clone()
    g0[:, t + 1:] = 0
    base = run(qkv, None, h, True, p, 5, g0, dtype=dtype)
    x2 = qkv.clone()
    x2[:, t + 1:] = A.bf16(torch.randn(b, l - t - 1, x2.shape[-1], generator=torch.Generator().manual_seed(1)))
    moved = run(x2, None, h, True, p, 5, g0, dtype=dtype)
    assert torch.equal(base[0][:, :t + 1], moved[0][:, :t + 1]) and torch.equal(base[1][..., :t + 1], moved[1][..., :t + 1])
    assert torch.equal(base[2][:, :t + 1], moved[2][:, :t + 1])
    assert not torch.equal(base[0][:, t + 1:], moved[0][:, t + 1:])
    # keys at or beyond lens[b] change nothing (their own dk, dv are zero)
    x3 = qkv.clone()
    x3[1, 90:, h * DH:] = 7.0
    padded = run(x3, lens, h, False, p, 5, dctx, dtype=dtype)
    plain = run(qkv, lens, h, False, p, 5, dctx, dtype=dtype)
    assert torch.equal(padded[0], plain[0]) and torch.equal(padded[1], plain[1]) and torch.equal(padded[2], plain[2])
    assert not plain[2][1, 90:, h * DH:].any()
    # a row with lens = 0: zero context, zero gradients
    ctx, lse, dqkv = run(qkv, torch.tensor([l, 0]), h, True, p, 5, dctx, dtype=dtype)
    assert not ctx[1].any() and not dqkv[1].any() and not lse[1].any()
    assert ctx[0].any() and dqkv[0].any()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_head_dim_32_through_the_new_entries_is_the_old_entries_bit_for_bit(dtype):
    for l, causal, p in ((131, True, 0.1), (64, False, 0.0)):
        qkv, dctx = inputs(2, l, 2, seed=31 + l, representable=False, dh=32)
        lens = torch.tensor([l, l - 9])
        new = run(qkv, lens, 2, causal, p, 5, dctx, dtype=dtype, head_dim=32)
        old = run(qkv, lens, 2, causal, p, 5, dctx, dtype=dtype, head_dim=32, entries="old")
        assert all(torch.equal(a, c) for a, c in zip(new, old)) and not torch.isnan(new[2]).any()


@pytest.mark.parametrize("head_dim", [48, 128, 0, 16])
def test_other_head_dims_are_an_argument_error_with_no_launch(head_dim):
    from smt_amd import native as N
    lib = N.lib()
    dh = max(head_dim, 32)
    qkv = torch.randn(1, 8, 3 * dh, device=DEV)
    ctx, lse = torch.full((1, 8, dh), float("nan"), device=DEV), torch.full((1, 1, 8), float("nan"), device=DEV)
    dqkv, delta = torch.full_like(qkv, float("nan")), torch.full_like(lse, float("nan"))
    for bf in (0, 1):
        rc = lib.smt_lm_attention_hd_fwd(N.ptr(qkv), None, N.ptr(ctx), N.ptr(lse), 1, 8, 1, 1, 0, None, 0, 1.0, head_dim, bf, N.stream_ptr())
        assert rc != 0 and f"got {head_dim}" in lib.smt_last_error().decode()
        with pytest.raises(RuntimeError, match=f"head dim must be 32 or 64 .got {head_dim}."):
            N.check(lib.smt_lm_attention_hd_bwd(N.ptr(qkv), None, N.ptr(ctx), N.ptr(lse), N.ptr(qkv), N.ptr(dqkv), N.ptr(delta), 1, 8, 1, 1, 0,
                                                None, 0, 1.0, head_dim, bf, N.stream_ptr()), "smt_lm_attention_hd_bwd")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (ctx, lse, dqkv, delta))


def test_binding_derives_the_head_dim_and_is_the_direct_calls_bit_for_bit():
    """smt_amd.lm.attention on qkv [.., 3 * 2 * 64] with 2 heads, through autograd, in both operand types; the profiler
    regions keep their names and count 64-channel products."""
    from smt_amd import lm as K
    qkv, dctx = inputs(2, 70, 2, seed=12, representable=False)
    lens = torch.tensor([70, 41])
    seen = []
    real = K.profiler.region

    def spy(name, **kw):
        seen.append((name, kw.get("dtype"), kw.get("flops")))
        return real(name, **kw)

    K.profiler.region = spy
    try:
        outs = {}
        for name, kw in (("bf16", dict(compute_dtype=torch.bfloat16)), ("fp32", {})):
            leaf = qkv.to(DEV).requires_grad_(True)
            out = K.attention(leaf, lens.to(DEV, torch.int32), 2, True, K.Drop(0.1, True, 5, SITE), **kw)
            out.backward(dctx.to(DEV))
            outs[name] = (out.detach().cpu(), leaf.grad.cpu())
    finally:
        K.profiler.region = real
    pairs = 70 * 71 // 2
    assert seen == [("lm_attention_bf16:fwd", "bf16", 2 * 2 * pairs * 128 * 2), ("lm_attention_bf16:bwd", "bf16", 2 * 2 * pairs * 128 * 5),
                    ("lm_attention:fwd", "f32", 2 * 2 * pairs * 128 * 2), ("lm_attention:bwd", "f32", 2 * 2 * pairs * 128 * 5)]
    for name in ("bf16", "fp32"):
        direct = run(qkv, lens, 2, True, 0.1, 5, dctx, dtype=name)
        assert torch.equal(outs[name][0], direct[0]) and torch.equal(outs[name][1], direct[2])
    assert not torch.equal(outs["bf16"][0], outs["fp32"][0])
