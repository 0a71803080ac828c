"""The two rotary entries on the device (csrc/lm_rope.hip smt_lm_rope, csrc/lm_decode.hip smt_lm_decode_attention_rope, through
smt_amd.lm) against the float64 helper of tests/lm_rope_helpers.py.  The rotation is held to 4 u (|x[2i]| + |x[2i+1]|), u = 2^-24
(derived in that module; tests/test_lm_rope_cpu.py shows the assertion failing under five mutations on these inputs)."""
import math

import pytest
import torch
import torch.nn.functional as F

import lm_rope_helpers as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, HEADS = R.KERNEL_B, R.KERNEL_H


def _launch(x, table, dh, pos0, inverse, heads=HEADS, rows=None):
    """smt_lm_rope on a device tensor, in place, through the C entry (the binding's `rope` has no inverse switch)."""
    from smt_amd import native as N
    b, l, _ = x.shape
    N.check(N.lib().smt_lm_rope(N.ptr(x), N.ptr(table), b, l, heads, dh, table.shape[0] if rows is None else rows, pos0, int(inverse),
                                N.stream_ptr()), "smt_lm_rope")
    return x


@pytest.mark.parametrize("L,dh,pos0", R.KERNEL_CASES)
def test_rope_kernel_is_within_the_bound_and_leaves_v_and_the_next_row_alone(L, dh, pos0):
    from smt_amd import lm as K
    x, positions = R.kernel_case(L, dh, pos0)
    table = K.rope_table(pos0 + L, dh, device=DEV)                 # rope_rows = pos0 + L exactly
    d3 = x.shape[-1]
    for inverse in (False, True):
        buf = torch.full((B * L + 1, d3), -123.25, device=DEV)      # one sentinel row past the tensor
        buf[:B * L] = x.reshape(B * L, d3).to(DEV)
        dev = buf[:B * L].view(B, L, d3)
        _launch(dev, table, dh, pos0, inverse)
        got = dev.cpu()
        ratio = R.assert_rope(got, x, HEADS, positions, inverse=inverse)
        print(f"  L {L}, dh {dh}, pos0 {pos0}, inverse {inverse}: worst |err| / (4u(|x0| + |x1|)) = {ratio:.3f}")
        assert bool((buf[B * L] == -123.25).all())
        again = _launch(x.to(DEV), table, dh, pos0, inverse)
        assert torch.equal(again.cpu(), got)                        # equal inputs, equal bits


@pytest.mark.parametrize("dh", [32, 64])
def test_rope_binding_rotates_in_place_and_its_backward_is_the_inverse(dh):
    """`rope`: returns its (dirty) input; the gradient is the inverse rotation of the incoming one, v passed through; through
    F.linear and through the bf16 projection, whose backward does not need the projection's output."""
    from smt_amd import lm as K
    L, pos0 = 33, 37
    x, positions = R.kernel_case(L, dh, pos0)
    table = K.rope_table(pos0 + L, dh, device=DEV)
    leaf = x.to(DEV).requires_grad_(True)
    inp = leaf * 1.0
    out = K.rope(inp, table, HEADS, pos0)
    assert out.data_ptr() == inp.data_ptr()
    R.assert_rope(out.detach().cpu(), x, HEADS, positions)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
    gd = g.to(DEV)
    out.backward(gd)
    assert torch.equal(gd.cpu(), g)                                 # the incoming gradient is not modified
    R.assert_rope(leaf.grad.cpu(), g, HEADS, positions, inverse=True)
    # the in-projection in front of it: gradients of the weight, the bias and the input against float64
    d = HEADS * dh
    gen = torch.Generator().manual_seed(6)
    t, w, bias = torch.randn(B, L, d, generator=gen), torch.randn(3 * d, d, generator=gen) * d ** -0.5, torch.randn(3 * d, generator=gen)
    t64, w64, b64 = (v.double().requires_grad_(True) for v in (t, w, bias))
    (R.rope64(F.linear(t64, w64, b64), HEADS, positions) * g.double()).sum().backward()
    td, wd, bd = (v.to(DEV).requires_grad_(True) for v in (t, w, bias))
    (K.rope(K.linear(td, wd, bd), table, HEADS, pos0) * gd).sum().backward()
    for name, mine, ref in (("x", td, t64), ("weight", wd, w64), ("bias", bd, b64)):
        assert torch.allclose(mine.grad.cpu(), ref.grad.float(), atol=1e-4, rtol=1e-4), name      # add_layer_norm's gradient tolerance
    td2, wd2, bd2 = (v.to(DEV).requires_grad_(True) for v in (t, w, bias))
    (K.rope(K.linear(td2, wd2, bd2, compute_dtype=torch.bfloat16), table, HEADS, pos0) * gd).sum().backward()
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in (td2, wd2, bd2))
    # bf16 operands: the input gradient = dy W with both rounded to bf16 (2^-8 each), over d terms -> a loose 3e-2 of the scale
    assert float((td2.grad - td.grad).abs().max()) <= 3e-2 * float(td.grad.abs().max())


@pytest.mark.parametrize("dh", [32, 64])
def test_rope_is_relative_on_the_device(dh):
    """attention(rope(qkv, pos0 = 0)) and attention(rope(qkv, pos0 = 37)), causal, fp32: atol 2e-5, the project's tolerance for
    two fp32 summation orders of one attention.  A q / k inconsistency that the rotation test alone cannot see shows here."""
    from smt_amd import lm as K
    L = 33
    x, _ = R.kernel_case(L, dh, 0)
    table = K.rope_table(37 + L, dh, device=DEV)
    ctx = [K.attention(K.rope(x.to(DEV), table, HEADS, pos0), None, HEADS, True) for pos0 in (0, 37)]
    plain = K.attention(x.to(DEV), None, HEADS, True)
    err = float((ctx[0] - ctx[1]).abs().max())
    print(f"  dh {dh}: max |ctx(pos0 = 0) - ctx(pos0 = 37)| = {err:.3e}")
    assert err <= 2e-5
    assert float((ctx[0] - plain).abs().max()) > 1e-2               # and the rotation changes the attention
    from oracle import lm_oracle as lmo                             # float64 yardstick of the rotated attention itself
    want = lmo.attention_core(R.rope64(x, HEADS, torch.arange(L)), None, HEADS, True, lmo.CounterDropout(), 0)
    assert float((ctx[0].cpu().double() - want).abs().max()) <= 3e-5


def test_rope_argument_errors_by_message():
    from smt_amd import lm as K
    from smt_amd import native as N
    lib = N.lib()
    x = torch.randn(2, 5, 3 * 2 * 32, device=DEV)
    keep = x.clone()
    table = K.rope_table(42, 32, device=DEV)

    def call(qkv, rope, batch, length, heads, dh, rows, pos0):
        N.check(lib.smt_lm_rope(N.ptr(qkv), N.ptr(rope), batch, length, heads, dh, rows, pos0, 0, N.stream_ptr()), "smt_lm_rope")

    with pytest.raises(RuntimeError, match="null pointer"):
        call(None, table, 2, 5, 2, 32, 42, 0)
    with pytest.raises(RuntimeError, match="null pointer"):
        call(x, None, 2, 5, 2, 32, 42, 0)
    for dh in (16, 48, 128):
        with pytest.raises(RuntimeError, match=f"head dim must be 32 or 64 .got {dh}."):
            call(x, table, 2, 5, 2, dh, 42, 0)
    with pytest.raises(RuntimeError, match="outside the rope table"):
        call(x, table, 2, 5, 2, 32, 37 + 5 - 1, 37)                 # rope_rows = pos0 + L - 1
    with pytest.raises(RuntimeError, match="outside the rope table"):
        call(x, table, 2, 5, 2, 32, 42, -1)
    with pytest.raises(RuntimeError, match="below 2.31"):
        call(x, table, 1, 1 << 22, 8, 64, 1 << 22, 0)               # len * 3 * heads * head dim = 2^33 / ... >= 2^31
    call(x, table, 0, 5, 2, 32, 42, 0)                              # batch * len = 0: status 0, no launch
    call(x, table, 2, 0, 2, 32, 42, 0)
    call(None, None, 0, 0, 2, 32, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    with pytest.raises(AssertionError, match="table must be"):
        K.rope(x, K.rope_table(42, 64, device=DEV), 2)


# ------------------------------------------------------------------------------------------------ fused decode attention
L_MAX = 600
POSITIONS = [0, 7, 255, 256, 257, 511]          # the 256-row chunk boundaries tests/test_lm_decode_gpu.py walks


@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("b", [1, 4])
def test_decode_attention_rope_matches_float64(b, dh):
    """ctx against float64 (rotated q against the cached rows and the rotated k), atol 3e-5 -- the existing decode-attention
    test's; cache row pos = the rotated k within the rotation bound, its v the input bit for bit; rows past pos (NaN) never read;
    by-value and device positions give the same bits; rope = None gives the bits of the entry without it."""
    from smt_amd import lm as K
    h = HEADS
    g = torch.Generator().manual_seed(31 * b + dh)
    k_all, v_all = torch.randn(b, h, L_MAX, dh, generator=g), torch.randn(b, h, L_MAX, dh, generator=g)
    table = K.rope_table(L_MAX, dh, device=DEV)
    ws = K.decode_attention_workspace(b, h, L_MAX, DEV, head_dim=dh)
    worst = worst_k = 0.0
    for pos in POSITIONS:
        qkv = torch.randn(b, 3 * h * dh, generator=g)
        rot = R.rope64(qkv[:, None, :], h, torch.tensor([pos]))[:, 0]                 # float64, the step's row at position pos
        q, kn, _ = (t.reshape(b, h, dh) for t in rot.split(h * dh, dim=-1))
        vn = qkv[:, 2 * h * dh:].reshape(b, h, dh)
        kc, vc = k_all.clone(), v_all.clone()
        kc[:, :, pos], vc[:, :, pos] = 7.0, -7.0                                      # stale values the call must replace
        kc[:, :, pos + 1:], vc[:, :, pos + 1:] = float("nan"), float("nan")
        kd, vd = kc.to(DEV), vc.to(DEV)
        ctx = torch.full((b, h * dh), float("nan"), device=DEV)
        qd = qkv.to(DEV)
        K.decode_attention(qd, kd, vd, ctx, ws, pos=pos, rope=table)
        assert torch.equal(qd.cpu(), qkv)                                             # qkv stays as it is
        k64 = torch.cat([k_all[:, :, :pos].double(), kn[:, :, None]], dim=2)
        v64 = torch.cat([v_all[:, :, :pos], vn[:, :, None]], dim=2).double()
        w64 = F.softmax(torch.einsum("bhc,bhjc->bhj", q, k64) / math.sqrt(float(dh)), dim=-1)
        want = torch.einsum("bhj,bhjc->bhc", w64, v64).reshape(b, -1)
        got = ctx.cpu()
        assert torch.isfinite(got).all(), pos
        err = float((got.double() - want).abs().max())
        worst = max(worst, err)
        assert err <= 3e-5, (pos, err)
        # the stored row: [k | v] laid out as the q | k | v of a one-row qkv lets the rotation's own assertion judge it
        stored = torch.cat([kd[:, :, pos].cpu().reshape(b, 1, -1)] * 2 + [vd[:, :, pos].cpu().reshape(b, 1, -1)], dim=-1)
        src = torch.cat([qkv[:, None, h * dh:2 * h * dh]] * 2 + [qkv[:, None, 2 * h * dh:]], dim=-1)
        worst_k = max(worst_k, R.assert_rope(stored, src, h, torch.tensor([pos])))
        assert torch.equal(kd[:, :, :pos].cpu(), k_all[:, :, :pos]) and torch.equal(vd[:, :, :pos].cpu(), v_all[:, :, :pos]), pos
        assert torch.isnan(kd[:, :, pos + 1:]).all() and torch.isnan(vd[:, :, pos + 1:]).all(), pos
        kd2, vd2 = kc.to(DEV), vc.to(DEV)
        again = torch.full_like(ctx, float("nan"))
        K.decode_attention(qd, kd2, vd2, again, ws, pos=0, pos_dev=torch.tensor([pos], dtype=torch.int32, device=DEV), rope=table)
        assert torch.equal(again, ctx) and torch.equal(kd2[:, :, pos], kd[:, :, pos]), pos
        # rope = None: the launch of smt_lm_decode_attention_hd
        outs = []
        for kwargs in (dict(rope=None), dict()):
            kd3, vd3 = kc.to(DEV), vc.to(DEV)
            c3 = torch.full_like(ctx, float("nan"))
            K.decode_attention(qd, kd3, vd3, c3, ws, pos=pos, **kwargs)
            outs.append((c3, kd3[:, :, pos].clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert torch.equal(outs[0][1].cpu(), qkv[:, h * dh:2 * h * dh].reshape(b, h, dh))
    print(f"  batch {b}, dh {dh}: worst |ctx - float64| = {worst:.3e}, worst stored-k ratio of the rotation bound = {worst_k:.3f}")


def test_decode_attention_rope_null_table_through_the_c_entry_and_argument_errors():
    from smt_amd import lm as K
    from smt_amd import native as N
    lib = N.lib()
    b, h, dh, l_max = 2, 2, 32, 40
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(b, 3 * h * dh, generator=g).to(DEV)
    kc, vc = torch.randn(b, h, l_max, dh, generator=g).to(DEV), torch.randn(b, h, l_max, dh, generator=g).to(DEV)
    table = K.rope_table(20, dh, device=DEV)                        # shorter than the cache

    def call(rope, rows, pos, pos_dev=None, head_dim=dh, k=None, v=None, ctx=None):
        k, v = (kc.clone() if k is None else k), (vc.clone() if v is None else v)
        ctx = torch.full((b, h * dh), float("nan"), device=DEV) if ctx is None else ctx
        N.check(lib.smt_lm_decode_attention_rope(N.ptr(qkv), N.ptr(k), N.ptr(v), N.ptr(ctx), None, 0, b, h, l_max, head_dim, N.ptr(rope), rows,
                                                 pos, N.ptr(pos_dev), N.stream_ptr()), "smt_lm_decode_attention_rope")
        return ctx, k, v

    null = call(None, 0, 11)
    ref = (torch.full((b, h * dh), float("nan"), device=DEV), kc.clone(), vc.clone())
    N.check(lib.smt_lm_decode_attention_hd(N.ptr(qkv), N.ptr(ref[1]), N.ptr(ref[2]), N.ptr(ref[0]), None, 0, b, h, l_max, dh, 11, None, N.stream_ptr()),
            "smt_lm_decode_attention_hd")
    assert all(torch.equal(a, c) for a, c in zip(null, ref))
    with pytest.raises(RuntimeError, match="outside the rope table"):
        call(table, 20, 20)                                         # inside the cache, outside the table
    with pytest.raises(RuntimeError, match="outside the cache"):
        call(table, 20, 40)
    with pytest.raises(RuntimeError, match="head dim must be 32 or 64 .got 48."):
        call(table, 20, 0, head_dim=48)
    with pytest.raises(RuntimeError, match="null pointer"):
        N.check(lib.smt_lm_decode_attention_rope(None, N.ptr(kc), N.ptr(vc), N.ptr(ref[0]), None, 0, b, h, l_max, dh, N.ptr(table), 20, 0, None,
                                                 N.stream_ptr()), "smt_lm_decode_attention_rope")
    # a device position outside the table (or the cache): the launch writes nothing
    for bad in (20, 39, 40, -1):
        ctx, k, v = call(table, 20, 0, pos_dev=torch.tensor([bad], dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        assert bool(torch.isnan(ctx).all()) and torch.equal(k, kc) and torch.equal(v, vc), bad
    ctx, k, v = call(table, 20, 0, pos_dev=torch.tensor([19], dtype=torch.int32, device=DEV))      # the last row of the table
    assert bool(torch.isfinite(ctx).all()) and not torch.equal(k[:, :, 19], kc[:, :, 19])
    # the same rule with a cache of several chunks, where a second launch merges the partial softmaxes into ctx
    big_k, big_v = torch.randn(b, h, 600, dh, generator=g).to(DEV), torch.randn(b, h, 600, dh, generator=g).to(DEV)
    ws = K.decode_attention_workspace(b, h, 600, DEV, head_dim=dh)
    long_table = K.rope_table(300, dh, device=DEV)
    for bad in (300, 599):
        k, v, ctx = big_k.clone(), big_v.clone(), torch.full((b, h * dh), float("nan"), device=DEV)
        K.decode_attention(qkv, k, v, ctx, ws, pos_dev=torch.tensor([bad], dtype=torch.int32, device=DEV), rope=long_table)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ctx).all()) and torch.equal(k, big_k) and torch.equal(v, big_v), bad
