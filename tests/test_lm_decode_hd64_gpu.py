"""The one-token attention over the cache and the prompt prefill at head dim 64 (csrc/lm_decode.hip,
smt_lm_decode_attention_hd / smt_lm_decode_prefill_kv_hd through smt_amd.lm, which reads the head dim from the cache shape),
against float64.  Every tolerance is stated where it is asserted."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DH = 64

# csrc/lm_decode.hip at head dim 64: sixteen lanes share a cache row and a wave loads 4 rows per instruction, 32 per pass; the
# four waves of a workgroup cover 128 rows per pass and a workgroup owns 256 rows -> boundaries at 4, 8, 32, 256 and 512
L_MAX = 600
POSITIONS = [0, 1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 511, 512, 513, L_MAX - 1]


def _want(q, k64, v64):
    w64 = F.softmax(torch.einsum("bhc,bhjc->bhj", q.double(), k64) / math.sqrt(float(DH)), dim=-1)
    return torch.einsum("bhj,bhjc->bhc", w64, v64).reshape(q.shape[0], -1)


@pytest.mark.parametrize("b,h", [(1, 1), (3, 2)])
def test_decode_attention_over_the_cache_matches_float64(b, h):
    """softmax(q K^T / sqrt(64)) V over rows 0..pos in float64, atol 3e-5 (tests/test_lm_decode_gpu.py's bound for the same
    arithmetic); cache row pos = the step's k / v bit for bit, earlier rows untouched, later rows (NaN) never read; by-value
    and device-resident positions give the same bits."""
    from smt_amd import lm as K
    g = torch.Generator().manual_seed(17 * b + h)
    k_all, v_all = torch.randn(b, h, L_MAX, DH, generator=g), torch.randn(b, h, L_MAX, DH, generator=g)
    ws = K.decode_attention_workspace(b, h, L_MAX, DEV, head_dim=DH)
    assert ws is not None and ws.numel() == b * h * 3 * (4 + DH) * 4     # L_MAX spans three workgroup chunks
    worst = 0.0
    for pos in POSITIONS:
        qkv = torch.randn(b, 3 * h * DH, generator=g)
        q, kn, vn = (t.reshape(b, h, DH) for t in qkv.split(h * DH, dim=-1))
        kc, vc = k_all.clone(), v_all.clone()
        kc[:, :, pos], vc[:, :, pos] = 7.0, -7.0                       # stale values the call must replace
        kc[:, :, pos + 1:], vc[:, :, pos + 1:] = float("nan"), float("nan")
        kd, vd = kc.to(DEV), vc.to(DEV)
        ctx = torch.full((b, h * DH), float("nan"), device=DEV)
        K.decode_attention(qkv.to(DEV), kd, vd, ctx, ws, pos=pos)
        k64 = torch.cat([k_all[:, :, :pos], kn[:, :, None]], dim=2).double()
        v64 = torch.cat([v_all[:, :, :pos], vn[:, :, None]], dim=2).double()
        got = ctx.cpu()
        assert torch.isfinite(got).all(), pos
        err = float((got.double() - _want(q, k64, v64)).abs().max())
        worst = max(worst, err)
        assert err <= 3e-5, (pos, err)
        assert torch.equal(kd[:, :, pos].cpu(), kn) and torch.equal(vd[:, :, pos].cpu(), vn), pos
        assert torch.equal(kd[:, :, :pos].cpu(), k_all[:, :, :pos]) and torch.equal(vd[:, :, :pos].cpu(), v_all[:, :, :pos]), pos
        assert torch.isnan(kd[:, :, pos + 1:]).all() and torch.isnan(vd[:, :, pos + 1:]).all(), pos
        again = torch.full_like(ctx, float("nan"))
        K.decode_attention(qkv.to(DEV), kd, vd, again, ws, pos=0, pos_dev=torch.tensor([pos], dtype=torch.int32, device=DEV))
        assert torch.equal(again, ctx), pos
    print(f"  {b} x {h} heads: worst |ctx - float64| = {worst:.3e}")


def test_decode_attention_single_chunk_cache_and_bad_position():
    """A cache of at most 256 rows needs no workspace and no merge launch; a by-value position outside the cache is refused
    before anything is launched."""
    from smt_amd import lm as K
    g = torch.Generator().manual_seed(3)
    assert K.decode_attention_workspace(2, 2, 256, DEV, head_dim=DH) is None
    kc, vc = torch.randn(2, 2, 256, DH, generator=g), torch.randn(2, 2, 256, DH, generator=g)
    for pos in (0, 200, 255):
        qkv = torch.randn(2, 3 * 2 * DH, generator=g)
        q, kn, vn = (t.reshape(2, 2, DH) for t in qkv.split(2 * DH, dim=-1))
        kd, vd = kc.to(DEV), vc.to(DEV)
        kd[:, :, pos + 1:], vd[:, :, pos + 1:] = float("nan"), float("nan")
        ctx = torch.empty(2, 2 * DH, device=DEV)
        K.decode_attention(qkv.to(DEV), kd, vd, ctx, None, pos=pos)
        k64 = torch.cat([kc[:, :, :pos], kn[:, :, None]], dim=2).double()
        v64 = torch.cat([vc[:, :, :pos], vn[:, :, None]], dim=2).double()
        assert float((ctx.cpu().double() - _want(q, k64, v64)).abs().max()) <= 3e-5, pos
    before = (kd.clone(), vd.clone(), ctx.clone())
    for pos in (256, -1):
        with pytest.raises(RuntimeError, match="outside the cache"):
            K.decode_attention(qkv.to(DEV), kd, vd, ctx, None, pos=pos)
    torch.cuda.synchronize()
    assert all(torch.equal(a.nan_to_num(1.5), c.nan_to_num(1.5)) for a, c in zip(before, (kd, vd, ctx)))


@pytest.mark.parametrize("length", [1, 33])
def test_prefill_kv_copies_the_rows_bit_for_bit(length):
    from smt_amd import lm as K
    b, h, l_max = 3, 2, 40
    d = h * DH
    qkv = torch.randn(b, length, 3 * d, generator=torch.Generator().manual_seed(100 * b + length)).to(DEV)
    kc = torch.full((b, h, l_max, DH), -7.5, device=DEV)
    vc = torch.full((b, h, l_max, DH), 9.25, device=DEV)
    K.decode_prefill_kv(qkv, kc, vc)
    k, v = (qkv[:, :, j * d:(j + 1) * d].reshape(b, length, h, DH).permute(0, 2, 1, 3) for j in (1, 2))
    assert torch.equal(kc[:, :, :length], k) and torch.equal(vc[:, :, :length], v)
    assert bool((kc[:, :, length:] == -7.5).all()) and bool((vc[:, :, length:] == 9.25).all())


def test_the_c_entries_refuse_other_head_dims_with_no_launch():
    from smt_amd import native as N
    lib = N.lib()
    qkv = torch.randn(1, 3 * 128, device=DEV)
    kc, vc = torch.full((1, 1, 4, 128), float("nan"), device=DEV), torch.full((1, 1, 4, 128), float("nan"), device=DEV)
    ctx = torch.full((1, 128), float("nan"), device=DEV)
    for head_dim in (48, 128):
        with pytest.raises(RuntimeError, match=f"head dim must be 32 or 64 .got {head_dim}."):
            N.check(lib.smt_lm_decode_attention_hd(N.ptr(qkv), N.ptr(kc), N.ptr(vc), N.ptr(ctx), None, 0, 1, 1, 4, head_dim, 0, None, N.stream_ptr()),
                    "smt_lm_decode_attention_hd")
        with pytest.raises(RuntimeError, match=f"head dim must be 32 or 64 .got {head_dim}."):
            N.check(lib.smt_lm_decode_prefill_kv_hd(N.ptr(qkv), N.ptr(kc), N.ptr(vc), 1, 1, 1, 4, head_dim, N.stream_ptr()),
                    "smt_lm_decode_prefill_kv_hd")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (kc, vc, ctx))
