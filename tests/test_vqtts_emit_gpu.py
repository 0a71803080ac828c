"""smt_vqtts_emit (csrc/vqtts_emit.hip) through smt_amd.vqtts.emit_codes against plain torch indexing, bit for bit: every
way a frame can be without a code gives the zero row and -1, every other frame its codebook row and absolute code."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_VOCAB, L_BINS, TX = 5, 7, 6


def _inputs(b, tq, d, seed):
    g = torch.Generator().manual_seed(seed)
    rows = N_VOCAB * L_BINS
    # distinct values everywhere: row r, column c holds r + c / 1024 (exact in fp32), so a wrong row or column cannot pass
    codebook = torch.arange(rows, dtype=torch.float32)[:, None] + torch.arange(d, dtype=torch.float32)[None, :] / 1024.0
    codebook[3, 0] = -0.0                                                       # a sign bit that only a bit-exact copy keeps
    x_id = torch.randint(0, N_VOCAB, (b, TX), generator=g)
    idx = torch.randint(0, TX, (b, tq), generator=g, dtype=torch.int32)
    pred = torch.randint(0, L_BINS, (b, tq), generator=g, dtype=torch.int32)
    q_lens = torch.full((b,), tq, dtype=torch.int32)
    if b >= 2:
        q_lens[1] = 0                                                           # a whole item without frames
        x_id[0, 1], x_id[0, 2] = -1, N_VOCAB                                    # token ids just outside the vocabulary
        x_id[b - 1, 0] = N_VOCAB - 1
    if b >= 3:
        q_lens[2] = tq - 5                                                      # frames at or past q_lens
    flat = lambda t: t.view(-1)                                                 # noqa: E731
    n = b * tq
    if n >= 12:                                                                 # plant every kind of frame without a code
        flat(idx)[0], flat(idx)[1], flat(idx)[2] = -1, TX, TX + 100
        flat(pred)[3], flat(pred)[4] = -1, L_BINS
        flat(idx)[5], flat(idx)[6] = 1, 2                                       # item 0's tokens -1 and n_vocab (b >= 2)
        flat(idx)[7], flat(pred)[7] = -2 ** 31, 0
        flat(idx)[8], flat(pred)[8] = 0, 2 ** 31 - 1
        flat(idx)[tq - 1], flat(pred)[tq - 1] = 0, L_BINS - 1                   # item 0's last frame: the last bin of its token
    return pred, x_id, idx, q_lens, codebook


def _reference(pred, x_id, idx, q_lens, codebook):
    """The contract in plain torch indexing (CPU)."""
    b, tq = pred.shape
    tx = x_id.shape[1]
    j = torch.arange(tq)[None, :]
    i = idx.long()
    ok = (j < q_lens[:, None]) & (i >= 0) & (i < tx)
    tok = torch.gather(x_id, 1, i.clamp(0, tx - 1))
    ok &= (tok >= 0) & (tok < N_VOCAB) & (pred >= 0) & (pred < L_BINS)
    q = torch.where(ok, tok * L_BINS + pred.long(), torch.full_like(tok, -1))
    y = torch.where(ok[..., None], codebook[q.clamp(min=0)], torch.zeros(()))
    return y, q


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("b,tq", [(1, 1), (3, 37), (2, 300)])
@pytest.mark.parametrize("d", [4, 64, 128, 132])
def test_emit_is_bit_identical_to_indexing(b, tq, d):
    from smt_amd import native as N
    from smt_amd import vqtts
    pred, x_id, idx, q_lens, codebook = _inputs(b, tq, d, seed=100 * d + tq)
    want_y, want_q = _reference(pred, x_id, idx, q_lens, codebook)
    if b * tq >= 12:                                                            # the planted frames are what they were meant to be
        assert (want_q.view(-1)[:9] == -1).all() and (want_q[0, 9:] >= 0).any()
        assert want_q[0, tq - 1] == x_id[0, 0] * L_BINS + L_BINS - 1
    if b >= 2:
        assert (want_q[1] == -1).all()
    if b >= 3:
        assert (want_q[2, tq - 5:] == -1).all() and (want_q[2, :tq - 5] >= 0).any()
    dev = [t.to(DEV) for t in (pred, x_id, idx, q_lens, codebook)]
    y, q = vqtts.emit_codes(*dev, N_VOCAB, L_BINS)
    assert y.shape == (b, tq, d) and y.dtype == torch.float32 and q.shape == (b, tq) and q.dtype == torch.int64
    assert torch.equal(q.cpu(), want_q)
    assert torch.equal(_bits(y.cpu()), _bits(want_y))                           # bits: -0.0 stays -0.0, no row is NaN
    assert (y.cpu()[want_q == -1] == 0).all() and not torch.signbit(y.cpu()[want_q == -1]).any()     # exactly +0.0f
    y2, q2 = vqtts.emit_codes(*dev, N_VOCAB, L_BINS)
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(q2, q)              # equal inputs, equal bits

    # the entry point itself on buffers pre-filled with NaN / a sentinel: every element is written; q_abs may be NULL
    yb = torch.full((b, tq, d), float("nan"), device=DEV)
    qb = torch.full((b, tq), 12345, dtype=torch.int64, device=DEV)
    args = [N.ptr(t) for t in dev] + [b, TX, tq, N_VOCAB, L_BINS, d]
    N.check(N.lib().smt_vqtts_emit(*args, N.ptr(qb), N.ptr(yb), N.stream_ptr()), "smt_vqtts_emit")
    assert torch.equal(_bits(yb.cpu()), _bits(want_y)) and torch.equal(qb.cpu(), want_q)
    yb.fill_(float("nan"))
    N.check(N.lib().smt_vqtts_emit(*args, None, N.ptr(yb), N.stream_ptr()), "smt_vqtts_emit")
    assert torch.equal(_bits(yb.cpu()), _bits(want_y))


def test_emit_replaces_the_torch_chain():
    """On frames that all have a code the call equals synthesize_codes -> Bottleneck.decode -> length mask."""
    from models.vqtts import Bottleneck, CodePredictor
    from smt_amd import vqtts
    torch.manual_seed(5)
    b, tq, d, n_vocab, l_bins = 2, 50, 32, 4, 32
    bott = Bottleneck(n_vocab, l_bins, d, 0.99, 1.0).to(DEV)
    bott.k.copy_(torch.randn(n_vocab * l_bins, d))
    head = CodePredictor(d, l_bins)                              # stays on the CPU: synthesize_codes touches no parameter, only l_bins
    x_id = torch.randint(0, n_vocab, (b, 9), device=DEV)
    idx = torch.randint(0, 9, (b, tq), device=DEV, dtype=torch.int32)
    pred = torch.randint(0, l_bins, (b, tq), device=DEV, dtype=torch.int32)
    q_lens = torch.tensor([tq, 31], dtype=torch.int32, device=DEV)
    keep = torch.arange(tq, device=DEV)[None, :] < q_lens[:, None]
    q_chain = head.synthesize_codes(pred, x_id, idx)
    y_chain = bott.decode(q_chain) * keep[..., None]
    y, q = vqtts.emit_codes(pred, x_id, idx, q_lens, bott.k, n_vocab, l_bins)
    assert torch.equal(y, y_chain) and torch.equal(q[keep], q_chain[keep]) and (q[~keep] == -1).all()


def test_emit_arguments():
    from smt_amd import native as N
    from smt_amd import vqtts

    def call(b=2, tq=5, d=8, rows=N_VOCAB * L_BINS, **over):
        a = dict(pred=torch.zeros(b, tq, dtype=torch.int32, device=DEV), x_id=torch.zeros(b, TX, dtype=torch.int64, device=DEV),
                 align_idx=torch.zeros(b, tq, dtype=torch.int32, device=DEV), q_lens=torch.full((b,), tq, dtype=torch.int32, device=DEV),
                 codebook=torch.ones(rows, d, device=DEV))
        a.update(over)
        return vqtts.emit_codes(a["pred"], a["x_id"], a["align_idx"], a["q_lens"], a["codebook"], N_VOCAB, L_BINS)
    with pytest.raises(ValueError, match="multiple of 4"):
        call(d=6)
    with pytest.raises(ValueError, match="pred"):
        call(pred=torch.zeros(2, 5, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="x_id"):
        call(x_id=torch.zeros(2, TX, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="q_lens"):
        call(q_lens=torch.zeros(2, 1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="codebook"):
        call(codebook=torch.ones(3, 8, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="do not agree"):
        call(align_idx=torch.zeros(2, 6, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="rows"):
        call(rows=N_VOCAB * L_BINS + 1)
    with pytest.raises(ValueError, match="device tensor"):
        call(pred=torch.zeros(2, 5, dtype=torch.int32))
    y, q = call(b=0)
    assert y.shape == (0, 5, 8) and q.shape == (0, 5) and q.dtype == torch.int64
    y, q = call(tq=0)
    assert y.shape == (2, 0, 8) and q.shape == (2, 0)
    y, q = call()
    assert (y == 1).all() and (q == 0).all()
    # the library refuses what the wrapper refuses: dim 6, and a row pointer that is not 16-byte aligned
    z = torch.zeros(2, 5, dtype=torch.int32, device=DEV)
    x = torch.zeros(2, TX, dtype=torch.int64, device=DEV)
    ql = torch.full((2,), 5, dtype=torch.int32, device=DEV)
    cb, out = torch.ones(N_VOCAB * L_BINS * 8 + 4, device=DEV), torch.zeros(2 * 5 * 8 + 4, device=DEV)
    lib = N.lib()

    def raw(cb_ptr, out_ptr, d):
        return lib.smt_vqtts_emit(N.ptr(z), N.ptr(x), N.ptr(z), N.ptr(ql), cb_ptr, 2, TX, 5, N_VOCAB, L_BINS, d, None, out_ptr, N.stream_ptr())
    assert raw(N.ptr(cb), N.ptr(out), 6) != 0 and "multiple of 4" in lib.smt_last_error().decode()
    assert raw(ctypes.c_void_p(cb.data_ptr() + 4), N.ptr(out), 8) != 0 and "16-byte aligned" in lib.smt_last_error().decode()
    assert raw(N.ptr(cb), ctypes.c_void_p(out.data_ptr() + 4), 8) != 0
    assert raw(N.ptr(cb), N.ptr(out), 8) == 0
    torch.cuda.synchronize()
    assert (out[:80] == 1).all() and (out[80:] == 0).all()
