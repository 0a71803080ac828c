"""VQTTS text-audio alignment on the HIP library (include/smt_hip.h, "VQTTS alignment"): the Euclidean distance between
text-encoder means and audio-encoder frames, the monotonic search over it and the loss on the found path.  fp32,
channels-last rows [B, T, D], prefix masks as int32 lengths on the device, no host synchronisation.
Reference: models/vqtts/vqtts.py:133-137, 150-156."""
import torch

from . import native as N
from . import profiler

# the fused search's own constants (csrc/vqtts_align.hip): columns per distance slab, columns per backtrack chunk,
# columns per walk step, rows per ballot word
ALIGN_SLAB, ALIGN_CHUNK, ALIGN_WALK, ALIGN_WORD = 32, 512, 64, 64


def _f(t):
    assert t.dtype == torch.float32 and t.is_cuda, "the VQTTS alignment kernels take fp32 device tensors"
    return t.contiguous()


def _i(t):
    assert t.is_cuda
    return (t if t.dtype == torch.int32 else t.to(torch.int32)).contiguous()


def _shapes(x_enc, y_enc):
    b, tx, d = x_enc.shape
    assert y_enc.dim() == 3 and y_enc.shape[0] == b and y_enc.shape[2] == d, "x_enc [B, Tx, D] and y_enc [B, Tq, D]"
    return b, tx, y_enc.shape[1], d


@torch.no_grad()
def distance(x_enc, y_enc):
    """dist [B, Tx, Tq] = |x_enc[b, i] - y_enc[b, j]|_2, dense (tests and small shapes; ``align`` never builds it)."""
    x_enc, y_enc = _f(x_enc), _f(y_enc)
    b, tx, tq, d = _shapes(x_enc, y_enc)
    dist = torch.empty(b, tx, tq, device=x_enc.device)
    N.check(N.lib().smt_vqtts_distance(N.ptr(x_enc), N.ptr(y_enc), N.ptr(dist), b, tx, tq, d, N.stream_ptr()), "smt_vqtts_distance")
    return dist


@torch.no_grad()
def align(x_enc, y_enc, x_lens, q_lens):
    """Monotonic alignment of frames to tokens under the negated distance: (idx [B, Tq] int32, the token of each frame,
    -1 = none; dur [B, Tx] fp32, frames per token) -- ``maximum_path(-distances, x_mask (x) q_mask)`` of the reference in
    the index form of ``glow.align_index``, without the distance matrix."""
    x_enc, y_enc = _f(x_enc), _f(y_enc)
    b, tx, tq, d = _shapes(x_enc, y_enc)
    x_lens, q_lens = _i(x_lens), _i(q_lens)
    assert x_lens.shape == (b,) and q_lens.shape == (b,)
    idx = torch.empty(b, tq, dtype=torch.int32, device=x_enc.device)
    dur = torch.empty(b, tx, device=x_enc.device)
    lib = N.lib()
    ws = N.workspace.get(max(int(lib.smt_vqtts_align_workspace_bytes(b, tx, tq)), 16), x_enc.device)
    with profiler.region("vqtts_align", flops=3.0 * b * tx * tq * d, bound="valu", dtype="f32"):
        N.check(lib.smt_vqtts_align(N.ptr(x_enc), N.ptr(y_enc), N.ptr(x_lens), N.ptr(q_lens), b, tx, tq, d, N.ptr(idx), N.ptr(dur),
                                    N.ptr(ws), ws.numel(), N.stream_ptr()), "smt_vqtts_align")
    return idx, dur


class _AlignLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_enc, y_enc, idx, denom):
        x_enc, y_enc = _f(x_enc), _f(y_enc)
        b, tx, tq, d = _shapes(x_enc, y_enc)
        idx = _i(idx)
        assert idx.shape == (b, tq)
        fd = torch.empty(b, tq, device=x_enc.device)
        s = torch.empty(1, device=x_enc.device)
        with profiler.region("vqtts_align_loss:fwd", nbytes=2 * y_enc.numel() * 4, bound="hbm"):
            N.check(N.lib().smt_vqtts_align_loss(N.ptr(x_enc), N.ptr(y_enc), N.ptr(idx), b, tx, tq, d, N.ptr(fd), N.ptr(s), N.stream_ptr()),
                    "smt_vqtts_align_loss")
        ctx.save_for_backward(x_enc, y_enc, idx, fd, denom)
        return s[0] / denom

    @staticmethod
    def backward(ctx, g):
        x_enc, y_enc, idx, fd, denom = ctx.saved_tensors
        b, tx, tq, d = _shapes(x_enc, y_enc)
        coef = (g / denom).reshape(1).float().contiguous()
        dx, dy = torch.empty_like(x_enc), torch.empty_like(y_enc)
        with profiler.region("vqtts_align_loss:bwd", nbytes=4 * y_enc.numel() * 4, bound="hbm"):
            N.check(N.lib().smt_vqtts_align_loss_bwd(N.ptr(x_enc), N.ptr(y_enc), N.ptr(idx), N.ptr(fd), N.ptr(coef), b, tx, tq, d, N.ptr(dx),
                                                     N.ptr(dy), N.stream_ptr()), "smt_vqtts_align_loss_bwd")
        return dx, dy, None, None


def align_loss(x_enc, y_enc, idx, denom):
    """sum over the frames with a token of |x_enc[b, idx[b, j]] - y_enc[b, j]|_2, divided by ``denom`` (a device scalar) --
    ``(distances * attn).sum() / attn_mask.sum()`` of the reference on the path.  Gradients to both encodings; a frame at
    distance exactly 0 contributes none (the reference's sqrt backward gives NaN there)."""
    return _AlignLoss.apply(x_enc, y_enc, idx, denom)
