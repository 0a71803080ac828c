"""VQTTS text-audio alignment on the HIP library (include/smt_hip.h, "VQTTS alignment"): the Euclidean distance between
text-encoder means and audio-encoder frames, the monotonic search over it and the loss on the found path.  fp32,
channels-last rows [B, T, D], prefix masks as int32 lengths on the device, no host synchronisation.
Reference: models/vqtts/vqtts.py:133-137, 150-156.

The code head ("VQTTS code head" of the header, csrc/vqtts_codes.hip): the projection to l_bins logits fused with the
cross-entropy, the argmax or a draw (``code_head_sample``) -- reference models/vqtts/vqtts.py:144, 157, 176, 190.

The code emission ("VQTTS code emission", csrc/vqtts_emit.hip): predicted code -> absolute code and codebook row, the
synthesis side of the grouped bottleneck -- reference models/vqtts/vqtts.py:170-174."""
import math

import torch

from . import packing
from . import native as N
from . import profiler

# the fused search's own constants (csrc/vqtts_align.hip): columns per distance slab, columns per backtrack chunk,
# columns per walk step, rows per ballot word
ALIGN_SLAB, ALIGN_CHUNK, ALIGN_WALK, ALIGN_WORD = 32, 512, 64, 64
# the code head's constants (csrc/vqtts_codes.hip, CH_*): rows per workgroup of the row kernels, weight rows staged per step,
# columns of V per workgroup and rows per slice of the weight-gradient kernel, the most slabs its reduce adds, the most
# partial sums of the forward's reduce, the limits
CH_ROWS, CH_VT, CH_VCOLS, CH_SLICE, CH_MAX_SLICES, CH_SUM_PARTS, CH_MAX_C, CH_MAX_V = 128, 64, 64, 4096, 256, 256, 256, 1024


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


# ------------------------------------------------------------------------------------------------------- code head
class WeightSplit:
    """The bf16-pair split of one projection weight (smt_vqtts_code_head_prepare), kept by whoever owns the weight and
    redone when the weight has or may have changed.  The key is the weight's (data_ptr, _version) -- the rule of
    ``Bottleneck._search_prep`` -- and the generation of ``packing.mark_dirty``: a fused optimizer step
    writes the parameters without moving ``_version``, and every optimizer step, every training forward of a module of this
    build, ``EMA.swap`` and ``load_checkpoint`` announce themselves there (the packed conv operands obey the same signal)."""

    def __init__(self):
        self.key, self.buf = None, None

    def get(self, weight):
        key = (weight.data_ptr(), weight._version, packing.generation(), tuple(weight.shape), weight.device)
        if self.key != key:
            v, c = weight.shape
            lib = N.lib()
            need = max(int(lib.smt_vqtts_code_head_workspace_bytes(c, v)), 16)
            if self.buf is None or self.buf.numel() < need or self.buf.device != weight.device:
                self.buf = torch.empty(need, dtype=torch.uint8, device=weight.device)
            N.check(lib.smt_vqtts_code_head_prepare(N.ptr(weight), c, v, N.ptr(self.buf), self.buf.numel(), N.stream_ptr()),
                    "smt_vqtts_code_head_prepare")
            self.key = key
        return self.buf


def _split_of(weight, split):
    """Without a ``WeightSplit`` of the caller's the weight is split for this call alone (one small launch)."""
    return (split if split is not None else WeightSplit()).get(weight)


def _head_args(h, weight, bias):
    h, weight, bias = _f(h), _f(weight.reshape(weight.shape[0], -1)), _f(bias)
    v, c = weight.shape
    assert h.shape[-1] == c and bias.shape == (v,), "h [..., C], weight [V, C] (or [V, C, 1]) and bias [V]"
    return h, weight, bias, h.numel() // c if c else 0, c, v


def _head_fwd(h, weight, bias, target, want_lse, split=None):
    h, weight, bias, n, c, v = _head_args(h, weight, bias)
    ws = _split_of(weight.detach(), split)
    dev = h.device
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    lse = torch.empty(n, device=dev) if want_lse or target is not None else None
    row_loss = correct = sums = None
    if target is not None:
        assert target.dtype == torch.int64 and target.numel() == n and target.is_cuda
        target = target.reshape(n).contiguous()
        row_loss, correct = torch.empty(n, device=dev), torch.empty(n, device=dev)
        # three sums, then the partial sums of the reduce's first stage; no rows: no target pointer, the sums are zero
        sums = (torch.empty if n else torch.zeros)(3 + 3 * CH_SUM_PARTS, dtype=torch.float64, device=dev)
    with profiler.region("vqtts_code_head:fwd", flops=6.0 * n * c * v, bound="mfma", dtype="bf16"):
        N.check(N.lib().smt_vqtts_code_head_fwd(N.ptr(h), N.ptr(ws), ws.numel(), N.ptr(bias), N.ptr(target), n, c, v, N.ptr(lse),
                                                N.ptr(row_loss), N.ptr(pred), N.ptr(correct), N.ptr(sums), N.stream_ptr()),
                "smt_vqtts_code_head_fwd")
    return h, weight, bias, target, ws, lse, row_loss, correct, sums, pred


class _CodeHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, bias, target, split):
        shape = h.shape[:-1]
        h2, w2, bias, target, ws, lse, row_loss, _, sums, pred = _head_fwd(h, weight, bias, target, True, split)
        count = sums[2]
        denom = torch.clamp(count, min=1.0)
        loss = (sums[0] / denom).float()
        acc = (sums[1] / denom).float()
        ctx.save_for_backward(h2, w2, bias, target, lse, denom, ws)
        ctx.shapes = (h.shape, weight.shape)
        pred = pred.view(shape)
        count = count.to(torch.int64)
        ctx.mark_non_differentiable(acc, count, pred)
        return loss, acc, count, pred

    @staticmethod
    def backward(ctx, g, *_unused):
        h, weight, bias, target, lse, denom, ws = ctx.saved_tensors
        n, c = h.numel() // h.shape[-1], h.shape[-1]
        v = weight.shape[0]
        coef = (g.double() / denom).float().reshape(1).contiguous()
        dh, dw, db = torch.empty_like(h), torch.empty_like(weight), torch.empty_like(bias)
        lib = N.lib()
        scratch = N.workspace.get(max(int(lib.smt_vqtts_code_head_bwd_workspace_bytes(n, c, v)), 16), h.device)
        with profiler.region("vqtts_code_head:bwd", flops=18.0 * n * c * v, bound="mfma", dtype="bf16"):
            N.check(lib.smt_vqtts_code_head_bwd(N.ptr(h), N.ptr(ws), ws.numel(), N.ptr(bias), N.ptr(target), N.ptr(lse), N.ptr(coef), n,
                                                c, v, N.ptr(dh), N.ptr(dw), N.ptr(db), N.ptr(scratch), scratch.numel(),
                                                N.stream_ptr()), "smt_vqtts_code_head_bwd")
        h_shape, w_shape = ctx.shapes
        return dh.view(h_shape), dw.view(w_shape), db, None, None


def code_head(h, weight, bias, target, split=None):
    """(loss, accuracy, count, pred): the mean over the rows with ``target >= 0`` of the cross-entropy of
    ``h @ weight.T + bias`` against ``target``, the share of those rows whose argmax is the target, their number (int64)
    and the argmax of every row (int32, lowest index on ties) -- ``F.cross_entropy(quant_proj(y_qh), y_q)`` and ``q_acc`` of
    the reference without the logits.  h [..., C] fp32, weight [V, C] or the conv layout [V, C, 1], target int64 of h's
    leading shape; no rows give loss 0 and count 0.  Gradients to h, weight and bias; the other three results are not
    differentiable.  ``split``: the owner's ``WeightSplit`` (the split is then kept until the weight changes)."""
    return _CodeHead.apply(h, weight, bias, target, split)


@torch.no_grad()
def code_head_predict(h, weight, bias, split=None):
    """pred [...] int32 = argmax of ``h @ weight.T + bias`` over the bins, lowest index on ties (the synthesis form)."""
    shape = h.shape[:-1]
    return _head_fwd(h, weight, bias, None, False, split)[-1].view(shape)


def sample_cut(temperature, min_p):
    """(1 / T, cut = T ln(min_p)) as the floats the C entry takes; the cut is computed in double and rounded once (by the
    binding's conversion to float), -inf for min_p = 0.  ValueError for a temperature that is not finite and > 0 or a min_p
    outside [0, 1]."""
    temperature, min_p = float(temperature), float(min_p)
    if not (math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"code_head_sample: temperature must be a finite number > 0, got {temperature}")
    if not 0.0 <= min_p <= 1.0:
        raise ValueError(f"code_head_sample: min_p must lie in [0, 1], got {min_p}")
    return 1.0 / temperature, (temperature * math.log(min_p) if min_p > 0 else -math.inf)


@torch.no_grad()
def code_head_sample(h, weight, bias, seeds, t_q, temperature, min_p=0.0, split=None, want_kept=False):
    """pred [N] int32: one draw per row of ``h`` [..., C] from softmax((h @ weight.T + bias) / temperature), restricted to
    the bins with p >= min_p * p_max (min-p; 0 keeps all) -- "VQTTS code head", sample, of the header: Gumbel-max inside
    the fused sweep, no [N, V] tensor.  Row r is frame r % t_q of item r // t_q and draws with (seeds[r // t_q], r % t_q)
    alone; seeds [N / t_q] int32 on the device.  ``want_kept`` adds n_kept [N] int32, the size of each row's kept set.  Not
    differentiable.  ``split``: the owner's ``WeightSplit``."""
    inv_t, cut = sample_cut(temperature, min_p)
    h, weight, bias, n, c, v = _head_args(h, weight, bias)
    t_q = int(t_q)
    if t_q < 1 or n % t_q:
        raise ValueError(f"code_head_sample: {n} rows are not a whole number of items of t_q = {t_q} frames")
    if not (isinstance(seeds, torch.Tensor) and seeds.dtype == torch.int32 and seeds.is_cuda and tuple(seeds.shape) == (n // t_q,)):
        raise ValueError(f"code_head_sample: seeds must be an int32 device tensor of shape ({n // t_q},)")
    ws = _split_of(weight.detach(), split)
    pred = torch.empty(n, dtype=torch.int32, device=h.device)
    kept = torch.empty(n, dtype=torch.int32, device=h.device) if want_kept else None
    with profiler.region("vqtts_code_head:sample", flops=(12.0 if min_p > 0 else 6.0) * n * c * v, bound="mfma", dtype="bf16"):
        N.check(N.lib().smt_vqtts_code_head_sample(N.ptr(h), N.ptr(ws), ws.numel(), N.ptr(bias), N.ptr(seeds.contiguous()), n, t_q, c, v,
                                                   inv_t, cut, N.ptr(pred), N.ptr(kept), N.stream_ptr()),
                "smt_vqtts_code_head_sample")
    return (pred, kept) if want_kept else pred


# --------------------------------------------------------------------------------------------------- code emission
@torch.no_grad()
def emit_codes(pred, x_id, align_idx, q_lens, codebook, n_vocab, l_bins):
    """(y_d [B, Tq, D] fp32, q_abs [B, Tq] int64): frame (b, j) with a code -- j < q_lens[b], a token index in
    [0, Tx), a token id in [0, n_vocab) and pred in [0, l_bins) -- gets q_abs = token * l_bins + pred and the codebook row
    of it, every other frame -1 and an exactly zero row ("VQTTS code emission" of the header, csrc/vqtts_emit.hip).  One
    launch for ``CodePredictor.synthesize_codes`` -> ``Bottleneck.decode`` -> the length mask.  pred [B, Tq] int32,
    x_id [B, Tx] int64, align_idx [B, Tq] int32, q_lens [B] int32, codebook [n_vocab * l_bins, D] fp32 with D % 4 == 0;
    anything else raises ValueError before the launch."""
    def need(cond, what):
        if not cond:
            raise ValueError(f"emit_codes: {what}")
    for name, t, dtype, dim in (("pred", pred, torch.int32, 2), ("x_id", x_id, torch.int64, 2), ("align_idx", align_idx, torch.int32, 2),
                                ("q_lens", q_lens, torch.int32, 1), ("codebook", codebook, torch.float32, 2)):
        need(isinstance(t, torch.Tensor) and t.dtype == dtype and t.dim() == dim and t.is_cuda,
             f"{name} must be a {dim}-D {dtype} device tensor, got "
             f"{(t.dtype, tuple(t.shape), t.device.type) if isinstance(t, torch.Tensor) else type(t).__name__}")
    b, tq = pred.shape
    tx, (rows, d) = x_id.shape[1], codebook.shape
    need(x_id.shape[0] == b and tuple(align_idx.shape) == (b, tq) and tuple(q_lens.shape) == (b,),
         f"pred {tuple(pred.shape)}, x_id {tuple(x_id.shape)}, align_idx {tuple(align_idx.shape)} and q_lens {tuple(q_lens.shape)} "
         "do not agree on [B, Tq] / [B, Tx] / [B]")
    need(n_vocab >= 0 and l_bins >= 0 and rows == n_vocab * l_bins, f"codebook has {rows} rows, n_vocab * l_bins = {n_vocab * l_bins}")
    need(d % 4 == 0, f"the code width {d} is not a multiple of 4")
    dev = codebook.device
    y_d = torch.empty(b, tq, d, device=dev)
    q_abs = torch.empty(b, tq, dtype=torch.int64, device=dev)
    pred, x_id, align_idx, q_lens, codebook = (t.detach().contiguous() for t in (pred, x_id, align_idx, q_lens, codebook))
    with profiler.region("vqtts_emit", nbytes=2 * y_d.numel() * 4, bound="hbm"):
        N.check(N.lib().smt_vqtts_emit(N.ptr(pred), N.ptr(x_id), N.ptr(align_idx), N.ptr(q_lens), N.ptr(codebook), b, tx, tq, n_vocab,
                                       l_bins, d, N.ptr(q_abs), N.ptr(y_d), N.stream_ptr()), "smt_vqtts_emit")
    return y_d, q_abs
