"""Shared by the float64 tests of the VQ-VAE's boundary and resampling kernels: csrc/conv_misc.hip (conv_in, conv_out, gate_mix) and
csrc/conv_resample.hip (smt_conv4s2 / smt_convt4s2) with the generic kernel's stride-2 and phase-split launches (csrc/conv.hip).
Every reference is a plain float64 evaluation on the operands AS THE KERNEL READS THEM (bf16-rounded where it reads bf16) and
returns (value, bound); the magnitude `mag` of a bound is computed by hand next to its value, as conv_ref_helpers.conv_ref does.
tests/test_conv_edge_cpu.py pins every reference to the torch functional and its autograd in float64, shows that an fp32
emulation of each kernel's arithmetic stays inside the bound, and that the bounds have teeth.  The tests allow SLACK = 2 times a
bound (conv_ref_helpers.py explains the factor: 2^-9 is the bf16 rounding step at the top of a binade, 2^-8 at the bottom).

Resampling convs (k = 4, stride 2, padding 1; header of csrc/conv_resample.hip).  Rows of x at t >= lens_in[b] read as zero, rows
of y at t >= lens_out[b] are exact zeros, there is no residual:

    strided     y[t]    = b + sum_j W_j x[2 t + j - 1]                                   n = 4 c_in
    transposed  y[2m]   = b + W_1 x[m] + W_3 x[m - 1]      y[2m+1] = b + W_2 x[m] + W_0 x[m + 1]      n = 2 c_in per phase

    |y - y64| <= n * 2^-23 * mag + 2^-9 * |y64|,      mag = |b| + (|x| conv |W|)

The first term is the fp32 accumulation (MFMA chains, then the bias add); the second is the ONE rounding to bf16.  Read in the
code: the streaming kernels' rs_store packs (acc + bias) * keep straight from the fp32 accumulators (pack_bf16x2, one conversion);
the generic kernel stages (T)(acc + bias) through LDS ("bias joins in fp32 before the (single, for residual-free layers) rounding
to T") and, with neither an activation derivative nor a residual, multiplies that bf16 value by the 0 / 1 row mask and converts it
again, which changes nothing.  The fp32 path has no rounding term.  Where the bound is 0 (masked output rows) the kernel must give
exactly 0.  Their weight and bias gradients keep the project's bound for those (conv_ref_helpers.wgrad_bounds).

conv_in (c_in = 1, taps <= 8, x and w fp32): one fma per tap on top of the bias, so (taps + 1) * 2^-23 * mag, plus 2^-9 |y| for
a bf16 output.  conv_out (c_out = 1): c_in fmas and the bias add in any order (a lane's chain, then a shuffle tree), so
(c_in + 1) * 2^-23 * mag; padded rows give y = bias and dx = 0 exactly and still count in db; dx = dy * w is one product (2^-23,
doubled by SLACK to cover nothing more than itself), rounded once when it is bf16.  Every dW / db of the two is an fp32 sum over
the rows of the launch in an order the test does not assume (lanes, waves, workgroup slabs, a reduce kernel): the order-free
(rows + 1) * 2^-23 * sum |terms| of lm_linear_helpers.bound.  dy is read rounded when it is bf16.

gate_mix: g = sum_d tanh(t_d) p_d, p = softmax_d(s_d), and its backward dt_d = dg p_d (1 - tanh^2 t_d),
ds_d = dg p_d (tanh t_d - g).  The kernels use hardware intrinsics (gate_tanh = 1 - 2 rcp(exp2(2 x log2 e) + 1), __expf, rcp for
the bf16 results and IEEE divisions for fp32), so the bound has a derived FORM and one measured constant K per dtype:

  * gate_tanh cancels near zero: the error of rcp(e + 1) is relative to a value near 1/2, so the error of tanh is ABSOLUTE, a
    few 2^-23, whatever |tanh| is.  One unit: a = 2^-23.
  * a softmax weight is a quotient of exponentials: its error is RELATIVE.  exp(s_d - m) through exp2 multiplies the argument by
    log2 e in fp32, which costs |s_d - m| * 2^-24 of the result; the denominator is a sum of `depth` such terms.  In units of 2^-23:
    r_d = depth + 2 + |s_d - m| + sum_k p_k |s_k - m|      (own exponential, the p-weighted ones of the denominator, the additions,
    the reciprocal or division and the products that follow).
  * an exponential or a result below the smallest normal fp32 number may be flushed to zero: FLUSH = 2^-126, absolute.

      form(g)    = 2^-23 * sum_d p_d (1 + |tanh_d| r_d)                                              + FLUSH
      form(dt_d) = 2^-23 * |dg| p_d ((1 - tanh_d^2) (r_d + 3) + 2 |tanh_d|)                          + FLUSH (1 + |dg|)
      form(ds_d) = 2^-23 * |dg| p_d (|tanh_d - g| (r_d + 3) + 2 + sum_k p_k |tanh_k| r_k)            + FLUSH (1 + |dg|)

    (1 - tanh^2 carries twice the absolute error of tanh times |tanh|; tanh_d - g carries that of tanh_d, of the p-weighted
    tanh_k inside g, and the relative errors of the p_k inside g), and the bound is

      bound = K * form + 2^-9 * |value|      (the last term for bf16 results only: ONE rounding of the result).

K is not derivable from the code alone: it is measured as the worst |err| / form of the kernels on an MI355X over all cases of
tests/test_conv_misc_float64_gpu.py (for bf16 results: the worst (|err| - half a bf16 step at the result) / form, what the rounding
cannot explain; it comes from the elements near zero, where the rounding term is far below 2^-23), and the helper allows
twice the measurement, because different but equally sound intrinsic sequences differ by a few ulp.  GATE_MIX_K holds
(measured, allowed) per dtype; DESIGN.md section 26 repeats them.
"""
import torch
import torch.nn.functional as F

import lm_linear_helpers as L
from conv_ref_helpers import BF16_STEP, F32_STEP, SLACK, check, row_mask, wgrad_bounds, worst  # noqa: F401  (re-exported)

FLUSH = 2.0 ** -126
BF = torch.bfloat16

# (measured worst |err| / form on an MI355X, allowed = 2 x measured), forward and backward together
GATE_MIX_K = {"f32": (1.620, 3.240), "bf16": (1.493, 2.986)}

# ---- the cases of the GPU tests (the CPU emulations run on the same ones) ----
CONV_IN_GEOMS = [(4, 2, 1), (8, 4, 2), (1, 1, 0)]                      # taps, stride, pad
CONV_IN_WIDTHS = [8, 32, 64]
CONV_OUT_WIDTHS = {"f32": [8, 64, 128, 256], "bf16": [8, 128, 512]}
GATE_MIX_GEOMS = [(64, 3), (32, 3), (8, 5), (128, 4), (16, 1), (64, 8), (64, 4)]      # width, depth
GATE_MIX_ROWS = [1, 3, 157, 40000]
GATE_MIX_SCALES = [2.0, 1e-3, 30.0]
RESAMPLE_T = [1, 2, 127, 128, 129, 257]
RESAMPLE_WGRAD_T = [1, 2, 129]


def edge_rows(taps):
    """(b, t) of the conv_in / conv_out edge cases: one partial vector of rows, exactly `taps` rows, one full grid, ragged."""
    return [(1, 2), (1, taps), (3, 1000), (4, 66)]


def edge_lens(b, t, device="cpu"):
    return torch.tensor([t, t - 1, 1, 0][:b], dtype=torch.int32, device=device)


def resample_lens(t_masked, big):
    """Lengths L on the masked side of a resampling case whose masked side has t_masked rows: full, and -- from two tiles on --
    the rows of the two-row halo and of the first DMA piece of the second tile."""
    return [t_masked] + ([v for v in big if v != t_masked] if t_masked >= max(big) else [])


def as_read(t, dtype):
    """The operand as a kernel of element type `dtype` reads it, in float64."""
    return t.to(dtype).double()


def _masked(x, lens):
    xd = x.double()
    return xd if lens is None else xd * row_mask(lens, x.shape[1])


# ---------------------------------------------------------------------------------------------- resampling convs
def strided_conv_ref(x, w, bias, lens_in=None, lens_out=None, rounded=True):
    """(y, bound) float64 [B, T_out, C_out], T_out = (T_in - 2) // 2 + 1.  x [B, T_in, C_in], w [C_out, C_in, 4] (torch Conv1d
    layout), bias [C_out] or None; `rounded`: the result is stored as bf16."""
    b, t_in, c_in = x.shape
    t_out = (t_in - 2) // 2 + 1
    xp = F.pad(_masked(x, lens_in), (0, 0, 1, 2))                        # row l of xp = input row l - 1
    wd = w.double()
    y = torch.zeros(b, t_out, w.shape[0], dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(y)
    for j in range(4):
        rows = xp[:, j:j + 2 * t_out:2][:, :t_out]                       # input rows 2 t + j - 1
        y += rows @ wd[:, :, j].T
        mag += rows.abs() @ wd[:, :, j].abs().T
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    return _resample_out(y, mag, 4 * c_in, lens_out, rounded)


def transposed_conv_ref(x, w, bias, lens_in=None, lens_out=None, rounded=True):
    """(y, bound) float64 [B, 2 T_in, C_out].  x [B, T_in, C_in], w [C_in, C_out, 4] (torch ConvTranspose1d layout)."""
    b, t_in, c_in = x.shape
    xp = F.pad(_masked(x, lens_in), (0, 0, 1, 1))                        # row l of xp = input row l - 1
    wd = w.double()
    cur, prv, nxt = xp[:, 1:t_in + 1], xp[:, 0:t_in], xp[:, 2:t_in + 2]
    y = torch.zeros(b, 2 * t_in, w.shape[1], dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(y)
    y[:, 0::2] = cur @ wd[:, :, 1] + prv @ wd[:, :, 3]
    y[:, 1::2] = cur @ wd[:, :, 2] + nxt @ wd[:, :, 0]
    mag[:, 0::2] = cur.abs() @ wd[:, :, 1].abs() + prv.abs() @ wd[:, :, 3].abs()
    mag[:, 1::2] = cur.abs() @ wd[:, :, 2].abs() + nxt.abs() @ wd[:, :, 0].abs()
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    return _resample_out(y, mag, 2 * c_in, lens_out, rounded)


def _resample_out(y, mag, n, lens_out, rounded):
    bound = n * F32_STEP * mag + (BF16_STEP * y.abs() if rounded else 0.0)
    if lens_out is not None:
        m = row_mask(lens_out, y.shape[1]).double()
        y, bound = y * m, bound * m
    return y, bound


def strided_wgrad_ref(x, dy, lens_in=None):
    """(dW [C_out, C_in, 4], dW bound, db [C_out], db bound) of the strided conv, float64; the bounds are the project's for the
    fp32 sums over rows = B * T_out rows."""
    b, t_out, _ = dy.shape
    xp = F.pad(_masked(x, lens_in), (0, 0, 1, 2))
    dyd = dy.double()
    dw = torch.stack([torch.einsum("bto,bti->oi", dyd, xp[:, j:j + 2 * t_out:2][:, :t_out]) for j in range(4)], dim=2)
    db = dyd.sum((0, 1))
    dw_b, db_b = wgrad_bounds(dw, db, b * t_out)
    return dw, dw_b, db, db_b


def transposed_wgrad_ref(x, dy, lens_in=None):
    """(dW [C_in, C_out, 4], dW bound, db [C_out], db bound) of the transposed conv.  Every tap of dW is a sum over the
    rows = B * T_in rows of one phase; db sums both phases, 2 B T_in rows."""
    b, t_in, _ = x.shape
    xp = F.pad(_masked(x, lens_in), (0, 0, 1, 1))
    cur, prv, nxt = xp[:, 1:t_in + 1], xp[:, 0:t_in], xp[:, 2:t_in + 2]
    dyd = dy.double()
    ev, od = dyd[:, 0::2], dyd[:, 1::2]
    taps = [("bti,bto->io", nxt, od), ("bti,bto->io", cur, ev), ("bti,bto->io", cur, od), ("bti,bto->io", prv, ev)]
    dw = torch.stack([torch.einsum(e, a, c) for e, a, c in taps], dim=2)
    db = dyd.sum((0, 1))
    return dw, wgrad_bounds(dw, db, b * t_in)[0], db, wgrad_bounds(dw, db, 2 * b * t_in)[1]


# ---------------------------------------------------------------------------------------------- conv_in
def conv_in_t_out(t_in, taps, stride, pad):
    return max(0, (t_in + 2 * pad - taps) // stride + 1)


def _conv_in_rows(x, lens, taps, stride, pad, t_out):
    """[taps][B, T_out] float64: input sample t * stride + j - pad of every output row, 0 outside [0, min(lens[b], T_in))."""
    b, t_in = x.shape
    xd = x.double()
    if lens is not None:
        xd = xd * row_mask(lens, t_in)[:, :, 0]
    xp = F.pad(xd, (pad, pad + taps + stride))
    return [xp[:, j:j + stride * t_out:stride][:, :t_out] for j in range(taps)]


def conv_in_ref(x, w, bias, lens, stride, pad, rounded):
    """(y, bound) float64 [B, T_out, C].  x fp32 [B, T_in], w fp32 [C, 1, taps], bias fp32 [C]; `rounded`: y is bf16."""
    c, _, taps = w.shape
    t_out = conv_in_t_out(x.shape[1], taps, stride, pad)
    wd = w.double()[:, 0]
    y = bias.double().expand(x.shape[0], t_out, c).clone()
    mag = y.abs()
    for j, xs in enumerate(_conv_in_rows(x, lens, taps, stride, pad, t_out)):
        y += xs[:, :, None] * wd[:, j]
        mag += xs.abs()[:, :, None] * wd[:, j].abs()
    return y, (taps + 1) * F32_STEP * mag + (BF16_STEP * y.abs() if rounded else 0.0)


def conv_in_wgrad_ref(x, dy, lens, taps, stride, pad):
    """(dW [C, 1, taps], bound, db [C], bound) float64.  dy [B, T_out, C] holds the values the kernel reads."""
    b, t_out, c = dy.shape
    dyd = dy.double()
    rows = b * t_out
    xs = _conv_in_rows(x, lens, taps, stride, pad, t_out)
    dw = torch.stack([torch.einsum("bto,bt->o", dyd, r) for r in xs], dim=1)[:, None, :]
    mag = torch.stack([torch.einsum("bto,bt->o", dyd.abs(), r.abs()) for r in xs], dim=1)[:, None, :]
    return dw, L.bound(rows, mag), dyd.sum((0, 1)), L.bound(rows, dyd.abs().sum((0, 1)))


# ---------------------------------------------------------------------------------------------- conv_out
def conv_out_ref(x, w, bias, lens):
    """(y, bound) float64 [B, T].  x [B, T, C] as read, w fp32 [1, C, 1], bias fp32 [1]; padded rows give the bias alone."""
    xm, wd = _masked(x, lens), w.double().reshape(-1)
    y = xm @ wd + bias.double()
    mag = xm.abs() @ wd.abs() + bias.double().abs()
    return y, (x.shape[2] + 1) * F32_STEP * mag


def conv_out_bwd_ref(x, w, dy, lens, rounded):
    """(dx, bound, dw [1, C, 1], bound, db [1], bound) float64; dy fp32 [B, T].  dx is 0 on padded rows, which still count in
    db; `rounded`: dx is bf16."""
    b, t, c = x.shape
    dyd, wd = dy.double(), w.double().reshape(-1)
    m = torch.ones(b, t, 1, dtype=torch.float64, device=x.device) if lens is None else row_mask(lens, t).double()
    dx = dyd[:, :, None] * wd * m
    dw = torch.einsum("bt,btc->c", dyd, x.double() * m)
    mag = torch.einsum("bt,btc->c", dyd.abs(), x.double().abs() * m)
    rows = b * t
    return (dx, (F32_STEP + (BF16_STEP if rounded else 0.0)) * dx.abs(), dw.reshape(1, c, 1), L.bound(rows, mag).reshape(1, c, 1),
            dyd.sum().reshape(1), L.bound(rows, dyd.abs().sum()).reshape(1))


# ---------------------------------------------------------------------------------------------- gate_mix
def gate_mix_ref(z, depth, dg=None):
    """Float64 gate_mix on z [rows, depth * 2 * w] (as read; branch d has t at [d 2w, d 2w + w), s at [d 2w + w, (d + 1) 2w)).
    Returns dict(g, g_form) and, with dg [rows, w] (as read), dz, dz_form in z's layout.  A bound is gate_mix_bound(...)."""
    rows = z.shape[0]
    w = z.shape[1] // (2 * depth)
    zz = z.double().reshape(rows, depth, 2, w)
    th, s = torch.tanh(zz[:, :, 0]), zz[:, :, 1]
    m = s.max(dim=1, keepdim=True).values
    ex = torch.exp(s - m)
    p = ex / ex.sum(1, keepdim=True)
    g = (th * p).sum(1)
    dist = (s - m).abs()
    r = depth + 2 + dist + (p * dist).sum(1, keepdim=True)
    out = {"g": g, "g_form": F32_STEP * (p * (1 + th.abs() * r)).sum(1) + FLUSH}
    if dg is not None:
        go = dg.double()[:, None, :]
        dt = go * p * (1 - th * th)
        ds = go * p * (th - g[:, None])
        f_dt = F32_STEP * go.abs() * p * ((1 - th * th) * (r + 3) + 2 * th.abs())
        f_ds = F32_STEP * go.abs() * p * ((th - g[:, None]).abs() * (r + 3) + 2 + (p * th.abs() * r).sum(1, keepdim=True))
        out["dz"] = torch.stack([dt, ds], dim=2).reshape(rows, -1)
        out["dz_form"] = (torch.stack([f_dt, f_ds], dim=2) + FLUSH * (1 + go.abs())[:, :, None]).reshape(rows, -1)
    return out


def gate_mix_bound(value, form, dtype):
    """K * form (+ one rounding to bf16) with the allowed constant of the dtype."""
    bf = dtype == BF
    return GATE_MIX_K["bf16" if bf else "f32"][1] * form + (BF16_STEP * value.abs() if bf else 0.0)


def gate_mix_measure(got, value, form, dtype):
    """The figure GATE_MIX_K is measured by: worst |err| / form, for bf16 results after taking off what the one rounding can
    explain -- half a bf16 step at the result (2^-8 of the power of two below it: 2^-9 of the value at the top of a binade, 2^-8
    at the bottom, which is what SLACK times the bound's rounding term allows)."""
    err = (got.double() - value).abs()
    if dtype == BF:
        top = torch.maximum(got.double().abs(), value.abs()).clamp_min(FLUSH)
        err = (err - torch.exp2(torch.floor(torch.log2(top)) - 8)).clamp_min(0)
    return float((err / form).max()) if err.numel() else 0.0


# ---------------------------------------------------------------------------------------------- kernel emulations
# fp32 torch ops on the rounded operands, then the stated roundings: what the CPU test holds against the bounds, and what its
# mutations damage.  `drop` names one mutation (None = the kernel as it is).
def store(v32, dtype, truncate=False):
    """The kernel's store of an fp32 value: round to nearest even for bf16 (or, as a mutation, truncate)."""
    if dtype != BF:
        return v32
    if truncate:
        return (v32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)
    return v32.to(BF)


def emulate_strided(x, w, bias, lens_in, lens_out, dtype, drop=None):
    """x, w in `dtype`; returns [B, T_out, C_out] in `dtype`.  drop in {None, 'tap', 'lens', 'vector', 'bias', 'truncate'}."""
    b, t_in, c_in = x.shape
    t_out = (t_in - 2) // 2 + 1
    off = 1 if drop == "lens" else 0
    xm = x.float() if lens_in is None else x.float() * row_mask(lens_in - off, t_in)
    if drop == "vector":
        xm = xm.clone()
        xm[:, :, 8:16] = 0
    xp = F.pad(xm, (0, 0, 1, 2))
    acc = torch.zeros(b, t_out, w.shape[0])
    for j in range(4):
        if not (drop == "tap" and j == 3):
            acc = acc + xp[:, j:j + 2 * t_out:2][:, :t_out] @ w.float()[:, :, j].T
    if bias is not None and drop != "bias":
        acc = acc + bias
    if lens_out is not None:
        acc = acc * row_mask(lens_out - off, t_out)
    return store(acc, dtype, drop == "truncate")


def emulate_transposed(x, w, bias, lens_in, lens_out, dtype, drop=None):
    """drop in {None, 'tap', 'phases', 'lens', 'vector', 'bias', 'truncate'}."""
    b, t_in, c_in = x.shape
    off = 1 if drop == "lens" else 0
    xm = x.float() if lens_in is None else x.float() * row_mask(lens_in - off, t_in)
    if drop == "vector":
        xm = xm.clone()
        xm[:, :, 8:16] = 0
    xp = F.pad(xm, (0, 0, 1, 1))
    cur, prv, nxt = xp[:, 1:t_in + 1], xp[:, 0:t_in], xp[:, 2:t_in + 2]
    wf = w.float()
    ev = prv @ wf[:, :, 3] + cur @ wf[:, :, 1]                           # increasing input offset, as the kernel accumulates
    od = cur @ wf[:, :, 2] + (0 if drop == "tap" else nxt @ wf[:, :, 0])
    if drop == "phases":
        ev, od = od, ev
    acc = torch.stack([ev, od], dim=2).reshape(b, 2 * t_in, -1)
    if bias is not None and drop != "bias":
        acc = acc + bias
    if lens_out is not None:
        acc = acc * row_mask(lens_out - off, 2 * t_in)
    return store(acc, dtype, drop == "truncate")


def emulate_conv_in(x, w, bias, lens, stride, pad, dtype, drop=None):
    """drop in {None, 'tap', 'lens', 'bias', 'truncate'}."""
    c, _, taps = w.shape
    t_out = conv_in_t_out(x.shape[1], taps, stride, pad)
    lens = lens - 1 if (drop == "lens" and lens is not None) else lens
    acc = (torch.zeros(c) if drop == "bias" else bias).expand(x.shape[0], t_out, c).clone()
    for j, xs in enumerate(_conv_in_rows(x, lens, taps, stride, pad, t_out)):
        if not (drop == "tap" and j == taps - 1):
            acc = acc + xs.float()[:, :, None] * w[:, 0, j]
    return store(acc, dtype, drop == "truncate")


def emulate_conv_out(x, w, bias, lens, drop=None):
    """x in its dtype; fp32 [B, T].  drop in {None, 'lens', 'vector', 'bias'}."""
    lens = lens - 1 if (drop == "lens" and lens is not None) else lens
    xm = x.float() if lens is None else x.float() * row_mask(lens, x.shape[1])
    wf = w.reshape(-1).clone()
    if drop == "vector":
        wf[-8:] = 0
    return xm @ wf + (0 if drop == "bias" else bias)


def emulate_conv_out_dx(x, w, dy, lens, drop=None):
    """dx in x's dtype.  drop in {None, 'lens', 'vector', 'truncate'}."""
    lens = lens - 1 if (drop == "lens" and lens is not None) else lens
    m = 1.0 if lens is None else row_mask(lens, x.shape[1]).float()
    dx = dy[:, :, None] * w.reshape(-1) * m
    if drop == "vector":
        dx = dx.clone()
        dx[:, :, -8:] = 0
    return store(dx, x.dtype, drop == "truncate")


def emulate_gate_mix(z, depth, dg=None, drop=None):
    """The kernels' sequence in fp32 (exp2 of 2 x log2 e, 1 - 2 / (e + 1); exp of s - max; one reciprocal), results in z's dtype.
    Returns (g, dz or None).  drop in {None, 'branches', 'truncate'}: 'branches' pairs every gate with the next branch's weight."""
    rows = z.shape[0]
    w = z.shape[1] // (2 * depth)
    zz = z.float().reshape(rows, depth, 2, w)
    e = torch.exp2(zz[:, :, 0] * 2.885390081777927)
    th = 1.0 - 2.0 * (1.0 / (e + 1.0))
    s = zz[:, :, 1]
    if drop == "branches":
        s = s.roll(1, dims=1)
    ex = torch.exp(s - s.max(dim=1, keepdim=True).values)
    inv = 1.0 / ex.sum(1, keepdim=True)
    g32 = (ex * th).sum(1, keepdim=True) * inv
    g = store(g32[:, 0], z.dtype, drop == "truncate")
    if dg is None:
        return g, None
    gs = dg.float()[:, None, :] * ex * inv
    dt, ds = gs * (1.0 - th * th), gs * (th - g32)
    return g, store(torch.stack([dt, ds], dim=2).reshape(rows, -1), z.dtype, drop == "truncate")
