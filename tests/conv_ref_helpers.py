"""Shared by the float64 tests of the conv kernels (csrc/conv.hip, csrc/conv_wgrad.hip behind smt_amd.convops): a plain
float64 evaluation of what ONE conv descriptor computes from the bf16 operands the kernel is handed, and the per-element
error bound of the kernel's bf16 / fp32 arithmetic against it.  tests/test_conv_ref_cpu.py pins all of it to
torch.nn.functional.conv1d in float64.

What a descriptor computes (stride 1, channels last; read from the epilogue of conv_gemm_kernel / conv_gemm_dma_kernel):

    a[b, t, co] = bias[co] + sum_s sum_ci x[b, t + s * dil - pad, ci] * w[co, ci, s]      rows of x outside [0, lens_in[b]) are 0
    c           = a                                   staged through LDS as bf16                            (rounding 1)
    o           = u_src != 0 ? c * scale : 0          activation derivative, if the descriptor has one      (exact mask)
    o           = o * [t < lens_out[b]]               row mask: AFTER the derivative, BEFORE the residual
    o           = o + res                             residual, if any
    y           = o                                   stored as bf16                                        (rounding 2)
    u           = keep ? relu(o) * drop_scale : 0     second output, from the fp32 o, stored as bf16        (rounding 2')

    dW[co, ci, s] = sum_{b, t} dy[b, t, co] * x[b, t + s * dil - pad, ci]      db[co] = sum_{b, t} dy[b, t, co]

The bound, derived, not tuned.  With mag = |bias| + (|x| conv |w|), evaluated in float64 next to a, and n = c_in * taps:

  * the fp32 accumulation (MFMA chains and the bias add) is off by at most n * 2^-23 * mag;
  * every rounding to bf16 costs 2^-9 of the magnitude at that point: the staged c costs 2^-9 |a|, so
        e_c = n * 2^-23 * mag + 2^-9 * |a|;
  * the derivative scales it (e_o = scale * e_c where u_src != 0, else 0: the mask is read, not computed), the row mask
    zeroes it, the residual is an exact bf16 operand and adds nothing;
  * the store of y is one more rounding:    e_y = e_o + 2^-9 * |y|;
  * relu is 1-Lipschitz, so a sign of o that differs from the reference's moves u by no more than the error of o; the
    dropout mask is reproduced bit for bit and the store rounds once:    e_u = keep * drop_scale * e_o + 2^-9 * |u|.

Where a bound is 0 (masked rows without a residual, dropped elements, derivative off) the kernel must give exactly 0.
The tests allow SLACK = 2 times the bound: 2^-9 is the rounding step of bf16 at the top of a binade and half of it at the
bottom (so the doubled rounding terms are the worst case of round-to-nearest, 2^-8 each); the products of two error terms,
about 2^-16 |a|, and the fp32 multiplications by scale / drop_scale (2^-24 each) fit in the doubled accumulation term,
n * 2^-22 * mag >= n * 2^-22 * |a|, from n = 128 on (round-to-nearest fp32 sums of n terms are themselves within
n * 2^-24 * mag).  Measured on the 256-channel kernels: 1.1 to 1.9 times the bound.  A dropped tap, row or channel chunk
moves an element by about |a| itself, hundreds of times the bound.

Weight and bias gradients are fp32 sums over the rows = B * T rows of the launch; they keep the project's bound for those
(tests/test_conv_gpu.py): 2e-6 * max|ref| * sqrt(rows) + 1e-4 for dW and + 1e-3 for db.
"""
import functools

import torch
import torch.nn.functional as F

from oracle import vqvae_oracle as orc

BF16_STEP = 2.0 ** -9
F32_STEP = 2.0 ** -23
SLACK = 2.0


def row_mask(lens, t):
    """[B, T, 1] bool: row t of item b is inside lens[b]."""
    return (torch.arange(t, device=lens.device)[None, :] < lens[:, None])[:, :, None]


def _masked_padded(x, lens_in, pad):
    xd = x.double()
    if lens_in is not None:
        xd = xd * row_mask(lens_in, x.shape[1])
    return F.pad(xd, (0, 0, pad, pad))


def conv_ref(x, w, bias, dil, pad, lens_in=None):
    """(a, mag) in float64, [B, T_out, C_out] each.  x [B, T, C_in] and w [C_out, C_in, k] hold the values the kernel reads
    (bf16-representable); bias [C_out] fp32 or None."""
    c_out, _, k = w.shape
    t_out = x.shape[1] + 2 * pad - dil * (k - 1)
    xp = _masked_padded(x, lens_in, pad)
    wd = w.double()
    a = torch.zeros(x.shape[0], t_out, c_out, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(a)
    for s in range(k):
        rows = xp[:, s * dil:s * dil + t_out]
        a += rows @ wd[:, :, s].T
        mag += rows.abs() @ wd[:, :, s].abs().T
    if bias is not None:
        a += bias.double()
        mag += bias.double().abs()
    return a, mag


def epilogue_ref(a, mag, n, *, act_grad_src=None, scale=1.0, lens_out=None, res=None, keep=None, drop_scale=1.0):
    """The epilogue in the kernel's order on (a, mag) of conv_ref; n = c_in * taps.  keep: the dropout keep mask of the
    second output (bool [B, T_out, C_out]) or None when the descriptor has no second output.
    Returns dict(y, y_bound[, u, u_bound]), float64."""
    e_c = n * F32_STEP * mag + BF16_STEP * a.abs()
    o, e_o = a, e_c
    if act_grad_src is not None:
        on = (act_grad_src != 0).double()
        o, e_o = o * scale * on, e_o * scale * on
    if lens_out is not None:
        m = row_mask(lens_out, a.shape[1]).double()
        o, e_o = o * m, e_o * m
    if res is not None:
        o = o + res.double()
    out = {"y": o, "y_bound": e_o + BF16_STEP * o.abs()}
    if keep is not None:
        kd = keep.double() * drop_scale
        u = torch.relu(o) * kd
        out["u"], out["u_bound"] = u, e_o * kd + BF16_STEP * u
    return out


def wgrad_ref(x, dy, k, dil, pad, lens_in=None):
    """(dW [C_out, C_in, k], db [C_out]) in float64: the einsum of the weight-gradient tests."""
    t_out = dy.shape[1]
    xp = _masked_padded(x, lens_in, pad)
    dyd = dy.double()
    dw = torch.stack([torch.einsum("bto,bti->oi", dyd, xp[:, s * dil:s * dil + t_out]) for s in range(k)], dim=2)
    return dw, dyd.sum((0, 1))


def wgrad_bounds(dw_ref, db_ref, rows):
    """The fp32-accumulation bounds of the weight-gradient tests for (dW, db) summed over `rows` rows."""
    return (2e-6 * float(dw_ref.abs().max()) * rows ** 0.5 + 1e-4, 2e-6 * float(db_ref.abs().max()) * rows ** 0.5 + 1e-3)


@functools.lru_cache(maxsize=4)
def _keep_np(seed, site, b, t, c, p):
    return orc.dropout_keep_ntc(seed, site, b, t, c, p)


def keep_mask(seed, site, b, t, c, p, device):
    """The counter-based dropout keep mask of one site whose rows are c channels wide (computed once per shape)."""
    return torch.from_numpy(_keep_np(seed, site, b, t, c, p)).to(device)


def worst(got, ref, bound):
    """max over elements of |got - ref| / bound, with 0 / 0 = 0 and x / 0 = inf: <= SLACK passes."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


def check(name, got, ref, bound):
    """Print the figure, then assert it."""
    w = worst(got, ref, bound)
    print(f"  {name}: worst |err| / bound = {w:.3f} (allowed {SLACK})")
    assert w <= SLACK, f"{name}: |err| / bound = {w:.3f} > {SLACK}"
