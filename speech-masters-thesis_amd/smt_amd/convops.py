"""Channels-last ("NTC", [B, T, C]) building blocks of the encoder / decoder stacks, on the HIP
library (include/smt_hip.h, "conv stack").  This is the single seam between the model code
(models/vqvae/*) and the arithmetic: every function here is a torch.autograd.Function whose forward
and backward are libsmt_hip.so launches on torch's current stream.

    conv1d            implicit-GEMM MFMA conv (any k / dilation / stride), fused input row-mask,
                      ReLU+dropout prologue, bias, residual
    conv_transpose1d  the same kernel, one launch per output phase
    conv_in / conv_out  the C_in = 1 and C_out = 1 ends of the network (HBM-bound kernels)
    gate_mix          sum_d tanh(t_d) * softmax_d(s_d)
    wavenet_gate      tanh(t) * sigmoid(s), the WaveNet gate
    wavenet_tail      x + bias + W_g . wavenet_gate(z): one WaveNet layer's gate, 1x1 and residual (fused in bf16)

Data gradients are the same GEMM kernel on repacked weights; weight / bias gradients use the
transposed-fragment kernel (conv_wgrad.hip) with a fixed-order reduction.  The operand-layout copies of the
weights are described here ("operand layouts") and owned by smt_amd.packing.
"""
import contextlib
import ctypes
import os
from dataclasses import dataclass

import torch

from . import native as N
from . import packing
from . import profiler
from .packing import Part

SMT_F32, SMT_BF16 = 0, 1
_DT = {torch.float32: SMT_F32, torch.bfloat16: SMT_BF16}


class ConvDesc(ctypes.Structure):
    """Mirror of ``smt_conv_desc`` (include/smt_hip.h)."""
    _fields_ = [("dtype", ctypes.c_int), ("batch", ctypes.c_int), ("t_in", ctypes.c_int), ("t_out", ctypes.c_int),
                ("t_y", ctypes.c_int), ("c_in", ctypes.c_int), ("c_out", ctypes.c_int), ("taps", ctypes.c_int),
                ("stride", ctypes.c_int), ("dilation", ctypes.c_int), ("padding", ctypes.c_int),
                ("out_stride", ctypes.c_int), ("out_offset", ctypes.c_int), ("act_out", ctypes.c_int),
                ("act_grad", ctypes.c_int), ("site_width", ctypes.c_int), ("ld_x", ctypes.c_int),
                ("ld_y", ctypes.c_int), ("ld_res", ctypes.c_int), ("ld_act", ctypes.c_int), ("ld_yact", ctypes.c_int),
                ("drop_keys", ctypes.c_uint32 * 8), ("drop_thresh16", ctypes.c_uint32), ("drop_scale", ctypes.c_float),
                ("bs_x", ctypes.c_int64), ("bs_y", ctypes.c_int64), ("bs_res", ctypes.c_int64),
                ("bs_act", ctypes.c_int64), ("bs_yact", ctypes.c_int64), ("x", ctypes.c_void_p), ("w", ctypes.c_void_p),
                ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p), ("y_act", ctypes.c_void_p), ("res", ctypes.c_void_p),
                ("act_grad_src", ctypes.c_void_p), ("lens_in", ctypes.c_void_p), ("lens_out", ctypes.c_void_p),
                ("w_swizzled", ctypes.c_int), ("zero_page", ctypes.c_void_p),
                ("x2", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("bias2", ctypes.c_void_p),
                ("lens_in2", ctypes.c_void_p), ("c_in2", ctypes.c_int), ("ld_x2", ctypes.c_int),
                ("bs_x2", ctypes.c_int64), ("drop_keys_dev", ctypes.c_void_p), ("drop_keys_dev_stride", ctypes.c_int)]


@dataclass
class DropSpec:
    """relu(dropout(.)) of a conv OUTPUT (reference models/vqvae/resnet.py:22-26), produced in the
    conv's epilogue with the counter-based generator of include/smt_hip.h ("dropout")."""
    p: float
    training: bool
    seed: int = 0
    site: int = 0

    def params(self):
        """(key, thresh16, scale): eval mode / p == 0 degenerates to a plain ReLU."""
        if not self.training or self.p <= 0.0:
            return 0, 0, 1.0
        return dropout_key(self.seed, self.site), int(round(self.p * 65536.0)), 1.0 / (1.0 - self.p)


def _fmix32(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def dropout_key(seed, site):
    return _fmix32(seed * 0x9E3779B1 + site * 0x7F4A7C15 + 1)


def _geom(t):
    """(data_ptr, batch stride, row pitch) of a [B, T, C] tensor whose channel axis is dense."""
    assert t.dim() == 3 and t.stride(2) == 1 and t.is_cuda, "need [B, T, C] with unit channel stride on the GPU"
    return ctypes.c_void_p(t.data_ptr()), t.stride(0), t.stride(1)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _i32(lens):
    if lens is None:
        return None
    return lens if lens.dtype == torch.int32 else lens.to(torch.int32)


_zero_pages = {}


def _zero_page(device):
    key = (device.type, device.index)
    if key not in _zero_pages:
        _zero_pages[key] = torch.zeros(4096, dtype=torch.uint8, device=device)
    return _zero_pages[key]


def _dma_ok(dtype, c_in, c_out):
    """LDS-DMA kernel: bf16, both channel counts multiples of 128, stride 1 (include/smt_hip.h)."""
    return dtype == torch.bfloat16 and c_in % 128 == 0 and c_out % 128 == 0


def _phases(kernel, stride, padding):
    """Output-phase decomposition of a transposed convolution: for output index s*m + ph the
    contributing taps j satisfy (ph + padding - j) % s == 0 and read input row m + (ph+padding-j)/s.
    Returns per phase (tap list ordered by increasing input offset, effective left padding)."""
    out = []
    for ph in range(stride):
        taps = [(j, (ph + padding - j) // stride) for j in range(kernel) if (ph + padding - j) % stride == 0]
        taps.sort(key=lambda jt: jt[1])
        offs = [o for _, o in taps]
        assert offs == list(range(offs[0], offs[0] + len(offs))), "phase taps must touch consecutive rows"
        out.append(([j for j, _ in taps], -offs[0]))
    return out


_K3GATE = not bool(int(os.environ.get("SMT_NO_K3GATE", "0")))       # A/B switches for tests and profiles
_RESAMPLE = not bool(int(os.environ.get("SMT_NO_RESAMPLE", "0")))
_WN_TAIL = not bool(int(os.environ.get("SMT_NO_WN_TAIL", "0")))     # the fused WaveNet layer tail (smt_wavenet_tail_fwd)
_WN_TAIL_WIDTHS = (64, 128)     # widths at which the fused tail is the default: where it measured faster


# ---- operand layouts: which element of a torch-layout weight goes where (packed and kept current by smt_amd.packing) ----
def _pack(weight, dtype, n_out, n_in, s_out, s_in, s_tap, tap_map, swizzle=False):
    """Operand [len(tap_map)][n_out][n_in] with element (tap, o, i) = weight[o*s_out + i*s_in + tap_map[tap]*s_tap]."""
    return packing.pack([Part.dense(weight, n_out, n_in, s_out, s_in, s_tap, tap_map, swizzle)], dtype,
                        (len(tap_map), n_out, n_in))


def _pack_fwd(weight, dtype, swizzle=False):
    c_out, c_in, k = weight.shape
    return _pack(weight, dtype, c_out, c_in, c_in * k, k, 1, range(k), swizzle)


def _pack_bwd(weight, dtype, swizzle=False):
    """[tap][ci][co] with flipped taps: the data gradient of a stride-1 conv is a conv with these."""
    c_out, c_in, k = weight.shape
    return _pack(weight, dtype, c_in, c_out, k, c_in * k, 1, range(k - 1, -1, -1), swizzle)


def _pack_cat_fwd(weights, dtype, swizzle=False):
    """1x1 weights [O_d, I, 1] of several layers stacked along the output axis: operand [1][sum O_d][I]; with ``swizzle``
    the LDS-DMA chunk swizzle inside every [O_d][I] part (I a multiple of 128)."""
    n_in = weights[0].shape[1]
    total = sum(w.shape[0] for w in weights)
    parts, row0 = [], 0
    for w in weights:
        parts.append(Part(w, w.shape[0], n_in, n_in, 1, 1, (0,), bool(swizzle), row0 * n_in, total * n_in, n_in))
        row0 += w.shape[0]
    return packing.pack(parts, dtype, (1, total, n_in))


def _pack_cat_bwd(weights, dtype):
    """Data-gradient operand [1][I][sum O_d] of the same stack (rows = input channels, columns = output channels)."""
    n_in = weights[0].shape[1]
    total = sum(w.shape[0] for w in weights)
    parts, col0 = [], 0
    for w in weights:
        parts.append(Part(w, n_in, w.shape[0], 1, n_in, 1, (0,), False, col0, n_in * total, total))
        col0 += w.shape[0]
    return packing.pack(parts, dtype, (1, n_in, total))


def _cat_bias(biases):
    """fp32 biases of several layers side by side, kept current by the pack cache (no torch.cat per step)."""
    total = sum(b.shape[0] for b in biases)
    parts, row0 = [], 0
    for b in biases:
        parts.append(Part(b, b.shape[0], 1, 1, 1, 1, (0,), False, row0, total, 1))
        row0 += b.shape[0]
    return packing.pack(parts, torch.float32, (1, total, 1))


# ---- launch wrappers ----
@contextlib.contextmanager
def reduce_batch(device):
    """The weight-gradient calls inside the block queue their slab reductions; ONE launch (per 16 jobs) reduces them all when
    the block ends (smt_wgrad_reduce_defer).  A GatedHiFi block's backward has ten of them: 172 -> ~30 reduce launches per
    train step.  Every call gets a workspace region of its own from ``native.workspace.arena``."""
    lib = N.lib()
    with N.workspace.arena(device):
        N.check(lib.smt_wgrad_reduce_defer(1, N.stream_ptr()), "smt_wgrad_reduce_defer")
        try:
            yield
        finally:
            with profiler.region("conv_wgrad_reduce", bound="hbm"):
                N.check(lib.smt_wgrad_reduce_defer(0, N.stream_ptr()), "smt_wgrad_reduce_defer")


def _use_dma(d, w_packed):
    d.w = _p(w_packed)
    d.w_swizzled = 1
    d.zero_page = _p(_zero_page(w_packed.device))


def _tag(desc):
    return f"k{desc.taps}d{desc.dilation}s{desc.stride}o{desc.out_stride}_c{desc.c_in}x{desc.c_out}"


def _kernel_of(desc):
    """Which kernel smt_conv1d_ntc dispatches to (asked of the library: one dispatch rule, csrc/conv.hip and csrc/conv_ws.hip)."""
    return N.lib().smt_conv1d_kernel_name(ctypes.byref(desc)).decode()


def _dma_plan_of(desc):
    """(tile rows, row classes) of the conv_gemm_dma launch of this descriptor, (0, 0) for any other kernel."""
    rows, classes = ctypes.c_int(0), ctypes.c_int(0)
    N.check(N.lib().smt_conv1d_dma_plan(ctypes.byref(desc), ctypes.byref(rows), ctypes.byref(classes)), "smt_conv1d_dma_plan")
    return rows.value, classes.value


def _launch(desc, name, flops=0.0, nbytes=0.0):
    dtype = "bf16" if desc.dtype == SMT_BF16 else "f32"
    name = _kernel_of(desc) + ":" + name.replace("conv_", "")      # e.g. conv_gemm_dma:fwd
    if profiler.DETAIL:
        name = name + "_" + _tag(desc)
    with profiler.region(name, nbytes=nbytes, flops=flops, bound="mfma", dtype=dtype):
        N.check(N.lib().smt_conv1d_ntc(ctypes.byref(desc), N.stream_ptr()), "smt_conv1d_ntc")


def _conv_flops(d):
    return 2.0 * d.batch * d.t_out * d.c_out * d.c_in * d.taps


def _conv_bytes(d, esz):
    """Algorithmic HBM bytes of one launch: every operand row once (x, y and/or y_act, residual, activation source,
    folded x2) plus the weights."""
    outs = (1 if d.y else 0) + (1 if d.act_out else 0) + (1 if d.res else 0) + (1 if d.act_grad else 0)
    rows_in = float(d.batch) * d.t_in * (d.c_in + (d.c_in2 if d.x2 else 0))
    return (rows_in + float(d.batch) * d.t_out * d.c_out * outs) * esz + d.taps * d.c_in * d.c_out * esz


def _base_desc(x, y, lens_in, c_in, c_out, taps, stride, dil, pad, t_out, out_stride=1, out_offset=0, t_y=None):
    d = ConvDesc()
    d.dtype = _DT[x.dtype]
    d.batch, d.t_in, d.t_out, d.t_y = x.shape[0], x.shape[1], t_out, (y.shape[1] if t_y is None else t_y)
    d.c_in, d.c_out = c_in, c_out
    d.taps, d.stride, d.dilation, d.padding = taps, stride, dil, pad
    d.out_stride, d.out_offset = out_stride, out_offset
    d.x, d.bs_x, d.ld_x = _geom(x)
    if y is not None:
        d.y, d.bs_y, d.ld_y = _geom(y)
    d.lens_in = _p(lens_in)
    d.drop_scale = 1.0
    return d


def _wgrad(desc, dweight, s_out, s_in, s_tap, tap_map, dbias):
    lib = N.lib()
    desc.zero_page = _p(_zero_page(dweight.device))     # enables the LDS-DMA variant where eligible
    ws_bytes = lib.smt_conv1d_wgrad_workspace_bytes(ctypes.byref(desc))
    ws = N.workspace.get(ws_bytes, dweight.device)
    arr = (ctypes.c_int * len(tap_map))(*tap_map)
    dtype = "bf16" if desc.dtype == SMT_BF16 else "f32"
    name = lib.smt_conv1d_wgrad_kernel_name(ctypes.byref(desc)).decode() + ("_" + _tag(desc) if profiler.DETAIL else "")
    with profiler.region(name, flops=_conv_flops(desc), bound="mfma", dtype=dtype):
        N.check(lib.smt_conv1d_wgrad(ctypes.byref(desc), _p(dweight), s_out, s_in, s_tap, arr, _p(dbias), _p(ws),
                                     ws.numel(), N.stream_ptr()), "smt_conv1d_wgrad")


def _conv1x1_bwd(desc, dweight, s_out, s_in, dbias):
    """Fused data + weight gradient of a 128 -> 128 1x1 conv behind relu+dropout (smt_conv1x1_bwd): `desc` is the
    data-gradient descriptor with act_grad set; one pass over dy and u instead of two."""
    lib = N.lib()
    ws_bytes = lib.smt_conv1x1_bwd_workspace_bytes(ctypes.byref(desc))
    ws = N.workspace.get(ws_bytes, dweight.device)
    rows = float(desc.batch) * desc.t_out
    name = "conv1x1_bwd" + ("_" + _tag(desc) if profiler.DETAIL else "")
    with profiler.region(name, flops=2 * _conv_flops(desc), nbytes=rows * 3 * desc.c_in * 2, bound="hbm", dtype="bf16"):
        N.check(lib.smt_conv1x1_bwd(ctypes.byref(desc), _p(dweight), s_out, s_in, _p(dbias), _p(ws), ws.numel(),
                                    N.stream_ptr()), "smt_conv1x1_bwd")


def _conv_gate_bwd(dy, g, w_packed_bwd, dx, lens32, dweight, dbias):
    """Fused data + weight gradient of the 64 -> 64 gate conv (smt_conv_gate_bwd): one pass over dy."""
    lib = N.lib()
    b, t = g.shape[0], g.shape[1]
    ws = N.workspace.get(lib.smt_conv_gate_bwd_workspace_bytes(b, t), g.device)
    (pdy, bsdy, lddy), (pg, bsg, ldg), (pdx, bsdx, lddx) = _geom(dy), _geom(g), _geom(dx)
    rows = float(b) * t
    with profiler.region("conv_gate_bwd", flops=4.0 * rows * 64 * 64, nbytes=rows * 3 * 64 * 2, bound="hbm", dtype="bf16"):
        N.check(lib.smt_conv_gate_bwd(pdy, bsdy, lddy, pg, bsg, ldg, _p(w_packed_bwd), pdx, bsdx, lddx, _p(lens32), b, t,
                                      _p(_zero_page(g.device)), _p(dweight), dweight.stride(0), dweight.stride(1),
                                      _p(dbias), _p(ws), ws.numel(), N.stream_ptr()), "smt_conv_gate_bwd")


def _conv_k1_bwd(dh, x, w_packed_bwd, res, dx, lens32, dweight, dbias):
    """Fused data + weight gradient of the 64 -> 512 K1 layer (smt_conv_k1_bwd): one pass over dh."""
    lib = N.lib()
    b, t = x.shape[0], x.shape[1]
    ws = N.workspace.get(lib.smt_conv_k1_bwd_workspace_bytes(b, t), x.device)
    (pdh, bsdh, lddh), (px, bsx, ldx_), (pr, bsr, ldr), (pdx, bsdx, lddx) = _geom(dh), _geom(x), _geom(res), _geom(dx)
    rows = float(b) * t
    with profiler.region("conv_k1_bwd", flops=4.0 * rows * 512 * 64, nbytes=rows * (512 + 3 * 64) * 2, bound="hbm",
                         dtype="bf16"):
        N.check(lib.smt_conv_k1_bwd(pdh, bsdh, lddh, px, bsx, ldx_, _p(w_packed_bwd), pr, bsr, ldr, pdx, bsdx, lddx,
                                    _p(lens32), b, t, _p(_zero_page(x.device)), _p(dweight), dweight.stride(0),
                                    dweight.stride(1), _p(dbias), _p(ws), ws.numel(), N.stream_ptr()),
                "smt_conv_k1_bwd")


def _conv_k3gate(u2, x, w3p, w1p, b3, b1, z, g, lens32):
    """K3 of the four branches + the gate in one pass (smt_conv_k3gate_fwd)."""
    b, t = x.shape[0], x.shape[1]
    (pu, bsu, ldu), (px, bsx, ldx_), (pz, bsz, ldz), (pg, bsg, ldg) = _geom(u2), _geom(x), _geom(z), _geom(g)
    rows = float(b) * t
    with profiler.region("conv_k3gate", flops=2.0 * rows * 512 * (128 + 64), nbytes=rows * (1024 + 128) * 2, bound="hbm",
                         dtype="bf16"):
        N.check(N.lib().smt_conv_k3gate_fwd(pu, bsu, ldu, px, bsx, ldx_, _p(w3p), _p(w1p), _p(b3), _p(b1), pz, bsz, ldz, pg,
                                            bsg, ldg, _p(lens32), b, t, _p(_zero_page(x.device)), N.stream_ptr()),
                "smt_conv_k3gate_fwd")


# Per-site dropout keys in device memory (int32 tensor indexed by site id), set by a model around its forward when its step
# is to be captured in a hipGraph (models/vqvae/vqvae.py::enable_device_keys); None = keys travel by value.
DEVICE_KEYS = None


def make_device_keys(seed_dev, keys_dev):
    """keys_dev[s] = dropout_key(seed_dev[0], s) for every site s, on the device (smt_lm_make_keys: the derivation is the
    same for every model of this build)."""
    assert seed_dev.is_cuda and keys_dev.is_cuda and seed_dev.dtype == torch.int32 and keys_dev.dtype == torch.int32
    N.check(N.lib().smt_lm_make_keys(_p(seed_dev), _p(keys_dev), keys_dev.numel(), N.stream_ptr()), "smt_lm_make_keys")


def _set_act_out(d, u, keys, thresh, scale, site_width, first_site=None, site_stride=1):
    d.act_out, d.site_width = 1, site_width
    d.y_act, d.bs_yact, d.ld_yact = _geom(u)
    for i, k in enumerate(keys):
        d.drop_keys[i] = k
    d.drop_thresh16, d.drop_scale = thresh, scale
    if DEVICE_KEYS is not None and thresh > 0 and first_site is not None:
        assert first_site + (len(keys) - 1) * site_stride < DEVICE_KEYS.numel()
        d.drop_keys_dev = ctypes.c_void_p(DEVICE_KEYS.data_ptr() + 4 * first_site)
        d.drop_keys_dev_stride = site_stride


def _set_act_grad(d, u, scale):
    """Data-gradient epilogue: times d relu(dropout(h))/dh = scale * [u != 0]."""
    d.act_grad = 1
    d.act_grad_src, d.bs_act, d.ld_act = _geom(u)
    d.drop_scale = scale


def _dgrad_stride1(dy, weight_packed_bwd, dx, k, dilation, padding):
    c_in, c_out = dx.shape[2], dy.shape[2]
    d = _base_desc(dy, dx, None, c_out, c_in, k, 1, dilation, (k - 1) * dilation - padding, dx.shape[1])
    d.w = _p(weight_packed_bwd)
    return d


def _resample_ok(x_dtype, k, stride, padding, dilation, c_narrow, c_wide):
    """k = 4 / stride 2 / padding 1 at width 64 (the narrow side) and 64 or 128 on the other: the streaming kernels."""
    return (_RESAMPLE and x_dtype == torch.bfloat16 and k == 4 and stride == 2 and padding == 1 and dilation == 1 and
            c_narrow == 64 and c_wide in (64, 128))


def _resample(kind, name, x, wp, bias, y, lens_in, lens_out, c_other):
    """kind 'conv' = smt_conv4s2 (c_other = input channels), 'convt' = smt_convt4s2 (c_other = output channels)."""
    (px, bsx, ldx_), (py, bsy, ldy) = _geom(x), _geom(y)
    b, t_in = x.shape[0], x.shape[1]
    nbytes = (x.numel() + y.numel()) * 2.0
    flops = 2.0 * b * (t_in // 2 if kind == "conv" else t_in * 2) * (4 if kind == "conv" else 2) * 64 * c_other
    fn = N.lib().smt_conv4s2 if kind == "conv" else N.lib().smt_convt4s2
    with profiler.region(("conv4s2:" if kind == "conv" else "convt4s2:") + name, nbytes=nbytes, flops=flops, bound="hbm", dtype="bf16"):
        N.check(fn(px, bsx, ldx_, _p(wp), _p(bias), py, bsy, ldy, _p(lens_in), _p(lens_out), b, t_in, c_other,
                   _p(_zero_page(x.device)), N.stream_ptr()), "smt_conv4s2" if kind == "conv" else "smt_convt4s2")


def _gate_mix_fwd(z, g, depth):
    """g = sum_d tanh(t_d) * softmax_d(s_d) over the ``depth`` branches side by side in z's rows (smt_gate_mix_fwd)."""
    w = g.shape[-1]
    with profiler.region("gate_mix_fwd", nbytes=z.numel() * z.element_size() * 1.125, bound="hbm"):
        N.check(N.lib().smt_gate_mix_fwd(_p(z), _p(g), _DT[z.dtype], z.numel() // z.shape[-1], w, depth, z.shape[-1], w,
                                         N.stream_ptr()), "smt_gate_mix_fwd")


def _gate_mix_bwd(z, dg, dz, depth):
    w = dg.shape[-1]
    with profiler.region("gate_mix_bwd", nbytes=z.numel() * z.element_size() * 2.125, bound="hbm"):
        N.check(N.lib().smt_gate_mix_bwd(_p(z), _p(dg), _p(dz), _DT[z.dtype], z.numel() // z.shape[-1], w, depth,
                                         z.shape[-1], w, z.shape[-1], N.stream_ptr()), "smt_gate_mix_bwd")


# ---- autograd functions ----
class _Conv1d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, lens, stride, padding, dilation):
        b, t_in, c_in = x.shape
        c_out, _, k = weight.shape
        t_out = (t_in + 2 * padding - dilation * (k - 1) - 1) // stride + 1
        y = torch.empty(b, t_out, c_out, dtype=x.dtype, device=x.device)
        lens32 = _i32(lens)
        wp = _pack_fwd(weight, x.dtype)
        if residual is None and t_in % 2 == 0 and _resample_ok(x.dtype, k, stride, padding, dilation, c_out, c_in):
            _resample("conv", "fwd", x, wp, bias, y, lens32, None, c_in)
        else:
            d = _base_desc(x, y, lens32, c_in, c_out, k, stride, dilation, padding, t_out)
            d.w, d.bias = _p(wp), _p(bias)
            if residual is not None:
                d.res, d.bs_res, d.ld_res = _geom(residual)
            _launch(d, "conv_fwd", _conv_flops(d), _conv_bytes(d, x.element_size()))
        ctx.save_for_backward(x, weight, lens32 if lens32 is not None else torch.empty(0))
        ctx.cfg = (stride, padding, dilation, lens is not None, residual is not None, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, lens32 = ctx.saved_tensors
        stride, padding, dilation, has_lens, has_res, has_bias = ctx.cfg
        lens32 = lens32 if has_lens else None
        b, t_in, c_in = x.shape
        c_out, _, k = weight.shape
        if dy.stride(2) != 1:
            dy = dy.contiguous()
        t_out = dy.shape[1]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(b, t_in, c_in, dtype=x.dtype, device=x.device)
            if stride == 1:
                d = _dgrad_stride1(dy, _pack_bwd(weight, x.dtype), dx, k, dilation, padding)
                d.lens_out = _p(lens32)
                _launch(d, "conv_dgrad", _conv_flops(d), _conv_bytes(d, x.element_size()))
            elif t_in == 2 * t_out and _resample_ok(x.dtype, k, stride, padding, dilation, c_out, c_in):
                # dx[2m + ph] = two taps of W^T on dy: the transposed streaming kernel, both phases from one read of dy
                wt = _pack(weight, x.dtype, c_in, c_out, k, c_in * k, 1, list(range(k)))
                _resample("convt", "dgrad", dy, wt, None, dx, None, lens32, c_in)
            else:
                for ph, (taps, pad_eff) in enumerate(_phases(k, stride, padding)):
                    n_ph = (t_in - ph + stride - 1) // stride
                    if n_ph <= 0:
                        continue
                    wb = _pack(weight, x.dtype, c_in, c_out, k, c_in * k, 1, taps)
                    d = _base_desc(dy, dx, None, c_out, c_in, len(taps), 1, 1, pad_eff, n_ph, stride, ph)
                    d.w = _p(wb)
                    d.lens_out = _p(lens32)
                    _launch(d, "conv_dgrad", _conv_flops(d), _conv_bytes(d, x.element_size()))
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(weight)
            db = torch.empty(c_out, dtype=torch.float32, device=x.device)
            d = _base_desc(x, dy, lens32, c_in, c_out, k, stride, dilation, padding, t_out)
            _wgrad(d, dw, c_in * k, k, 1, list(range(k)), db)
            if not has_bias:
                db = None
        return dx, dw, db, (dy if has_res else None), None, None, None, None


def conv1d(x, weight, bias, *, stride=1, padding=0, dilation=1, lens=None, residual=None):
    """y[b,t,:] = bias + sum_j W_j . x[b, t*stride + j*dilation - padding, :] (+ residual), rows
    t >= lens[b] of x read as zero; ``weight`` keeps torch's Conv1d layout [Cout, Cin, k]."""
    return _Conv1d.apply(x, weight, bias, residual, lens, stride, padding, dilation)


class _ConvTranspose1d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, lens, stride, padding):
        b, t_in, c_in = x.shape
        _, c_out, k = weight.shape
        t_y = (t_in - 1) * stride - 2 * padding + k
        y = torch.empty(b, t_y, c_out, dtype=x.dtype, device=x.device)
        lens32 = _i32(lens)
        fast = _resample_ok(x.dtype, k, stride, padding, 1, c_in, c_out)
        if fast:
            _resample("convt", "fwd", x, _pack(weight, x.dtype, c_out, c_in, k, c_out * k, 1, list(range(k))), bias, y, lens32,
                      None, c_out)
        for ph, (taps, pad_eff) in enumerate(() if fast else _phases(k, stride, padding)):
            n_ph = (t_y - ph + stride - 1) // stride
            wp = _pack(weight, x.dtype, c_out, c_in, k, c_out * k, 1, taps)
            d = _base_desc(x, y, lens32, c_in, c_out, len(taps), 1, 1, pad_eff, n_ph, stride, ph)
            d.w, d.bias = _p(wp), _p(bias)
            _launch(d, "conv_fwd", _conv_flops(d), _conv_bytes(d, x.element_size()))
        ctx.save_for_backward(x, weight, lens32 if lens32 is not None else torch.empty(0))
        ctx.cfg = (stride, padding, lens is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, lens32 = ctx.saved_tensors
        stride, padding, has_lens = ctx.cfg
        lens32 = lens32 if has_lens else None
        b, t_in, c_in = x.shape
        _, c_out, k = weight.shape
        if dy.stride(2) != 1:
            dy = dy.contiguous()
        t_y = dy.shape[1]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            # dx[m, ci] = sum_j sum_co dy[s*m + j - p, co] W[ci, co, j]: a strided convolution over dy
            dx = torch.empty(b, t_in, c_in, dtype=x.dtype, device=x.device)
            wb = _pack(weight, x.dtype, c_in, c_out, c_out * k, k, 1, list(range(k)))
            if t_y == 2 * t_in and _resample_ok(x.dtype, k, stride, padding, 1, c_in, c_out):
                _resample("conv", "dgrad", dy, wb, None, dx, None, lens32, c_out)
            else:
                d = _base_desc(dy, dx, None, c_out, c_in, k, stride, 1, padding, t_in)
                d.w = _p(wb)
                d.lens_out = _p(lens32)
                _launch(d, "conv_dgrad", _conv_flops(d), _conv_bytes(d, x.element_size()))
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(weight)
            db = torch.zeros(c_out, dtype=torch.float32, device=x.device)
            for ph, (taps, pad_eff) in enumerate(_phases(k, stride, padding)):
                n_ph = (t_y - ph + stride - 1) // stride
                d = _base_desc(x, dy, lens32, c_in, c_out, len(taps), 1, 1, pad_eff, n_ph, stride, ph)
                db_ph = torch.empty(c_out, dtype=torch.float32, device=x.device)
                _wgrad(d, dw, k, c_out * k, 1, taps, db_ph)
                db += db_ph
        return dx, dw, db, None, None, None


def conv_transpose1d(x, weight, bias, *, stride, padding, lens=None):
    """ConvTranspose1d with torch's [Cin, Cout, k] weight layout (one launch per output phase)."""
    return _ConvTranspose1d.apply(x, weight, bias, lens, stride, padding)


class _GateMix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, depth):
        b, t, c = z.shape
        g = torch.empty(b, t, c // (2 * depth), dtype=z.dtype, device=z.device)
        assert z.is_contiguous()
        _gate_mix_fwd(z, g, depth)
        ctx.save_for_backward(z)
        ctx.depth = depth
        return g

    @staticmethod
    def backward(ctx, dg):
        z, = ctx.saved_tensors
        dz = torch.empty_like(z)
        _gate_mix_bwd(z, dg.contiguous(), dz, ctx.depth)
        return dz, None


def gate_mix(z, depth: int):
    """sum_d tanh(t_d) * softmax_d(s_d); z = [.., d*2w + (0..w-1)] = t_d, [.., d*2w + (w..2w-1)] = s_d."""
    return _GateMix.apply(z, depth)


def _wavenet_gate_fwd(z, a, lens32):
    (pz, bsz, ldz), (pa, bsa, lda) = _geom(z), _geom(a)
    b, t, h = a.shape
    with profiler.region("wavenet_gate_fwd", nbytes=float(b) * t * 3 * h * z.element_size(), bound="hbm"):
        N.check(N.lib().smt_wavenet_gate_fwd(pz, bsz, ldz, pa, bsa, lda, _p(lens32), b, t, h, _DT[z.dtype], N.stream_ptr()),
                "smt_wavenet_gate_fwd")


def _wavenet_gate_bwd(z, da, dz, lens32):
    (pz, bsz, ldz), (pda, bsda, ldda), (pdz, bsdz, lddz) = _geom(z), _geom(da), _geom(dz)
    b, t, h = da.shape
    with profiler.region("wavenet_gate_bwd", nbytes=float(b) * t * 5 * h * z.element_size(), bound="hbm"):
        N.check(N.lib().smt_wavenet_gate_bwd(pz, bsz, ldz, pda, bsda, ldda, pdz, bsdz, lddz, _p(lens32), b, t, h, _DT[z.dtype],
                                             N.stream_ptr()), "smt_wavenet_gate_bwd")


class _WaveNetGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, lens):
        b, t, c = z.shape
        lens32 = _i32(lens)
        a = torch.empty(b, t, c // 2, dtype=z.dtype, device=z.device)
        _wavenet_gate_fwd(z, a, lens32)
        ctx.save_for_backward(z, lens32 if lens32 is not None else torch.empty(0))
        ctx.has_lens = lens is not None
        return a

    @staticmethod
    def backward(ctx, da):
        z, lens32 = ctx.saved_tensors
        dz = torch.empty_like(z)
        _wavenet_gate_bwd(z, da.contiguous(), dz, lens32 if ctx.has_lens else None)
        return dz, None


def wavenet_gate(z, lens=None):
    """tanh(z[..., :H]) * sigmoid(z[..., H:]) on rows t < lens[b], zero on the others (which are not read); z is [B, T, 2H]."""
    return _WaveNetGate.apply(z, lens)


def _wn_tail_ok(dtype, hidden):
    return _WN_TAIL and dtype == torch.bfloat16 and hidden in _WN_TAIL_WIDTHS


class _WaveNetTail(torch.autograd.Function):
    """The fused tail: z is the only activation kept (the gated a is recomputed in backward)."""

    @staticmethod
    def forward(ctx, z, x, weight, bias, lens):
        b, t, h = x.shape
        lens32 = _i32(lens)
        y = torch.empty(b, t, h, dtype=x.dtype, device=x.device)
        (pz, bsz, ldz), (px, bsx, ldx_), (py, bsy, ldy) = _geom(z), _geom(x), _geom(y)
        rows = float(b) * t
        with profiler.region("wavenet_tail", flops=2.0 * rows * h * h, nbytes=rows * 4 * h * 2 + h * h * 2, bound="hbm",
                             dtype="bf16"):
            N.check(N.lib().smt_wavenet_tail_fwd(pz, bsz, ldz, px, bsx, ldx_, _p(_pack_fwd(weight, x.dtype)), _p(bias), py, bsy,
                                                 ldy, _p(lens32), b, t, h, N.stream_ptr()), "smt_wavenet_tail_fwd")
        ctx.save_for_backward(z, weight, lens32 if lens32 is not None else torch.empty(0))
        ctx.cfg = (lens is not None, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, weight, lens32 = ctx.saved_tensors
        has_lens, has_bias = ctx.cfg
        lens32 = lens32 if has_lens else None
        b, t, c = z.shape
        h = c // 2
        dy = dy.contiguous()
        a = torch.empty(b, t, h, dtype=z.dtype, device=z.device)          # scratch: recomputed, not kept by forward
        _wavenet_gate_fwd(z, a, lens32)
        da = torch.empty_like(a)
        dw = torch.empty_like(weight)
        db = torch.empty(h, dtype=torch.float32, device=z.device)
        if h == 64:       # data, weight and bias gradient of the 64 -> 64 1x1 in one pass over dy
            _conv_gate_bwd(dy, a, _pack_bwd(weight, z.dtype), da, lens32, dw, db)
        else:
            d = _dgrad_stride1(dy, _pack_bwd(weight, z.dtype), da, 1, 1, 0)
            d.lens_out = _p(lens32)
            _launch(d, "conv_dgrad", _conv_flops(d), _conv_bytes(d, z.element_size()))
            _wgrad(_base_desc(a, dy, lens32, h, h, 1, 1, 1, 0, t), dw, h, 1, 1, [0], db)
        del a
        dz = torch.empty_like(z)
        _wavenet_gate_bwd(z, da, dz, lens32)
        return dz, dy, dw, (db if has_bias else None), None


def wavenet_tail(z, x, weight, bias, lens=None):
    """One WaveNet layer after its dilated conv: x + bias + W_g . (tanh(z_t) * sigmoid(z_s)); z [B, T, 2H], x [B, T, H], ``weight``
    the 1x1 gate conv in torch's layout [H, H, 1].  In bf16 at the widths of _WN_TAIL_WIDTHS this is one kernel that never
    stores the gated tensor (rows >= lens[b] of its output are zero); otherwise the gate kernel followed by conv1d."""
    if _wn_tail_ok(x.dtype, x.shape[2]):
        return _WaveNetTail.apply(z, x, weight, bias, lens)
    return conv1d(wavenet_gate(z, lens), weight, bias, lens=lens, residual=x)


class _ConvIn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, lens, stride, padding, out_dtype):
        b, t_in = x.shape
        c_out, _, k = weight.shape
        t_out = max(0, (t_in + 2 * padding - k) // stride + 1)       # an input shorter than the kernel gives no rows
        y = torch.empty(b, t_out, c_out, dtype=out_dtype, device=x.device)
        lens32 = _i32(lens)
        with profiler.region("conv_in_fwd", nbytes=x.numel() * 4 + y.numel() * y.element_size(), bound="hbm"):
            if y.numel():                                            # (an empty tensor has no storage to point the kernel at)
                N.check(N.lib().smt_conv_in_fwd(_p(x), _p(weight), _p(bias), _p(lens32), _p(y), _DT[out_dtype], b, t_in,
                                                t_out, c_out, k, stride, padding, N.stream_ptr()), "smt_conv_in_fwd")
        ctx.save_for_backward(x, weight, lens32 if lens32 is not None else torch.empty(0))
        ctx.cfg = (stride, padding, lens is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, lens32 = ctx.saved_tensors
        stride, padding, has_lens = ctx.cfg
        lens32 = lens32 if has_lens else None
        b, t_in = x.shape
        c_out, _, k = weight.shape
        dy = dy.contiguous()
        if dy.numel() == 0:                                          # no output rows: nothing to sum
            return None, torch.zeros_like(weight), torch.zeros(c_out, dtype=torch.float32, device=x.device), None, None, None, None
        dw = torch.empty_like(weight)
        db = torch.empty(c_out, dtype=torch.float32, device=x.device)
        lib = N.lib()
        ws_bytes = lib.smt_conv_in_wgrad_workspace_bytes(b, dy.shape[1], c_out)
        ws = N.workspace.get(ws_bytes, x.device)
        with profiler.region("conv_in_wgrad", nbytes=x.numel() * 4 + dy.numel() * dy.element_size(), bound="hbm"):
            N.check(lib.smt_conv_in_wgrad(_p(x), _p(dy), _p(lens32), _p(dw), _p(db), _DT[dy.dtype], b, t_in,
                                          dy.shape[1], c_out, k, stride, padding, _p(ws), ws.numel(), N.stream_ptr()),
                    "smt_conv_in_wgrad")
        return None, dw, db, None, None, None, None


def conv_in(x, weight, bias, *, stride, padding, lens=None, out_dtype=torch.float32):
    """First encoder conv: x fp32 [B, T] (one channel) -> [B, T_out, C]."""
    return _ConvIn.apply(x, weight, bias, lens, stride, padding, out_dtype)


class _ConvOut(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, lens):
        b, t, c = x.shape
        assert x.is_contiguous()
        y = torch.empty(b, t, dtype=torch.float32, device=x.device)
        lens32 = _i32(lens)
        with profiler.region("conv_out_fwd", nbytes=x.numel() * x.element_size() + y.numel() * 4, bound="hbm"):
            N.check(N.lib().smt_conv_out_fwd(_p(x), _p(weight), _p(bias), _p(lens32), _p(y), _DT[x.dtype], b, t, c,
                                             N.stream_ptr()), "smt_conv_out_fwd")
        ctx.save_for_backward(x, weight, lens32 if lens32 is not None else torch.empty(0))
        ctx.has_lens = lens is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, lens32 = ctx.saved_tensors
        lens32 = lens32 if ctx.has_lens else None
        b, t, c = x.shape
        dy = dy.contiguous().float()
        dx = torch.empty_like(x)
        dw = torch.empty_like(weight)
        db = torch.empty(1, dtype=torch.float32, device=x.device)
        lib = N.lib()
        ws_bytes = lib.smt_conv_out_bwd_workspace_bytes(b, t, c)
        ws = N.workspace.get(ws_bytes, x.device)
        with profiler.region("conv_out_bwd", nbytes=2 * x.numel() * x.element_size() + dy.numel() * 4, bound="hbm"):
            N.check(lib.smt_conv_out_bwd(_p(x), _p(weight), _p(lens32), _p(dy), _p(dx), _p(dw), _p(db), _DT[x.dtype], b,
                                         t, c, _p(ws), ws.numel(), N.stream_ptr()), "smt_conv_out_bwd")
        return dx, dw, db, None


def conv_out(x, weight, bias, *, lens=None):
    """Final decoder projection to one channel on masked rows: [B, T, C] -> fp32 [B, T]."""
    return _ConvOut.apply(x, weight, bias, lens)


# ----------------------------------------------------------------------------------------------
# GatedHiFiBlock as ONE autograd node (reference models/vqvae/resnet.py:184-241).
#
# forward                                             tensors kept for backward
#   h1|u1 = K1cat(x*mask)        one GEMM, N = D*2w   u1   (u = relu(dropout(h)), written by the
#   u2_d  = act(K2_d(u1_d))      dilated, per branch  u2    producing conv's epilogue; h2 is never
#   z_d   = h1_d + K3_d(u2_d)    1x1 + residual       z     stored, h1 only until z is formed)
#   g     = gate_mix(z)                               g
#   out   = x + Kg(g*mask)                            x
# backward: every data gradient is the same GEMM kernel on repacked weights with the activation
# derivative (scale * [u != 0]), the row mask and the residual-gradient add fused in its epilogue.
# ----------------------------------------------------------------------------------------------
class _GatedHiFi(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lens, geometry, drop, n_params, *params):
        """params = per branch (w1, b1, w2, b2, w3, b3) * depth + (wg, bg); drop = (p, training, seed, site_base)."""
        depth = len(geometry)
        b, t, w = x.shape
        c2 = 2 * w
        dt, dev = x.dtype, x.device
        lens32 = _i32(lens)
        p_drop, training, seed, site_base = drop
        specs = [[DropSpec(p_drop, training, seed, site_base + 2 * d + s).params() for s in (0, 1)] for d in range(depth)]
        thresh, scale = specs[0][0][1], specs[0][0][2]
        br = [params[6 * d:6 * d + 6] for d in range(depth)]
        wg, bg = params[6 * depth], params[6 * depth + 1]

        # K1 for all branches at once.  On the LDS-DMA path (bf16, 2w == 128, w == 64) only the activated
        # output u1 is written: K3 recomputes its residual h1 = K1(x) + b1 from x (folded second term).
        fold = _dma_ok(dt, c2, c2) and c2 == 128 and w == 64
        b1cat = _cat_bias([p[1] for p in br])
        u1 = torch.empty(b, t, depth * c2, dtype=dt, device=dev)
        h1 = None if fold else torch.empty_like(u1)
        d1 = _base_desc(x, h1, lens32, w, depth * c2, 1, 1, 1, 0, t, t_y=t)
        d1.w, d1.bias = _p(_pack_cat_fwd([p[0] for p in br], dt)), _p(b1cat)
        _set_act_out(d1, u1, [specs[d][0][0] for d in range(depth)], thresh, scale, c2, site_base, 2)
        if fold:
            d1.zero_page = _p(_zero_page(dev))     # enables the persistent activated-output kernel (conv_k1act)
        _launch(d1, "conv_fwd", _conv_flops(d1), _conv_bytes(d1, x.element_size()))

        u2 = torch.empty_like(u1)
        z = torch.empty_like(u1)
        for d, (k, dil, pad) in enumerate(geometry):
            sl = slice(d * c2, (d + 1) * c2)
            u1_d, u2_d = u1[:, :, sl], u2[:, :, sl]
            d2 = _base_desc(u1_d, None, None, c2, c2, k, 1, dil, pad, t, t_y=t)
            dma = _dma_ok(dt, c2, c2)
            wp2 = _pack_fwd(br[d][2], dt, dma)
            d2.w, d2.bias = _p(wp2), _p(br[d][3])
            if dma:
                _use_dma(d2, wp2)
            _set_act_out(d2, u2_d, [specs[d][1][0]], thresh, scale, c2, site_base + 2 * d + 1, 1)
            _launch(d2, "conv_fwd", _conv_flops(d2), _conv_bytes(d2, x.element_size()))
        k3gate = fold and depth == 4 and _K3GATE
        g = torch.empty(b, t, w, dtype=dt, device=dev)
        if k3gate:     # K3 of the four branches + tanh * softmax gate in one pass: z is written once and never re-read here
            _conv_k3gate(u2, x, _pack_cat_fwd([p[4] for p in br], dt, swizzle=True), _pack_cat_fwd([p[0] for p in br], dt),
                         _cat_bias([p[5] for p in br]), b1cat, z, g, lens32)
        for d in range(0 if k3gate else depth):
            sl = slice(d * c2, (d + 1) * c2)
            d3 = _base_desc(u2[:, :, sl], z[:, :, sl], None, c2, c2, 1, 1, 1, 0, t)
            dma = _dma_ok(dt, c2, c2)
            wp3 = _pack_fwd(br[d][4], dt, dma)
            d3.w, d3.bias = _p(wp3), _p(br[d][5])
            if dma:
                _use_dma(d3, wp3)
            if fold:
                w1p = _pack_fwd(br[d][0], dt)                   # [2w][w], plain layout
                d3.x2, d3.bs_x2, d3.ld_x2 = _geom(x)
                d3.w2, d3.bias2, d3.c_in2, d3.lens_in2 = _p(w1p), _p(br[d][1]), w, _p(lens32)
            else:
                d3.res, d3.bs_res, d3.ld_res = _geom(h1[:, :, sl])
            _launch(d3, "conv_fwd", _conv_flops(d3) * (1.0 + (0.5 if fold else 0.0)),
                    _conv_bytes(d3, x.element_size()))
        del h1
        if not k3gate:
            _gate_mix_fwd(z, g, depth)
        out = torch.empty_like(x)
        dg_ = _base_desc(g, out, lens32, w, w, 1, 1, 1, 0, t)
        dg_.w, dg_.bias = _p(_pack_fwd(wg, dt)), _p(bg)
        dg_.res, dg_.bs_res, dg_.ld_res = _geom(x)
        dg_.zero_page = _p(_zero_page(x.device))   # opts into the streaming kernels (conv1x1_c64 at width 64)
        _launch(dg_, "conv_fwd", _conv_flops(dg_), _conv_bytes(dg_, x.element_size()))

        ctx.save_for_backward(x, lens32 if lens32 is not None else torch.empty(0), u1, u2, z, g, *params)
        ctx.cfg = (geometry, scale, lens is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, lens32, u1, u2, z, g, *params = ctx.saved_tensors
        geometry, scale, has_lens = ctx.cfg
        lens32 = lens32 if has_lens else None
        dout = dout.contiguous()
        with reduce_batch(x.device):      # the block's ten weight gradients: one slab-reduction launch at the end
            return _GatedHiFi._backward(x, lens32, u1, u2, z, g, params, geometry, scale, dout)

    @staticmethod
    def _backward(x, lens32, u1, u2, z, g, params, geometry, scale, dout):
        depth = len(geometry)
        b, t, w = x.shape
        c2 = 2 * w
        dt, dev = x.dtype, x.device
        br = [params[6 * d:6 * d + 6] for d in range(depth)]
        wg, bg = params[6 * depth], params[6 * depth + 1]
        grads = [None] * len(params)

        def f32(shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)

        # gate conv: dg = (dout . Wg^T) * mask ; dWg, dbg
        dg = torch.empty_like(g)
        grads[6 * depth], grads[6 * depth + 1] = torch.empty_like(wg), f32(bg.shape)
        if dt == torch.bfloat16 and w == 64:
            # data gradient and weight gradient both read dout: one fused pass
            _conv_gate_bwd(dout, g, _pack_bwd(wg, dt), dg, lens32, grads[6 * depth], grads[6 * depth + 1])
        else:
            d = _dgrad_stride1(dout, _pack_bwd(wg, dt), dg, 1, 1, 0)
            d.lens_out = _p(lens32)
            _launch(d, "conv_dgrad", _conv_flops(d), _conv_bytes(d, x.element_size()))
            _wgrad(_base_desc(g, dout, lens32, w, w, 1, 1, 1, 0, t), grads[6 * depth], w, 1, 1, [0], grads[6 * depth + 1])

        dz = torch.empty_like(z)
        _gate_mix_bwd(z, dg, dz, depth)
        del dg
        dh1 = torch.empty_like(z)
        dh2 = torch.empty(b, t, c2, dtype=dt, device=dev)     # one branch at a time
        for dd, (k, dil, pad) in enumerate(geometry):
            sl = slice(dd * c2, (dd + 1) * c2)
            w1, b1, w2, b2, w3, b3 = br[dd]
            dz_d, u1_d, u2_d = dz[:, :, sl], u1[:, :, sl], u2[:, :, sl]
            # K3: dh2 = (dz_d . W3^T) * act'(u2);  dW3 = u2^T dz_d
            dma = _dma_ok(dt, c2, c2)
            wb3 = _pack_bwd(w3, dt, dma)
            d = _dgrad_stride1(dz_d, wb3, dh2, 1, 1, 0)
            if dma:
                _use_dma(d, wb3)
            _set_act_grad(d, u2_d, scale)
            grads[6 * dd + 4], grads[6 * dd + 5] = torch.empty_like(w3), f32(b3.shape)
            if dma and c2 == 128:
                # data gradient and weight gradient read the same two operands (dz_d, u2_d): one fused pass
                _conv1x1_bwd(d, grads[6 * dd + 4], c2, 1, grads[6 * dd + 5])
            else:
                _launch(d, "conv_dgrad", _conv_flops(d), _conv_bytes(d, x.element_size()))
                _wgrad(_base_desc(u2_d, dz_d, None, c2, c2, 1, 1, 1, 0, t), grads[6 * dd + 4], c2, 1, 1, [0],
                       grads[6 * dd + 5])
            # K2: dh1_d = (dh2 * W2^T) * act'(u1) + dz_d;  dW2 = u1^T dh2
            wb2 = _pack_bwd(w2, dt, dma)
            d = _dgrad_stride1(dh2, wb2, dh1[:, :, sl], k, dil, pad)
            if dma:
                _use_dma(d, wb2)
            _set_act_grad(d, u1_d, scale)
            d.res, d.bs_res, d.ld_res = _geom(dz_d)
            _launch(d, "conv_dgrad", _conv_flops(d), _conv_bytes(d, x.element_size()))
            grads[6 * dd + 2], grads[6 * dd + 3] = torch.empty_like(w2), f32(b2.shape)
            _wgrad(_base_desc(u1_d, dh2, None, c2, c2, k, 1, dil, pad, t), grads[6 * dd + 2], c2 * k, k, 1,
                   list(range(k)), grads[6 * dd + 3])
        del dz, dh2
        # K1cat: dx = (dh1 . W1cat^T) * mask + dout ; dW1cat
        dx = torch.empty_like(x)
        dw1cat, db1cat = torch.empty(depth * c2, w, 1, dtype=torch.float32, device=dev), f32((depth * c2,))
        if dt == torch.bfloat16 and w == 64 and depth * c2 == 512:
            # data gradient and weight gradient both stream the 1 KiB rows of dh1: one fused pass
            _conv_k1_bwd(dh1, x, _pack_cat_bwd([p[0] for p in br], dt), dout, dx, lens32, dw1cat, db1cat)
        else:
            d = _dgrad_stride1(dh1, _pack_cat_bwd([p[0] for p in br], dt), dx, 1, 1, 0)
            d.lens_out = _p(lens32)
            d.res, d.bs_res, d.ld_res = _geom(dout)
            _launch(d, "conv_dgrad", _conv_flops(d), _conv_bytes(d, x.element_size()))
            _wgrad(_base_desc(x, dh1, lens32, w, depth * c2, 1, 1, 1, 0, t), dw1cat, w, 1, 1, [0], db1cat)
        for dd in range(depth):
            grads[6 * dd] = dw1cat[dd * c2:(dd + 1) * c2]
            grads[6 * dd + 1] = db1cat[dd * c2:(dd + 1) * c2]
        return (dx, None, None, None, None, *grads)


def gated_hifi_block(x, lens, geometry, params, *, p_drop, training, seed, site_base):
    """x [B, T, w]; geometry = [(k, dilation, padding)] per branch; params = flat list
    (w1, b1, w2, b2, w3, b3) per branch followed by (gate.weight, gate.bias)."""
    return _GatedHiFi.apply(x, lens, tuple(geometry), (p_drop, training, seed, site_base), len(params), *params)
