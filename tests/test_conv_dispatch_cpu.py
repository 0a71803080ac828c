"""The dispatch rule of the dilated 128 -> 128 convs, asked of the library without a GPU: smt_conv1d_kernel_name reads only the
descriptor, so a hand-filled one with dummy non-null pointers answers.  The names are what the profiler regions, the GPU
kernel-selection tests and tools/bench_ws.py key on."""
import ctypes

import pytest

from smt_amd import convops as C
from smt_amd import native as N

DUMMY = 0x1000      # never dereferenced


def desc(batch, t, k, dil, epilogue):
    d = C.ConvDesc()
    d.dtype = C.SMT_BF16
    d.batch, d.t_in, d.t_out, d.t_y = batch, t, t, t
    d.c_in = d.c_out = 128
    d.taps, d.stride, d.dilation, d.padding = k, 1, dil, (k - 1) * dil // 2
    d.out_stride, d.out_offset = 1, 0
    d.ld_x = d.ld_y = d.ld_res = d.ld_act = d.ld_yact = 128
    d.bs_x = d.bs_y = d.bs_res = d.bs_act = d.bs_yact = 128 * t
    d.x = d.w = d.bias = d.zero_page = DUMMY
    d.w_swizzled = 1
    d.drop_scale = 1.0
    y, res, actgrad, actout = {"plain": (1, 0, 0, 0), "res+actgrad+actout": (1, 1, 1, 1),
                               "actout-only": (0, 0, 0, 1), "res+actgrad": (1, 1, 1, 0)}[epilogue]
    if y:
        d.y = DUMMY
    if res:
        d.res = DUMMY
    if actgrad:
        d.act_grad, d.act_grad_src = 1, DUMMY
    if actout:
        d.act_out, d.y_act, d.site_width, d.drop_thresh16 = 1, DUMMY, 128, 6554
    return d


def name(*a):
    return N.lib().smt_conv1d_kernel_name(ctypes.byref(desc(*a))).decode()


EPILOGUES = ("plain", "res+actgrad+actout", "actout-only", "res+actgrad")


@pytest.mark.parametrize("k,dil,expect", [
    (3, 1, ("conv_ws", "conv_ws", "conv_ws2", "conv_ws2")),
    (5, 3, ("conv_ws", "conv_ws", "conv_ws_pipe", "conv_ws")),
    (7, 9, ("conv_ws", "conv_ws", "conv_ws_pipe", "conv_ws")),
    (9, 27, ("conv_ws", "conv_ws", "conv_ws_pipe", "conv_ws")),
])
def test_weight_stationary_variant_per_tap_count_and_epilogue(k, dil, expect):
    assert tuple(name(3, 50021, k, dil, e) for e in EPILOGUES) == expect


@pytest.mark.parametrize("k,dil,ws", [(3, 1, "conv_ws2"), (5, 3, "conv_ws_pipe")])
def test_weight_stationary_kernels_start_at_512_tiles(k, dil, ws):
    # 128-row tiles: 65,408 rows are 511 tiles, one more row makes 512
    assert name(1, 65408, k, dil, "actout-only") == "conv_gemm_dma"
    assert name(1, 65409, k, dil, "actout-only") == ws


def test_dilation_classes_below_the_tile_threshold_use_the_streaming_kernel():
    assert name(1, 4096, 9, 27, "actout-only") == "conv_gemm_dma"
