"""The dispatch rule of the dilated 128 -> 128 convs, asked of the library without a GPU: smt_conv1d_kernel_name reads only the
descriptor, so a hand-filled one with dummy non-null pointers answers.  The names are what the profiler regions, the GPU
kernel-selection tests and tools/bench_ws.py key on.  smt_conv1d_dma_plan tells the variants behind "conv_gemm_dma" apart
(tile rows, dilation classes): the thresholds of the 256-channel level, which tests/test_conv_wide_gpu.py relies on, are
pinned here."""
import ctypes

import pytest

from smt_amd import convops as C
from smt_amd import native as N

DUMMY = 0x1000      # never dereferenced


def desc(batch, t, k, dil, epilogue, c=128):
    d = C.ConvDesc()
    d.dtype = C.SMT_BF16
    d.batch, d.t_in, d.t_out, d.t_y = batch, t, t, t
    d.c_in = d.c_out = c
    d.taps, d.stride, d.dilation, d.padding = k, 1, dil, (k - 1) * dil // 2
    d.out_stride, d.out_offset = 1, 0
    d.ld_x = d.ld_y = d.ld_res = d.ld_act = d.ld_yact = c
    d.bs_x = d.bs_y = d.bs_res = d.bs_act = d.bs_yact = c * t
    d.x = d.w = d.bias = d.zero_page = DUMMY
    d.w_swizzled = 1
    d.drop_scale = 1.0
    y, res, actgrad, actout = {"plain": (1, 0, 0, 0), "res+actgrad+actout": (1, 1, 1, 1),
                               "actout-only": (0, 0, 0, 1), "res+actgrad": (1, 1, 1, 0),
                               "res": (1, 1, 0, 0), "actgrad": (1, 0, 1, 0)}[epilogue]
    if y:
        d.y = DUMMY
    if res:
        d.res = DUMMY
    if actgrad:
        d.act_grad, d.act_grad_src = 1, DUMMY
    if actout:
        d.act_out, d.y_act, d.site_width, d.drop_thresh16 = 1, DUMMY, c, 6554
    return d


def name(*a, **kw):
    return N.lib().smt_conv1d_kernel_name(ctypes.byref(desc(*a, **kw))).decode()


def plan(*a, **kw):
    """(tile rows, row classes) of smt_conv1d_dma_plan."""
    rows, classes = ctypes.c_int(-1), ctypes.c_int(-1)
    assert N.lib().smt_conv1d_dma_plan(ctypes.byref(desc(*a, **kw)), ctypes.byref(rows), ctypes.byref(classes)) == 0
    return rows.value, classes.value


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


# ---- the 256-channel level (width 128): conv_gemm_dma at every size; smt_conv1d_dma_plan tells its variants apart ----
WIDE_K2 = [(3, 1), (5, 3), (7, 9), (9, 27)]
WIDE_SIZES = [(1, 1), (3, 700), (5, 6950), (2, 65700), (32, 18176), (32, 72704)]


@pytest.mark.parametrize("k,dil", WIDE_K2 + [(1, 1)])
def test_256_channels_run_on_the_streaming_kernel_at_every_size(k, dil):
    epilogues = ("res", "actgrad") if k == 1 else ("actout-only", "res+actgrad", "plain", "res+actgrad+actout")
    for b, t in WIDE_SIZES:
        for e in epilogues:
            assert name(b, t, k, dil, e, c=256) == "conv_gemm_dma", (b, t, e)
            rows, classes = plan(b, t, k, dil, e, c=256)
            assert rows in (128, 256) and classes >= 1


def test_plan_is_zero_off_the_streaming_kernel():
    assert name(3, 50021, 9, 27, "plain") == "conv_ws" and plan(3, 50021, 9, 27, "plain") == (0, 0)
    assert name(3, 700, 1, 1, "res") == "conv1x1_dma" and plan(3, 700, 1, 1, "res") == (0, 0)
    d = desc(3, 700, 3, 1, "plain", c=256)
    d.w_swizzled, d.zero_page = 0, None
    assert N.lib().smt_conv1d_kernel_name(ctypes.byref(d)).decode() == "conv_gemm"
    rows, classes = ctypes.c_int(-1), ctypes.c_int(-1)
    assert N.lib().smt_conv1d_dma_plan(ctypes.byref(d), ctypes.byref(rows), ctypes.byref(classes)) == 0
    assert (rows.value, classes.value) == (0, 0)
    assert N.lib().smt_conv1d_dma_plan(None, ctypes.byref(rows), ctypes.byref(classes)) == 0 and rows.value == 0
    assert N.lib().smt_conv1d_dma_plan(ctypes.byref(desc(3, 700, 3, 1, "plain", c=256)), None, None) == 0


@pytest.mark.parametrize("c", [128, 256])
def test_classes_switch_on_at_128_rows_per_class(c):
    for e in ("actout-only", "res+actgrad"):
        assert plan(2, 3455, 9, 27, e, c=c) == (128, 1) and plan(2, 3456, 9, 27, e, c=c) == (128, 27)
        assert plan(2, 1151, 7, 9, e, c=c) == (128, 1) and plan(2, 1152, 7, 9, e, c=c) == (128, 9)
        assert plan(2, 1151, 9, 27, e, c=c) == (128, 1) and plan(2, 1152, 9, 27, e, c=c) == (128, 1)
        for t in (127, 128, 1152, 3456, 6950):          # dilation 3 and 1: never
            assert plan(2, t, 5, 3, e, c=c) == (128, 1) and plan(2, t, 3, 1, e, c=c) == (128, 1)
    assert plan(5, 6950, 7, 9, "actout-only", c=256) == (128, 9) and plan(5, 6950, 9, 27, "res+actgrad", c=256) == (128, 27)


@pytest.mark.parametrize("k,dil", WIDE_K2)
def test_256_row_tiles_start_at_131072_class_rows(k, dil):
    # tc_max * B * rs >= 131072 with tc_max = ceil(T / rs): for one item the first such T is (ceil(131072 / rs) - 1) * rs + 1
    rs = dil if dil >= 8 else 1
    t_on = (-(-131072 // rs) - 1) * rs + 1
    for e in ("actout-only", "res+actgrad"):
        assert plan(1, t_on - 1, k, dil, e, c=256) == (128, rs)
        assert plan(1, t_on, k, dil, e, c=256) == (256, rs)
        assert plan(2, 65700, k, dil, e, c=256) == (256, rs)          # the GPU test's size
        assert plan(32, 18176, k, dil, e, c=256) == (256, rs)         # training size of the level


def test_k9_dilation_27_needs_classes_for_256_row_tiles():
    # without classes the halo of a 256-row tile is 8 * 27 rows: 472 rows x 256 B + two weight buffers do not fit in LDS
    assert plan(38, 3455, 9, 27, "actout-only", c=256) == (128, 1)            # 131,290 rows, classes off
    assert plan(38, 3456, 9, 27, "actout-only", c=256) == (256, 27)
    assert plan(114, 1151, 7, 9, "actout-only", c=256) == (256, 1)            # k = 7, dilation 9 fits without them


def test_one_tap_is_never_256_row():
    for e in ("res", "actgrad"):
        for b, t in WIDE_SIZES + [(1, 300000)]:
            assert plan(b, t, 1, 1, e, c=256) == (128, 1)


def test_even_tap_count_at_128_channels_is_the_single_chunk_256_row_tile():
    for e in ("actout-only", "res+actgrad"):
        d = desc(2, 65700, 4, 1, e)
        d.t_out = d.t_y = 65699                      # k = 4, padding 1: one output row fewer
        assert N.lib().smt_conv1d_kernel_name(ctypes.byref(d)).decode() == "conv_gemm_dma"
        rows, classes = ctypes.c_int(-1), ctypes.c_int(-1)
        N.lib().smt_conv1d_dma_plan(ctypes.byref(d), ctypes.byref(rows), ctypes.byref(classes))
        assert (rows.value, classes.value) == (256, 1)
