"""The plan of smt_conv1d_wgrad, asked of the library without a GPU: smt_conv1d_wgrad_kernel_name and
smt_conv1d_wgrad_workspace_bytes read only the descriptor, so a hand-filled one with dummy non-null pointers answers.  The
names are what the profiler regions, tests/test_fastpath_parity_gpu.py and bench.py's rooflines_other.conv_wgrad group key on;
the byte counts size the workspace that convops hands to every weight gradient."""
import ctypes

import pytest

from smt_amd import convops as C
from smt_amd import native as N

DUMMY = 0x1000      # never dereferenced


def desc(batch, t, k, dil=1, c_in=128, c_out=128, dtype=C.SMT_BF16, zero_page=True, stride=1, pad=None, t_out=None,
         out_stride=1, out_offset=0):
    d = C.ConvDesc()
    d.dtype = dtype
    t_out = t if t_out is None else t_out
    d.batch, d.t_in, d.t_out, d.t_y = batch, t, t_out, t_out * out_stride
    d.c_in, d.c_out = c_in, c_out
    d.taps, d.stride, d.dilation, d.padding = k, stride, dil, ((k - 1) * dil // 2 if pad is None else pad)
    d.out_stride, d.out_offset = out_stride, out_offset
    d.ld_x, d.ld_y = c_in, c_out
    d.bs_x, d.bs_y = c_in * t, c_out * d.t_y
    d.x = d.y = DUMMY
    if zero_page:
        d.zero_page = DUMMY
    d.drop_scale = 1.0
    return d


def name(*a, **kw):
    return N.lib().smt_conv1d_wgrad_kernel_name(ctypes.byref(desc(*a, **kw))).decode()


def ws_bytes(*a, **kw):
    return N.lib().smt_conv1d_wgrad_workspace_bytes(ctypes.byref(desc(*a, **kw)))


def down(**kw):
    """the 64 -> 64, k = 4, stride-2 resampling conv"""
    return desc(3, 4000, 4, c_in=64, c_out=64, stride=2, pad=1, t_out=2000, **kw)


def up_phase(**kw):
    """a two-tap phase (rows x[m - 1], x[m] against dy[2m]) of the 64 -> 128 transposed resampling conv"""
    return desc(3, 2000, 2, c_in=64, c_out=128, pad=1, out_stride=2, **kw)


DILATED = [(3, 1), (5, 3), (7, 9), (9, 27)]


@pytest.mark.parametrize("k,dil", DILATED)
def test_dilated_128_channel_convs_use_the_shift_kernel_only_in_bf16_with_a_zero_page(k, dil):
    assert name(3, 50021, k, dil) == "conv_wgrad_shift"
    assert name(3, 50021, k, dil, zero_page=False) == "conv_wgrad"
    assert name(3, 50021, k, dil, dtype=C.SMT_F32) == "conv_wgrad"


@pytest.mark.parametrize("k,dil,t", [(3, 1, 32640), (5, 3, 32640), (7, 9, 32256), (9, 27, 31104)])
def test_shift_kernel_starts_at_256_tiles(k, dil, t):
    # 128-row tiles per (batch, dilation class) item: one more row makes the 256th tile
    assert name(1, t, k, dil) == "conv_wgrad_dma"
    assert name(1, t + 1, k, dil) == "conv_wgrad_shift"


def test_a_dilation_class_needs_128_rows():
    assert name(32, 3455, 9, 27) == "conv_wgrad_dma"
    assert name(32, 3456, 9, 27) == "conv_wgrad_shift"


def test_other_shapes():
    assert name(3, 50021, 1) == "conv_wgrad_dma"
    assert name(3, 50021, 4, pad=1, t_out=50020) == "conv_wgrad_dma"
    assert name(3, 50021, 3, c_out=96) == "conv_wgrad"
    assert name(3, 50021, 3, c_in=256) == "conv_wgrad_shift"
    assert name(3, 50021, 3, c_out=192) == "conv_wgrad_shift"
    lib = N.lib()
    assert lib.smt_conv1d_wgrad_kernel_name(ctypes.byref(down())).decode() == "conv_wgrad"
    assert lib.smt_conv1d_wgrad_kernel_name(ctypes.byref(up_phase())).decode() == "conv_wgrad"


def test_the_window_switch_does_nothing(monkeypatch):
    """SMT_WGRAD_WINDOW=1 used to move the resampling convs to a slower mode of the LDS-DMA kernel; that mode is gone."""
    monkeypatch.setenv("SMT_WGRAD_WINDOW", "1")
    lib = N.lib()
    for d in (down(), up_phase()):
        assert lib.smt_conv1d_wgrad_kernel_name(ctypes.byref(d)).decode() == "conv_wgrad"
    assert lib.smt_conv1d_wgrad_workspace_bytes(ctypes.byref(down())) == 3932160
    assert lib.smt_conv1d_wgrad_workspace_bytes(ctypes.byref(up_phase())) == 4718592


@pytest.mark.parametrize("args,kw,expect", [
    ((3, 50021, 3, 1), {}, 62128128), ((3, 50021, 5, 3), {}, 93192192),
    ((3, 50021, 7, 9), {}, 139788288), ((3, 50021, 9, 27), {}, 170852352),
    ((1, 32640, 3, 1), {}, 66846720), ((1, 32640, 5, 3), {}, 100270080),
    ((1, 31104, 9, 27), {}, 175177728),
    ((3, 50021, 1), {}, 31064064),
    ((2, 300, 3), dict(c_in=32, c_out=64, dtype=C.SMT_F32), 655360),
])
def test_workspace_bytes(args, kw, expect):
    assert ws_bytes(*args, **kw) == expect


def test_workspace_bytes_of_the_resampling_convs():
    lib = N.lib()
    assert lib.smt_conv1d_wgrad_workspace_bytes(ctypes.byref(down())) == 3932160
    assert lib.smt_conv1d_wgrad_workspace_bytes(ctypes.byref(up_phase())) == 4718592
