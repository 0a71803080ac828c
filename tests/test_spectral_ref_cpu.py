"""Without a GPU: (1) the float64 references of tests/spectral_ref_helpers.py pinned to the committed upstream fixtures, so
that what tests/test_spectral_float64_gpu.py compares the kernels with is provably the upstream operation; (2) the case table
of that test; (3) the length check of the spectral entry points and the frame count of the library against
smt_amd.spectral.num_frames -- both answer before any launch, so dummy non-null pointers do (as tests/test_conv_dispatch_cpu.py).

Measured (float64 reference against the fp32 fixtures): magnitudes <= 1.1e-6 of the largest bin; loss_stft 2.4e-9 and
loss_stft_nolog 4.6e-8 relative; grad_stft 4.1e-4 relative L2 (the fixture's own fp32 error: the existing GPU test allows 1e-3
against it, which is why the float64 test exists); mel 3.0e-6; inverse 4.8e-7.
"""
import ctypes

import numpy as np
import pytest
import torch

import spectral_ref_helpers as H
from smt_amd import native as N
from smt_amd import spectral

T = torch.from_numpy
DUMMY = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch


# ------------------------------------------------------------------------------ the references are the upstream operations

@pytest.mark.parametrize("cfg", [(1024, 256, 1024), (2048, 240, 1200), (1024, 120, 600), (512, 50, 240)])
def test_magnitude_reference_matches_the_upstream_fixture(golden, cfg):
    g = golden("stft")
    ref = T(g["mag_%d_%d_%d" % cfg]).double()
    mine = H.magnitude64(T(g["x"]), cfg)
    assert mine.shape == ref.shape
    err = float((mine - ref).abs().max() / ref.max())
    print(cfg, "max abs error / largest bin", err)
    assert err <= 2e-6


def _multires(g, use_log):
    y, yh, lens = T(g["y"])[:, 0], T(g["yh"])[:, 0], g["lens"].tolist()
    refs = [H.stft_loss64(y, yh, lens, cfg, use_log, upstream=1.0 / 3) for cfg in H.MODEL_RESOLUTIONS]
    return sum(r["loss"] for r in refs) / 3, sum(r["grad"] for r in refs)


def test_loss_reference_matches_the_upstream_fixture(golden):
    g = golden("losses")
    loss, grad = _multires(g, True)
    nolog, _ = _multires(g, False)
    ref = T(g["grad_stft"])[:, 0].double()
    e_log = abs(loss - float(g["loss_stft"])) / loss
    e_nolog = abs(nolog - float(g["loss_stft_nolog"])) / nolog
    e_grad = H.rel_l2(ref, grad)
    print(f"loss_stft {e_log:.3g} loss_stft_nolog {e_nolog:.3g} relative; grad_stft {e_grad:.3g} relative L2")
    # the fixture is fp32: its stored value rounds at 6e-8, its sums over ~1e6 fp32 terms add a few 1e-7
    assert e_log <= 1e-6 and e_nolog <= 1e-6
    assert e_grad < 1e-3
    # the masked tail: no gradient beyond the support of the last kept frame, in both
    assert (grad[2, 3072 + 2048:] == 0).all() and (ref[2, 3072 + 2048:] == 0).all()


def test_log_mel_reference_matches_the_upstream_fixture(golden):
    g = golden("mel")
    ref = H.log_mel64(T(g["x"]), (1024, 256, 1024), T(g["mel_basis"]))
    err = H.max_abs(T(g["mel"]), ref["mel"])
    print("mel max abs error", err)
    assert err <= 2e-5


def test_inverse_reference_matches_the_upstream_fixture(golden):
    g = golden("stft_inverse")
    for tag in "abc":
        cfg = tuple(int(v) for v in g[f"{tag}_cfg"])
        mine = H.stft_inverse64(T(g[f"{tag}_mag"]), T(g[f"{tag}_phase"]), cfg)
        ref = T(g[f"{tag}_y"])
        assert mine.shape == ref.shape
        err = H.max_abs(ref, mine)
        print(tag, cfg, "inverse max abs error", err, "max|ref|", float(ref.abs().max()))
        assert err <= 1e-5


def test_zero_sum_items_have_zero_loss_and_zero_gradient():
    """Where the reference departs from torch's autograd on purpose (inf * 0 = nan): identical signals and unkept items."""
    cfg = (256, 64, 256)
    y, yh = H.make_signals(cfg, 323)
    yh[1] = y[1]
    ref = H.stft_loss64(y, yh, [323, 323, 0], cfg, True)
    assert np.isfinite(ref["loss"]) and torch.isfinite(ref["grad"]).all()
    assert (ref["grad"][1:] == 0).all() and ref["grad"][0].abs().max() > 0


# ------------------------------------------------------------------------------------------------------ the case table

def test_case_table_covers_every_frame_remainder():
    rem = set()
    for cfg in H.CONFIGS:
        n_fft, hop, win = cfg
        for t in H.lengths(cfg):
            assert H.pad_of(n_fft, hop) < t <= 3 * n_fft + 17
            rem.add(H.num_frames(t, n_fft, hop) % 4)
        assert H.num_frames(H.lengths(cfg)[0], n_fft, hop) >= 1
        # the long clip has frames of all three kinds; items 1 and 2 of an odd length start off 16-byte alignment
        t, pad = H.lengths(cfg)[-1], H.pad_of(n_fft, hop)
        starts = [f * hop - pad for f in range(H.num_frames(t, n_fft, hop))]
        assert t % 2 == 1 and starts[0] < 0 and starts[-1] + n_fft > t and any(0 <= s and s + n_fft <= t for s in starts)
    assert rem == {0, 1, 2, 3}
    assert any((n_fft - hop) % 2 for n_fft, hop, _ in H.CONFIGS)
    assert len(H.loss_cases()) == len(H.CONFIGS) * 3 * 2 * 2


def test_lens_sets_put_the_boundary_on_a_centre_tap():
    for cfg in H.CONFIGS:
        for t in H.lengths(cfg):
            frames = H.num_frames(t, cfg[0], cfg[1])
            k = frames // 2
            a, b = H.lens_sets(cfg, t)
            keep_a, keep_b = H.keep_mask(a, cfg, frames), H.keep_mask(b, cfg, frames)
            assert keep_a[0].all() and keep_b[2].all()
            assert keep_a[1].sum() == k and keep_b[0].sum() == k + 1      # lens == c_k drops frame k, c_k + 1 keeps it
            assert not keep_a[2].any() and not keep_b[1].any()            # lens 0 and 1


def test_four_filters_are_empty_at_n_fft_256_and_none_elsewhere():
    assert [int(H.mel_reference(cfg, n, f, H.lengths(cfg)[0])[3].sum()) for cfg, n, f in H.MEL_CASES] == [4, 0, 0, 0, 0, 0, 0]
    assert {n for _, n, _ in H.MEL_CASES} == {20, 80, 128}       # below and above the 64 lanes that walk the filters


# ------------------------------------------------------------------------------- argument check and frame count (no launch)

def _entry_points(t, n_fft, hop):
    lib = N.lib()
    return {
        "smt_stft_magnitude": lambda: lib.smt_stft_magnitude(DUMMY, DUMMY, DUMMY, DUMMY, 1, t, n_fft, hop, None),
        "smt_stft_loss_fwd": lambda: lib.smt_stft_loss_fwd(DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 1, t, n_fft, hop, None),
        "smt_stft_loss_bwd": lambda: lib.smt_stft_loss_bwd(DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 1, t, n_fft, hop,
                                                           DUMMY, 1 << 30, None),
        "smt_melspec": lambda: lib.smt_melspec(DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 1, t, n_fft, hop, 80, None),
    }


# -hop < t + 2 pad - n_fft < 0: C's truncating division counted one frame here, Python's floor division none -- the library
# launched a frame into outputs sized for zero.  (200, 512, 256) and (255, 512, 256) are that range at n_fft 512.
@pytest.mark.parametrize("t,n_fft,hop", [(257, 1024, 512), (511, 1024, 512), (200, 512, 256), (255, 512, 256)])
def test_signal_shorter_than_one_frame_is_an_error_at_every_entry_point(t, n_fft, hop):
    assert t > H.pad_of(n_fft, hop) and spectral.num_frames(t, n_fft, hop) <= 0
    assert N.lib().smt_stft_num_frames(t, n_fft, hop) == spectral.num_frames(t, n_fft, hop)
    assert N.lib().smt_stft_loss_bwd_workspace_bytes(3, t, n_fft, hop) == 0
    for name, call in _entry_points(t, n_fft, hop).items():
        assert call() == 1, name
        msg = N.lib().smt_last_error().decode()
        assert msg.startswith(name) and "signal shorter than one frame" in msg and f"t={t}" in msg, msg


@pytest.mark.parametrize("t,n_fft,hop", [(512, 1024, 512), (300, 512, 256), (256, 512, 256)])
def test_shortest_signal_of_one_frame_is_accepted(t, n_fft, hop):
    """t + 2 pad >= n_fft: exactly one frame, which the upstream conv computes too.  ((300, 512, 256): pad 128, 556 padded samples.)"""
    assert N.lib().smt_stft_num_frames(t, n_fft, hop) == spectral.num_frames(t, n_fft, hop) == 1
    assert N.lib().smt_stft_loss_bwd_workspace_bytes(3, t, n_fft, hop) == 3 * n_fft * 4
    # batch 0 passes the argument checks and returns before any launch
    lib = N.lib()
    assert lib.smt_stft_magnitude(DUMMY, DUMMY, DUMMY, DUMMY, 0, t, n_fft, hop, None) == 0
    assert lib.smt_stft_loss_fwd(DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 0, t, n_fft, hop, None) == 0
    assert lib.smt_stft_loss_bwd(DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 0, t, n_fft, hop, DUMMY, 0, None) == 0
    assert lib.smt_melspec(DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 0, t, n_fft, hop, 80, None) == 0


def test_signal_not_longer_than_the_reflect_padding_is_still_an_error():
    for name, call in _entry_points(256, 1024, 512).items():
        assert call() == 1, name
        assert "shorter than the reflect padding" in N.lib().smt_last_error().decode()


@pytest.mark.parametrize("n_fft,hop", [(c[0], c[1]) for c in H.CONFIGS] + [(1024, 512)])
def test_library_frame_count_floors_like_the_python_side(n_fft, hop):
    lib = N.lib()
    for t in range(0, n_fft + 3 * hop + 2):
        want = spectral.num_frames(t, n_fft, hop)
        assert want == H.num_frames(t, n_fft, hop) == (t + 2 * ((n_fft - hop) // 2) - n_fft) // hop + 1
        assert lib.smt_stft_num_frames(t, n_fft, hop) == want, (t, n_fft, hop)
        assert lib.smt_stft_loss_bwd_workspace_bytes(2, t, n_fft, hop) == 2 * max(want, 0) * n_fft * 4, (t, n_fft, hop)


@pytest.mark.parametrize("t", [257, 511, 300])
def test_python_guard_raises_the_library_error_before_sizing_outputs(t):
    """smt_amd.spectral checks the length before it allocates (num_frames can be negative): same RuntimeError, same text.
    t = 300 is shorter than the reflect padding of (2048, 240): the other message."""
    n_fft, hop, win = (1024, 512, 1024) if t != 300 else (2048, 240, 1200)
    x = torch.zeros(2, t)
    calls = {
        "smt_stft_magnitude": lambda: spectral.stft_magnitude(x, n_fft, hop, win),
        "smt_stft_loss_fwd": lambda: spectral.stft_loss(x, x.clone().requires_grad_(True), None, n_fft, hop, win, True),
        "smt_melspec": lambda: spectral.log_mel(x, None, None, n_fft, hop, win),
    }
    for name, call in calls.items():
        assert _entry_points(t, n_fft, hop)[name]() == 1
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == f"{name} failed (status 1): " + N.lib().smt_last_error().decode()
