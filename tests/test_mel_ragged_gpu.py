"""smt_melspec_ragged (csrc/spectral.hip) behind smt_amd.spectral.log_mel_ragged and datasets.transforms.BatchLogMel: the log-mels
of a zero-padded ragged batch in one launch, every clip transformed alone.

Per configuration ONE batch of length T = 3 n_fft + 17 (odd: item bases are not 16-byte aligned) holds the clip lengths
  T, pad + 1 (the shortest clip with a frame: every frame reflects on both sides), n_fft + hop + 3, 0, pad (too short: all fill)
and further lengths so that the frame counts F_b take all four remainders mod 4 (four frames share a workgroup).  NaN stands
past every length and the output is prefilled with garbage.  Asserted:
  * valid columns bit-equal to spectral.log_mel on the truncated clip (a frame inside the buffer that crosses the clip's end
    must reflect about the clip's end: judging "interior" against T instead fails here -- DESIGN.md section 18);
  * valid columns within bound_mel(E32) of the float64 reference of tests/spectral_ref_helpers.py on the truncated clip;
  * every other column exactly the fill, no NaN anywhere, spect_len = F_b, two calls bit-equal.
The references are computed once per configuration and shared."""
import functools
import math

import numpy as np
import pytest
import torch

import spectral_ref_helpers as H

pytestmark = pytest.mark.gpu

CASES = [((1024, 256, 1024), 80), ((512, 50, 240), 80), ((256, 64, 256), 20)]
F_MAX = 8000.0
FILL = float(np.float32(math.log(1e-7)))


def clip_frames(length, n_fft, hop):
    pad = H.pad_of(n_fft, hop)
    return H.num_frames(length, n_fft, hop) if length > pad and length + 2 * pad >= n_fft else 0


def case_lengths(cfg):
    n_fft, hop, _ = cfg
    pad, t = H.pad_of(n_fft, hop), 3 * n_fft + 17
    lens = [t, pad + 1, n_fft + hop + 3, 0, pad]
    for r in range(4):                      # the smallest clip above one frame whose frame count has the missing remainder
        if r not in {clip_frames(n, n_fft, hop) % 4 for n in lens if clip_frames(n, n_fft, hop) > 0}:
            lens.append(next(n for n in range(n_fft + 1, t) if clip_frames(n, n_fft, hop) % 4 == r))
    return t, lens


@functools.lru_cache(maxsize=None)
def run_case(index):
    from oracle import vqvae_oracle as orc
    from smt_amd import spectral
    cfg, n_mels = CASES[index]
    n_fft, hop, win = cfg
    t, lens = case_lengths(cfg)
    module = H.mel_module(cfg, n_mels, F_MAX)
    basis, band = module.mel_basis.cuda(), module.band.cuda()
    x = H.make_signals(cfg, t, batch=len(lens))[0].clone()
    for b, n in enumerate(lens):
        x[b, n:] = float("nan")
    xd = x.cuda()
    lens_cpu = torch.tensor(lens, dtype=torch.int64)
    # garbage where the output will be allocated: the caching allocator hands the freed block back
    junk = torch.full((len(lens), n_mels, clip_frames(t, n_fft, hop)), float("nan"), device="cuda")
    del junk
    mel_a, frames_a = spectral.log_mel_ragged(xd, lens_cpu, basis, band, n_fft, hop, win, FILL)
    mel_b, _ = spectral.log_mel_ragged(xd, lens_cpu, basis, band, n_fft, hop, win, FILL)
    alone, ref64, e32 = {}, {}, {}
    for b, n in enumerate(lens):
        if clip_frames(n, n_fft, hop) > 0:
            clip = x[b:b + 1, :n].contiguous()
            alone[b] = spectral.log_mel(clip.cuda(), basis, band, n_fft, hop, win).cpu()
            ref64[b] = H.log_mel64(clip, cfg, module.mel_basis.cpu())["mel"]
            e32[b] = H.max_abs(orc.mel_spectrogram(clip, module.mel_basis.cpu(), *cfg), ref64[b])
    return dict(cfg=cfg, n_mels=n_mels, t=t, lens=lens, mel=mel_a.cpu(), mel_again=mel_b.cpu(), frames=frames_a,
                alone=alone, ref64=ref64, e32=e32)


def test_case_lengths_cover_every_remainder_and_edge():
    for cfg, _ in CASES:
        n_fft, hop, _ = cfg
        t, lens = case_lengths(cfg)
        pad = H.pad_of(n_fft, hop)
        assert t % 4 == 1 and lens[:5] == [t, pad + 1, n_fft + hop + 3, 0, pad]
        frames = [clip_frames(n, n_fft, hop) for n in lens]
        assert frames[3] == 0 and frames[4] == 0 and frames[1] >= 1
        assert {f % 4 for f in frames if f > 0} == {0, 1, 2, 3}, (cfg, frames)
        # at least one clip ends inside the buffer with a frame that lies inside the buffer but crosses the clip's end
        assert any(0 < n < t and (clip_frames(n, n_fft, hop) - 1) * hop - pad + n_fft > n
                   and (clip_frames(n, n_fft, hop) - 1) * hop - pad + n_fft <= t for n in lens), cfg


@pytest.mark.parametrize("index", range(len(CASES)))
def test_valid_columns_bit_equal_log_mel_on_the_truncated_clip(index):
    r = run_case(index)
    assert r["alone"]
    for b, alone in r["alone"].items():
        f = alone.shape[-1]
        assert f == clip_frames(r["lens"][b], r["cfg"][0], r["cfg"][1])
        got = r["mel"][b, :, :f]
        diff = int((got.view(torch.int32) != alone[0].view(torch.int32)).sum())
        print(f"{r['cfg']} item {b} len {r['lens'][b]} frames {f}: {diff} elements differ in bits, "
              f"max abs diff {float((got - alone[0]).abs().max()):.3g}")
        assert diff == 0, (r["cfg"], b, r["lens"][b], diff)


@pytest.mark.parametrize("index", range(len(CASES)))
def test_valid_columns_within_the_float64_bound(index):
    r = run_case(index)
    for b, ref in r["ref64"].items():
        f = ref.shape[-1]
        err = H.max_abs(r["mel"][b:b + 1, :, :f], ref)
        print(f"{r['cfg']} item {b} len {r['lens'][b]} frames {f}: err {err:.3g} E32 {r['e32'][b]:.3g}")
        assert err <= H.bound_mel(r["e32"][b]), (r["cfg"], b, err, r["e32"][b])


@pytest.mark.parametrize("index", range(len(CASES)))
def test_fill_lengths_no_nan_and_reproducible(index):
    r = run_case(index)
    n_fft, hop, _ = r["cfg"]
    frames = [clip_frames(n, n_fft, hop) for n in r["lens"]]
    assert r["frames"].dtype == torch.int64 and r["frames"].tolist() == frames
    assert r["mel"].shape == (len(frames), r["n_mels"], max(frames))
    assert not torch.isnan(r["mel"]).any()
    fill_bits = torch.tensor(FILL, dtype=torch.float32).view(torch.int32)
    for b, f in enumerate(frames):
        assert (r["mel"][b, :, f:].contiguous().view(torch.int32) == fill_bits).all(), (r["cfg"], b)
    assert torch.equal(r["mel"].view(torch.int32), r["mel_again"].view(torch.int32))


def test_dataset_shaped_batch_and_device_clamp():
    """[4096, 1536, 512] samples at (1024, 256): BatchLogMel against the per-clip MelSpectrogram; then the C entry with a device
    length LARGER than T for item 0: the kernel clamps it, same result."""
    from datasets.transforms import BatchLogMel, MelSpectrogram
    from smt_amd import native as N
    from smt_amd import spectral
    t, lens = 4096, [4096, 1536, 512]
    kw = dict(sample_rate=H.SAMPLE_RATE, n_fft=1024, win_length=1024, hop_length=256, n_mels=80, f_min=0.0, f_max=F_MAX)
    batch_mel, mel = BatchLogMel(**kw).cuda(), MelSpectrogram(**kw).cuda()
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(3, 1, t, generator=g) * 2 - 1) * 0.5
    for b, n in enumerate(lens):
        x[b, :, n:] = 0.0                                  # what collate leaves there
    xd = x.cuda()
    spect, spect_len = batch_mel(xd, torch.tensor(lens))
    assert spect_len.tolist() == [16, 6, 2] and spect.shape == (3, 80, 16)
    for b, n in enumerate(lens):
        alone = mel(xd[b, :, :n].contiguous())
        assert torch.equal(spect[b, :, :spect_len[b]], alone[0]), b
        assert (spect[b, :, spect_len[b]:] == BatchLogMel.FILL).all()
    # the padded-batch transform differs at the item ends (the hole this kernel closes): item 1's last frame
    padded = mel(xd[:, 0])
    assert not torch.equal(padded[1, :, 5], spect[1, :, 5])
    out = torch.full_like(spect, float("nan"))
    window, tw = spectral._get_tables(1024, 1024, xd.device)
    dev_lens = torch.tensor([t + 904, 1536, 512], dtype=torch.int32).cuda()
    N.check(N.lib().smt_melspec_ragged(N.ptr(xd.reshape(3, t)), N.ptr(dev_lens), N.ptr(window), N.ptr(tw), N.ptr(batch_mel.mel_basis),
                                       N.ptr(batch_mel.band), N.ptr(out), 3, t, 1024, 256, 80, 16, BatchLogMel.FILL,
                                       N.stream_ptr()), "smt_melspec_ragged")
    assert torch.equal(out, spect)
