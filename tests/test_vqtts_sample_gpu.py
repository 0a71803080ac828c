"""Sampling in the VQTTS code head on the device (smt_vqtts_code_head_sample, smt_amd.vqtts.code_head_sample,
CodePredictor.forward(sample=...), VQTTS.infer(temperature=...), scripts.synthesize --temperature) against the float64
restatement of tests/vqtts_sample_helpers.py.

Every comparison uses the derived bound of that file: on EVERY row the drawn bin must be possibly
kept and its float64 score must reach every surely kept bin's within e_s; n_kept must lie between the surely-kept and the
possibly-kept count.  Data: h ~ N(0, 1), W ~ 2 N(0, 1) / sqrt(C), a small bias.  The float64 logits and e_r of a case are
computed once and shared by its temperatures, truncations and layouts."""
import functools
import os
import wave

import numpy as np
import pytest
import torch

import vqtts_model_helpers as H
import vqtts_sample_helpers as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
TEMPERATURES, MIN_PS = (0.5, 1.0, 2.0), (0.0, 0.05, 0.2)


@functools.lru_cache(maxsize=None)
def _case(n, c, v, seed):
    """(h, w, b) on the device and the float64 logits and e_r of the case (numpy)."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, c, generator=g)
    w = 2.0 * torch.randn(v, c, generator=g) / c ** 0.5
    b = 0.1 * torch.randn(v, generator=g)
    h64, w64, b64 = (t.double().numpy() for t in (h, w, b))
    logits = h64 @ w64.T + b64
    return h.to(DEV), w.to(DEV), b.to(DEV), logits, S.row_bound(h64, w64, b64, logits)


def _seeds(batch, salt):
    """Distinct int32 seeds, negative ones among them."""
    g = torch.Generator().manual_seed(1000 + salt)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (batch,), generator=g, dtype=torch.int64).to(torch.int32)


def _draw(h, w, b, seeds, t_q, temperature, min_p, split=None):
    from smt_amd import vqtts
    pred, kept = vqtts.code_head_sample(h, w, b, seeds.to(DEV), t_q, temperature, min_p, split=split, want_kept=True)
    assert pred.dtype == torch.int32 and kept.dtype == torch.int32 and pred.shape == kept.shape == (h.shape[0],)
    return pred.cpu().numpy(), kept.cpu().numpy()


def _check_case(n, c, v, seed, t_qs):
    from smt_amd import vqtts
    h, w, b, logits, e_r = _case(n, c, v, seed)
    split = vqtts.WeightSplit()
    shares = []
    for t_q in t_qs:
        seeds = _seeds(n // t_q, seed + t_q)
        for temperature in TEMPERATURES:
            for min_p in MIN_PS:
                pred, kept = _draw(h, w, b, seeds, t_q, temperature, min_p, split)
                share = S.check_draw(pred, kept, logits, e_r, seeds.numpy(), t_q, temperature, min_p)
                shares.append(share)
                if min_p == 0.0:
                    assert bool((kept == v).all()), "without truncation every bin is kept"
                else:
                    assert kept.min() >= 1
    print(f"n={n} c={c} v={v}: rows pinned to one bin, min over {len(shares)} draws: {min(shares):.4%}")


@pytest.mark.parametrize("n,t_qs", [(1, (1,)), (31, (1, 31)), (32, (1, 4, 32)), (33, (1, 3, 11, 33)), (65, (1, 5, 13, 65)),
                                    (257, (1, 257))])
def test_rows(n, t_qs):
    _check_case(n, 128, 512, 200 + n, t_qs)


@pytest.mark.parametrize("c,v", [(c, v) for c in (16, 64, 256) for v in (32, 96, 1024)])
def test_widths(c, v):
    _check_case(257, c, v, c + v, (1, 257))


@pytest.mark.parametrize("c,v,min_p", [(128, 512, 0.05), (128, 512, 0.0), (16, 32, 0.2), (256, 1024, 0.1)])
def test_the_criterion_has_teeth(c, v, min_p):
    """At 4,096 rows the criterion leaves exactly one admissible bin on at least 99 % of the rows (a property the float64
    restatement alone has on such data: 99.6-99.98 % over these four cases), so passing it pins the draw."""
    n, t_q = 4096, 512
    h, w, b, logits, e_r = _case(n, c, v, 7)
    seeds = _seeds(n // t_q, 7)
    pred, kept = _draw(h, w, b, seeds, t_q, 1.0, min_p)
    share = S.check_draw(pred, kept, logits, e_r, seeds.numpy(), t_q, 1.0, min_p)
    agree = float((pred == S.draw64(logits, seeds.numpy(), t_q, 1.0, min_p)["pred"]).mean())
    print(f"c={c} v={v} min_p={min_p}: pinned rows {share:.4%}, rows equal to the float64 draw {agree:.4%}")
    assert share >= 0.99


# ---- exact checks -----------------------------------------------------------------------------------------------------
def test_min_p_one_keeps_the_maxima_alone():
    """cut = 0: only the bins whose logit EQUALS the row maximum are kept.  With a unique maximum the draw is the argmax,
    bit-identical to ``code_head_predict``.  With duplicated weight rows planted as the maximum both copies tie exactly (one
    instruction sequence for every column), both are kept, n_kept is exactly 2, and the copy with the higher score -- equal
    logits, so the higher noise -- wins: the winner is decided through the scores, as the contract says, and follows the
    float64 noise wherever the two noises differ by more than their bound."""
    from smt_amd import vqtts
    n, c, v, t_q = 257, 128, 512, 257
    h, w, b, logits, e_r = _case(n, c, v, 457)
    seeds = _seeds(1, 3)
    for temperature in TEMPERATURES:
        pred, kept = _draw(h, w, b, seeds, t_q, temperature, 1.0)
        assert kept.min() >= 1
        assert np.array_equal(pred, vqtts.code_head_predict(h, w, b).cpu().numpy())
        assert bool((kept == 1).all())                       # no exact ties among continuous random logits
    g = S.gumbel(S.row_keys(seeds.numpy(), t_q), v)
    for lo, hi in ((3, 4), (4, 8), (37, 300), (0, 511)):    # same registers / across lane halves / across staged tiles
        w2, b2 = w.clone(), b.clone()
        w2[hi] = w2[lo]
        b2[lo] = b2[hi] = 30.0
        pred, kept = _draw(h, w2, b2, seeds, t_q, 1.0, 1.0)
        assert bool((kept == 2).all()) and bool(np.isin(pred, (lo, hi)).all())
        assert bool((vqtts.code_head_predict(h, w2, b2) == lo).all())
        clear = np.abs(g[:, lo] - g[:, hi]) > S.E_G * (2 + np.abs(g[:, lo]) + np.abs(g[:, hi])) + 2.0 ** -22 * (30.0 + 40.0)
        want = np.where(g[:, lo] >= g[:, hi], lo, hi)
        assert clear.mean() > 0.99 and np.array_equal(pred[clear], want[clear])
        assert (pred == lo).any() and (pred == hi).any()


def test_equal_inputs_give_equal_bits():
    h, w, b, _, _ = _case(257, 128, 512, 457)
    seeds = _seeds(1, 5)
    for min_p in (0.0, 0.05):
        a, ka = _draw(h, w, b, seeds, 257, 1.0, min_p)
        c, kc = _draw(h, w, b, seeds, 257, 1.0, min_p)
        assert np.array_equal(a, c) and np.array_equal(ka, kc)


@pytest.mark.parametrize("min_p", [0.0, 0.05])
def test_rows_past_the_end_are_not_written_and_n_kept_may_be_null(min_p):
    from smt_amd import native as N
    from smt_amd import vqtts
    n, c, v, t_q = 33, 128, 512, 11
    h, w, b, logits, e_r = _case(n, c, v, 233)
    seeds = _seeds(n // t_q, 9).to(DEV)
    ws = vqtts.WeightSplit().get(w)
    inv_t, cut = vqtts.sample_cut(1.0, min_p)
    pad = 300                                                  # past the workgroup's 128 rows
    pred = torch.full((n + pad,), -7, dtype=torch.int32, device=DEV)
    kept = torch.full((n + pad,), -9, dtype=torch.int32, device=DEV)
    N.check(N.lib().smt_vqtts_code_head_sample(N.ptr(h), N.ptr(ws), ws.numel(), N.ptr(b), N.ptr(seeds), n, t_q, c, v, inv_t, cut,
                                               N.ptr(pred), N.ptr(kept), N.stream_ptr()), "sample")
    assert bool((pred[n:] == -7).all()) and bool((kept[n:] == -9).all())
    want, want_kept = _draw(h, w, b, seeds, t_q, 1.0, min_p)
    assert np.array_equal(pred[:n].cpu().numpy(), want) and np.array_equal(kept[:n].cpu().numpy(), want_kept)
    # NULL n_kept, a NaN-patterned pred
    pred2 = torch.full((n + pad,), 0x7FC00000, dtype=torch.int32, device=DEV)
    N.check(N.lib().smt_vqtts_code_head_sample(N.ptr(h), N.ptr(ws), ws.numel(), N.ptr(b), N.ptr(seeds), n, t_q, c, v, inv_t, cut,
                                               N.ptr(pred2), None, N.stream_ptr()), "sample")
    assert np.array_equal(pred2[:n].cpu().numpy(), want) and bool((pred2[n:] == 0x7FC00000).all())
    # no rows: nothing is launched
    empty = vqtts.code_head_sample(h[:0], w, b, seeds[:0], t_q, 1.0, min_p)
    assert empty.shape == (0,) and empty.dtype == torch.int32


@pytest.mark.parametrize("min_p", [0.0, 0.05])
def test_a_draw_depends_on_seed_frame_and_bin_alone(min_p):
    """The same h rows with the same seed at another batch position, under a larger t_q and in another workgroup and lane
    draw the same codes; other seeds draw other codes on most rows."""
    h, w, b, _, _ = _case(257, 128, 512, 457)
    seeds = _seeds(2, 11)
    t_a, t_b = 33, 50
    a, ka = _draw(h[:2 * t_a], w, b, seeds, t_a, 1.0, min_p)
    # three items of 50 frames: item 2 starts with item 0's frames, item 0 with item 1's; the rest are other rows
    rows = torch.cat([h[t_a:2 * t_a], h[100:117], h[120:170], h[:t_a], h[170:187]])
    seeds_b = torch.stack([seeds[1], torch.tensor(12345, dtype=torch.int32), seeds[0]])
    c, kc = _draw(rows, w, b, seeds_b, t_b, 1.0, min_p)
    assert np.array_equal(c[2 * t_b:2 * t_b + t_a], a[:t_a]) and np.array_equal(kc[2 * t_b:2 * t_b + t_a], ka[:t_a])
    assert np.array_equal(c[:t_a], a[t_a:]) and np.array_equal(kc[:t_a], ka[t_a:])
    other, _ = _draw(h[:2 * t_a], w, b, _seeds(2, 12), t_a, 1.0, min_p)
    assert (other != a).mean() > 0.5
    swapped, _ = _draw(h[:2 * t_a], w, b, seeds.flip(0), t_a, 1.0, min_p)
    assert (swapped != a).mean() > 0.5


# ---- distribution -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature,min_p", [(1.0, 0.0), (0.7, 0.0), (1.0, 0.2)])
def test_distribution(temperature, min_p):
    """65,536 identical rows (C = 16, V = 32; four items with distinct seeds): the counts against softmax64(l / T), with
    min_p against the renormalised kept set at its own degrees of freedom; nothing outside the kept set is ever drawn.  The
    row's logits are ~ 1.5 N(0, 1) (W scaled by 1.5 / |h|); the data seed is one at which the chi-square law applies in all
    three cases -- every bin expects at least 5 draws, and min_p = 0.2 keeps several bins -- which is asserted below."""
    n, c, v, t_q = 65536, 16, 32, 16384
    g = torch.Generator().manual_seed(10)
    h1 = torch.randn(c, generator=g)
    w = 1.5 * torch.randn(v, c, generator=g) / float(h1.norm())
    b = 0.1 * torch.randn(v, generator=g)
    l = w.double().numpy() @ h1.double().numpy() + b.double().numpy()
    seeds = torch.tensor([11, -12, 2 ** 31 - 1, 0], dtype=torch.int32)
    pred, kept = _draw(h1.expand(n, c).contiguous().to(DEV), w.to(DEV), b.to(DEV), seeds, t_q, temperature, min_p)
    inv_t, cut = S.device_scalars(temperature, min_p)
    e_r = S.row_bound(h1.double().numpy()[None], w.double().numpy(), b.double().numpy(), l[None])[0]
    in_set = l >= l.max() + cut
    assert not (np.abs(l - (l.max() + cut)) <= 2 * e_r).any(), "a bin sits on the threshold: choose other data"
    assert bool((kept == in_set.sum()).all())
    counts = np.bincount(pred, minlength=v)
    assert not counts[~in_set].any(), "a bin outside the kept set was drawn"
    p = np.where(in_set, np.exp((l - l.max()) * inv_t), 0.0)
    chi = S.chi_square(counts, p / p.sum())
    dof = int(in_set.sum()) - 1
    assert (dof == v - 1 if min_p == 0 else 3 <= dof < v - 1) and (n * p / p.sum())[in_set].min() >= 5.0
    print(f"T={temperature} min_p={min_p}: chi-square {chi:.2f} at {dof} degrees of freedom (limit {S.CHI2_999[dof]})")
    assert chi < S.CHI2_999[dof]


# ---- upper layers -----------------------------------------------------------------------------------------------------
def _model(seed=0):
    """The model of tests/test_vqtts_model_gpu.py: seeded parameters (zero-initialised tensors included), a random codebook."""
    from models.vqtts import VQTTS
    from utils import config as C
    torch.manual_seed(seed)
    model = VQTTS(C.create(H.config_dict())).to(DEV)
    H.randomize_zero_init(model)
    model.text_encoder.pre.p_dropout = 0.0
    blk = model.quant_bottleneck
    blk.k.copy_(0.5 * torch.randn(blk.k.shape, generator=torch.Generator().manual_seed(seed + 1)))
    blk.restore_k(threshold=blk.threshold)
    return model.eval()


def _front(model, x, lens):
    """VQTTS.infer up to the predictor: (x_dev, x_enc, idx, z_lens)."""
    from smt_amd import glow
    valid = torch.arange(x.shape[1])[None, :] < lens[:, None]
    x_dev = torch.where(valid, x, 0).to(DEV)
    x_enc, _, logw, lens32 = model.text_encoder(x_dev, lens.to(DEV))
    _, z_lens, cum = glow.durations(logw, lens32, 1.0, 1)
    idx = glow.duration_index(cum, lens32, z_lens, int(z_lens.max()))
    return x_dev, x_enc, idx, z_lens


def test_predictor_forward_samples_through_the_op():
    from smt_amd import vqtts
    model = _model()
    x, x_lens, _, _ = H.batch()
    with torch.no_grad():
        _, x_enc, idx, z_lens = _front(model, x, x_lens)
        seeds = torch.tensor([4, 5, 6], dtype=torch.int32, device=DEV)
        for temperature, min_p in ((1.0, 0.0), (0.7, 0.1)):
            pred = model.predictor(x_enc, idx, z_lens, sample=(temperature, min_p, seeds))
            hid, _ = model.predictor.hidden(x_enc, idx, z_lens)
            want = vqtts.code_head_sample(hid, model.quant_proj.weight, model.quant_proj.bias, seeds, hid.shape[1], temperature, min_p)
            assert pred.shape == idx.shape and pred.dtype == torch.int32 and torch.equal(pred.reshape(-1), want)
        greedy = model.predictor(x_enc, idx, z_lens)
        assert torch.equal(model.predictor(x_enc, idx, z_lens, sample=None), greedy)
        assert not torch.equal(pred, greedy)
        with pytest.raises(ValueError, match="target"):
            model.predictor(x_enc, idx, z_lens, target=greedy.long(), sample=(1.0, 0.0, seeds))


def test_infer_samples():
    from smt_amd import vqtts
    model = _model()
    x, x_lens, _, _ = H.batch()
    greedy, lengths = model.infer(x, x_lens)
    same, same_lengths = model.infer(x, x_lens, temperature=0.0)
    assert torch.equal(same, greedy) and torch.equal(same_lengths, lengths)                # temperature 0 is today's path
    wave1, l1 = model.infer(x, x_lens, temperature=1.0, seed=5)
    wave2, l2 = model.infer(x, x_lens, temperature=1.0, seed=5)
    assert torch.equal(wave1, wave2) and torch.equal(l1, lengths) and torch.equal(l2, lengths)
    assert wave1.shape == greedy.shape and wave1.dtype == torch.float32
    other, _ = model.infer(x, x_lens, temperature=1.0, seed=6)
    assert not torch.equal(other, wave1) and not torch.equal(wave1, greedy)
    assert torch.equal(model.infer(x, x_lens, temperature=1.0, seed=[5, 6, 7])[0], wave1)  # an int seed is seed + b per item
    assert torch.equal(model.infer(x, x_lens, temperature=1.0, seed=2 ** 31 + 5)[0], wave1)  # ... mod 2^31
    for b, n in enumerate(lengths.tolist()):
        assert bool((wave1[b, n:] == 0).all()) and bool(wave1[b, :n].any())
    # the waveform is emit_codes -> decoder on the sampled pred, unchanged
    with torch.no_grad():
        x_dev, x_enc, idx, z_lens = _front(model, x, x_lens)
        seeds = torch.tensor([5, 6, 7], dtype=torch.int32, device=DEV)
        for min_p, got in ((0.0, wave1), (0.3, model.infer(x, x_lens, temperature=1.0, min_p=0.3, seed=5)[0])):
            pred = model.predictor(x_enc, idx, z_lens, sample=(1.0, min_p, seeds))
            y_d, _ = vqtts.emit_codes(pred, x_dev, idx, z_lens, model.quant_bottleneck.k, model.n_vocab, model.l_bins)
            want, _ = model.audio_decoder(y_d, z_lens)
            keep = torch.arange(want.shape[1], device=DEV)[None, :] < lengths[:, None]
            assert torch.equal(got, torch.where(keep, want.float(), 0.0))
    with pytest.raises(ValueError, match="needs seed"):
        model.infer(x, x_lens, temperature=1.0)


def test_synthesize_with_a_temperature(tmp_path):
    from scripts import synthesize
    from utils import config as C
    model = _model()
    log_dir = tmp_path / "run"
    os.makedirs(log_dir / "ckpts")
    C.save(C.create({**H.config_dict(), "train": {"n_gpus": 1, "ema": False, "batch_size": 2}}), str(log_dir / "config.yaml"))
    torch.save({"model": model.state_dict()}, str(log_dir / "ckpts" / "ckpt.1.pt"))
    utterances = ([5, 1, 0, 9, 3, 11], [7, 7, 1], [2, 4, 6, 8])
    tokens = tmp_path / "utterances.txt"
    tokens.write_text("\n".join(" ".join(map(str, u)) for u in utterances) + "\n")
    common = ["--log_dir", str(log_dir), "--ckpt_num", "1", "--tokens", str(tokens), "--batch_size", "1", "--temperature", "1",
              "--seed", "3"]
    first = synthesize.main(common + ["--dump_dir", str(tmp_path / "a")])
    second = synthesize.main(common + ["--dump_dir", str(tmp_path / "b")])
    plain = synthesize.main(common[:-4] + ["--dump_dir", str(tmp_path / "c")])
    differs = False
    for i, ids in enumerate(utterances):
        raw = [open(os.path.join(d, f"wav_{i}.wav"), "rb").read() for d in (first, second, plain)]
        assert raw[0] == raw[1]                                                          # repeats bit for bit
        differs |= raw[0] != raw[2]
        wav, lengths = model.infer(torch.tensor([ids]), temperature=1.0, seed=[3 + i])   # utterance i draws with seed + i
        with wave.open(os.path.join(first, f"wav_{i}.wav"), "rb") as f:
            assert f.getnframes() == int(lengths[0])
            pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
        assert np.array_equal(pcm, (np.clip(wav[0].double().cpu().numpy(), -1.0, 1.0) * 32767.0).astype("<i2"))
    assert differs, "the sampled waveforms equal the argmax ones"
    with pytest.raises(ValueError, match="--min_p"):
        synthesize.main(common[:-4] + ["--min_p", "0.1", "--dump_dir", str(tmp_path / "d")])


def test_glow_tts_refuses_the_code_flags(tmp_path):
    """GlowTTS emits no codes: ``--temperature`` / ``--min_p`` are refused for it, as VQTTS refuses ``--noise_scale``."""
    from oracle import glow_oracle as go
    from scripts import synthesize
    from utils import config as C
    from utils.commons import get_model
    cfg = C.create({"model": dict(_import_="models.glow_tts.glow_tts.GlowTTS", n_speakers=1, gin_channels=0,
                                  encoder=dict(go.GOLDEN_CFG["encoder"]), decoder=dict(go.GOLDEN_CFG["decoder"])),
                    "dataset": dict(n_mels=8, intersperse_blanks=False, cmudict_path=""), "train": dict(n_gpus=1, ema=False)})
    log_dir = tmp_path / "run"
    (log_dir / "ckpts").mkdir(parents=True)
    C.save(cfg, str(log_dir / "config.yaml"))
    model, _ = get_model(cfg, DEV)
    torch.save({"model": {k: v.cpu() for k, v in model.state_dict().items()}}, str(log_dir / "ckpts" / "ckpt.1.pt"))
    (tmp_path / "tokens.txt").write_text("1 2 3\n")
    common = ["--log_dir", str(log_dir), "--ckpt_num", "1", "--tokens", str(tmp_path / "tokens.txt"), "--dump_dir", str(tmp_path / "out")]
    with pytest.raises(ValueError, match="GlowTTS has no codes"):
        synthesize.main(common + ["--temperature", "1"])
    with pytest.raises(ValueError, match="GlowTTS has no codes"):
        synthesize.main(common + ["--temperature", "0.5", "--min_p", "0.1", "--seed", "2"])
