"""Incremental decoding of the TransformerLM (csrc/lm_decode.hip, TransformerLM.sample(causal=True) / step_logits) against the
float64 oracle (oracle/lm_oracle.py, causal=True): the four kernels alone, teacher-forced logits of the small and the shipped
configuration, and whole sampling runs.  Every tolerance is stated where it is asserted."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import lm_oracle as lmo
from test_lm_gpu import DEV, PKG, SMALL, _build, _lm_config, _vqvae_run

pytestmark = pytest.mark.gpu

# csrc/lm_decode.hip: eight lanes share a cache row and a wave loads 8 rows per instruction, 32 per pass; the four waves of a
# workgroup cover 128 rows per pass and a workgroup owns 256 rows -> boundaries at 8, 32, 128, 256 and 512 inside L_MAX
L_MAX = 600
POSITIONS = sorted({0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 7, 8, 9, 127, 128, 129, 383, 384, 385, 511, 512, 513, L_MAX - 1})


# ------------------------------------------------------------------------------------------------ 1. attention over the cache
@pytest.mark.parametrize("b,h", [(1, 1), (3, 2), (4, 16)])
def test_decode_attention_over_the_cache_matches_float64(b, h):
    """softmax(q K^T / sqrt(32)) V over rows 0..pos in float64, atol 3e-5 (test_attention_edge_shapes' bound for the same
    arithmetic); cache row pos = the step's k / v bit for bit, earlier rows untouched, later rows (NaN) never read; by-value
    and device-resident positions and two runs give the same bits."""
    from smt_amd import lm as K
    g = torch.Generator().manual_seed(17 * b + h)
    k_all, v_all = torch.randn(b, h, L_MAX, 32, generator=g), torch.randn(b, h, L_MAX, 32, generator=g)
    ws = K.decode_attention_workspace(b, h, L_MAX, DEV)
    assert ws is not None                                              # L_MAX spans three workgroup chunks
    for pos in POSITIONS:
        qkv = torch.randn(b, 3 * h * 32, generator=g)
        q, kn, vn = (t.reshape(b, h, 32) for t in qkv.split(h * 32, dim=-1))
        kc, vc = k_all.clone(), v_all.clone()
        kc[:, :, pos], vc[:, :, pos] = 7.0, -7.0                       # stale values the call must replace
        kc[:, :, pos + 1:], vc[:, :, pos + 1:] = float("nan"), float("nan")
        kd, vd = kc.to(DEV), vc.to(DEV)
        ctx = torch.full((b, h * 32), float("nan"), device=DEV)
        K.decode_attention(qkv.to(DEV), kd, vd, ctx, ws, pos=pos)
        k64 = torch.cat([k_all[:, :, :pos], kn[:, :, None]], dim=2).double()
        v64 = torch.cat([v_all[:, :, :pos], vn[:, :, None]], dim=2).double()
        w64 = F.softmax(torch.einsum("bhc,bhjc->bhj", q.double(), k64) / math.sqrt(32.0), dim=-1)
        want = torch.einsum("bhj,bhjc->bhc", w64, v64).reshape(b, h * 32)
        got = ctx.cpu()
        assert torch.isfinite(got).all(), pos
        err = float((got.double() - want).abs().max())
        assert err <= 3e-5, (pos, err)
        assert torch.equal(kd[:, :, pos].cpu(), kn) and torch.equal(vd[:, :, pos].cpu(), vn), pos
        assert torch.equal(kd[:, :, :pos].cpu(), k_all[:, :, :pos]) and torch.equal(vd[:, :, :pos].cpu(), v_all[:, :, :pos]), pos
        assert torch.isnan(kd[:, :, pos + 1:]).all() and torch.isnan(vd[:, :, pos + 1:]).all(), pos
        again = torch.full_like(ctx, float("nan"))
        K.decode_attention(qkv.to(DEV), kd, vd, again, ws, pos=0, pos_dev=torch.tensor([pos], dtype=torch.int32, device=DEV))
        assert torch.equal(again, ctx), pos


def test_decode_attention_single_chunk_cache_and_bad_position():
    """A cache of at most 256 rows needs no workspace and no merge launch; a by-value position outside the cache is refused."""
    from smt_amd import lm as K
    g = torch.Generator().manual_seed(3)
    assert K.decode_attention_workspace(2, 2, 256, DEV) is None
    kc, vc = torch.randn(2, 2, 256, 32, generator=g), torch.randn(2, 2, 256, 32, generator=g)
    for pos in (0, 200, 255):
        qkv = torch.randn(2, 3 * 64, generator=g)
        q, kn, vn = (t.reshape(2, 2, 32) for t in qkv.split(64, dim=-1))
        kd, vd = kc.to(DEV), vc.to(DEV)
        kd[:, :, pos + 1:], vd[:, :, pos + 1:] = float("nan"), float("nan")
        ctx = torch.empty(2, 64, device=DEV)
        K.decode_attention(qkv.to(DEV), kd, vd, ctx, None, pos=pos)
        k64 = torch.cat([kc[:, :, :pos], kn[:, :, None]], dim=2).double()
        v64 = torch.cat([vc[:, :, :pos], vn[:, :, None]], dim=2).double()
        w64 = F.softmax(torch.einsum("bhc,bhjc->bhj", q.double(), k64) / math.sqrt(32.0), dim=-1)
        want = torch.einsum("bhj,bhjc->bhc", w64, v64).reshape(2, 64)
        assert float((ctx.cpu().double() - want).abs().max()) <= 3e-5, pos
    with pytest.raises(RuntimeError, match="outside the cache"):
        K.decode_attention(qkv.to(DEV), kd, vd, ctx, None, pos=256)


# ------------------------------------------------------------------------------------------------ 2. skinny linear
# (4160, 8): a contraction longer than one launch covers (2048) -- the accumulate path
SHAPES = [(512, 1536), (512, 512), (512, 2048), (2048, 512), (512, 1024), (64, 16), (128, 64), (64, 1), (64, 37), (4160, 8)]


@pytest.mark.parametrize("k,n", SHAPES)
@pytest.mark.parametrize("b", [1, 4, 5, 32])
def test_decode_linear_matches_float64(b, k, n):
    """|error| <= K 2^-23 max|x| max|W| (the forward-error bound of an fp32 dot product of length K) and relative L2 < 1e-5."""
    from smt_amd import lm as K
    g = torch.Generator().manual_seed(1000 * b + k + n)
    x, w, bias = torch.randn(b, k, generator=g), torch.randn(n, k, generator=g) * k ** -0.5, torch.randn(n, generator=g)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    bound = k * 2.0 ** -23 * float(x.abs().max()) * float(w.abs().max())
    for with_bias in (False, True):
        for relu in (False, True):
            want = x.double() @ w.double().t() + (bias.double() if with_bias else 0.0)
            want = F.relu(want) if relu else want
            got = K.decode_linear(xd, wd, bd if with_bias else None, relu=relu).cpu().double()
            err, rel = float((got - want).abs().max()), float((got - want).norm() / want.norm().clamp_min(1e-30))
            assert err <= bound and rel < 1e-5, (with_bias, relu, err, bound, rel)
    out = torch.empty(b, n, device=DEV)
    assert K.decode_linear(xd, wd, bd, out=out) is out and torch.equal(out, K.decode_linear(xd, wd, bd))     # same bits every run


def test_decode_linear_rejects_bad_shapes():
    from smt_amd import lm as K
    with pytest.raises(RuntimeError, match="multiple of 64"):
        K.decode_linear(torch.randn(2, 96, device=DEV), torch.randn(8, 96, device=DEV))
    with pytest.raises(RuntimeError, match="batch must be 1..32"):
        K.decode_linear(torch.randn(33, 64, device=DEV), torch.randn(8, 64, device=DEV))


# ------------------------------------------------------------------------------------------------ 3. sampler
def _cdf_ok(logits64, sigma, u, k, tau):
    """c = cumsum(softmax(l / sigma)) in float64: c[k - 1] - tau <= u <= c[k] + tau, c[-1] = 0; per row -> bool tensor."""
    c = torch.cumsum(F.softmax(logits64 / sigma, dim=-1), dim=-1)
    c = torch.cat([torch.zeros_like(c[..., :1]), c], dim=-1)
    lo, hi = c.gather(-1, k[..., None])[..., 0], c.gather(-1, k[..., None] + 1)[..., 0]
    return (lo - tau <= u) & (u <= hi + tau)


@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("b", [1, 32])
@pytest.mark.parametrize("v", [16, 256, 512, 1024])
def test_decode_sample_draws_the_inverse_cdf(v, b, sigma):
    """tau = V 2^-23, the bound on an fp32 sum of V non-negative terms; every row of every case must satisfy it."""
    from smt_amd import lm as K
    g = torch.Generator().manual_seed(v + b)
    n = 8
    u = torch.rand(n, b, generator=g)
    u[n - 2], u[n - 1] = 0.0, 1.0 - 2.0 ** -24
    cases = {"unit": torch.randn(b, v, generator=g), "wide": torch.randn(b, v, generator=g) * 30.0, "tie": torch.randn(b, v, generator=g)}
    cases["tie"][0, 3] = cases["tie"][0, v - 2] = float(cases["tie"][0].max()) + 1.0      # two equal maxima in one row
    for name, logits in cases.items():
        tokens = torch.full((b, n + 1), -1, dtype=torch.int64, device=DEV)
        codes = torch.full((b, n), -1, dtype=torch.int64, device=DEV)
        ld, ud = logits.to(DEV), u.to(DEV)
        for pos in range(n):
            K.decode_sample(ld, ud, tokens, codes, sigma, pos=pos)
        k = codes.cpu()
        assert int(k.min()) >= 0 and int(k.max()) < v, name
        assert torch.equal(tokens[:, 1:].cpu(), k + 2) and bool((tokens[:, 0] == -1).all()), name
        ok = _cdf_ok(logits.double()[None].expand(n, b, v), sigma, u.double(), k.t(), v * 2.0 ** -23)
        assert bool(ok.all()), (name, ok.logical_not().nonzero().tolist())


# ------------------------------------------------------------------------------------------------ 4./5. teacher-forced parity
def _teacher_forced(model, x):
    """Logits [B, L, vocab] of pushing the tokens x [B, L] one by one through step_logits / push."""
    st = model.new_decode_state(x.shape[0], x.shape[1], DEV)
    out = []
    for t in range(x.shape[1]):
        out.append(model.step_logits(st))
        if t + 1 < x.shape[1]:
            st.push(x[:, t + 1])
    assert torch.equal(st.tokens[:, :x.shape[1]], x.to(DEV)) and st.pos == x.shape[1] - 1 == int(st.pos_dev)
    return torch.stack(out, dim=1)


def test_teacher_forced_small_model_matches_the_causal_oracle(tmp_path):
    """atol 1e-4: the project's bound for this model's logits against the oracle."""
    model, _ = _build(tmp_path, **SMALL)
    p32 = lmo.init_params(16, 64, 2, 128, 2, seed=71)
    model.load_state_dict(p32, strict=False)
    model.eval()
    x, _ = lmo.synthetic_tokens(3, 40, 16, seed=72, ragged=False)
    x[:, 0] = lmo.BOS
    got = _teacher_forced(model, x)
    want = lmo.lm_logits(x, None, {k: v.double() for k, v in p32.items()}, heads=2, num_layers=2, causal=True)
    err = float((got.cpu().double() - want).abs().max())
    print(f"small model, incremental vs float64 oracle: max abs error {err:.3e}")
    assert err <= 1e-4


def test_teacher_forced_shipped_configuration_is_as_close_to_the_oracle_as_the_full_prefix_path(tmp_path):
    """12 layers, d 512, 16 heads, ff 2048, vocab 512; B = 2, 40 tokens.  e_inc <= 2 e_full + 1e-5: both are fp32 evaluations
    of the same function that differ in summation order only.  The test prints both errors."""
    model, _ = _build(tmp_path)
    p32 = lmo.init_params(512, 512, 16, 2048, 12, seed=73)
    model.load_state_dict(p32, strict=False)
    model.eval()
    x, _ = lmo.synthetic_tokens(2, 40, 512, seed=74, ragged=False)
    x[:, 0] = lmo.BOS
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    want = lmo.lm_logits(x, None, {k: v.double() for k, v in p32.items()}, heads=16, num_layers=12, causal=True)
    with torch.no_grad():
        full = model.logits(x.to(DEV), None, causal=True)
    inc = _teacher_forced(model, x)
    e_full = float((full.cpu().double() - want).abs().max())
    e_inc = float((inc.cpu().double() - want).abs().max())
    print(f"shipped configuration vs float64 oracle: e_full {e_full:.3e}, e_inc {e_inc:.3e}")
    assert e_inc <= 2 * e_full + 1e-5, (e_inc, e_full)


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_causal_sample_follows_the_oracle_distribution_and_is_reproducible(tmp_path):
    """Every sampled code satisfies the CDF condition under ONE float64 causal forward over [BOS | returned tokens], with
    tau' = V 2^-23 + 2 (1e-4) / sigma (the logits tolerance of the small model carried into the probabilities)."""
    model, _ = _build(tmp_path, **SMALL)
    p32 = lmo.init_params(16, 64, 2, 128, 2, seed=75)
    model.load_state_dict(p32, strict=False)
    model.eval()
    sigma = 1.0
    u = torch.rand(40, 3, generator=torch.Generator().manual_seed(76))
    audio, q = model.sample(batch_size=3, n_steps=40, device=DEV, sigma=sigma, causal=True, uniforms=u)
    assert q.shape == (3, 40) and q.dtype == torch.int64 and int(q.min()) >= 0 and int(q.max()) < 16
    assert audio.shape == (3, 40 * 128) and audio.dtype == torch.float32 and torch.isfinite(audio).all()
    x = torch.cat([torch.full((3, 1), lmo.BOS, dtype=torch.int64), q.cpu() + lmo.OFFSET], dim=1)
    logits = lmo.lm_logits(x, None, {k: v.double() for k, v in p32.items()}, heads=2, num_layers=2, causal=True)[:, :40]
    ok = _cdf_ok(logits, sigma, u.double().t(), q.cpu(), 16 * 2.0 ** -23 + 2 * 1e-4 / sigma)
    assert bool(ok.all()), ok.logical_not().nonzero().tolist()
    # the same uniforms, the same generator seed: the same codes
    assert torch.equal(model.sample(3, 40, DEV, sigma, causal=True, uniforms=u.to(DEV))[1], q)
    a = model.sample(3, 40, DEV, causal=True, generator=torch.Generator(device=DEV).manual_seed(5))[1]
    b = model.sample(3, 40, DEV, causal=True, generator=torch.Generator(device=DEV).manual_seed(5))[1]
    c = model.sample(3, 40, DEV, causal=True, generator=torch.Generator().manual_seed(5))[1]
    d = model.sample(3, 40, DEV, causal=True, generator=torch.Generator().manual_seed(5))[1]
    assert torch.equal(a, b) and torch.equal(c, d)
    # one captured step replayed: the same launches, so the same bits
    audio_g, q_g = model.sample(3, 40, DEV, sigma, causal=True, uniforms=u, graph=True)
    assert torch.equal(q_g, q) and torch.equal(audio_g, audio)


# ------------------------------------------------------------------------------------------------ 7. long prefix
@pytest.mark.parametrize("batch", [1, 32])
def test_causal_sample_walks_a_prefix_longer_than_every_split(tmp_path, batch):
    model, _ = _build(tmp_path, **{**SMALL, "max_len": 600})
    model.eval()
    audio, q = model.sample(batch_size=batch, n_steps=520, device=DEV, causal=True, generator=torch.Generator().manual_seed(batch))
    assert q.shape == (batch, 520) and int(q.min()) >= 0 and int(q.max()) < 16
    assert audio.shape == (batch, 520 * 128) and torch.isfinite(audio).all()


# ------------------------------------------------------------------------------------------------ 8. arguments
def test_causal_sample_argument_errors_and_the_untouched_default_path(tmp_path):
    model, _ = _build(tmp_path, **SMALL)                       # max_len 64
    model.eval()
    ok = dict(batch_size=2, n_steps=5, device=DEV, causal=True)
    for bad in (dict(sigma=0.0), dict(sigma=-1.0), dict(n_steps=0), dict(n_steps=64), dict(batch_size=0), dict(batch_size=33),
                dict(uniforms=torch.rand(4, 2)), dict(uniforms=torch.rand(5, 3)), dict(uniforms=torch.rand(5, 2, dtype=torch.float64)),
                dict(uniforms=torch.ones(5, 2)), dict(uniforms=-torch.rand(5, 2) - 0.1)):
        with pytest.raises(ValueError):
            model.sample(**{**ok, **bad})
    assert model.sample(**{**ok, "n_steps": 63})[1].shape == (2, 63)          # n_steps + 1 == max_len still fits
    for extra in (dict(uniforms=torch.rand(5, 2)), dict(generator=torch.Generator()), dict(graph=True)):
        with pytest.raises(ValueError):
            model.sample(2, 5, DEV, **extra)
        with pytest.raises(ValueError):
            model.sample(2, 5, DEV, causal=False, **extra)
    model.train()
    with pytest.raises(ValueError):
        model.sample(**ok)
    with pytest.raises(ValueError):
        model.step_logits(model.new_decode_state(2, 5, DEV))
    model.eval()
    st = model.new_decode_state(2, 2, DEV)
    model.step_logits(st)
    st.push(torch.tensor([3, 4]))
    model.step_logits(st)
    st.push(torch.tensor([5, 6]))
    with pytest.raises(ValueError):
        model.step_logits(st)                                  # both positions used
    with pytest.raises(ValueError):
        st.push(torch.tensor([5, 6]))
    # the default path is the code it was: the same global-RNG draws with and without the new keyword
    torch.manual_seed(11)
    audio_a, q_a = model.sample(batch_size=3, n_steps=6, device=DEV, sigma=1.0)
    torch.manual_seed(11)
    audio_b, q_b = model.sample(batch_size=3, n_steps=6, device=DEV, sigma=1.0, causal=False)
    assert torch.equal(q_a, q_b) and torch.equal(audio_a, audio_b)


# ------------------------------------------------------------------------------------------------ 9. command line
def test_sample_from_lm_script_with_causal_flags(tmp_path):
    import wave
    from scripts import sample_from_lm as S
    from utils import config as C
    from utils.commons import get_model, setup_logdir
    log_vq, _ = _vqvae_run(tmp_path, l_bins=16)
    log_dir = str(tmp_path / "run")
    cfg = C.merge(_lm_config(log_vq, **SMALL), C.load(os.path.join(PKG, "configs/datasets/vqlatent.yaml")),
                  C.create({"train": {"batch_size": 2, "n_gpus": 1, "ema": False, "log_dir": log_dir}}))
    setup_logdir(cfg)
    torch.manual_seed(0)
    model, _ = get_model(cfg, DEV)
    torch.save({"model": model.state_dict()}, os.path.join(log_dir, "ckpts", "ckpt.5.pt"))
    common = ["--log_dir", log_dir, "--ckpt_num", "5", "--n_steps", "24", "--n_samples", "2"]
    plain = S.main(common + ["--dump_dir", str(tmp_path / "plain")])
    causal = S.main(common + ["--dump_dir", str(tmp_path / "causal"), "--causal", "--seed", "0"])
    graphed = S.main(common + ["--dump_dir", str(tmp_path / "graphed"), "--causal", "--seed", "0", "--graph"])
    assert sorted(os.listdir(causal)) == sorted(os.listdir(plain)) == ["mel_spectrograms.png", "sample_0.wav", "sample_1.wav", "tokens.txt"]
    with wave.open(os.path.join(causal, "sample_1.wav")) as w:
        assert w.getnframes() == 24 * 128
    table = open(os.path.join(causal, "tokens.txt")).read().splitlines()
    assert len(table) == 4 and len(table[2].split()) == 24 and all(0 <= int(t) < 16 for t in table[2].split())
    assert open(os.path.join(graphed, "tokens.txt")).read() == "\n".join(table) + "\n"      # same seed: same codes, graphed or not
    with pytest.raises(ValueError):
        S.main(common + ["--dump_dir", str(tmp_path / "bad"), "--seed", "0"])
