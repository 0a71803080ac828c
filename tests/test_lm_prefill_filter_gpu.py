"""Primed and truncated sampling of the TransformerLM (csrc/lm_decode.hip: lm_decode_prefill_kv, lm_decode_sample_filtered;
TransformerLM.prefill, sample(prompt=, top_k=, top_p=)): the copy kernel bit for bit, the filter against its float64
definition written out below, prefilled logits against the float64 oracle (oracle/lm_oracle.py, causal=True), whole runs, the
arguments and the command line.  Every tolerance is stated where it is asserted."""
import os

import pytest
import torch

from oracle import lm_oracle as lmo
from test_lm_decode_gpu import _cdf_ok
from test_lm_gpu import DEV, PKG, SMALL, _build, _lm_config, _vqvae_run

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. prompt keys / values
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("length", [1, 2, 7, 255, 256, 257])
@pytest.mark.parametrize("b,h", [(1, 1), (3, 2), (32, 16)])
def test_prefill_kv_is_a_bit_exact_copy(b, h, length, extra):
    """Rows < len equal the k / v thirds of qkv bit for bit, rows >= len keep the sentinel."""
    from smt_amd import lm as K
    l_max, d = length + extra, h * 32
    qkv = torch.randn(b, length, 3 * d, generator=torch.Generator().manual_seed(100 * b + length)).to(DEV)
    kc = torch.full((b, h, l_max, 32), -7.5, device=DEV)
    vc = torch.full((b, h, l_max, 32), 9.25, device=DEV)
    K.decode_prefill_kv(qkv, kc, vc)
    k, v = (qkv[:, :, j * d:(j + 1) * d].reshape(b, length, h, 32).permute(0, 2, 1, 3) for j in (1, 2))
    assert torch.equal(kc[:, :, :length], k) and torch.equal(vc[:, :, :length], v)
    assert bool((kc[:, :, length:] == -7.5).all()) and bool((vc[:, :, length:] == 9.25).all())


def test_prefill_kv_rejects_bad_arguments():
    from smt_amd import lm as K
    from smt_amd import native as N
    qkv, kc, vc = torch.zeros(2, 4, 3 * 64, device=DEV), torch.zeros(2, 2, 4, 32, device=DEV), torch.zeros(2, 2, 4, 32, device=DEV)
    call = N.lib().smt_lm_decode_prefill_kv
    for args, what in (((N.ptr(qkv), N.ptr(kc), N.ptr(vc), 2, 0, 2, 4), "len"), ((N.ptr(qkv), N.ptr(kc), N.ptr(vc), 2, 5, 2, 4), "len"),
                       ((N.ptr(qkv), N.ptr(kc), N.ptr(vc), 0, 4, 2, 4), "batch"), ((N.ptr(qkv), N.ptr(kc), N.ptr(vc), 33, 4, 2, 4), "batch"),
                       ((None, N.ptr(kc), N.ptr(vc), 2, 4, 2, 4), "null"), ((N.ptr(qkv), None, N.ptr(vc), 2, 4, 2, 4), "null"),
                       ((N.ptr(qkv), N.ptr(kc), None, 2, 4, 2, 4), "null")):
        with pytest.raises(RuntimeError, match=what):
            N.check(call(*args, N.stream_ptr()), "smt_lm_decode_prefill_kv")
    with pytest.raises(RuntimeError, match="len"):
        K.decode_prefill_kv(torch.zeros(2, 5, 3 * 64, device=DEV), kc, vc)
    torch.cuda.synchronize()
    assert not bool(kc.any()) and not bool(vc.any())


# ------------------------------------------------------------------------------------------------ 2.-4. filtered sampler
N_POS = 8


def _sampler_cases(v, b):
    """The logits of test_decode_sample_draws_the_inverse_cdf (unit, x 30, a row with two equal maxima) and uniforms with 0
    and 1 - 2^-24 among them."""
    g = torch.Generator().manual_seed(v + b)
    u = torch.rand(N_POS, b, generator=g)
    u[N_POS - 2], u[N_POS - 1] = 0.0, 1.0 - 2.0 ** -24
    cases = {"unit": torch.randn(b, v, generator=g), "wide": torch.randn(b, v, generator=g) * 30.0, "tie": torch.randn(b, v, generator=g)}
    cases["tie"][0, min(3, v - 1)] = cases["tie"][0, max(v - 2, 0)] = float(cases["tie"][0].max()) + 1.0
    return u, cases


def _filters(v):
    return [(None, 0.9), (min(4, v), None), (v, 0.5), (min(3, v), 0.7), (1, None)]


def _run_filtered(logits, u, sigma, top_k, top_p):
    """All N_POS draws of one logits matrix -> (codes [N_POS, B], kept [N_POS, B]) on the host."""
    from smt_amd import lm as K
    b = logits.shape[0]
    tokens = torch.full((b, N_POS + 1), -1, dtype=torch.int64, device=DEV)
    codes = torch.full((b, N_POS), -1, dtype=torch.int64, device=DEV)
    kept = torch.full((N_POS, b), -1, dtype=torch.int32, device=DEV)
    ld, ud = logits.to(DEV), u.to(DEV)
    for pos in range(N_POS):
        K.decode_sample_filtered(ld, ud, tokens, codes, sigma, top_k, top_p, kept, pos=pos)
    assert torch.equal(tokens[:, 1:], codes + 2) and bool((tokens[:, 0] == -1).all())
    return codes.cpu().t().contiguous(), kept.cpu().long()


def _filter_reference(logits, sigma, top_k):
    """float64: rank [B, V] of every code in the order pi (logit descending, then index ascending; the fp32 logits cast to
    float64, which is exact), the cumulative mass [B, V] along pi normalised over the K candidates, and K."""
    l64 = logits.double()
    v = l64.shape[-1]
    k = v if top_k is None else min(top_k, v)
    order = torch.sort(l64, dim=-1, descending=True, stable=True).indices
    w = torch.exp((l64 - l64.max(-1, keepdim=True).values) / sigma).gather(-1, order)
    w[:, k:] = 0.0
    rank = torch.empty_like(order)
    rank.scatter_(-1, order, torch.arange(v).expand_as(order))
    return rank, torch.cumsum(w, -1) / w.sum(-1, keepdim=True), k


@pytest.mark.parametrize("sigma", [0.5, 2.0])
@pytest.mark.parametrize("b", [1, 32])
@pytest.mark.parametrize("v", [1, 16, 63, 64, 65, 512, 1024])
def test_filtered_sampler_keeps_the_float64_prefix_and_draws_its_inverse_cdf(v, b, sigma):
    """tau = V 2^-23, the bound on an fp32 sum of V non-negative terms (the existing sampler test's).  Every row of every case:
    1 <= n <= K; n = K without top-p; with top-p the first n codes of pi hold >= top_p - tau of the candidates' mass and the
    first n - 1 hold < top_p + tau (or n = 1); the code is among the first n of pi and satisfies the CDF condition on the
    logits masked to -inf outside them."""
    u, cases = _sampler_cases(v, b)
    tau = v * 2.0 ** -23
    for name, logits in cases.items():
        for top_k, top_p in _filters(v):
            what = (name, top_k, top_p)
            code, n = _run_filtered(logits, u, sigma, top_k, top_p)                  # [N_POS, B]
            rank, cm, k = _filter_reference(logits, sigma, top_k)
            assert int(n.min()) >= 1 and int(n.max()) <= k, what
            if top_p is None:
                assert bool((n == k).all()), what
            else:
                cm_n = cm[None].expand(N_POS, b, v)
                mass_n = cm_n.gather(-1, (n - 1)[..., None])[..., 0]
                mass_before = cm_n.gather(-1, (n - 2).clamp_min(0)[..., None])[..., 0]
                assert bool((mass_n >= top_p - tau).all()), (what, float(mass_n.min()))
                assert bool(((n == 1) | (mass_before < top_p + tau)).all()), what
            assert int(code.min()) >= 0 and int(code.max()) < v, what
            code_rank = rank[None].expand(N_POS, b, v).gather(-1, code[..., None])[..., 0]
            assert bool((code_rank < n).all()), what
            masked = logits.double()[None].expand(N_POS, b, v).masked_fill(rank[None] >= n[..., None], float("-inf"))
            ok = _cdf_ok(masked, sigma, u.double(), code, tau)
            assert bool(ok.all()), (what, ok.logical_not().nonzero().tolist())


def _draw(logits, u, **filt):
    """One row of logits, one draw per uniform -> (codes, kept) as lists."""
    from smt_amd import lm as K
    n = len(u)
    tokens, codes = torch.zeros(1, n + 1, dtype=torch.int64, device=DEV), torch.zeros(1, n, dtype=torch.int64, device=DEV)
    kept = torch.zeros(n, 1, dtype=torch.int32, device=DEV)
    ud = torch.tensor(u, dtype=torch.float32, device=DEV)[:, None].contiguous()
    for pos in range(n):
        K.decode_sample_filtered(logits.to(DEV)[None], ud, tokens, codes, 1.0, kept=kept, pos=pos, **filt)
    return codes[0].tolist(), kept[:, 0].tolist()


def test_filtered_sampler_breaks_ties_by_index_exactly():
    flat = torch.zeros(16)
    eighths = [1 / 8, 3 / 8, 5 / 8, 7 / 8]
    assert _draw(flat, eighths, top_k=4) == ([0, 1, 2, 3], [4] * 4)
    assert _draw(flat, eighths, top_p=0.25) == ([0, 1, 2, 3], [4] * 4)       # 4.0 >= 0.25 * 16.0 exactly in fp32
    three = torch.randn(16, generator=torch.Generator().manual_seed(3))
    three[[2, 9, 13]] = float(three.max()) + 1.0
    codes, kept = _draw(three, [(i + 0.5) / 32 for i in range(32)], top_k=2)
    assert set(codes) == {2, 9} and kept == [2] * 32


@pytest.mark.parametrize("sigma", [0.5, 2.0])
@pytest.mark.parametrize("b", [1, 32])
@pytest.mark.parametrize("v", [1, 16, 63, 64, 65, 512, 1024])
def test_filtered_sampler_without_a_filter_is_the_old_sampler(v, b, sigma):
    from smt_amd import lm as K
    u, cases = _sampler_cases(v, b)
    for name, logits in cases.items():
        tokens = torch.full((b, N_POS + 1), -1, dtype=torch.int64, device=DEV)
        codes = torch.full((b, N_POS), -1, dtype=torch.int64, device=DEV)
        for pos in range(N_POS):
            K.decode_sample(logits.to(DEV), u.to(DEV), tokens, codes, sigma, pos=pos)
        for top_k, top_p in ((None, None), (None, 1.0)):
            got, n = _run_filtered(logits, u, sigma, top_k, top_p)
            assert torch.equal(got, codes.cpu().t()) and bool((n == v).all()), (name, top_k, top_p)


def test_filtered_sampler_rejects_bad_arguments():
    from smt_amd import lm as K
    b, n = 2, 3
    tokens, codes = torch.zeros(b, n + 1, dtype=torch.int64, device=DEV), torch.zeros(b, n, dtype=torch.int64, device=DEV)
    u = torch.zeros(n, b, device=DEV)
    ok = torch.zeros(b, 16, device=DEV)
    for logits, filt, what in ((ok, dict(top_k=-1), "top_k"), (ok, dict(top_p=0.0), "top_p"), (ok, dict(top_p=1.5), "top_p"),
                               (ok, dict(top_k=2, pos=n), "pos"), (torch.zeros(b, 4097, device=DEV), dict(top_k=2), "cap")):
        with pytest.raises(RuntimeError, match=what):
            K.decode_sample_filtered(logits, u, tokens, codes, 1.0, **filt)
    # a device position outside the buffers: the launch returns without touching memory
    K.decode_sample_filtered(ok, u, tokens, codes, 1.0, top_k=2, pos_dev=torch.tensor([n], dtype=torch.int32, device=DEV))
    K.decode_sample_filtered(torch.zeros(b, 4096, device=DEV), u, tokens, codes, 1.0, top_k=20000, top_p=0.5, pos=1)   # K = min(top_k, V)
    torch.cuda.synchronize()
    assert not bool(tokens[:, [0, 1, 3]].any()) and not bool(codes[:, [0, 2]].any())


# ------------------------------------------------------------------------------------------------ 5. prefill against the oracle
def _small(tmp_path, seed, **over):
    model, _ = _build(tmp_path, **{**SMALL, **over})
    p32 = lmo.init_params(16, 64, 2, 128, 2, seed=seed)
    model.load_state_dict(p32, strict=False)
    model.eval()
    return model, {k: v.double() for k, v in p32.items()}


def _prefill_then_push(model, x, p):
    """Prompt = the first p codes of the tokens x [B, L] (x[:, 0] = <bos>); logits [B, L - p, vocab] of positions p .. L - 1:
    step_logits after the prefill, then one push per further token."""
    st = model.new_decode_state(x.shape[0], x.shape[1], DEV)
    model.prefill(st, x[:, 1:p + 1] - lmo.OFFSET)
    assert st.pos == p == int(st.pos_dev) and torch.equal(st.tokens[:, :p + 1], x[:, :p + 1].to(DEV))
    assert torch.equal(st.codes[:, :p], (x[:, 1:p + 1] - lmo.OFFSET).to(DEV))
    out = [model.step_logits(st)]
    for t in range(p + 1, x.shape[1]):
        st.push(x[:, t])
        out.append(model.step_logits(st))
    return torch.stack(out, dim=1)


@pytest.mark.parametrize("p", [1, 5, 39])
def test_prefilled_small_model_matches_the_causal_oracle(tmp_path, p):
    """atol 1e-4, the project's bound for this model's logits against the oracle: position P after the prefill and three
    pushed tokens after it."""
    model, p64 = _small(tmp_path, 81)
    x, _ = lmo.synthetic_tokens(3, p + 4, 16, seed=82 + p, ragged=False)
    got = _prefill_then_push(model, x, p)
    want = lmo.lm_logits(x, None, p64, heads=2, num_layers=2, causal=True)[:, p:]
    assert got.shape == want.shape == (3, 4, 16)
    err = float((got.cpu().double() - want).abs().max())
    print(f"small model, prefill of {p} + 3 pushes vs float64 oracle: max abs error {err:.3e}")
    assert err <= 1e-4


@pytest.mark.parametrize("p", [255, 256, 257])
def test_prefilled_rows_are_read_across_the_chunk_boundary_of_the_decode_attention(tmp_path, p):
    """The decode attention takes cache rows in chunks of 256: step_logits after a prefill of 255 / 256 / 257 rows and after
    one more push, atol 1e-4 as above."""
    model, p64 = _small(tmp_path, 83, max_len=600)
    x, _ = lmo.synthetic_tokens(3, p + 2, 16, seed=84 + p, ragged=False)
    got = _prefill_then_push(model, x, p)
    want = lmo.lm_logits(x, None, p64, heads=2, num_layers=2, causal=True)[:, p:]
    err = float((got.cpu().double() - want).abs().max())
    print(f"small model, prefill of {p} + 1 push vs float64 oracle: max abs error {err:.3e}")
    assert got.shape == (3, 2, 16) and err <= 1e-4


def test_prefilled_shipped_configuration_is_as_close_to_the_oracle_as_the_full_prefix_path(tmp_path):
    """12 layers, d 512, 16 heads, ff 2048, vocab 512; B = 2, a prompt of 20 codes and 19 pushes.  e_pre <= 2 e_full + 1e-5 over
    the positions 20..39 both produce (fp32 evaluations of one function that differ in summation order only).  Prints both."""
    model, _ = _build(tmp_path)
    p32 = lmo.init_params(512, 512, 16, 2048, 12, seed=85)
    model.load_state_dict(p32, strict=False)
    model.eval()
    x, _ = lmo.synthetic_tokens(2, 40, 512, seed=86, ragged=False)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    want = lmo.lm_logits(x, None, {k: v.double() for k, v in p32.items()}, heads=16, num_layers=12, causal=True)[:, 20:]
    with torch.no_grad():
        full = model.logits(x.to(DEV), None, causal=True)[:, 20:]
    pre = _prefill_then_push(model, x, 20)
    e_full = float((full.cpu().double() - want).abs().max())
    e_pre = float((pre.cpu().double() - want).abs().max())
    print(f"shipped configuration vs float64 oracle, positions 20..39: e_full {e_full:.3e}, e_pre {e_pre:.3e}")
    assert pre.shape == (2, 20, 512) and e_pre <= 2 * e_full + 1e-5, (e_pre, e_full)


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_primed_and_filtered_sampling_end_to_end(tmp_path):
    """tau' = V 2^-23 + 2 (1e-4) / sigma for the new codes under ONE float64 causal forward over [BOS | codes] (the bound of the
    existing end-to-end test); the filtered run equals, bit for bit, prefill + step_logits + the stand-alone filtered sampler
    + push driven from here; graph = eager; the same uniforms / generator seed give the same codes."""
    from smt_amd import lm as K
    model, p64 = _small(tmp_path, 87)
    sigma, n_p, n_s = 1.0, 5, 35
    g = torch.Generator().manual_seed(88)
    prompt = torch.randint(0, 16, (3, n_p), generator=g)
    u = torch.rand(n_s, 3, generator=g)
    audio, q = model.sample(3, n_s, DEV, sigma, causal=True, uniforms=u, prompt=prompt)
    assert q.shape == (3, 40) and q.dtype == torch.int64 and torch.equal(q[:, :n_p].cpu(), prompt)
    assert int(q.min()) >= 0 and int(q.max()) < 16
    assert audio.shape == (3, 40 * 128) and audio.dtype == torch.float32 and torch.isfinite(audio).all()
    x = torch.cat([torch.full((3, 1), lmo.BOS, dtype=torch.int64), q.cpu() + lmo.OFFSET], dim=1)
    logits = lmo.lm_logits(x, None, p64, heads=2, num_layers=2, causal=True)[:, n_p:40]
    ok = _cdf_ok(logits, sigma, u.double().t(), q.cpu()[:, n_p:], 16 * 2.0 ** -23 + 2 * 1e-4 / sigma)
    assert bool(ok.all()), ok.logical_not().nonzero().tolist()
    assert torch.equal(model.sample(3, n_s, DEV, sigma, causal=True, uniforms=u.to(DEV), prompt=prompt.to(DEV))[1], q)
    assert torch.equal(model.sample(3, n_s, DEV, sigma, causal=True, uniforms=u, prompt=prompt[0])[1][0], q[0])   # [P]: every row

    filt = dict(top_k=4, top_p=0.9)
    audio_f, q_f = model.sample(3, n_s, DEV, sigma, causal=True, uniforms=u, prompt=prompt, **filt)
    assert q_f.shape == (3, 40) and torch.equal(q_f[:, :n_p].cpu(), prompt)
    st = model.new_decode_state(3, n_p + n_s, DEV, torch.cat([torch.zeros(n_p, 3), u]))
    model.prefill(st, prompt)
    tokens, codes = torch.zeros_like(st.tokens), torch.zeros_like(st.codes)
    kept = torch.zeros_like(st.kept)
    for _ in range(n_s):
        K.decode_sample_filtered(model.step_logits(st), st.uniforms, tokens, codes, sigma, kept=kept, pos=st.pos, **filt)
        st.push(tokens[:, st.pos + 1].clone())
    assert torch.equal(codes[:, n_p:], q_f[:, n_p:])
    assert int(kept[n_p:].min()) >= 1 and int(kept[n_p:].max()) <= 4 and not bool(kept[:n_p].any())

    for kw, (a_ref, q_ref) in ((dict(), (audio, q)), (filt, (audio_f, q_f))):
        a_g, q_g = model.sample(3, n_s, DEV, sigma, causal=True, uniforms=u, prompt=prompt, graph=True, **kw)
        assert torch.equal(q_g, q_ref) and torch.equal(a_g, a_ref), kw
    a = model.sample(3, n_s, DEV, causal=True, generator=torch.Generator(device=DEV).manual_seed(5), prompt=prompt, **filt)[1]
    b = model.sample(3, n_s, DEV, causal=True, generator=torch.Generator(device=DEV).manual_seed(5), prompt=prompt, **filt)[1]
    c = model.sample(3, n_s, DEV, causal=True, generator=torch.Generator().manual_seed(5), top_p=0.5)[1]
    d = model.sample(3, n_s, DEV, causal=True, generator=torch.Generator().manual_seed(5), top_p=0.5)[1]
    assert torch.equal(a, b) and torch.equal(c, d) and c.shape == (3, n_s)


# ------------------------------------------------------------------------------------------------ 7. arguments
def test_prompt_and_filter_argument_errors_and_the_untouched_plain_path(tmp_path):
    from smt_amd import lm as K
    model, _ = _small(tmp_path, 89)                             # vocab 16, max_len 64
    prompt = torch.tensor([[1, 2, 3], [4, 5, 6]])
    for extra in (dict(prompt=prompt), dict(top_k=4), dict(top_p=0.9)):
        with pytest.raises(ValueError):
            model.sample(2, 5, DEV, **extra)
        with pytest.raises(ValueError):
            model.sample(2, 5, DEV, causal=False, **extra)
    ok = dict(batch_size=2, n_steps=5, device=DEV, causal=True)
    for bad in (dict(top_k=0), dict(top_k=17), dict(top_k=2.0), dict(top_p=0.0), dict(top_p=1.5), dict(prompt=torch.tensor([[1, 2], [3, 16]])),
                dict(prompt=torch.tensor([[1, 2], [3, -1]])), dict(prompt=prompt.to(torch.int32)), dict(prompt=prompt.float()),
                dict(prompt=torch.tensor([[1, 2, 3]] * 3)), dict(prompt=torch.zeros(2, 0, dtype=torch.int64)), dict(prompt=[1, 2, 3]),
                dict(prompt=prompt, n_steps=61)):
        with pytest.raises(ValueError):
            model.sample(**{**ok, **bad})
    assert model.sample(**{**ok, "prompt": prompt, "n_steps": 60, "top_k": 16, "top_p": 1.0})[1].shape == (2, 63)   # 3 + 60 + 1 == max_len
    st = model.new_decode_state(2, 8, DEV)
    model.train()
    with pytest.raises(ValueError):
        model.prefill(st, prompt)
    model.eval()
    with pytest.raises(ValueError):
        model.prefill(st, torch.zeros(2, 9, dtype=torch.int64))           # <bos> + 9 codes do not fit 9 tokens
    model.prefill(st, prompt)
    with pytest.raises(ValueError):
        model.prefill(st, prompt)                                         # not at position 0 any more
    pushed = model.new_decode_state(2, 8, DEV)
    pushed.push(torch.tensor([3, 4]))
    with pytest.raises(ValueError):
        model.prefill(pushed, prompt)
    # without the new arguments sample() is the step loop over the entry points it had before them
    u = torch.rand(8, 3, generator=torch.Generator().manual_seed(90))
    audio, q = model.sample(3, 8, DEV, causal=True, uniforms=u)
    old = model.new_decode_state(3, 8, DEV, u)
    for _ in range(8):
        model._decode_logits(old)
        K.decode_sample(old.logits, old.uniforms, old.tokens, old.codes, 1.0, 0, old.pos_dev, model.OFFSET)
        old.advance()
    assert q.shape == (3, 8) and torch.equal(q, old.codes) and audio.shape == (3, 8 * 128)


# ------------------------------------------------------------------------------------------------ 8. command line
def test_sample_from_lm_script_with_prompt_and_filter_flags(tmp_path):
    from datasets.vqlatent import dump_plain_pickle
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
    utterance = [7, 0, 15, 3, 3, 9, 1, 12]
    prompt_file = str(tmp_path / "00000.pkl")
    dump_plain_pickle({"x": [0.0] * (128 * len(utterance)), "q": utterance}, prompt_file)
    common = ["--log_dir", log_dir, "--ckpt_num", "5", "--n_steps", "24", "--n_samples", "2"]
    flags = ["--top_k", "4", "--top_p", "0.9", "--prompt_file", prompt_file, "--prompt_len", "5", "--seed", "0"]
    out = S.main(common + ["--dump_dir", str(tmp_path / "primed"), "--causal"] + flags)
    table = open(os.path.join(out, "tokens.txt")).read().splitlines()
    assert len(table) == 4
    for row in table[2:]:
        cells = [int(t) for t in row.split()]
        assert len(cells) == 5 + 24 and cells[:5] == utterance[:5] and all(0 <= t < 16 for t in cells)
    again = S.main(common + ["--dump_dir", str(tmp_path / "again"), "--causal", "--graph"] + flags)
    assert open(os.path.join(again, "tokens.txt")).read() == "\n".join(table) + "\n"     # same seed: same codes, graphed or not
    for bad in (["--top_k", "4"], ["--top_p", "0.9"], ["--prompt_file", prompt_file], ["--prompt_len", "5"]):
        with pytest.raises(ValueError):
            S.main(common + ["--dump_dir", str(tmp_path / "bad")] + bad)
    with pytest.raises(ValueError):
        S.main(common + ["--dump_dir", str(tmp_path / "bad"), "--causal", "--prompt_file", prompt_file, "--prompt_len", "9"])
    # more samples than one decoding state takes: chunks of at most 32
    many = S.main(["--log_dir", log_dir, "--ckpt_num", "5", "--n_steps", "24", "--n_samples", "33", "--dump_dir", str(tmp_path / "many"),
                   "--causal", "--top_k", "4", "--seed", "0"])
    assert len(open(os.path.join(many, "tokens.txt")).read().splitlines()) == 2 + 33
    assert os.path.exists(os.path.join(many, "sample_32.wav"))
