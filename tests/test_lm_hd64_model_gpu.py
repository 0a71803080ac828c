"""The TransformerLM at head dim 64 (nhead = d_model / 64) end to end: eval logits, a train step with dropout in fp32 and
with `attention_dtype: bf16`, the incremental path (step_logits, prefill, sample, the captured step), one composition with
pre-norm + GELU, and `train.py --model transformer_lm_h8` with `scripts.sample_from_lm --causal` on its checkpoint.

The small model: vocab 16, d_model = embed_dim = 128, 2 heads, 2 layers, ff 128, max_len 64, built the way tests/test_lm_gpu.py
builds its SMALL (through tests/lm_bf16_helpers.build, which holds the same lines).  The yardstick is oracle.lm_oracle in
float64 with heads = 2 (it derives dh = 64); every tolerance is the one the head-dim-32 test of the same quantity uses and is
stated where it is asserted."""
import os

import pytest
import torch

import lm_attn_hd_helpers as A
import lm_bf16_helpers as B
from oracle import lm_oracle as lmo

pytestmark = pytest.mark.gpu
DEV = B.DEV
SMALL = dict(vocab_size=16, embed_dim=128, max_len=64, num_layers=2, d_model=128, nhead=2, dim_feedforward=128, dropout=0.0)
FACTOR, FLOOR = 2.0, 1e-6          # tests/test_lm_attn_bf16_model_gpu.py: the device gets twice the rounded oracle's own error plus 1e-6


def _params(seed, num_layers=2):
    return lmo.init_params(16, 128, 2, 128, num_layers, seed=seed)


def _within(name, device_err, yardstick_err, factor=FACTOR):
    print(f"  {name}: yardstick {yardstick_err:.3e}, device {device_err:.3e} (allowed {factor} x yardstick + {FLOOR})")
    assert device_err <= factor * yardstick_err + FLOOR, (name, device_err, yardstick_err)


def test_eval_logits_match_the_float64_oracle(tmp_path):
    """atol 1e-4: the project's bound for this model family's logits (tests/test_lm_gpu.py)."""
    p32 = _params(11)
    model, _ = B.build(tmp_path, p32, **SMALL)
    assert model.transformer.layers[0].self_attn.num_heads == 2 and model.d_model == 128
    model.eval()
    x, lens = lmo.synthetic_tokens(4, 33, 16, seed=12)
    with torch.no_grad():
        logits = model.logits(x.to(DEV), lens.to(DEV, torch.int32))
    want = lmo.lm_logits(x, lens, {k: v.double() for k, v in p32.items()}, heads=2, num_layers=2)
    keep = torch.arange(33)[None, :] < lens[:, None]
    err = float((logits.cpu().double() - want)[keep].abs().max())
    print(f"  eval logits vs float64 oracle: max abs error {err:.3e}")
    assert torch.allclose(logits.cpu()[keep], want.float()[keep], atol=1e-4), err


def test_train_mode_with_dropout_matches_the_oracle(tmp_path):
    """Dropout 0.1 at every site, the oracle restating the product's masks: loss 2e-5, accuracy 1e-6, gradients 1e-3 rel-L2
    (test_small_model_train_mode_with_dropout_matches_the_oracle)."""
    p32 = _params(21, 3)
    model, _ = B.build(tmp_path, p32, **dict(SMALL, dropout=0.1, num_layers=3))
    x, lens = lmo.synthetic_tokens(4, 33, 16, seed=22)
    model.train()
    model._drop_seed = 40
    loss_dict, metrics = model(x.to(DEV), lens.to(DEV), None, None)
    loss_dict["loss"].backward()
    p64 = {k: v.double().requires_grad_(True) for k, v in p32.items()}
    logits = lmo.lm_logits(x, lens, p64, heads=2, num_layers=3, drop=lmo.CounterDropout(seed=41, p=0.1))   # forward bumps the seed
    loss, acc = lmo.lm_loss(x, logits)
    loss.backward()
    print(f"  loss |err| {abs(float(loss_dict['loss'].detach()) - float(loss.detach())):.3e}; worst gradient rel-L2 "
          f"{max(B.rel(g, p64[n].grad) for n, g in B.named_grads(model).items()):.3e}")
    assert abs(float(loss_dict["loss"]) - float(loss)) < 2e-5 and abs(float(metrics["accuracy"]) - float(acc)) < 1e-6
    for name, grad in B.named_grads(model).items():
        assert B.rel(grad, p64[name].grad) < 1e-3, (name, B.rel(grad, p64[name].grad))


def test_train_mode_with_bf16_attention_is_within_the_rounded_oracles_error(tmp_path):
    """The same step with attention_dtype bf16: loss and every gradient against the exact float64 oracle, within twice what
    the oracle with the rounded attention swapped in is off by, plus 1e-6 (test_train_mode_with_the_products_masks_injected)."""
    p32 = _params(21, 3)
    x, lens = lmo.synthetic_tokens(4, 33, 16, seed=22)
    drop = lmo.CounterDropout(seed=41, p=0.1)
    loss_e, _, grads_e, _ = B.oracle_step(x, lens, p32, 2, 3, False, drop)
    with A.oracle_attention(True):
        loss_r, _, grads_r, _ = B.oracle_step(x, lens, p32, 2, 3, False, drop)
    assert float(loss_r) != float(loss_e)
    model, _ = B.build(tmp_path, p32, **dict(SMALL, dropout=0.1, num_layers=3, attention_dtype="bf16"))
    assert model.attention_dtype == torch.bfloat16
    model.train()
    model._drop_seed = 40
    loss_dict, _ = model(x.to(DEV), lens.to(DEV), None, None)
    loss_dict["loss"].backward()
    _within("loss |err|", abs(float(loss_dict["loss"].detach()) - float(loss_e)), abs(float(loss_r) - float(loss_e)))
    for name, grad in B.named_grads(model).items():
        _within(f"grad {name} rel-L2", B.rel(grad, grads_e[name]), B.rel(grads_r[name], grads_e[name]))


def _teacher_forced(model, x):
    """Logits [B, L, vocab] of pushing the tokens x [B, L] one by one through step_logits / push."""
    st = model.new_decode_state(x.shape[0], x.shape[1], DEV)
    assert st.kv.shape[-3:] == (2, x.shape[1], 64)
    out = []
    for t in range(x.shape[1]):
        out.append(model.step_logits(st))
        if t + 1 < x.shape[1]:
            st.push(x[:, t + 1])
    assert torch.equal(st.tokens[:, :x.shape[1]], x.to(DEV)) and st.pos == x.shape[1] - 1 == int(st.pos_dev)
    return torch.stack(out, dim=1)


def test_incremental_path_matches_the_causal_oracle_and_itself(tmp_path):
    """Teacher-forced step_logits over 40 tokens against the causal float64 oracle, atol 1e-4 (the bound of
    test_teacher_forced_small_model_matches_the_causal_oracle); a prefill of 17 prompt codes followed by step_logits against
    the one-by-one path and against the oracle, atol 1e-4 (test_prefilled_small_model_matches_the_causal_oracle);
    sample(causal=True, uniforms=u) twice gives the same codes, and graph=True gives them too."""
    p32 = _params(71)
    model, _ = B.build(tmp_path, p32, **SMALL)
    model.eval()
    x, _ = lmo.synthetic_tokens(3, 40, 16, seed=72, ragged=False)
    x[:, 0] = lmo.BOS
    got = _teacher_forced(model, x)
    want = lmo.lm_logits(x, None, {k: v.double() for k, v in p32.items()}, heads=2, num_layers=2, causal=True)
    err = float((got.cpu().double() - want).abs().max())
    print(f"  incremental vs float64 oracle: max abs error {err:.3e}")
    assert err <= 1e-4
    n = 17
    st = model.new_decode_state(3, 40, DEV)
    model.prefill(st, x[:, 1:n + 1].to(DEV) - lmo.OFFSET)
    assert st.pos == n == int(st.pos_dev)
    pre = [model.step_logits(st)]
    for t in range(n + 1, n + 4):
        st.push(x[:, t])
        pre.append(model.step_logits(st))
    pre = torch.stack(pre, dim=1)
    e_step = float((pre - got[:, n:n + 4]).abs().max())
    e_orc = float((pre.cpu().double() - want[:, n:n + 4]).abs().max())
    print(f"  prefill of {n} + 3 pushes: vs one-by-one stepping {e_step:.3e}, vs float64 oracle {e_orc:.3e}")
    assert e_step <= 1e-4 and e_orc <= 1e-4
    u = torch.rand(30, 3, generator=torch.Generator().manual_seed(76))
    audio, q = model.sample(batch_size=3, n_steps=30, device=DEV, sigma=1.0, causal=True, uniforms=u)
    assert q.shape == (3, 30) and int(q.min()) >= 0 and int(q.max()) < 16 and torch.isfinite(audio).all()
    assert torch.equal(model.sample(3, 30, DEV, 1.0, causal=True, uniforms=u.to(DEV))[1], q)
    audio_g, q_g = model.sample(3, 30, DEV, 1.0, causal=True, uniforms=u, graph=True)
    assert torch.equal(q_g, q) and torch.equal(audio_g, audio)


def test_composes_with_prenorm_and_gelu(tmp_path):
    """One combination of the other keys: a training step of the pre-norm + GELU model with finite loss and gradients."""
    model, _ = B.build(tmp_path, _params(15, 3), **dict(SMALL, num_layers=3, dropout=0.1, norm_first=True, activation="gelu"))
    x, lens = lmo.synthetic_tokens(3, 33, 16, seed=16)
    model.train()
    loss = model(x.to(DEV), lens.to(DEV), None, None)[0]["loss"]
    loss.backward()
    grads = B.named_grads(model)
    assert torch.isfinite(loss) and all(g is not None and bool(torch.isfinite(g).all()) and bool(g.any()) for g in grads.values())


def test_train_py_and_sample_from_lm_with_the_shipped_config(tmp_path, monkeypatch):
    """`train.py --model transformer_lm_h8 --dataset vqlatent` at a reduced depth (the config's 8 heads of dim 64 at d_model 512
    kept): two steps, a checkpoint, and `scripts.sample_from_lm --causal` on it."""
    import train
    from scripts import generate_vq_dataset as G
    from scripts import sample_from_lm as S
    from utils import config as C
    log_vq, _ = B.vqvae_run(tmp_path, l_bins=16)
    dump_dir = str(tmp_path / "VQ-Latent")
    ds_cfg = C.load(os.path.join(log_vq, "config.yaml"))
    ds_cfg.dataset.update(C.create(dict(num_clips=6, ragged=True)))
    C.save(ds_cfg, os.path.join(log_vq, "config.yaml"))
    G.main(["--log_dir", log_vq, "--ckpt_num", "3", "--dump_dir", dump_dir, "--batch_size", "3", "--n_processes", "1", "--n_workers", "0"])
    monkeypatch.chdir(B.PKG)
    cfg = B.lm_config(log_vq, base="transformer_lm_h8.yaml", vocab_size=16, max_len=64, num_layers=2, dim_feedforward=128)
    assert cfg.model.nhead == 8 and cfg.model.d_model == cfg.model.embed_dim == 512
    C.save(cfg, "configs/models/_test_lm_h8.yaml")
    vql = C.load("configs/datasets/vqlatent.yaml")
    vql.dataset.update(C.create(dict(dataset_path=dump_dir, segment_length=24)))
    C.save(vql, "configs/datasets/_test_vql_h8.yaml")
    try:
        log_dir = str(tmp_path / "run")
        train.main(["--model", "_test_lm_h8", "--dataset", "_test_vql_h8", "--batch_size", "3", "--num_workers", "0",
                    "--total_epochs", "1", "--log_every_n_steps", "1", "--ckpt_every_n_steps", "2", "--eval_every_n_epochs", "1",
                    "--log_dir", log_dir, "--n_gpus", "1"])
        last = torch.load(os.path.join(log_dir, "ckpts", "ckpt.last.pt"), weights_only=True)
        assert last["step"] == 2 and C.load(os.path.join(log_dir, "config.yaml")).model.nhead == 8
        assert last["model"]["transformer.layers.0.self_attn.in_proj_weight"].shape == (3 * 512, 512)
        out = S.main(["--log_dir", log_dir, "--ckpt_num", "2", "--n_steps", "24", "--n_samples", "2", "--dump_dir", str(tmp_path / "out"),
                      "--causal", "--seed", "0"])
        table = open(os.path.join(out, "tokens.txt")).read().splitlines()
        assert len(table[2].split()) == 24 and all(0 <= int(t) < 16 for t in table[2].split())
    finally:
        os.remove("configs/models/_test_lm_h8.yaml")
        os.remove("configs/datasets/_test_vql_h8.yaml")
