"""`model.attention_dtype: bf16` of the TransformerLM: the attention core's products on bf16 MFMAs, everything else as before.

Tolerances follow the rule of tests/test_lm_bf16_gpu.py.  The yardstick is the float64 CPU oracle with the rounded attention of
tests/lm_attn_bf16_helpers.py swapped in (and, when compute_dtype is bf16 too, the rounded linears of tests/lm_bf16_helpers.py);
its own error against the exact float64 oracle is computed here, on the CPU, and the device gets twice that plus 1e-6, quantity
by quantity, so that fp32 effects have room.  Each test prints the yardstick's figure next to the device's; DESIGN.md
section 23 records what came out on an MI355X.
"""
import os

import pytest
import torch

import lm_attn_bf16_helpers as A
import lm_bf16_helpers as B
import lm_prenorm_helpers as H
from oracle import lm_oracle as lmo

pytestmark = pytest.mark.gpu
DEV = B.DEV
FACTOR, FLOOR = 2.0, 1e-6
ATTN = dict(attention_dtype="bf16")
BOTH = dict(attention_dtype="bf16", compute_dtype="bf16")


def _within(name, device_err, yardstick_err, factor=FACTOR):
    print(f"  {name}: yardstick {yardstick_err:.3e}, device {device_err:.3e} (allowed {factor} x yardstick + {FLOOR})")
    assert device_err <= factor * yardstick_err + FLOOR, (name, device_err, yardstick_err)


def _oracle_step(x, lens, params, heads, num_layers, rounded_attn, rounded_linear, drop=None):
    with A.oracle_attention(rounded_attn):
        return B.oracle_step(x, lens, params, heads, num_layers, rounded=rounded_linear, drop=drop)


@pytest.mark.parametrize("over", [ATTN, BOTH], ids=["attention_bf16", "attention_and_projections_bf16"])
def test_reference_fixture_through_bf16_attention(golden, tmp_path, over):
    """tests/golden/transformer_lm.npz (the reference's own model and batch): loss, logits and every parameter gradient against
    the exact float64 oracle, within twice what the rounded oracle is off by.  Layer 0's saturated softmax makes its
    in-projection and embedding gradients sensitive to operand rounding; the yardstick carries that."""
    g = golden("transformer_lm")
    params = {k[len("param."):]: torch.from_numpy(g[k]) for k in g if k.startswith("param.")}
    x, lens = torch.from_numpy(g["x"]), torch.from_numpy(g["lens"])
    lin = "compute_dtype" in over
    loss_r, logits_r, grads_r, _ = _oracle_step(x, lens, params, 2, 2, True, lin)
    loss_e, logits_e, grads_e, _ = _oracle_step(x, lens, params, 2, 2, False, False)
    assert abs(float(loss_e) - float(g["loss"])) < 1e-5               # the unrounded oracle IS the fixture (an fp32 capture)

    model, _ = B.build(tmp_path, params, **dict(B.SMALL, **over))
    assert model.attention_dtype == torch.bfloat16
    model.train()
    xd, ld = x.to(DEV), lens.to(DEV)
    logits = model.logits(xd, ld.to(torch.int32))
    _within("logits max |err|", float((logits.detach().cpu().double() - logits_e).abs().max()), float((logits_r - logits_e).abs().max()))
    loss_dict, _ = model(xd, ld, None, None)
    _within("loss |err|", abs(float(loss_dict["loss"].detach()) - float(loss_e)), abs(float(loss_r) - float(loss_e)))
    loss_dict["loss"].backward()
    for name, grad in B.named_grads(model).items():
        _within(f"grad {name} rel-L2", B.rel(grad, grads_e[name]), B.rel(grads_r[name], grads_e[name]))


def test_train_mode_with_the_products_masks_injected(tmp_path):
    """Dropout 0.1, three layers, one seed: loss and gradients against the exact float64 oracle drawing the same masks."""
    cfg = dict(B.SMALL, dropout=0.1, num_layers=3)
    p32 = lmo.init_params(16, 64, 2, 128, 3, seed=21)
    x, lens = lmo.synthetic_tokens(4, 33, 16, seed=22)
    drop = lmo.CounterDropout(seed=41, p=0.1)
    loss_e, _, grads_e, _ = _oracle_step(x, lens, p32, 2, 3, False, False, drop)
    loss_r, _, grads_r, _ = _oracle_step(x, lens, p32, 2, 3, True, False, drop)
    model, _ = B.build(tmp_path, p32, **dict(cfg, **ATTN))
    model.train()
    model._drop_seed = 40
    loss_dict, _ = model(x.to(DEV), lens.to(DEV), None, None)
    loss_dict["loss"].backward()
    _within("loss |err|", abs(float(loss_dict["loss"].detach()) - float(loss_e)), abs(float(loss_r) - float(loss_e)))
    for name, grad in B.named_grads(model).items():
        _within(f"grad {name} rel-L2", B.rel(grad, grads_e[name]), B.rel(grads_r[name], grads_e[name]))


def test_training_trajectory_tracks_the_fp32_path(tmp_path):
    """20 AdamW steps, three layers, dropout 0.1, ragged lengths, equal weights, batch and seeds: the largest distance of the
    bf16-attention loss curve from the fp32 device curve is at most twice the largest distance between the rounded and the
    exact float64 oracle trained the same way (one band for all steps, as in tests/test_lm_bf16_gpu.py)."""
    cfg = dict(B.SMALL, dropout=0.1, num_layers=3)
    p32 = lmo.init_params(16, 64, 2, 128, 3, seed=33)
    x, lens = lmo.synthetic_tokens(4, 33, 16, seed=34)
    steps, lr, seed0 = 20, 2e-3, 70
    exact = B.oracle_trajectory(x, lens, p32, 2, 3, False, steps, lr, seed0, 0.1)
    with A.oracle_attention(True):
        rounded = B.oracle_trajectory(x, lens, p32, 2, 3, False, steps, lr, seed0, 0.1)
    yard = [abs(a - b) for a, b in zip(rounded, exact)]
    log_dir, curves = None, {}
    for name, over in (("fp32", {}), ("bf16", ATTN)):
        model, log_dir = B.build(tmp_path, p32, log_dir=log_dir, **dict(cfg, **over))
        model.train()
        model._drop_seed = seed0
        opt = torch.optim.AdamW([p for n, p in model.named_parameters() if not n.startswith("vqvae.")], lr=lr)
        losses = []
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            loss = model(x.to(DEV), lens.to(DEV), None, None)[0]["loss"]
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        curves[name] = losses
    diff = [abs(a - b) for a, b in zip(curves["bf16"], curves["fp32"])]
    print("  step: yardstick |rounded - exact|, device |bf16 - fp32|, fp32 loss")
    for k in range(steps):
        print(f"  {k:2d}: {yard[k]:.3e}  {diff[k]:.3e}  {curves['fp32'][k]:.4f}")
    for name in ("fp32", "bf16"):
        assert sum(curves[name][-3:]) / 3 < sum(curves[name][:3]) / 3 - 0.05, (name, curves[name])
    _within("largest loss distance over 20 steps", max(diff), max(yard))


def _run(model, x, lens):
    model.train()
    logits = model.logits(x.to(DEV), lens.to(DEV, torch.int32))
    model(x.to(DEV), lens.to(DEV), None, None)[0]["loss"].backward()
    return logits.detach(), B.named_grads(model)


def test_key_absent_is_fp32_bit_for_bit(tmp_path):
    p32 = lmo.init_params(16, 64, 2, 128, 2, seed=5)
    x, lens = lmo.synthetic_tokens(3, 20, 16, seed=6)
    log_dir, out = None, []
    for over in ({}, dict(attention_dtype="fp32"), ATTN):
        model, log_dir = B.build(tmp_path, p32, log_dir=log_dir, **dict(B.SMALL, **over))
        assert model.attention_dtype == (torch.bfloat16 if over is ATTN else torch.float32)
        out.append(_run(model, x, lens))
    assert torch.equal(out[0][0], out[1][0])
    for name in out[0][1]:
        if name == "embedding.weight":
            # smt_lm_embed_bwd adds the rows of a repeated token with fp32 atomics, in arrival order (tests/test_lm_bf16_gpu.py)
            assert B.rel(out[0][1][name], out[1][1][name]) < 1e-6, name
        else:
            assert torch.equal(out[0][1][name], out[1][1][name]), name
    assert not torch.equal(out[0][0], out[2][0])                      # and the key does something


def test_composes_with_prenorm_gelu_and_bf16_projections(tmp_path):
    """norm_first + gelu + both bf16 keys: logits and every gradient within the yardstick (the pre-norm float64 helper with the
    rounded attention and the rounded linears)."""
    p32 = lmo.init_params(16, 64, 2, 128, 3, seed=15)
    x, lens = lmo.synthetic_tokens(3, 33, 16, seed=16)
    linear = lambda t, w, b=None: B.RoundedLinear.apply(t, w, b)   # noqa: E731
    _, _, logits_e, grads_e = H.step64(x, lens, p32, 2, 3, True, "gelu")
    with A.oracle_attention(True):
        _, _, logits_r, grads_r = H.step64(x, lens, p32, 2, 3, True, "gelu", linear=linear)
    model, _ = B.build(tmp_path, p32, **dict(B.SMALL, num_layers=3, norm_first=True, activation="gelu", **BOTH))
    logits, grads = _run(model, x, lens)
    keep = H.unpadded(lens, 33)
    _within("logits max |err|", float((logits.cpu().double() - logits_e)[keep].abs().max()), float((logits_r - logits_e)[keep].abs().max()))
    for name, grad in grads.items():
        _within(f"grad {name} rel-L2", B.rel(grad, grads_e[name]), B.rel(grads_r[name], grads_e[name]))


@pytest.mark.parametrize("n_prompt", [5, 39])
def test_prefill_and_step_logits_follow_logits(tmp_path, n_prompt):
    """prefill (bf16 attention over the prompt) + step_logits (the fp32 one-token kernel) against `logits` on the same prefix:
    each is within E of the exact logits, E = twice the rounded oracle's own error, so the two are within 2 E of each other."""
    p32 = lmo.init_params(16, 64, 2, 128, 2, seed=9)
    model, _ = B.build(tmp_path, p32, **dict(B.SMALL, **ATTN))
    model.eval()
    codes = torch.randint(0, 16, (3, n_prompt), generator=torch.Generator().manual_seed(2))
    tokens = torch.cat([torch.full((3, 1), lmo.BOS), codes + lmo.OFFSET], dim=1)
    p64 = {k: v.double() for k, v in p32.items()}
    exact = lmo.lm_logits(tokens, None, p64, heads=2, num_layers=2)
    with A.oracle_attention(True):
        rounded = lmo.lm_logits(tokens, None, p64, heads=2, num_layers=2)
    e = float((rounded - exact).abs().max())
    st = model.new_decode_state(3, n_prompt + 3, DEV)
    model.prefill(st, codes.to(DEV))
    step = model.step_logits(st)
    with torch.no_grad():
        full = model.logits(tokens.to(DEV), None)[:, n_prompt]
    _within("logits vs exact, max |err|", float((full.cpu().double() - exact[:, n_prompt]).abs().max()), e)
    _within("prefill + step vs logits, max |diff|", float((step - full).abs().max()), 2 * e)


def test_causal_sampling_runs_and_decoding_stays_fp32(tmp_path):
    p32 = lmo.init_params(16, 64, 2, 128, 2, seed=9)
    m32, log_dir = B.build(tmp_path, p32, **B.SMALL)
    mbf, _ = B.build(tmp_path, p32, log_dir=log_dir, **dict(B.SMALL, **ATTN))
    m32.eval(), mbf.eval()
    u = torch.rand(10, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    _, q32 = m32.sample(3, 10, device=DEV, causal=True, uniforms=u)
    _, qbf = mbf.sample(3, 10, device=DEV, causal=True, uniforms=u)
    assert qbf.shape == (3, 10) and int(qbf.min()) >= 0 and int(qbf.max()) < 16
    assert torch.equal(q32, qbf)                                      # no prompt: only the fp32 one-token kernels ran


def test_train_py_with_the_shipped_config(tmp_path, monkeypatch):
    """`train.py --model transformer_lm_bf16_attn --dataset vqlatent` at a small size: one short epoch and a checkpoint."""
    import train
    from scripts import generate_vq_dataset as G
    from utils import config as C
    log_vq, _ = B.vqvae_run(tmp_path, l_bins=16)
    dump_dir = str(tmp_path / "VQ-Latent")
    ds_cfg = C.load(os.path.join(log_vq, "config.yaml"))
    ds_cfg.dataset.update(C.create(dict(num_clips=6, ragged=True)))
    C.save(ds_cfg, os.path.join(log_vq, "config.yaml"))
    G.main(["--log_dir", log_vq, "--ckpt_num", "3", "--dump_dir", dump_dir, "--batch_size", "3", "--n_processes", "1", "--n_workers", "0"])
    monkeypatch.chdir(B.PKG)
    cfg = B.lm_config(log_vq, base="transformer_lm_bf16_attn.yaml", **B.SMALL)
    assert cfg.model.compute_dtype == "bf16" and cfg.model.attention_dtype == "bf16"
    C.save(cfg, "configs/models/_test_lm_bf16_attn.yaml")
    vql = C.load("configs/datasets/vqlatent.yaml")
    vql.dataset.update(C.create(dict(dataset_path=dump_dir, segment_length=24)))
    C.save(vql, "configs/datasets/_test_vql_bf16_attn.yaml")
    try:
        log_dir = str(tmp_path / "run")
        train.main(["--model", "_test_lm_bf16_attn", "--dataset", "_test_vql_bf16_attn", "--batch_size", "3", "--num_workers", "0",
                    "--total_epochs", "1", "--log_every_n_steps", "1", "--ckpt_every_n_steps", "2", "--eval_every_n_epochs", "1",
                    "--log_dir", log_dir, "--n_gpus", "1"])
        last = torch.load(os.path.join(log_dir, "ckpts", "ckpt.last.pt"), weights_only=True)
        assert last["step"] == 2 and last["extra"]["drop_seed"] == 2
        assert C.load(os.path.join(log_dir, "config.yaml")).model.attention_dtype == "bf16"
    finally:
        os.remove("configs/models/_test_lm_bf16_attn.yaml")
        os.remove("configs/datasets/_test_vql_bf16_attn.yaml")
