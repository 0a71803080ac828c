"""`model.compute_dtype: bf16` of the TransformerLM: the six projections on csrc/lm_linear.hip, everything else as before.

The yardstick for every tolerance here is measured, not chosen: the float64 CPU oracle with only the operand roundings of the
projections applied (tests/lm_bf16_helpers.py) is compared with the same reference the device is compared with, and the
device gets twice the oracle's error, quantity by quantity (the factor covers fp32 accumulation order and the fp32 kernels
between the projections).  Each test prints the yardstick's figure next to the device's.

Measured on an MI355X (yardstick -> device), the figures DESIGN.md section 21 records:
  reference fixture: loss 9.13e-4 -> 9.13e-4, logits max 4.27e-2 -> 4.27e-2, worst gradient rel-L2 0.229 -> 0.229 (layer 0
    in-projection; the layers above it 2e-3 .. 6e-2, device = yardstick to four digits)
  train mode with dropout, three layers, random weights: loss 6.28e-4 -> 6.34e-4, worst gradient rel-L2 0.4925 -> 0.4925
    (embedding), forward bands of the feed-forward pre-activations 0.73 / 0.71 / 0.43
  20-step trajectory: largest loss distance 4.51e-2 (rounded vs exact oracle) -> 6.32e-2 (bf16 vs fp32 on the device)
The large first-layer figures are the model's, not the kernels': the embedding is scaled by sqrt(d_model), so the first
layer's attention scores are of order d_model and its softmax is close to an argmax, which a 2^-9 change of q and k can flip.
"""
import os

import pytest
import torch

import lm_bf16_helpers as B
from oracle import lm_oracle as lmo

pytestmark = pytest.mark.gpu
DEV = B.DEV
FACTOR = 2.0                       # device allowance over the yardstick's own error
BF16 = dict(compute_dtype="bf16")


def _within(name, device_err, yardstick_err):
    print(f"  {name}: yardstick {yardstick_err:.3e}, device {device_err:.3e} (allowed {FACTOR} x yardstick)")
    assert device_err <= FACTOR * yardstick_err, (name, device_err, yardstick_err)


def test_reference_fixture_through_the_bf16_path(golden, tmp_path):
    """tests/golden/transformer_lm.npz (the reference's own model and batch) with compute_dtype bf16: loss, logits and every
    parameter gradient against the fixture, within twice what the rounded float64 oracle is off by."""
    g = golden("transformer_lm")
    params = {k[len("param."):]: torch.from_numpy(g[k]) for k in g if k.startswith("param.")}
    x, lens = torch.from_numpy(g["x"]), torch.from_numpy(g["lens"])
    loss64, logits64, grads64, _ = B.oracle_step(x, lens, params, heads=2, num_layers=2, rounded=True)
    exact_loss, exact_logits, _, _ = B.oracle_step(x, lens, params, heads=2, num_layers=2, rounded=False)
    assert abs(float(exact_loss) - float(g["loss"])) < 1e-5          # the unrounded oracle IS the fixture (fp32 capture)

    model, _ = B.build(tmp_path, params, **dict(B.SMALL, **BF16))
    assert model.compute_dtype == torch.bfloat16
    model.train()
    xd, ld = x.to(DEV), lens.to(DEV)
    logits = model.logits(xd, ld.to(torch.int32))
    ref_logits = torch.from_numpy(g["logits"]).double()
    _within("logits max |err|", float((logits.detach().cpu().double() - ref_logits).abs().max()), float((logits64 - ref_logits).abs().max()))
    loss_dict, _ = model(xd, ld, None, None)
    _within("loss |err|", abs(float(loss_dict["loss"].detach()) - float(g["loss"])), abs(float(loss64) - float(g["loss"])))
    loss_dict["loss"].backward()
    for name, grad in B.named_grads(model).items():
        ref = torch.from_numpy(g["grad." + name])
        _within(f"grad {name} rel-L2", B.rel(grad, ref), B.rel(grads64[name], ref))


def test_train_mode_draws_the_fp32_masks_and_stays_inside_the_band(tmp_path, monkeypatch):
    """Dropout 0.1, three layers, one seed: the bf16 step and the fp32 step draw the same masks (the zero pattern after
    bias + ReLU + dropout agrees wherever both pre-activations are further from 0 than the forward band), and loss and
    gradients against the exact float64 oracle stay within twice the rounded oracle's error."""
    from smt_amd import lm as K
    cfg = dict(B.SMALL, dropout=0.1, num_layers=3)
    p32 = lmo.init_params(16, 64, 2, 128, 3, seed=21)
    x, lens = lmo.synthetic_tokens(4, 33, 16, seed=22)
    drop = lmo.CounterDropout(seed=41, p=0.1)
    pre_exact, pre_rounded = [], []
    loss_e, _, grads_e, _ = B.oracle_step(x, lens, p32, 2, 3, rounded=False, drop=drop, record=pre_exact, record_n_out=128)
    loss_r, _, grads_r, _ = B.oracle_step(x, lens, p32, 2, 3, rounded=True, drop=drop, record=pre_rounded, record_n_out=128)
    bands = [FACTOR * float((a - b).abs().max()) for a, b in zip(pre_exact, pre_rounded)]      # one per layer
    print("  forward bands of the feed-forward pre-activations, layer by layer: " + ", ".join(f"{b:.3e}" for b in bands))

    seen = []
    inner = K.bias_relu_dropout_

    def spy(h, bias, drop=K.NO_DROP):
        pre = (h + bias).detach().clone()
        out = inner(h, bias, drop)
        seen.append((pre, (out.detach() == 0).clone()))
        return out

    monkeypatch.setattr(K, "bias_relu_dropout_", spy)
    log_dir, results = None, {}
    for name, over in (("fp32", {}), ("bf16", BF16)):
        model, log_dir = B.build(tmp_path, p32, log_dir=log_dir, **dict(cfg, **over))
        model.train()
        model._drop_seed = 40
        seen.clear()
        loss_dict, _ = model(x.to(DEV), lens.to(DEV), None, None)
        loss_dict["loss"].backward()
        results[name] = (float(loss_dict["loss"]), B.named_grads(model), list(seen))
    assert len(results["fp32"][2]) == len(results["bf16"][2]) == 3
    for site, ((pre_a, zero_a), (pre_b, zero_b), pre64, band) in enumerate(zip(results["fp32"][2], results["bf16"][2], pre_exact, bands)):
        assert float((pre_a.cpu().double() - pre64).abs().max()) <= band and float((pre_b.cpu().double() - pre64).abs().max()) <= band
        clear = (pre_a.abs() > band) & (pre_b.abs() > band)
        covered = float(clear.float().mean())
        print(f"  layer {site}: {100 * covered:.1f} % of the {clear.numel()} elements are clear of the band")
        # these random weights give the first layer attention scores of order 64, so the rounded operands move the
        # activations by tenths (the band above says so) and a good part of the pre-activations lies inside it; a different
        # mask would still show on a tenth of whatever is covered, so a quarter of 16,896 elements is plenty
        assert covered > 0.25
        assert torch.equal(zero_a[clear], zero_b[clear]), f"site {site}: the two dtypes dropped different elements"
        assert 0.4 < float(zero_b.float().mean()) < 0.7             # ReLU zeroes half, dropout a tenth of the rest
    _within("loss |err|", abs(results["bf16"][0] - float(loss_e)), abs(float(loss_r) - float(loss_e)))
    for name, grad in results["bf16"][1].items():
        _within(f"grad {name} rel-L2", B.rel(grad, grads_e[name]), B.rel(grads_r[name], grads_e[name]))


def test_training_trajectory_tracks_the_fp32_path(tmp_path):
    """20 AdamW steps at SMALL with three layers, dropout 0.1 and ragged lengths, from equal weights, batch and seeds, in both
    dtypes.  Both losses decrease; the distance between the two curves stays within twice the largest distance between the
    rounded and the exact float64 oracle trained the same way (one band for all steps: the distance changes sign along the
    way, so a per-step yardstick would be 0 somewhere)."""
    cfg = dict(B.SMALL, dropout=0.1, num_layers=3)
    p32 = lmo.init_params(16, 64, 2, 128, 3, seed=33)
    x, lens = lmo.synthetic_tokens(4, 33, 16, seed=34)
    steps, lr, seed0 = 20, 2e-3, 70
    exact = B.oracle_trajectory(x, lens, p32, 2, 3, False, steps, lr, seed0, 0.1)
    rounded = B.oracle_trajectory(x, lens, p32, 2, 3, True, steps, lr, seed0, 0.1)
    yard = [abs(a - b) for a, b in zip(rounded, exact)]
    log_dir, curves = None, {}
    for name, over in (("fp32", {}), ("bf16", BF16)):
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
    print(f"  step 0: fp32 - exact {curves['fp32'][0] - exact[0]:+.3e}, bf16 - rounded {curves['bf16'][0] - rounded[0]:+.3e}")
    assert abs(curves["fp32"][0] - exact[0]) < 2e-5                 # the device's fp32 path is the exact oracle's
    _within("largest loss distance over 20 steps", max(diff), max(yard))


def test_fp32_and_no_key_are_the_same_path_bit_for_bit(tmp_path):
    p32 = lmo.init_params(16, 64, 2, 128, 2, seed=5)
    x, lens = lmo.synthetic_tokens(3, 20, 16, seed=6)
    log_dir, out = None, []
    for over in ({}, dict(compute_dtype="fp32")):
        model, log_dir = B.build(tmp_path, p32, log_dir=log_dir, **dict(B.SMALL, **over))
        assert model.compute_dtype == torch.float32
        model.train()
        logits = model.logits(x.to(DEV), lens.to(DEV, torch.int32))
        model(x.to(DEV), lens.to(DEV), None, None)[0]["loss"].backward()
        out.append((logits.detach(), B.named_grads(model)))
    assert torch.equal(out[0][0], out[1][0])
    for name in out[0][1]:
        if name == "embedding.weight":
            # smt_lm_embed_bwd adds the rows of a repeated token with fp32 atomics, in arrival order: two runs of ONE model
            # differ in the last bits there (tests/test_lm_gpu.py, device-keys test).  A reordered fp32 sum of n <= 60 rows
            # moves an element by at most n * 2^-24 of the sum of the magnitudes, so the tensors agree to 1e-6 in relative L2
            assert B.rel(out[0][1][name], out[1][1][name]) < 1e-6, name
        else:
            assert torch.equal(out[0][1][name], out[1][1][name]), name


def test_decoding_stays_fp32_and_prefill_follows_the_dtype(tmp_path):
    """sample(causal=True) of a bf16 model returns the codes of an fp32 model with the same state dict (the decode kernels read
    the fp32 masters); prefill (bf16 projections) + step_logits (fp32) agrees with the bf16 `logits` on the same prefix within
    the forward band: each is within E of the exact logits, E = the rounded oracle's own error, doubled for the device."""
    p32 = lmo.init_params(16, 64, 2, 128, 2, seed=9)
    m32, log_dir = B.build(tmp_path, p32, **B.SMALL)
    mbf, _ = B.build(tmp_path, None, log_dir=log_dir, **dict(B.SMALL, **BF16))
    mbf.load_state_dict(m32.state_dict())
    assert set(mbf.state_dict()) == set(m32.state_dict()) and all(v.dtype != torch.bfloat16 for v in mbf.state_dict().values())
    m32.eval(), mbf.eval()
    u = torch.rand(10, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    _, q32 = m32.sample(3, 10, device=DEV, causal=True, uniforms=u)
    _, qbf = mbf.sample(3, 10, device=DEV, causal=True, uniforms=u)
    assert torch.equal(q32, qbf)
    # prefill + one step against the full forward, both in bf16
    codes = torch.randint(0, 16, (3, 9), generator=torch.Generator().manual_seed(2))
    tokens = torch.cat([torch.full((3, 1), lmo.BOS), codes + lmo.OFFSET], dim=1)             # <bos> + 9 codes
    with B.oracle_linear(False):
        exact = lmo.lm_logits(tokens, None, {k: v.double() for k, v in p32.items()}, heads=2, num_layers=2)
    with B.oracle_linear(True):
        rounded = lmo.lm_logits(tokens, None, {k: v.double() for k, v in p32.items()}, heads=2, num_layers=2)
    e = float((rounded - exact).abs().max())
    st = mbf.new_decode_state(3, 12, DEV)
    mbf.prefill(st, codes.to(DEV))
    step = mbf.step_logits(st)
    with torch.no_grad():
        full = mbf.logits(tokens.to(DEV), None)[:, 9]
    _within("prefill + step vs logits, max |diff|", float((step - full).abs().max()), 2 * e)
    assert float((full.cpu().double() - exact[:, 9]).abs().max()) <= FACTOR * e
    # the non-causal sampler runs `logits`, so it follows the dtype too: it must simply run
    torch.manual_seed(0)
    _, q = mbf.sample(batch_size=2, n_steps=4, device=DEV)
    assert q.shape == (2, 4) and int(q.min()) >= 0 and int(q.max()) < 16


@pytest.mark.parametrize("key,value", [("d_model", 48), ("dim_feedforward", 80), ("vocab_size", 24)])
def test_constructor_refuses_what_the_kernels_cannot_run(tmp_path, key, value):
    from models.transformer_lm.transformer_lm import TransformerLM
    over = dict(B.SMALL, **{key: value})
    if key == "d_model":
        over.update(embed_dim=48, nhead=3)
    log_dir, _ = B.vqvae_run(tmp_path, l_bins=over["vocab_size"])
    with pytest.raises(ValueError, match=key):
        TransformerLM(B.lm_config(log_dir, **dict(over, **BF16)))
    TransformerLM(B.lm_config(log_dir, **over))                          # fp32 has no such limit
    with pytest.raises(ValueError, match="compute_dtype"):
        TransformerLM(B.lm_config(log_dir, **dict(B.SMALL, compute_dtype="fp16")))


def test_train_py_with_the_bf16_config(tmp_path, monkeypatch):
    """`train.py --model transformer_lm_bf16 --dataset vqlatent` at a small size: two steps, a checkpoint with fp32 tensors
    under the usual keys, and a second run that resumes from it."""
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
    cfg = B.lm_config(log_vq, base="transformer_lm_bf16.yaml", **B.SMALL)
    assert cfg.model.compute_dtype == "bf16"
    C.save(cfg, "configs/models/_test_lm_bf16.yaml")
    vql = C.load("configs/datasets/vqlatent.yaml")
    vql.dataset.update(C.create(dict(dataset_path=dump_dir, segment_length=24)))
    C.save(vql, "configs/datasets/_test_vql_bf16.yaml")
    try:
        log_dir = str(tmp_path / "run")
        argv = ["--model", "_test_lm_bf16", "--dataset", "_test_vql_bf16", "--batch_size", "3", "--num_workers", "0", "--total_epochs", "1",
                "--log_every_n_steps", "1", "--ckpt_every_n_steps", "2", "--eval_every_n_epochs", "1", "--log_dir", log_dir, "--n_gpus", "1"]
        train.main(argv)
        last = torch.load(os.path.join(log_dir, "ckpts", "ckpt.last.pt"), weights_only=True)
        assert last["step"] == 2 and last["extra"]["drop_seed"] == 2
        weights = {k: v for k, v in last["model"].items() if k.startswith(("transformer.", "classifier.", "embedding."))}
        assert "transformer.layers.1.self_attn.in_proj_weight" in weights and all(v.dtype == torch.float32 for v in weights.values())
        assert C.load(os.path.join(log_dir, "config.yaml")).model.compute_dtype == "bf16"
        train.main(argv + ["--load_ckpt", os.path.join(log_dir, "ckpts", "ckpt.last.pt"), "--total_epochs", "2"])
        assert torch.load(os.path.join(log_dir, "ckpts", "ckpt.last.pt"), weights_only=True)["step"] == 4
    finally:
        os.remove("configs/models/_test_lm_bf16.yaml")
        os.remove("configs/datasets/_test_vql_bf16.yaml")
