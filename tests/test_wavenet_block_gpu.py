"""The WaveNet block, and the two waveform models built from it, on the GPU: against the fixture captured from the reference's
own ``WaveNetBlock`` (tests/golden/wavenet_block.npz, float64), against the float64 restatement at the width of the product
configuration, and end to end (``VQVAE`` against the reference's eval step, ``train.py``, ``VQTTS``).  Tolerances are the
project's own for a block (tests/test_fastpath_parity_gpu.py): relative L2 <= 2e-5 forward / 2e-2 gradients in fp32,
<= 1e-2 / 7e-2 in bf16."""
import json
import os

import numpy as np
import pytest
import torch

import vqtts_model_helpers as H
import wavenet_helpers as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-masters-thesis_amd")
T = torch.from_numpy
TOL = {torch.float32: (2e-5, 2e-2), torch.bfloat16: (1e-2, 7e-2)}


def _run_block(blk, x, lens, r, dtype, record=False):
    """(y, dx, {name: grad}, region names) of one forward + backward of sum(y * r * mask) in `dtype`."""
    from smt_amd import profiler
    m = W.row_mask(lens, x.shape[1]).to(DEV)
    xa = x.to(DEV).to(dtype).requires_grad_(True)
    blk.zero_grad()
    names = set()
    if record:
        profiler.enable(True)
        profiler.reset()
    try:
        y = blk(xa, lens.to(DEV))
        (y.float() * (r.to(DEV).float() * m.float())).sum().backward()
        if record:
            names = set(profiler._records)
    finally:
        if record:
            profiler.enable(False)
            profiler.reset()
    torch.cuda.synchronize()
    return y.detach().cpu(), xa.grad.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in blk.named_parameters()}, names


def _compare(tag, dtype, m, y, dx, grads, y64, dx64, grads64):
    fwd_tol, grad_tol = TOL[dtype]
    errs = {"y": W.rel_l2(y * m, y64 * m), "dx": W.rel_l2(dx * m, dx64 * m)}
    errs.update({n: W.rel_l2(g, grads64[n]) for n, g in grads.items()})
    print(f"{tag} {dtype}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert set(grads) == set(grads64)
    for k, v in errs.items():
        assert v <= (fwd_tol if k == "y" else grad_tol), (k, v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_block_against_the_reference_fixture(golden, dtype):
    from models.vqvae.resnet import WaveNetBlock
    g = golden("wavenet_block")
    params = {k[2:]: T(v) for k, v in g.items() if k.startswith("p.")}
    blk = WaveNetBlock(16, 3, m_conv=2.0, dilation_growth_rate=3, dilation_cycle=2, zero_out=True).to(DEV).eval()
    blk.load_state_dict(params)
    x, r, lens = T(g["x"]).transpose(1, 2).contiguous(), T(g["r"]).transpose(1, 2).contiguous(), T(g["lens"])
    m = W.row_mask(lens, x.shape[1])
    y, dx, grads, _ = _run_block(blk, x, lens, r, dtype)
    if dtype == torch.float32:
        y64, dx64 = T(g["y"]).transpose(1, 2), T(g["g.x"]).transpose(1, 2)
        grads64 = {k: T(g["g." + k]) for k in params}
    else:                        # on the bf16-rounded fixture inputs: the restatement (which reproduces the fixture to 1e-12)
        p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
        x64 = x.to(dtype).double().requires_grad_(True)
        y64 = W.block64(x64, lens, p64, blk.dilations)
        (y64 * r.double() * m).sum().backward()
        y64, dx64, grads64 = y64.detach(), x64.grad, {k: v.grad for k, v in p64.items()}
    _compare("fixture", dtype, m, y, dx, grads, y64, dx64, grads64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_block_at_the_product_width(dtype):
    """W = 64, depth 4, growth 3 (dilations 1, 3, 9, 27); the third item is shorter than every dilation past the first."""
    from models.vqvae.resnet import WaveNetBlock
    torch.manual_seed(3)
    blk = WaveNetBlock(64, 4, m_conv=1.0, dilation_growth_rate=3, zero_out=False).to(DEV).train()
    assert blk.dilations == [1, 3, 9, 27]
    gen = torch.Generator().manual_seed(4)
    b, t = 3, 300
    lens = torch.tensor([300, 211, 5])
    x, r = torch.randn(b, t, 64, generator=gen), torch.randn(b, t, 64, generator=gen)
    m = W.row_mask(lens, t)
    y, dx, grads, names = _run_block(blk, x, lens, r, dtype, record=True)
    if dtype == torch.bfloat16:
        assert "wavenet_tail" in names
    else:
        assert "wavenet_tail" not in names and "wavenet_gate_fwd" in names
    assert "wavenet_gate_bwd" in names
    p64 = {k: v.detach().double().cpu().requires_grad_(True) for k, v in blk.state_dict().items()}
    x64 = x.to(dtype).double().requires_grad_(True)
    y64 = W.block64(x64, lens, p64, blk.dilations)
    (y64 * r.double() * m).sum().backward()
    _compare("W=64", dtype, m, y, dx, grads, y64.detach(), x64.grad, {k: v.grad for k, v in p64.items()})
    # forward and backward run twice are bit-equal
    y2, dx2, grads2, _ = _run_block(blk, x, lens, r, dtype)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ---- models -----------------------------------------------------------------------------------------------------------------
def _small_config(**model_over):
    from utils import config as C
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/vqvae_wavenet.yaml")),
                  C.load(os.path.join(PKG, "configs/datasets/synthetic_ljspeech.yaml")),
                  C.create({"train": {"batch_size": 3, "n_gpus": 1}}))
    cfg.model.update(C.create(dict(width=16, emb_width=32, l_bins=64, multipliers=[1, 1, 1], m_conv=2.0, dropout=0.0)))
    cfg.model.loss.linf_topk = 128
    cfg.model.update(C.create(model_over))
    return cfg


def test_vqvae_eval_step_matches_the_reference(golden):
    """tests/test_model_gpu.py::test_eval_step_matches_reference on the wavenet fixture, at its tolerances.  The fixture holds no
    parameters: both sides evaluate wavenet_helpers.det_uniform."""
    from models.vqvae.vqvae import VQVAE
    g = golden("vqvae_wavenet_small")
    model = VQVAE(_small_config(l_bins=int(g["k0"].shape[0]))).to(DEV)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(T(W.det_uniform(n, tuple(p.shape))))
    blk = model.bottleneck.level_blocks[0]
    blk.k.copy_(T(g["k0"]).float())
    blk.init = True
    model.eval()
    x, lens = T(g["x"]).to(DEV), T(g["lens"]).to(DEV)
    codes, _ = model.encode_and_quantize(x, lens)
    assert np.array_equal(codes.cpu().numpy(), g["enc_codes"])
    loss_dict, metrics = model.supervised_step([None, None, None, None, x, lens, None])
    assert metrics == {}
    loss_dict["loss"].backward()
    for kk in ("loss", "loss_recon", "loss_stft", "loss_commit"):
        print(kk, loss_dict[kk].item(), float(g["eval_" + kk]))
        assert np.isclose(loss_dict[kk].item(), float(g["eval_" + kk]), rtol=1e-4), kk
    assert torch.allclose(loss_dict["yh"].cpu().double(), T(g["eval_yh"]), atol=5e-5)
    named = dict(model.named_parameters())
    num = den = 0.0
    checked = 0
    for key, v in g.items():
        if key.startswith("eval_g."):
            name = key[len("eval_g."):]
            ref = T(v.astype(np.float64)) * float(g["eval_s." + name])
            got = named[name].grad
            assert got is not None, key
            diff = (got.cpu().double() - ref).norm().item()
            assert diff <= 0.5 * ref.norm().item() + 1e-6, key
            num += diff ** 2
            den += ref.norm().item() ** 2
            checked += 1
    print("gradient tensors", checked, "global relative L2", (num / den) ** 0.5)
    assert checked > 100
    assert (num / den) ** 0.5 <= 2e-2, (num / den) ** 0.5


def test_train_py_trains_and_its_checkpoint_reloads(tmp_path, monkeypatch):
    import train
    from models.vqvae.resnet import WaveNetBlock
    from models.vqvae.vqvae import VQVAE
    from utils import config as C
    monkeypatch.chdir(PKG)
    small = C.load("configs/models/vqvae_wavenet.yaml")
    small.model.update(C.create(dict(width=16, emb_width=32, l_bins=64, multipliers=[1, 1, 1])))
    small.model.loss.linf_topk = 128
    C.save(small, "configs/models/_test_wavenet_small.yaml")
    ds = C.load("configs/datasets/synthetic_ljspeech.yaml")
    ds.dataset.update(C.create(dict(num_clips=4, clip_length=4096, ragged=False)))
    C.save(ds, "configs/datasets/_test_wavenet_small.yaml")
    try:
        log_dir = str(tmp_path / "run")
        argv = ["--model", "_test_wavenet_small", "--dataset", "_test_wavenet_small", "--batch_size", "2", "--num_workers", "0",
                "--total_epochs", "1", "--log_every_n_steps", "1", "--ckpt_every_n_steps", "2", "--eval_every_n_epochs", "100",
                "--log_dir", log_dir, "--n_gpus", "1"]
        train.main(argv)
        last = torch.load(os.path.join(log_dir, "ckpts", "ckpt.last.pt"), weights_only=True)
        assert last["step"] == 2 and last["config"]["model"]["block_type"] == "wavenet"
        assert all(bool(torch.isfinite(v).all()) for v in last["model"].values() if v.is_floating_point())
        scal = os.path.join(log_dir, "scalars.jsonl")
        if os.path.exists(scal):
            losses = [json.loads(line) for line in open(scal)]
            losses = [e["value"] for e in losses if e["tag"] == "loss/train_loss"]
            assert len(losses) == 2 and all(np.isfinite(losses))
        train.main(argv + ["--load_ckpt", os.path.join(log_dir, "ckpts", "ckpt.last.pt")])     # the resume path loads it
        model = VQVAE(C.load("configs/models/_test_wavenet_small.yaml"))
        model.load_state_dict(last["model"])
        assert any(isinstance(mod, WaveNetBlock) for mod in model.modules())
        # the gates were zero at the start (zero_out) and have moved
        assert any(k.endswith("gates.0.weight") and bool(v.any()) for k, v in last["model"].items())
    finally:
        os.remove("configs/models/_test_wavenet_small.yaml")
        os.remove("configs/datasets/_test_wavenet_small.yaml")


def test_vqtts_trains_and_synthesizes_with_the_wavenet_block():
    from models.vqtts import VQTTS
    from models.vqvae.resnet import WaveNetBlock
    from utils import config as C
    d = H.config_dict()
    d["model"]["block_type"] = "wavenet"
    torch.manual_seed(0)
    model = VQTTS(C.create(d)).to(DEV)
    H.randomize_zero_init(model)
    n_blocks = sum(isinstance(m, WaveNetBlock) for m in model.modules())
    assert n_blocks >= 2 and n_blocks % 2 == 0                                     # the encoder's and the decoder's
    x, x_lens, y, y_lens = [t.to(DEV) for t in H.batch()]
    model.train()
    out, metrics = model(x, x_lens, y, y_lens)
    out["loss"].backward()
    assert bool(torch.isfinite(out["loss"])) and bool(torch.isfinite(out["yh"]).all())
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    model.eval()
    wave, wave_lengths = model.infer(x.cpu(), x_lens.cpu())
    assert wave.dtype == torch.float32 and wave.shape[0] == H.B and bool(torch.isfinite(wave).all())
    for b, n in enumerate(wave_lengths.tolist()):
        assert n > 0 and bool((wave[b, n:] == 0).all()) and bool(wave[b, :n].any())
