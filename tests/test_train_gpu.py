"""train.py end to end on the GPU with the synthetic dataset: registry, DataLoader + collate, train loop,
logging, checkpoint write / resume (reference train.py:146-221, 305-383, utils/train_utils.py:148-171)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-masters-thesis_amd")


def test_train_two_epochs_checkpoint_and_resume(tmp_path, monkeypatch):
    import train
    from utils import config as C
    monkeypatch.chdir(PKG)
    small = C.load("configs/models/vqvae.yaml")
    small.model.update(C.create(dict(width=16, emb_width=32, l_bins=64, multipliers=[1, 1, 1])))
    small.model.loss.linf_topk = 128
    C.save(small, "configs/models/_test_small.yaml")
    ds = C.load("configs/datasets/synthetic_ljspeech.yaml")
    ds.dataset.update(C.create(dict(num_clips=6, clip_length=4096, ragged=False)))
    C.save(ds, "configs/datasets/_test_small.yaml")
    try:
        log_dir = str(tmp_path / "run")
        argv = ["--model", "_test_small", "--dataset", "_test_small", "--batch_size", "2", "--num_workers", "0",
                "--total_epochs", "2", "--log_every_n_steps", "1", "--ckpt_every_n_steps", "2",
                "--eval_every_n_epochs", "1", "--log_dir", log_dir, "--ema", "--n_gpus", "1", "--run_sanity_val_epoch"]
        train.main(argv)
        assert os.path.exists(os.path.join(log_dir, "config.yaml"))
        last = torch.load(os.path.join(log_dir, "ckpts", "ckpt.last.pt"), weights_only=True)
        assert last["step"] == 6 and last["epoch"] == 2                   # 6 clips / batch 2 = 3 steps x 2 epochs
        assert "bottleneck.level_blocks.0.k" in last["model"] and last["config"]["model"]["levels"] == 1
        assert os.path.exists(os.path.join(log_dir, "ckpts", "ckpt.2.pt"))
        scal = os.path.join(log_dir, "scalars.jsonl")
        if os.path.exists(scal):                                           # JSON-lines writer when tensorboard is absent
            tags = {json.loads(line)["tag"] for line in open(scal)}
            assert {"loss/train_loss", "metrics/train_fit", "loss/val_loss"} <= tags
        # validation artefacts of a waveform model (reference train_utils.py:249-304): wavs + a log-mel grid per val epoch
        import wave
        for epoch in (0, 1, 2):
            assert open(os.path.join(log_dir, "spect", f"val_spect_{epoch}.png"), "rb").read(8) == b"\x89PNG\r\n\x1a\n"
            for kind in ("gt", "pred"):
                with wave.open(os.path.join(log_dir, "audio", f"val_audio_{epoch}_{kind}.wav")) as w:
                    assert w.getframerate() == 22050 and w.getnframes() == 4096 and w.getsampwidth() == 2
        # resume: total_epochs reached -> no further steps, but the load path runs
        train.main(argv + ["--load_ckpt", os.path.join(log_dir, "ckpts", "ckpt.last.pt")])
    finally:
        os.remove("configs/models/_test_small.yaml")
        os.remove("configs/datasets/_test_small.yaml")


def test_resume_keeps_the_trained_codebook(tmp_path):
    """save -> load -> one train step: the codebook moves by an EMA-sized step instead of being re-drawn from
    the batch (the reference's resume path re-initialises it: bottleneck.py:179 with init lost on load); the dropout
    counter continues; a reference-style checkpoint without the extra entry is kept alive with restore_k()."""
    import train as trainlib
    from oracle import vqvae_oracle as orc
    from utils import config as C
    from utils.commons import get_model, get_optimizer
    from utils.train_utils import save_checkpoint
    root = PKG
    cfg = C.merge(C.load(os.path.join(root, "configs/models/vqvae.yaml")),
                  C.load(os.path.join(root, "configs/datasets/synthetic_ljspeech.yaml")),
                  C.create({"train": {"batch_size": 2, "n_gpus": 1, "ema": True, "grad_clip_norm": None, "seed": 0,
                                      "log_dir": str(tmp_path), "total_epochs": 1}}))
    cfg.model.update(C.create(dict(width=16, emb_width=32, l_bins=64, multipliers=[1, 1, 1])))
    cfg.model.loss.linf_topk = 128
    os.makedirs(tmp_path / "ckpts")
    dev = torch.device("cuda", 0)

    def fresh():
        torch.manual_seed(0)
        m, e = get_model(C.create(cfg.to_dict()), dev)
        o, s = get_optimizer(cfg, m)
        return m, e, o, s

    x = orc.synthetic_clip_batch(2, 8192, 5).cuda()
    lens = torch.tensor([8192, 6144]).cuda()
    batch = [None, None, None, None, x, lens, None]
    model, ema, opt, sched = fresh()
    model.train()
    for step in range(3):
        trainlib.train_step(global_step=step, batch=batch, config=cfg, model=model, ema=ema, optimizer=opt, scheduler=sched,
                            device=dev)
    blk = model.bottleneck.level_blocks[0]
    k_trained, seed_trained = blk.k.clone(), model._drop_seed
    path = save_checkpoint(cfg, 3, 0, model, ema, opt, sched)

    m2, e2, o2, s2 = fresh()
    step, epoch = trainlib.load_checkpoint(path, m2, o2, s2, e2, dev)
    b2 = m2.bottleneck.level_blocks[0]
    assert (step, epoch) == (3, 0) and b2.init and m2._drop_seed == seed_trained
    assert torch.equal(b2.k, k_trained) and torch.equal(b2.k_sum, blk.k_sum) and torch.equal(b2.k_elem, blk.k_elem)
    m2.train()
    torch.manual_seed(123)        # dead codes are revived from RANDOM rows of the batch: same draw for both runs
    trainlib.train_step(global_step=3, batch=batch, config=cfg, model=m2, ema=e2, optimizer=o2, scheduler=s2, device=dev)
    torch.manual_seed(123)
    trainlib.train_step(global_step=3, batch=batch, config=cfg, model=model, ema=ema, optimizer=opt, scheduler=sched, device=dev)
    # the resumed run continues exactly like the uninterrupted one (same dropout seed, same accumulators) ...
    assert torch.allclose(b2.k, blk.k, atol=1e-6) and torch.allclose(b2.k_sum, blk.k_sum, atol=1e-5)
    # ... and the codebook moved by an EMA-sized step, it was not re-drawn
    alive = b2.k_elem >= b2.threshold                  # revived rows jump to fresh data rows by design
    moved = (b2.k - k_trained)[alive].norm() / k_trained[alive].norm()
    assert alive.any() and 0 < moved < 0.2, moved

    # a checkpoint without the extra entry (what the reference writes)
    ck = torch.load(path, weights_only=True)
    ck.pop("extra")
    torch.save(ck, tmp_path / "ckpts" / "ckpt.ref.pt")
    m3, e3, o3, s3 = fresh()
    trainlib.load_checkpoint(str(tmp_path / "ckpts" / "ckpt.ref.pt"), m3, o3, s3, e3, dev)
    b3 = m3.bottleneck.level_blocks[0]
    assert b3.init and torch.equal(b3.k, k_trained) and torch.equal(b3.k_sum, k_trained) and bool((b3.k_elem == 1).all())


def test_device_keys_and_graphed_step_reproduce_the_eager_vqvae_step(tmp_path):
    """dropout keys from device memory + forward/backward in a hipGraph, on a small bf16 VQ-VAE (dropout
    on, ragged).  The train step being bit-reproducible, three optimizer steps with keys by value, with keys from the device
    and with graph replays must give bit-identical losses -- same masks, same kernels, same weights all the way."""
    from oracle import vqvae_oracle as orc
    from smt_amd.graph import GraphedStep
    from utils import config as C
    from utils.commons import get_model, get_optimizer
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/vqvae.yaml")),
                  C.load(os.path.join(PKG, "configs/datasets/synthetic_ljspeech.yaml")),
                  C.create({"train": {"batch_size": 2, "n_gpus": 1, "ema": False, "grad_clip_norm": None, "seed": 0,
                                      "log_dir": str(tmp_path), "total_epochs": 1}}))
    cfg.model.update(C.create(dict(width=64, emb_width=128, l_bins=64, multipliers=[1, 1, 1], compute_dtype="bf16")))
    cfg.model.loss.linf_topk = 128
    cfg.model.revival_threshold = 0.0     # no code counts as dead: revival rows come from torch's generator, whose stream of
    dev = torch.device("cuda", 0)         # draws a captured graph does not share with the eager runs it is compared with
    x = orc.synthetic_clip_batch(2, 16384, 5).cuda()
    lens = torch.tensor([16384, 12288]).cuda()
    batch = [None, None, None, None, x, lens, None]

    def run(mode):
        torch.manual_seed(0)
        model, _ = get_model(C.create(cfg.to_dict()), dev)
        opt, sched = get_optimizer(cfg, model)
        model.train()
        first, _ = model.supervised_step(batch)   # the first forward initialises the codebook from the batch (host-side branch)
        first["loss"].backward()                  # ... and the first backward creates the packed data-gradient weights
        del first
        opt.zero_grad(set_to_none=True)
        model._drop_seed = 50
        graph = None
        if mode == "device":
            model.enable_device_keys(True)
        if mode == "graph":
            graph = GraphedStep(model, lambda *slots: model.supervised_step(list(slots)), batch,
                                lambda: opt.zero_grad(set_to_none=True), warmup=0)
        losses = []
        for _ in range(3):
            if graph is not None:
                loss_dict, _ = graph.replay(*batch)
            else:
                opt.zero_grad(set_to_none=True)
                loss_dict, _ = model.supervised_step(batch)
                loss_dict["loss"].backward()
            opt.step(); sched.step()
            losses.append(float(loss_dict["loss"].detach()))
            del loss_dict
        return losses, model._drop_seed, (int(model._seed_dev) if model._seed_dev is not None else None)

    by_value, seed_v, _ = run("value")
    from_device, seed_d, dev_d = run("device")
    graphed, seed_g, dev_g = run("graph")
    assert seed_v == seed_d == dev_d == seed_g == dev_g == 53 and len(set(by_value)) == 3
    assert from_device == by_value, (from_device, by_value)
    assert graphed == by_value, (graphed, by_value)


def test_vqvae_train_steps_are_bit_reproducible(tmp_path):
    """Two runs of three full train steps (bf16 conv stacks, dropout on, ragged lengths, codebook EMA + revival, AdamW) from
    the same seeds end with bit-identical losses, parameters and codebook: nothing on the step accumulates in floating point
    in arrival order any more (weight-gradient slabs are reduced in a fixed order, the codebook statistics in 64-bit fixed
    point, the spectral loss's overlap-add is a gather)."""
    import train as trainlib
    from oracle import vqvae_oracle as orc
    from utils import config as C
    from utils.commons import get_model, get_optimizer
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/vqvae.yaml")),
                  C.load(os.path.join(PKG, "configs/datasets/synthetic_ljspeech.yaml")),
                  C.create({"train": {"batch_size": 3, "n_gpus": 1, "ema": False, "grad_clip_norm": None, "seed": 0,
                                      "log_dir": str(tmp_path), "total_epochs": 1}}))
    cfg.model.update(C.create(dict(width=64, emb_width=128, l_bins=256, multipliers=[1, 1, 1], compute_dtype="bf16")))
    cfg.model.loss.linf_topk = 256
    dev = torch.device("cuda", 0)
    x = orc.synthetic_clip_batch(3, 32768, 9).cuda()
    lens = torch.tensor([32768, 20000, 27001]).cuda()
    batch = [None, None, None, None, x, lens, None]

    def run():
        torch.manual_seed(3)
        model, ema = get_model(C.create(cfg.to_dict()), dev)
        opt, sched = get_optimizer(cfg, model)
        model.train()
        losses = []
        for step in range(3):
            loss_dict, _ = trainlib.train_step(global_step=step, batch=batch, config=cfg, model=model, ema=ema, optimizer=opt,
                                               scheduler=sched, device=dev)
            losses.append(float(loss_dict["loss"].detach()))
        blk = model.bottleneck.level_blocks[0]
        return losses, [p.detach().clone() for p in model.parameters()], blk.k.clone(), blk.k_sum.clone()

    l1, p1, k1, s1 = run()
    l2, p2, k2, s2 = run()
    assert l1 == l2, (l1, l2)
    assert torch.equal(k1, k2) and torch.equal(s1, s2)
    assert all(torch.equal(a, b) for a, b in zip(p1, p2))



def test_packed_conv_weights_follow_the_optimizer(tmp_path):
    """Regression (round 2): fused AdamW does not move Tensor._version, so a cache keyed on versions alone kept the
    convolutions on the weights of step 0.  Three eager train steps must equal three steps with the packed copies thrown
    away before every forward, bit for bit (the step is reproducible), and the loss must actually move."""
    import train as trainlib
    from oracle import vqvae_oracle as orc
    from smt_amd import packing
    from utils import config as C
    from utils.commons import get_model, get_optimizer
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/vqvae.yaml")),
                  C.load(os.path.join(PKG, "configs/datasets/synthetic_ljspeech.yaml")),
                  C.create({"train": {"batch_size": 2, "n_gpus": 1, "ema": False, "grad_clip_norm": None, "seed": 0,
                                      "log_dir": str(tmp_path), "total_epochs": 1}}))
    cfg.model.update(C.create(dict(width=64, emb_width=128, l_bins=64, multipliers=[1, 1, 1], compute_dtype="bf16")))
    cfg.model.loss.linf_topk = 128
    dev = torch.device("cuda", 0)
    x = orc.synthetic_clip_batch(2, 16384, 5).cuda()
    lens = torch.tensor([16384, 12288]).cuda()
    batch = [None, None, None, None, x, lens, None]

    def run(invalidate):
        torch.manual_seed(0)
        model, ema = get_model(C.create(cfg.to_dict()), dev)
        opt, sched = get_optimizer(cfg, model)
        model.train()
        losses = []
        for step in range(3):
            if invalidate:
                packing.invalidate()
            loss_dict, _ = trainlib.train_step(global_step=step, batch=batch, config=cfg, model=model, ema=ema, optimizer=opt,
                                               scheduler=sched, device=dev)
            losses.append(float(loss_dict["loss"].detach()))
        return losses

    plain, fresh_packs = run(False), run(True)
    assert plain == fresh_packs, (plain, fresh_packs)
    assert abs(plain[1] - plain[0]) > 1e-3 * abs(plain[0])          # the first update is visible in the second loss


def test_an_optimizer_built_by_the_caller_trains_the_same_weights(tmp_path):
    """correctness of the packed conv weights is a property of the model, not a contract with
    get_optimizer.  Three train steps with a plain ``torch.optim.AdamW(model.parameters(), fused=True)`` built HERE -- the way
    the reference's utils/commons.get_optimizer (commons.py:126-134) or a notebook would -- equal three steps through this
    build's get_optimizer bit for bit, and so do three steps whose parameters are moved by a raw ``p.data`` write that no
    hook and no version counter can see."""
    from oracle import vqvae_oracle as orc
    from smt_amd import packing
    from utils import config as C
    from utils.commons import get_model, get_optimizer
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/vqvae.yaml")),
                  C.load(os.path.join(PKG, "configs/datasets/synthetic_ljspeech.yaml")),
                  C.create({"train": {"batch_size": 2, "n_gpus": 1, "ema": False, "grad_clip_norm": None, "seed": 0,
                                      "log_dir": str(tmp_path), "total_epochs": 1}}))
    cfg.model.update(C.create(dict(width=64, emb_width=128, l_bins=64, multipliers=[1, 1, 1], compute_dtype="bf16")))
    cfg.model.loss.linf_topk = 128
    dev = torch.device("cuda", 0)
    x = orc.synthetic_clip_batch(2, 16384, 5).cuda()
    lens = torch.tensor([16384, 12288]).cuda()
    batch = [None, None, None, None, x, lens, None]

    def run(mode):
        torch.manual_seed(0)
        model, _ = get_model(C.create(cfg.to_dict()), dev)
        if mode == "factory":
            opt, _ = get_optimizer(cfg, model)
        else:
            o = cfg.optimizer
            opt = torch.optim.AdamW(model.parameters(), lr=float(o.lr), betas=tuple(float(b) for b in o.betas),
                                    weight_decay=float(o.weight_decay), eps=float(o.eps), fused=True)
        model.train()
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss_dict, _ = model.supervised_step(batch)
            loss_dict["loss"].backward()
            if mode == "raw":                 # the update applied behind torch's back: p.data, no version bump, no hook
                shadow = [p.detach().clone() for p in model.parameters()]
                opt.step()
                new = [p.detach().clone() for p in model.parameters()]
                for p, old in zip(model.parameters(), shadow):
                    p.data.copy_(old)
                packing._is_dirty(clear=True)           # pretend nobody told the cache anything
                for p, n in zip(model.parameters(), new):
                    p.data.copy_(n)
                packing._is_dirty(clear=True)
            else:
                opt.step()
            losses.append(float(loss_dict["loss"].detach()))
        return losses, [p.detach().clone() for p in model.parameters()]

    (l_fac, p_fac), (l_own, p_own), (l_raw, p_raw) = run("factory"), run("own"), run("raw")
    assert l_own == l_fac and l_raw == l_fac, (l_fac, l_own, l_raw)
    assert all(torch.equal(a, b) for a, b in zip(p_fac, p_own)) and all(torch.equal(a, b) for a, b in zip(p_fac, p_raw))
    assert abs(l_fac[1] - l_fac[0]) > 1e-3 * abs(l_fac[0])          # the first update is visible in the second loss


def test_graphed_step_refuses_a_stale_autograd_graph_and_survives_ema_swaps(tmp_path):
    """GraphedStep raises instead of taking the process down.  Specification = the failure recorded in
    round 2 (gpurun_out/amdlog.txt: a live loss of an earlier eager iteration pins the AccumulateGrad nodes to the default
    stream; hipStreamEndCapture segfaults).  ADVICE r02: the graph holds raw pointers into the packed conv weights, and
    EMA.swap (validation in train.py) / load_checkpoint used to throw those copies away: now they only mark them stale, the
    captured repack refreshes them on the next replay, and replay -> swap, swap -> replay equals replay -> replay bit for bit."""
    from oracle import vqvae_oracle as orc
    from smt_amd.graph import GraphedStep
    from utils import config as C
    from utils.commons import get_model, get_optimizer
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/vqvae.yaml")),
                  C.load(os.path.join(PKG, "configs/datasets/synthetic_ljspeech.yaml")),
                  C.create({"train": {"batch_size": 2, "n_gpus": 1, "ema": True, "grad_clip_norm": None, "seed": 0,
                                      "log_dir": str(tmp_path), "total_epochs": 1}}))
    cfg.model.update(C.create(dict(width=64, emb_width=128, l_bins=64, multipliers=[1, 1, 1], compute_dtype="bf16")))
    cfg.model.loss.linf_topk = 128
    cfg.model.revival_threshold = 0.0
    dev = torch.device("cuda", 0)
    x = orc.synthetic_clip_batch(2, 16384, 5).cuda()
    lens = torch.tensor([16384, 12288]).cuda()
    batch = [None, None, None, None, x, lens, None]

    def run(swaps, hold_stale):
        torch.manual_seed(0)
        model, ema = get_model(C.create(cfg.to_dict()), dev)
        opt, sched = get_optimizer(cfg, model)
        model.train()
        first, _ = model.supervised_step(batch)
        first["loss"].backward()
        opt.zero_grad(set_to_none=True)

        def build():
            return GraphedStep(model, lambda *slots: model.supervised_step(list(slots)), batch,
                               lambda: opt.zero_grad(set_to_none=True), warmup=0)
        if hold_stale:
            # first["yh"] is the decoder's output: its grad_fn keeps the whole graph of that iteration alive
            with pytest.raises(RuntimeError, match="autograd graph of an earlier iteration"):
                build()
        del first
        graph = build()
        losses = []
        for step in range(3):
            losses.append(float(graph.replay(*batch)[0]["loss"]))
            opt.step(); sched.step(); ema.step()
            if swaps and step == 0:
                ema.swap(); ema.swap()               # validation between two train steps: parameters out and back in
        return losses

    plain, swapped = run(False, True), run(True, False)
    assert plain == swapped, (plain, swapped)
    assert len(set(plain)) == 3                      # the optimizer steps in between are visible


def test_training_on_one_batch_drives_the_loss_down(tmp_path):
    """End-to-end sanity that the optimizer's updates reach every kernel: 60 train steps on one ragged batch (bf16 conv
    stacks, dropout on, AdamW) must cut the training loss by a large factor -- measured: 4193 -> 1930, the spectral term
    dominating.  (With stale packed conv weights -- the bug fixed in round 2 -- it stayed within 1 % of its starting value.)"""
    import train as trainlib
    from oracle import vqvae_oracle as orc
    from utils import config as C
    from utils.commons import get_model, get_optimizer
    cfg = C.merge(C.load(os.path.join(PKG, "configs/models/vqvae.yaml")),
                  C.load(os.path.join(PKG, "configs/datasets/synthetic_ljspeech.yaml")),
                  C.create({"train": {"batch_size": 3, "n_gpus": 1, "ema": False, "grad_clip_norm": None, "seed": 0,
                                      "log_dir": str(tmp_path), "total_epochs": 1}}))
    cfg.model.update(C.create(dict(width=64, emb_width=128, l_bins=256, multipliers=[1, 1, 1], compute_dtype="bf16")))
    cfg.model.loss.linf_topk = 256
    dev = torch.device("cuda", 0)
    x = orc.synthetic_clip_batch(3, 32768, 9).cuda()
    lens = torch.tensor([32768, 20000, 27001]).cuda()
    batch = [None, None, None, None, x, lens, None]
    torch.manual_seed(0)
    model, ema = get_model(cfg, dev)
    opt, sched = get_optimizer(cfg, model)
    model.train()
    history = []
    for step in range(60):
        loss_dict, _ = trainlib.train_step(global_step=step, batch=batch, config=cfg, model=model, ema=ema, optimizer=opt,
                                           scheduler=sched, device=dev)
        history.append(float(loss_dict["loss"].detach()))
    assert min(history[-5:]) < 0.6 * history[0], (history[0], history[-5:])


def test_bf16_training_trajectory_tracks_the_fp32_path(tmp_path):
    """the headline path (bf16 conv stacks) against the fp32 parity path as a TRAINING TRAJECTORY, not
    one step: 20 train steps from the same seeds (same initial weights, same batches, same dropout masks, same revival draws),
    width 64 / codebook 256, ragged lengths, dropout on, AdamW.  Stated bands (measured in round 3: 6.9 % at step 0, 1.7 %
    at step 19; reconstruction 1.1 %): total loss within 8 % at every step -- the log-spectral term of an UNTRAINED decoder is
    the ill-conditioned one: it starts 7 % apart and the two curves close in as the decoder learns --
    and within 3 % over the last five steps; reconstruction loss within 2 % throughout; both runs train.  Code usage: index by
    index the two histograms are unrelated this early (the encoder starts as a near-constant map, so its codes are nearly
    coincident points and which one wins is decided by the last bits), so the comparison is distributional: the perplexity
    of the code usage and the number of codes in use agree within a factor 1.5."""
    import train as trainlib
    from oracle import vqvae_oracle as orc
    from utils import config as C
    from utils.commons import get_model, get_optimizer
    base = C.merge(C.load(os.path.join(PKG, "configs/models/vqvae.yaml")),
                   C.load(os.path.join(PKG, "configs/datasets/synthetic_ljspeech.yaml")),
                   C.create({"train": {"batch_size": 3, "n_gpus": 1, "ema": False, "grad_clip_norm": None, "seed": 0,
                                       "log_dir": str(tmp_path), "total_epochs": 1}}))
    base.model.update(C.create(dict(width=64, emb_width=128, l_bins=256, multipliers=[1, 1, 1])))
    base.model.loss.linf_topk = 256
    dev = torch.device("cuda", 0)
    pool = [(orc.synthetic_clip_batch(3, 32768, 40 + i).cuda(), torch.tensor([32768, 20000 + 512 * i, 27001]).cuda())
            for i in range(4)]

    def run(dtype):
        cfg = C.create(base.to_dict())
        cfg.model.compute_dtype = dtype
        torch.manual_seed(3)
        model, ema = get_model(cfg, dev)
        opt, sched = get_optimizer(cfg, model)
        model.train()
        torch.manual_seed(11)                        # the revival rows come from torch's generator: same stream for both runs
        hist, codes = [], None
        for step in range(20):
            x, lens = pool[step % len(pool)]
            loss_dict, metrics = trainlib.train_step(global_step=step, batch=[None, None, None, None, x, lens, None], config=cfg,
                                                     model=model, ema=ema, optimizer=opt, scheduler=sched, device=dev)
            hist.append({k: float(v) for k, v in loss_dict.items() if k.startswith("loss")} | {"usage": float(metrics["usage"])})
        model.eval()
        with torch.no_grad():
            codes, z_lens = model.encode_and_quantize(*pool[0])
        keep = torch.arange(codes.shape[1], device=dev)[None, :] < z_lens[:, None]
        usage = torch.bincount(codes[keep].reshape(-1), minlength=256).float()
        return hist, usage / usage.sum(), model.bottleneck.level_blocks[0].k.clone()

    h32, u32, k32 = run("fp32")
    h16, u16, k16 = run("bf16")
    worst = {k: max(abs(a[k] - b[k]) / abs(b[k]) for a, b in zip(h16, h32)) for k in ("loss", "loss_recon", "loss_stft")}
    late = max(abs(a["loss"] - b["loss"]) / abs(b["loss"]) for a, b in zip(h16[-5:], h32[-5:]))

    def perplexity(u):
        u = u[u > 0]
        return float(torch.exp(-(u * u.log()).sum()))
    px32, px16, n32, n16 = perplexity(u32), perplexity(u16), int((u32 > 0).sum()), int((u16 > 0).sum())
    print(f"\n[bf16 vs fp32, 20 steps] worst relative loss gaps {worst}, last five steps {late:.4f}; usage perplexity fp32 {px32:.1f} "
          f"bf16 {px16:.1f}, codes in use {n32} / {n16}; codebook rel-L2 {float((k16 - k32).norm() / k32.norm()):.3e}\n"
          f"  fp32 loss {[round(h['loss'], 1) for h in h32]}\n  bf16 loss {[round(h['loss'], 1) for h in h16]}")
    assert h32[-1]["loss"] < 0.9 * h32[0]["loss"]                      # both runs train ...
    assert h16[-1]["loss"] < 0.9 * h16[0]["loss"]
    assert worst["loss"] <= 0.08 and late <= 0.03 and worst["loss_recon"] <= 0.02, (worst, late)   # ... along the same curve
    assert 1 / 1.5 <= px16 / px32 <= 1.5 and 1 / 1.5 <= n16 / max(n32, 1) <= 1.5, (px32, px16, n32, n16)
