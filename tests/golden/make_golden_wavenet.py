#!/usr/bin/env python3
"""Generate the WaveNet-block fixtures by IMPORTING THE REFERENCE on the CPU, everything in float64 (`.double()`):

  wavenet_block.npz         the reference's own `WaveNetBlock(16, 3, m_conv=2.0, dilation_growth_rate=3, dilation_cycle=2,
                            zero_out=True)` (models/vqvae/resnet.py:123-181), zeroed gates given signal as `randomize` does:
                            x [2, 16, 40], lens [40, 23], the state dict, y, r, and the gradients of sum(y * r * mask) with
                            respect to x and every parameter.  x, r and the parameters were drawn in fp32 and are stored as
                            float32 without loss; y and the gradients are float64
  vqvae_wavenet_small.npz   the reference `VQVAE` at make_golden.SMALL with block_type="wavenet", m_conv=2.0: the eval-mode
                            supervised_step with a fixed codebook, what make_golden.gen_model (b) stores (losses, yh, every
                            gradient).  The model has 450 k parameters, so the file holds NO parameters: every parameter is
                            set to tests/wavenet_helpers.py::det_uniform(name, shape), a closed-form hash that the test
                            evaluates again, and every gradient tensor is stored as float16 of g / max|g| beside its scale
                            (2^-11 relative per element, against the test's 2e-2 relative L2)
  vqvae_wavenet_keys.json   encoder / decoder state-dict keys and shapes of the full default config at block_type="wavenet"

The harness of make_golden.py is reused (its import sets up the paths, the working directory and the stand-ins).  Nothing of
the reference is changed or copied.  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wavenet.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402  (REF first on sys.path, cwd = REF, librosa stand-in)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.vqvae.resnet import WaveNetBlock  # noqa: E402
from models.vqvae.vqvae import VQVAE  # noqa: E402

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
import wavenet_helpers as WH  # noqa: E402

orc = mg.orc


def gen_block():
    g = torch.Generator().manual_seed(41)
    torch.manual_seed(41)           # the module constructor draws from the GLOBAL generator, as in make_golden.gen_block
    blk = WaveNetBlock(16, 3, m_conv=2.0, dilation_growth_rate=3, dilation_cycle=2, zero_out=True)
    mg.randomize(blk, g)
    blk = blk.double().eval()
    b, t = 2, 40
    x = torch.randn(b, 16, t, generator=g).double().requires_grad_(True)
    r = torch.randn(b, 16, t, generator=g).double()
    lens = torch.tensor([40, 23])
    mask = orc.sequence_mask(lens, t).unsqueeze(1).double()
    y, _ = blk(x, mask)
    (y * r * mask).sum().backward()
    out = {"x": x.detach().float(), "lens": lens, "y": y.detach(), "r": r.float(), "g.x": x.grad}
    out.update({"p." + k: v.float() for k, v in blk.state_dict().items()})
    out.update({"g." + n: p.grad for n, p in blk.named_parameters()})
    assert torch.equal(out["x"].double(), x.detach()) and all(torch.equal(out["p." + k].double(), v)
                                                              for k, v in blk.state_dict().items())
    mg.save("wavenet_block", **out)


def gen_model():
    g = torch.Generator().manual_seed(51)
    over = dict(mg.SMALL, block_type="wavenet", m_conv=2.0)
    cfg = mg.small_loss_cfg(mg.load_cfg(**over))
    torch.manual_seed(5)
    model = VQVAE(cfg)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(WH.det_uniform(n, tuple(p.shape))))
    model = model.double().eval()
    b, t = 3, 2048
    x = mg.synth(b, t, 52).unsqueeze(1).double()
    lens = torch.tensor([2048, 1536, 1024])
    out = {"x": x.float(), "lens": lens}
    mask = orc.sequence_mask(lens, t).unsqueeze(1).double()
    with torch.no_grad():
        z, zm = model.encoders[0](x, mask)
    zf, mf = orc.vq_preprocess(z, zm)
    k0 = zf[(mf != 0)[:, 0]][torch.randperm(int(mf.sum()), generator=g)][:64].clone()
    model.bottleneck.level_blocks[0].k = k0.clone()
    with torch.no_grad():
        codes = model.bottleneck.level_blocks[0].encode(z, zm)
    out.update(k0=k0, enc_codes=codes)
    model.zero_grad()
    loss_dict, metrics = model.supervised_step([None, None, None, None, x, lens, None])
    assert metrics == {}
    loss_dict["loss"].backward()
    for kk in ("loss", "loss_recon", "loss_stft", "loss_commit", "yh"):
        out["eval_" + kk] = loss_dict[kk].detach()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    for n, v in grads.items():
        scale = v.abs().max().clamp_min(1e-300)
        out["eval_g." + n] = (v / scale).to(torch.float16)
        out["eval_s." + n] = scale
    assert any(n.startswith("encoders") for n in grads)
    mg.save("vqvae_wavenet_small", **out)

    full = VQVAE(mg.load_cfg(block_type="wavenet"))
    inv = {k: list(v.shape) for k, v in full.state_dict().items() if k.startswith(("encoders.", "decoders."))}
    path = os.path.join(mg.OUT, "vqvae_wavenet_keys.json")
    with open(path, "w") as f:
        json.dump(inv, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote vqvae_wavenet_keys.json: {len(inv)} keys ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    torch.set_num_threads(8)
    if not hasattr(np, "bool"):
        np.bool = bool
    gen_block()
    gen_model()
