#!/usr/bin/env python3
"""Generate tests/golden/glow_tts_speakers.npz by running THE REFERENCE's own multi-speaker GlowTTS (glow_tts.py:12-131 with
`n_speakers` > 1) on CPU: the small configuration of `gen_glow_tts` in make_golden.py plus n_speakers = 4, gin_channels = 16
(H + gin = 80, so the duration predictor's first convolution runs at 128 input channels with 48 zero columns).  The harness of
make_golden.py is reused (its import sets up the paths, the working directory and the stand-ins).  Run from the repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_glow_speakers.py

As written the reference cannot run its multi-speaker path; two repairs are made here, in memory, and nothing else is changed:
  * `self.emb_g(speaker)` of a [B] tensor is [B, gin], while `cond_layer` (a Conv1d) and `speaker_embeddings.expand(-1, -1, T)`
    need [B, gin, 1]: `emb_g` is replaced by an nn.Embedding subclass (same weight) whose forward appends that axis;
  * `CouplingBlock.__init__` (submodules.py:372) builds `WN(hidden_channels, kernel_size, dilation_rate, n_layers)` and passes on
    neither `gin_channels` nor `p_dropout`, so no `cond_layer` exists and `WN.forward` fails on it: every coupling block's `wn`
    is rebuilt as the reference's own `WN(..., p_dropout=0, gin_channels=gin)`.
Every parameter is perturbed as `gen_glow_tts` does (the zero-initialised `end` convolutions would otherwise give `cond_layer` no
gradient), every dropout is 0.  speaker = [2, 0, 2]: one speaker twice, speakers 1 and 3 absent (their rows of
`emb_g.weight.grad` are exactly zero).  Captured: the batch, the losses, every parameter and gradient, the eval-mode
reconstruction with its noise, and the reconstruction of the same tokens and noise under a second speaker vector -- all of
it from the reference run in float64 (see the comment in `main`); the noise is a float64 draw whose float32 rounding is stored.

Size: 390 k parameters and as many gradients are 3 MB in float32.  The perturbed parameters are therefore ROUNDED TO
float16-REPRESENTABLE VALUES BEFORE the reference runs, and stored as float16 without loss: the reference computed everything
here from exactly the stored values.  The gradients go to a second file, glow_tts_speakers_grads.npz, as float16 of
grad / max|grad| per tensor with the scale beside it (`gscale.<name>`): 11 significant bits, a relative L2 error of about
1.5e-4 per tensor, which the test's 2e-3 bound absorbs by being that much stricter on the product; exact zeros stay exact."""
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402  (REF first on sys.path, cwd = REF, librosa / np.bool stand-ins)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

N_SPEAKERS, GIN = 4, 16
SPEAKER, SPEAKER_2 = [2, 0, 2], [1, 3, 0]


class EmbG(nn.Embedding):
    """The first repair: [B] ids -> [B, gin, 1]."""

    def forward(self, ids):
        return super().forward(ids).unsqueeze(-1)


def main():
    from oracle import glow_oracle as go
    if not hasattr(np, "bool"):
        np.bool = bool
    parser = types.ModuleType("models.parser")
    parser.CMUDictParser = lambda path: None
    sys.modules.setdefault("models.parser", parser)
    import models.glow_tts.glow_tts as ref_glow
    import models.glow_tts.submodules as ref_sub

    enc, dec = dict(go.GOLDEN_CFG["encoder"]), dict(go.GOLDEN_CFG["decoder"])
    assert enc["p_dropout"] == 0.0 and dec["p_dropout"] == 0.0
    cfg = mg.wrap({"model": dict(n_speakers=N_SPEAKERS, gin_channels=GIN, encoder=enc, decoder=dec),
                   "dataset": dict(n_mels=8, intersperse_blanks=False, cmudict_path="")})
    torch.manual_seed(131)
    model = ref_glow.GlowTTS(cfg)
    emb = EmbG(N_SPEAKERS, GIN)
    emb.weight = model.emb_g.weight
    model.emb_g = emb
    for f in model.decoder.flows:
        if isinstance(f, ref_sub.CouplingBlock):                  # the second repair
            f.wn = ref_sub.WN(dec["hidden_channels"], dec["kernel_size"], dec["dilation_rate"], dec["n_layers"], p_dropout=0,
                              gin_channels=GIN)
    g = torch.Generator().manual_seed(132)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            prm.add_(torch.randn(prm.shape, generator=g) * (0.05 if ".end." in name or ".proj." in name else 0.02))
            prm.copy_(prm.half().float())                            # float16-representable: stored without loss
    assert all(torch.isfinite(p).all() for p in model.parameters())
    model.encoder.pre.relu_drop[1].p = 0.0                        # nn.Dropout(0.1) whatever p_dropout says (modules.py:62)
    tokens, x_lens, y, y_lens = go.synthetic_batch(3, 11, 46, 20, 8, seed=133)
    speaker, speaker_2 = torch.tensor(SPEAKER), torch.tensor(SPEAKER_2)

    # The reference runs twice on the same parameters: in float32, as it ships, and in float64 (`model.double()`, nothing
    # else changed).  The float64 run is what is stored.  The float32 run's own rounding is too large for the test's bound on
    # one tensor: the key bias of an attention layer has an exactly zero gradient (softmax is invariant to a constant added
    # to all keys' scores), float32 returns 8.6e-8 for `encoder.attn_layers.1.conv_k.bias`, and against the test's floor of
    # 1e-6 * (the largest gradient norm, 42.6) that noise alone is a relative error of 2.02e-3 -- above the 2e-3 bound for a
    # product that computed the exact value.  The two runs must agree with each other to fp32 accuracy (asserted below).
    model.train()
    l32, _ = model(tokens, x_lens, y, y_lens, speaker=speaker)
    l32["loss"].backward()
    g32 = {n: p.grad.detach().clone().double() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    model.double()
    y = y.double()
    loss_dict, _ = model(tokens, x_lens, y, y_lens, speaker=speaker)
    loss_dict["loss"].backward()
    assert torch.isfinite(loss_dict["loss_mle"]) and torch.isfinite(loss_dict["loss_length"])
    assert abs(l32["loss_mle"].item() - loss_dict["loss_mle"].item()) < 1e-5 * abs(loss_dict["loss_mle"].item())
    assert abs(l32["loss_length"].item() - loss_dict["loss_length"].item()) < 1e-5 * abs(loss_dict["loss_length"].item())
    gmax = max(float(p.grad.norm()) for p in model.parameters())
    worst = max((float((g32[n] - p.grad).norm() / (p.grad.norm() + 1e-6 * gmax)), n) for n, p in model.named_parameters())
    print("  float32 run against the float64 run: loss_mle", l32["loss_mle"].item() - loss_dict["loss_mle"].item(), "worst gradient rel-L2", worst)
    assert worst[0] < 2.5e-3, worst
    params = {k: v.detach().clone().float() for k, v in model.state_dict().items()}
    assert all(torch.equal(v.double(), model.state_dict()[k]) for k, v in params.items())
    grads = {"grad." + k: v.grad.detach().clone() for k, v in model.named_parameters()}
    assert all(torch.isfinite(v).all() for v in grads.values())
    eg = grads["grad.emb_g.weight"]
    assert (eg[[1, 3]] == 0).all() and (eg[[0, 2]].abs().sum(1) > 0).all(), "emb_g rows: only the speakers present have a gradient"
    assert all(float(grads[f"grad.decoder.flows.{k}.wn.cond_layer.weight_v"].abs().max()) > 0 for k in (2, 5))
    assert tuple(params["encoder.proj_w.conv_1.weight"].shape) == (enc["filter_channels"], enc["hidden_channels"] + GIN, enc["kernel_size"])
    print("  loss_mle", loss_dict["loss_mle"].item(), "loss_length", loss_dict["loss_length"].item())
    print("  state-dict names with the speaker:", sorted(k for k in params if "emb_g" in k or "cond_layer" in k))

    model.eval()
    draws, randn_like = [], torch.randn_like

    def capture_randn_like(t, *a, **k):                           # the one draw of an eval-mode forward (glow_tts.py:114)
        draws.append(randn_like(t, *a, **k))
        return draws[-1]
    torch.randn_like = capture_randn_like
    try:
        with torch.no_grad():
            torch.manual_seed(134)
            ev, _ = model(tokens, x_lens, y, y_lens, speaker=speaker)
            torch.manual_seed(134)
            ev2, _ = model(tokens, x_lens, y, y_lens, speaker=speaker_2)
    finally:
        torch.randn_like = randn_like
    assert len(draws) == 2 and draws[0].shape == (3, 8, 46) and torch.equal(draws[0], draws[1])
    noise = draws[0]
    assert ev["yh"].shape == ev2["yh"].shape == (3, 8, 46), (ev["yh"].shape, ev2["yh"].shape)
    print("  eval yh", tuple(ev["yh"].shape), "second speaker vector: max |difference|", float((ev["yh"] - ev2["yh"]).abs().max()))
    assert float((ev["yh"] - ev2["yh"]).abs().max()) > 1e-2
    assert all(torch.equal(v, v.half().float()) for k, v in params.items())
    mg.save("glow_tts_speakers", tokens=tokens, x_lens=x_lens, y=y, y_lens=y_lens, speaker=speaker, speaker_2=speaker_2,
            loss_mle=loss_dict["loss_mle"].detach(), loss_length=loss_dict["loss_length"].detach(), eval_yh=ev["yh"].float(),
            eval_noise=noise.float(), eval_yh_2=ev2["yh"].float(), eval_loss_mle_2=ev2["loss_mle"], **{"param." + k: v.half() for k, v in params.items()})
    packed = {}
    for k, v in grads.items():
        scale = float(v.abs().max()) or 1.0
        packed[k], packed["gscale." + k[len("grad."):]] = (v / scale).half(), np.float64(scale)
        back = packed[k].double() * scale
        assert float((back - v.double()).norm()) <= 3e-4 * float(v.double().norm()), k
    mg.save("glow_tts_speakers_grads", **packed)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
