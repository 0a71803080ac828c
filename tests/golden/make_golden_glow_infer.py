#!/usr/bin/env python3
"""Generate tests/golden/glow_tts_infer.npz by running THE REFERENCE's own `GlowTTS.infer_step` (glow_tts.py:133-168) on CPU,
with the parameters of tests/golden/glow_tts.npz (oracle.glow_oracle.GOLDEN_CFG: mean_only false, so x_logs is used).  The
harness of make_golden.py is reused (its import sets up the paths, the working directory and the stand-ins).  Run from the
repo root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_glow_infer.py

As written the reference cannot run `infer_step`, and three things are supplied in memory; nothing else is changed:
  * the text front end: `CMUDictParser` needs inflect / unidecode and a dictionary file.  The parser is replaced by a stub that
    returns the fixture utterance's token ids (the ids the parser would emit);
  * `sequence_mask` (submodules.py:18-25) is handed a Python int at glow_tts.py:158-159 (`int(z_lengths // n_sqz) * n_sqz`) and
    calls `.max()` on it: a shim wraps an int in a one-element tensor;
  * `self.device` (glow_tts.py:144) is read but never defined: the attribute is set to cpu.
Captured per utterance i: tokens_i, the durations w_i (the argument of generate_path), z_len_i, the one randn_like draw eps_i
and yh_i.  The script asserts that no valid token's exp(logw) lies within 1e-3 of an integer, so that the fp32 rounding of
a different exp cannot flip a ceil; `logw_bias_offset` (added to the duration predictor's output bias) stays 0 while that
holds."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402  (REF first on sys.path, cwd = REF, librosa / np.bool stand-ins)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import types  # noqa: E402

LOGW_BIAS_OFFSET = 0.0
MARGIN = 1e-3


def main():
    from oracle import glow_oracle as go
    if not hasattr(np, "bool"):
        np.bool = bool
    parser = types.ModuleType("models.parser")
    parser.CMUDictParser = lambda path: None
    sys.modules.setdefault("models.parser", parser)
    import models.glow_tts.glow_tts as ref_glow
    import models.glow_tts.submodules as ref_sub

    g = np.load(os.path.join(mg.OUT, "glow_tts.npz"))
    params = {k[len("param."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}
    params["encoder.proj_w.proj.bias"] = params["encoder.proj_w.proj.bias"] + LOGW_BIAS_OFFSET
    cfg = mg.wrap({"model": dict(n_speakers=1, gin_channels=0, encoder=dict(go.GOLDEN_CFG["encoder"]),
                                 decoder=dict(go.GOLDEN_CFG["decoder"])),
                   "dataset": dict(n_mels=8, intersperse_blanks=False, cmudict_path="")})
    model = ref_glow.GlowTTS(cfg)
    missing, unexpected = model.load_state_dict(params, strict=True)
    assert not missing and not unexpected
    model.device = torch.device("cpu")
    model.eval()

    seq_mask = ref_sub.sequence_mask
    ref_sub.sequence_mask = lambda length, max_length=None: seq_mask(
        torch.tensor([length]) if isinstance(length, int) else length, max_length)
    seen = {}
    gen_path = ref_sub.generate_path

    def generate_path(duration, mask):
        seen["w"], seen["z_len"] = duration.detach().clone(), mask.shape[-1]
        return gen_path(duration, mask)
    ref_sub.generate_path = generate_path
    randn_like = torch.randn_like

    def capture_randn_like(t, *a, **k):
        e = randn_like(t, *a, **k)
        seen.setdefault("eps", []).append(e.clone())
        return e
    torch.randn_like = capture_randn_like
    model.encoder.register_forward_hook(lambda mod, inp, out: seen.__setitem__("logw", out[2].detach().clone()))

    tokens, x_lens = g["tokens"], g["x_lens"]
    out = {"logw_bias_offset": np.float32(LOGW_BIAS_OFFSET)}
    try:
        for i in range(tokens.shape[0]):
            ids = [int(v) for v in tokens[i, :x_lens[i]]]
            model.parser = lambda text, ids=ids: ids
            seen.clear()
            torch.manual_seed(140 + i)
            yh = model.infer_step(f"utterance {i}.")
            e = torch.exp(seen["logw"]).flatten()
            dist = float((e - e.round()).abs().min())
            print(f"  utterance {i}: {len(ids)} tokens, durations {seen['w'].flatten().int().tolist()}, z_len {seen['z_len']}, "
                  f"yh {tuple(yh.shape)}; closest exp(logw) to an integer: {dist:.2e}")
            assert dist >= MARGIN, "a ceil could flip: raise LOGW_BIAS_OFFSET"
            assert len(seen["eps"]) == 1 and yh.shape == (1, 8, seen["z_len"])
            out.update({f"tokens_{i}": np.asarray(ids, dtype=np.int64), f"w_{i}": seen["w"].flatten(), f"z_len_{i}": seen["z_len"],
                        f"eps_{i}": seen["eps"][0][0], f"yh_{i}": yh[0]})
    finally:
        torch.randn_like = randn_like
        ref_sub.sequence_mask, ref_sub.generate_path = seq_mask, gen_path
    mg.save("glow_tts_infer", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
