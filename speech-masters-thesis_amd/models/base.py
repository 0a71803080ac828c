"""Model API of the reference (models/base.py:6-55): four abstract families, each
mapping the 7-slot batch ``(token, token_len, spect, spect_len, audio, audio_len,
speaker)`` onto ``forward`` and returning ``(loss_dict, metrics_dict)``.

``isinstance`` against these classes drives the dataset flag surgery in
utils/commons.get_model and the validation artefact type in train.py, so the
class names and the slot mapping are part of the drop-in contract.
"""
import torch
import torch.nn as nn

_SLOTS = ("token", "token_len", "spect", "spect_len", "audio", "audio_len", "speaker")


class _SlotModel(nn.Module):
    inputs = ()        # batch slots passed positionally to forward
    target = None      # slot stored back as loss_dict["y"]
    squeeze_target = False

    def supervised_step(self, batch):
        named = dict(zip(_SLOTS, batch))
        loss_dict, metrics_dict = self(*[named[s] for s in self.inputs], speaker=named["speaker"])
        y = named[self.target]
        loss_dict["y"] = y.squeeze(1) if self.squeeze_target else y
        return loss_dict, metrics_dict

    def forward(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} does not implement forward")


class TokenToWaveformModel(_SlotModel):
    inputs, target, squeeze_target = ("token", "token_len", "audio", "audio_len"), "audio", True


class WaveformReconstructionModel(_SlotModel):
    inputs, target, squeeze_target = ("audio", "audio_len"), "audio", True


class TokenToSpectrogramModel(_SlotModel):
    inputs, target = ("token", "token_len", "spect", "spect_len"), "spect"


class SpectrogramReconstructionModel(_SlotModel):
    inputs, target = ("spect", "spect_len"), "spect"


def text_frontend(config, n_vocab):
    """(parser, intersperse_blanks) of a token model: the text front end ``dataset.text_frontend`` names (models/parser.py),
    or None when the key is unset -- the model then takes token ids only.  ValueError when the parser's table is larger than
    the model's embedding (``encoder.n_vocab``; the blank id sits right behind the table)."""
    from models.parser import parser_from_config
    ds = config.dataset
    parser = parser_from_config(ds)
    if parser is not None and len(parser.symbols) > n_vocab:
        raise ValueError(f"dataset.text_frontend = {ds.text_frontend} has {len(parser.symbols)} symbols, more than "
                         f"encoder.n_vocab = {n_vocab}")
    return parser, bool(ds.get("intersperse_blanks", False))


def sentence_to_ids(model, text):
    """The token ids of one sentence for ``model.infer_step``, as the dataset makes them for training."""
    if getattr(model, "text_parser", None) is None:
        raise NotImplementedError("infer_step takes token ids: this model was configured without a text front end "
                                  "(dataset.text_frontend: chars, or cmudict with the CMUDict file at dataset.cmudict_path)")
    from models.parser import sentence_ids
    return sentence_ids(model.text_parser, text, model.intersperse_blanks)


def token_batch(x, x_lengths, n_vocab):
    """The checks of a synthesis call's token ids, shared by ``GlowTTS.infer`` and ``VQTTS.infer``: x [B, Tx] integer ids with
    B >= 1, x_lengths [B] integers in [1, Tx] (None = full width), every id inside its length in [0, n_vocab) -- ValueError
    otherwise, on the host, as the ids come from outside the program.  Returns (ids int64 [B, Tx], lengths int64 [B], valid
    bool [B, Tx]), all on the CPU."""
    x = torch.as_tensor(x).detach()
    if x.dim() != 2 or x.shape[0] == 0:
        raise ValueError(f"x must be token ids [B, Tx] with B >= 1, got shape {tuple(x.shape)}")
    b, tx = x.shape
    if x_lengths is None:
        lens = torch.full((b,), tx, dtype=torch.int64)
    else:
        lens = torch.as_tensor(x_lengths).detach().cpu()
        if lens.shape != (b,) or lens.is_floating_point() or lens.is_complex():
            raise ValueError(f"x_lengths must be {b} integers, got {lens.dtype} of shape {tuple(lens.shape)}")
        lens = lens.long()
    for i, n in enumerate(lens.tolist()):
        if not 1 <= n <= tx:
            raise ValueError(f"item {i} has {n} tokens: every item needs 1 to {tx} (the width of x)")
    if x.is_floating_point() or x.is_complex() or x.dtype == torch.bool:
        raise ValueError(f"x must hold integer token ids, got {x.dtype}")
    xc = x.cpu().long()
    valid = torch.arange(tx)[None, :] < lens[:, None]
    bad = valid & ((xc < 0) | (xc >= n_vocab))
    if bad.any():
        i, t = (int(v) for v in bad.nonzero()[0])
        raise ValueError(f"item {i}, token {t}: id {int(xc[i, t])} is outside [0, {n_vocab})")
    return xc, lens, valid
