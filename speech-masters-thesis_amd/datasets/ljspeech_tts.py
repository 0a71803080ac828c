"""LJSpeech-1.1 for the token models (GlowTTS, VQTTS): transcripts through the text front end, waveforms, and the log-mels made
ON THE DEVICE from the collated waveforms (reference datasets/ljspeech.py:70-112 makes them in the DataLoader workers).

``dataset.text_frontend`` chooses the front end (models/parser.py): ``chars`` needs no file, ``cmudict`` needs the CMU
pronouncing dictionary at ``dataset.cmudict_path``.  Items are the 7-tuples of ``datasets.ljspeech.LJSpeech``:
``(token, token_len, None, None, audio, audio_len, None)``.  The spectrogram slots stay empty: with ``dataset.device_spect``
train.py fills them from ``datasets.transforms.BatchLogMel`` after the batch reached the device, which is why the audio is
returned for a spectrogram model too, although ``get_model`` switched ``use_audio`` off for it.
"""
import os
import random

import torch

from datasets.ljspeech import TRUNC_MOD, LJSpeech, read_wav
from models.parser import parser_from_config, sentence_ids


class LJSpeechTTS(LJSpeech):
    def __init__(self, config, split: str):
        super().__init__(config, split)
        ds = config.dataset
        self.parser = parser_from_config(ds)
        if self.parser is None:
            raise ValueError("LJSpeechTTS needs dataset.text_frontend (chars or cmudict)")
        self.intersperse_blanks = bool(ds.get("intersperse_blanks", False))
        self.device_spect = bool(ds.get("device_spect", False))
        if self.use_spect and not self.device_spect:
            raise NotImplementedError("use_spect: log-mel is computed on the device (dataset.device_spect: true, datasets."
                                      "transforms.BatchLogMel), not inside DataLoader workers")
        self.n_fft, self.hop_length = ds.n_fft, ds.hop_length
        with open(os.path.join(self.root, "metadata.csv"), encoding="utf-8") as f:
            texts = [line.strip().split("|")[2] for line in f if line.strip()]
        self.token = texts[10:] if split == "train" else texts[:10]          # the parent's split of the same lines
        assert len(self.token) == len(self.audio)

    def __getitem__(self, index):
        path = self.audio[index]
        audio = read_wav(path)
        if 0 < self.segment_length < audio.shape[-1]:
            start = random.randint(0, audio.shape[-1] - self.segment_length)
            audio = audio[start:start + self.segment_length]
        audio = audio[:len(audio) - len(audio) % TRUNC_MOD]
        audio_len = audio.shape[-1]
        pad = (self.n_fft - self.hop_length) // 2
        if audio_len <= pad or audio_len + 2 * pad < self.n_fft:
            raise ValueError(f"{path}: {audio_len} samples after the cut to a multiple of {TRUNC_MOD} are too short for one "
                             f"frame (n_fft={self.n_fft}, hop_length={self.hop_length})")
        token = token_len = None
        if self.use_token:
            try:
                token = torch.tensor(sentence_ids(self.parser, self.token[index], self.intersperse_blanks), dtype=torch.long)
            except ValueError as e:
                raise ValueError(f"{path}: {e}") from None
            token_len = token.shape[-1]
        if not (self.use_audio or (self.use_spect and self.device_spect)):
            audio = audio_len = None
        return token, token_len, None, None, audio, audio_len, None
