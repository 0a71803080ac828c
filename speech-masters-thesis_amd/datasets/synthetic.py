"""LJSpeech-shaped synthetic clips behind the reference's dataset contract
(``Dataset(config, split)``, 7-slot items, static ``collate``; datasets/ljspeech.py:17-140).

There is no LJSpeech audio offline, so benchmarks and tests draw clips from the seeded
generator of SURVEY.md 8(d): 0.5*(0.6*sum_{h<=8} sin(2 pi h f0 t + phi_h)/h + 0.4*U(-1,1)),
f0 ~ U[90, 250] Hz, clamped to [-1, 1], 22.05 kHz.
"""
import math

import torch
from torch.utils.data import Dataset

from datasets.ljspeech import LJSpeech, TRUNC_MOD


def synth_clip(length, seed, sample_rate=22050):
    g = torch.Generator().manual_seed(seed)
    f0 = 90.0 + 160.0 * torch.rand(1, generator=g, dtype=torch.float64)
    phi = 2 * math.pi * torch.rand(8, generator=g, dtype=torch.float64)
    t = torch.arange(length, dtype=torch.float64) / sample_rate
    tone = sum(torch.sin(2 * math.pi * h * f0 * t + phi[h - 1]) / h for h in range(1, 9))
    noise = torch.rand(length, generator=g, dtype=torch.float64) * 2 - 1
    return (0.5 * (0.6 * tone + 0.4 * noise)).clamp(-1, 1).to(torch.float32)


class SyntheticLJSpeech(Dataset):
    def __init__(self, config, split):
        super().__init__()
        ds = config.dataset
        self.n = int(ds.get("num_clips", 256)) if split == "train" else 10
        self.offset = 0 if split == "val" else 10
        self.fixed_length = int(ds.get("clip_length", 145408))
        self.ragged = bool(ds.get("ragged", False))
        self.sample_rate = int(ds.get("sample_rate", 22050))
        self.use_audio = ds.get("use_audio", True)
        self.segment_length = int(ds.get("segment_length", -1))

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        seed = self.offset + index
        length = self.fixed_length
        if self.ragged:
            g = torch.Generator().manual_seed(10_000 + seed)
            length = int(torch.randint(24064, 222720 + 1, (1,), generator=g))
        audio = synth_clip(length, seed, self.sample_rate)
        if 0 < self.segment_length < audio.shape[-1]:
            audio = audio[:self.segment_length]
        audio = audio[:len(audio) - len(audio) % TRUNC_MOD]
        if not self.use_audio:
            return None, None, None, None, None, None, None
        return None, None, None, None, audio, audio.shape[-1], None

    collate = staticmethod(LJSpeech.collate)


class SyntheticTTS(Dataset):
    """Token ids + log-mel-like frames with LJSpeech-like proportions behind the reference's dataset contract, for the
    token-to-spectrogram models (GlowTTS): item = (token [Tx] int64, Tx, spect [n_mels, Ty] fp32, Ty, None, None, None)."""

    def __init__(self, config, split):
        super().__init__()
        ds = config.dataset
        self.n = int(ds.get("num_clips", 256)) if split == "train" else 10
        self.offset = 0 if split == "val" else 10
        self.max_tokens = int(ds.get("max_tokens", 160))
        self.fpt = int(ds.get("frames_per_token", 5))
        self.n_vocab = int(ds.get("n_vocab", 148)) + int(bool(ds.get("intersperse_blanks", False)))
        self.n_mels = int(ds.get("n_mels", 80))

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(50_000 + self.offset + index)
        tx = int(torch.randint(max(2, self.max_tokens // 2), self.max_tokens + 1, (1,), generator=g))
        ty = tx * self.fpt + int(torch.randint(0, 2 * self.fpt, (1,), generator=g))
        token = torch.randint(1, self.n_vocab, (tx,), generator=g)
        # frames that depend on the token under them (so that an alignment exists to be found) + noise, log-mel range
        owner = torch.div(torch.arange(ty) * tx, ty, rounding_mode="floor").clamp(max=tx - 1)
        basis = torch.randn(self.n_vocab, self.n_mels, generator=torch.Generator().manual_seed(7))
        spect = (basis[token[owner]] * 1.5 - 4.0 + 0.5 * torch.randn(ty, self.n_mels, generator=g)).t().contiguous()
        return token, tx, spect, ty, None, None, None

    collate = staticmethod(LJSpeech.collate)


class SyntheticTTSAudio(Dataset):
    """Token ids + a waveform that depends on them, for the token-to-waveform models (VQTTS): item = (token [Tx] int64, Tx,
    None, None, audio [T] fp32, T, None), T a multiple of TRUNC_MOD.  Every token id owns an f0 in [90, 250] Hz; the clip is
    cut into Tx segments of drawn lengths (each at least ``min_segment`` samples, so that every token keeps more than one
    frame of a x256 encoder) and a segment is ``synth_clip``'s signal at its token's f0: eight harmonics with the clip's
    phases, continuous in time, plus the clip's noise.  So an alignment exists to be found, and it is not uniform."""

    def __init__(self, config, split):
        super().__init__()
        ds = config.dataset
        self.n = int(ds.get("num_clips", 256)) if split == "train" else 10
        self.offset = 0 if split == "val" else 10
        self.fixed_length = int(ds.get("clip_length", 145408))
        self.ragged = bool(ds.get("ragged", False))
        self.sample_rate = int(ds.get("sample_rate", 22050))
        self.max_tokens = int(ds.get("max_tokens", 160))
        self.min_segment = int(ds.get("min_segment", 512))
        self.n_vocab = int(ds.get("n_vocab", 148)) + int(bool(ds.get("intersperse_blanks", False)))

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        seed = self.offset + index
        g = torch.Generator().manual_seed(70_000 + seed)
        length = self.fixed_length
        if self.ragged:
            length = int(torch.randint(24064, 222720 + 1, (1,), generator=g))
        length -= length % TRUNC_MOD
        tx_max = max(1, min(self.max_tokens, length // self.min_segment))
        tx = int(torch.randint(max(1, tx_max // 2), tx_max + 1, (1,), generator=g))
        token = torch.randint(1, self.n_vocab, (tx,), generator=g)
        # segment lengths: min_segment each, the rest of the clip shared out in proportion to drawn weights
        w = 0.25 + torch.rand(tx, generator=g, dtype=torch.float64)
        ends = torch.round(torch.cumsum(w, 0) / w.sum() * (length - tx * self.min_segment)).long()
        ends = ends + self.min_segment * torch.arange(1, tx + 1)
        ends[-1] = length
        owner = torch.searchsorted(ends, torch.arange(length), right=True).clamp(max=tx - 1)
        f0 = 90.0 + 160.0 * token.double() / max(self.n_vocab - 1, 1)
        phi = 2 * math.pi * torch.rand(8, generator=g, dtype=torch.float64)
        phase = 2 * math.pi * torch.cumsum(f0[owner], 0) / self.sample_rate          # continuous across segment borders
        tone = sum(torch.sin(h * phase + phi[h - 1]) / h for h in range(1, 9))
        noise = torch.rand(length, generator=g, dtype=torch.float64) * 2 - 1
        audio = (0.5 * (0.6 * tone + 0.4 * noise)).clamp(-1, 1).to(torch.float32)
        return token, tx, None, None, audio, length, None

    collate = staticmethod(LJSpeech.collate)


class SyntheticTTSSpeakers(SyntheticTTS):
    """``SyntheticTTS`` for ``n_speakers`` voices: the same seeded items plus a seeded speaker id in slot 7, and frames that
    depend on the speaker as well -- every speaker shifts the token basis by its own offset vector, so that a speaker
    embedding has something to learn.  item = (token, Tx, spect [n_mels, Ty], Ty, None, None, speaker id); ``collate`` stacks
    the ids to int64 [B]."""

    def __init__(self, config, split):
        super().__init__(config, split)
        self.n_speakers = int(config.dataset.get("n_speakers", 8))
        assert self.n_speakers >= 1

    def __getitem__(self, index):
        token, tx, spect, ty, _, _, _ = super().__getitem__(index)
        g = torch.Generator().manual_seed(90_000 + self.offset + index)
        speaker = int(torch.randint(0, self.n_speakers, (1,), generator=g))
        offsets = torch.randn(self.n_speakers, self.n_mels, generator=torch.Generator().manual_seed(11))
        return token, tx, spect + 1.5 * offsets[speaker][:, None], ty, None, None, speaker

    @staticmethod
    def collate(batch):
        out = list(LJSpeech.collate(batch))
        out[6] = torch.tensor([item[6] for item in batch], dtype=torch.long)
        return tuple(out)
