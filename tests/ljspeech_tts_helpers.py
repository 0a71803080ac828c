"""Shared by tests/test_ljspeech_tts_cpu.py and tests/test_ljspeech_tts_gpu.py: a small LJSpeech-format tree (metadata.csv with
`id|raw|normalised` lines and 16-bit mono 22,050 Hz wavs, written with the stdlib `wave` module) and the dataset section of a
configuration on it."""
import os
import wave

import numpy as np

TEXTS = ["Hello world.", "no period here", "Is it so?", "Dr. Smith paid $3.50 in 1905!", "  spaces around  ", "A well-known co. name.",
         "btw it works", "Wait... what?!", "{HH AH0 L OW1} again.", "Short."]


def write_tree(root, n, seed, lengths=None, texts=None):
    """n clips LJ000-0000 ... under `root`: seeded tone + noise, `lengths` samples each (default: seeded in [4096, 8192], not
    multiples of 512).  Returns (texts, lengths) in file order; the first ten are the validation split."""
    rng = np.random.default_rng(seed)
    lengths = list(lengths) if lengths is not None else [int(v) for v in rng.integers(4096, 8193, n)]
    texts = list(texts) if texts is not None else [TEXTS[i % len(TEXTS)] for i in range(n)]
    assert len(lengths) == len(texts) == n
    os.makedirs(os.path.join(str(root), "wavs"), exist_ok=True)
    with open(os.path.join(str(root), "metadata.csv"), "w", encoding="utf-8") as meta:
        for i in range(n):
            name = f"LJ000-{i:04d}"
            t = np.arange(lengths[i]) / 22050.0
            clip = 0.4 * np.sin(2 * np.pi * (150.0 + 40.0 * i) * t) + 0.2 * rng.uniform(-1, 1, lengths[i])
            with wave.open(os.path.join(str(root), "wavs", name + ".wav"), "wb") as f:
                f.setnchannels(1)
                f.setsampwidth(2)
                f.setframerate(22050)
                f.writeframes(np.round(clip * 32767).astype("<i2").tobytes())
            meta.write(f"{name}|{texts[i]}|{texts[i]}\n")
    return texts, lengths


def dataset_config(root, **overrides):
    """{"dataset": ...} as a utils.config tree: configs/datasets/ljspeech_tts.yaml's keys on `root`, character front end."""
    from utils import config as C
    ds = dict(_import_="datasets.ljspeech_tts.LJSpeechTTS", dataset_path=str(root), text_frontend="chars", cmudict_path="",
              device_spect=True, segment_length=-1, sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=80,
              intersperse_blanks=True, use_audio=True, use_spect=True, use_token=True)
    ds.update(overrides)
    return C.create({"dataset": ds})
