"""datasets.ljspeech_tts.LJSpeechTTS on an LJSpeech-format tree written with the stdlib `wave` module, and the host side of the
ragged log-mel (smt_amd.spectral.log_mel_ragged, the smt_melspec_ragged entry): refusals and export.  No GPU."""
import ctypes
import os

import pytest
import torch

from ljspeech_tts_helpers import dataset_config, write_tree

DUMMY = ctypes.c_void_p(0x1000)      # a non-null pointer for calls that must fail before they launch anything


def test_split_tokens_lengths_and_audio(tmp_path):
    from datasets.ljspeech_tts import LJSpeechTTS
    from models.parser import CMUDictParser
    texts, lengths = write_tree(tmp_path, n=13, seed=0)
    cfg = dataset_config(tmp_path)
    train, val = LJSpeechTTS(cfg, "train"), LJSpeechTTS(cfg, "val")
    assert len(val) == 10 and len(train) == 3
    with pytest.raises(ValueError, match="split"):
        LJSpeechTTS(cfg, "test")
    parser = CMUDictParser(None)
    for ds, offset in ((val, 0), (train, 10)):
        for i in range(len(ds)):
            token, token_len, spect, spect_len, audio, audio_len, speaker = ds[i]
            text = texts[offset + i].strip()
            want = parser(text if text[-1] in ".!?" else text + ".")
            assert token.dtype == torch.long and token_len == len(token) == 2 * len(want) + 1
            assert token[1::2].tolist() == want and set(token[0::2].tolist()) == {64}      # the blank id: len(symbols)
            assert spect is None and spect_len is None and speaker is None
            n = lengths[offset + i]
            assert audio_len == audio.shape[-1] == n - n % 512 and audio.dtype == torch.float32
    # the appended period: item 1's transcript has none, item 2's ends in "?"
    assert not texts[1].strip().endswith(".") and val[1][0][-2] == parser(".")[0]
    assert texts[2].strip().endswith("?") and val[2][0][-2] == parser("?")[0]
    batch = LJSpeechTTS.collate([val[i] for i in range(4)])
    assert batch[0].shape == (4, int(batch[1].max())) and batch[2] is None and batch[4].shape == (4, 1, int(batch[5].max()))
    assert batch[5].dtype == torch.long and not batch[5].is_cuda


def test_without_blanks_and_with_the_dictionary(tmp_path):
    from datasets.ljspeech_tts import LJSpeechTTS
    from models.parser import CMUDictParser
    texts, _ = write_tree(tmp_path, n=11, seed=1)
    tiny = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_cmudict.txt")
    ds = LJSpeechTTS(dataset_config(tmp_path, intersperse_blanks=False, text_frontend="cmudict", cmudict_path=tiny), "val")
    assert len(ds.parser.symbols) == 148
    assert ds[0][0].tolist() == CMUDictParser(tiny)(texts[0].strip())
    with pytest.raises(ValueError, match="no_such_dict.txt"):
        LJSpeechTTS(dataset_config(tmp_path, text_frontend="cmudict", cmudict_path=str(tmp_path / "no_such_dict.txt")), "val")
    with pytest.raises(ValueError, match="text_frontend"):
        LJSpeechTTS(dataset_config(tmp_path, text_frontend=None), "val")


def test_flag_surgery_keeps_the_audio_for_the_device_spectrogram(tmp_path):
    from datasets.ljspeech_tts import LJSpeechTTS
    write_tree(tmp_path, n=11, seed=2)
    # what get_model leaves for a token-to-spectrogram model: use_audio off, use_spect on
    item = LJSpeechTTS(dataset_config(tmp_path, use_audio=False), "val")[0]
    assert item[0] is not None and item[2] is None and item[4] is not None and item[5] == item[4].shape[-1]
    # ... and for a token-to-waveform model: use_spect off
    item = LJSpeechTTS(dataset_config(tmp_path, use_spect=False), "val")[0]
    assert item[4] is not None
    # neither: no audio
    item = LJSpeechTTS(dataset_config(tmp_path, use_audio=False, use_spect=False), "val")[0]
    assert item[4] is None and item[5] is None
    # a spectrogram inside the workers is refused, as by the parent class
    with pytest.raises(NotImplementedError, match="use_spect"):
        LJSpeechTTS(dataset_config(tmp_path, device_spect=False), "val")
    item = LJSpeechTTS(dataset_config(tmp_path, device_spect=False, use_spect=False, use_token=False), "val")[0]
    assert item[0] is None and item[1] is None and item[4] is not None


def test_segment_length_and_too_short_clip(tmp_path):
    from datasets.ljspeech_tts import LJSpeechTTS
    write_tree(tmp_path, n=11, seed=3, lengths=[8000, 600, 300] + [4096] * 8)
    ds = LJSpeechTTS(dataset_config(tmp_path, segment_length=1024), "val")
    assert ds[0][5] == 1024 and ds[3][5] == 1024
    with pytest.raises(AssertionError, match="multiple of 512"):
        LJSpeechTTS(dataset_config(tmp_path, segment_length=1000), "val")
    ds = LJSpeechTTS(dataset_config(tmp_path), "val")
    assert ds[0][5] == 7680 and ds[1][5] == 512          # 512 samples: two frames at (1024, 256)
    with pytest.raises(ValueError, match="LJ000-0002.wav"):   # 300 samples are cut to 0
        ds[2]
    ds = LJSpeechTTS(dataset_config(tmp_path, n_fft=2048, hop_length=240, win_length=1200), "val")
    with pytest.raises(ValueError, match="LJ000-0001.wav.*too short for one frame"):     # 512 <= pad = 904
        ds[1]


def test_prepare_batch_without_the_key_is_to_device_alone():
    import train
    from utils import config as C
    cfg = C.create({"dataset": dict(use_audio=True, use_spect=False, use_token=True)})
    batch = (torch.arange(6).reshape(2, 3), torch.tensor([3, 2]), None, None, torch.zeros(2, 1, 512), torch.tensor([512, 256]), None)
    out = train.prepare_batch(batch, cfg, torch.device("cpu"), train.batch_mel_for(cfg, torch.device("cpu")))
    assert train.batch_mel_for(cfg, torch.device("cpu")) is None
    assert isinstance(out, list) and len(out) == 7 and out[2] is None and out[6] is None
    assert all(a is b or torch.equal(a, b) for a, b in zip(out, batch))


# ------------------------------------------------------------------------------------------- ragged log-mel, host side

def _mel_args():
    return torch.zeros(80, 513), torch.zeros(80, 2, dtype=torch.int32)


def test_log_mel_ragged_refuses_on_the_host():
    from smt_amd import spectral
    basis, band = _mel_args()
    x = torch.zeros(2, 4096)
    bad = [
        (dict(lens=torch.tensor([4096, 4097])), "item 1 has length 4097, outside \\[0, T=4096\\]"),
        (dict(lens=torch.tensor([-1, 4096])), "item 0 has length -1"),
        (dict(lens=torch.tensor([4096])), "2 lengths"),
        (dict(lens=torch.tensor([4096.0, 1.0])), "integer tensor on the CPU"),
        (dict(lens=[4096, 4096]), "integer tensor on the CPU"),
        (dict(x=torch.zeros(4096)), "\\[B, T\\]"),
        (dict(n_fft=1000), "n_fft=1000 unsupported"),
        (dict(hop=0), "hop=0 outside"),
        (dict(hop=2048), "hop=2048 outside"),
    ]
    for change, message in bad:
        kw = dict(x=x, lens=torch.tensor([4096, 2048]), n_fft=1024, hop=256)
        kw.update(change)
        with pytest.raises(ValueError, match=message):
            spectral.log_mel_ragged(kw["x"], kw["lens"], basis, band, kw["n_fft"], kw["hop"], 1024, -16.0)
    assert [spectral.clip_frames(n, 1024, 256) for n in (0, 384, 385, 512, 1536, 4096)] == [0, 0, 1, 2, 6, 16]
    assert spectral.clip_frames(200, 512, 256) == 0 and spectral.clip_frames(300, 512, 256) == 1    # pad 128: 456 < 512 <= 556


def test_entry_is_exported_and_checks_its_arguments():
    from smt_amd import native as N
    lib = N.lib()
    assert "smt_melspec_ragged" in N.exported_symbols() and lib.smt_abi_version() == N.ABI_VERSION == 10

    def call(x=DUMMY, lens=DUMMY, mel=DUMMY, batch=2, t=4096, n_fft=1024, hop=256, n_mels=80, frames_out=16):
        return lib.smt_melspec_ragged(x, lens, DUMMY, DUMMY, DUMMY, DUMMY, mel, batch, t, n_fft, hop, n_mels, frames_out, -16.0, None)

    bad = [(dict(x=None), "null pointer"), (dict(lens=None), "null pointer"), (dict(mel=None), "null pointer"),
           (dict(n_fft=1000), "n_fft=1000 unsupported (256, 512, 1024, 2048)"), (dict(n_fft=4096), "n_fft=4096 unsupported"),
           (dict(hop=0), "hop=0 outside [1, n_fft=1024]"), (dict(hop=1025), "hop=1025 outside"),
           (dict(n_mels=0), "n_mels=0, need >= 1"), (dict(t=0), "t=0 outside [1, 2^30]"),
           (dict(frames_out=-1), "frames_out=-1, need >= 0"), (dict(batch=-1), "batch=-1 outside"),
           (dict(batch=65536), "batch=65536 outside [0, 65535]")]
    for change, message in bad:
        assert call(**change) == 1, change
        got = lib.smt_last_error().decode()
        assert got.startswith("smt_melspec_ragged: ") and message in got, (change, got)
    # nothing to do: returns before any launch (the pointers are not real)
    assert call(batch=0) == 0 and call(frames_out=0) == 0
    # ... but only after the argument checks
    assert call(batch=0, n_fft=1000) == 1 and call(frames_out=0, hop=0) == 1
