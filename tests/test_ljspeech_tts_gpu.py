"""GlowTTS and VQTTS trained from text on an LJSpeech-format tree: datasets.ljspeech_tts.LJSpeechTTS (character front end),
train.prepare_batch making the log-mels on the device (datasets.transforms.BatchLogMel, smt_melspec_ragged), one train step,
a validation epoch, and synthesis from a sentence.

Twelve seeded clips of 4,096-8,192 samples; every transcript is short enough that its tokens, blanks included, do not exceed
its decoder frames (mel frames / n_sqz = samples / 512).  GlowTTS at the widths of the golden fixture (hidden 64, 8 mels),
VQTTS at the widths of tests/vqtts_model_helpers.py, both with a 64-symbol vocabulary."""
import math

import numpy as np
import pytest
import torch

import vqtts_model_helpers as VH
from ljspeech_tts_helpers import dataset_config, write_tree

pytestmark = pytest.mark.gpu
DEV = "cuda"
# text (with its closing mark) by length: a clip of L samples has L // 512 decoder frames and takes 2 n + 1 tokens
TEXT_BY_LENGTH = {3: "hi", 4: "yes", 5: "stop", 6: "hello", 7: "we go?"}


def _texts_for(lengths):
    out = []
    for n in lengths:
        budget = ((n - n % 512) // 512 - 1) // 2
        assert budget >= 3
        out.append(TEXT_BY_LENGTH[min(budget, 7)])
    return out


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("ljspeech")
    lengths = [int(v) for v in np.random.default_rng(7).integers(4096, 8193, 12)]
    texts, lengths = write_tree(root, n=12, seed=7, lengths=lengths, texts=_texts_for(lengths))
    return root, texts, lengths


def _train_section(tmp_path):
    return dict(batch_size=4, num_workers=0, ema=False, grad_clip_norm=None, n_gpus=1, log_dir=str(tmp_path), seed=0)


OPTIMIZER = dict(name="adam", lr=1e-3, betas=[0.9, 0.98], weight_decay=0, eps=1e-9)


def _glow_config(root, tmp_path):
    from oracle import glow_oracle as go
    from utils import config as C
    model = dict(_import_="models.glow_tts.glow_tts.GlowTTS", n_speakers=1, gin_channels=0,
                 encoder=dict(go.GOLDEN_CFG["encoder"], n_vocab=64), decoder=dict(go.GOLDEN_CFG["decoder"]))
    return C.merge(dataset_config(root, n_mels=8), C.create({"model": model, "optimizer": OPTIMIZER, "train": _train_section(tmp_path)}))


def _all_items(cfg):
    from datasets.ljspeech_tts import LJSpeechTTS
    val, train = LJSpeechTTS(cfg, "val"), LJSpeechTTS(cfg, "train")
    assert len(val) == 10 and len(train) == 2
    return [val[i] for i in range(10)] + [train[i] for i in range(2)]


def test_glow_tts_from_text(tree, tmp_path):
    import train as trainlib
    from datasets.ljspeech_tts import LJSpeechTTS
    from datasets.transforms import MelSpectrogram
    from utils.commons import get_dataloaders, get_model, get_optimizer
    from utils.train_utils import ScalarWriter
    root, texts, lengths = tree
    cfg = _glow_config(root, tmp_path)
    torch.manual_seed(0)
    model, ema = get_model(cfg, DEV)
    assert cfg.dataset.use_audio is False and cfg.dataset.use_spect is True           # the flag surgery for a spectrogram model
    optimizer, scheduler = get_optimizer(cfg, model)

    # ---- the prepared batch: per-clip log-mels, log(1e-7) behind them, no audio left
    collated = LJSpeechTTS.collate(_all_items(cfg))
    audio, audio_len = collated[4], collated[5]
    assert audio_len.tolist() == [n - n % 512 for n in lengths] and len(set(audio_len.tolist())) > 1
    batch = trainlib.prepare_batch(collated, cfg, torch.device(DEV), trainlib.batch_mel_for(cfg, torch.device(DEV)))
    token, token_len, spect, spect_len = batch[:4]
    assert batch[4] is None and batch[5] is None and token.is_cuda and spect_len.is_cuda and spect_len.dtype == torch.int64
    assert spect_len.tolist() == [n // 256 for n in audio_len.tolist()] and spect.shape == (12, 8, int(spect_len.max()))
    assert all(int(t) <= int(f) // 2 for t, f in zip(token_len, spect_len))          # tokens fit the decoder frames
    mel = MelSpectrogram(sample_rate=22050, n_fft=1024, win_length=1024, hop_length=256, n_mels=8, f_min=0.0, f_max=8000.0).to(DEV)
    fill = torch.tensor(math.log(1e-7), dtype=torch.float32)
    for b, n in enumerate(audio_len.tolist()):
        alone = mel(audio[b, :, :n].to(DEV))
        assert torch.equal(spect[b, :, :n // 256], alone[0]), b
        assert (spect[b, :, n // 256:].cpu() == fill).all(), b

    # ---- one train step on four of the clips
    before = [p.detach().clone() for p in model.parameters()]
    model.train()
    small = LJSpeechTTS.collate(_all_items(cfg)[:4])
    loss_dict, _ = trainlib.train_step(global_step=0, batch=small, config=cfg, model=model, ema=ema, optimizer=optimizer,
                                       scheduler=scheduler, device=torch.device(DEV))
    assert all(torch.isfinite(loss_dict[k]) for k in ("loss", "loss_mle", "loss_length"))
    changed = sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, model.parameters()))
    print(f"glow_tts: loss {float(loss_dict['loss'].detach()):.4f}; {changed} of {len(before)} parameter tensors changed")
    assert changed > len(before) // 2
    assert all(torch.isfinite(p).all() for p in model.parameters())

    # ---- a validation epoch through the DataLoader (three batches of the ten validation clips)
    _, val_loader = get_dataloaders(cfg)
    stats = trainlib.val_epoch(epoch=0, config=cfg, model=model, ema=ema, val_dataloader=val_loader,
                               writer=ScalarWriter(str(tmp_path)), device=torch.device(DEV))
    assert math.isfinite(stats["loss"]) and math.isfinite(stats["loss_mle"])

    # ---- synthesis from a sentence: the ids of the dataset, blanks included
    model.eval()
    yh = model.infer_step("hello world.")
    assert yh.shape[:2] == (1, 8) and yh.shape[2] >= 2 and torch.isfinite(yh).all()
    ids = model.text_parser("hello world.")
    blanks = [64] * (2 * len(ids) + 1)
    blanks[1::2] = ids
    torch.manual_seed(3)
    want = model.infer_step(blanks)
    torch.manual_seed(3)
    assert torch.equal(model.infer_step("  hello world "), want)


def test_vqtts_step_from_text(tree, tmp_path):
    import train as trainlib
    from datasets.ljspeech_tts import LJSpeechTTS
    from utils import config as C
    from utils.commons import get_model, get_optimizer
    root, texts, lengths = tree
    raw = VH.config_dict()
    raw["model"]["encoder"]["n_vocab"] = 64
    cfg = C.merge(C.create(raw), dataset_config(root), C.create({"optimizer": OPTIMIZER, "train": _train_section(tmp_path)}))
    torch.manual_seed(0)
    model, ema = get_model(cfg, DEV)
    assert cfg.dataset.use_audio is True and cfg.dataset.use_spect is False           # a waveform model: no spectrogram made
    VH.randomize_zero_init(model)
    optimizer, scheduler = get_optimizer(cfg, model)
    batch = LJSpeechTTS.collate(_all_items(cfg)[:4])
    prepared = trainlib.prepare_batch(batch, cfg, torch.device(DEV), trainlib.batch_mel_for(cfg, torch.device(DEV)))
    assert prepared[2] is None and prepared[3] is None and prepared[4].is_cuda and prepared[4].shape[1] == 1
    before = [p.detach().clone() for p in model.parameters()]
    model.train()
    loss_dict, _ = trainlib.train_step(global_step=0, batch=batch, config=cfg, model=model, ema=ema, optimizer=optimizer,
                                       scheduler=scheduler, device=torch.device(DEV))
    assert all(torch.isfinite(loss_dict[k]) for k in ("loss", "loss_recon", "loss_stft", "loss_ce", "loss_align", "loss_dur"))
    changed = sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, model.parameters()))
    print(f"vqtts: loss {float(loss_dict['loss'].detach()):.4f}; {changed} of {len(before)} parameter tensors changed")
    assert changed > len(before) // 2
    model.eval()
    wave = model.infer_step("hi")
    assert wave.dim() == 2 and wave.shape[0] == 1 and wave.shape[1] % VH.STRIDE == 0 and torch.isfinite(wave).all()
