"""``datasets.synthetic.SyntheticTTSSpeakers`` (configs/datasets/synthetic_tts_speakers.yaml): the multi-speaker form of the
synthetic token / mel corpus -- seeded items, speaker ids in range in slot 7, frames that depend on the speaker, and a collate
that stacks the ids to int64 [B].  Host code only; no GPU."""
import os

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "speech-masters-thesis_amd")


def _cfg(**kw):
    from utils import config as C
    cfg = C.load(os.path.join(PKG, "configs/datasets/synthetic_tts_speakers.yaml"))
    cfg.dataset.update(C.create(dict(num_clips=12, max_tokens=16, **kw)))
    return cfg


def test_items_are_seeded_and_the_ids_are_in_range():
    from datasets.synthetic import SyntheticTTS, SyntheticTTSSpeakers
    cfg = _cfg(n_speakers=5)
    ds, again, plain = SyntheticTTSSpeakers(cfg, "train"), SyntheticTTSSpeakers(cfg, "train"), SyntheticTTS(cfg, "train")
    assert len(ds) == 12 and len(SyntheticTTSSpeakers(cfg, "val")) == 10
    seen = []
    for i in range(len(ds)):
        token, tx, spect, ty, audio, audio_len, speaker = ds[i]
        t2, _, s2, _, _, _, sp2 = again[i]
        assert torch.equal(token, t2) and torch.equal(spect, s2) and speaker == sp2                     # seeded
        assert isinstance(speaker, int) and 0 <= speaker < 5 and audio is None and audio_len is None
        pt, ptx, ps, pty, *_ = plain[i]                          # the same item of SyntheticTTS: same tokens, same lengths
        assert torch.equal(token, pt) and (tx, ty) == (ptx, pty) and spect.shape == ps.shape == (80, ty)
        shift = spect - ps                                       # the speaker's offset of the basis: constant over the frames
        assert torch.allclose(shift, shift[:, :1].expand_as(shift), atol=1e-5) and float(shift.abs().max()) > 0.1
        seen.append((speaker, shift[:, 0]))
    assert len({s for s, _ in seen}) > 1, "12 items drew a single speaker"
    for (s1, o1) in seen:
        for (s2, o2) in seen:
            assert torch.allclose(o1, o2, atol=1e-5) == (s1 == s2)      # one offset per speaker, different between speakers
    assert SyntheticTTSSpeakers(cfg, "val")[0][6] in range(5)


def test_train_and_val_items_differ():
    from datasets.synthetic import SyntheticTTSSpeakers
    cfg = _cfg()
    a, b = SyntheticTTSSpeakers(cfg, "train")[0], SyntheticTTSSpeakers(cfg, "val")[0]
    assert a[0].shape != b[0].shape or not torch.equal(a[0], b[0])


def test_collate_stacks_the_speaker_ids():
    from datasets.synthetic import SyntheticTTSSpeakers
    ds = SyntheticTTSSpeakers(_cfg(), "train")
    items = [ds[i] for i in range(4)]
    token, token_len, spect, spect_len, audio, audio_len, speaker = SyntheticTTSSpeakers.collate(items)
    assert speaker.dtype == torch.int64 and speaker.shape == (4,) and speaker.tolist() == [it[6] for it in items]
    assert int(speaker.min()) >= 0 and int(speaker.max()) < 8                       # n_speakers of the shipped configuration
    assert token.shape == (4, int(token_len.max())) and spect.shape == (4, 80, int(spect_len.max())) and audio is None and audio_len is None
    for i, it in enumerate(items):                                                  # the other slots are LJSpeech.collate's
        assert torch.equal(token[i, :it[1]], it[0]) and torch.equal(spect[i, :, :it[3]], it[2])


def test_dataloader_registry_builds_batches_with_speaker_ids():
    """`get_dataloaders` (what train.py calls) resolves the class from the configuration and collates with its own collate."""
    from utils import config as C
    from utils.commons import get_dataloaders
    cfg = C.merge(_cfg(), C.create({"train": {"batch_size": 4, "num_workers": 0}}))
    train_loader, val_loader = get_dataloaders(cfg, shuffle_train=False)
    batch = next(iter(train_loader))
    assert len(batch) == 7 and batch[6].dtype == torch.int64 and batch[6].shape == (4,) and batch[0].shape[0] == 4
    assert sum(b[6].numel() for b in val_loader) == 10
