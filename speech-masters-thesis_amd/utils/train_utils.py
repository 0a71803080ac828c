"""Helpers of the train loop (reference utils/train_utils.py): barrier, seeding, running
averages, scalar logging, checkpoints, and the val-time spectrogram / audio dumps.  The reference makes
those with librosa + soundfile + matplotlib; here the mel front end, the mel inversion and Griffin-Lim
run on the device (datasets.transforms) and the files are written with the stdlib."""
import json
import logging
import os
import random

import numpy as np
import torch
import torch.distributed as dist

logger = logging.getLogger(__name__)


def barrier():
    if dist.is_initialized():
        dist.barrier()


def seed_all_rng(seed, cuda=True):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if cuda and torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


class ScalarWriter:
    """TensorBoard ``SummaryWriter`` when tensorboard is importable, JSON-lines otherwise
    (same ``add_scalar`` / ``close`` surface; train_utils.py:135-145)."""

    def __init__(self, log_dir):
        self._tb = None
        try:
            from torch.utils.tensorboard import SummaryWriter
            self._tb = SummaryWriter(log_dir)
        except Exception:  # tensorboard absent
            os.makedirs(log_dir, exist_ok=True)
            self._f = open(os.path.join(log_dir, "scalars.jsonl"), "a", encoding="utf-8")

    def add_scalar(self, tag, value, step):
        if self._tb is not None:
            self._tb.add_scalar(tag, value, step)
        else:
            self._f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
            self._f.flush()

    def close(self):
        (self._tb or self._f).close()


def accumulate_stats(over_n_steps, loss_dict, metrics_dict, accumulated_loss, accumulated_metrics):
    """Running means of every ``*loss*`` entry and every metric (train_utils.py:120-132).
    All scalars of a step are fetched with ONE device->host copy instead of one per key."""
    loss_keys = [k for k in loss_dict if "loss" in k]
    metric_keys = list(metrics_dict)
    if not loss_keys and not metric_keys:
        return
    stacked = torch.stack([loss_dict[k].detach().float().reshape(()) for k in loss_keys] +
                          [torch.as_tensor(metrics_dict[k]).detach().float().reshape(()).to(loss_dict[loss_keys[0]].device)
                           for k in metric_keys]).cpu().tolist()
    for k, v in zip(loss_keys, stacked[:len(loss_keys)]):
        accumulated_loss[k] += v / over_n_steps
    for k, v in zip(metric_keys, stacked[len(loss_keys):]):
        accumulated_metrics[k] += v / over_n_steps


def log_stats(step_or_epoch, writer, losses, metrics, prefix="train"):
    for key, value in losses.items():
        writer.add_scalar(f"loss/{prefix}_{key}", value, step_or_epoch)
    for key, value in metrics.items():
        writer.add_scalar(f"metrics/{prefix}_{key}", value, step_or_epoch)


def save_checkpoint(config, global_step, epoch, model, ema, optimizer, scheduler):
    """Same dictionary layout as the reference (train_utils.py:148-171); ``epoch=-1`` writes
    ``ckpt.last.pt``.  The config is stored as a plain dict so the file loads with
    ``torch.load(..., weights_only=True)``."""
    name = "last" if epoch == -1 else global_step
    path = os.path.join(config.train.log_dir, "ckpts", f"ckpt.{name}.pt")
    torch.save({
        "config": config.to_dict() if hasattr(config, "to_dict") else dict(config),
        "model": model.state_dict(),
        "optim": optimizer.state_dict(),
        "sched": scheduler.state_dict(),
        "ema": ema.state_dict(),
        "step": global_step,
        "epoch": config.train.total_epochs if epoch == -1 else epoch,
        # not in the reference's checkpoints (train_utils.py:148-171): the codebook's EMA accumulators and the dropout step
        # counter are plain attributes there and are lost on resume (bottleneck.py:20-24,179); loaders tolerate the key
        "extra": extra_train_state(model),
    }, path)
    return path


def _codebooks(model):
    """(state name, block) of every EMA codebook of a model: the VQ-VAE's per-level blocks, VQTTS's grouped one."""
    blocks = [(f"bottleneck.level_blocks.{i}", blk) for i, blk in enumerate(getattr(getattr(model, "bottleneck", None), "level_blocks", []))]
    if hasattr(model, "quant_bottleneck"):
        blocks.append(("quant_bottleneck", model.quant_bottleneck))
    return blocks


def extra_train_state(model):
    """Training state that lives outside ``state_dict()``: per codebook ``k_sum`` / ``k_elem`` / ``init``, and the
    dropout step counter."""
    out = {}
    for name, blk in _codebooks(model):
        if getattr(blk, "init", False) and blk.k_sum is not None:
            out[name] = {"k_sum": blk.k_sum.detach().clone(), "k_elem": blk.k_elem.detach().clone(), "threshold": float(blk.threshold)}
    if hasattr(model, "_drop_seed"):
        out["drop_seed"] = int(model._drop_seed)
    return out


def restore_extra_train_state(model, extra):
    """Counterpart of ``extra_train_state``.  Without the extra entry (a checkpoint written by the reference) a codebook
    that was trained (non-zero ``k``) is kept with ``restore_k()`` (bottleneck.py:48-58) instead of being re-drawn from
    the first batch, which is what the reference's resume path silently does (``init`` is False after loading)."""
    extra = extra or {}
    for name, blk in _codebooks(model):
        st = extra.get(name)
        if st is not None:
            blk.k_sum = st["k_sum"].to(blk.k.device, torch.float32).clone()
            blk.k_elem = st["k_elem"].to(blk.k.device, torch.float32).clone()
            blk.threshold = float(st.get("threshold", blk.threshold))
            blk.init = True
        elif bool(blk.k.abs().sum() > 0):
            blk.restore_k(threshold=blk.threshold)
    if "drop_seed" in extra and hasattr(model, "_drop_seed"):
        model._drop_seed = int(extra["drop_seed"])


def write_wav(path, samples, sample_rate):
    """16-bit mono PCM through the stdlib (the reference uses soundfile, train_utils.py:267-277)."""
    import wave
    pcm = (np.clip(np.asarray(samples, dtype=np.float64), -1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(path, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(int(sample_rate))
        f.writeframes(pcm.tobytes())


def write_png_gray(path, image):
    """8-bit greyscale PNG with zlib + struct only (the reference draws its grids with matplotlib + PIL)."""
    import struct
    import zlib
    img = np.ascontiguousarray(image, dtype=np.uint8)
    h, w = img.shape
    raw = b"".join(b"\x00" + img[r].tobytes() for r in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def spects_to_grid(ys, yhs, n=4):
    """Pairs of spectrograms [n_mels, frames] -> one uint8 image: row i = ground truth | prediction, low frequencies at
    the bottom, a common grey scale per pair (train_utils.py:174-195 without matplotlib)."""
    rows = []
    for i in range(min(n, len(ys))):
        a, b = np.asarray(ys[i], dtype=np.float32), np.asarray(yhs[i], dtype=np.float32)
        frames = max(a.shape[1], b.shape[1])
        lo, hi = min(a.min(), b.min()), max(a.max(), b.max())
        pair = np.zeros((a.shape[0], 2 * frames + 4), dtype=np.uint8)
        for off, m in ((0, a), (frames + 4, b)):
            pair[:, off:off + m.shape[1]] = np.clip(255.0 * (m[::-1] - lo) / max(hi - lo, 1e-12), 0, 255).astype(np.uint8)
        rows += [pair, np.zeros((4, pair.shape[1]), dtype=np.uint8)]
    width = max(r.shape[1] for r in rows)
    return np.concatenate([np.pad(r, ((0, 0), (0, width - r.shape[1]))) for r in rows], axis=0)


@torch.no_grad()
def save_audio_and_computed_spect(config, global_step, writer, audio, audio_pred, n=4):
    """Validation artefacts of a waveform model (reference train_utils.py:249-304): the first clip and its reconstruction as
    wav files, and a grid of the log-mel spectrograms of the first `n` pairs.  The mel front end is this build's HIP
    kernel (the reference's own MelSpectrogram, log of the mel-filtered MAGNITUDE) instead of librosa's power-dB
    spectrogram, which is not available offline; the image is a greyscale PNG."""
    from datasets.transforms import MelSpectrogram
    ds, log_dir = config.dataset, config.train.log_dir
    for sub in ("audio", "spect"):
        os.makedirs(os.path.join(log_dir, sub), exist_ok=True)
    audio, audio_pred = audio.detach().float().clamp(-1, 1), audio_pred.detach().float().clamp(-1, 1)
    write_wav(os.path.join(log_dir, "audio", f"val_audio_{global_step}_gt.wav"), audio[0].cpu().numpy(), ds.sample_rate)
    write_wav(os.path.join(log_dir, "audio", f"val_audio_{global_step}_pred.wav"), audio_pred[0].cpu().numpy(), ds.sample_rate)
    k = min(n, audio.shape[0])
    device = audio.device if audio.is_cuda else torch.device("cuda")
    mel = MelSpectrogram(sample_rate=ds.sample_rate, n_fft=ds.n_fft, win_length=ds.win_length, hop_length=ds.hop_length,
                         n_mels=ds.n_mels, f_min=0.0, f_max=8000.0).to(device)
    spect, spect_pred = mel(audio[:k].to(device)).cpu().numpy(), mel(audio_pred[:k].to(device)).cpu().numpy()
    grid = spects_to_grid(spect, spect_pred, n=k)
    path = os.path.join(log_dir, "spect", f"val_spect_{global_step}.png")
    write_png_gray(path, grid)
    tb = getattr(writer, "_tb", None)
    if tb is not None:
        tb.add_image("mel/val", grid, global_step, dataformats="HW")
        tb.add_audio("audio/val_gt", audio[0].cpu(), global_step=global_step, sample_rate=ds.sample_rate)
        tb.add_audio("audio/val_pred", audio_pred[0].cpu(), global_step=global_step, sample_rate=ds.sample_rate)
    return path


@torch.no_grad()
def save_spect_and_inverted_audio(config, global_step, writer, spect, spect_pred, lens, n=4):
    """Validation artefacts of a spectrogram model (reference train_utils.py:198-246): a grid of the first `n` pairs of
    log-mels, each trimmed to its lens[i] frames, as spect/val_spect_<step>.png, and the first pair inverted to audio --
    audio/val_audio_<step>_gt.wav and _syn.wav -- by datasets.transforms.GriffinLim on the device (32 NNLS updates, 32
    iterations of fast Griffin-Lim at momentum 0.99; the reference calls librosa.feature.inverse.mel_to_audio).  spect,
    spect_pred: sequences of [n_mels, frames_i] tensors.  A pair too short to invert is skipped with a log line."""
    from datasets.transforms import GriffinLim
    from smt_amd.spectral import invertible
    ds, log_dir = config.dataset, config.train.log_dir
    for sub in ("audio", "spect"):
        os.makedirs(os.path.join(log_dir, sub), exist_ok=True)
    k = min(n, len(spect), len(spect_pred))
    lens = [int(v) for v in lens[:k]]
    lens_pred = [min(lens[i], spect_pred[i].shape[-1]) for i in range(k)]
    gts = [spect[i][:, :lens[i]].detach().float().cpu().numpy() for i in range(k)]
    preds = [spect_pred[i][:, :lens_pred[i]].detach().float().cpu().numpy() for i in range(k)]
    drawn = [i for i in range(k) if lens[i] > 0 and lens_pred[i] > 0]
    path = os.path.join(log_dir, "spect", f"val_spect_{global_step}.png")
    grid = None
    if drawn:
        grid = spects_to_grid([gts[i] for i in drawn], [preds[i] for i in drawn], n=len(drawn))
        write_png_gray(path, grid)
    tb = getattr(writer, "_tb", None)
    if tb is not None and grid is not None:
        tb.add_image("mel/val", grid, global_step, dataformats="HW")
    if k == 0 or not (invertible(lens[0], ds.n_fft, ds.hop_length) and invertible(lens_pred[0], ds.n_fft, ds.hop_length)):
        logger.info("validation audio of step %s skipped: the first spectrogram pair is too short to invert (%s frames)",
                    global_step, (lens[0], lens_pred[0]) if k else 0)
        return path
    device = spect[0].device if spect[0].is_cuda else torch.device("cuda")
    frames = max(lens[0], lens_pred[0])
    pair = torch.zeros(2, gts[0].shape[0], frames, device=device)
    pair[0, :, :lens[0]] = spect[0][:, :lens[0]].detach().float().to(device)
    pair[1, :, :lens_pred[0]] = spect_pred[0][:, :lens_pred[0]].detach().float().to(device)
    wave, wave_lens = GriffinLim(config).to(device)(pair, torch.tensor([lens[0], lens_pred[0]]))
    wave = wave.clamp(-1, 1).cpu()
    for i, name in enumerate(("gt", "syn")):
        audio = wave[i, :int(wave_lens[i])]
        write_wav(os.path.join(log_dir, "audio", f"val_audio_{global_step}_{name}.wav"), audio.numpy(), ds.sample_rate)
        if tb is not None:
            tb.add_audio("audio/val_gt" if i == 0 else "audio/val_pred", audio, global_step=global_step, sample_rate=ds.sample_rate)
    return path


def print_top_level_summary(model):
    rows = []
    for name, module in model.named_children():
        n_params = sum(p.numel() for p in module.parameters() if p.requires_grad)
        n_buffers = sum(b.numel() for b in module.buffers())
        rows.append(f"  {name:<20s} {type(module).__name__:<32s} params {n_params:>12,d}  buffers {n_buffers:>10,d}")
    total = sum(p.numel() for p in model.parameters() if p.requires_grad)
    print("\n".join(rows) + f"\n  trainable parameters: {total:,d} ({total * 4e-6:,.1f} MB fp32)\n")
