"""Synthesis from token ids or text with a trained token-to-spectrogram or token-to-waveform model (the reference's `infer_step`,
batched): mel spectrograms from a GlowTTS, waveforms from a VQTTS.

    python -m scripts.synthesize --log_dir ./logs/glow_tts --ckpt_num 5000 (--tokens utterances.txt | --text sentences.txt) --dump_dir ./outputs \
        [--batch_size 16] [--noise_scale 0.667] [--length_scale 1.0] [--seed 0] [--temperature 0] [--min_p 0] [--speaker N] \
        [--vocoder griffin_lim [--gl_iters 32]]

``--tokens`` holds one utterance per line as whitespace-separated integer ids (the ids of datasets/synthetic.py, or the ones
models/parser.py emits).  ``--text`` holds one sentence per line instead, for a checkpoint trained with
``dataset.text_frontend``: the sentences go through that front end as the dataset's transcripts did.
Exactly one of the two is given.  Writes
``<dump_dir>/<ModelClass>@<ckpt>/mel_<i>.npy`` (float32 [n_mels, frames], trimmed to the utterance's length) and one
``mel_spectrograms.png``.  Synthesis runs on MI355X through libsmt_hip.so (`GlowTTS.infer`).  With ``--vocoder griffin_lim``
every spectrogram is also inverted to ``wav_<i>.wav`` (16-bit mono, ``frames * hop_length`` samples, clamped to [-1, 1]) on the
device: 32 non-negative least-squares updates back to linear magnitudes, then ``--gl_iters`` iterations of fast Griffin-Lim at
momentum 0.99 (datasets.transforms.GriffinLim).  Utterance i starts from the phases of seed ``--seed`` + i
whatever ``--batch_size``.  There is no neural vocoder; without the flag the outputs are the spectrograms alone.

A token-to-waveform model (VQTTS, `VQTTS.infer`) writes ``wav_<i>.wav`` (16-bit mono at the dataset's sample rate, trimmed to
the utterance's length) and the log-mel spectrograms of the waveforms as ``mel_spectrograms.png``; it has no prior noise,
so ``--noise_scale`` other than 1 is refused for it, and it makes waveforms itself, so ``--vocoder`` is refused too.  ``--temperature`` > 0 draws its codes instead of taking the argmax
(``--min_p`` truncates the draw); utterance i of the tokens file draws with seed ``--seed`` + i whatever ``--batch_size``.  GlowTTS
has no codes and refuses both flags.  ``--speaker N`` is the voice of every utterance: required by a multi-speaker GlowTTS
checkpoint (``n_speakers`` > 1 in its config), an error for any other model."""
import argparse
import logging
import math
import os

import numpy as np
import torch

from scripts.sample_from_lm import mel_grid
from utils import config as cfglib
from utils.commons import get_model
from utils.train_utils import write_png_gray, write_wav

logger = logging.getLogger(__name__)


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--log_dir", type=str, required=True, help="Log directory of training")
    p.add_argument("--ckpt_num", type=int, required=True, help="Checkpoint number to load")
    p.add_argument("--tokens", type=str, default=None, help="One utterance per line: whitespace-separated token ids")
    p.add_argument("--text", type=str, default=None,
                   help="One sentence per line, for a checkpoint trained with dataset.text_frontend (instead of --tokens)")
    p.add_argument("--dump_dir", type=str, default="./outputs", help="Directory to dump the spectrograms")
    p.add_argument("--batch_size", type=int, default=16, help="Utterances per inference call")
    p.add_argument("--noise_scale", type=float, default=1.0, help="Scale of the prior noise (1 = the reference)")
    p.add_argument("--length_scale", type=float, default=1.0, help="Scale of the predicted durations (1 = the reference)")
    p.add_argument("--seed", type=int, default=0, help="Seed of the prior noise (GlowTTS) or of the code draws (VQTTS, --temperature > 0)")
    p.add_argument("--temperature", type=float, default=0.0, help="VQTTS: temperature of the code draw (0 = argmax)")
    p.add_argument("--min_p", type=float, default=0.0, help="VQTTS: draw among the codes with p >= min_p * p_max (0 = all)")
    p.add_argument("--speaker", type=int, default=None, help="Multi-speaker GlowTTS: the speaker id of every utterance")
    p.add_argument("--vocoder", type=str, default=None, choices=["griffin_lim"],
                   help="GlowTTS: also invert every spectrogram to wav_<i>.wav on the device")
    p.add_argument("--gl_iters", type=int, default=None, help="Iterations of fast Griffin-Lim with --vocoder griffin_lim (32)")
    args = p.parse_args(argv)
    args.gl_iters_given = args.gl_iters is not None
    if args.gl_iters is None:
        args.gl_iters = 32
    return args


def read_tokens(path):
    """Non-empty lines -> lists of ints."""
    with open(path, encoding="utf-8") as f:
        rows = [line.split() for line in f]
    try:
        return [[int(v) for v in r] for r in rows if r]
    except ValueError as e:
        raise ValueError(f"{path}: every line must hold whitespace-separated integer token ids ({e})") from None


def read_sentences(path):
    """Non-empty lines, stripped."""
    with open(path, encoding="utf-8") as f:
        return [line.strip() for line in f if line.strip()]


def sentences_to_tokens(model, sentences, path):
    """The ids the checkpoint's own text front end gives (as its dataset made them for training, blanks included)."""
    from models.parser import sentence_ids
    if getattr(model, "text_parser", None) is None:
        raise ValueError("--text needs a checkpoint whose config sets dataset.text_frontend (chars or cmudict); this one was "
                         "trained on token ids: use --tokens")
    out = []
    for i, sentence in enumerate(sentences):
        try:
            out.append(sentence_ids(model.text_parser, sentence, model.intersperse_blanks))
        except ValueError as e:
            raise ValueError(f"{path}, sentence {i}: {e}") from None
    return out


def batches(utterances, batch_size):
    """(padded ids [B, Tx] int64, lengths [B]) per batch."""
    for lo in range(0, len(utterances), batch_size):
        part = utterances[lo:lo + batch_size]
        x = torch.zeros(len(part), max(len(t) for t in part), dtype=torch.int64)
        for i, t in enumerate(part):
            x[i, :len(t)] = torch.tensor(t, dtype=torch.int64)
        yield x, torch.tensor([len(t) for t in part])


def draw_mels(dump_dir, mels):
    drawn = [m for m in mels if m.shape[1] > 0]
    if drawn:
        width = max(m.shape[1] for m in drawn)
        write_png_gray(os.path.join(dump_dir, "mel_spectrograms.png"),
                       mel_grid([np.pad(m, ((0, 0), (0, width - m.shape[1])), constant_values=m.min()) for m in drawn]))


def refuse_vocoder_for(model):
    raise ValueError(f"--vocoder applies to a token-to-spectrogram model; {type(model).__name__} makes waveforms itself")


def vocode(config, yh, y_lengths, first, args, dump_dir, device):
    """wav_<first + i>.wav of one batch of spectrograms; utterance number j starts from the phases of seed --seed + j.  An
    utterance too short to invert (fewer samples than the reflect padding) is written as silence of its length."""
    from datasets.transforms import GriffinLim
    from smt_amd.spectral import invertible
    ds = config.dataset
    lengths = [int(n) for n in y_lengths.tolist()]
    ok = [invertible(n, ds.n_fft, ds.hop_length) for n in lengths]
    frames = torch.tensor([n if k else 0 for n, k in zip(lengths, ok)])
    wave, _ = GriffinLim(config).to(device)(yh.float(), frames, n_iter=args.gl_iters,
                                            seed=[(args.seed + first + i) % (1 << 31) for i in range(len(lengths))])
    wave = wave.clamp(-1, 1).cpu().numpy()
    for i, n in enumerate(lengths):
        samples = n * ds.hop_length
        if not ok[i] and n > 0:
            logger.info("utterance %d has %d frames: too short to invert, written as silence", first + i, n)
        out = np.zeros(samples, dtype=np.float32)
        out[:min(samples, wave.shape[1])] = wave[i, :samples]
        write_wav(os.path.join(dump_dir, f"wav_{first + i}.wav"), out, ds.sample_rate)


def synthesize_waveforms(model, config, utterances, args, dump_dir, device):
    """The token-to-waveform branch: wav files and the log-mel image of what was synthesized."""
    from datasets.transforms import MelSpectrogram
    if args.noise_scale != 1.0:
        raise ValueError(f"--noise_scale applies to GlowTTS's prior; {type(model).__name__} has no noise input")
    ds = config.dataset
    mel = MelSpectrogram(sample_rate=ds.sample_rate, n_fft=ds.n_fft, win_length=ds.win_length, hop_length=ds.hop_length,
                         n_mels=ds.n_mels, f_min=0.0, f_max=8000.0).to(device)
    mels, count = [], 0
    for x, x_lengths in batches(utterances, args.batch_size):
        draw = dict(temperature=args.temperature, min_p=args.min_p,
                    seed=[args.seed + count + i for i in range(x.shape[0])]) if args.temperature > 0 else {}
        wave, wave_lengths = model.infer(x, x_lengths, length_scale=args.length_scale, **draw)
        for i, n in enumerate(wave_lengths.tolist()):
            write_wav(os.path.join(dump_dir, f"wav_{count}.wav"), wave[i, :n].clamp(-1, 1).cpu().numpy(), ds.sample_rate)
            count += 1
            if n >= ds.n_fft:
                mels.append(mel(wave[i:i + 1, :n].clamp(-1, 1))[0].cpu().numpy())
    draw_mels(dump_dir, mels)
    logger.info("Saved %d waveforms under %s", count, dump_dir)
    return dump_dir


def main(argv=None):
    args = parse_args(argv)
    if (args.tokens is None) == (args.text is None):
        raise ValueError("exactly one of --tokens (integer ids) and --text (sentences) must be given, got "
                         + ("both" if args.tokens is not None else "neither"))
    if args.batch_size < 1:
        raise ValueError("--batch_size must be >= 1")
    if not (math.isfinite(args.temperature) and args.temperature >= 0):
        raise ValueError(f"--temperature must be a finite number >= 0, got {args.temperature}")
    if not 0.0 <= args.min_p <= 1.0 or (args.temperature == 0 and args.min_p != 0):
        raise ValueError(f"--min_p must lie in [0, 1] and applies to --temperature > 0 only, got {args.min_p}")
    if args.gl_iters < 0:
        raise ValueError(f"--gl_iters must be >= 0, got {args.gl_iters}")
    if args.gl_iters_given and args.vocoder is None:
        raise ValueError("--gl_iters applies to --vocoder griffin_lim")
    if not torch.cuda.is_available():
        raise RuntimeError("synthesize runs the model on MI355X (libsmt_hip.so); no GPU is visible")
    source = args.tokens if args.tokens is not None else args.text
    utterances = read_tokens(source) if args.tokens is not None else read_sentences(source)
    if not utterances:
        raise ValueError(f"{source} holds no utterance")
    device = torch.device("cuda")
    config = cfglib.load(os.path.join(args.log_dir, "config.yaml"))
    config.train.n_gpus = 1
    ckpt = torch.load(os.path.join(args.log_dir, "ckpts", f"ckpt.{args.ckpt_num}.pt"), map_location=device, weights_only=True)
    model, _ = get_model(config, device=device)
    model.load_state_dict(ckpt["model"])
    model.eval()
    if args.text is not None:
        utterances = sentences_to_tokens(model, utterances, source)
    dump_dir = os.path.join(args.dump_dir, f"{type(model).__name__}@{args.ckpt_num}")
    os.makedirs(dump_dir, exist_ok=True)

    from models.base import TokenToWaveformModel
    n_speakers = int(getattr(model, "n_speakers", 1))
    if n_speakers > 1 and args.speaker is None:
        raise ValueError(f"this checkpoint has {n_speakers} speakers: --speaker N (0 <= N < {n_speakers}) is required")
    if n_speakers <= 1 and args.speaker is not None:
        raise ValueError(f"--speaker applies to a multi-speaker GlowTTS checkpoint; this {type(model).__name__} is single-speaker")
    if n_speakers > 1 and not 0 <= args.speaker < n_speakers:
        raise ValueError(f"--speaker must lie in [0, {n_speakers}), got {args.speaker}")
    if isinstance(model, TokenToWaveformModel) and args.vocoder is not None:
        refuse_vocoder_for(model)
    if isinstance(model, TokenToWaveformModel):
        return synthesize_waveforms(model, config, utterances, args, dump_dir, device)
    if args.temperature != 0.0 or args.min_p != 0.0:
        raise ValueError(f"--temperature and --min_p apply to a token-to-waveform model's code draw; {type(model).__name__} has no codes")
    torch.manual_seed(args.seed)
    mels = []
    for x, x_lengths in batches(utterances, args.batch_size):
        voice = {} if args.speaker is None else {"speaker": args.speaker}
        yh, y_lengths = model.infer(x, x_lengths, noise_scale=args.noise_scale, length_scale=args.length_scale, **voice)
        if args.vocoder is not None:
            vocode(config, yh, y_lengths, len(mels), args, dump_dir, device)
        yh = yh.cpu().numpy()
        mels += [np.ascontiguousarray(yh[i, :, :n], dtype=np.float32) for i, n in enumerate(y_lengths.tolist())]
    for i, m in enumerate(mels):
        np.save(os.path.join(dump_dir, f"mel_{i}.npy"), m)
    draw_mels(dump_dir, mels)
    logger.info("Saved %d spectrograms under %s", len(mels), dump_dir)
    return dump_dir


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
