"""VQTTS (reference models/vqtts/vqtts.py:16-191): a waveform VQ-VAE whose codebook is conditioned on the text.  The text
encoder's means and the audio encoder's frames are aligned monotonically; each frame is quantised among the ``l_bins`` codes
of the token it is aligned to; a code predictor learns, from the text side alone, which of them the quantiser chose; the
audio decoder turns the quantised frames back into a waveform.  Synthesis (``infer``) runs text encoder -> durations ->
code predictor -> codebook rows -> audio decoder.  Single speaker.  DESIGN.md section 14 has the composition table.

The reference's own ``forward`` cannot run as written (it builds the flat ``BottleneckBlock`` and calls it with the grouped
signature, its ``matmul(x_enc, attn)`` needs B = 1, its live eval line indexes the codebook with a relative code); the three
places where this model therefore departs from the text of the reference:
  * the codebook is the grouped ``models.vqtts.Bottleneck`` with ``n_vocab * l_bins`` codes (vqtts.py:74-76 builds l_bins);
  * eval-mode ``yh`` decodes the PREDICTED absolute code ``token * l_bins + argmax`` (the commented lines 170-174, not the
    live 175-178);
  * ``loss_ce`` / ``q_acc`` leave out the frames without a token or past ``q_lens`` (models/vqtts/predictor.py).
"""
import math

import torch

from models.base import TokenToWaveformModel, sentence_to_ids, text_frontend, token_batch
from models.glow_tts import submodules
from models.glow_tts.modules import TextEncoder
from models.vqtts.align import TextAudioAlignment
from models.vqtts.bottleneck import Bottleneck
from models.vqtts.predictor import CodePredictor
from models.vqvae.encdec import Decoder, Encoder
from models.vqvae.losses import MultiNormReconstructionLoss, MultiResolutionSpectralLoss
from smt_amd import glow, packing, profiler, vqtts

PARTS = ("x_enc", "logw_enc", "x_lens", "y_enc", "q_lens", "align_idx", "durations", "q_rel", "y_d", "pred")
PREDICTOR_SEED_BIT = 1 << 31        # the predictor's dropout seed is the step counter with this bit set


class VQTTS(TokenToWaveformModel):

    def __init__(self, config):
        super().__init__()
        m, ds = config.model, config.dataset
        if m.n_speakers > 1:
            raise ValueError("n_speakers > 1 (speaker embeddings) has no native path; configs/models/vqtts.yaml is single-speaker")
        e = m.encoder
        if e.out_channels != m.emb_width:
            raise ValueError(f"encoder.out_channels ({e.out_channels}) must equal emb_width ({m.emb_width}): text and audio "
                             "encodings are compared frame by token")
        multipliers = list(m.multipliers) if m.get("multipliers") is not None else [1] * m.levels
        # ONE encoder and ONE decoder with all levels chained, at the last multiplier (vqtts.py:24-57)
        block_kwargs = dict(
            width=m.width * multipliers[-1], depth=m.depth * multipliers[-1], m_conv=m.get("m_conv", 1.0),
            dilation_growth_rate=m.dilation_growth_rate, dilation_cycle=m.get("dilation_cycle"),
            kernel_size_growth_rate=m.kernel_size_growth_rate, kernel_size_cycle=m.get("kernel_size_cycle"),
            zero_out=m.zero_out, dropout=m.get("dropout", 0.1))
        self.audio_encoder = Encoder(1, m.emb_width, m.levels, m.downs_t, m.strides_t, m.block_type, site_base=0, **block_kwargs)
        self.audio_decoder = Decoder(1, m.emb_width, m.levels, m.downs_t, m.strides_t, m.block_type,
                                     site_base=self.audio_encoder.n_sites,
                                     reverse_decoder_dilation=m.get("reverse_decoder_dilation", False), **block_kwargs)
        self.stride = math.prod(s ** d for s, d in zip(m.strides_t, m.downs_t))
        # the text encoder's dropout sites are numbered after the audio stacks' (one seed, disjoint sites)
        self.sites = submodules._Sites()
        for i in range(self.audio_encoder.n_sites):
            self.sites.add(f"audio_encoder.{i}")
        for i in range(self.audio_decoder.n_sites):
            self.sites.add(f"audio_decoder.{i}")
        n_vocab = e.n_vocab + int(bool(ds.get("intersperse_blanks", False)))
        self.text_encoder = TextEncoder(n_vocab=n_vocab, out_channels=e.out_channels, hidden_channels=e.hidden_channels,
                                        filter_channels=e.filter_channels,
                                        filter_channels_dp=e.filter_channels,     # as the reference passes it (vqtts.py:64)
                                        n_heads=e.n_heads, n_layers=e.n_layers, kernel_size=e.kernel_size, p_dropout=e.p_dropout,
                                        window_size=e.window_size, mean_only=e.mean_only, prenet=e.prenet,
                                        gin_channels=m.gin_channels, sites=self.sites)
        self.quant_bottleneck = Bottleneck(n_vocab, m.l_bins, m.emb_width, m.mu, m.revival_threshold)
        # The predictor's two modules are registered HERE, under the reference's names, so state_dict() / named_parameters()
        # carry `quant_decoder.*` and `quant_proj.*` once and without a prefix; the predictor itself is held outside the
        # module tree (train() below reaches it; .to() moves the shared modules).
        predictor = CodePredictor(e.out_channels, m.l_bins, p_dropout=m.get("dropout", 0.1))
        self.quant_decoder, self.quant_proj = predictor.quant_decoder, predictor.quant_proj
        object.__setattr__(self, "predictor", predictor)
        self.align = TextAudioAlignment()

        loss = m.loss
        self.multi_stft_loss = MultiResolutionSpectralLoss(n_ffts=loss.n_ffts, hop_lengths=loss.hop_lengths,
                                                           win_lengths=loss.win_lengths, window=loss.window, log=loss.log)
        self.multi_recon_loss = MultiNormReconstructionLoss(l1=loss.l1, l2=loss.l2, linf=loss.linf, linf_topk=loss.linf_topk)
        self.n_vocab, self.l_bins = n_vocab, m.l_bins
        self.l_commit, self.l_stft, self.l_align = loss.commit, loss.multispectral, loss.align
        self.compute_dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[m.get("compute_dtype", "fp32")]
        for stage in self.audio_encoder.level_blocks:
            stage.act_dtype = self.compute_dtype
        self._drop_seed = 0
        self.text_parser, self.intersperse_blanks = text_frontend(config, e.n_vocab)

    def train(self, mode=True):
        self.predictor.train(mode)
        return super().train(mode)

    def dropout_sites(self):
        """Site name -> id of the audio stacks' and the text encoder's dropouts (the predictor numbers its own 0-7 under its
        own seed)."""
        return {n: i for i, n in enumerate(self.sites.names)}

    # checkpoints written by the reference carry the DFT-basis buffers of the loss; derived data here (as VQVAE)
    def load_state_dict(self, state_dict, strict=True, **kw):
        state_dict = {k: v for k, v in state_dict.items() if not k.endswith("_basis")}
        return super().load_state_dict(state_dict, strict=strict, **kw)

    @packing.forward_scope
    def forward(self, x, x_lengths, y, y_lengths, speaker=None, *, return_parts=False):
        """x [B, Tx] int64 token ids, y [B, 1, T] fp32 in [-1, 1] with T a multiple of the total stride ->
        ({loss, loss_recon, loss_stft, loss_commit, loss_dur, loss_align, loss_ce, yh [B, T]}, {q_acc, + the quantiser's
        metrics in training mode}); ``return_parts`` adds the dict of the intermediate tensors named in ``PARTS``."""
        assert speaker is None
        b, c, t = y.shape
        assert c == 1 and t % self.stride == 0, f"y must be [B, 1, T] with T a multiple of {self.stride}, got {tuple(y.shape)}"
        self._drop_seed += 1
        seed = self._drop_seed
        if x_lengths is None:
            x_lengths = torch.full((b,), x.shape[1], device=x.device)
        if y_lengths is None:
            y_lengths = torch.full((b,), t, device=y.device)
        y_lens = y_lengths.to(torch.int32)
        target = y.reshape(b, t)

        stage = profiler.region                        # per-stage device time when smt_amd.profiler is on (tools/bench_vqtts_step.py)
        with stage("vqtts:text_encoder"):
            x_enc, _, logw_enc, x_lens = self.text_encoder(x, x_lengths, seed)
        with stage("vqtts:audio_encoder"):
            y_enc, q_lens = self.audio_encoder(target, y_lens, seed)
            y_enc = y_enc.float()
        with stage("vqtts:align"):
            align_idx, durations, loss_align = self.align(x_enc, x_lens, y_enc, q_lens)
        with stage("vqtts:quantise"):
            q_rel, y_d, loss_commit, vq_metrics = self.quant_bottleneck(y_enc, x, align_idx)
        with stage("vqtts:predictor"):
            loss_ce, q_acc, pred = self.predictor(x_enc, align_idx, q_lens, target=q_rel, drop_seed=seed | PREDICTOR_SEED_BIT)
        with stage("vqtts:audio_decoder"):
            y_h, _ = self.audio_decoder(y_d.to(self.compute_dtype), q_lens, seed)
        assert y_h.shape == (b, t), f"Expected shape {(b, t)}, got {tuple(y_h.shape)}."

        with stage("vqtts:losses"):
            loss_recon = self.multi_recon_loss(target, y_h, y_lens)
            loss_stft = self.multi_stft_loss(target, y_h, y_lens)
            loss_dur = glow.length_loss(logw_enc, durations, x_lens, x_lengths.sum().float())
            loss = (loss_recon + self.l_stft * loss_stft + self.l_commit * loss_commit + loss_dur + self.l_align * loss_align
                    + loss_ce)
        if not self.training:             # what synthesis would produce from these alignments: the PREDICTED codes
            with torch.no_grad():
                y_pred, _ = vqtts.emit_codes(pred, x, align_idx, q_lens, self.quant_bottleneck.k, self.n_vocab, self.l_bins)
                y_h, _ = self.audio_decoder(y_pred.to(self.compute_dtype), q_lens)
        out = {"loss": loss, "loss_recon": loss_recon, "loss_stft": loss_stft, "loss_commit": loss_commit, "loss_dur": loss_dur,
               "loss_align": loss_align / (1 + self.l_align), "loss_ce": loss_ce, "yh": y_h}
        metrics = {"q_acc": q_acc, **(vq_metrics if self.training else {})}
        if return_parts:
            parts = dict(zip(PARTS, (x_enc, logw_enc, x_lens, y_enc, q_lens, align_idx, durations, q_rel, y_d, pred)))
            return out, metrics, parts
        return out, metrics

    @torch.no_grad()
    def infer(self, x, x_lengths=None, *, length_scale=1.0, temperature=0.0, min_p=0.0, seed=None):
        """Waveforms from token ids: x [B, Tx] integer ids, ragged with x_lengths [B] -> (wave [B, T_out * stride] fp32,
        wave_lengths [B] int64), T_out = the longest item's frames, wave exactly 0 at or past wave_lengths[b].

        text encoder -> smt_glow_durations (w = ceil(exp(logw) length_scale), prefix sums, lengths) -> ONE host read of the
        lengths -> smt_glow_duration_index (frame -> token) -> code predictor (argmax of the code head) -> smt_vqtts_emit
        (absolute code and codebook row of every frame) -> audio decoder.  Invalid inputs raise ValueError before the
        launch they would corrupt: the checks of ``models.base.token_batch``, length_scale <= 0, and an item whose
        durations are not finite or sum past 2^24 frames.

        ``temperature`` > 0 draws every frame's code from softmax(logits / temperature) instead (inside the code head,
        smt_vqtts_code_head_sample), among the codes with p >= ``min_p`` * p_max; it needs ``seed``: an int (item b draws
        with (seed + b) mod 2^31) or a sequence of B ints.  Equal seeds give equal waveforms; a frame's draw depends on its item's
        seed, its index and its own logits only, not on the batch around it.  ``temperature`` = 0 is the argmax and takes
        neither."""
        if self.training:
            raise RuntimeError(f"{type(self).__name__}.infer needs evaluation mode: call .eval() first")
        if not (math.isfinite(length_scale) and length_scale > 0):
            raise ValueError(f"length_scale must be a finite number > 0, got {length_scale}")
        if not (math.isfinite(temperature) and temperature >= 0):
            raise ValueError(f"temperature must be a finite number >= 0, got {temperature}")
        if not 0.0 <= min_p <= 1.0:
            raise ValueError(f"min_p must lie in [0, 1], got {min_p}")
        if temperature == 0 and (min_p != 0 or seed is not None):
            raise ValueError("min_p and seed apply to sampling: temperature = 0 is the argmax of the code head")
        if temperature > 0 and seed is None:
            raise ValueError("temperature > 0 draws the codes and needs seed= (an int, or one int per item)")
        dev = self.text_encoder.emb.weight.device
        xc, lens, valid = token_batch(x, x_lengths, self.n_vocab)
        b = xc.shape[0]
        seeds = None
        if temperature > 0:
            if isinstance(seed, int) and not isinstance(seed, bool):
                seeds = [(seed + i) % 2 ** 31 for i in range(b)]
            else:
                seeds = list(seed.tolist() if isinstance(seed, torch.Tensor) else seed)
                if len(seeds) != b or not all(isinstance(v, int) and not isinstance(v, bool) for v in seeds):
                    raise ValueError(f"seed must be an int or a sequence of {b} ints (one per item), got {len(seeds)} values")
                seeds = [v % 2 ** 31 for v in seeds]
        x_dev = torch.where(valid, xc, 0).to(dev)
        x_enc, _, logw, lens32 = self.text_encoder(x_dev, lens.to(dev))
        _, z_lens, cum = glow.durations(logw, lens32, length_scale, 1)
        z_host = z_lens.cpu()                                          # the one host read
        invalid = (z_host < 0).nonzero().flatten().tolist()
        if invalid:
            raise ValueError(f"item {invalid[0]}: the predicted durations are not finite or sum past 2^24 frames "
                             f"(length_scale {length_scale}; invalid items: {invalid})")
        t_out = int(z_host.max())
        wave_lengths = (z_host.long() * self.stride).to(dev)
        if t_out == 0:
            return torch.zeros(b, 0, device=dev), wave_lengths
        idx = glow.duration_index(cum, lens32, z_lens, t_out)
        sample = (temperature, min_p, torch.tensor(seeds, dtype=torch.int32).to(dev)) if seeds is not None else None
        pred = self.predictor(x_enc, idx, z_lens, sample=sample)
        y_d, _ = vqtts.emit_codes(pred, x_dev, idx, z_lens, self.quant_bottleneck.k, self.n_vocab, self.l_bins)
        wave, _ = self.audio_decoder(y_d.to(self.compute_dtype), z_lens)
        keep = torch.arange(wave.shape[1], device=dev)[None, :] < wave_lengths[:, None]
        return torch.where(keep, wave.float(), 0.0), wave_lengths

    @torch.no_grad()
    def infer_step(self, t, speaker=None):
        """One utterance -> wave [1, T]: its token ids (a list or a 1-D tensor), or, on a model configured with
        ``dataset.text_frontend``, the sentence itself, turned into ids as the dataset does for training (blanks included;
        DESIGN.md section 18).  ValueError for a text that leaves no symbol."""
        if isinstance(t, str):
            t = sentence_to_ids(self, t)
        if speaker is not None:
            raise ValueError("speaker embeddings (n_speakers > 1) have no native path; configs/models/vqtts.yaml is single-speaker")
        x = torch.as_tensor(t)
        if x.dim() != 1:
            raise ValueError(f"infer_step takes one utterance's token ids (1-D), got shape {tuple(x.shape)}")
        wave, _ = self.infer(x.unsqueeze(0))
        return wave
