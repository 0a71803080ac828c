"""GlowTTS (reference models/glow_tts/glow_tts.py:12-168): text encoder -> prior statistics, flow decoder -> latent, monotonic
alignment search between them ON THE DEVICE (the reference round-trips through numpy every step, glow_tts.py:87-97), MLE and
duration losses; synthesis from token ids (``infer`` / ``infer_step``).  One voice, or ``n_speakers`` > 1 voices: a speaker embedding
conditions every WN gate of the decoder and the duration predictor.  Activations are channels-last; the
public tensors keep the reference's layouts (spectrograms [B, n_mels, T])."""
import math

import torch
import torch.nn as nn

import models.glow_tts.submodules as submodules
from models.base import TokenToSpectrogramModel, sentence_to_ids, text_frontend, token_batch
from models.glow_tts.modules import FlowSpecDecoder, TextEncoder
from smt_amd import glow


class GlowTTS(TokenToSpectrogramModel):

    def __init__(self, config):
        super().__init__()
        m, ds = config.model, config.dataset
        self.n_speakers, gin = int(m.n_speakers), int(m.gin_channels or 0)
        if self.n_speakers > 1 and gin <= 0:
            raise ValueError(f"n_speakers = {self.n_speakers} needs gin_channels > 0 (the width of the speaker embedding), got {gin}")
        if self.n_speakers <= 1 and gin > 0:
            raise ValueError(f"gin_channels = {gin} needs n_speakers > 1: a single-speaker model has no speaker embedding to condition on")
        if self.n_speakers > 1:
            self.emb_g = nn.Embedding(self.n_speakers, gin)                # glow_tts.py:17-19: U(-0.1, 0.1), not normalised
            nn.init.uniform_(self.emb_g.weight, -0.1, 0.1)
            # 1 where a forward pass in training mode saw a speaker id outside [0, n_speakers) (`check_speaker_ids`)
            self.register_buffer("_speaker_bad", torch.zeros((), dtype=torch.bool), persistent=False)
        e, d = m.encoder, m.decoder
        self.sites = submodules._Sites()
        self.encoder = TextEncoder(n_vocab=e.n_vocab + int(bool(ds.get("intersperse_blanks", False))), out_channels=ds.n_mels,
                                   hidden_channels=e.hidden_channels, filter_channels=e.filter_channels,
                                   filter_channels_dp=e.filter_channels,          # as the reference passes it (glow_tts.py:27)
                                   n_heads=e.n_heads, n_layers=e.n_layers, kernel_size=e.kernel_size, p_dropout=e.p_dropout,
                                   window_size=e.window_size, mean_only=e.mean_only, prenet=e.prenet, gin_channels=gin,
                                   sites=self.sites)
        self.decoder = FlowSpecDecoder(in_channels=ds.n_mels, hidden_channels=d.hidden_channels, kernel_size=d.kernel_size,
                                       dilation_rate=d.dilation_rate, n_blocks=d.n_blocks, n_layers=d.n_layers, p_dropout=d.p_dropout,
                                       n_split=d.n_split, n_sqz=d.n_sqz, sigmoid_scale=d.sigmoid_scale, gin_channels=gin,
                                       sites=self.sites)
        self._drop_seed = 0
        self.text_parser, self.intersperse_blanks = text_frontend(config, e.n_vocab)

    def dropout_sites(self):
        """Site name -> id of every dropout in forward order (the oracle replays the masks by name)."""
        return {n: i for i, n in enumerate(self.sites.names)}

    @torch.no_grad()
    def ddi(self, batch):
        """Data-dependent initialisation of the ActNorm layers (glow_tts.py:49-56)."""
        self.train()
        for f in self.decoder.flows:
            if getattr(f, "set_ddi", False):
                f.set_ddi(True)
        _ = self.supervised_step(batch)

    def _speaker_embeddings(self, speaker, batch, device, on_host):
        """g [B, gin] = emb_g(speaker) for a multi-speaker model, None for a single-speaker one.  ``speaker``: int64 [B], or an
        int for all items.  ValueError when a single-speaker model gets a speaker, a multi-speaker model gets none, the shape
        or dtype is wrong, or an id lies outside [0, n_speakers).  Ids that already live on the device are range-checked on
        the host only when ``on_host`` (synthesis and evaluation, which read the device anyway); a training step must not
        wait for the device, so there they are clamped for the lookup and compared on the device: an item whose id was out of
        range gets a NaN embedding (the step's loss is NaN, never a silently wrong voice) and the sticky flag that
        ``check_speaker_ids`` turns into the ValueError."""
        if self.n_speakers <= 1:
            if speaker is not None:
                raise ValueError("this GlowTTS is single-speaker (n_speakers = 1): it takes no speaker ids")
            return None
        if speaker is None:
            raise ValueError(f"this GlowTTS has n_speakers = {self.n_speakers}: forward / infer need the speaker ids (int64 [B])")
        if isinstance(speaker, int) and not isinstance(speaker, bool):
            speaker = torch.full((batch,), speaker, dtype=torch.int64)
        ids = torch.as_tensor(speaker)
        if ids.shape != (batch,) or ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
            raise ValueError(f"speaker must be {batch} integer ids (int64 [B]), got {ids.dtype} of shape {tuple(ids.shape)}")
        checked = on_host or not ids.is_cuda
        if checked:
            host = ids.detach().cpu().long()
            bad = ((host < 0) | (host >= self.n_speakers)).nonzero().flatten().tolist()
            if bad:
                raise ValueError(f"item {bad[0]}: speaker id {int(host[bad[0]])} is outside [0, {self.n_speakers})")
        ids = ids.detach().to(device).long()
        safe = ids.clamp(0, self.n_speakers - 1)
        g = nn.functional.embedding(safe, self.emb_g.weight)
        if not checked:
            bad = ids != safe
            self._speaker_bad |= bad.any()
            g = torch.where(bad.unsqueeze(-1), torch.full_like(g, float("nan")), g)
        return g

    def check_speaker_ids(self):
        """ValueError if a training-mode forward since the last call saw a speaker id outside [0, n_speakers) on the device
        (one host read; train.py calls it when its NaN guard fires)."""
        if self.n_speakers > 1 and bool(self._speaker_bad):
            self._speaker_bad.zero_()
            raise ValueError(f"a speaker id outside [0, {self.n_speakers}) reached a training step (its item's embedding was set to NaN)")

    def forward(self, x, x_lengths, y, y_lengths, speaker=None, noise=None):
        """x [B, Tx] tokens, y [B, n_mels, Ty] log-mels, speaker int64 [B] (multi-speaker models only) ->
        ({loss_mle, loss_length, loss, yh}, {})."""
        g = self._speaker_embeddings(speaker, x.shape[0], x.device, on_host=not self.training)
        self._drop_seed += 1
        seed, n_sqz = self._drop_seed, self.decoder.n_sqz
        if x_lengths is None:
            x_lengths = torch.full((x.shape[0],), x.shape[1], device=x.device)
        x_m, x_logs, logw_enc, x_lens = self.encoder(x, x_lengths, seed, speaker_embeddings=g)
        y_max = (y.size(2) // n_sqz) * n_sqz
        if y_lengths is None:
            y_lengths = torch.full((y.shape[0],), y_max, device=y.device)
        y_lens = ((y_lengths // n_sqz) * n_sqz).to(torch.int32)
        spect = y[:, :, :y_max].transpose(1, 2).contiguous().float()                      # [B, Ty, n_mels]
        z_dec, logdet = self.decoder(spect, y_lens, speaker_embeddings=g, reverse=False, seed=seed)

        # monotonic alignment search on the device: prior log-likelihood -> smt_maximum_path -> frame -> token index
        with torch.no_grad():
            logp = glow.prior_logp(x_m, x_logs, z_dec)
            tx, ty = logp.shape[1], logp.shape[2]
            attn_mask = (submodules.sequence_mask(x_lens, tx).unsqueeze(-1) & submodules.sequence_mask(y_lens, ty).unsqueeze(1)).float()
            attn = submodules.maximum_path(logp, attn_mask)
            idx, durations = glow.align_index(attn)
        z_m = glow.align_gather(x_m, idx)
        z_logs = None if x_logs is None else glow.align_gather(x_logs, idx)

        yh = None
        if not self.training:
            with torch.no_grad():
                w = durations * submodules.sequence_mask(x_lens, tx).float()
                z_lens = ((torch.clamp_min(w.sum(1), 1).long() // n_sqz) * n_sqz).to(torch.int32)
                eps = torch.randn_like(z_m) if noise is None else noise.transpose(1, 2).contiguous()
                t_out = int(z_lens.max())              # sequence_mask(z_lengths, None): the mask is as long as the longest item
                z_enc = self._prior_sample(z_m, z_logs, eps, z_lens, t_out)
                yh_rows, _ = self.decoder(z_enc, z_lens, speaker_embeddings=g, reverse=True)
                yh = yh_rows.transpose(1, 2)
        denom = (y_lens.sum() * z_dec.shape[2]).float()
        l_mle = glow.mle_loss(z_dec, z_m, z_logs, torch.sum(logdet), denom)
        l_length = glow.length_loss(logw_enc, durations, x_lens, x_lengths.sum().float())
        return {"loss_mle": l_mle, "loss_length": l_length, "loss": l_mle + l_length, "yh": yh}, {}

    @staticmethod
    def _prior_sample(z_m, z_logs, eps, z_lens, t_out, noise_scale=1.0):
        """z = (z_m + exp(z_logs) noise_scale eps) on the first z_lens[b] frames of [B, T, n_mels] rows, exactly 0 after
        (glow_tts.py:110, 165); rows of eps past z_lens[b] are selected away, so they may hold anything, NaN included."""
        scale = torch.exp(z_logs) if z_logs is not None else 1.0
        if noise_scale != 1.0:
            scale = scale * noise_scale
        keep = submodules.sequence_mask(z_lens, t_out).unsqueeze(-1)
        return torch.where(keep, (z_m + scale * eps)[:, :t_out], 0.0).contiguous()

    @torch.no_grad()
    def infer(self, x, x_lengths=None, *, noise_scale=1.0, length_scale=1.0, noise=None, speaker=None):
        """Mels from token ids (glow_tts.py:133-168 from the token ids on): x [B, Tx] int64, ragged with x_lengths [B] ->
        (yh [B, n_mels, T_out] fp32, y_lengths [B] int64), T_out = max y_lengths and yh exactly 0 at or past y_lengths[b].

        encoder -> smt_glow_durations (w = ceil(exp(logw) length_scale), prefix sums, lengths) -> ONE host read of the lengths
        (the reference syncs there too) -> smt_glow_duration_index (frame -> token) -> align_gather of x_m / x_logs ->
        z = (z_m + exp(z_logs) noise_scale eps) mask -> decoder(z, reverse=True).  eps = ``noise`` ([B, n_mels, T_out], the
        layout of ``forward``'s noise; frames past y_lengths[b] are never read) or a torch.randn draw in that layout.
        noise_scale = length_scale = 1 is the reference's computation.  Invalid inputs raise ValueError before the launch
        they would corrupt: token ids outside [0, n_vocab) or an empty item (ids are checked on the host, as they come from
        outside the program), length_scale <= 0, noise_scale < 0, a noise tensor of the wrong shape, and an item whose
        durations are not finite or sum past 2^24 frames (smt_glow_durations returns -1 for it).  ``speaker``: int64 [B] or one
        int for all items -- required by a multi-speaker model, refused by a single-speaker one, range-checked on the host."""
        if self.training:
            raise RuntimeError(f"{type(self).__name__}.infer needs evaluation mode: call .eval() first")
        if not (math.isfinite(length_scale) and length_scale > 0):
            raise ValueError(f"length_scale must be a finite number > 0, got {length_scale}")
        if not (math.isfinite(noise_scale) and noise_scale >= 0):
            raise ValueError(f"noise_scale must be a finite number >= 0, got {noise_scale}")
        dev, n_vocab = self.encoder.emb.weight.device, self.encoder.emb.num_embeddings
        n_mels, n_sqz = self.decoder.flows[0].channels // self.decoder.n_sqz, self.decoder.n_sqz
        xc, lens, valid = token_batch(x, x_lengths, n_vocab)
        b, tx = xc.shape
        if noise is not None and (noise.dim() != 3 or tuple(noise.shape[:2]) != (b, n_mels)):
            raise ValueError(f"noise must be [B={b}, n_mels={n_mels}, T_out], got shape {tuple(noise.shape)}")

        g = self._speaker_embeddings(speaker, b, dev, on_host=True)
        x_m, x_logs, logw, lens32 = self.encoder(torch.where(valid, xc, 0).to(dev), lens.to(dev), speaker_embeddings=g)
        _, z_lens, cum = glow.durations(logw, lens32, length_scale, n_sqz)
        z_host = z_lens.cpu()                                          # the one host read (the reference's int(z_lengths))
        invalid = (z_host < 0).nonzero().flatten().tolist()
        if invalid:
            raise ValueError(f"item {invalid[0]}: the predicted durations are not finite or sum past 2^24 frames "
                             f"(length_scale {length_scale}; invalid items: {invalid})")
        t_out = int(z_host.max())
        if noise is not None and noise.shape[2] != t_out:
            raise ValueError(f"noise must be [B={b}, n_mels={n_mels}, T_out={t_out}], got shape {tuple(noise.shape)}")
        y_lengths = z_host.long().to(dev)
        if t_out == 0:
            return torch.zeros(b, n_mels, 0, device=dev), y_lengths
        idx = glow.duration_index(cum, lens32, z_lens, t_out)
        z_m = glow.align_gather(x_m, idx)
        z_logs = None if x_logs is None else glow.align_gather(x_logs, idx)
        eps = (torch.randn(b, n_mels, t_out, device=dev) if noise is None else noise.to(dev, torch.float32)).transpose(1, 2)
        z = self._prior_sample(z_m, z_logs, eps, z_lens, t_out, noise_scale)
        yh_rows, _ = self.decoder(z, z_lens, speaker_embeddings=g, reverse=True)
        return yh_rows.transpose(1, 2), y_lengths

    @torch.no_grad()
    def infer_step(self, t, speaker=None):
        """One utterance -> yh [1, n_mels, T] (glow_tts.py:133-168): its token ids (a list or a 1-D tensor), or, on a model
        configured with ``dataset.text_frontend``, the sentence itself -- stripped, closed with a period, parsed and
        interspersed with blanks as the dataset does for training (the reference's infer_step omits the blanks although it
        trains with them: repaired).  ValueError for a text that leaves no symbol."""
        if isinstance(t, str):
            t = sentence_to_ids(self, t)
        x = torch.as_tensor(t)
        if x.dim() != 1:
            raise ValueError(f"infer_step takes one utterance's token ids (1-D), got shape {tuple(x.shape)}")
        yh, _ = self.infer(x.unsqueeze(0), speaker=speaker)
        return yh
