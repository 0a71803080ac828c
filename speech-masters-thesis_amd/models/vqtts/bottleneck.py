"""Text-conditioned grouped VQ bottleneck of VQTTS (reference models/vqtts/bottleneck.py).

The codebook holds ``n_vocab * l_bins`` codes; an audio frame searches only the ``l_bins`` codes of the text token it is
aligned to, and the EMA update runs over the whole table.  The reference gathers ``k[x_id]`` ([N, l_bins, D]) before a
bmm; here the rows are bucketed by token and the search, dequantisation, commit / fit terms, straight-through backward
and the codebook statistics / update all run in libsmt_hip.so (``smt_amd.vq``, the ``grouped_*`` calls).  Everything the
flat block does around those calls -- initialisation, dead-code revival rows, the single all-reduce under data
parallelism -- is inherited from it.
"""
import torch

from models.vqvae.bottleneck import BottleneckBlock
from smt_amd import vq


class Bottleneck(BottleneckBlock):
    def __init__(self, n_vocab: int, l_bins: int, emb_width: int, mu: float, threshold: float):
        super().__init__(k_bins=n_vocab * l_bins, emb_width=emb_width, mu=mu, threshold=threshold)
        self.n_vocab, self.l_bins = n_vocab, l_bins

    # -- the derived data is per group (each token's codes centred at their own mean) ------------------------------
    def _search_prep(self):
        key = (self.k.data_ptr(), self.k._version)
        if self._prep_key != key:
            self._prep = vq.grouped_prepare(self.k, self.n_vocab, self.l_bins, self._prep)
            self._prep_key = key
        return self._prep

    def _ema_apply(self, stats, revival):
        return vq.grouped_ema_apply(self.k, self.k_sum, self.k_elem, stats, revival, self.mu, self.threshold,
                                    self.n_vocab, self.l_bins, self._prep)

    def _groups(self, x_id, align):
        """(group int32 [B*T], row_mask f32 [B*T]) from token ids and the alignment: ``align`` is either the index form
        of glow.align_index ([B, T] int32, -1 = no token) or a dense 0/1 path [B, Tx, T]."""
        if align.dim() == 3:
            from smt_amd import glow
            align, _ = glow.align_index(align)
        return vq.align_groups(x_id.reshape(x_id.shape[0], -1).long(), align.to(torch.int32), self.n_vocab)

    @torch.no_grad()
    def encode(self, y_enc, x_id, align_idx):
        """y_enc [B, T, D] -> (q_rel [B, T], q_abs [B, T])."""
        b, t, d = y_enc.shape
        group, row_mask = self._groups(x_id, align_idx)
        q_rel, q_abs, _, _, _ = vq.grouped_forward_raw(y_enc.reshape(b * t, d).float().contiguous(), group, self.k, self.n_vocab,
                                                       self.l_bins, row_mask, want_xd=False, prep=self._search_prep())
        return q_rel.view(b, t), q_abs.view(b, t)

    def decode(self, q_abs):
        """q_abs [B, T] absolute codes -> [B, T, D]."""
        return torch.nn.functional.embedding(q_abs, self.k)

    def forward(self, y_enc, x_id, align_idx, k_rand=None, k_rand_init=None):
        """y_enc [B, T, D] channels-last, x_id [B, Tx] int64, align_idx [B, T] int32 (or a dense path [B, Tx, T]) ->
        (q_rel [B, T], y_d [B, T, D], commit_loss, metrics).  The codebook is updated in training mode only."""
        b, t, d = y_enc.shape
        rows = y_enc.reshape(b * t, d).float().contiguous()
        group, row_mask = self._groups(x_id, align_idx)
        if self.training and not self.init:
            self.init_k(rows.detach(), None, k_rand_init)       # from ALL rows, masked ones included (bottleneck.py:35-36)
        # update_k rewrites self.k in place afterwards; backward reads the quantised rows from y_d, not from k
        y_d, q_rel, q_abs, commit, fit = vq.vq_grouped_straight_through(rows, group, self.k, self.n_vocab, self.l_bins, row_mask,
                                                                        prep=self._search_prep())
        metrics = dict(fit=fit)
        if self.training:
            metrics.update(self.update_k(rows.detach(), q_abs, row_mask, k_rand))
        return q_rel.view(b, t), y_d.view(b, t, d), commit, metrics
