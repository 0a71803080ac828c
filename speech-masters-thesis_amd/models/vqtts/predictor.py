"""Code predictor of VQTTS: the text-encoder means, gathered onto the frames, go through a four-layer residual stack
(``quant_decoder``) and a projection to ``l_bins`` logits (``quant_proj``) that is trained with the cross-entropy against
the codes the quantiser chose; at synthesis its argmax picks the code, or a draw from its tempered distribution does.

Reference: models/vqtts/vqtts.py:77-87 (the two modules), 142-144 (forward), 157 and 190 (loss, accuracy), 175-178
(synthesis).  The parameter tree keeps the reference's keys (``quant_decoder.model.{i}.model.{2,5}``, ``quant_proj``), so
checkpoints interchange; activations are channels-last [B, T, C] fp32.  The projection and the loss run fused
(``smt_amd.vqtts.code_head``, include/smt_hip.h "VQTTS code head"): no [B, T, l_bins] tensor exists.

Deviation: the reference's ``F.cross_entropy`` averages over every frame, padded ones included; here frames at or past
``q_lens`` and frames without a token are not scored.  With full lengths the two agree.
"""
import torch
import torch.nn as nn

from smt_amd import convops, glow, packing, vqtts
from smt_amd.lm import Drop

from ..vqvae.resnet import ConvParams, _numbered


class CodePredictor(nn.Module):
    N_DEPTH, M_CONV, GROWTH = 4, 2, 3                              # vqtts.py:79-81; reverse_dilation: 27, 9, 3, 1

    def __init__(self, channels, l_bins, p_dropout=0.1):
        super().__init__()
        self.channels, self.l_bins, self.p_dropout = channels, l_bins, p_dropout
        self.dilations = [self.GROWTH ** d for d in range(self.N_DEPTH)][::-1]
        layers = [_numbered(model=_numbered(_2=ConvParams(channels, self.M_CONV * channels, 3),
                                            _5=ConvParams(self.M_CONV * channels, channels, 1, zero=True)))
                  for _ in self.dilations]
        self.quant_decoder = _numbered(model=nn.ModuleList(layers))
        self.quant_proj = ConvParams(channels, l_bins, 1)
        self._split = vqtts.WeightSplit()

    def stack(self, x, lens, drop_seed=0):
        """The residual stack (the reference's base ``ResNetBlock``, resnet.py:16-78, res_scale = 1): per layer
        x + conv1(relu(drop(conv3(relu(drop(x)))))), rows at or past ``lens`` read as zero by every conv."""
        for i, (layer, dil) in enumerate(zip(self.quant_decoder.model, self.dilations)):
            conv3, conv1 = getattr(layer.model, "2"), getattr(layer.model, "5")
            drops = [Drop(self.p_dropout, self.training, drop_seed, 2 * i + s) for s in (0, 1)]
            u = torch.relu(glow.dropout(x, drops[0]))
            u = convops.conv1d(u, conv3.weight, conv3.bias, padding=dil, dilation=dil, lens=lens)
            u = torch.relu(glow.dropout(u, drops[1]))
            x = convops.conv1d(u, conv1.weight, conv1.bias, lens=lens, residual=x)
        return x

    def hidden(self, x_enc, align_idx, q_lens, drop_seed=0):
        """x_enc [B, Tx, C] (detached), align_idx [B, Tq] int32 (-1 = no token), q_lens [B] -> the stack's output
        [B, Tq, C] with the rows at or past q_lens zeroed."""
        q_lens = q_lens.to(torch.int32)
        x = glow.align_gather(x_enc.detach().float(), align_idx.to(torch.int32))
        x = self.stack(x, q_lens, drop_seed)
        valid = torch.arange(x.shape[1], device=x.device)[None, :] < q_lens[:, None]
        return x * valid[..., None].to(x.dtype), valid

    @packing.forward_scope
    def forward(self, x_enc, align_idx, q_lens, target=None, drop_seed=0, sample=None):
        """With ``target`` (q_rel [B, Tq] of the bottleneck): (loss_ce, q_acc, pred); frames without a token or at or past
        q_lens are not scored.  Without: pred [B, Tq] int32, the argmax of the code head or, with
        ``sample = (temperature, min_p, seeds)`` (seeds [B] int32 on the device), one draw per frame
        (``smt_amd.vqtts.code_head_sample``)."""
        if sample is not None and target is not None:
            raise ValueError("CodePredictor.forward: sample= draws codes at synthesis; it cannot be combined with target=")
        h, valid = self.hidden(x_enc, align_idx, q_lens, drop_seed)
        if target is None:
            if sample is not None:
                temperature, min_p, seeds = sample
                pred = vqtts.code_head_sample(h, self.quant_proj.weight, self.quant_proj.bias, seeds, h.shape[1], temperature, min_p,
                                              split=self._split)
                return pred.view(h.shape[:-1])
            return vqtts.code_head_predict(h, self.quant_proj.weight, self.quant_proj.bias, split=self._split)
        scored = valid & (align_idx >= 0)
        target = torch.where(scored, target.to(torch.int64), torch.full_like(target, -1, dtype=torch.int64))
        loss, acc, _, pred = vqtts.code_head(h, self.quant_proj.weight, self.quant_proj.bias, target, split=self._split)
        return loss, acc, pred

    def synthesize_codes(self, pred, x_id, align_idx):
        """q_abs [B, Tq] int64 = token * l_bins + pred on the frames with a token (0 elsewhere), ready for
        ``Bottleneck.decode`` -- what the reference's commented-out line 172 computes."""
        has = align_idx >= 0
        token = torch.gather(x_id.to(torch.int64), 1, align_idx.clamp(min=0).to(torch.int64))
        return torch.where(has, token * self.l_bins + pred.to(torch.int64), torch.zeros_like(token))
