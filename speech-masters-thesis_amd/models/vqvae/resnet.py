"""Residual blocks of the VQ-VAE encoder / decoder: the gated multi-receptive-field block and the WaveNet stack.

They mirror the parameter trees of the reference ``GatedHiFiBlock`` (models/vqvae/
resnet.py:184-241; per branch ``Sequential(Conv1d 1x1, ResLayer)``, resnet.py:16-36) and
``WaveNetBlock`` (resnet.py:123-181) so checkpoints interchange, but activations are
channels-last and the arithmetic goes through ``smt_amd.convops``.  ``block_type: gated_hifi``
and ``wavenet`` are implemented natively; ``base`` and ``hifi`` are not (models/vqvae/conv.py).
"""
import math

import torch
import torch.nn as nn

from smt_amd import convops, packing


class ConvParams(nn.Module):
    """weight / bias of one (transposed) 1-D convolution in torch's layouts and default init."""

    def __init__(self, c_in, c_out, kernel, transposed=False, zero=False):
        super().__init__()
        shape = (c_in, c_out, kernel) if transposed else (c_out, c_in, kernel)
        self.weight = nn.Parameter(torch.empty(shape))
        self.bias = nn.Parameter(torch.empty(c_out))
        self.c_in, self.c_out, self.kernel, self.transposed = c_in, c_out, kernel, transposed
        self.reset_parameters(zero)

    @torch.no_grad()
    def reset_parameters(self, zero=False):
        if zero:
            self.weight.zero_()
            self.bias.zero_()
            return
        bound = 1.0 / math.sqrt(self.weight.shape[1] * self.weight.shape[2])  # torch's fan_in rule
        self.weight.uniform_(-bound, bound)
        self.bias.uniform_(-bound, bound)


def _numbered(**children):
    holder = nn.Module()
    for name, child in children.items():
        holder.add_module(name.lstrip("_"), child)
    return holder


def mod_cycle(depth, cycle):
    return depth if cycle is None else depth % cycle


class WaveNetBlock(nn.Module):
    """Stack of WaveNet residual layers (reference ``WaveNetBlock``, models/vqvae/resnet.py:123-181), with its parameter tree:
    ``conv_in`` (1x1, n_in -> H), per layer ``convs.d`` (k = 3, dilated, H -> 2H) and ``gates.d`` (1x1, H -> H), ``conv_out``
    (1x1, H -> n_in), H = int(m_conv * n_in).  No ReLU and no dropout: the block uses no dropout site, ``drop_seed`` is
    accepted for the common block interface; ``reverse_dilation``, ``kernel_size_*`` and ``dropout`` are ignored as the
    reference's ``**kwargs`` ignores them."""

    def __init__(self, n_in, n_depth, m_conv=1.0, dilation_growth_rate=1, dilation_cycle=None, zero_out=True,
                 res_scale=False, site_base=0, **unused):
        super().__init__()
        self.n_in, self.n_depth, self.n_hid = n_in, n_depth, int(m_conv * n_in)
        self.res_scale = 1.0 if not res_scale else 1.0 / math.sqrt(n_depth)
        self.dilations = [dilation_growth_rate ** mod_cycle(d, dilation_cycle) for d in range(n_depth)]
        h = self.n_hid
        self.conv_in = ConvParams(n_in, h, 1)
        self.conv_out = ConvParams(h, n_in, 1)
        self.convs = nn.ModuleList([ConvParams(h, 2 * h, 3) for _ in range(n_depth)])
        self.gates = nn.ModuleList([ConvParams(h, h, 1, zero=zero_out) for _ in range(n_depth)])

    @packing.forward_scope
    def forward(self, x, lens, drop_seed=0):
        """x [B, T, n_in]; lens [B] valid lengths (the block's row mask)."""
        if self.res_scale != 1.0:
            raise NotImplementedError("res_scale=True is not used by the reference configs (conv.py:55)")
        x = convops.conv1d(x, self.conv_in.weight, self.conv_in.bias, lens=lens)
        for dil, conv, gate in zip(self.dilations, self.convs, self.gates):
            z = convops.conv1d(x, conv.weight, conv.bias, padding=dil, dilation=dil, lens=lens)
            x = convops.wavenet_tail(z, x, gate.weight, gate.bias, lens)
        return convops.conv1d(x, self.conv_out.weight, self.conv_out.bias, lens=lens)


class GatedHiFiBlock(nn.Module):
    def __init__(self, n_in, n_depth, dilation_growth_rate=1, dilation_cycle=None, kernel_size_growth_rate=2,
                 kernel_size_cycle=None, zero_out=True, res_scale=False, dropout=0.1, site_base=0, **unused):
        super().__init__()
        self.n_in, self.n_depth, self.dropout = n_in, n_depth, dropout
        self.res_scale = 1.0 if not res_scale else 1.0 / math.sqrt(n_depth)
        self.site_base = site_base
        self.geometry = []
        branches = []
        for d in range(n_depth):
            dil = dilation_growth_rate ** mod_cycle(d, dilation_cycle)
            k = 3 + kernel_size_growth_rate * mod_cycle(d, kernel_size_cycle)
            self.geometry.append((k, dil, ((k - 1) * dil) // 2))
            res = _numbered(model=_numbered(_2=ConvParams(2 * n_in, 2 * n_in, k),
                                            _5=ConvParams(2 * n_in, 2 * n_in, 1, zero=zero_out)))
            branches.append(_numbered(_0=ConvParams(n_in, 2 * n_in, 1), _1=res))
        self.blocks = nn.ModuleList(branches)
        self.gate = ConvParams(n_in, n_in, 1, zero=zero_out)

    @packing.forward_scope
    def forward(self, x, lens, drop_seed=0):
        """x [B, T, n_in]; lens [B] valid lengths (the block's row mask)."""
        if self.res_scale != 1.0:
            raise NotImplementedError("res_scale=True is not used by the reference configs (conv.py:55)")
        params = []
        for branch in self.blocks:
            expand, res = getattr(branch, "0"), getattr(branch, "1").model
            conv_k, conv_1 = getattr(res, "2"), getattr(res, "5")
            params += [expand.weight, expand.bias, conv_k.weight, conv_k.bias, conv_1.weight, conv_1.bias]
        params += [self.gate.weight, self.gate.bias]
        return convops.gated_hifi_block(x, lens, self.geometry, params, p_drop=self.dropout, training=self.training,
                                        seed=drop_seed, site_base=self.site_base)
