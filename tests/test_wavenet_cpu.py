"""The WaveNet block without a GPU: the three entry points are declared, bound and exported under the unchanged ABI number;
their argument errors are decided on the host; the float64 restatement (tests/wavenet_helpers.py) reproduces the fixture
captured from the reference's own class; the error bounds catch the mistakes a kernel could make; the module carries the
reference's parameter tree and both waveform models construct with ``block_type: wavenet``."""
import json
import os
import re

import numpy as np
import pytest
import torch

import wavenet_helpers as W
from conftest import GOLDEN, PKG, REPO

NAMES = ("smt_wavenet_gate_fwd", "smt_wavenet_gate_bwd", "smt_wavenet_tail_fwd")
T = torch.from_numpy
F32, BF16 = 0, 1


def test_entry_points_are_declared_bound_and_exported():
    from smt_amd import native
    text = open(os.path.join(REPO, "include", "smt_hip.h")).read()
    assert "WaveNet block ---- */" in text
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(smt_\w+)\s*\(", header))
    abi = int(re.search(r"smt_abi_version\(void\)\s*\{\s*return\s+(\d+)", open(os.path.join(PKG, "csrc", "common.hip")).read()).group(1))
    lib = native.lib()
    assert abi == native.ABI_VERSION == lib.smt_abi_version() == 10
    for name, n_args in zip(NAMES, (12, 15, 16)):
        assert name in declared and name in native.exported_symbols() and hasattr(lib, name)
        res, args = native._SIGNATURES[name]
        assert res is native.c_int and len(args) == n_args and args[-1] is native.c_ptr
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert all(name in integration for name in NAMES)


def _calls():
    """The three entries with good arguments (pointers that are never dereferenced: every call returns before a launch)."""
    from smt_amd import native
    lib = native.lib()
    P = native.c_ptr

    def gate_fwd(z=0x10000, a=0x80000, bs_z=128 * 40, ld_z=128, bs_a=64 * 40, ld_a=64, batch=2, t=40, hidden=64, dtype=BF16, **_):
        return lib.smt_wavenet_gate_fwd(P(z), bs_z, ld_z, P(a), bs_a, ld_a, None, batch, t, hidden, dtype, None)

    def gate_bwd(z=0x10000, a=0x80000, dz=0x100000, bs_z=128 * 40, ld_z=128, bs_a=64 * 40, ld_a=64, batch=2, t=40, hidden=64,
                 dtype=BF16, **_):
        return lib.smt_wavenet_gate_bwd(P(z), bs_z, ld_z, P(a), bs_a, ld_a, P(dz), bs_z, ld_z, None, batch, t, hidden, dtype, None)

    def tail(z=0x10000, a=0x80000, dz=0x100000, w=0x200000, bs_z=128 * 40, ld_z=128, bs_a=64 * 40, ld_a=64, batch=2, t=40,
             hidden=64, dtype=BF16, **_):
        return lib.smt_wavenet_tail_fwd(P(z), bs_z, ld_z, P(a), bs_a, ld_a, P(w), None, P(dz), bs_a, ld_a, None, batch, t, hidden, None)

    return lib, dict(zip(NAMES, (gate_fwd, gate_bwd, tail)))


COMMON_ERRORS = (
    (dict(z=0), b"null pointer (z)"), (dict(a=0), b"null pointer"), (dict(z=0x10004), b"z must be 16-byte aligned"),
    (dict(a=0x80008), b"must be 16-byte aligned"), (dict(ld_z=120), b"pitch ld_z=120 is smaller than the row width 128"),
    (dict(ld_a=56), b"is smaller than the row width 64"), (dict(ld_z=132), b"ld_z=132 must be a multiple of 8 elements"),
    (dict(ld_a=68), b"=68 must be a multiple of 8 elements"), (dict(bs_z=128 * 40 + 4), b"batch stride bs_z"),
    (dict(batch=2 ** 16, t=2 ** 15), b"batch * t = 2147483648 rows must be at most 2^31 - 1"),
    (dict(batch=-1), b"must not be negative"), (dict(t=-5), b"must not be negative"),
)


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_need_no_launch(name):
    lib, calls = _calls()
    call = calls[name]
    errors = list(COMMON_ERRORS)               # the good arguments are only the base of the bad ones: they are never passed whole
    if name == "smt_wavenet_gate_fwd":
        errors += [(dict(a=0x10000 + 2 * 64), b"a must not alias z"), (dict(a=0x10000 - 64), b"a must not alias z")]
    if name == "smt_wavenet_tail_fwd":
        errors += [(dict(hidden=32), b"hidden=32 must be 64 or 128"), (dict(hidden=256), b"hidden=256 must be 64 or 128"),
                   (dict(w=0), b"null pointer (w_packed)"), (dict(w=0x200002), b"w_packed must be 16-byte aligned"),
                   (dict(dz=0), b"null pointer (y)"), (dict(dz=0x10000 + 64), b"y must not alias z"),
                   (dict(dz=0x80000), b"y must not alias x")]
    else:
        errors += [(dict(hidden=12), b"hidden=12 must be a positive multiple of 8"), (dict(hidden=0), b"hidden=0 must be"),
                   (dict(dtype=2), b"dtype=2 must be SMT_F32 (0) or SMT_BF16 (1)"), (dict(dtype=-1), b"dtype=-1")]
    if name == "smt_wavenet_gate_bwd":
        errors += [(dict(dz=0), b"null pointer (dz)"), (dict(dz=0x10000), b"dz must not alias z"),
                   (dict(dz=0x80000 + 16), b"dz must not alias da")]
    for kwargs, words in errors:
        assert call(**kwargs) == 1, kwargs     # 1 = argument error (2 would be a failed launch)
        err = lib.smt_last_error()
        assert name.encode() in err and words in err, (kwargs, err)
    # no rows: nothing is launched and the pointers may be NULL
    assert call(batch=0, z=0, a=0, dz=0) == 0 and call(t=0, z=0, a=0, dz=0) == 0


# ---- the restatement against the reference's own class -------------------------------------------------------------------
def _fixture(golden):
    g = golden("wavenet_block")
    params = {k[2:]: T(v).double() for k, v in g.items() if k.startswith("p.")}
    x = T(g["x"]).double().transpose(1, 2).contiguous()                    # the fixture is [B, C, T]
    return g, params, x, T(g["lens"])


def test_fixture_holds_what_the_reference_computed(golden):
    g, params, x, lens = _fixture(golden)
    assert x.shape == (2, 40, 16) and lens.tolist() == [40, 23] and g["y"].dtype == np.float64 and g["g.x"].dtype == np.float64
    assert set(params) == {f"{m}.{p}" for m in ("conv_in", "conv_out", "convs.0", "convs.1", "convs.2", "gates.0", "gates.1", "gates.2")
                           for p in ("weight", "bias")}
    assert all(params[f"gates.{d}.weight"].abs().sum() > 0 and params[f"gates.{d}.bias"].abs().sum() > 0 for d in range(3))
    assert all(("g." + k) in g and g["g." + k].shape == tuple(v.shape) for k, v in params.items())
    assert os.path.getsize(os.path.join(GOLDEN, "wavenet_block.npz")) < 300_000


def test_restatement_reproduces_the_reference_block(golden):
    g, params, x, lens = _fixture(golden)
    for p in params.values():
        p.requires_grad_(True)
    x.requires_grad_(True)
    m = W.row_mask(lens, 40)
    y = W.block64(x, lens, params, W.block_dilations(3, 3, 2))
    r = T(g["r"]).double().transpose(1, 2)
    (y * r * m).sum().backward()
    y_ref = T(g["y"]).transpose(1, 2)
    assert ((y - y_ref) * m).abs().max().item() <= 1e-12
    assert ((x.grad - T(g["g.x"]).transpose(1, 2)) * m).abs().max().item() <= 1e-12
    for k, p in params.items():
        assert (p.grad - T(g["g." + k])).abs().max().item() <= 1e-12, k


def _fixture_layers(golden):
    """(z, x, W_g, bias) of every layer of the fixture block on its valid rows, from the restatement."""
    g, params, x, lens = _fixture(golden)
    m = W.row_mask(lens, 40)
    valid = m[..., 0].bool()
    x = W.conv64(x * m, params["conv_in.weight"], params["conv_in.bias"])
    out = []
    for d, dil in enumerate(W.block_dilations(3, 3, 2)):
        z = W.conv64(x * m, params[f"convs.{d}.weight"], params[f"convs.{d}.bias"], dil, dil)
        out.append((z[valid], x[valid], params[f"gates.{d}.weight"], params[f"gates.{d}.bias"]))
        x = x + W.conv64(W.gate64(z) * m, params[f"gates.{d}.weight"], params[f"gates.{d}.bias"])
    return out


def test_bounds_have_teeth_on_the_fixtures_own_z(golden):
    """A kernel with one of these mistakes exceeds its bound on at least 90 % of the elements."""
    layers = _fixture_layers(golden)
    z = torch.cat([l[0] for l in layers])
    h = z.shape[-1] // 2
    assert z.abs().max() < W.GATE_DOMAIN
    a = W.gate64(z)
    swapped = W.gate64(torch.cat([z[:, h:], z[:, :h]], dim=-1))
    tanh_for_sigmoid = torch.tanh(z[:, :h]) * torch.tanh(z[:, h:])
    for name, wrong in (("swapped halves", swapped), ("tanh for sigmoid", tanh_for_sigmoid)):
        for bound in (torch.full_like(a, W.E_F), W.BF16_GATE_REL * a.abs()):
            frac = ((wrong - a).abs() > bound).double().mean().item()
            assert frac >= 0.9, (name, frac)
    da = torch.ones_like(a)
    dz, dz_sw = W.gate_grad64(z, da), W.gate_grad64(torch.cat([z[:, h:], z[:, :h]], dim=-1), da)
    assert ((torch.cat([dz_sw[:, h:], dz_sw[:, :h]], dim=-1) - dz).abs() > W.E_B).double().mean().item() >= 0.9
    fr = {"swapped halves": [], "tanh for sigmoid": [], "dropped residual": [], "dropped bias": []}
    for z, x, w, b in layers:
        y, s = W.tail64(z, x, w, b)
        bound = W.tail_bound(y, s, h)
        w2 = w.reshape(h, h)
        wrong = {"swapped halves": x + b + W.gate64(torch.cat([z[:, h:], z[:, :h]], dim=-1)) @ w2.t(),
                 "tanh for sigmoid": x + b + (torch.tanh(z[:, :h]) * torch.tanh(z[:, h:])) @ w2.t(),
                 "dropped residual": y - x, "dropped bias": y - b}
        for name, v in wrong.items():
            fr[name].append(((v - y).abs() > bound).double().mean().item())
    for name, v in fr.items():
        print(name, ["%.3f" % f for f in v])
        assert min(v) >= 0.9, (name, v)


# ---- module and models ------------------------------------------------------------------------------------------------
def test_block_carries_the_references_parameter_tree(golden):
    from models.vqvae.conv import get_block
    from models.vqvae.resnet import WaveNetBlock
    g, params, _, _ = _fixture(golden)
    assert get_block("wavenet") is WaveNetBlock
    torch.manual_seed(0)
    blk = WaveNetBlock(16, 3, m_conv=2.0, dilation_growth_rate=3, dilation_cycle=2, zero_out=True, reverse_dilation=True,
                       kernel_size_growth_rate=2, kernel_size_cycle=None, dropout=0.1)
    sd = blk.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in params.items()}
    assert blk.dilations == [1, 3, 1] and blk.n_hid == 32
    assert all(sd[f"gates.{d}.{p}"].abs().sum() == 0 for d in range(3) for p in ("weight", "bias"))
    assert sd["convs.0.weight"].abs().sum() > 0 and sd["conv_out.weight"].abs().sum() > 0
    assert WaveNetBlock(16, 2, zero_out=False).gates[0].weight.abs().sum() > 0
    blk.load_state_dict({k: v.float() for k, v in params.items()})
    for bad in ("base", "hifi"):
        with pytest.raises(ValueError, match="'base' and 'hifi'"):
            get_block(bad)
    with pytest.raises(NotImplementedError, match="res_scale"):
        WaveNetBlock(16, 2, res_scale=True)(torch.zeros(1, 8, 16), torch.tensor([8]))


def _yaml(name):
    from utils import config as C
    return C.load(os.path.join(PKG, "configs", "models", name))


def test_models_construct_with_the_wavenet_block():
    from models.vqtts import VQTTS
    from models.vqvae.resnet import WaveNetBlock
    from models.vqvae.vqvae import VQVAE
    from utils import config as C
    with open(os.path.join(GOLDEN, "vqvae_wavenet_keys.json")) as f:
        keys = json.load(f)
    cfg = _yaml("vqvae_wavenet.yaml")
    base = _yaml("vqvae.yaml")
    assert cfg.model.block_type == "wavenet"
    cfg.model.block_type = "gated_hifi"
    assert cfg == base                                   # vqvae.yaml with the one key changed
    cfg.model.block_type = "wavenet"
    model = VQVAE(cfg)
    mine = {k: list(v.shape) for k, v in model.state_dict().items() if k.startswith(("encoders.", "decoders."))}
    assert mine == keys
    n_sites = [m.n_sites for m in model.modules() if hasattr(m, "n_sites")]
    ref_sites = [m.n_sites for m in VQVAE(base).modules() if hasattr(m, "n_sites")]
    assert n_sites == ref_sites                          # the site numbering does not change; the block uses none
    # m_conv reaches the block
    cfg.model.m_conv = 2.0
    wide = VQVAE(cfg)
    assert {m.n_hid // m.n_in for m in wide.modules() if isinstance(m, WaveNetBlock)} == {2}
    # VQTTS at the same stack geometry has the same trees under its own names
    tts = C.merge(_yaml("vqtts.yaml"), C.load(os.path.join(PKG, "configs", "datasets", "synthetic_vqtts.yaml")))
    tts.model.block_type = "wavenet"
    for k in ("levels", "downs_t", "strides_t", "multipliers", "width", "depth", "m_conv", "emb_width", "dilation_growth_rate",
              "dilation_cycle"):
        tts.model[k] = base.model[k]
    model = VQTTS(tts)
    assert any(isinstance(m, WaveNetBlock) for m in model.modules())
    mapped = {k.replace("audio_encoder.", "encoders.0.").replace("audio_decoder.", "decoders.0."): list(v.shape)
              for k, v in model.state_dict().items() if k.startswith(("audio_encoder.", "audio_decoder."))}
    # (VQTTS keeps one stack where the full VQ-VAE inventory has one per level: every key it has is in the inventory)
    assert len(mapped) > 200 and all(keys.get(k) == v for k, v in mapped.items())
