"""Rotary positions without a GPU: the host-side table, the float64 helper's own properties (orthogonal, relative), the proof
that the kernel tests' assertion can fail (each mutation of tests/lm_rope_helpers.py, on the kernel tests' own inputs), the new
symbols and the configuration keys."""
import math
import os

import numpy as np
import pytest
import torch

import lm_rope_helpers as R
from oracle import lm_oracle as lmo


@pytest.mark.parametrize("dh,base,rows", [(32, 10000.0, 70), (64, 10000.0, 70), (32, 500.0, 41), (64, 123.5, 41)])
def test_rope_table_is_the_float64_formula_rounded_once(dh, base, rows):
    from smt_amd import lm as K
    table = K.rope_table(rows, dh, base)
    assert table.shape == (rows, dh // 2, 2) and table.dtype == torch.float32 and table.is_contiguous()
    theta = np.power(np.float64(base), -2.0 * np.arange(dh // 2, dtype=np.float64) / dh)
    a = np.arange(rows, dtype=np.float64)[:, None] * theta[None, :]
    want = np.stack([np.cos(a), np.sin(a)], axis=-1).astype(np.float32)
    assert np.array_equal(table.numpy(), want)
    assert torch.equal(table, R.table64(rows, dh, base).float())
    assert np.array_equal(table[0].numpy(), np.stack([np.ones(dh // 2), np.zeros(dh // 2)], -1).astype(np.float32))    # position 0: identity


def test_rope_table_refuses_other_head_dims_and_bases():
    from smt_amd import lm as K
    with pytest.raises(AssertionError, match="head dim 32 or 64"):
        K.rope_table(4, 48)
    for base in (1.0, 0.5, -3.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="base"):
            K.rope_table(4, 32, base)


@pytest.mark.parametrize("L,dh,pos0", R.KERNEL_CASES)
def test_helper_is_orthogonal(L, dh, pos0):
    """inverse(forward(x)) = x to 1e-12, norms of every pair kept, v untouched."""
    x, positions = R.kernel_case(L, dh, pos0)
    y = R.rope64(x, R.KERNEL_H, positions)
    back = R.rope64(y, R.KERNEL_H, positions, inverse=True)
    assert float((back - x.double()).abs().max()) <= 1e-12
    n_in = x.double().reshape(*x.shape[:-1], -1, 2).norm(dim=-1)
    n_out = y.reshape(*x.shape[:-1], -1, 2).norm(dim=-1)
    assert float((n_in - n_out).abs().max()) <= 1e-12
    assert torch.equal(y[..., 2 * x.shape[-1] // 3:], x.double()[..., 2 * x.shape[-1] // 3:])


@pytest.mark.parametrize("dh", [32, 64])
def test_helper_is_relative(dh):
    """Scores rope(q, p + s) . rope(k, r + s) do not depend on the shift s."""
    h, l = 2, 9
    g = torch.Generator().manual_seed(dh)
    x = torch.randn(1, l, 3 * h * dh, generator=g, dtype=torch.float64)

    def scores(shift):
        y = R.rope64(x, h, torch.arange(l) + shift).reshape(l, 3, h, dh)
        return torch.einsum("phc,rhc->hpr", y[:, 0], y[:, 1])

    base = scores(0)
    for shift in (1, 37, 4000):
        assert float((scores(shift) - base).abs().max()) <= 1e-9, shift
    assert float((scores(0) - torch.einsum("phc,rhc->hpr", *x.reshape(l, 3, h, dh).unbind(1)[:2])).abs().max()) > 1e-2     # and it does rotate


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_the_kernel_assertion_fails_under_each_mutation(mutate):
    """`assert_rope`, the GPU tests' assertion, on the helper's own output rounded to fp32: passes unmutated, fails for every
    mutation on every kernel case -- except the one row at position 0 (L = 1, pos0 = 0), where the rotation is the identity and
    only the off-by-one position can show."""
    for L, dh, pos0 in R.KERNEL_CASES:
        x, positions = R.kernel_case(L, dh, pos0)
        for inverse in (False, True):
            good = R.rope64(x, R.KERNEL_H, positions, inverse=inverse).float()
            assert R.assert_rope(good, x, R.KERNEL_H, positions, inverse=inverse) <= 0.5       # rounding the exact value: u (|y|) at most
            bad = R.rope64(x, R.KERNEL_H, positions, inverse=inverse, mutate=mutate).float()
            if (L, pos0) == (1, 0) and mutate != "pos_off_by_one":
                continue
            with pytest.raises(AssertionError):
                R.assert_rope(bad, x, R.KERNEL_H, positions, inverse=inverse)


def test_model_helper_without_rotation_is_the_sinusoidal_helper_without_its_table():
    """The float64 rotary model differs from lm_prenorm_helpers.lm_logits in two places only -- no table on the embedding, the
    rotation after the in-projection: with every row at position 0 the rotation is the identity, and on a one-token sequence the
    two agree once the sinusoidal row 0 (0, 1, 0, 1, ...) is taken off the embedding."""
    import lm_prenorm_helpers as H
    p = {k: v.double() for k, v in lmo.init_params(16, 64, 2, 128, 2, seed=3).items()}
    x = torch.tensor([[lmo.BOS], [5]])
    lens = torch.tensor([1, 1])
    for norm_first, activation in H.COMBOS:
        got = R.lm_logits(x, lens, p, 2, 2, norm_first, activation)
        shifted = dict(p)
        shifted["embedding.weight"] = p["embedding.weight"] - lmo.positional_table(1, 64).double() / math.sqrt(64)
        want = H.lm_logits(x, lens, shifted, 2, 2, norm_first, activation)
        assert float((got - want).abs().max()) <= 1e-12, (norm_first, activation)


def test_new_symbols_are_exported_and_the_abi_is_10():
    from smt_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = native.lib()
    for name in ("smt_lm_rope", "smt_lm_decode_attention_rope"):
        assert name in native.exported_symbols() and hasattr(lib, name), name
    assert native.ABI_VERSION == 10 and lib.smt_abi_version() == 10


def test_shipped_config_is_the_shipped_model_plus_the_position_key():
    from utils import config as C
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-masters-thesis_amd")
    rope = C.load(os.path.join(pkg, "configs/models/transformer_lm_rope.yaml"))
    plain = C.load(os.path.join(pkg, "configs/models/transformer_lm.yaml"))
    assert rope.model.position == "rotary" and float(rope.model.rope_base) == 10000.0
    assert "position" not in plain.model and "rope_base" not in plain.model
    for section in ("optimizer", "scheduler"):
        assert rope[section] == plain[section]
    for key in plain.model:
        assert rope.model[key] == plain.model[key], key
    assert set(rope.model) - set(plain.model) == {"position", "rope_base"}
