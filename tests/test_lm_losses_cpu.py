"""The TransformerLM's focal and MMI losses without a GPU: the C ABI (symbols, every argument error -- all of them are
returned before any HIP call), the float64 reference of tests/lm_loss_helpers.py against the closed forms the kernels
implement (include/smt_hip.h), and the model's configuration surface."""
import math
import os

import pytest
import torch

import lm_loss_helpers as H

NEW_SYMBOLS = ["smt_lm_focal_fwd", "smt_lm_focal_bwd", "smt_lm_mmi_workspace_bytes", "smt_lm_mmi_fwd", "smt_lm_mmi_bwd"]
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-masters-thesis_amd")


@pytest.fixture(scope="module")
def lib():
    from smt_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return native.lib()


def _err(lib):
    return lib.smt_last_error().decode()


def test_new_symbols_are_exported_and_bound_under_abi_10(lib):
    from smt_amd import native
    assert native.ABI_VERSION == 10 and lib.smt_abi_version() == 10
    for name in NEW_SYMBOLS:
        assert name in native.exported_symbols() and hasattr(lib, name)
    with open(os.path.join(os.path.dirname(PKG), "include", "smt_hip.h")) as f:
        header = f.read()
    assert all(name + "(" in header for name in NEW_SYMBOLS)
    assert header.index("smt_lm_ce_bwd(") < header.index("smt_lm_focal_fwd(") < header.index("smt_lm_decode_embed(")


# Every call below passes NULL for every pointer: whichever check fires, nothing can be launched.
def _focal_fwd(lib, rows, vocab, gamma):
    return lib.smt_lm_focal_fwd(None, None, None, None, None, rows, vocab, gamma, None)


def _focal_bwd(lib, rows, vocab):
    return lib.smt_lm_focal_bwd(None, None, None, None, None, None, rows, vocab, None)


def _mmi_fwd(lib, rows, vocab, ws_bytes):
    return lib.smt_lm_mmi_fwd(None, None, None, None, None, None, None, rows, vocab, None, ws_bytes, None)


def _mmi_bwd(lib, rows, vocab):
    return lib.smt_lm_mmi_bwd(None, None, None, None, None, None, rows, vocab, None)


def test_null_pointers_are_argument_errors(lib):
    big = lib.smt_lm_mmi_workspace_bytes(4, 16)
    assert _focal_fwd(lib, 4, 16, 2.0) == 1 and _err(lib) == "smt_lm_focal_fwd: null pointer"
    assert _focal_bwd(lib, 4, 16) == 1 and _err(lib) == "smt_lm_focal_bwd: null pointer"
    assert _mmi_fwd(lib, 4, 16, big) == 1 and _err(lib) == "smt_lm_mmi_fwd: null pointer"
    assert _mmi_bwd(lib, 4, 16) == 1 and _err(lib) == "smt_lm_mmi_bwd: null pointer"


def test_row_and_vocab_limits_are_named(lib):
    calls = {"smt_lm_focal_fwd": lambda r, v: _focal_fwd(lib, r, v, 2.0), "smt_lm_focal_bwd": lambda r, v: _focal_bwd(lib, r, v),
             "smt_lm_mmi_fwd": lambda r, v: _mmi_fwd(lib, r, v, 1 << 30), "smt_lm_mmi_bwd": lambda r, v: _mmi_bwd(lib, r, v)}
    for name, call in calls.items():
        assert call(-1, 16) == 1 and _err(lib).startswith(name + ": rows must be in 0..2^33 - 4 (got -1)")
        assert call(2 ** 33, 16) == 1 and _err(lib).startswith(name + ": rows must be in 0..2^33 - 4")
        assert call(4, 0) == 1 and _err(lib) == name + ": vocab must be >= 1 (got 0)"
        assert call(4, -3) == 1 and _err(lib) == name + ": vocab must be >= 1 (got -3)"
        assert call(0, 16) == 0                                     # no rows: nothing to do, nothing is looked at


@pytest.mark.parametrize("gamma", [-1.0, -0.0001, 0.5, 0.999, 1e-30, math.inf, -math.inf, math.nan])
def test_gamma_outside_the_built_set_is_refused(lib, gamma):
    assert _focal_fwd(lib, 4, 16, gamma) == 1
    assert _err(lib).startswith("smt_lm_focal_fwd: gamma must be 0 or a finite value >= 1") and "not built" in _err(lib)
    assert _focal_fwd(lib, 0, 16, gamma) == 1                       # also with nothing to do


@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, 10.0])
def test_built_gammas_pass_the_gamma_check(lib, gamma):
    assert _focal_fwd(lib, 4, 16, gamma) == 1 and _err(lib) == "smt_lm_focal_fwd: null pointer"


def test_mmi_workspace_size_and_a_workspace_that_is_too_small(lib):
    size = lib.smt_lm_mmi_workspace_bytes
    assert size(0, 512) == 0 and size(-3, 512) == 0 and size(5, 0) == 0
    assert size(1, 1) == 8 and size(16, 64) == 2 * 64 * 4 and size(17, 64) == 3 * 64 * 4
    assert size(2064, 512) == (129 + 1) * 512 * 4
    need = size(1030, 64)
    assert _mmi_fwd(lib, 1030, 64, need - 1) == 1
    assert _err(lib) == f"smt_lm_mmi_fwd: workspace too small ({need - 1} bytes, needs {need})"
    assert _mmi_fwd(lib, 1030, 64, 0) == 1 and "workspace too small" in _err(lib)
    assert _mmi_fwd(lib, 1030, 64, need) == 1 and _err(lib) == "smt_lm_mmi_fwd: null pointer"


@pytest.mark.parametrize("rows,vocab", [(5, 16), (41, 512)])
def test_float64_helper_equals_the_closed_forms(rows, vocab):
    """Autograd through the torch classes in float64 == the formulas of include/smt_hip.h, loss and gradient."""
    for kind, gammas in (("focal", H.GAMMAS), ("mmi", [None])):
        for gamma in gammas:
            logits, target, loss64, _, count, grad64 = H.case_reference(kind, rows, vocab, gamma)
            loss_cf, grad_cf = H.closed_form(kind, logits, target, gamma)
            assert count == int((target >= 0).sum()) and count < rows
            assert abs(loss_cf - loss64) <= 1e-12 * max(1.0, abs(loss64)), (kind, gamma, loss_cf, loss64)
            assert float((grad_cf - grad64).abs().max()) <= 1e-13, (kind, gamma)
            assert H.rel_l2(grad_cf, grad64) <= 1e-10, (kind, gamma)
            assert float(grad64[target < 0].abs().max()) == 0.0


def test_focal_at_gamma_zero_is_the_cross_entropy_in_the_helper():
    logits, target, loss64, _, _, grad64 = H.case_reference("focal", 41, 512, 0.0)
    keep = target >= 0
    l64 = logits.double().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(l64[keep], target[keep])
    (ce * H.UPSTREAM).backward()
    assert abs(float(ce.detach()) - loss64) < 1e-12 and float((l64.grad - grad64).abs().max()) < 1e-14


def _config(**over):
    from utils import config as C
    cfg = C.load(os.path.join(PKG, "configs/models/transformer_lm.yaml"))
    cfg.model.update(C.create(dict(vocab_size=16, embed_dim=64, max_len=64, num_layers=1, d_model=64, nhead=2, dim_feedforward=128,
                                   dropout=0.0, **over)))
    return cfg


def test_model_reads_focal_gamma_and_refuses_an_unknown_loss_type(monkeypatch):
    from models.transformer_lm import transformer_lm as T
    from models.transformer_lm.losses import FocalLoss, MaximumMutualInformationLoss
    monkeypatch.setattr(T.TransformerLM, "load_vqvae", staticmethod(lambda log_dir, ckpt_num: torch.nn.ModuleDict()))
    assert "focal_gamma" not in _config().model                      # the YAML carries it as a commented default only
    model = T.TransformerLM(_config(loss_type="focal"))
    assert model.focal_gamma == 10.0 and isinstance(model.loss, FocalLoss) and model.loss.gamma == 10.0
    model = T.TransformerLM(_config(loss_type="focal", focal_gamma=2.0))
    assert model.focal_gamma == 2.0 and model.loss.gamma == 2.0
    model = T.TransformerLM(_config(loss_type="mmi"))
    assert isinstance(model.loss, MaximumMutualInformationLoss) and model.loss.num_classes == 16
    assert T.TransformerLM(_config(loss_type="ce")).loss is None
    with pytest.raises(ValueError, match="Loss function hinge not supported"):
        T.TransformerLM(_config(loss_type="hinge"))
