"""The grouped bottleneck of VQTTS without a GPU: the fixture captured from the reference is internally consistent, the
module constructs with the reference's buffer names and loads the fixture's codebook, and the binding still mirrors
the header."""
import os
import re

import numpy as np
import torch

from conftest import REPO


def test_fixture_is_internally_consistent(golden):
    """Recomputing q_rel in float64 from the stored inputs and the codebook in force at each step reproduces it on every
    row (masked rows search group 0), and y_d is that code times the mask."""
    g = golden("vqtts_bottleneck")
    n_vocab, l_bins = int(g["n_vocab"]), int(g["l_bins"])
    k = g["s0_k_rand_init"]
    for tag in ("s0", "s1", "s2", "e"):
        y, x_id, align = g[f"{tag}_y_enc"], g[f"{tag}_x_id"], g[f"{tag}_align_idx"]
        b, t, d = y.shape
        assert k.shape == (n_vocab * l_bins, d)
        assert np.array_equal(g[f"{tag}_attn"].argmax(1).astype(np.int32)[align >= 0], align[align >= 0])
        assert np.array_equal(g[f"{tag}_attn"].sum(1) > 0, align >= 0)
        mask = (align >= 0).reshape(-1)
        group = np.where(mask, x_id[np.arange(b)[:, None], np.maximum(align, 0)].reshape(-1), 0)
        kk = k.astype(np.float64).reshape(n_vocab, l_bins, d)[group]            # [N, L, D]: fine at fixture size
        dist = ((y.reshape(-1, 1, d).astype(np.float64) - kk) ** 2).sum(-1)
        q_rel = dist.argmin(1)
        assert np.array_equal(q_rel, g[f"{tag}_q_rel"].reshape(-1)), tag
        y_d = k[group * l_bins + q_rel] * mask[:, None]
        assert np.allclose(g[f"{tag}_y_d"].reshape(-1, d), y_d, atol=1e-6 * max(1.0, np.abs(y_d).max())), tag
        commit = (dist.min(1)[mask]).sum() / (mask.sum() * d)
        assert np.isclose(float(g[f"{tag}_commit"]), commit, rtol=1e-5), tag
        assert np.isclose(float(g[f"{tag}_m_fit"]), dist.min(1).sum() / l_bins, rtol=2e-5), tag
        if tag != "e":
            k = g[f"{tag}_k"]


def test_module_constructs_on_cpu_and_loads_reference_state(golden):
    from models.vqtts.bottleneck import Bottleneck
    from models.vqvae.bottleneck import BottleneckBlock
    g = golden("vqtts_bottleneck")
    n_vocab, l_bins = int(g["n_vocab"]), int(g["l_bins"])
    d = g["s2_k"].shape[1]
    m = Bottleneck(n_vocab, l_bins, d, float(g["mu"]), float(g["threshold"]))
    assert isinstance(m, BottleneckBlock) and m.k_bins == n_vocab * l_bins and (m.n_vocab, m.l_bins) == (n_vocab, l_bins)
    assert list(m.state_dict()) == ["k"] and m.k.shape == (n_vocab * l_bins, d)     # the reference's buffer name
    m.load_state_dict({"k": torch.from_numpy(g["s2_k"])})                           # a reference state dict loads as is
    assert np.array_equal(m.k.numpy(), g["s2_k"])
    q_abs = torch.from_numpy(g["e_q_rel"]) + l_bins * (n_vocab - 1)                  # codes of the last group
    assert m.decode(q_abs).shape == (*q_abs.shape, d)
    m.restore_k()
    assert m.init and m.k_elem.shape == (n_vocab * l_bins,)


def test_grouped_entry_points_are_declared_and_bound():
    from smt_amd import native
    header = open(os.path.join(REPO, "include", "smt_hip.h")).read()
    declared = set(re.findall(r"\b(smt_\w+)\s*\(", header))
    new = {"smt_vq_grouped_prep_bytes", "smt_vq_grouped_prepare", "smt_vq_align_groups",
           "smt_vq_grouped_forward_workspace_bytes", "smt_vq_grouped_forward", "smt_vq_grouped_ema_apply"}
    assert new <= declared and new <= set(native.exported_symbols())
    abi = int(re.search(r"smt_abi_version\(void\)\s*\{\s*return\s+(\d+)", open(os.path.join(
        REPO, "speech-masters-thesis_amd", "csrc", "common.hip")).read()).group(1))
    assert abi == native.ABI_VERSION
