"""The VQTTS code head without a GPU: the entry points are declared, bound and exported with ABI 10 on both sides, the
kernel constants are mirrored, and the predictor constructs with the reference's parameter tree."""
import os
import re

from conftest import REPO

NEW = {"smt_vqtts_code_head_workspace_bytes", "smt_vqtts_code_head_prepare", "smt_vqtts_code_head_fwd",
       "smt_vqtts_code_head_bwd_workspace_bytes", "smt_vqtts_code_head_bwd"}
CSRC = os.path.join(REPO, "speech-masters-thesis_amd", "csrc")


def test_code_head_entry_points_are_declared_bound_and_exported():
    from smt_amd import native
    header = open(os.path.join(REPO, "include", "smt_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(smt_\w+)\s*\(", header))
    assert NEW <= declared and NEW <= set(native.exported_symbols())
    abi = int(re.search(r"smt_abi_version\(void\)\s*\{\s*return\s+(\d+)", open(os.path.join(CSRC, "common.hip")).read()).group(1))
    assert abi == native.ABI_VERSION == 10
    lib = native.lib()                                        # the built library exports them with the bound signatures
    assert lib.smt_abi_version() == 10
    for name in NEW:
        assert hasattr(lib, name)


def test_workspace_sizes():
    from smt_amd import native
    lib = native.lib()
    assert lib.smt_vqtts_code_head_workspace_bytes(128, 0) == 0
    assert lib.smt_vqtts_code_head_workspace_bytes(0, 512) == 0
    assert lib.smt_vqtts_code_head_workspace_bytes(128, 512) == 8 * 512 * 128      # hi and lo, both orientations, bf16
    assert lib.smt_vqtts_code_head_workspace_bytes(48, 96) == 8 * 96 * 64          # channels padded to 64
    assert lib.smt_vqtts_code_head_bwd_workspace_bytes(0, 128, 512) == 0
    from smt_amd import vqtts
    per_slice = 512 * (128 * 4 + 8)
    assert lib.smt_vqtts_code_head_bwd_workspace_bytes(3 * vqtts.CH_SLICE + 5, 128, 512) == 4 * per_slice
    # past CH_MAX_SLICES slices the slices grow instead: the logits are never bought back by slabs
    assert lib.smt_vqtts_code_head_bwd_workspace_bytes(2 ** 31 - 1, 128, 512) <= vqtts.CH_MAX_SLICES * per_slice


def test_kernel_constants_match_the_source():
    from smt_amd import vqtts
    src = open(os.path.join(CSRC, "vqtts_codes.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (CH_\w+) = (\d+);", src)}
    mirrored = dict(CH_ROWS=vqtts.CH_ROWS, CH_VT=vqtts.CH_VT, CH_VCOLS=vqtts.CH_VCOLS, CH_SLICE=vqtts.CH_SLICE,
                    CH_MAX_SLICES=vqtts.CH_MAX_SLICES, CH_SUM_PARTS=vqtts.CH_SUM_PARTS, CH_MAX_C=vqtts.CH_MAX_C, CH_MAX_V=vqtts.CH_MAX_V)
    assert {k: const[k] for k in mirrored} == mirrored
    assert (vqtts.CH_MAX_C, vqtts.CH_MAX_V) == (256, 1024)


def test_predictor_constructs_on_cpu_with_the_reference_keys():
    import torch
    from models.vqtts import CodePredictor
    from models.vqtts.predictor import CodePredictor as direct
    assert direct is CodePredictor
    c, v = 128, 512
    m = CodePredictor(c, v)
    want = {}
    for i in range(4):
        want[f"quant_decoder.model.{i}.model.2.weight"] = (2 * c, c, 3)
        want[f"quant_decoder.model.{i}.model.2.bias"] = (2 * c,)
        want[f"quant_decoder.model.{i}.model.5.weight"] = (c, 2 * c, 1)
        want[f"quant_decoder.model.{i}.model.5.bias"] = (c,)
    want["quant_proj.weight"], want["quant_proj.bias"] = (v, c, 1), (v,)
    sd = m.state_dict()
    assert {k: tuple(t.shape) for k, t in sd.items()} == want
    assert set(dict(m.named_parameters())) == set(want)
    for i in range(4):
        assert not sd[f"quant_decoder.model.{i}.model.5.weight"].any() and not sd[f"quant_decoder.model.{i}.model.5.bias"].any()
        assert sd[f"quant_decoder.model.{i}.model.2.weight"].any()
    assert m.dilations == [27, 9, 3, 1] and m.p_dropout == 0.1
    assert torch.is_floating_point(sd["quant_proj.weight"]) and sd["quant_proj.weight"].any()


def test_synthesize_codes_on_cpu():
    import torch
    from models.vqtts import CodePredictor
    m = CodePredictor(16, 32)
    x_id = torch.tensor([[5, 7, 9], [2, 0, 0]])
    align = torch.tensor([[0, 0, 1, 2, -1], [0, -1, -1, -1, -1]], dtype=torch.int32)
    pred = torch.tensor([[3, 31, 0, 8, 4], [1, 2, 3, 4, 5]], dtype=torch.int32)
    q = m.synthesize_codes(pred, x_id, align)
    assert q.dtype == torch.int64
    assert q.tolist() == [[5 * 32 + 3, 5 * 32 + 31, 7 * 32, 9 * 32 + 8, 0], [2 * 32 + 1, 0, 0, 0, 0]]
