"""The VQTTS text-audio alignment without a GPU: the new entry points are declared in the header and bound with matching
ABI numbers, and the module constructs with no state."""
import os
import re

from conftest import REPO

NEW = {"smt_vqtts_distance", "smt_vqtts_align_workspace_bytes", "smt_vqtts_align", "smt_vqtts_align_loss",
       "smt_vqtts_align_loss_bwd"}


def test_alignment_entry_points_are_declared_and_bound():
    from smt_amd import native
    header = open(os.path.join(REPO, "include", "smt_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(smt_\w+)\s*\(", header))
    assert NEW <= declared and NEW <= set(native.exported_symbols())
    abi = int(re.search(r"smt_abi_version\(void\)\s*\{\s*return\s+(\d+)", open(os.path.join(
        REPO, "speech-masters-thesis_amd", "csrc", "common.hip")).read()).group(1))
    assert abi == native.ABI_VERSION >= 9
    lib = native.lib()                                        # the built library exports them with the bound signatures
    assert lib.smt_vqtts_align_workspace_bytes(32, 200, 18176) == 32 * 18176 * 4 * 8
    assert lib.smt_vqtts_align_workspace_bytes(0, 200, 18176) == 0


def test_kernel_constants_match_the_source():
    from smt_amd import vqtts
    src = open(os.path.join(REPO, "speech-masters-thesis_amd", "csrc", "vqtts_align.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (VA_\w+) = (\d+);", src)}
    assert (const["VA_SLAB"], const["VA_CHUNK"], const["VA_WALK"]) == (vqtts.ALIGN_SLAB, vqtts.ALIGN_CHUNK, vqtts.ALIGN_WALK)


def test_module_constructs_on_cpu_with_no_state():
    from models.vqtts import TextAudioAlignment
    from models.vqtts.align import TextAudioAlignment as direct
    m = TextAudioAlignment()
    assert direct is TextAudioAlignment
    assert len(m.state_dict()) == 0 and list(m.parameters()) == [] and list(m.buffers()) == []
