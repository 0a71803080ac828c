"""The VQTTS code-emission entry point without a GPU: declared, bound and exported under the unchanged ABI number, and its
argument errors, which are decided on the host before any launch."""
import os
import re

import pytest
import torch

from conftest import PKG, REPO

CSRC = os.path.join(PKG, "csrc")


def test_emit_entry_point_is_declared_bound_and_exported():
    from smt_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "smt_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smt_\w+)\s*\(", header))
    assert "smt_vqtts_emit" in declared and "smt_vqtts_emit" in native.exported_symbols()
    assert declared == set(native.exported_symbols())
    abi = int(re.search(r"smt_abi_version\(void\)\s*\{\s*return\s+(\d+)", open(os.path.join(CSRC, "common.hip")).read()).group(1))
    lib = native.lib()
    assert abi == native.ABI_VERSION == lib.smt_abi_version()
    assert hasattr(lib, "smt_vqtts_emit")
    res, args = native._SIGNATURES["smt_vqtts_emit"]
    assert res is native.c_int and len(args) == 14 and args[5:11] == [native.c_int] * 6


def test_emit_argument_errors_need_no_launch():
    from smt_amd import native
    lib = native.lib()
    assert lib.smt_vqtts_emit(None, None, None, None, None, 1, 1, 1, 1, 1, 6, None, None, None) != 0
    assert b"multiple of 4" in lib.smt_last_error()
    assert lib.smt_vqtts_emit(None, None, None, None, None, 0, 5, 7, 3, 2, 8, None, None, None) == 0      # batch 0: no-op
    assert lib.smt_vqtts_emit(None, None, None, None, None, 2, 5, 0, 3, 2, 8, None, None, None) == 0      # t_q 0
    assert lib.smt_vqtts_emit(None, None, None, None, None, 2, 5, 7, 3, 2, 0, None, None, None) == 0      # dim 0
    assert lib.smt_vqtts_emit(None, None, None, None, None, 2, 5, 7, 3, 2, 8, None, None, None) != 0      # null pointers
    assert lib.smt_vqtts_emit(None, None, None, None, None, -1, 5, 7, 3, 2, 8, None, None, None) != 0     # negative size


def test_emit_codes_refuses_host_tensors():
    from smt_amd import vqtts
    with pytest.raises(ValueError, match="device tensor"):
        vqtts.emit_codes(torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1, dtype=torch.int32),
                         torch.zeros(1, dtype=torch.int32), torch.zeros(4, 8), 2, 2)
