"""The launch plan and the tile split of the streaming conv kernels (csrc/conv_stream.h: plan_stream, tile_run) compiled for
the HOST and checked for every plan in use: the closed formula, whole XCD octets, and runs that are pairwise disjoint, cover
all tiles and use every workgroup slot once: tests/native/stream_plan_host.cpp.  No GPU involved; hipcc only as the compiler."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_plan_on_the_host(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "stream_plan_host"
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests/native/stream_plan_host.cpp"), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and "FAIL" not in res.stdout and "failures 0" in res.stdout, res.stdout[-4000:]
    assert res.stdout.count("case ntiles") == 14 * 5, res.stdout[-4000:]
