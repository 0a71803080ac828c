#!/bin/bash
# Diagnostic build of conv_wgrad.hip with -DSMT_WGRAD_STAMP=1 (per-wave cycle sums of the phases of conv_wgrad_kernel and
# conv_wgrad_shift_kernel) into a library of its own (the product build is never touched), then tools/wgrad_phases.py (shift
# kernel) and tools/wgrad_generic_phases.py (generic kernel).  Run on the GPU box.  WGRAD_FLAGS adds to the diagnostic build,
# e.g. WGRAD_FLAGS=-DSMT_WGRAD_PREFETCH=0 for the generic kernel without its register prefetch.
set -e
cd "$(dirname "$0")/../speech-masters-thesis_amd/csrc"
make -s && mkdir -p build_abl && cp build/*.o build_abl/
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=on -DSMT_WGRAD_STAMP=1 $WGRAD_FLAGS -c conv_wgrad.hip -o build_abl/conv_wgrad.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../smt_amd/libsmt_hip_abl.so build_abl/*.o
export SMT_HIP_LIB="$PWD/../smt_amd/libsmt_hip_abl.so"
cd ../.. && python3 tools/wgrad_phases.py && python3 tools/wgrad_generic_phases.py
