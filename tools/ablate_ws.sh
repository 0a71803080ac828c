#!/bin/bash
# A/B build of conv_ws.hip with -DSMT_WS_AB=1 (the SMT_CONV_NO_WS2 / SMT_CONV_NO_PIPE switches and the six kernel
# instantiations only they can reach) into a library of its own (the product build is never touched), then
# tools/bench_ws.py with the default dispatch, without the two-wave kernels and without the pipelined kernel.  Run on the GPU box.
set -e
cd "$(dirname "$0")/../speech-masters-thesis_amd/csrc"
make -s && mkdir -p build_abl && cp build/*.o build_abl/
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=on -DSMT_WS_AB=1 -c conv_ws.hip -o build_abl/conv_ws.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../smt_amd/libsmt_hip_abl.so build_abl/*.o
export SMT_HIP_LIB="$PWD/../smt_amd/libsmt_hip_abl.so"
cd ../..
echo "== default";          python3 tools/bench_ws.py
echo "== SMT_CONV_NO_WS2";  SMT_CONV_NO_WS2=1 python3 tools/bench_ws.py
echo "== SMT_CONV_NO_PIPE"; SMT_CONV_NO_PIPE=1 python3 tools/bench_ws.py
