#!/bin/bash
# Experiment build of the HIP library into xbuild/ (git-ignored, travels to the GPU box):
#   tools/build_exp.sh NAME [extra hipcc flags, e.g. -DWRENC_EXP_SKIP_QUANT]
# then  WRENC_GPU_LIB=xbuild/NAME.so python tools/fill_probe.py ...
# The WRENC_EXP_* switches compile only with WRENC_EXPERIMENT_BUILD, which this script passes.  A failed compile
# leaves no xbuild/NAME.so and no xbuild/NAME.flags behind (the flags file is written only next to a fresh library).
set -euo pipefail
cd "$(dirname "$0")/.."
name=$1
shift
mkdir -p xbuild
rm -f "xbuild/$name.so" "xbuild/$name.flags"
if ! /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -mllvm -sink-insts-to-avoid-spills=1 -mllvm -disable-machine-licm \
        -DWRENC_EXPERIMENT_BUILD "$@" -o "xbuild/$name.so" wrenc_amd/csrc/wrenc_gpu.hip wrenc_amd/csrc/wrenc_gpu_io.hip \
        wrenc_amd/csrc/const_block.cpp wrenc_amd/csrc/wrenc_gpu_test.hip > "xbuild/$name.log" 2>&1; then
    grep -E " error|error:" "xbuild/$name.log" >&2 || tail -n 20 "xbuild/$name.log" >&2
    rm -f "xbuild/$name.so"
    echo "build_exp.sh: $name failed (xbuild/$name.log)" >&2
    exit 1
fi
echo "$(git rev-parse --short HEAD)$(git diff --quiet || echo +dirty) $*" > "xbuild/$name.flags"
ls -la "xbuild/$name.so"
