#!/bin/bash
# ASan + UBSan over the host writer and the stream parser: bash tools/sanitize/run.sh [WIDTH HEIGHT QP DEPTH]
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
W=${1:-256}; H=${2:-128}; QP=${3:-27}; D=${4:-3}
T=$(mktemp -d)
python3 - "$R" "$T" "$W" "$H" "$QP" "$D" <<'PY'
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import pyoracle as po
from wrenc_amd import synth
t, w, h, qp, d = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
y, cb, cr = synth.synth_textured_frame(1920, 1088, 1)
rec = po.encode_picture(y[:h, :w].copy(), cb[:h // 2, :w // 2].copy(), cr[:h // 2, :w // 2].copy(), qp, d)
for k in ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr"):
    np.ascontiguousarray(rec[k]).tofile("%s/%s.bin" % (t, k))
PY
H0=$R/wrenc_amd/csrc/host
g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -o "$T/harness" "$R/tools/sanitize/harness.cpp" $H0/slice_data.cpp $H0/headers.cpp $H0/wrenc_bitstream.cpp \
    "$R/oracle/vvc_parse.cpp" "$R/oracle/wrenc_oracle.cpp" 2> "$T/build.log" || { cat "$T/build.log"; exit 1; }
# QP of the stream is fixed to 32 in the harness's writer calls; the record's own QP only shaped its levels
"$T/harness" "$T" "$W" "$H"
g++ -O1 -g -std=c++17 -ffp-contract=off -mavx2 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -o "$T/oracle_search" "$R/tools/sanitize/oracle_search.cpp" "$R/oracle/wrenc_oracle.cpp" "$R/oracle/vvc_parse.cpp"
"$T/oracle_search"
# the scaling filter's tap derivation (include/wrenc_scale.h), 64-bit intermediates at the largest sizes included
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -o "$T/scale_taps" "$R/tools/sanitize/scale_taps.cpp"
"$T/scale_taps"
# the source-format converter's kernel body on the host (wrenc_amd/csrc/dev_format.h against include/wrenc_format.h); clang++
# for the vector types the kernel is written with
${CLANGXX:-/opt/rocm/lib/llvm/bin/clang++} -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -o "$T/format_convert" "$R/tools/sanitize/format_convert.cpp"
"$T/format_convert"
# the buffer model's host code: the rate histogram's definition (include/wrenc_ratecurve.h) and the controller's chooser,
# bucket and re-encode step (include/wrenc_rate_vbv.h) over random histograms and sizes
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -o "$T/rate_vbv" "$R/tools/sanitize/rate_vbv.cpp" $H0/rate_control.cpp
"$T/rate_vbv"
# the quality mode's host code: the distortion curve's definition (include/wrenc_distcurve.h), the kernel's division-free
# quantiser (wrenc_amd/csrc/distcurve_quant.h) against it at every magnitude and QP, and the controller
# (include/wrenc_rate_quality.h) over random curves and PSNR tables.  -ffp-contract=off as the library is built: the
# quantiser's multiply-adds are explicit fmaf calls either way, the flag keeps everything around them uncontracted too
g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -o "$T/rate_quality" "$R/tools/sanitize/rate_quality.cpp" $H0/rate_quality.cpp
"$T/rate_quality"
# the launch plan of an encode call (wrenc_amd/csrc/encode_plan.h) over the sweep of tests/test_encode_plan.py
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -o "$T/encode_plan" "$R/tools/sanitize/encode_plan.cpp"
"$T/encode_plan"
# the items of wrenc_gpu_test_predict (wrenc_amd/csrc/predict_items.h): the cases of tests/test_predict_layout.py and random items
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -o "$T/predict_items" "$R/tools/sanitize/predict_items.cpp"
"$T/predict_items"
# the owners of device memory, streams and events (wrenc_amd/csrc/host_mem.h) against stub definitions of the HIP calls they
# use: no HIP library
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -D__HIP_PLATFORM_AMD__ -I"${ROCM_PATH:-/opt/rocm}/include" -o "$T/host_mem" "$R/tools/sanitize/host_mem.cpp"
"$T/host_mem"
# the rate model and the constant block (wrenc_amd/csrc/const_block.cpp): every QP and depth, the --extra-params strings of the
# tests and malformed ones; the library's own source under g++, warnings on: no HIP
g++ -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -o "$T/const_block" "$R/tools/sanitize/const_block.cpp" "$R/wrenc_amd/csrc/const_block.cpp"
"$T/const_block"
rm -rf "$T"
