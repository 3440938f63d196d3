// wrenc_dev.h -- CDNA4 (gfx950) device code of the all-intra RD-search path.
//
// Execution model: ONE 64-lane wavefront owns one 32x32 CTU; a workgroup is WPB = 4 waves working on
// the SAME CTU position of 4 different pictures, so the waves make the same sequence of full
// evaluations; each walks its own trellis (the one serial stage).  A wave keeps its
// working set in LDS (transform buffers, cached reference samples, the reconstruction tile with its
// neighbour border, trellis decisions, decision maps, search state: 7.2 KB, sized so that five workgroups
// = 20 waves fit a CU: the kernel is latency-bound per wave and its throughput follows the waves in
// flight); originals come from the picture's CTU tile (L1 / L2) or a staged copy in LDS, saved
// reconstructions live in a small pool of global scratch.  Search control
// is a scalar state machine that hands evaluation requests to one inlined evaluator: no device function
// calls, no scratch, every branch scalar.
//
// What is computed follows the reference function by function (paths relative to the reference's
// src/, cited at each function); how it is computed is wave-parallel.
//
// The search's headers, included below (wrenc_gpu.hip holds the search kernels, wrenc_gpu_test.hip runs their functions
// on single blocks), each with the part of the reference it follows and how its lanes share the work:
//   dev_const.h      (wrenc_gpu_config)             the constant block of a QP, plain C++ (filled by const_block.cpp)
//   dev_common.h     (shared by every device header) per-picture buffers, the LDS working set, search state, wave helpers
//   dev_predict.h    intra_predictor.rs:56-2055     lane = sample; SAD lists of many modes in one loop
//   dev_pk16.h       (helpers of the rows)          two samples of a row per 16-bit packed instruction
//   dev_transform.h  transformer.rs:2040-2737       lane = basis row, v_dot2 / v_mad_i24
//   dev_scan.h       ctu.rs:54-77, 827-845          the coefficient scan as arithmetic
//   dev_quant.h      quantizer.rs:338-759           backward 4-state Viterbi, one lane per state, DPP
//   dev_search.h     block_splitter.rs:64-1154, ctu_encoder.rs:1421-1461
// The picture passes, included by the unit that launches them (wrenc_gpu_io.hip) over dev_common.h and two helpers of the
// search (dev_quant.h's state maps for the tokens, dev_transform.h's dot2 for the scaler):
//   dev_bins.h       ctu_encoder.rs:1786-2269       residual_coding as a token stream for the host's arithmetic coder
//   dev_metrics.h    (the evaluation harness)       PSNR / SSIM sums of originals against the reconstruction
//   dev_hash.h       (no counterpart)               decoded picture hash (MD5, CRC, checksum) of the reconstruction
//   dev_complexity.h (no counterpart)               SATD of the originals per CTU and picture, for the rate control
//   dev_ratecurve.h  (no counterpart)               rate histogram of the originals (prediction, Hadamard, magnitude bins)
//   dev_distcurve.h  (no counterpart)               distortion curve of the originals (the same coefficients at all 64 QPs)
//   dev_pad.h        (no counterpart)               a picture's last column and row replicated into the coded size's margin
//   dev_scale.h      (no counterpart)               resampling of an uploaded picture to the visible size
//   dev_format.h     (no counterpart)               10-bit, NV12 / P010 and 4:2:2 uploads to the 8-bit 4:2:0 planes
//   dev_rgb.h        (no counterpart)               RGB uploads to the 8-bit 4:2:0 Y'CbCr planes (matrix, range, 2x2 chroma mean)
#pragma once

// The WRENC_EXP_* switches are measurement builds (tools/README.md); several of them give wrong results on purpose.
// tools/build_exp.sh builds them with WRENC_EXPERIMENT_BUILD, which nothing else defines.
#if !defined(WRENC_EXPERIMENT_BUILD) &&                                                                             \
    (defined(WRENC_EXP_CTRL_ONLY) || defined(WRENC_EXP_LDS_PAD) || defined(WRENC_EXP_NOINLINE_SAD) ||               \
     defined(WRENC_EXP_NO_ORG) || defined(WRENC_EXP_OLD_PDPC) || defined(WRENC_EXP_SKIP_DCT) ||                     \
     defined(WRENC_EXP_SKIP_PRED) || defined(WRENC_EXP_SKIP_QUANT) || defined(WRENC_EXP_SKIP_REFS) ||               \
     defined(WRENC_EXP_SKIP_SAD))
#error "a WRENC_EXP_* switch is set outside an experiment build: use tools/build_exp.sh"
#endif

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_common.h"
#include "dev_pk16.h"
#include "dev_predict.h"
#include "dev_transform.h"
#include "dev_scan.h"
#include "dev_quant.h"
#include "dev_search.h"
