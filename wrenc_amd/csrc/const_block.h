// const_block.h -- everything the library derives from a config alone, as host-only C++ (const_block.cpp): the rate model
// (a wrenc_gpu_config's tables from the reference's --extra-params constants) and the constant block of one QP (DevConst,
// dev_const.h) from such a config.  No HIP header, no context: the same source is compiled into libwrenc_gpu.so and into
// a stand-alone program (tools/sanitize/const_block.cpp), and wrenc_gpu_test_const_field shows every member to the CPU tests.
#pragma once
#include "../../include/wrenc_gpu.h"
#include "dev_const.h"

#include <string>

#ifndef WRENC_HIDDEN
#define WRENC_HIDDEN __attribute__((visibility("hidden")))
#endif

// The RD-model constants the reference reads from --extra-params, with its defaults for the live
// (dependent quantisation + trellis) variants: block_splitter.rs:29-44,187-375,594-693,775 and
// quantizer.rs:16-19,650-683.  Types follow the reference's parse::<f64> / <f32> / <i64>.
struct RdParams {
    double lv_pow = 0.48592678233563835, lv_offset = 0.15150746310196822;               // lv_dq_trellis_table
    double quant_lv_pow = 0.5004010166085378;                                            // dq_table
    double quant_qp_div = 5.218413785332902, quant_lambda_mul = 1.2709404305806742;      // lambda of the trellis
    long long quant_lambda_offset = 11;
    float qp_div = 4.4043665f, lambda_mul = 1.1282581f;
    float non_planar_offset = 2.2153597f, mpm_idx_offset = 1.3660221f, mpm_remainder_mult = 0.5007182f,
          mpm_remainder_offset = 2.2973304f, planar_offset = 0.9626864f, header_bits = 1.1772872f,
          chroma_header_bits = 1.309252f, cclm_pow = 0.4587651f, mpm_idx_pow = 0.40271285f,
          mpm_remainder_pow = 0.34385094f, cclm_mode_idx_offset = 2.1f, non_cclm_offset = 0.89f, cclm_offset = 0.53f;
    bool has_a = false; // "a" replaces lambda_mul in the chroma cost function (block_splitter.rs:775-778)
    float a = 0.0f;
};

// the tables and lambdas of cfg->qp from `p` (the size, depth, device and slots of `cfg` are left alone)
WRENC_HIDDEN void resolve_config(wrenc_gpu_config* cfg, const RdParams& p);
// wrenc_gpu_config_extra_params without the error path: WRENC_GPU_OK, or WRENC_GPU_EINVAL with the message in `err`
WRENC_HIDDEN int config_extra_params(wrenc_gpu_config* cfg, const char* extra_params, std::string& err);
// the device's 32-bit trellis costs cover this config's rate model (else kRateModelMsg)
WRENC_HIDDEN bool rate_model_fits(const wrenc_gpu_config& cfg);
WRENC_HIDDEN extern const char* const kRateModelMsg;
// the constant block of cfg.qp
WRENC_HIDDEN void fill_dev_const(const wrenc_gpu_config& cfg, wrenc::DevConst& k);
