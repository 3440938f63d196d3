// ASan + UBSan over wrenc_amd/csrc/const_block.cpp, the host unit that derives a config's tables and a QP's constant block:
// default configs at every QP and depth through resolve_config, rate_model_fits and fill_dev_const; the --extra-params
// strings of tests/test_abi.py and tests/test_gpu_extra_params.py; malformed strings, with the status each has today.
// Stand-alone, no HIP (tools/sanitize/run.sh builds it with g++ and runs it); never loaded into Python.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../../wrenc_amd/csrc/const_block.h"

using namespace wrenc;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "const_block: line %d: %s (%s)\n", __LINE__, #cond, what); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

// wrenc_gpu_default_config, which lives with the ABI
static void default_config(wrenc_gpu_config& cfg, int qp, int depth) {
    memset(&cfg, 0, sizeof(cfg));
    cfg.width = 64;
    cfg.height = 96;
    cfg.qp = qp;
    cfg.max_split_depth = depth;
    cfg.n_slots = 1;
    resolve_config(&cfg, RdParams());
}

// the block of a config the library would build one for (wrenc_gpu_create refuses the others before it gets here)
static int block_of(const wrenc_gpu_config& cfg, DevConst& k, const char* what) {
    fill_dev_const(cfg, k);
    CHECK(k.qp == cfg.qp && k.W == cfg.width && k.H == cfg.height && k.max_depth == cfg.max_split_depth);
    CHECK(k.ctu_cols == cfg.width / 32 && k.ctu_rows == cfg.height / 32 && k.lsc > 0 && k.div_magic != 0);
    for (int idx = 0; idx < 4; ++idx) { // the scan table is a permutation of each block size's positions
        const int nn = 16 << (2 * idx);
        bool seen[1024] = {};
        for (int p = 0; p < nn; ++p) {
            CHECK(k.scan_idx[idx][p] < nn && !seen[k.scan_idx[idx][p]]);
            seen[k.scan_idx[idx][p]] = true;
        }
        for (int r = 0; r < 6; r += 2) CHECK(k.head_rng[idx][r] >= 0 && k.head_rng[idx][r + 1] >= 0 && k.head_rng[idx][r + 1] <= 65536);
    }
    for (const float f : k.split_floor) CHECK(f >= 0.0f);
    return 0;
}

int main() {
    std::unique_ptr<DevConst> k(new DevConst());
    wrenc_gpu_config cfg;
    std::string err;
    int blocks = 0, strings = 0;
    for (int qp = 0; qp < 64; ++qp)
        for (int depth = 0; depth < 4; ++depth) {
            const char* what = "default config";
            default_config(cfg, qp, depth);
            CHECK(rate_model_fits(cfg));
            if (block_of(cfg, *k, what)) return 1;
            ++blocks;
        }
    // strings the parser accepts: every live key (with dead and unknown ones), dead keys only, the rate models that
    // wrenc_gpu_create then refuses, no string and an empty one, an empty key, unknown keys, 64 KB of items
    const std::string live =
        "lv_pow_dq_trellis=0.52,lv_offset_dq_trellis=0.2,quant_lv_pow=0.49,quant_qp_div_trellis=5.0,"
        "quant_lambda_mul_trellis=1.4,quant_lambda_offset_trellis=7,qp_div_dq_trellis=4.2,lambda_mul_dq_trellis=1.3,"
        "non_planar_offset_dq_trellis=2.0,mpm_idx_offset_dq_trellis=1.5,mpm_remainder_mult_dq_trellis=0.6,"
        "mpm_remainder_offset_dq_trellis=2.1,planer_offset_dq_trellis=1.1,header_bits_dq_trellis=1.0,"
        "chroma_header_bits_dq_trellis=1.5,cclm_pow=0.5,mpm_idx_pow=0.45,mpm_remainder_pow=0.3,"
        "cclm_mode_idx_offset_dq_trellis=2.4,non_cclm_offset_dq_trellis=0.7,cclm_offset_dq_trellis=0.6,a=0.9,"
        "lv_pow_dq=0.1,header_bits=9.0,some_future_knob=1";
    std::string long_ok;
    while (long_ok.size() < 65536) long_ok += "some_future_knob=1,";
    long_ok += "a=0.5";
    const std::string good[] = {live, "lv_pow_dq=0.1,header_bits=9.0,x=y", "quant_lv_pow=2.5", "quant_qp_div_trellis=1.5",
                                "quant_lambda_mul_trellis=-3", "quant_lambda_mul_trellis=0.02", "quant_lambda_mul_trellis=60",
                                "quant_lambda_mul_trellis=0", "quant_qp_div_trellis=3.2", "quant_lv_pow=0.8,quant_lambda_offset_trellis=9",
                                "quant_lv_pow=0.3", "a=0.05", "a=3.0", "quant_lambda_mul_trellis=3.0,quant_lambda_offset_trellis=40",
                                "quant_lambda_mul_trellis=86", "quant_lambda_mul_trellis=44", "", "=1", "no_such_key=1", "no_such_key=",
                                long_ok};
    // every string at the QPs the tests use any of them with (22, 27, 32, 37) and at both ends of the range
    for (const std::string& s : good)
        for (const int qp : {0, 22, 27, 32, 37, 63}) {
            const char* what = s.size() > 80 ? "a long string" : s.c_str();
            default_config(cfg, qp, 3);
            CHECK(config_extra_params(&cfg, s.c_str(), err) == WRENC_GPU_OK);
            // the two models at the edge of what wrenc_gpu_create accepts (tests/test_gpu_extra_params.py), where the
            // products of fill_dev_const and fill_head_ranges are largest: accepted, so their blocks are built here
            if ((s == "quant_lambda_mul_trellis=86" && qp == 32) || (s == "quant_lambda_mul_trellis=44" && qp == 37))
                CHECK(rate_model_fits(cfg) && cfg.lambda_q * cfg.dq_table[1023] > 24000000);
            if (rate_model_fits(cfg) && block_of(cfg, *k, what)) return 1;
            ++strings;
        }
    {
        const char* what = "no string";
        default_config(cfg, 32, 2);
        const wrenc_gpu_config before = cfg;
        CHECK(config_extra_params(&cfg, nullptr, err) == WRENC_GPU_OK && !memcmp(&before, &cfg, sizeof(cfg)));
    }
    // strings it refuses: the config stays as it was and the message names the string or the key
    const std::string bad[] = {"a", "a=", "a=1=2", "a=1,", "a=1,,b=2", ",", "qp_div_dq_trellis=abc", "quant_lambda_offset_trellis=1.5",
                               "cclm_pow=1e", "some_future_knob=1,a", std::string(65536, 'a'), long_ok + ","};
    for (const std::string& s : bad) {
        const char* what = s.size() > 80 ? "a long string" : s.c_str();
        default_config(cfg, 32, 2);
        const wrenc_gpu_config before = cfg;
        err.clear();
        CHECK(config_extra_params(&cfg, s.c_str(), err) == WRENC_GPU_EINVAL);
        CHECK(!err.empty() && !memcmp(&before, &cfg, sizeof(cfg)));
        ++strings;
    }
    printf("const_block: %d constant blocks, %d extra-params strings clean\n", blocks, strings);
    return 0;
}
