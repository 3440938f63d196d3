// wrenc_gpu_test.hip -- the block tests of libwrenc_gpu.so (include/wrenc_gpu_test.h): kernels that run ONE device
// function of the search on blocks the caller brings, and the entries that launch them or run a device pass on a picture
// of their own.  A translation unit and a code object of its own: what is added or changed here cannot move an
// instruction of the kernels in wrenc_gpu.hip, which is built into the same library by the same command.
//
// The trace and profile builds (-DWRENC_TRACE, -DWRENC_PROFILE) define their device globals in dev_common.h; this unit
// records no trace and counts no cycles, so it compiles without them and the library holds one copy of each: the one
// wrenc_gpu_trace_read and wrenc_gpu_prof_read (wrenc_gpu.hip) read.
#undef WRENC_TRACE
#undef WRENC_PROFILE
#include <hip/hip_runtime.h>
// dev_metrics.h and dev_hash.h define kernels that are no templates.  This unit needs the two headers for what its
// metrics and hash entries hand to the launchers of wrenc_gpu_io.hip (MetricsPartial, HashTables, met_plane, ...) and
// launches none of their kernels: here they are device functions nothing calls, so they are neither compiled a second
// time nor defined twice in the library.
#pragma push_macro("__global__")
#pragma push_macro("__launch_bounds__")
#undef __global__
#undef __launch_bounds__
#define __global__ static __device__
#define __launch_bounds__(...)
#include "wrenc_dev.h"
#include "dev_metrics.h"
#include "dev_hash.h"
#include "gpu_ctx.h"
#pragma pop_macro("__launch_bounds__")
#pragma pop_macro("__global__")
#include "../../include/wrenc_gpu_test.h"
#include "predict_items.h"

#include <cstring>
#include <memory>

static_assert(kItemCclmFirst == LT_CCLM && kItemCclmLast == T_CCLM && kItemNoMode == kNoMode, "predict_items.h restates the modes");

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// building-block kernels: one wave per group of nb blocks of side 1 << lg, laid out [blk][y][x]; the transforms and the
// dequantiser work on r1[o1 ..], where the search puts a pack's chroma behind its luma (the host entries check that the
// group fits r1 and r2)
__global__ __launch_bounds__(64) void test_fwd_dct_kernel(const DevConst* __restrict__ k,
                                                          const int16_t* in, int lg, int nb, int o1, int16_t* out,
                                                          int arm, int reps) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    const int total = nb << (2 * lg);
    // arm: DCT_SEARCH, or the version of the 8x8 / 16x16 transforms the host names (dev_transform.h); reps repeats the
    // transform of the same group for the micro-benchmark
    for (int rep = 0; rep < reps; ++rep) {
        for (int i = threadIdx.x; i < total; i += 64) SH.r1[o1 + i] = in[(size_t)blockIdx.x * total + i];
        WSYNC();
        if (arm == DCT_VDOT2)
            fwd_dct_lg<DCT_VDOT2>(c, lg, nb, o1);
        else if (arm == DCT_MFMA)
            fwd_dct_lg<DCT_MFMA>(c, lg, nb, o1);
        else
            fwd_dct_lg(c, lg, nb, o1);
    }
    for (int i = threadIdx.x; i < total; i += 64) out[(size_t)blockIdx.x * total + i] = SH.r1[o1 + i];
}

// MFMA experiment: the 32x32 forward transform as i8 MFMAs (dev_transform.h); `reps` repeats the transform
// of the same block in place for the micro-benchmark (the result of the last repetition is stored)
__shared__ int32_t s_h32[33 * 32]; // the v_dot2 arm's i32 intermediate (the search kernel has no such room)
__global__ __launch_bounds__(64) void test_fwd_dct32_kernel(const DevConst* __restrict__ k, const int16_t* in, int16_t* out,
                                                           int mfma, int reps) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    for (int rep = 0; rep < reps; ++rep) {
        for (int i = threadIdx.x; i < 1024; i += 64) SH.r1[i] = in[(size_t)blockIdx.x * 1024 + i];
        WSYNC();
        if (mfma)
            fwd_dct32_mfma(c, 0);
        else
            fwd_dct<5, (int)sizeof(s_h32)>(c, 1, 0, (LDS_AS int32_t*)s_h32);
    }
    for (int i = threadIdx.x; i < 1024; i += 64) out[(size_t)blockIdx.x * 1024 + i] = SH.r1[i];
}

// the same for the inverse 32x32 transform: dequantised blocks in (row-major), residuals out
__global__ __launch_bounds__(64) void test_inv_dct32_kernel(const DevConst* __restrict__ k, const int16_t* in, int16_t* out,
                                                           int mfma, int reps) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    for (int rep = 0; rep < reps; ++rep) {
        for (int i = threadIdx.x; i < 1024; i += 64) // transposed load: dT[x][i] = d[i][x]
            ((int16_t*)SH.r2)[(i & 31) * 32 + (i >> 5)] = in[(size_t)blockIdx.x * 1024 + i];
        WSYNC();
        if (mfma)
            inv_dct32_mfma(c, 0);
        else
            inv_dct<5>(c, 1, 0);
    }
    for (int i = threadIdx.x; i < 1024; i += 64) out[(size_t)blockIdx.x * 1024 + i] = SH.r1[i];
}

__global__ __launch_bounds__(64) void test_inv_dct_kernel(const DevConst* __restrict__ k,
                                                          const int16_t* in, int lg, int nb, int o1, int16_t* out,
                                                          int arm, int reps) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    const int n = 1 << lg, nn = n * n, total = nb * nn;
    for (int rep = 0; rep < reps; ++rep) {
        for (int i = threadIdx.x; i < total; i += 64) { // transposed load, block by block: dT[blk][x][i] = d[blk][i][x]
            const int ii = i & (nn - 1);
            ((int16_t*)SH.r2)[(i - ii) + (ii & (n - 1)) * n + (ii >> lg)] = in[(size_t)blockIdx.x * total + i];
        }
        WSYNC();
        if (arm == DCT_VDOT2)
            inv_dct_lg<DCT_VDOT2>(c, lg, nb, o1);
        else if (arm == DCT_MFMA)
            inv_dct_lg<DCT_MFMA>(c, lg, nb, o1);
        else
            inv_dct_lg(c, lg, nb, o1);
    }
    for (int i = threadIdx.x; i < total; i += 64) out[(size_t)blockIdx.x * total + i] = SH.r1[o1 + i];
}

// quantize_solo: nb = 1 (a luma block) or 2 (the Cb + Cr pair) blocks at r1[0 ..]; per group the summed level cost and the
// *any_level the function reported
__global__ __launch_bounds__(64) void test_quantize_kernel(const DevConst* __restrict__ k,
                                                           const int16_t* in, int lg, int nb, int16_t* out,
                                                           long long* cost, int* any_level, int* overflow) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    load_tables(c);
    const int total = nb << (2 * lg);
    for (int i = threadIdx.x; i < total; i += 64) SH.r1[i] = in[(size_t)blockIdx.x * total + i];
    WSYNC();
    int ovf = 0;
    bool any = false;
    const long long lc = quantize_solo(c, lg, nb, &ovf, &any);
    for (int i = threadIdx.x; i < total; i += 64) out[(size_t)blockIdx.x * total + i] = SH.r1[i];
    if (threadIdx.x == 0) {
        cost[blockIdx.x] = lc;
        any_level[blockIdx.x] = any ? 1 : 0;
        if (ovf) atomicOr(overflow, 1);
    }
}

// DevConst::head_rng against the functions it stands for, over every 16-bit coefficient (grid: 1024 blocks of 64 lanes;
// block size and DC flag in blockIdx.y): out[0] += coefficients the range lets into the region that head_alpha ends it
// at (never allowed), out[1] += coefficients the range ends the region at that head_alpha would let in (allowed, not
// expected), out[2] += coefficients whose "quotient >= 2" differs from the range's, out[3] += alpha differences
__global__ __launch_bounds__(64) void test_head_ranges_kernel(const DevConst* __restrict__ kk, int* out) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)kk;
    load_tables(c);
    const CONST_AS DevConst* k = c.k;
    const int lg = 2 + (int)(blockIdx.y >> 1);
    const bool dcn = blockIdx.y & 1;
    const int tc = (int)(blockIdx.x * 64 + threadIdx.x) - 32768;
    const int sh = lg + 4, off = (1 << sh) >> 1;
    const HeadK hk = head_consts(sh, off, k->lsc);
    const HeadT ht = head_ranges(k, lg);
    const int qd = quotient(k, tc, sh, off);
    bool bad;
    const int alpha = head_alpha(tc, qd, dcn, hk, &bad);
    const bool rbad = head_bad(tc, dcn, ht);
    if (bad && !rbad) atomicAdd(out + 0, 1);
    if (!bad && rbad) atomicAdd(out + 1, 1);
    if ((qd >= 2) != head_sig(tc, ht)) atomicAdd(out + 2, 1);
    if (alpha != head_alpha1(tc, hk)) atomicAdd(out + 3, 1);
}

// DevConst::avail_tab + the picture's edges (block_avail_mask) against the formulas (block_avail_formula): one block per
// thread -- blockIdx.x = CTU, threadIdx.x = 4x4 position, blockIdx.y = size -- for luma and chroma spacing; *out +=
// differences
__global__ __launch_bounds__(64) void test_avail_tab_kernel(const DevConst* __restrict__ kk, int* out) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)kk;
    c.W = kk->W;
    c.ctu_x = 32 * (int)(blockIdx.x % (unsigned)kk->ctu_cols);
    c.ctu_y = 32 * (int)(blockIdx.x / (unsigned)kk->ctu_cols);
    const int lg = 2 + (int)blockIdx.y;
    const int bx = 4 * (int)(threadIdx.x & 7), by = 4 * (int)(threadIdx.x >> 3);
    if ((bx | by) & ((1 << lg) - 1)) return;
    for (int st = 1; st <= 2; ++st)
        if (block_avail_formula(c, bx, by, lg, st) != block_avail_mask(c, bx, by, lg, st)) atomicAdd(out, 1);
    // what cclm_params reads off the mask
    const int m = block_avail_mask(c, bx, by, lg, 1), tn = 1 << lg, gx = c.ctu_x + bx, gy = c.ctu_y + by;
    if (above_right_avail(c, bx, by, lg) != (((m >> 4) & 1) != 0)) atomicAdd(out, 1);
    if (below_left_avail(c, bx, by, lg) != ((m & 1) != 0)) atomicAdd(out, 1);
    if (nb_avail(c, gx, gy, tn, gx - 1, gy, false, false) != (((m >> 1) & 1) != 0)) atomicAdd(out, 1);
    if (nb_avail(c, gx, gy, tn, gx, gy - 1, false, false) != (((m >> 3) & 1) != 0)) atomicAdd(out, 1);
}

// quantize_p16_reg (the packed 4x4 leaf search's quantiser): each wave takes up to four consecutive 4x4 blocks
__global__ __launch_bounds__(64) void test_quantize_p16_kernel(const DevConst* __restrict__ k, const int16_t* in, int count,
                                                               int16_t* out, long long* cost, int* overflow) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    load_tables(c);
    const int first = 4 * blockIdx.x;
    const int nb = min(4, count - first);
    const bool mine = threadIdx.x < 16 * nb;
    int ovf = 0, any = 0;
    long long lvl[4];
    // the lane's coefficient in, the lane's level out
    const int level = quantize_p16_reg(c, nb, mine ? (int)in[(size_t)first * 16 + threadIdx.x] : 0, &ovf, lvl, &any);
    if (mine) out[(size_t)first * 16 + threadIdx.x] = (int16_t)level;
    if (threadIdx.x == 0) {
        for (int b = 0; b < nb; ++b) cost[first + b] = lvl[b];
        if (ovf) atomicOr(overflow, 1);
    }
}

// The register transforms of the 4x4 passes (dev_transform.h): four consecutive 4x4 blocks per wave, lane = (block,
// sample); forward: residuals -> fwd_dct4_reg; inverse: levels -> dequantize4_lane -> inv_dct4_reg.  Every lane runs the
// transform (rows past the last block carry zeros) and only the lanes of a block load and store.
__global__ __launch_bounds__(64) void test_dct4_reg_kernel(const DevConst* __restrict__ k, const int16_t* in, int count, int inverse,
                                                           int16_t* out) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    const size_t at = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool mine = at < (size_t)count * 16;
    const int v = mine ? (int)in[at] : 0;
    const int r = inverse ? inv_dct4_reg(dequantize4_lane(c, v)) : fwd_dct4_reg(v);
    if (mine) out[at] = (int16_t)r;
}

// recon_row4 (dev_predict.h): one row of four samples per lane, the lanes past the last row neither load nor store
__global__ __launch_bounds__(64) void test_recon_rows_kernel(const uint32_t* pred, const uint2* res, const uint32_t* org, int count,
                                                             uint32_t* rec, uint32_t* ssd) {
    const size_t at = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (at >= (size_t)count) return;
    unsigned s = 0;
    int v[4];
    rec[at] = recon_row4(pred[at], res[at], org[at], v, s);
    ssd[at] = s;
}

// quantize_pk (the packed leaf searches' quantiser): one wave per pack of nc candidates
__global__ __launch_bounds__(64) void test_quantize_pk_kernel(const DevConst* __restrict__ k, const int16_t* in, int lgl, int nc,
                                                              int16_t* out, long long* cost, int* overflow) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    load_tables(c);
    const int total = nc * 3 * (1 << (2 * lgl)) / 2;
    for (int i = threadIdx.x; i < total; i += 64) SH.r1[i] = in[(size_t)blockIdx.x * total + i];
    WSYNC();
    int ovf = 0;
    bool any_y = false, any_c = false;
    long long ly[3], lc[3];
    if (lgl == 3)
        quantize_pk<3>(c, nc, &ovf, ly, lc, &any_y, &any_c);
    else
        quantize_pk<4>(c, nc, &ovf, ly, lc, &any_y, &any_c);
    for (int i = threadIdx.x; i < total; i += 64) out[(size_t)blockIdx.x * total + i] = SH.r1[i];
    if (threadIdx.x == 0) {
        for (int b = 0; b < nc; ++b) {
            cost[((size_t)blockIdx.x * nc + b) * 2] = ly[b];
            cost[((size_t)blockIdx.x * nc + b) * 2 + 1] = lc[b];
        }
        if (ovf) atomicOr(overflow, 1);
    }
}

__global__ __launch_bounds__(64) void test_dequantize_kernel(const DevConst* __restrict__ k,
                                                             const int16_t* in, int lg, int nb, int o1, int16_t* out) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    const int n = 1 << lg, nn = n * n, total = nb * nn;
    for (int i = threadIdx.x; i < total; i += 64) SH.r1[o1 + i] = in[(size_t)blockIdx.x * total + i];
    WSYNC();
    dequantize_t(c, lg, nb, o1);
    for (int i = threadIdx.x; i < total; i += 64) { // undo the transpose, block by block
        const int ii = i & (nn - 1);
        out[(size_t)blockIdx.x * total + i] = ((const int16_t*)SH.r2)[(i - ii) + (ii & (n - 1)) * n + (ii >> lg)];
    }
}

// Prediction of single blocks in the environment of given reconstruction planes (one wave per item; the kinds, their mode
// words and output sizes: predict_items.h): the CTU's reconstruction tile and border are loaded from the planes, then
// reference samples + prediction run exactly as in a full evaluation of the final pass.  A SAD list takes the block's own
// samples in the planes as "originals" and puts out the 16 accumulators of lanes 0..15; a full candidate and a pack take
// them too (a CTU tile of originals is staged for c.org, and stage_org_leaf runs for blocks <= 16x16, as in the search)
// and put out the prediction bytes read back from the destination, in its layout, then the i16 residuals of r1.
constexpr int kTestPredictScratch = 1024 + kOrgTile; // per item: PRED_SCRATCH | the CTU's tile of originals

// an item as its kind's function gets it: the block in the picture and in its CTU, the planes, where the output goes
struct PredictItem {
    int x, y, tx, ty, tlg, kind, mode;
    const GLOBAL_AS uint8_t* rec;
    uint8_t* out;
};

// the block's own chroma samples where a SAD list reads its originals (stage_org / stage_org_leaf's layout): Cb | Cr
__device__ __forceinline__ void item_stage_chroma(Ctx& c, const PredictItem& q) {
    uint8_t* oc = (uint8_t*)SH.r2 + org_byte(1, q.tlg);
    const int nc = 1 << (q.tlg - 1), Wc = c.W >> 1;
    for (int i = LANE; i < 2 * nc * nc; i += 64) {
        const int pl = i >= nc * nc ? 1 : 0, ii = i - pl * nc * nc;
        oc[i] = q.rec[plane_off(c, 1 + pl) + (size_t)((q.y >> 1) + ii / nc) * Wc + (q.x >> 1) + ii % nc];
    }
}

// PK_LUMA, PK_CHROMA: predict_full to scratch
__device__ __forceinline__ void item_predict(Ctx& c, const PredictItem& q) {
    const int comp = q.kind;
    if (q.mode < LT_CCLM) build_refs(c, comp, q.tx, q.ty, q.tlg);
    if (comp == 0)
        predict_full<0>(c, q.tx, q.ty, q.tlg, q.mode, 0, PRED_SCRATCH);
    else
        predict_full<1>(c, q.tx, q.ty, q.tlg, q.mode, 0, PRED_SCRATCH);
    const int n = 1 << (q.tlg - (comp ? 1 : 0));
    const int total = (comp ? 2 : 1) * n * n;
    __threadfence_block();
    for (int i = LANE; i < total; i += 64) q.out[i] = c.pred_scratch[i];
}

// PK_LUMA4, the packed predictor of the 4x4 leaf search: the item's mode in row 0, other modes in the rows next to it
__device__ __forceinline__ void item_predict4(Ctx& c, const PredictItem& q) {
    build_refs(c, 0, q.tx, q.ty, 2);
    const int row = LANE >> 4;
    const int v = predict4_lane(c, row == 0 ? q.mode : (q.mode + 1 + 22 * row) % 67);
    if (LANE < 16) q.out[LANE] = (uint8_t)v;
}

// PK_SAD_LUMA, _CHROMA, _BOTH: sad_list_angular of entries m0 + j * stride (kNoMode beyond 66)
__device__ __forceinline__ void item_sad_list(Ctx& c, const PredictItem& q) {
    const int comps = q.kind - 3, m0 = q.mode & 255, nm = (q.mode >> 8) & 255, stride = q.mode >> 16;
    uint8_t* ol = (uint8_t*)SH.r2 + org_byte(0, q.tlg);
    const int n = 1 << q.tlg;
    for (int i = LANE; i < n * n; i += 64) ol[i] = q.rec[(size_t)(q.y + (i >> q.tlg)) * c.W + q.x + (i & (n - 1))];
    if (comps & 2) item_stage_chroma(c, q);
    WSYNC();
    if (comps & 1) build_refs(c, 0, q.tx, q.ty, q.tlg);
    if (comps & 2) build_refs(c, 1, q.tx, q.ty, q.tlg);
    unsigned long long lo = 0, hi = 0;
    for (int j = 0; j < nm; ++j) {
        const int m = m0 + j * stride;
        const unsigned long long e = (unsigned long long)(m <= 66 ? m : kNoMode) << (8 * (j & 7));
        if (j < 8) lo |= e; else hi |= e;
    }
    const unsigned acc = sad_list_angular(c, comps, q.tx, q.ty, q.tlg, nm, lo, hi);
    if (LANE < 16) ((uint32_t*)q.out)[LANE] = acc;
}

// PK_SAD_CCLM: sad_list_cclm of the chroma pair, lanes 0..2 = LT_CCLM, T_CCLM, L_CCLM
__device__ __forceinline__ void item_sad_cclm(Ctx& c, const PredictItem& q) {
    item_stage_chroma(c, q);
    WSYNC();
    const unsigned acc = sad_list_cclm(c, q.tx, q.ty, q.tlg);
    if (LANE < 16) ((uint32_t*)q.out)[LANE] = acc;
}

// PK_FULL_LUMA and beyond: the CTU's originals as retile_kernel lays them out, Y 32x32 | Cb 16x16 | Cr 16x16 (samples
// outside the picture: 0), for c.org; comps: what the kind predicts (bit 0 luma, bit 1 the chroma pair)
__device__ __forceinline__ void item_stage_originals(Ctx& c, const PredictItem& q, int comps) {
    uint8_t* tile = c.pred_scratch + 1024;
    const int W = c.W, Wc = W >> 1, H = c.k->H;
    for (int i = LANE; i < kOrgTile; i += 64) {
        const int pc = i < 1024 ? 0 : 1 + ((i - 1024) >> 8);
        const int ii = pc ? (i - 1024) & 255 : i;
        const int lgw = pc ? 4 : 5;
        const int gx = (pc ? c.ctu_x >> 1 : c.ctu_x) + (ii & ((1 << lgw) - 1)), gy = (pc ? c.ctu_y >> 1 : c.ctu_y) + (ii >> lgw);
        const int pw = pc ? Wc : W, ph = pc ? H >> 1 : H;
        tile[i] = (gx < pw && gy < ph) ? q.rec[plane_off(c, pc) + (size_t)gy * pw + gx] : 0;
    }
    __threadfence_block();
    WSYNC();
    c.org = (const GLOBAL_AS uint8_t*)tile;
    if (q.tlg <= 4) stage_org_leaf(c, comps, q.tx, q.ty, q.tlg);
}

// PK_FULL_LUMA, PK_FULL_CHROMA: predict_full of the luma block / the chroma pair into the recon tile
__device__ __forceinline__ void item_full(Ctx& c, const PredictItem& q) {
    const int cmp = q.kind - PK_FULL_LUMA;
    item_stage_originals(c, q, 1 + cmp);
    if (q.mode < LT_CCLM) build_refs(c, cmp, q.tx, q.ty, q.tlg);
    if (cmp == 0)
        predict_full<0>(c, q.tx, q.ty, q.tlg, q.mode, 0, PRED_TILE);
    else
        predict_full<1>(c, q.tx, q.ty, q.tlg, q.mode, 0, PRED_TILE);
    const int lg = q.tlg - cmp, n = 1 << lg, total = (cmp ? 2 : 1) * n * n;
    for (int i = LANE; i < total; i += 64) {
        const int blk = i >> (2 * lg), ii = i & (n * n - 1);
        q.out[i] = (uint8_t)rec_get(cmp + blk, (q.tx >> cmp) + (ii & (n - 1)), (q.ty >> cmp) + (ii >> lg));
        ((int16_t*)(q.out + total))[i] = SH.r1[i];
    }
}

// PK_PACK8: the luma part of an 8x8 pack (predict_pack8_luma) into PRED_PARK
__device__ __forceinline__ void item_pack8(Ctx& c, const PredictItem& q) {
    const int nc = q.mode >> 24, m0 = q.mode & 255, m1 = (q.mode >> 8) & 255, m2 = (q.mode >> 16) & 255;
    item_stage_originals(c, q, 1);
    build_refs(c, 0, q.tx, q.ty, 3);
    predict_pack8_luma(c, nc, m0, m1, m2);
    WSYNC();
    const uint8_t* park = (const uint8_t*)SH.decw + kParkByte;
    for (int i = LANE; i < 64 * nc; i += 64) {
        q.out[i] = park[i];
        ((int16_t*)(q.out + 64 * nc))[i] = SH.r1[i];
    }
}

// PK_PACK16: a 16x16 pack, luma and chroma pair (pack16_predict), into PRED_PARK16 (a candidate mode of kNoMode rides
// along as zeros)
__device__ __forceinline__ void item_pack16(Ctx& c, const PredictItem& q) {
    const int nc = q.mode >> 24, m0 = q.mode & 255, m1 = (q.mode >> 8) & 255;
    item_stage_originals(c, q, 3);
    build_refs(c, 0, q.tx, q.ty, 4);
    build_refs(c, 1, q.tx, q.ty, 4);
    pack16_predict(c, q.tx, q.ty, nc, m0, m1);
    WSYNC();
    for (int i = LANE; i < 384 * nc; i += 64) {
        q.out[i] = *park16(i, 256 * nc);
        ((int16_t*)(q.out + 384 * nc))[i] = SH.r1[i];
    }
}

// items: the host's checked items (predict_items.h), each followed by the offset of its output
__global__ __launch_bounds__(64) void test_predict_kernel(const DevConst* __restrict__ k, const uint8_t* planes,
                                                          const int* items, uint8_t* scratch, uint8_t* out) {
    const int* it = items + (kPredictItemInts + 1) * blockIdx.x;
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    c.org = (const GLOBAL_AS uint8_t*)planes; // residuals are computed against these and ignored
    c.W = k->W;
    c.WH = k->W * k->H;
    c.pred_scratch = scratch + (size_t)blockIdx.x * kTestPredictScratch;
    c.ctu_x = it[0] & ~31;
    c.ctu_y = it[1] & ~31;
    c.write = 1;
    load_tables(c);
    const int W = c.W, Wc = W >> 1;
    const GLOBAL_AS uint8_t* rec = (const GLOBAL_AS uint8_t*)planes;
    for (int i = LANE; i < 72; i += 64) {
        const int gx = c.ctu_x - 4 + i, gy = c.ctu_y - 1;
        SH.recYtop[i] = (gx >= 0 && gx < W && gy >= 0) ? rec[(size_t)gy * W + gx] : 0;
    }
    for (int i = LANE; i < 32 * 36; i += 64) {
        const int yy = i / 36, xx = i % 36 - 4;
        const int gx = c.ctu_x + xx, gy = c.ctu_y + yy;
        SH.recY[yy * 36 + xx + 4] = gx >= 0 ? rec[(size_t)gy * W + gx] : 0;
    }
    for (int pc = 1; pc < 3; ++pc) {
        for (int i = LANE; i < 40; i += 64) {
            const int gx = (c.ctu_x >> 1) - 4 + i, gy = (c.ctu_y >> 1) - 1;
            SH.recCtop[pc - 1][i] = (gx >= 0 && gx < Wc && gy >= 0) ? rec[plane_off(c, pc) + (size_t)gy * Wc + gx] : 0;
        }
        for (int i = LANE; i < 16 * 20; i += 64) {
            const int yy = i / 20, xx = i % 20 - 4;
            const int gx = (c.ctu_x >> 1) + xx, gy = (c.ctu_y >> 1) + yy;
            SH.recC[pc - 1][yy * 20 + xx + 4] = gx >= 0 ? rec[plane_off(c, pc) + (size_t)gy * Wc + gx] : 0;
        }
    }
    WSYNC();
    const PredictItem q = {it[0], it[1], it[0] & 31, it[1] & 31, it[2], it[3], it[4], rec, out + it[kPredictItemInts]};
    switch (q.kind) {
    case PK_LUMA:
    case PK_CHROMA: return item_predict(c, q);
    case PK_LUMA4: return item_predict4(c, q);
    case PK_SAD_LUMA:
    case PK_SAD_CHROMA:
    case PK_SAD_BOTH: return item_sad_list(c, q);
    case PK_SAD_CCLM: return item_sad_cclm(c, q);
    case PK_FULL_LUMA:
    case PK_FULL_CHROMA: return item_full(c, q);
    case PK_PACK8: return item_pack8(c, q);
    case PK_PACK16: return item_pack16(c, q);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

// One device buffer of an entry: `bytes` that are uploaded from `src` before the launch (NULL: cleared where `zero`, else
// left as they come) and downloaded to `dst` after it (NULL: not).  An empty one stays a null pointer.
struct TestBuf {
    const void* src;
    void* dst;
    size_t bytes;
    bool zero;
    DevBuf<uint8_t> d;
    template <class T>
    T* as() const { return reinterpret_cast<T*>(d.get()); }
};
template <class T>
TestBuf buf_in(const T* src, size_t n) { return TestBuf{src, nullptr, n * sizeof(T), false, {}}; }
template <class T>
TestBuf buf_out(T* dst, size_t n, bool zero = false) { return TestBuf{nullptr, dst, n * sizeof(T), zero, {}}; }

// What every entry does around its kernels, in this order and on the context's stream: the device, the buffers' memory,
// the uploads, launch(stream) and its launch check, the downloads, one synchronise.
// kernel_ms: NULL, or where the HIP-event duration of what `launch` queued goes (the transform micro-benchmarks)
template <class Launch>
int run_on_stream(wrenc_gpu_ctx* ctx, const std::vector<TestBuf*>& bufs, Launch launch, float* kernel_ms = nullptr) {
    hipStream_t st = ctx->stream.get();
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    for (TestBuf* b : bufs) HIP_TRY(ctx, b->d.alloc(b->bytes));
    HipEvent e0, e1;
    if (kernel_ms) {
        *kernel_ms = 0.f;
        HIP_TRY(ctx, e0.create());
        HIP_TRY(ctx, e1.create());
    }
    for (TestBuf* b : bufs) {
        if (b->src)
            HIP_TRY(ctx, hipMemcpyAsync(b->d.get(), b->src, b->bytes, hipMemcpyHostToDevice, st));
        else if (b->zero)
            HIP_TRY(ctx, hipMemsetAsync(b->d.get(), 0, b->bytes, st));
    }
    if (kernel_ms) HIP_TRY(ctx, hipEventRecord(e0.get(), st));
    HIP_TRY(ctx, launch(st));
    HIP_TRY(ctx, hipGetLastError());
    if (kernel_ms) HIP_TRY(ctx, hipEventRecord(e1.get(), st));
    for (TestBuf* b : bufs)
        if (b->dst && b->bytes) HIP_TRY(ctx, hipMemcpyAsync(b->dst, b->d.get(), b->bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (kernel_ms) HIP_TRY(ctx, hipEventElapsedTime(kernel_ms, e0.get(), e1.get()));
    return WRENC_GPU_OK;
}

// `count` groups of `nb` blocks to the device, launch(d_in, d_out) on the context's stream, as many blocks back;
// more: what the kernel reads or writes besides
template <class Launch>
int run_block_test(wrenc_gpu_ctx* ctx, const int16_t* in, int log2n, int count, int16_t* out, Launch launch, int nb = 1,
                   float* kernel_ms = nullptr, std::vector<TestBuf*> more = {}) {
    if (!ctx || !in || !out) return WRENC_GPU_EINVAL;
    if (log2n < 2 || log2n > 5 || count < 1 || nb < 1) return fail(ctx, WRENC_GPU_EINVAL, "log2n must be 2..5 and count >= 1");
    const size_t n = (size_t)count * nb << (2 * log2n);
    TestBuf d_in = buf_in(in, n), d_out = buf_out(out, n);
    more.insert(more.end(), {&d_in, &d_out});
    return run_on_stream(ctx, more, [&](hipStream_t) {
        launch(d_in.as<int16_t>(), d_out.as<int16_t>());
        return hipSuccess;
    }, kernel_ms);
}

// A picture of a test entry's own (never a slot of the context): up to two sets of three planes of the context's size, Y |
// Cb | Cr back to back like a slot's slabs, originals first; `host` holds the upload until the entry has synchronised.
TestBuf test_picture(const wrenc_gpu_config& c, const uint8_t* const org[3], const uint8_t* const rec[3], std::vector<uint8_t>& host) {
    for (const uint8_t* const* from : {org, rec})
        for (int comp = 0; from && comp < 3; ++comp) host.insert(host.end(), from[comp], from[comp] + plane_bytes(c, comp, 1));
    return buf_in(host.data(), host.size());
}
// ... and the PicBufs of it, once it has its device memory
PicBufs picture_bufs(const wrenc_gpu_config& c, const TestBuf& slab, bool org, bool rec) {
    PicBufs pb = {};
    uint8_t* at = slab.as<uint8_t>();
    for (int p = org ? 0 : 3; p < (rec ? 6 : 3); ++p) {
        if (p < 3) pb.org[p] = at; else pb.rec[p - 3] = at;
        at += plane_bytes(c, p % 3, 1);
    }
    return pb;
}

// the quantiser test entries' own overflow word (d_overflow[1]), read once the entry's kernel has finished and cleared
// again whatever `rc`, the entry's status so far, is: the call that raised it fails with WRENC_GPU_ELEVEL -- or with the
// earlier failure `rc` names --, and the next call on the context starts clean either way
// (include/wrenc_gpu.h: "keep a word of their own and never poison a context")
int take_test_overflow(wrenc_gpu_ctx* ctx, int rc) {
    int ovf = 0;
    hipError_t e = hipMemcpyAsync(&ovf, ctx->d_overflow.get() + 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream.get());
    if (e == hipSuccess) e = hipMemsetAsync(ctx->d_overflow.get() + 1, 0, sizeof(int), ctx->stream.get());
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream.get());
    if (rc != WRENC_GPU_OK) return rc;
    if (e != hipSuccess) return fail(ctx, WRENC_GPU_EHIP, hipGetErrorString(e));
    if (!ovf) return WRENC_GPU_OK;
    return fail(ctx, WRENC_GPU_ELEVEL, "a quantised level reached 1024 (reference panics: block_splitter.rs:453)");
}
} // namespace

extern "C" {

int wrenc_gpu_test_metrics(wrenc_gpu_ctx* ctx, const uint8_t* const org[3], const uint8_t* const rec[3], wrenc_gpu_metrics* out,
                           float* const ssim_map[3]) {
    if (!ctx || !org || !rec || !out) return WRENC_GPU_EINVAL;
    for (int p = 0; p < 3; ++p)
        if (!org[p] || !rec[p]) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_metrics: null plane");
    const wrenc_gpu_config& c = ctx->cfg;
    const MetPlane L = met_plane(c.width, c.height, 0), C = met_plane(c.width, c.height, 1);
    const size_t n_win = (size_t)L.windows + 2 * (size_t)C.windows;
    MetricsSums sums = {};
    std::vector<float> map(ssim_map ? n_win : 0);
    std::vector<uint8_t> host;
    PicBufs pb;
    TestBuf planes = test_picture(c, org, rec, host), pic = buf_out<PicBufs>(nullptr, 1), sum = buf_out(&sums, 1);
    TestBuf part = buf_out<MetricsPartial>(nullptr, (size_t)(L.waves + 2 * C.waves)), maps = buf_out(map.data(), map.size());
    const int rc = run_on_stream(ctx, {&planes, &pic, &part, &sum, &maps}, [&](hipStream_t st) {
        pb = picture_bufs(c, planes, true, true);
        const hipError_t e = hipMemcpyAsync(pic.d.get(), &pb, sizeof(pb), hipMemcpyHostToDevice, st);
        return e != hipSuccess ? e : launch_metrics(c, c.width, c.height, st, pic.as<PicBufs>(), 0, 1, part.as<MetricsPartial>(),
                                                    sum.as<MetricsSums>(), maps.as<float>());
    });
    if (rc) return rc;
    fill_metrics(c.width, c.height, sums, *out);
    if (ssim_map) {
        const size_t at[3] = {0, (size_t)L.windows, (size_t)L.windows + (size_t)C.windows};
        for (int p = 0; p < 3; ++p)
            if (ssim_map[p]) memcpy(ssim_map[p], map.data() + at[p], (size_t)(p ? C.windows : L.windows) * sizeof(float));
    }
    return WRENC_GPU_OK;
}

int wrenc_gpu_test_hash(wrenc_gpu_ctx* ctx, const uint8_t* const rec[3], int hash_type, wrenc_picture_hash* out) {
    if (!ctx || !rec || !out) return WRENC_GPU_EINVAL;
    if (hash_type != WRENC_HASH_MD5 && hash_type != WRENC_HASH_CRC && hash_type != WRENC_HASH_CHECKSUM)
        return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_hash: unknown hash type");
    for (int p = 0; p < 3; ++p)
        if (!rec[p]) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_hash: null plane");
    const wrenc_gpu_config& c = ctx->cfg;
    const auto tab = std::make_unique<HashTables>();
    hash_fill_tables(*tab);
    std::vector<uint8_t> host;
    PicBufs pb;
    TestBuf planes = test_picture(c, nullptr, rec, host), pic = buf_out<PicBufs>(nullptr, 1), tables = buf_in(tab.get(), 1);
    TestBuf part = buf_out<uint32_t>(nullptr, hash_partials(c)), values = buf_out(out, 1);
    return run_on_stream(ctx, {&planes, &pic, &tables, &part, &values}, [&](hipStream_t st) {
        pb = picture_bufs(c, planes, false, true);
        const hipError_t e = hipMemcpyAsync(pic.d.get(), &pb, sizeof(pb), hipMemcpyHostToDevice, st);
        return e != hipSuccess ? e : launch_hashes(c, st, pic.as<PicBufs>(), 0, 1, hash_type, tables.as<HashTables>(),
                                                   part.as<uint32_t>(), values.as<wrenc_picture_hash>());
    });
}

int wrenc_gpu_test_head_ranges(wrenc_gpu_ctx* ctx, int counts[4], int ranges[24]) {
    if (!ctx || !counts) return WRENC_GPU_EINVAL;
    TestBuf d = buf_out(counts, 4, true);
    const int rc = run_on_stream(ctx, {&d}, [&](hipStream_t st) {
        hipLaunchKernelGGL(test_head_ranges_kernel, dim3(1024, 8), dim3(64), 0, st, ctx->ctx_const(), d.as<int>());
        return hipSuccess;
    });
    if (rc == WRENC_GPU_OK && ranges) {
        const auto hk = std::make_unique<DevConst>();
        fill_dev_const(ctx->cfg, *hk);
        memcpy(ranges, hk->head_rng, sizeof(hk->head_rng));
    }
    return rc;
}

int wrenc_gpu_test_avail_tab(wrenc_gpu_ctx* ctx, int* differences) {
    if (!ctx || !differences) return WRENC_GPU_EINVAL;
    TestBuf d = buf_out(differences, 1, true);
    return run_on_stream(ctx, {&d}, [&](hipStream_t st) {
        hipLaunchKernelGGL(test_avail_tab_kernel, dim3(ctx->ctu_cols * ctx->ctu_rows, 4), dim3(64), 0, st, ctx->ctx_const(), d.as<int>());
        return hipSuccess;
    });
}

// ---- building-block entry points ----

// the 32x32 forward transform runs as i8 MFMAs on two base-256 digits of the residual (fwd_dct32_mfma): exact for
// |residual| <= 255, which is all the search can produce; the test entries refuse anything else
static bool residuals_fit_9_bits(const int16_t* res, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (res[i] < -255 || res[i] > 255) return false;
    return true;
}

// What the group entries refuse, before anything is allocated or launched: a group the device functions are not written
// for or that does not fit the wave's buffers (r1: 1024 i16 from o1 on; r2: the 1024 i16 of the scan-order or transposed
// blocks).  nb_max: 2 for the quantiser (a luma block or the Cb + Cr pair).  nullptr = fine.
static const char* group_shape_error(int log2n, int nb, int o1, int nb_max) {
    if (log2n < 2 || log2n > 5) return "log2n must be 2..5";
    if (nb < 1 || nb > nb_max) return "nb outside what the device function takes";
    if (log2n == 5 && nb > 1) return "a 32x32 block is always alone";
    if (o1 < 0 || (o1 & 1)) return "o1 must be even and >= 0";
    if ((nb << (2 * log2n)) > 1024) return "the group does not fit r2";
    if (o1 + (nb << (2 * log2n)) > 1024) return "the group does not fit r1 behind o1";
    return nullptr;
}
constexpr int kGroupMaxBlocks = 64; // (1024 / 16: group_shape_error's size rules are what bounds a transform group)

// The 8x8 and 16x16 transforms exist as i8 MFMAs too (fwd_dct_mfma / inv_dct_mfma; the search runs them at 16x16):
// 16-byte row reads, so o1 a multiple of 8, and for the forward transform |residual| <= 255.  The search has both by
// construction; a test group that has not runs the retained v_dot2 templates (the host decides before the launch: no
// data-dependent branch on the device).
static bool group_takes_mfma(const int16_t* res, int log2n, int nb, int o1, int count, bool inverse) {
    if (o1 & 7) return false;
    return inverse || count < 1 || residuals_fit_9_bits(res, (size_t)count * ((size_t)nb << (2 * log2n)));
}
// use_mfma: -1 = the plain entries: what the search runs at this size where the group meets its preconditions, else the
// v_dot2 templates; 0 = the v_dot2 templates; 1 = the MFMA versions, or EINVAL
static int run_dct_group(wrenc_gpu_ctx* ctx, const int16_t* in, int log2n, int nb, int o1, int count, int16_t* out,
                         int use_mfma, int reps, float* kernel_ms, bool inverse) {
    if (!ctx || !in || !out || reps < 1) return WRENC_GPU_EINVAL;
    if (const char* why = group_shape_error(log2n, nb, o1, kGroupMaxBlocks)) return fail(ctx, WRENC_GPU_EINVAL, why);
    if (!inverse && log2n == 5 && count >= 1 && !residuals_fit_9_bits(in, (size_t)count * 1024))
        return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_fwd_dct: a 32x32 residual lies outside +-255");
    int arm = DCT_SEARCH; // (4x4 and 32x32: nothing to choose)
    if (log2n == 3 || log2n == 4) {
        const bool takes = group_takes_mfma(in, log2n, nb, o1, count, inverse);
        if (use_mfma == 1 && !takes)
            return fail(ctx, WRENC_GPU_EINVAL, "the MFMA transforms take residuals within +-255 and an o1 that is a multiple of 8");
        arm = use_mfma == 1 ? DCT_MFMA : (use_mfma == 0 || !takes ? DCT_VDOT2 : DCT_SEARCH);
    }
    float ms = 0.f;
    const int rc = run_block_test(ctx, in, log2n, count, out, [&](int16_t* i, int16_t* o) {
        if (inverse)
            hipLaunchKernelGGL(test_inv_dct_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, log2n, nb, o1, o, arm, reps);
        else
            hipLaunchKernelGGL(test_fwd_dct_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, log2n, nb, o1, o, arm, reps);
    }, nb, kernel_ms ? &ms : nullptr);
    if (kernel_ms) *kernel_ms = ms;
    return rc;
}
int wrenc_gpu_test_fwd_dct_nb(wrenc_gpu_ctx* ctx, const int16_t* res, int log2n, int nb, int o1, int count, int16_t* coef) {
    return run_dct_group(ctx, res, log2n, nb, o1, count, coef, -1, 1, nullptr, false);
}
int wrenc_gpu_test_fwd_dct_mfma(wrenc_gpu_ctx* ctx, const int16_t* res, int log2n, int nb, int o1, int count, int16_t* coef,
                                int use_mfma, int reps, float* kernel_ms) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (log2n != 3 && log2n != 4) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_fwd_dct_mfma: log2n must be 3 or 4");
    return run_dct_group(ctx, res, log2n, nb, o1, count, coef, use_mfma ? 1 : 0, reps, kernel_ms, false);
}
int wrenc_gpu_test_inv_dct_mfma(wrenc_gpu_ctx* ctx, const int16_t* deq, int log2n, int nb, int o1, int count, int16_t* res,
                                int use_mfma, int reps, float* kernel_ms) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (log2n != 3 && log2n != 4) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_inv_dct_mfma: log2n must be 3 or 4");
    return run_dct_group(ctx, deq, log2n, nb, o1, count, res, use_mfma ? 1 : 0, reps, kernel_ms, true);
}
int wrenc_gpu_test_fwd_dct(wrenc_gpu_ctx* ctx, const int16_t* res, int log2n, int count, int16_t* coef) {
    return wrenc_gpu_test_fwd_dct_nb(ctx, res, log2n, 1, 0, count, coef);
}
// a 32x32 transform micro-benchmark: `count` blocks, `reps` repetitions each, HIP-event duration of the one kernel
static int run_dct32_bench(wrenc_gpu_ctx* ctx, const int16_t* in, int count, int16_t* out, int use_mfma, int reps,
                           float* kernel_ms, bool inverse) {
    if (!ctx || !in || !out || count < 1 || reps < 1) return WRENC_GPU_EINVAL;
    if (!inverse && use_mfma && !residuals_fit_9_bits(in, (size_t)count * 1024))
        return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_fwd_dct32: a residual lies outside +-255 (MFMA path)");
    float ms = 0.f;
    const int rc = run_block_test(ctx, in, 5, count, out, [&](int16_t* i, int16_t* o) {
        if (inverse)
            hipLaunchKernelGGL(test_inv_dct32_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, o, use_mfma, reps);
        else
            hipLaunchKernelGGL(test_fwd_dct32_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, o, use_mfma, reps);
    }, 1, &ms);
    if (kernel_ms) *kernel_ms = ms;
    return rc;
}
int wrenc_gpu_test_fwd_dct32(wrenc_gpu_ctx* ctx, const int16_t* res, int count, int16_t* coef, int use_mfma, int reps,
                             float* kernel_ms) {
    return run_dct32_bench(ctx, res, count, coef, use_mfma, reps, kernel_ms, false);
}
int wrenc_gpu_test_inv_dct32(wrenc_gpu_ctx* ctx, const int16_t* deq, int count, int16_t* res, int use_mfma, int reps,
                             float* kernel_ms) {
    return run_dct32_bench(ctx, deq, count, res, use_mfma, reps, kernel_ms, true);
}
int wrenc_gpu_test_inv_dct_nb(wrenc_gpu_ctx* ctx, const int16_t* deq, int log2n, int nb, int o1, int count, int16_t* res) {
    return run_dct_group(ctx, deq, log2n, nb, o1, count, res, -1, 1, nullptr, true);
}
int wrenc_gpu_test_inv_dct(wrenc_gpu_ctx* ctx, const int16_t* deq, int log2n, int count, int16_t* res) {
    return wrenc_gpu_test_inv_dct_nb(ctx, deq, log2n, 1, 0, count, res);
}
int wrenc_gpu_test_fwd_dct4_reg(wrenc_gpu_ctx* ctx, const int16_t* res, int count, int16_t* coef) {
    return run_block_test(ctx, res, 2, count, coef, [&](int16_t* i, int16_t* o) {
        hipLaunchKernelGGL(test_dct4_reg_kernel, dim3((count + 3) / 4), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, count, 0, o);
    });
}
int wrenc_gpu_test_inv_dct4_reg(wrenc_gpu_ctx* ctx, const int16_t* levels, int count, int16_t* res) {
    return run_block_test(ctx, levels, 2, count, res, [&](int16_t* i, int16_t* o) {
        hipLaunchKernelGGL(test_dct4_reg_kernel, dim3((count + 3) / 4), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, count, 1, o);
    });
}
int wrenc_gpu_test_dequantize_nb(wrenc_gpu_ctx* ctx, const int16_t* levels, int log2n, int nb, int o1, int count, int16_t* deq) {
    if (!ctx || !levels || !deq) return WRENC_GPU_EINVAL;
    if (const char* why = group_shape_error(log2n, nb, o1, kGroupMaxBlocks)) return fail(ctx, WRENC_GPU_EINVAL, why);
    return run_block_test(ctx, levels, log2n, count, deq, [&](int16_t* i, int16_t* o) {
        hipLaunchKernelGGL(test_dequantize_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, log2n, nb, o1, o);
    }, nb);
}
int wrenc_gpu_test_dequantize(wrenc_gpu_ctx* ctx, const int16_t* levels, int log2n, int count, int16_t* deq) {
    return wrenc_gpu_test_dequantize_nb(ctx, levels, log2n, 1, 0, count, deq);
}
// (any_level may be null: the one-block entry does not hand it on)
int wrenc_gpu_test_quantize_nb(wrenc_gpu_ctx* ctx, const int16_t* coef, int log2n, int nb, int count, int16_t* levels,
                               int64_t* level_cost, int32_t* any_level) {
    if (!ctx || !coef || !levels || !level_cost) return WRENC_GPU_EINVAL;
    if (const char* why = group_shape_error(log2n, nb, 0, 2)) return fail(ctx, WRENC_GPU_EINVAL, why);
    if (count < 1) return fail(ctx, WRENC_GPU_EINVAL, "count must be >= 1");
    TestBuf cost = buf_out(level_cost, (size_t)count), any = buf_out(any_level, (size_t)count);
    return take_test_overflow(ctx, run_block_test(ctx, coef, log2n, count, levels, [&](int16_t* i, int16_t* o) {
        hipLaunchKernelGGL(test_quantize_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, log2n, nb, o,
                           cost.as<long long>(), any.as<int>(), ctx->d_overflow.get() + 1);
    }, nb, nullptr, {&cost, &any}));
}
int wrenc_gpu_test_quantize(wrenc_gpu_ctx* ctx, const int16_t* coef, int log2n, int count, int16_t* levels,
                            int64_t* level_cost) {
    return wrenc_gpu_test_quantize_nb(ctx, coef, log2n, 1, count, levels, level_cost, nullptr);
}

int wrenc_gpu_test_quantize_p16(wrenc_gpu_ctx* ctx, const int16_t* coef, int count, int16_t* levels, int64_t* level_cost) {
    if (!ctx || !level_cost) return WRENC_GPU_EINVAL;
    if (count < 1) return fail(ctx, WRENC_GPU_EINVAL, "count must be >= 1");
    TestBuf cost = buf_out(level_cost, (size_t)count);
    return take_test_overflow(ctx, run_block_test(ctx, coef, 2, count, levels, [&](int16_t* i, int16_t* o) {
        hipLaunchKernelGGL(test_quantize_p16_kernel, dim3((count + 3) / 4), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, count, o,
                           cost.as<long long>(), ctx->d_overflow.get() + 1);
    }, 1, nullptr, {&cost}));
}

int wrenc_gpu_test_quantize_pk(wrenc_gpu_ctx* ctx, const int16_t* coef, int log2n, int nc, int n_packs, int16_t* levels,
                               int64_t* level_cost) {
    if (!ctx || !coef || !levels || !level_cost) return WRENC_GPU_EINVAL;
    if (!((log2n == 3 && nc >= 1 && nc <= 3) || (log2n == 4 && nc >= 1 && nc <= 2)) || n_packs < 1)
        return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_quantize_pk: log2n 3 with nc 1..3 or log2n 4 with nc 1..2");
    const size_t total = (size_t)n_packs * nc * 3 * ((size_t)1 << (2 * log2n)) / 2;
    TestBuf in = buf_in(coef, total), out = buf_out(levels, total), cost = buf_out(level_cost, (size_t)2 * nc * n_packs);
    return take_test_overflow(ctx, run_on_stream(ctx, {&in, &out, &cost}, [&](hipStream_t st) {
        hipLaunchKernelGGL(test_quantize_pk_kernel, dim3(n_packs), dim3(64), 0, st, ctx->ctx_const(), in.as<int16_t>(), log2n, nc,
                           out.as<int16_t>(), cost.as<long long>(), ctx->d_overflow.get() + 1);
        return hipSuccess;
    }));
}

int wrenc_gpu_test_recon_rows(wrenc_gpu_ctx* ctx, const uint8_t* pred, const int16_t* res, const uint8_t* org, int count,
                              uint8_t* rec, uint32_t* ssd) {
    if (!ctx || !pred || !res || !org || !rec || !ssd) return WRENC_GPU_EINVAL;
    if (count < 1) return fail(ctx, WRENC_GPU_EINVAL, "count must be >= 1");
    const size_t n = (size_t)count * 4;
    TestBuf d_pred = buf_in(pred, n), d_res = buf_in(res, n), d_org = buf_in(org, n), d_rec = buf_out(rec, n),
            d_ssd = buf_out(ssd, (size_t)count);
    return run_on_stream(ctx, {&d_pred, &d_res, &d_org, &d_rec, &d_ssd}, [&](hipStream_t st) {
        hipLaunchKernelGGL(test_recon_rows_kernel, dim3((count + 63) / 64), dim3(64), 0, st, d_pred.as<uint32_t>(), d_res.as<uint2>(),
                           d_org.as<uint32_t>(), count, d_rec.as<uint32_t>(), d_ssd.as<uint32_t>());
        return hipSuccess;
    });
}

int wrenc_gpu_test_predict_layout(int width, int height, int n_items, const int32_t* items, size_t* offsets) {
    if (!items || !offsets || n_items < 1) return WRENC_GPU_EINVAL;
    return predict_items_layout(width, height, n_items, items, offsets) < 0 ? WRENC_GPU_OK : WRENC_GPU_EINVAL;
}

int wrenc_gpu_test_predict(wrenc_gpu_ctx* ctx, const uint8_t* rec_y, const uint8_t* rec_cb, const uint8_t* rec_cr,
                           int n_items, const int32_t* items, uint8_t* out, size_t out_bytes) {
    if (!ctx || !rec_y || !rec_cb || !rec_cr || !items || !out || n_items < 1) return WRENC_GPU_EINVAL;
    const wrenc_gpu_config& c = ctx->cfg;
    // operand shapes are checked on the host (predict_items.h): a bad item must never reach the kernel
    std::vector<size_t> at((size_t)n_items + 1);
    if (predict_items_layout(c.width, c.height, n_items, items, at.data()) >= 0)
        return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_predict: bad item");
    if (at[n_items] != out_bytes) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_predict: output size does not match the items");
    std::vector<int> dev_items; // the kernel's: the item, then its output offset
    for (int i = 0; i < n_items; ++i) {
        dev_items.insert(dev_items.end(), items + kPredictItemInts * i, items + kPredictItemInts * (i + 1));
        dev_items.push_back((int)at[i]);
    }
    const uint8_t* const rec[3] = {rec_y, rec_cb, rec_cr};
    std::vector<uint8_t> host;
    TestBuf planes = test_picture(c, nullptr, rec, host), its = buf_in(dev_items.data(), dev_items.size());
    TestBuf scratch = buf_out<uint8_t>(nullptr, (size_t)n_items * kTestPredictScratch), res = buf_out(out, out_bytes);
    return run_on_stream(ctx, {&planes, &its, &scratch, &res}, [&](hipStream_t st) {
        hipLaunchKernelGGL(test_predict_kernel, dim3(n_items), dim3(64), 0, st, ctx->ctx_const(), planes.as<uint8_t>(), its.as<int>(),
                           scratch.as<uint8_t>(), res.as<uint8_t>());
        return hipSuccess;
    });
}

int wrenc_gpu_test_const_field(const wrenc_gpu_config* cfg, const char* name, void* out, size_t cap) {
    if (!cfg || !name || !out) return WRENC_GPU_EINVAL;
    if (!rate_model_fits(*cfg)) return WRENC_GPU_EINVAL; // (as wrenc_gpu_create: fill_dev_const multiplies lambda_q and dq_table)
#define CONST_FIELD(m) {#m, offsetof(DevConst, m), sizeof(DevConst::m)}
    static const struct { const char* name; size_t at, bytes; } fields[] = {
        CONST_FIELD(W), CONST_FIELD(H), CONST_FIELD(qp), CONST_FIELD(max_depth), CONST_FIELD(ctu_cols), CONST_FIELD(ctu_rows),
        CONST_FIELD(lsc), CONST_FIELD(div_magic), CONST_FIELD(div_shift), CONST_FIELD(lambda_q), CONST_FIELD(lambda_rd),
        CONST_FIELD(lambda_rd_chroma), CONST_FIELD(ldq), CONST_FIELD(lv), CONST_FIELD(hb_luma), CONST_FIELD(hb_chroma),
        CONST_FIELD(dct), CONST_FIELD(dct_t), CONST_FIELD(diag4), CONST_FIELD(diag_sb), CONST_FIELD(scan_idx),
        CONST_FIELD(intra_angle), CONST_FIELD(ang_tab), CONST_FIELD(fc), CONST_FIELD(dct32_a), CONST_FIELD(dct32_p),
        CONST_FIELD(idct32_b), CONST_FIELD(idct32_p), CONST_FIELD(idct32_k1), CONST_FIELD(idct32_k2), CONST_FIELD(fdct_b),
        CONST_FIELD(fdct16_p), CONST_FIELD(fdct8_p), CONST_FIELD(idct_b), CONST_FIELD(idct16_p), CONST_FIELD(idct8_p),
        CONST_FIELD(idct_k1), CONST_FIELD(idct16_k2), CONST_FIELD(idct8_k2), CONST_FIELD(head_rng), CONST_FIELD(avail_tab),
        CONST_FIELD(split_floor), CONST_FIELD(cand_floor), CONST_FIELD(cand_floor_ang),
    };
#undef CONST_FIELD
    for (const auto& f : fields) {
        if (strcmp(name, f.name)) continue;
        if (cap < f.bytes) return WRENC_GPU_EINVAL;
        std::unique_ptr<DevConst> hk(new (std::nothrow) DevConst());
        if (!hk) return WRENC_GPU_ENOMEM;
        fill_dev_const(*cfg, *hk);
        memcpy(out, (const char*)hk.get() + f.at, f.bytes);
        return (int)f.bytes;
    }
    return WRENC_GPU_EINVAL;
}

} // extern "C"
