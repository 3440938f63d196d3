// dev_distcurve.h -- the distortion curve of a picture from its uploaded originals alone (include/wrenc_gpu.h:
// wrenc_gpu_download_dist_curve; the definition, in exact integers, is include/wrenc_distcurve.h): the coefficients of
// dev_ratecurve.h (per picture-aligned 8x8 block of every plane the best of DC, V and H from the neighbours' originals, the
// unnormalised Hadamard transform of the residual), each quantised at every QP 0 .. 63, and per plane and QP the sum of
// the squared quantisation errors.  All integers, all exact.
//
// Layout: dev_ratecurve.h's, and its code up to the coefficients (rh_load, rh_coefficients).  A wave is a strip of 16 CTUs of
// one CTU row; a lane owns two blocks at a time, one in each 16-bit half of its registers, through prediction and
// butterflies.
// The QP loop is the new part and all of the time: 64 quantise-and-square steps per coefficient, four instructions each
// (distcurve_quant.h: two v_fma_f32 -- packed, two steps an instruction --, v_trunc_f32, v_cvt_i32_f32 and a 24-bit
// multiply-add), every step's T, 1 / T and rounding offset literals.
// For the 64 sums of a plane to stay in registers (128 VGPRs as 64-bit pairs) the loop over QPs is unrolled and the loop
// over coefficients is not, so the 64 packed magnitudes of a lane's pair wait in LDS, one column of dwords per lane (a
// lane reads back only what it wrote: no barrier, no bank conflict), and come back kDcFold at a time: that many e e fit a
// 32-bit partial, which is then added to the QP's 64-bit sum (two more instructions per kDcFold steps).  The two halves
// of a pair are two passes over the column, so that one set of sums serves luma (both halves one plane) and chroma (Cb,
// then Cr).
// After a pass the wave adds its lanes' sums up by a butterfly of ds_bpermute (768 per pass against 16,384 steps) and lane q
// keeps the total of QP q; a wave stores its 3 x 64 totals at its own index and dist_curve_finish_kernel adds a picture's
// waves in index order: no global atomics, the same table in any slot, batch and run.
// 16 KiB of LDS a wave, two waves a workgroup.
#pragma once

#include "distcurve_quant.h"

#include <utility>

namespace wrenc {

constexpr int kDcQps = 64;  // WRENC_DISTCURVE_QPS
constexpr int kDcWaves = 2; // of a workgroup
// e e < 2^30 (include/wrenc_distcurve.h: |e| <= 29,184), so a 32-bit partial holds four of them
constexpr int kDcFold = 4;
static_assert((unsigned long long)kDcFold * ((1ull << 30) - 1) < (1ull << 32), "a partial of kDcFold squared errors fits 32 bits");
static_assert(64 % kDcFold == 0, "a block's coefficients come in whole folds");

struct DistCurveSums { // one wave, or one picture: wrenc_dist_curve
    unsigned long long sse8[3][kDcQps];
};

template <int... Q>
__device__ __forceinline__ void dc_fold(const float (&mf)[kDcFold], unsigned long long (&acc)[kDcQps], std::integer_sequence<int, Q...>) {
    static_assert(kDcFold == 4, "the partial below is written out");
    ((acc[Q] += (unsigned long long)(dq_error2<Q>(mf[0]) + dq_error2<Q>(mf[1]) + dq_error2<Q>(mf[2]) + dq_error2<Q>(mf[3]))), ...);
}

// One half (shift 0: block a, 16: block b) of the lane's 64 packed magnitudes mags[64 i], added to acc at every QP.
__device__ __forceinline__ void dc_accumulate(const uint32_t* mags, int shift, unsigned long long (&acc)[kDcQps]) {
#pragma unroll 1
    for (int i = 0; i < 64; i += kDcFold) {
        float mf[kDcFold]; // m = 8 |c|
#pragma unroll
        for (int k = 0; k < kDcFold; ++k) mf[k] = (float)(((mags[64 * (i + k)] >> shift) & 0xFFFFu) << 3);
        dc_fold(mf, acc, std::make_integer_sequence<int, kDcQps>());
    }
}

// The wave's total of every QP (lanes that own nothing add nothing); lane q returns QP q's.
__device__ __forceinline__ unsigned long long dc_wave_sums(const unsigned long long (&acc)[kDcQps], bool own, int lane) {
    unsigned long long mine = 0;
#pragma unroll
    for (int q = 0; q < kDcQps; ++q) {
        unsigned long long s = own ? acc[q] : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == q) mine = s;
    }
    return mine;
}

// The curves of blocks a (low halves) and b (high halves), summed over the wave: lane q gets QP q's in sum_a and sum_b.
// mags: the lane's column of the wave's LDS.
__device__ __forceinline__ void dc_pair(const RhBlock& a, const RhBlock& b, bool top_a, bool top_b, bool has_left, bool own, uint32_t* mags,
                                        int lane, unsigned long long& sum_a, unsigned long long& sum_b) {
    {
        Pk16 v[64];
        rh_coefficients(a, b, top_a, top_b, has_left, v);
#pragma unroll
        for (int i = 0; i < 64; ++i) mags[64 * i] = __builtin_bit_cast(uint32_t, __builtin_elementwise_abs(v[i]));
    }
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        unsigned long long acc[kDcQps];
#pragma unroll
        for (int q = 0; q < kDcQps; ++q) acc[q] = 0;
        dc_accumulate(mags, 16 * half, acc);
        const unsigned long long s = dc_wave_sums(acc, own, lane);
        if (half == 0)
            sum_a = s;
        else
            sum_b = s;
    }
}

// One wave per (picture, CTU row, strip of kCplxCtus CTUs): cplx_waves(W, H) waves a picture, kDcWaves a workgroup.
__global__ __launch_bounds__(64 * kDcWaves) void dist_curve_kernel(const PicBufs* __restrict__ slots, int first_slot, int n_pics, int W, int H,
                                                                   DistCurveSums* __restrict__ partials) {
    __shared__ uint32_t lds[kDcWaves][64][64]; // [wave][coefficient][lane]
    const int strips = cplx_strips(W), per_pic = cplx_waves(W, H), total = n_pics * per_pic;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int at = uni((int)(blockIdx.x * kDcWaves) + wave);
    const bool live = at < total;         // (the whole wave) a wave past the last strip does the last one again and stores nothing
    const int id = live ? at : total - 1;
    const int pic = id / per_pic, rem = id - pic * per_pic;
    const int ctu_y = rem / strips, strip = rem - ctu_y * strips;
    const PicBufs& pb = slots[first_slot + pic];
    const uint8_t* org_y = pb.org[0];
    const uint8_t* org_cb = pb.org[1];
    const uint8_t* org_cr = pb.org[2];
    const int cw = W >> 1;
    uint32_t* mags = &lds[wave][0][lane];

    { // luma: lane = block column of the strip; block rows 0 | 1, then 2 | 3 of the CTU row
        const int bx = strip * (4 * kCplxCtus) + lane;
        const bool own = live && bx < (W >> 3);
        const int x = min(bx, (W >> 3) - 1);
        const uint8_t* p = org_y + (size_t)(32 * ctu_y) * W + 8 * x;
        unsigned long long sum = 0;
#pragma unroll 1
        for (int round = 0; round < 2; ++round) {
            const uint8_t* pa = p + (size_t)(16 * round) * W;
            const bool top_a = ctu_y > 0 || round > 0;
            RhBlock a, b;
            rh_load(a, pa, W, top_a, x > 0);
            rh_load(b, pa + (size_t)8 * W, W, true, x > 0);
            unsigned long long sum_a, sum_b;
            dc_pair(a, b, top_a, true, x > 0, own, mags, lane, sum_a, sum_b);
            sum += sum_a + sum_b;
        }
        if (live) partials[id].sse8[0][lane] = sum;
    }
    { // chroma: lane & 31 = block column, lane >> 5 = block row of the CTU row; Cb | Cr
        const int cx = strip * (2 * kCplxCtus) + (lane & 31);
        const bool own = live && cx < (W >> 4);
        const int x = min(cx, (W >> 4) - 1), by = 2 * ctu_y + (lane >> 5);
        const size_t c_at = (size_t)(8 * by) * cw + 8 * x;
        RhBlock a, b;
        rh_load(a, org_cb + c_at, cw, by > 0, x > 0);
        rh_load(b, org_cr + c_at, cw, by > 0, x > 0);
        unsigned long long sum_cb, sum_cr;
        dc_pair(a, b, by > 0, by > 0, x > 0, own, mags, lane, sum_cb, sum_cr);
        if (live) {
            partials[id].sse8[1][lane] = sum_cb;
            partials[id].sse8[2][lane] = sum_cr;
        }
    }
}

// A picture's waves added up in index order, one thread per (plane, QP).
__global__ __launch_bounds__(192) void dist_curve_finish_kernel(const DistCurveSums* __restrict__ partials, int W, int H,
                                                               DistCurveSums* __restrict__ sums) {
    const int t = (int)threadIdx.x;
    if (t >= 3 * kDcQps) return;
    const int count = cplx_waves(W, H);
    const DistCurveSums* p = partials + (size_t)blockIdx.x * count;
    unsigned long long s = 0;
    for (int i = 0; i < count; ++i) s += p[i].sse8[t / kDcQps][t % kDcQps];
    sums[blockIdx.x].sse8[t / kDcQps][t % kDcQps] = s;
}

} // namespace wrenc
