// dev_ratecurve.h -- the rate histogram of a picture from its uploaded originals alone (include/wrenc_gpu.h:
// wrenc_gpu_download_rate_hist; the definition, in exact integers, is include/wrenc_ratecurve.h): per picture-aligned 8x8
// block of every plane the best of the DC, V and H predictions from the neighbours' ORIGINALS by SAD, the unnormalised
// 2-D Hadamard transform of the residual, DC included, and per plane the number of coefficients in each log-magnitude
// bin.  All integers, all exact.
//
// Layout: dev_complexity.h's.  A wave is a strip of 16 CTUs of one CTU row; a lane owns TWO blocks at a time, one in each
// 16-bit half of its registers (luma: the block and the one below it, two rounds; chroma: the Cb and the Cr block at one
// position), so that the residual and all six butterfly stages are v_pk_sub_i16 / v_pk_add_i16 (|coefficient| <= 64 x 255).
// Per block a lane loads its eight rows (8 bytes each), the row above (8 bytes) and the column to the left (8 single
// bytes, lines the neighbouring lane's rows fetch anyway); a block on the plane's top row or left column reads its own
// first row / column instead and never uses it.  The three SADs are v_sad_u8 on the bytes as loaded, four samples an
// instruction.  Lanes beyond the plane's last block read that block again and own nothing.
// Counting.  bin = (bits of (float)m >> 21) - 507: the exponent and the two mantissa bits below the leading one, m exact in
// a float.  Real content puts most coefficients into a few low bins, where one LDS counter per bin would serialise the
// wave; so a lane counts its zeros in a register and adds them once per plane, and a wave keeps 16 sub-histograms per
// plane in LDS (counter [plane][bin][lane & 15]: at most 4 lanes meet on one ds_add_u32, and the 16 counters of a bin lie
// in 16 banks).  (A ballot + popcount per coefficient into a scalar was tried first: 128 ballots per pair spilled 351
// SGPRs.)
// 12 KiB a wave, 48 KiB a workgroup: the kernel shares no workgroup with the search.  A wave adds its sub-histograms up
// and stores its 3 x 64 counts at its own index; rate_hist_finish_kernel adds a picture's waves in index order: no global
// atomics, the same figures in any slot, batch and run.
#pragma once

namespace wrenc {

constexpr int kRhBins = 64; // WRENC_RATECURVE_BINS
constexpr int kRhSub = 16;  // sub-histograms of a wave

struct RateHistPartial { // one wave
    uint32_t count[3][kRhBins];
};
struct RateHistCounts { // one picture: wrenc_rate_hist
    unsigned long long count[3][kRhBins];
};

__device__ __forceinline__ uint32_t rh_sad8(Dwords2 a, uint32_t b0, uint32_t b1, uint32_t acc) {
    return __builtin_amdgcn_sad_u8(a[1], b1, __builtin_amdgcn_sad_u8(a[0], b0, acc));
}

struct RhBlock { // one block: its rows, the row above and the column to the left (one sample a word)
    Dwords2 s[8], top;
    uint32_t left[8];
};
// p: the block's first sample; has_top / has_left: whether the plane has the neighbours
__device__ __forceinline__ void rh_load(RhBlock& b, const uint8_t* p, int pitch, bool has_top, bool has_left) {
    const uint8_t* pt = has_top ? p - pitch : p;
    const uint8_t* pl = has_left ? p - 1 : p;
    b.top = *(GlobalRow8)pt;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        b.s[y] = *(GlobalRow8)(p + (size_t)y * pitch);
        b.left[y] = pl[(size_t)y * pitch];
    }
}

// the winning prediction as rows of 8 bytes (wrenc_ratecurve_predict)
__device__ __forceinline__ void rh_predict(const RhBlock& b, bool has_top, bool has_left, Dwords2 pred[8]) {
    const uint32_t sum_t = rh_sad8(b.top, 0u, 0u, 0u);
    uint32_t sum_l = 0;
#pragma unroll
    for (int y = 0; y < 8; ++y) sum_l += b.left[y];
    const uint32_t dc = has_top && has_left ? (sum_t + sum_l + 8) >> 4 : (has_top ? (sum_t + 4) >> 3 : (has_left ? (sum_l + 4) >> 3 : 128u));
    const uint32_t dc4 = dc * 0x01010101u;
    uint32_t sad_dc = 0, sad_v = 0, sad_h = 0;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const uint32_t l4 = b.left[y] * 0x01010101u;
        sad_dc = rh_sad8(b.s[y], dc4, dc4, sad_dc);
        sad_v = rh_sad8(b.s[y], b.top[0], b.top[1], sad_v);
        sad_h = rh_sad8(b.s[y], l4, l4, sad_h);
    }
    int best = 0; // DC, V, H: a later one wins only with a strictly smaller SAD
    uint32_t least = sad_dc;
    if (has_top && sad_v < least) {
        best = 1;
        least = sad_v;
    }
    if (has_left && sad_h < least) best = 2;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const uint32_t l4 = b.left[y] * 0x01010101u;
        pred[y][0] = best == 0 ? dc4 : (best == 1 ? b.top[0] : l4);
        pred[y][1] = best == 0 ? dc4 : (best == 1 ? b.top[1] : l4);
    }
}

// The coefficients of blocks a (low halves) and b (high halves): wrenc_ratecurve_block of each (dev_distcurve.h starts
// from them too)
__device__ __forceinline__ void rh_coefficients(const RhBlock& a, const RhBlock& b, bool top_a, bool top_b, bool has_left, Pk16 v[64]) {
    Dwords2 pa[8], pb[8];
    rh_predict(a, top_a, has_left, pa);
    rh_predict(b, top_b, has_left, pb);
#pragma unroll
    for (int y = 0; y < 8; ++y)
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            // [a's byte, 0, b's byte, 0]
            const uint32_t sel = 0x0c040c00u | (uint32_t)(x & 3) << 16 | (uint32_t)(x & 3);
            v[8 * y + x] = __builtin_bit_cast(Pk16, __builtin_amdgcn_perm(b.s[y][x >> 2], a.s[y][x >> 2], sel)) -
                           __builtin_bit_cast(Pk16, __builtin_amdgcn_perm(pb[y][x >> 2], pa[y][x >> 2], sel));
        }
#pragma unroll
    for (int h = 1; h < 64; h <<= 1)
#pragma unroll
        for (int i = 0; i < 64; ++i)
            if (!(i & h)) {
                const Pk16 p = v[i], q = v[i | h];
                v[i] = p + q;
                v[i | h] = p - q;
            }
}

// The coefficients of blocks a and b counted into the wave's sub-histograms hist_a / hist_b (already at the lane's column)
// and, the zeros, into the lane's zeros_a / zeros_b.
__device__ __forceinline__ void rh_pair(const RhBlock& a, const RhBlock& b, bool top_a, bool top_b, bool has_left, bool own,
                                        uint32_t* hist_a, uint32_t* hist_b, uint32_t& zeros_a, uint32_t& zeros_b) {
    Pk16 v[64];
    rh_coefficients(a, b, top_a, top_b, has_left, v);
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const uint32_t w = __builtin_bit_cast(uint32_t, __builtin_elementwise_abs(v[i]));
        const uint32_t ma = w & 0xFFFFu, mb = w >> 16;
        zeros_a += ma == 0 ? 1u : 0u;
        zeros_b += mb == 0 ? 1u : 0u;
        const uint32_t bin_a = min((__float_as_uint((float)ma) >> 21) - 507u, (uint32_t)(kRhBins - 1));
        const uint32_t bin_b = min((__float_as_uint((float)mb) >> 21) - 507u, (uint32_t)(kRhBins - 1));
        if (own && ma != 0) atomicAdd(hist_a + bin_a * kRhSub, 1u);
        if (own && mb != 0) atomicAdd(hist_b + bin_b * kRhSub, 1u);
    }
}

// One wave per (picture, CTU row, strip of kCplxCtus CTUs): cplx_waves(W, H) waves a picture, four a workgroup.
__global__ __launch_bounds__(256) void rate_hist_kernel(const PicBufs* __restrict__ slots, int first_slot, int n_pics, int W, int H,
                                                        RateHistPartial* __restrict__ partials) {
    __shared__ uint32_t lds[4][3][kRhBins][kRhSub];
    const int strips = cplx_strips(W), per_pic = cplx_waves(W, H), total = n_pics * per_pic;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int at = uni((int)(blockIdx.x * 4) + wave);
    const bool live = at < total;         // (the whole wave) a wave past the last strip does the last one again and stores nothing
    const int id = live ? at : total - 1;
    const int pic = id / per_pic, rem = id - pic * per_pic;
    const int ctu_y = rem / strips, strip = rem - ctu_y * strips;
    const PicBufs& pb = slots[first_slot + pic];
    const uint8_t* org_y = pb.org[0];
    const uint8_t* org_cb = pb.org[1];
    const uint8_t* org_cr = pb.org[2];
    const int cw = W >> 1;

    uint32_t* mine = &lds[wave][0][0][0];
    for (int i = lane; i < 3 * kRhBins * kRhSub; i += 64) mine[i] = 0u;
    __syncthreads();
    uint32_t* col = mine + (lane & (kRhSub - 1));
    uint32_t zeros[3] = {0u, 0u, 0u};

    { // luma: lane = block column of the strip; block rows 0 | 1, then 2 | 3 of the CTU row
        const int bx = strip * (4 * kCplxCtus) + lane;
        const bool own = live && bx < (W >> 3);
        const int x = min(bx, (W >> 3) - 1);
        const uint8_t* p = org_y + (size_t)(32 * ctu_y) * W + 8 * x;
#pragma unroll 1
        for (int round = 0; round < 2; ++round) {
            const uint8_t* pa = p + (size_t)(16 * round) * W;
            const bool top_a = ctu_y > 0 || round > 0;
            RhBlock a, b;
            rh_load(a, pa, W, top_a, x > 0);
            rh_load(b, pa + (size_t)8 * W, W, true, x > 0);
            rh_pair(a, b, top_a, true, x > 0, own, col, col, zeros[0], zeros[0]);
        }
        if (own) atomicAdd(col, zeros[0]);
    }
    { // chroma: lane & 31 = block column, lane >> 5 = block row of the CTU row; Cb | Cr
        const int cx = strip * (2 * kCplxCtus) + (lane & 31);
        const bool own = live && cx < (W >> 4);
        const int x = min(cx, (W >> 4) - 1), by = 2 * ctu_y + (lane >> 5);
        const size_t c_at = (size_t)(8 * by) * cw + 8 * x;
        RhBlock a, b;
        rh_load(a, org_cb + c_at, cw, by > 0, x > 0);
        rh_load(b, org_cr + c_at, cw, by > 0, x > 0);
        rh_pair(a, b, by > 0, by > 0, x > 0, own, col + kRhBins * kRhSub, col + 2 * kRhBins * kRhSub, zeros[1], zeros[2]);
        if (own) {
            atomicAdd(col + kRhBins * kRhSub, zeros[1]);
            atomicAdd(col + 2 * kRhBins * kRhSub, zeros[2]);
        }
    }
    __syncthreads();
    // the wave's 3 x 64 counts: three (plane, bin) entries a lane, each the sum of its 16 sub-counters
    if (live) {
#pragma unroll
        for (int plane = 0; plane < 3; ++plane) {
            const uint32_t* c = mine + (plane * kRhBins + lane) * kRhSub;
            uint32_t s = 0;
#pragma unroll
            for (int k = 0; k < kRhSub; ++k) s += c[(k + lane) & (kRhSub - 1)]; // (rotated: 16 banks, not 2)
            partials[id].count[plane][lane] = s;
        }
    }
}

// A picture's waves added up in index order, one thread per (plane, bin).
__global__ __launch_bounds__(192) void rate_hist_finish_kernel(const RateHistPartial* __restrict__ partials, int W, int H,
                                                              RateHistCounts* __restrict__ sums) {
    const int t = (int)threadIdx.x;
    if (t >= 3 * kRhBins) return;
    const int count = cplx_waves(W, H);
    const RateHistPartial* p = partials + (size_t)blockIdx.x * count;
    unsigned long long s = 0;
    for (int i = 0; i < count; ++i) s += p[i].count[t / kRhBins][t % kRhBins];
    sums[blockIdx.x].count[t / kRhBins][t % kRhBins] = s;
}

} // namespace wrenc
