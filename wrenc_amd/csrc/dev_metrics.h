// dev_metrics.h -- PSNR / SSIM sums of (original, reconstruction) on the device (include/wrenc_gpu.h:
// wrenc_gpu_download_metrics).  The arithmetic is ffmpeg's vf_ssim.c / vf_psnr.c for 8-bit planes as
// wrenc_amd/metrics.py restates it: 4x4 block sums s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b; a
// window is 2x2 blocks, windows one block apart; the window's value is an f32 quotient of integer expressions; the
// plane's squared error is sum (ss - 2 s12).
//
// Layout.  A lane owns a GROUP of four 4x4 blocks side by side: per sample row one 16-byte load of the original and one
// of the reconstruction, contiguous across the wave (1 KiB per load instruction), so a block row costs a lane eight
// global_load_dwordx4.  The block sums come from v_dot4_u32_u8 on the packed bytes (five per dword pair).  A wave is a
// STRIP of 64 groups (1024 samples) that walks down kMetRows block rows: the pair sums of the block row above stay in
// registers, the right neighbour's first block comes over DPP (wave_shl:1), nothing goes through LDS.  Lane 63 of a strip
// is the same group as lane 0 of the next one (it only hands its first block to lane 62), and the last block row of a
// wave is the first one of the wave below: those are the only samples read twice, and the four waves of a workgroup
// are neighbours in one strip, so the second read of a row is a cache hit.
// Every wave leaves one {squared error, sum of window values} pair in a scratch array at its own index and
// metrics_finish_kernel adds a plane's pairs in index order: no atomics, the same bits in any slot and batch.
//
// Window (WIN; a context with a visible size, wrenc_gpu_set_visible_size): the planes keep the coded pitch and the pass
// measures their top-left vw x vh rectangle, any even size: a chroma plane may be 17 wide.  The dealing is the same with
// the plane's last group and last block row possibly partial: the 16-byte loads stay inside the coded plane (its pitch is
// a multiple of 16, its height of 16), samples outside the rectangle are masked to zero in both pictures before the dot
// products -- they add nothing to the squared error -- and a window counts only where its four blocks are whole.  On a
// rectangle whose sides are multiples of 16 and 4 the masks are all ones and the sums are those of the plain pass.
#pragma once

namespace wrenc {

constexpr int kMetRows = 16;       // window rows (= block rows it owns) per wave; part of the summation order: do not tune per call
constexpr int kMetStripLanes = 63; // lanes of a strip that own blocks and windows

struct MetricsPartial {
    unsigned long long sse;
    double ssim;
};
struct MetricsSums { // per picture: Y, Cb, Cr
    unsigned long long sse[3];
    double ssim[3];
};

// how a plane (chroma = 0 luma, 1 Cb / Cr) of a W x H picture is dealt to waves (W x H: the size that is measured, whole
// CTUs or a visible size; the last group and the last block row of a plane may be partial)
struct MetPlane {
    int pw, ph;    // samples
    int groups;    // 16-sample column groups
    int brows;     // 4-sample block rows
    int strips, segs, waves;
    int windows;   // (pw / 4 - 1)(ph / 4 - 1)
};
__host__ __device__ inline MetPlane met_plane(int W, int H, int chroma) {
    MetPlane m;
    m.pw = W >> chroma;
    m.ph = H >> chroma;
    m.groups = (m.pw + 15) >> 4;
    m.brows = (m.ph + 3) >> 2;
    m.strips = (m.groups + kMetStripLanes - 1) / kMetStripLanes;
    m.segs = (m.brows - 1 + kMetRows - 1) / kMetRows;
    m.waves = m.strips * m.segs;
    m.windows = ((m.pw >> 2) - 1) * ((m.ph >> 2) - 1);
    return m;
}

struct BlockSums {
    uint32_t s1, s2, ss, s12;
};
__device__ __forceinline__ BlockSums operator+(const BlockSums& a, const BlockSums& b) {
    return BlockSums{a.s1 + b.s1, a.s2 + b.s2, a.ss + b.ss, a.s12 + b.s12};
}

// what lane + 1 holds (lane 63: 0)
__device__ __forceinline__ uint32_t from_right_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, false); // wave_shl:1
}

// vf_ssim.c ssim_end1 on the sums of one window.  Every integer fits 32 bits (64 ss <= 532,684,800); the four
// conversions, the two products and the quotient are f32 operations rounded one by one (-ffp-contract=off).
__device__ __forceinline__ float ssim_window(const BlockSums& w) {
    const int s1 = (int)w.s1, s2 = (int)w.s2;
    const int vars = (int)w.ss * 64 - s1 * s1 - s2 * s2;
    const int covar = (int)w.s12 * 64 - s1 * s2;
    const float num = (float)(2 * s1 * s2 + 416) * (float)(2 * covar + 235963);
    const float den = (float)(s1 * s1 + s2 * s2 + 416) * (float)(vars + 235963);
    return __fdiv_rn(num, den);
}

// the 4 x 16 samples of a lane's group in one block row, both pictures
typedef uint32_t Dwords4 __attribute__((ext_vector_type(4)));
struct GroupRows {
    Dwords4 a[4], b[4];
};
typedef const __attribute__((address_space(1))) Dwords4* GlobalRow; // (a plane pointer read from PicBufs would give flat loads)
__device__ __forceinline__ void load_group_rows(GroupRows& g, const uint8_t* org, const uint8_t* rec, size_t at, int pw) { // pw: the planes' pitch
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        g.a[r] = *(GlobalRow)(org + at + (size_t)r * pw);
        g.b[r] = *(GlobalRow)(rec + at + (size_t)r * pw);
    }
}

// One wave per (picture, plane, strip, kMetRows window rows).  MAP (test entry): the windows' values also go to `maps`,
// per picture Y | Cb | Cr, each plane in raster order of its windows.  W x H: the planes' (coded) size; WIN: the pass
// measures their top-left VW x VH (else VW x VH is not read).
template <bool MAP, bool WIN>
__global__ __launch_bounds__(256) void metrics_kernel(const PicBufs* __restrict__ slots, int first_slot, int n_pics, int W, int H,
                                                      int VW, int VH, MetricsPartial* __restrict__ partials,
                                                      float* __restrict__ maps) {
    const MetPlane L = met_plane(WIN ? VW : W, WIN ? VH : H, 0), C = met_plane(WIN ? VW : W, WIN ? VH : H, 1);
    const int per_pic = L.waves + 2 * C.waves;
    const int id = uni((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (id >= n_pics * per_pic) return; // (the whole wave)
    const int pic = id / per_pic;
    int rem = id - pic * per_pic, plane = 0;
    if (rem >= L.waves) {
        rem -= L.waves;
        plane = 1;
        if (rem >= C.waves) {
            rem -= C.waves;
            plane = 2;
        }
    }
    const MetPlane P = plane ? C : L;
    const int strip = rem / P.segs, seg = rem - strip * P.segs;
    const PicBufs& pb = slots[first_slot + pic];
    const uint8_t* org = pb.org[plane];
    const uint8_t* rec = pb.rec[plane];

    const int lane = (int)(threadIdx.x & 63);
    const int grp = strip * kMetStripLanes + lane;
    const bool own = grp < P.groups && lane < kMetStripLanes; // the group exists, and its blocks and the windows that start in its first three are this lane's
    const bool own3 = own && grp + 1 < P.groups;        // ... and the window of its fourth block and the right neighbour's first
    const int bh = P.brows, win_w = (P.pw >> 2) - 1;
    const int whole_rows = P.ph >> 2;                   // (WIN) block rows that lie inside the rectangle: bh or bh - 1
    const int pitch = WIN ? W >> (plane ? 1 : 0) : P.pw;
    const int r0 = seg * kMetRows;
    const int r_end = min(r0 + kMetRows, bh - 1);       // block rows r0 .. r_end; r_end is the next wave's r0 unless it is the last
    const bool last_seg = r_end == bh - 1;
    // a lane beyond the plane's last group reads that group again (same addresses as its owner: no traffic) and owns nothing
    const size_t col = (size_t)16 * min(grp, P.groups - 1);
    // (WIN) the bytes of the group's four dwords that lie inside the rectangle
    uint32_t col_mask[4] = {~0u, ~0u, ~0u, ~0u};
    if (WIN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int valid = min(max(P.pw - (int)col - 4 * j, 0), 4);
            col_mask[j] = valid >= 4 ? ~0u : (1u << (8 * valid)) - 1u;
        }
    }
    float* map = nullptr;
    if (MAP) map = maps + (size_t)pic * (L.windows + 2 * C.windows) + (plane ? L.windows + (plane - 1) * C.windows : 0);

    uint32_t sse = 0; // a lane's share: at most 17 rows x 4 blocks x 16 x 255^2 < 2^27
    double ssim = 0.0;
    BlockSums above[4] = {};
    // one block row: its blocks' sums, its squared error if the row is this wave's, and the windows it closes
    const auto block_row = [&](const GroupRows& g, int br, bool sse_row, bool windows) {
        BlockSums blk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                uint32_t a = g.a[r][j], b = g.b[r][j];
                if (WIN) {
                    const uint32_t m = 4 * br + r < P.ph ? col_mask[j] : 0u;
                    a &= m;
                    b &= m;
                }
                s1 = __builtin_amdgcn_udot4(a, 0x01010101u, s1, false);
                s2 = __builtin_amdgcn_udot4(b, 0x01010101u, s2, false);
                ss = __builtin_amdgcn_udot4(a, a, ss, false);
                ss = __builtin_amdgcn_udot4(b, b, ss, false);
                s12 = __builtin_amdgcn_udot4(a, b, s12, false);
            }
            blk[j] = BlockSums{s1, s2, ss, s12};
        }
        // sum (a - b)^2 = ss - 2 s12
        const uint32_t sq = (blk[0].ss - 2 * blk[0].s12) + (blk[1].ss - 2 * blk[1].s12) + (blk[2].ss - 2 * blk[2].s12) + (blk[3].ss - 2 * blk[3].s12);
        sse += own && sse_row ? sq : 0u;
        const BlockSums right = {from_right_lane(blk[0].s1), from_right_lane(blk[0].s2), from_right_lane(blk[0].ss),
                                 from_right_lane(blk[0].s12)};
        const BlockSums pair[4] = {blk[0] + blk[1], blk[1] + blk[2], blk[2] + blk[3], blk[3] + right};
        if (windows) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = ssim_window(above[j] + pair[j]);
                const bool mine = WIN ? own && 4 * grp + j < win_w : (j < 3 ? own : own3);
                ssim += mine ? (double)v : 0.0;
                if (MAP && mine) map[(size_t)(br - 1) * win_w + 4 * grp + j] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) above[j] = pair[j];
    };
    GroupRows cur, nxt;
    load_group_rows(cur, org, rec, (size_t)(4 * r0) * pitch + col, pitch);
    for (int br = r0; br < r_end; ++br) {
        // the next block row is on its way while this one is summed
        load_group_rows(nxt, org, rec, (size_t)(4 * br + 4) * pitch + col, pitch);
        block_row(cur, br, true, br > r0);
        cur = nxt;
    }
    // (r_end > r0: every wave has a block row below its first; WIN: a partial last block row closes no windows)
    block_row(cur, r_end, last_seg, WIN ? r_end < whole_rows : true);
    // the wave's pair: a fixed butterfly, so the same lanes' values are always added in the same order
    unsigned long long sse_w = sse;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        sse_w += __shfl_xor(sse_w, d, 64);
        ssim += __shfl_xor(ssim, d, 64);
    }
    if (lane == 0) partials[id] = MetricsPartial{sse_w, ssim};
}

// A picture's partials added up in index order, one thread per plane.
__global__ __launch_bounds__(64) void metrics_finish_kernel(const MetricsPartial* __restrict__ partials, int W, int H,
                                                            MetricsSums* __restrict__ sums) {
    const MetPlane L = met_plane(W, H, 0), C = met_plane(W, H, 1);
    const int plane = (int)threadIdx.x;
    if (plane >= 3) return;
    const int count = plane ? C.waves : L.waves;
    const MetricsPartial* p = partials + (size_t)blockIdx.x * (L.waves + 2 * C.waves) + (plane ? L.waves + (plane - 1) * C.waves : 0);
    unsigned long long sse = 0;
    double ssim = 0.0;
    for (int i = 0; i < count; ++i) {
        sse += p[i].sse;
        ssim += p[i].ssim;
    }
    sums[blockIdx.x].sse[plane] = sse;
    sums[blockIdx.x].ssim[plane] = ssim;
}

} // namespace wrenc
