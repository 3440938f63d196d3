// const_block.cpp -- the rate model and the constant block (const_block.h): pure host arithmetic over a config, no device
// code and no HIP call.  Built into libwrenc_gpu.so by the library's own hipcc command and flags (hipcc compiles it as it
// does the .hip units, so pow and the float code come from the compiler they always came from; its code object holds
// no code, only the copy of kRateModelMsg that a const global gets there), and by plain g++ into tools/sanitize/const_block.cpp's program.
#include "const_block.h"

// dev_scan.h marks its constexpr functions for both sides of a HIP compilation; a plain compiler knows one side
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#include "dev_scan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace wrenc;

namespace {

// DCT-2 integer cosines c[j] ~ 64*sqrt(2)*cos(j*pi/128), H.266 8.7.4.5
// (the reference's 64-point matrix, transformer.rs:934-1191, is row k = c[(2n+1)k])
const int kCos[65] = {64, 91, 90, 90, 90, 90, 90, 90, 89, 88, 88, 87, 87, 86, 85, 84, 83, 83, 82, 81, 80, 79,
                      78, 77, 75, 73, 73, 71, 70, 69, 67, 65, 64, 62, 61, 59, 57, 56, 54, 52, 50, 48, 46, 44,
                      43, 41, 38, 37, 36, 33, 31, 28, 25, 24, 22, 20, 18, 15, 13, 11, 9,  7,  4,  2,  0};

int dct64(int k, int n) {
    int t = ((2 * n + 1) * k) % 256;
    if (t > 128) t = 256 - t;
    return t > 64 ? -kCos[128 - t] : kCos[t];
}

// H.266 Table 24 (common.rs:145) and Table 25 fC (common.rs:153)
const int16_t kIntraAngle[95] = {
    512, 341, 256, 171, 128, 102, 86,  73,  64,  57,  51,  45,  39,  35,  0,   0,   32,  29,  26,
    23,  20,  18,  16,  14,  12,  10,  8,   6,   4,   3,   2,   1,   0,   -1,  -2,  -3,  -4,  -6,
    -8,  -10, -12, -14, -16, -18, -20, -23, -26, -29, -32, -29, -26, -23, -20, -18, -16, -14, -12,
    -10, -8,  -6,  -4,  -3,  -2,  -1,  0,   1,   2,   3,   4,   6,   8,   10,  12,  14,  16,  18,
    20,  23,  26,  29,  32,  35,  39,  45,  51,  57,  64,  73,  86,  102, 128, 171, 256, 341, 512};
const int8_t kFC[32][4] = {
    {0, 64, 0, 0},    {-1, 63, 2, 0},   {-2, 62, 4, 0},   {-2, 60, 7, -1},  {-2, 58, 10, -2}, {-3, 57, 12, -2},
    {-4, 56, 14, -2}, {-4, 55, 15, -2}, {-4, 54, 16, -2}, {-5, 53, 18, -2}, {-6, 52, 20, -2}, {-6, 49, 24, -3},
    {-6, 46, 28, -4}, {-5, 44, 29, -4}, {-4, 42, 30, -4}, {-4, 39, 33, -4}, {-4, 36, 36, -4}, {-4, 33, 39, -4},
    {-4, 30, 42, -4}, {-4, 29, 44, -5}, {-4, 28, 46, -6}, {-3, 24, 49, -6}, {-2, 20, 52, -6}, {-2, 18, 53, -5},
    {-2, 16, 54, -4}, {-2, 15, 55, -4}, {-2, 14, 56, -4}, {-2, 12, 57, -3}, {-2, 10, 58, -2}, {-1, 7, 60, -2},
    {0, 4, 62, -2},   {0, 2, 63, -1}};

constexpr void diag_scan(int lw, int lh, uint8_t (*out)[2]) { // ctu.rs:54-77
    const int bw = 1 << lw, bh = 1 << lh;
    int i = 0, x = 0, y = 0;
    bool stop = false;
    while (!stop) {
        while (y >= 0) {
            if (x < bw && y < bh) {
                out[i][0] = (uint8_t)x;
                out[i][1] = (uint8_t)y;
                ++i;
            }
            --y;
            ++x;
        }
        y = x;
        x = 0;
        if (i >= bw * bh) stop = true;
    }
}

// The quantisers compute the scan (dev_scan.h) where wrenc_gpu_config below fills DevConst::scan_idx for everyone else:
// the closed form against that construction -- diag_scan and the fill loop, as a constant expression -- for every
// position of every block size.  A wrong formula does not build.
constexpr bool scan_closed_form_holds() {
    for (int idx = 0; idx < 4; ++idx) {
        const int lg = idx + 2, n = 1 << lg, nsb = 1 << (2 * lg - 4);
        uint8_t d4[16][2] = {}, dsb[64][2] = {};
        diag_scan(2, 2, d4);
        diag_scan(idx, idx, dsb);
        for (int p = 0; p < n * n; ++p) {
            const int sb = nsb - 1 - (p >> 4), sp = 15 - (p & 15);
            const int x = (dsb[sb][0] << 2) + d4[sp][0];
            const int y = (dsb[sb][1] << 2) + d4[sp][1];
            if (wrenc::scan_raster(lg, p) != y * n + x) return false;
            if (wrenc::scan_sb_origin(lg, p >> 4) + wrenc::scan_nib_offset(lg, (int)wrenc::scan_nibs_from(p & 15) & 15) != y * n + x) return false;
            const int org = wrenc::scan_sb_origin(lg, p >> 4); // ... and the forms the quantisers take the origin in
            if (wrenc::scan_word_origin(wrenc::scan_batch_word(lg, p >> 6), (p >> 4) & 3) != org) return false;
            if (lg == 3 && wrenc::scan_sb_origin_ct<3>(p >> 4) != org) return false;
            if (lg == 4 && wrenc::scan_sb_origin_ct<4>(p >> 4) != org) return false;
        }
    }
    return true;
}
static_assert(scan_closed_form_holds(), "dev_scan.h: the closed form differs from the scan table's construction");

// DevConst::head_rng: the coefficients that do not end the head proof's region, and those with a quotient below 2, as one
// interval around zero each (dev_quant.h: head_alpha, quotient -- the same integer arithmetic here on the host, over
// every 16-bit coefficient; test_head_ranges_kernel holds the result against the device functions).  An interval that
// stops at the first coefficient that fails can only be too narrow, which costs a longer walk, never a wrong level.
void fill_head_ranges(DevConst& k) {
    const int ldq1 = (int32_t)k.ldq[1], ldq2 = (int32_t)k.ldq[2], ldq3 = (int32_t)k.ldq[3]; // (the 32-bit table of the kernels' LDS)
    for (int idx = 0; idx < 4; ++idx) {
        const int sh = idx + 2 + 4, off = (1 << sh) >> 1, lsc = k.lsc;
        const int dp[4] = {0, (lsc + off) >> sh, (2 * lsc + off) >> sh, (3 * lsc + off) >> sh};
        const int dn[4] = {0, (-lsc + off) >> sh, (-2 * lsc + off) >> sh, (-3 * lsc + off) >> sh};
        const auto quot = [&](int tc) {
            int S = (int)((unsigned)tc << sh) - off;
            if (tc < 0) S = -S;
            return tc == 0 ? 0 : (int)((uint32_t)(((uint64_t)(uint32_t)S * k.div_magic) >> 32) >> k.div_shift);
        };
        const auto bad = [&](int tc, bool dcn) {
            const int qd = quot(tc);
            const bool neg = tc < 0;
            const int d1 = abs(tc - (neg ? dn[1] : dp[1])), d2 = abs(tc - (neg ? dn[2] : dp[2])), d3 = abs(tc - (neg ? dn[3] : dp[3]));
            const int d1o = abs(tc - (neg ? dp[1] : dn[1]));
            const int c0tz = 128 * abs(tc);
            const int c0d0 = c0tz + ldq1;
            const int c1d0 = 128 * d2 + ldq2;
            const int c0d1 = dcn ? 128 * d1o + ldq1 : (qd ? 128 * d1 + ldq2 : c0d0);
            const int c1d1 = (qd && !dcn) ? 128 * d3 + ldq3 : 128 * d1 + ldq2;
            int alpha = c1d0 - c0tz;
            int beta = std::min(std::min(c0d0, c0d1), c1d1) - c0tz;
            if (tc == 0) {
                alpha = 1 << 28;
                beta = ldq1;
            }
            return qd >= 2 || alpha < 0 || beta < 0 || ldq1 < 0;
        };
        const auto interval = [&](int32_t* r, auto&& fails) { // r[0] = -lowest, r[1] = how many: the run of passing coefficients around 0
            r[0] = r[1] = 0;
            if (fails(0)) return;
            int tp = 0, tn = 0;
            while (tp < 32767 && !fails(tp + 1)) ++tp;
            while (tn < 32768 && !fails(-(tn + 1))) ++tn;
            r[0] = tn;
            r[1] = tp + tn + 1;
        };
        interval(&k.head_rng[idx][0], [&](int tc) { return bad(tc, false); });
        interval(&k.head_rng[idx][2], [&](int tc) { return bad(tc, true); });
        interval(&k.head_rng[idx][4], [&](int tc) { return quot(tc) >= 2; });
    }
}

// DevConst::avail_tab: the reference's availability rules (ctu.rs:2083-2188, encoder_context.rs:918-956 -- the same
// arithmetic as above_right_avail / below_left_avail / nb_avail of dev_common.h) evaluated on the host for a CTU in the
// middle of a 3 x 3-CTU picture, every block position and size.
void fill_avail_tab(DevConst& k) {
    const int W = 96, H = 96, ctu_x = 32, ctu_y = 32;
    const auto above_right = [&](int bx, int by, int lg) {
        for (;;) {
            const int n = 1 << lg;
            if (ctu_x + bx + n >= W) return false;
            if (lg == 5) return ctu_y > 0 && ctu_x + 32 < W;
            const int px = bx & ~(2 * n - 1), py = by & ~(2 * n - 1);
            if (bx == px && by == py) return ctu_y + by > 0;
            if (by == py) {
                bx = px;
                by = py;
                lg += 1;
                continue;
            }
            return bx == px;
        }
    };
    const auto below_left = [&](int bx, int by, int lg) {
        for (;;) {
            const int n = 1 << lg;
            if (ctu_y + by + n >= H) return false;
            if (lg == 5) return false;
            const int px = bx & ~(2 * n - 1), py = by & ~(2 * n - 1);
            if (px < bx) return false;
            if (by + n < py + 2 * n) return ctu_x + bx > 0;
            bx = px;
            by = py;
            lg += 1;
        }
    };
    for (int lg = 2; lg <= 5; ++lg)
        for (int by = 0; by < 32; by += 4)
            for (int bx = 0; bx < 32; bx += 4) {
                int avm = 0;
                if (!(bx & ((1 << lg) - 1)) && !(by & ((1 << lg) - 1))) {
                    const int tn = 1 << lg, gx = ctu_x + bx, gy = ctu_y + by;
                    const bool ar = above_right(bx, by, lg), bl = below_left(bx, by, lg);
                    const auto nb = [&](int xn, int yn) {
                        return xn >= 0 && yn >= 0 && xn < W && yn < H && ((xn >> 5) <= (gx >> 5) || (yn >> 5) < (gy >> 5)) &&
                               (yn >> 5) < (gy >> 5) + 1 && (xn < gx + tn || ar) && (yn < gy + tn || bl);
                    };
                    avm = (nb(gx - 1, gy + tn) ? 1 : 0) | (nb(gx - 1, gy) ? 2 : 0) | (nb(gx - 1, gy - 1) ? 4 : 0) | (nb(gx, gy - 1) ? 8 : 0) |
                          (nb(gx + tn, gy - 1) ? 16 : 0);
                }
                k.avail_tab[lg - 2][(by >> 2) * 8 + (bx >> 2)] = (uint8_t)avm;
            }
}

// DevConst::split_floor (dev_search.h, kSplitCut): lower bounds of what the children of a split cost, from the tables of
// this config alone.  A leaf costs (float)ssd + lambda * ((float)(level cost + header bits) / 16384) with ssd >= 0.  The
// level cost is a sum of lv_table entries (block_splitter.rs:415-460) and 0 for a block without levels, so 0 is its
// greatest lower bound when no entry is negative; the header bits are one entry of the leaf's tree type.  Conversion to
// f32, the product with a lambda >= 0 and the f32 sum are monotone, so the same expression over the smallest entry is
// <= every cost of that tree type.  A node returns its unsplit cost or the f32 sum of its children in z-order from 0.0,
// hence min(the unsplit floor, the children's floors summed the same way); a node at max-split-depth is a leaf.
// Where the tables prove nothing (a negative lv_table entry or header-bit minimum, a lambda that is not >= 0) every
// floor is 0.0, which is the sibling rule's own premise that costs are >= 0.
// DevConst::cand_floor (dev_search.h, kCandidateCut) under the same conditions: per mode class of a 4x4 DUAL_TREE_LUMA
// leaf the expression of rd_cost itself over ssd = 0 and the class's header bits alone, and the smallest of them over
// the classes only an angular mode can have; -inf where the tables prove nothing or a floor is not finite.
void fill_split_floors(const wrenc_gpu_config& cfg, DevConst& k) {
#ifdef __clang__ // (another compiler is given -ffp-contract=off)
#pragma clang fp contract(off)
#endif
    for (float& f : k.split_floor) f = 0.0f;
    for (float& f : k.cand_floor) f = -INFINITY;
    k.cand_floor_ang = -INFINITY;
    for (int i = 0; i < 1024; ++i)
        if (cfg.lv_table[i] < 0) return;
    if (!(cfg.lambda_rd >= 0.0f) || !(cfg.lambda_rd_chroma >= 0.0f)) return;
    int64_t dual = INT64_MAX, single = INT64_MAX, chroma = INT64_MAX;
    for (int cls = 0; cls < 67; ++cls) dual = std::min(dual, cfg.header_bits_luma[1][0][cls]); // (a 4x4 luma leaf is never CCLM)
    for (int cc = 0; cc < 4; ++cc) {
        for (int cls = 0; cls < 67; ++cls) single = std::min(single, cfg.header_bits_luma[0][cc][cls]);
        chroma = std::min(chroma, cfg.header_bits_chroma[cc]);
    }
    if (dual < 0 || single < 0 || chroma < 0) return;
    const auto floor_of = [](float lambda, int64_t bits) {
        const float f = 0.0f + lambda * ((float)bits / 16384.0f);
        return f >= 0.0f ? f : 0.0f;
    };
    const float f4 = floor_of(cfg.lambda_rd, dual), fc = floor_of(cfg.lambda_rd_chroma, chroma);
    const float fs = floor_of(cfg.lambda_rd, single);
    k.split_floor[0] = f4;
    k.split_floor[1] = fc;
    for (int level = 2; level >= 0; --level) {
        float sum = 0.0f;
        if (level == 2)
            sum = ((((sum + f4) + f4) + f4) + f4) + fc;
        else
            for (int i = 0; i < 4; ++i) sum = sum + k.split_floor[2 + level + 1];
        k.split_floor[2 + level] = level < cfg.max_split_depth ? std::min(fs, sum) : fs;
    }
    float cand[67], ang = INFINITY;
    for (int cls = 0; cls < 67; ++cls) {
        const float lv = (float)cfg.header_bits_luma[1][0][cls] * (1.0f / 16384.0f); // (rd_cost, dev_search.h, term by term)
        const float prod = cfg.lambda_rd * lv;
        cand[cls] = (float)0ULL + prod;
        if (!std::isfinite(cand[cls])) return;
        if (cls >= 2) ang = std::min(ang, cand[cls]);
    }
    memcpy(k.cand_floor, cand, sizeof(cand));
    k.cand_floor_ang = ang;
}

} // namespace

void fill_dev_const(const wrenc_gpu_config& cfg, DevConst& k) {
    memset(&k, 0, sizeof(k));
    fill_split_floors(cfg, k);
    k.W = cfg.width;
    k.H = cfg.height;
    k.qp = cfg.qp;
    k.max_depth = cfg.max_split_depth;
    k.ctu_cols = cfg.width / 32;
    k.ctu_rows = cfg.height / 32;
    static const int level_scale[6] = {40, 45, 51, 57, 64, 72}; // quantizer.rs:8
    k.lsc = (16 * level_scale[(cfg.qp + 1) % 6]) << ((cfg.qp + 1) / 6);
    {
        // n / lsc for n < 2^26 (|tc << sh| of a 16-bit coefficient) as mul_hi(n, m) >> s: with k = 26 + ceil(log2 lsc) and
        // m = floor(2^k / lsc) + 1 the error n (m lsc - 2^k) / (lsc 2^k) stays below 1 / lsc, and m < 2^28 fits 32 bits
        // (n itself does not depend on the QP: a 16-bit coefficient, the largest shift 8 + 5 - 5 + 1 = 9 of a 32x32 block, the rounding offset)
        static_assert((32768LL << 9) + (1 << 8) < (1LL << 26), "quotient(): |(tc << sh) - off| stays below 2^26");
        int lg = 0;
        while ((1 << lg) < k.lsc) ++lg;
        const int kk = 26 + lg;
        k.div_magic = (uint32_t)(((1ULL << kk) / (uint64_t)k.lsc) + 1);
        k.div_shift = (uint32_t)(kk - 32);
    }
    k.lambda_q = cfg.lambda_q;
    k.lambda_rd = cfg.lambda_rd;
    k.lambda_rd_chroma = cfg.lambda_rd_chroma;
    for (int i = 0; i < 1024; ++i) {
        k.ldq[i] = cfg.lambda_q * cfg.dq_table[i];
        k.lv[i] = cfg.lv_table[i];
    }
    memcpy(k.hb_luma, cfg.header_bits_luma, sizeof(k.hb_luma));
    memcpy(k.hb_chroma, cfg.header_bits_chroma, sizeof(k.hb_chroma));
    for (int idx = 0; idx < 4; ++idx) {
        const int n = 4 << idx, step = 64 / n;
        for (int u = 0; u < n; ++u)
            for (int x = 0; x < n; ++x) {
                k.dct[idx][u][x] = (int16_t)dct64(u * step, x);
                k.dct_t[idx][x][u] = (int16_t)dct64(u * step, x);
            }
    }
    diag_scan(2, 2, k.diag4);
    for (int idx = 0; idx < 4; ++idx) diag_scan(idx, idx, k.diag_sb[idx]);
    for (int idx = 0; idx < 4; ++idx) { // reverse-scan position -> raster index (ctu.rs:827-845: 4x4 sub-blocks)
        const int lg = idx + 2, n = 1 << lg, nsb = 1 << (2 * lg - 4);
        for (int p = 0; p < n * n; ++p) {
            const int sb = nsb - 1 - (p >> 4), sp = 15 - (p & 15);
            const int x = (k.diag_sb[idx][sb][0] << 2) + k.diag4[sp][0];
            const int y = (k.diag_sb[idx][sb][1] << 2) + k.diag4[sp][1];
            k.scan_idx[idx][p] = (uint16_t)(y * n + x);
        }
    }
    memcpy(k.intra_angle, kIntraAngle, sizeof(kIntraAngle));
    for (int mode = 0; mode < 67; ++mode) {
        // intraPredAngle and invAngle (intra_predictor.rs:1287-1310) of mode 2..66, one dword per mode
        const int angle = mode >= 2 ? kIntraAngle[14 + mode] : 0;
        int inv = 0;
        if (angle > 0)
            inv = (512 * 32 + angle / 2) / angle;
        else if (angle < 0)
            inv = -((512 * 32 + (-angle) / 2) / -angle);
        k.ang_tab[mode] = (int32_t)(((uint32_t)(uint16_t)(int16_t)angle) | ((uint32_t)(uint16_t)(int16_t)inv << 16));
    }
    memcpy(k.fc, kFC, sizeof(kFC));
    for (int u = 0; u < 32; ++u) // MFMA experiment: the 32-point basis as signed bytes
        for (int x = 0; x < 32; ++x) k.dct32_a[u][x] = (int8_t)dct64(u * 2, x);
    for (int v = 0; v < 32; ++v)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 16; ++j) k.dct32_p[v][h][j] = (int8_t)dct64(v * 2, 8 * (j / 4) + 4 * h + j % 4);
    int colsum[32];
    for (int n = 0; n < 32; ++n) {
        colsum[n] = 0;
        for (int i = 0; i < 32; ++i) colsum[n] += dct64(i * 2, n);
    }
    for (int y = 0; y < 32; ++y) {
        for (int i = 0; i < 32; ++i) k.idct32_b[y][i] = (int8_t)dct64(i * 2, y);
        k.idct32_k1[y] = 128 * colsum[y] + 64;
    }
    for (int x = 0; x < 32; ++x)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 16; ++j) k.idct32_p[x][h][j] = (int8_t)dct64((8 * (j / 4) + 4 * h + j % 4) * 2, x);
    for (int h = 0; h < 2; ++h)
        for (int w = 0; w < 16; ++w) k.idct32_k2[h][w] = 128 * colsum[8 * (w / 4) + 4 * h + w % 4] + 2048;
    // the 8x8 and 16x16 transforms as i8 MFMAs (DevConst::fdct_b ...)
    memset(k.fdct_b, 0, sizeof(k.fdct_b));
    memset(k.fdct16_p, 0, sizeof(k.fdct16_p));
    memset(k.fdct8_p, 0, sizeof(k.fdct8_p));
    memset(k.idct_b, 0, sizeof(k.idct_b));
    memset(k.idct16_p, 0, sizeof(k.idct16_p));
    memset(k.idct8_p, 0, sizeof(k.idct8_p));
    for (int idx = 0; idx < 2; ++idx) {
        const int n = 8 << idx, step = 64 / n;
        auto T = [&](int u, int x) { return dct64(u * step, x); };
        auto yk = [](int j, int h) { return 8 * (j / 4) + 4 * h + j % 4; };
        int s[16];
        for (int y = 0; y < n; ++y) {
            s[y] = 0;
            for (int i = 0; i < n; ++i) s[y] += T(i, y);
        }
        for (int m = 0; m < 32; ++m)
            for (int h = 0; h < 2; ++h) {
                for (int j = 0; j < 16; ++j) {
                    const int blk = n == 16 ? h : 2 * h + j / 8, x = j % n;
                    if (m / n == blk) {
                        k.fdct_b[idx][m][h][j] = (int8_t)T(m % n, x);
                        k.idct_b[idx][m][h][j] = (int8_t)T(x, m % n);
                    }
                    if (n == 16) {
                        if (j < 8 && m < 16) k.fdct16_p[m][h][j] = (int8_t)T(m, yk(j, h));
                        if (j / 8 == m / 16) k.idct16_p[m][h][j] = (int8_t)T(yk(j % 8, h), m % 16);
                    } else {
                        if (j / 4 == m / 8 && m / 8 < 3) k.fdct8_p[m][h][j] = (int8_t)T(m % 8, 4 * h + j % 4);
                        if (j < 8 && j / 4 == m / 16 && m % 16 < 8) k.idct8_p[m][h][j] = (int8_t)T(4 * h + j % 4, m % 16);
                    }
                }
                for (int w = 0; w < n / 2; ++w)
                    (n == 16 ? k.idct16_k2[h][w] : k.idct8_k2[h][w]) = 128 * s[yk(w, h)] + 2048;
            }
        for (int m = 0; m < 32; ++m) k.idct_k1[idx][m] = 128 * s[m % n] + 64;
    }
    fill_head_ranges(k);
    fill_avail_tab(k);
}

void resolve_config(wrenc_gpu_config* cfg, const RdParams& p) {
    const int qp = cfg->qp;
    // block_splitter.rs:29-53 (lv_dq_trellis), quantizer.rs:16-25
    for (int i = 0; i < 1024; ++i) {
        cfg->lv_table[i] = (int64_t)(std::pow((double)i + p.lv_offset, p.lv_pow) * 16384.0);
        cfg->dq_table[i] = (int64_t)std::pow((double)(i * 16384), p.quant_lv_pow);
    }
    // quantizer.rs:650-683
    cfg->lambda_q = (int64_t)(std::pow(2.0, (double)qp / p.quant_qp_div) * p.quant_lambda_mul) + p.quant_lambda_offset;
    // block_splitter.rs:289-309,472
    cfg->lambda_rd = std::pow(2.0f, (float)qp / p.qp_div) * p.lambda_mul;
    cfg->lambda_rd_chroma = std::pow(2.0f, (float)qp / p.qp_div) * (p.has_a ? p.a : p.lambda_mul); // :775-778
    // block_splitter.rs:187-406 (dep-quant + trellis variants)
    for (int tree = 0; tree < 2; ++tree)
        for (int cc = 0; cc < 4; ++cc)
            for (int cls = 0; cls < 67; ++cls) {
                float cclm_bits;
                if (cc > 0)
                    cclm_bits = p.cclm_offset + std::pow((float)(cc - 1) + p.cclm_mode_idx_offset, p.cclm_pow);
                else if (tree == 1)
                    cclm_bits = 0.0f;
                else
                    cclm_bits = p.non_cclm_offset;
                float mode_bits;
                if (cls == 0) {
                    mode_bits = p.planar_offset;
                } else {
                    float t;
                    if (cls <= 5)
                        t = std::pow((float)(cls - 1) + p.mpm_idx_offset, p.mpm_idx_pow);
                    else
                        t = p.mpm_remainder_mult * std::pow((float)(cls - 6) + p.mpm_remainder_offset, p.mpm_remainder_pow);
                    mode_bits = p.non_planar_offset + t;
                }
                mode_bits = mode_bits + cclm_bits;
                const float hb = tree == 0 ? p.header_bits + mode_bits : p.header_bits / 3.0f + mode_bits;
                cfg->header_bits_luma[tree][cc][cls] = (int64_t)(hb * 16384.0f);
            }
    for (int cc = 0; cc < 4; ++cc) {
        const float mode_bits =
            cc > 0 ? p.cclm_offset + std::pow((float)(cc - 1) + p.cclm_mode_idx_offset, p.cclm_pow) : p.non_cclm_offset;
        cfg->header_bits_chroma[cc] = (int64_t)((p.chroma_header_bits + mode_bits) * 16384.0f);
    }
}

int config_extra_params(wrenc_gpu_config* cfg, const char* extra_params, std::string& err) {
    const auto fail = [&err](int code, const std::string& msg) {
        err = msg;
        return code;
    };
    RdParams p;
    const struct { const char* key; double* f64; float* f32; long long* i64; } live[] = {
        {"lv_pow_dq_trellis", &p.lv_pow, nullptr, nullptr},
        {"lv_offset_dq_trellis", &p.lv_offset, nullptr, nullptr},
        {"quant_lv_pow", &p.quant_lv_pow, nullptr, nullptr},
        {"quant_qp_div_trellis", &p.quant_qp_div, nullptr, nullptr},
        {"quant_lambda_mul_trellis", &p.quant_lambda_mul, nullptr, nullptr},
        {"quant_lambda_offset_trellis", nullptr, nullptr, &p.quant_lambda_offset},
        {"qp_div_dq_trellis", nullptr, &p.qp_div, nullptr},
        {"lambda_mul_dq_trellis", nullptr, &p.lambda_mul, nullptr},
        {"non_planar_offset_dq_trellis", nullptr, &p.non_planar_offset, nullptr},
        {"mpm_idx_offset_dq_trellis", nullptr, &p.mpm_idx_offset, nullptr},
        {"mpm_remainder_mult_dq_trellis", nullptr, &p.mpm_remainder_mult, nullptr},
        {"mpm_remainder_offset_dq_trellis", nullptr, &p.mpm_remainder_offset, nullptr},
        {"planer_offset_dq_trellis", nullptr, &p.planar_offset, nullptr}, // sic
        {"header_bits_dq_trellis", nullptr, &p.header_bits, nullptr},
        {"chroma_header_bits_dq_trellis", nullptr, &p.chroma_header_bits, nullptr},
        {"cclm_pow", nullptr, &p.cclm_pow, nullptr},
        {"mpm_idx_pow", nullptr, &p.mpm_idx_pow, nullptr},
        {"mpm_remainder_pow", nullptr, &p.mpm_remainder_pow, nullptr},
        {"cclm_mode_idx_offset_dq_trellis", nullptr, &p.cclm_mode_idx_offset, nullptr},
        {"non_cclm_offset_dq_trellis", nullptr, &p.non_cclm_offset, nullptr},
        {"cclm_offset_dq_trellis", nullptr, &p.cclm_offset, nullptr},
        {"a", nullptr, &p.a, nullptr},
    };
    const std::string text = extra_params ? extra_params : "";
    size_t pos = 0;
    while (!text.empty() && pos <= text.size()) {
        size_t end = text.find(',', pos);
        if (end == std::string::npos) end = text.size();
        const std::string item = text.substr(pos, end - pos);
        const size_t eq = item.find('=');
        if (eq == std::string::npos || item.find('=', eq + 1) != std::string::npos)
            return fail(WRENC_GPU_EINVAL, "Invalid extra-params: " + text); // main.rs:205-215
        const std::string key = item.substr(0, eq), val = item.substr(eq + 1);
        for (const auto& l : live) {
            if (key != l.key) continue;
            char* rest = nullptr;
            if (l.f64) *l.f64 = strtod(val.c_str(), &rest);
            if (l.f32) *l.f32 = strtof(val.c_str(), &rest);
            if (l.i64) *l.i64 = strtoll(val.c_str(), &rest, 10);
            if (val.empty() || (rest && *rest)) // the reference's parse().unwrap() panics here
                return fail(WRENC_GPU_EINVAL, "extra-params: " + key + " has no numeric value: " + val);
            if (key == "a") p.has_a = true;
        }
        // any other key is stored and never read by the live code path, as in the reference
        pos = end + 1;
    }
    resolve_config(cfg, p);
    return WRENC_GPU_OK;
}

// The trellis keeps path costs in 32 bits (dev_quant.h, above kNoBranch): exact as long as one step costs less than 2^25,
// i.e. 128 * 65535 + lambda_q * dq_table[bits] < 2^25 for every table entry -- true for the reference's defaults at every
// QP (22.6 M at QP 63) and for rate models anywhere near them, not for e.g. quant_lv_pow = 2.5 or quant_qp_div_trellis =
// 1.5 (--extra-params), where the reference's own i64 products reach 10^11 .. 10^19.  Refused rather than searched
// with other results than the reference's.  (lambda_q grows with the QP: a model may fit at one QP and not at another.)
bool rate_model_fits(const wrenc_gpu_config& cfg) {
    constexpr long long kStepRoom = (1LL << 25) - 128LL * 65535LL;
    bool fits = cfg.lambda_q >= 0 && cfg.lambda_q < kStepRoom;
    for (int i = 0; fits && i < 1024; ++i)
        fits = cfg.dq_table[i] >= 0 && cfg.dq_table[i] < kStepRoom && cfg.lambda_q * cfg.dq_table[i] < kStepRoom;
    return fits;
}
const char* const kRateModelMsg =
    "the quantiser's rate model (lambda_q x dq_table) is outside the range the device's 32-bit trellis costs cover";
