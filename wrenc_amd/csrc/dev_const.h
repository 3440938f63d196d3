// dev_const.h -- the constant block of one config (one QP): what the host derives from a wrenc_gpu_config before the first
// launch (const_block.cpp, fill_dev_const) and the kernels read through the constant address space.  Plain C++: the host
// unit that fills it and the device headers that read it (dev_common.h includes this file) see the same bytes.
#pragma once
#include <stdint.h>

namespace wrenc {

// Constants resolved on the host (see wrenc_gpu_config in include/wrenc_gpu.h).
struct DevConst {
    int32_t W, H, qp, max_depth, ctu_cols, ctu_rows;
    int32_t lsc;              // quantizer.rs:617-622 (16*LEVEL_SCALE[0][(qp+1)%6]) << ((qp+1)/6)
    uint32_t div_magic;       // floor(2^k / lsc) + 1, k = 26 + ceil(log2 lsc): exact n / lsc = mul_hi(n, magic) >> (k - 32) for n < 2^26
    uint32_t div_shift;       // k - 32
    int64_t lambda_q;
    float lambda_rd;
    float lambda_rd_chroma;
    int64_t ldq[1024];        // lambda_q * dq_table[bits]  (quantizer.rs:29-31)
    int64_t lv[1024];
    int64_t hb_luma[2][4][67];
    int64_t hb_chroma[4];
    int16_t dct[4][32][32];   // T_N[u][k] = dct64[u * 64/N][k], N = 4 << idx (transformer.rs:1212-1221)
    int16_t dct_t[4][32][32]; // transposed: dct_t[idx][y][i] = T_N[i][y]
    uint8_t diag4[16][2];     // 4x4 up-right diagonal scan (x, y)   (ctu.rs:14-81)
    uint8_t diag_sb[4][64][2]; // sub-block scan for 1, 4, 16, 64 sub-blocks
    uint16_t scan_idx[4][1024]; // raster index y*n+x of reverse-scan position p (p = 0: last in scan)
    int16_t intra_angle[95];  // common.rs:145
    int32_t ang_tab[67];      // per mode: intraPredAngle (low half) | invAngle (high half), read with one scalar load
    int8_t fc[32][4];         // common.rs:153
    // MFMA experiment (dev_transform.h, fwd_dct32_mfma): the 32-point basis as signed bytes (|T| <= 90),
    // [u][x] for the stage that contracts over x, and with the k order of an MFMA accumulator
    // ([v][h][j] = T[v][8 (j / 4) + 4 h + j % 4]) for the stage that contracts over the first stage's output
    int8_t dct32_a[32][32];
    int8_t dct32_p[32][2][16];
    // the same for the inverse transform (inv_dct32_mfma): [y][i] = T[i][y] for its first stage, [x][h][j] =
    // T[8 (j / 4) + 4 h + j % 4][x] for its second; both stages feed 16-bit operands as a signed high byte and a low
    // byte minus 128, so 128 * sum_i T[i][n] comes back with the rounding constant: idct32_k1[y] = 128 S[y] + 64,
    // idct32_k2[h][w] = 128 S[x] + 2048 for the x of accumulator w in lane half h
    int8_t idct32_b[32][32];
    int8_t idct32_p[32][2][16];
    int32_t idct32_k1[32];
    int32_t idct32_k2[2][16];
    // The 8x8 and 16x16 transforms as i8 MFMAs (dev_transform.h, fwd_dct_mfma / inv_dct_mfma), T = T_N, N = 8 << idx;
    // [n][h][j]: byte j of the operand of lane n + 32 h; column n = (block n / N, index n % N); yk(j, h) = 8 (j / 4) + 4 h
    // + j % 4 is the accumulator row of register j in lane half h.
    //   fdct_b[idx]: block-diagonal T[u][x] (N = 16: block h, x = j; N = 8: block 2 h + j / 8, x = j % 8), else 0
    //   fdct16_p:    rows m < 16: T[m][yk(j, h)], rows 16..31: 0 (three chained digit products)
    //   fdct8_p:     rows m = 8 a + v, a < 3: T[v][4 h + j % 4] where j / 4 == a, else 0 (digit a of slot group j / 4)
    //   idct_b[idx]: block-diagonal T[i][y], as fdct_b with (u, x) -> (y, i)
    //   idct16_p:    rows m = 16 b + x: T[yk(j % 8, h)][x] where j / 8 == b, else 0
    //   idct8_p:     rows m = 16 b + x, x < 8: T[4 h + j % 4][x] where j / 4 == b, else 0
    //   idct_k1[idx][n] = 128 S[n % N] + 64, idct16_k2[h][w] = 128 S[yk(w, h)] + 2048, idct8_k2[h][w] = 128 S[4 h + w] + 2048,
    //   S[n] = sum_i T[i][n]
    alignas(16) int8_t fdct_b[2][32][2][16];
    alignas(16) int8_t fdct16_p[32][2][8];
    alignas(16) int8_t fdct8_p[32][2][16];
    alignas(16) int8_t idct_b[2][32][2][16];
    alignas(16) int8_t idct16_p[32][2][16];
    alignas(16) int8_t idct8_p[32][2][8];
    alignas(16) int32_t idct_k1[2][32];
    alignas(16) int32_t idct16_k2[2][8];
    alignas(16) int32_t idct8_k2[2][4];
    // The head proof's per-coefficient conditions (dev_quant.h, head_alpha) as range tests, per block size lg - 2: a coefficient tc
    // (a) does not end the region  <=>  (unsigned)(tc + r[0]) < (unsigned)r[1];  (b) the same at the DC position with r[2], r[3];
    // (c) has a quotient below 2  <=>  (unsigned)(tc + r[4]) < (unsigned)r[5].  Filled by the host from the same formulas
    // (fill_head_ranges; test_head_ranges_kernel compares them with the device functions over every 16-bit coefficient).
    int32_t head_rng[4][6];
    // Which of a block's five reference segments (bit 0 below-left, 1 left, 2 corner, 3 above, 4 above-right) the coding
    // order makes available, for a block at (bx, by) of log2 size lg inside a CTU away from every picture edge:
    // [lg - 2][(by / 4) * 8 + bx / 4] (block_avail_mask adds the edges).  From the formulas themselves on the host
    // (fill_avail_tab); test_avail_tab_kernel holds the two against each other at every position of small pictures.
    uint8_t avail_tab[4][64];
    // Split-cut floors (dev_search.h, kSplitCut; fill_split_floors): what a child of a split costs at least at this QP.
    // [0] a DUAL_TREE_LUMA 4x4 leaf, [1] the DUAL_TREE_CHROMA leaf, [2 + level] a node at tree level 0 .. 2 (32x32,
    // 16x16, 8x8).  All 0.0 where the tables prove nothing.
    float split_floor[5];
    // Candidate floors of a 4x4 DUAL_TREE_LUMA leaf (dev_search.h, kCandidateCut; fill_split_floors): per mode class what a
    // candidate of that class costs with no distortion and no levels, rd_cost(0, hb_luma[1][0][cls], lambda_rd), and the
    // smallest of them over the classes 2 .. 66 (mpm_idx 1 .. 4 and every remainder, which only angular modes can have).
    // All -inf where the tables prove nothing: a floor of -inf never reaches a cost.
    float cand_floor[67];
    float cand_floor_ang;
};

} // namespace wrenc
