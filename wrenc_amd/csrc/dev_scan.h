// The coefficient scan as arithmetic: raster index y * n + x of reverse-scan position p in a block of side n = 1 << lg
// (p = 0: last in scan), the mapping DevConst::scan_idx holds as a table (ctu.rs:54-77, 827-845).  No memory, no LDS,
// no static table: the quantisers (dev_quant.h) compute the index instead of loading it.  const_block.cpp holds every
// function here against the table's construction at compile time, for every p of every size.
//
// The scan visits the 4x4 sub-blocks of the block along up-right diagonals, and the 16 positions of a sub-block the
// same way.  Forward, index k of a g x g grid lies on diagonal d, the largest d with d (d + 1) / 2 <= k, at
// x = k - d (d + 1) / 2, y = d - x, as long as the diagonal is not cut by the grid's edge, which holds for k < g g / 2;
// the grid's scan is symmetric under a half turn (k <-> g g - 1 - k, (x, y) <-> (g - 1 - x, g - 1 - y)), which gives the
// other half -- and the reverse scan, sub-block s of which is forward sub-block g g - 1 - s.
//
// What a kernel may spend on it: the search kernels are bound by instruction issue, and a table load costs about four
// instructions.  scan_sb_origin per lane is some twenty VALU instructions: right once per call
// (the traces), a loss once per batch of a gather.  There the block size and the batch are compile-time constants and
// the four origins of a batch one literal (scan_batch_word): a bit-field extract per lane.
#pragma once
#include <stdint.h>

namespace wrenc {

// the largest d with d (d + 1) / 2 <= k, for k <= 31: one bit per triangular number 0, 1, 3, 6, 10, 15, 21, 28
constexpr __host__ __device__ inline int scan_tri_root(int k) { return __builtin_popcount(0x1020844Bu & ((2u << k) - 1u)) - 1; }

// raster index of the first sample (top left) of reverse-scan sub-block s (= p >> 4) of a block of log2 size lg
constexpr __host__ __device__ inline int scan_sb_origin(int lg, int s) {
    const int nsb = 1 << (2 * lg - 4), g1 = (1 << (lg - 2)) - 1;
    const bool low = 2 * s < nsb;              // forward sub-block nsb - 1 - s is in the upper half: the half turn of s
    const int k = low ? s : nsb - 1 - s;       // < max(nsb / 2, 1) <= 32
    const int d = scan_tri_root(k);
    const int x = k - ((d * (d + 1)) >> 1), y = d - x;
    const int bx = low ? g1 - x : x, by = low ? g1 - y : y;
    return (by << (lg + 2)) + (bx << 2);
}

// y4 * 4 + x4 of position i (= p & 15) inside its sub-block: for a 4x4 block the whole raster index
constexpr __host__ __device__ inline int scan_nib(int i) { return (int)(0x041852C963DA7EBFull >> (4 * i)) & 15; }
// the sixteen of them from position i on, one per nibble (a loop over consecutive positions shifts them out)
constexpr __host__ __device__ inline unsigned long long scan_nibs_from(int i) { return 0x041852C963DA7EBFull >> (4 * i); }
// raster offset of such a nibble from the sub-block's origin
constexpr __host__ __device__ inline int scan_nib_offset(int lg, int nib) { return ((nib >> 2) << lg) + (nib & 3); }

// The origins of the four sub-blocks 4 t .. 4 t + 3 -- those of the batch of 64 positions 64 t .. 64 t + 63, one per
// 16-lane row --, a quarter of each (it fits a byte up to 32x32) in byte 0 .. 3.  With lg and t known at compile time the
// word is a literal and a lane's origin one bit-field extract away.
constexpr __host__ __device__ inline uint32_t scan_batch_word(int lg, int t) {
    const int nsb = 1 << (2 * lg - 4);
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j)
        if (4 * t + j < nsb) w |= (uint32_t)(scan_sb_origin(lg, 4 * t + j) >> 2) << (8 * j);
    return w;
}
constexpr __host__ __device__ inline int scan_word_origin(uint32_t w, int row) { return (int)((w >> (8 * row)) & 0xFFu) << 2; }
// the origin of sub-block s (per lane) of a block whose size is known at compile time: selects between literals
template <int LG>
constexpr __host__ __device__ inline int scan_sb_origin_ct(int s) {
    static_assert(LG >= 2 && LG <= 4, "4x4, 8x8 and 16x16");
    if constexpr (LG == 2) {
        return 0;
    } else if constexpr (LG == 3) {
        constexpr uint32_t w0 = scan_batch_word(3, 0);
        return scan_word_origin(w0, s);
    } else {
        constexpr uint32_t w0 = scan_batch_word(4, 0), w1 = scan_batch_word(4, 1), w2 = scan_batch_word(4, 2), w3 = scan_batch_word(4, 3);
        const int q = s >> 2;
        return scan_word_origin(q == 0 ? w0 : (q == 1 ? w1 : (q == 2 ? w2 : w3)), s & 3);
    }
}

constexpr __host__ __device__ inline int scan_raster(int lg, int p) { return scan_sb_origin(lg, p >> 4) + scan_nib_offset(lg, scan_nib(p & 15)); }

} // namespace wrenc
