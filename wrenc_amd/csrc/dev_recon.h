// dev_recon.h -- the reconstruction of a slot on its way out (include/wrenc_gpu.h: wrenc_gpu_download_recon, _recon_device;
// the rules are defined in include/wrenc_recon.h, in integers, and met bit for bit): dev_rgb.h turned round.  The kernels
// read the VISIBLE rectangle of the slot's reconstruction planes (coded pitch) and write the picture in the output format
// into the context's recon staging planes; the entry then copies those rows into the caller's planes with the caller's
// strides (a 2-D copy).  The upload's design mirrored: the library's kernels keep the library's own alignment.
//
// recon_rgb_kernel<layout>: one launch per picture.  A workgroup is 4 waves; a wave takes one PAIR of luma rows 2j, 2j + 1,
// so the rows and every base address are scalar, and a lane makes kReconGroup = 8 neighbouring pixels of each of the two
// rows.  It loads 8 luma bytes per row and, of each chroma plane, the dword of samples 4g .. 4g + 3 of rows j - 1, j, j + 1
// (row indices clamped to the visible plane).  Cb and Cr of a column travel as one dword, Cb in the low half and Cr in the
// high half: the vertical sums 3 C(j) + C(j -+ 1) (at most 1020) are taken once per column for the upper and for the lower
// luma row -- each is used by the two or three pixels that touch the column -- and the horizontal step 3 V(i) + V(i') (at most
// 4080) gives Cb16 and Cr16 of a pixel with two integer operations.
// The neighbour columns 4g - 1 and 4g + 4 come from the ADJACENT LANES as vertical sums (four wave shuffles a lane, no LDS
// allocated); the lanes at a wave's edge (lane 0 behind the first workgroup of a row, lane 63 in front of the next) load
// their six bytes each themselves.  The alternative -- every lane loads its neighbour bytes, hitting the cache -- costs every
// lane twelve more byte loads and their address arithmetic for data a neighbour holds in a register.  Columns beyond the
// visible plane are never used: the last lane of a row replaces them by its last visible column (the clamp of the rules),
// whatever the margin holds.
// The multiply: bu of the tv tables (34610, 33050) does not fit a signed 16-bit operand, so the v_dot2 form of the forward
// converter cannot take these tables.  Every operand here fits 24 bits (16 cy = 305232, |U|, |V| <= 2048), so each product is
// one v_mad_i32_i24 at full rate: luma is cy' Y + k with cy' = 16 cy and k = (1 << 17) - cy' yoff folded on the host side of
// the launch (exact: no intermediate leaves 32 bits), and R, G, B take one, two and one more.
// Stores per row: 24 bytes (rgb24, bgr24: three 8-byte stores), 32 bytes (rgb0, bgr0: two 16-byte stores) or 8 bytes to each
// of three planes (gbrp).  A pixel is one dword R | G << 8 | B << 16 | 255 << 24 (recon_pixel tells why it is made by
// v_perm_b32 too); the packed layouts are v_perm_b32 of neighbouring pixels, and the bgr layouts are another selector, not a
// branch.
//
// recon_yuv_kernel<pairs>: the crop (yuv420p) and the CbCr interleave (nv12).  A wave takes one row of one plane, a lane 8
// samples: an 8-byte load and store, or 8 Cb and 8 Cr into one 16-byte store.
//
// Alignment and bounds.  Reads: the planes have the coded pitch W (a multiple of 32) and W / 2; a live lane has 8g < w or
// 4g < w / 2 (8g < w / 2 for a chroma row of the yuv kernel), so its 8-byte and 4-byte loads end inside the row's pitch.
// Writes: a staging row is recon_stage_pitch() long: room for what every live lane stores, rounded up to 32 bytes; planes
// follow each other at pitch x rows.  Full-width stores therefore never leave a row's pitch, and what a tail lane writes
// beyond the row's samples is never copied out.  No LDS, no table, no division, no scratch.
#pragma once

#include "../../include/wrenc_recon.h"
#include "dev_format.h"

namespace wrenc {

constexpr int kReconGroup = 8; // luma samples per lane and row
constexpr int kReconRows = 4;  // row pairs (rgb) or rows (yuv) per workgroup: one per wave

// bytes a lane stores of one row of plane `plane` (0: luma or the RGB planes; else a chroma plane)
__host__ __device__ constexpr int recon_lane_bytes(int format, int plane) {
    return format < WRENC_RGB_COUNT ? (format == WRENC_RGB_GBRP ? kReconGroup : format >= WRENC_RGB_RGB0 ? 4 * kReconGroup : 3 * kReconGroup)
                                      : (format == WRENC_RECON_NV12 && plane ? 2 * kReconGroup : kReconGroup);
}
// the pitch of a staging plane whose rows hold `samples` luma or chroma samples (nv12's second plane: pairs)
__host__ __device__ inline size_t recon_stage_pitch(int format, int plane, int samples) {
    return format_raw_pitch((size_t)recon_lane_bytes(format, plane) * (size_t)((samples + kReconGroup - 1) / kReconGroup));
}

struct ReconArgs {
    const uint8_t* rec[3]; // the slot's reconstruction planes (PicBufs::rec), coded pitch
    uint8_t* dst;          // the recon staging planes: one allocation
    size_t dst_off[3];     // byte offset of each staging plane, as wrenc_recon_layout numbers them
    int dst_pitch[3];      // bytes, multiples of kFormatRawAlign
    int W;                 // the coded luma pitch
    int w, h;              // the visible size: the picture that is made
    int row_blocks[2];     // yuv kernel: workgroups down the luma plane and down a chroma plane
    int cy16, yk;          // rgb kernel: 16 cy, and (1 << 17) - 16 cy yoff
    int rv, gu, gv, bu;
};

__host__ __device__ constexpr uint32_t recon_sel(int b0, int b1, int b2, int b3) {
    return (uint32_t)b0 | (uint32_t)b1 << 8 | (uint32_t)b2 << 16 | (uint32_t)b3 << 24;
}

// byte k of cb in the low half, byte k of cr in the high half
template <int K>
__device__ __forceinline__ uint32_t recon_pair(uint32_t cb, uint32_t cr) { return __builtin_amdgcn_perm(cr, cb, recon_sel(K, 0x0C, 4 + K, 0x0C)); }

// the vertical sums of chroma column `col` (a wave edge's neighbour column), for the upper and the lower luma row
__device__ __forceinline__ void recon_edge_column(const ReconArgs& a, int jm, int j, int jp, int col, uint32_t& top, uint32_t& bot) {
    const size_t cp = (size_t)(a.W >> 1);
    const uint8_t *b = a.rec[1] + col, *r = a.rec[2] + col;
    const uint32_t m = (uint32_t)b[(size_t)jm * cp] | (uint32_t)r[(size_t)jm * cp] << 16;
    const uint32_t c = (uint32_t)b[(size_t)j * cp] | (uint32_t)r[(size_t)j * cp] << 16;
    const uint32_t p = (uint32_t)b[(size_t)jp * cp] | (uint32_t)r[(size_t)jp * cp] << 16;
    top = 3 * c + m;
    bot = 3 * c + p;
}

__device__ __forceinline__ int recon_clip(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// Four clipped samples as the bytes of a dword, and a pixel R | G << 8 | B << 16 | 255 << 24.  Neighbouring bytes are joined by
// v_perm_b32 of two dwords that hold samples 16 bits apart, never by `a | b << 8`: the compiler turns clip(x >> 18) |
// clip(y >> 18) << 8 into one v_ashr_pk_u8_i32 and takes the upper half of its result for zero, which on the device it was
// not (the wrong bytes were B | byte 2 of what the destination register held before), so a third byte ORed on top came out
// wrong.
__device__ __forceinline__ uint32_t recon_bytes(int b0, int b1, int b2, int b3) {
    return __builtin_amdgcn_perm((uint32_t)b1 | (uint32_t)b3 << 16, (uint32_t)b0 | (uint32_t)b2 << 16, recon_sel(0, 4, 2, 6));
}
__device__ __forceinline__ uint32_t recon_pixel(int r, int g, int b) {
    return __builtin_amdgcn_perm((uint32_t)g, (uint32_t)r | (uint32_t)b << 16, recon_sel(0, 4, 2, 0x0D)); // selector 13: 0xFF
}

// L: the layout (wrenc_rgb.h).  Grid: x over groups of 64 lanes along a luma row, y over workgroups of kReconRows row pairs.
template <int L>
__global__ __launch_bounds__(64 * kReconRows) void recon_rgb_kernel(ReconArgs a) {
    static_assert(L >= 0 && L < WRENC_RGB_COUNT, "a layout of wrenc_rgb.h");
    constexpr bool kSwap = L == WRENC_RGB_BGR24 || L == WRENC_RGB_BGR0;
    const int lane = (int)threadIdx.x, g = (int)(blockIdx.x * 64) + lane;
    const int j = __builtin_amdgcn_readfirstlane((int)blockIdx.y * kReconRows + (int)threadIdx.y);
    const int cw = a.w >> 1, ch = a.h >> 1;
    if (j >= ch || kReconGroup * g >= a.w) return;
    const int jm = j > 0 ? j - 1 : 0, jp = j + 1 < ch ? j + 1 : ch - 1;
    const size_t cp = (size_t)(a.W >> 1);
    // the lane's own four columns of the three rows
    const uint8_t *pb = a.rec[1] + 4 * g, *pr = a.rec[2] + 4 * g;
    const uint32_t bm = *(const uint32_t*)(pb + (size_t)jm * cp), bc = *(const uint32_t*)(pb + (size_t)j * cp), bp = *(const uint32_t*)(pb + (size_t)jp * cp);
    const uint32_t rm = *(const uint32_t*)(pr + (size_t)jm * cp), rc = *(const uint32_t*)(pr + (size_t)j * cp), rp = *(const uint32_t*)(pr + (size_t)jp * cp);
    const uint2 y0 = *(const uint2*)(a.rec[0] + (size_t)(2 * j) * a.W + kReconGroup * g);
    const uint2 y1 = *(const uint2*)(a.rec[0] + (size_t)(2 * j + 1) * a.W + kReconGroup * g);
    // columns -1 .. 4 of the lane: [0] and [5] are the neighbours'
    uint32_t top[6], bot[6];
    {
        const uint32_t c0 = recon_pair<0>(bc, rc), c1 = recon_pair<1>(bc, rc), c2 = recon_pair<2>(bc, rc), c3 = recon_pair<3>(bc, rc);
        top[1] = 3 * c0 + recon_pair<0>(bm, rm), bot[1] = 3 * c0 + recon_pair<0>(bp, rp);
        top[2] = 3 * c1 + recon_pair<1>(bm, rm), bot[2] = 3 * c1 + recon_pair<1>(bp, rp);
        top[3] = 3 * c2 + recon_pair<2>(bm, rm), bot[3] = 3 * c2 + recon_pair<2>(bp, rp);
        top[4] = 3 * c3 + recon_pair<3>(bm, rm), bot[4] = 3 * c3 + recon_pair<3>(bp, rp);
    }
    // the last lane of a row: columns beyond the visible plane are its last visible column
    const int live = cw - 4 * g; // >= 1
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (k >= live) top[1 + k] = top[k], bot[1 + k] = bot[k];
    // the neighbours' columns: every live lane of the wave takes part in the shuffles
    const uint32_t lt = (uint32_t)__shfl_up((int)top[4], 1), lb = (uint32_t)__shfl_up((int)bot[4], 1);
    const uint32_t nt = (uint32_t)__shfl_down((int)top[1], 1), nb = (uint32_t)__shfl_down((int)bot[1], 1);
    top[0] = lt, bot[0] = lb, top[5] = nt, bot[5] = nb;
    if (g == 0) {
        top[0] = top[1], bot[0] = bot[1];
    } else if (lane == 0) {
        recon_edge_column(a, jm, j, jp, 4 * g - 1, top[0], bot[0]);
    }
    if (live <= 4) {
        top[5] = top[4], bot[5] = bot[4];
    } else if (lane == 63) {
        recon_edge_column(a, jm, j, jp, 4 * g + 4, top[5], bot[5]);
    }
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        const uint2 yy = row ? y1 : y0;
        const uint32_t* v = row ? bot : top;
        int r[kReconGroup], gg[kReconGroup], b[kReconGroup];
#pragma unroll
        for (int q = 0; q < kReconGroup; ++q) {
            const int e = 1 + (q >> 1);
            const uint32_t c16 = 3 * v[e] + v[(q & 1) ? e + 1 : e - 1]; // Cb16 | Cr16 << 16
            const int cu = (int)(c16 & 0xFFFFu) - 2048, cv = (int)(c16 >> 16) - 2048;
            const int luma = (int)(((q < 4 ? yy.x : yy.y) >> (8 * (q & 3))) & 0xFFu);
            const int yd = __mul24(luma, a.cy16) + a.yk;
            r[q] = recon_clip((__mul24(cv, a.rv) + yd) >> 18);
            gg[q] = recon_clip((__mul24(cu, a.gu) + __mul24(cv, a.gv) + yd) >> 18);
            b[q] = recon_clip((__mul24(cu, a.bu) + yd) >> 18);
        }
        const size_t line = (size_t)(2 * j + row) * (size_t)a.dst_pitch[0];
        if (L == WRENC_RGB_GBRP) {
            const int* comp[3] = {gg, b, r};
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const int* c = comp[p];
                const uint2 o = make_uint2(recon_bytes(c[0], c[1], c[2], c[3]), recon_bytes(c[4], c[5], c[6], c[7]));
                *(uint2*)(a.dst + a.dst_off[p] + line + kReconGroup * g) = o;
            }
        } else {
            uint32_t px[kReconGroup]; // R | G << 8 | B << 16 | 255 << 24
#pragma unroll
            for (int q = 0; q < kReconGroup; ++q) px[q] = recon_pixel(r[q], gg[q], b[q]);
            uint8_t* out = a.dst + a.dst_off[0] + line + (size_t)recon_lane_bytes(L, 0) * g;
            if (L == WRENC_RGB_RGB0 || L == WRENC_RGB_BGR0) {
                uint32_t o[kReconGroup];
#pragma unroll
                for (int q = 0; q < kReconGroup; ++q) o[q] = kSwap ? __builtin_amdgcn_perm(0u, px[q], recon_sel(2, 1, 0, 3)) : px[q];
                *(uint4*)out = make_uint4(o[0], o[1], o[2], o[3]);
                *(uint4*)(out + 16) = make_uint4(o[4], o[5], o[6], o[7]);
            } else {
                // four pixels are three dwords: P0 P0 P0 P1 | P1 P1 P2 P2 | P2 P3 P3 P3
                constexpr uint32_t s0 = kSwap ? recon_sel(2, 1, 0, 6) : recon_sel(0, 1, 2, 4);
                constexpr uint32_t s1 = kSwap ? recon_sel(1, 0, 6, 5) : recon_sel(1, 2, 4, 5);
                constexpr uint32_t s2 = kSwap ? recon_sel(0, 6, 5, 4) : recon_sel(2, 4, 5, 6);
                uint32_t o[6];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    o[3 * t] = __builtin_amdgcn_perm(px[4 * t + 1], px[4 * t], s0);
                    o[3 * t + 1] = __builtin_amdgcn_perm(px[4 * t + 2], px[4 * t + 1], s1);
                    o[3 * t + 2] = __builtin_amdgcn_perm(px[4 * t + 3], px[4 * t + 2], s2);
                }
                *(uint2*)out = make_uint2(o[0], o[1]);
                *(uint2*)(out + 8) = make_uint2(o[2], o[3]);
                *(uint2*)(out + 16) = make_uint2(o[4], o[5]);
            }
        }
    }
}

// PAIRS: nv12 (CbCr interleaved into plane 1), else yuv420p.  Grid: x over groups of 64 lanes along a luma row, y over
// row_blocks[0] workgroups of luma rows, then row_blocks[1] of chroma rows once (interleaved) or twice (planar).
template <bool PAIRS>
__global__ __launch_bounds__(64 * kReconRows) void recon_yuv_kernel(ReconArgs a) {
    int by = (int)blockIdx.y, plane = 0;
    if (by >= a.row_blocks[0]) {
        by -= a.row_blocks[0];
        plane = 1;
        if (!PAIRS && by >= a.row_blocks[1]) {
            by -= a.row_blocks[1];
            plane = 2;
        }
    }
    const int c = plane ? 1 : 0;
    const int g = (int)(blockIdx.x * 64 + threadIdx.x), r = by * kReconRows + (int)threadIdx.y;
    if (r >= (a.h >> c) || kReconGroup * g >= (a.w >> c)) return;
    const size_t sp = (size_t)(a.W >> c);
    if (PAIRS && plane) {
        const uint2 u = *(const uint2*)(a.rec[1] + (size_t)r * sp + kReconGroup * g), v = *(const uint2*)(a.rec[2] + (size_t)r * sp + kReconGroup * g);
        constexpr uint32_t lo = recon_sel(0, 4, 1, 5), hi = recon_sel(2, 6, 3, 7);
        *(uint4*)(a.dst + a.dst_off[1] + (size_t)r * a.dst_pitch[1] + 2 * kReconGroup * g) =
            make_uint4(__builtin_amdgcn_perm(v.x, u.x, lo), __builtin_amdgcn_perm(v.x, u.x, hi), __builtin_amdgcn_perm(v.y, u.y, lo), __builtin_amdgcn_perm(v.y, u.y, hi));
    } else {
        *(uint2*)(a.dst + a.dst_off[plane] + (size_t)r * a.dst_pitch[plane] + kReconGroup * g) = *(const uint2*)(a.rec[plane] + (size_t)r * sp + kReconGroup * g);
    }
}

} // namespace wrenc
