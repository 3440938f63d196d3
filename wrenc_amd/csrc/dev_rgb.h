// dev_rgb.h -- conversion of an uploaded RGB picture to the planar 8-bit 4:2:0 Y'CbCr planes the rest of the library reads
// (include/wrenc_gpu.h: wrenc_gpu_set_source_rgb; the rules are defined in include/wrenc_rgb.h, in integers, and met bit for
// bit).  It stands where dev_format.h's converter stands: the upload copies the caller's RAW planes into the context's raw
// staging planes; this kernel reads them and writes the source-size rectangle of the 8-bit planes: the scaler's staging
// planes when a source size is set, else the visible rectangle of the slot's planes at the coded pitch.
//
// One launch per picture.  A workgroup is 4 waves; a wave takes one PAIR of luma rows, so the rows and every base address
// are scalar, and a lane makes kRgbGroup = 8 neighbouring luma samples of each of the two rows (two 8-byte stores) and the
// 4 Cb and 4 Cr samples below them (two 4-byte stores).  What a lane loads per row:
//   rgb24 / bgr24   24 bytes at 24 g: three 8-byte loads
//   rgb0 / bgr0     32 bytes at 32 g: two 16-byte loads
//   gbrp            8 bytes at 8 g of each of the three planes
// A pixel becomes two dwords by v_perm_b32: (R | G << 16) and (B | 0 << 16), 16-bit lanes with the high byte zero; the bgr
// layouts have another selector, not a branch.  Luma is v_dot2_i32_i16 of (R, G) with (yr, yg) on top of the rounding
// constant, then one more of (B, 0) with (yb, 0): products reach 255 * 11718, the accumulator is 32-bit.  The four pixels of
// a 2x2 block are summed as dwords -- 4 * 255 stays inside a 16-bit lane -- and chroma is the same two dots on the sums
// (1020 * 8192).
// Luma needs no clip: with coefficients that sum to round(sy 2^14) it lies in yoff .. yoff + 219 or 0 .. 255.  Chroma never
// falls below 1 but reaches 256 (pc, pure blue or red): one min.  The nine coefficients and yoff are kernel arguments.
//
// Alignment and bounds.  The library owns every pitch involved.  A raw staging row is rgb_raw_pitch() long: room for what
// every lane with a sample in the row reads (24, 32 or 8 bytes times ceil(w / 8)), rounded up to kFormatRawAlign; the
// allocation is pitch x rows, so the last lane's loads may reach past the row's samples but not past its pitch.  The 8-bit
// destinations are dev_format.h's: 8-byte luma stores at 8 g and 4-byte chroma stores at 4 g are aligned.  Where a row
// ends inside a lane's eight samples they are stored one by one (format_store): nothing is written outside the rectangle.
// No LDS, no table, no division.
#pragma once

#include "../../include/wrenc_rgb.h"
#include "dev_format.h"

namespace wrenc {

constexpr int kRgbGroup = kFormatGroup; // luma samples per lane and row
constexpr int kRgbRows = 4;             // row pairs (waves) per workgroup

// bytes a lane reads of one row of one raw plane
__host__ __device__ constexpr int rgb_lane_bytes(int layout) { return layout == WRENC_RGB_GBRP ? kRgbGroup : layout >= WRENC_RGB_RGB0 ? 4 * kRgbGroup : 3 * kRgbGroup; }
__host__ __device__ inline size_t rgb_raw_pitch(int layout, int w) {
    return format_raw_pitch((size_t)rgb_lane_bytes(layout) * (size_t)((w + kRgbGroup - 1) / kRgbGroup));
}

struct RgbArgs {
    const uint8_t* raw;   // the raw staging planes: one allocation
    uint8_t* dst;         // the 8-bit planes: a slot's originals (PicBufs::org[0]) or the scaler's staging planes
    size_t raw_off[3];    // byte offset of each raw plane (packed layouts: [0] alone)
    size_t dst_off[3];    // ... of Y, Cb, Cr in dst
    int raw_pitch;        // bytes, a multiple of kFormatRawAlign; the three planes of gbrp share it
    int dst_pitch[2];     // luma and chroma
    int w, h;             // the picture: the context's source size
    int k[10];            // wrenc_rgb_coefficients: yr yg yb | br bg bb | rr rg rb | yoff
};

__device__ __forceinline__ uint32_t rgb_pack16(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }

// the selector that puts byte `a` of the eight bytes hi:lo into byte 0 and byte `b` into byte 2, zeros between (b < 0: zero)
__host__ __device__ constexpr uint32_t rgb_sel(int a, int b) { return (uint32_t)a | 0x0C00u | ((b < 0 ? 0x0Cu : (uint32_t)b) << 16) | 0x0C000000u; }

// eight pixels of one row at `src` (the lane's bytes of plane 0; gbrp: the planes are `plane` bytes apart):
// rg[k] = R | G << 16, b[k] = B
template <int L>
__device__ __forceinline__ void rgb_load_row(const uint8_t* src, size_t plane, uint32_t rg[kRgbGroup], uint32_t b[kRgbGroup]) {
    constexpr bool kSwap = L == WRENC_RGB_BGR24 || L == WRENC_RGB_BGR0;
    constexpr int kR = kSwap ? 2 : 0, kB = kSwap ? 0 : 2;
    if (L == WRENC_RGB_GBRP) {
        const uint2 gg = *(const uint2*)src, bb = *(const uint2*)(src + plane), rr = *(const uint2*)(src + 2 * plane);
#pragma unroll
        for (int k = 0; k < kRgbGroup; ++k) {
            const uint32_t gd = k < 4 ? gg.x : gg.y, bd = k < 4 ? bb.x : bb.y, rd = k < 4 ? rr.x : rr.y;
            rg[k] = __builtin_amdgcn_perm(gd, rd, rgb_sel(k & 3, 4 + (k & 3)));
            b[k] = __builtin_amdgcn_perm(0u, bd, rgb_sel(k & 3, -1));
        }
    } else if (L == WRENC_RGB_RGB0 || L == WRENC_RGB_BGR0) {
        const uint4 p = *(const uint4*)src, q = *(const uint4*)(src + 16);
        const uint32_t d[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < kRgbGroup; ++k) {
            rg[k] = __builtin_amdgcn_perm(0u, d[k], rgb_sel(kR, 1));
            b[k] = __builtin_amdgcn_perm(0u, d[k], rgb_sel(kB, -1));
        }
    } else {
        const uint2 p = *(const uint2*)src, q = *(const uint2*)(src + 8), r = *(const uint2*)(src + 16);
        const uint32_t d[6] = {p.x, p.y, q.x, q.y, r.x, r.y};
#pragma unroll
        for (int k = 0; k < kRgbGroup; ++k) { // pixel k: bytes 3k .. 3k + 2, inside dwords i and i + 1
            const int i = 3 * k / 4, o = 3 * k % 4;
            const uint32_t lo = d[i], hi = d[i + 1 < 6 ? i + 1 : 5];
            rg[k] = __builtin_amdgcn_perm(hi, lo, rgb_sel(o + kR, o + 1));
            b[k] = __builtin_amdgcn_perm(hi, lo, rgb_sel(o + kB, -1));
        }
    }
}

// L: the layout (wrenc_rgb.h).  Grid: x over groups of 64 lanes along a luma row, y over workgroups of kRgbRows row pairs.
template <int L>
__global__ __launch_bounds__(64 * kRgbRows) void convert_rgb_kernel(RgbArgs a) {
    static_assert(L >= 0 && L < WRENC_RGB_COUNT, "a layout of wrenc_rgb.h");
    const int g = (int)(blockIdx.x * 64 + threadIdx.x), rp = (int)blockIdx.y * kRgbRows + (int)threadIdx.y;
    const int left = a.w - kRgbGroup * g;
    if (rp >= (a.h >> 1) || left <= 0) return;
    // coefficient pairs for (R, G) and for (B, 0)
    const uint32_t ky = rgb_pack16(a.k[0], a.k[1]), kb = rgb_pack16(a.k[3], a.k[4]), kr = rgb_pack16(a.k[6], a.k[7]);
    const uint32_t ky_b = rgb_pack16(a.k[2], 0), kb_b = rgb_pack16(a.k[5], 0), kr_b = rgb_pack16(a.k[8], 0);
    const int y_round = (a.k[9] << 14) + (1 << 13), c_round = (128 << 16) + (1 << 15);
    const size_t plane = (size_t)a.raw_pitch * (size_t)a.h; // gbrp: from one raw plane to the next
    const uint8_t* src = a.raw + a.raw_off[0] + (size_t)(2 * rp) * a.raw_pitch + (size_t)rgb_lane_bytes(L) * g;
    uint8_t* out = a.dst + a.dst_off[0] + (size_t)(2 * rp) * a.dst_pitch[0] + kRgbGroup * g;
    uint32_t rg[2][kRgbGroup], b[2][kRgbGroup];
    rgb_load_row<L>(src, plane, rg[0], b[0]);
    rgb_load_row<L>(src + a.raw_pitch, plane, rg[1], b[1]);
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        uint32_t y[kRgbGroup];
#pragma unroll
        for (int k = 0; k < kRgbGroup; ++k) y[k] = (uint32_t)dot2(b[row][k], ky_b, dot2(rg[row][k], ky, y_round)) >> 14;
        const uint2 v = make_uint2(y[0] | y[1] << 8 | y[2] << 16 | y[3] << 24, y[4] | y[5] << 8 | y[6] << 16 | y[7] << 24);
        format_store(out + (size_t)row * a.dst_pitch[0], v, left);
    }
    uint32_t cb = 0, cr = 0;
#pragma unroll
    for (int j = 0; j < kRgbGroup / 2; ++j) {
        const uint32_t srg = rg[0][2 * j] + rg[0][2 * j + 1] + rg[1][2 * j] + rg[1][2 * j + 1];
        const uint32_t sb = b[0][2 * j] + b[0][2 * j + 1] + b[1][2 * j] + b[1][2 * j + 1];
        const int u = dot2(sb, kb_b, dot2(srg, kb, c_round)) >> 16, v = dot2(sb, kr_b, dot2(srg, kr, c_round)) >> 16;
        cb |= (uint32_t)(u < 255 ? u : 255) << (8 * j);
        cr |= (uint32_t)(v < 255 ? v : 255) << (8 * j);
    }
    const int left_c = left >> 1; // w is even and a lane starts at a multiple of 8: whole chroma samples
    uint8_t* out_cb = a.dst + a.dst_off[1] + (size_t)rp * a.dst_pitch[1] + (kRgbGroup / 2) * g;
    uint8_t* out_cr = a.dst + a.dst_off[2] + (size_t)rp * a.dst_pitch[1] + (kRgbGroup / 2) * g;
    if (left_c >= kRgbGroup / 2) {
        *(uint32_t*)out_cb = cb;
        *(uint32_t*)out_cr = cr;
    } else {
        for (int k = 0; k < left_c; ++k) {
            out_cb[k] = (uint8_t)(cb >> (8 * k));
            out_cr[k] = (uint8_t)(cr >> (8 * k));
        }
    }
}

} // namespace wrenc
