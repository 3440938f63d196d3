// dev_format.h -- conversion of an uploaded picture from the context's source format to the planar 8-bit 4:2:0 planes the
// rest of the library reads (include/wrenc_gpu.h: wrenc_gpu_set_source_format; the sample rules are defined in
// include/wrenc_format.h, in integers, and met bit for bit).  The upload copies the caller's RAW planes -- 16-bit words,
// interleaved CbCr, 4:2:2 rows, as they come -- into the context's raw staging planes; this kernel reads them and writes
// the source-size rectangle of the 8-bit planes: the scaler's staging planes when a source size is set (dev_scale.h
// runs next), else the visible rectangle of the slot's planes at the coded pitch (dev_pad.h then fills the margin).
//
// One launch covers the three planes.  A workgroup is 4 waves; a wave takes one row of one plane, so the plane, the row
// and with them every base address are scalar, and a lane makes kFormatGroup = 8 neighbouring output bytes of that row
// with one 8-byte store (an interleaved CbCr row: 8 bytes of Cb and 8 of Cr).  What a lane loads for them:
//   8-bit luma                    8 bytes
//   10-bit luma, 4:2:0 chroma     one 16-byte load
//   4:2:2 chroma                  rows 2j and 2j + 1: two 8-byte loads (8-bit), two 16-byte loads (10-bit)
//   nv12 CbCr                     one 16-byte load: 8 Cb and 8 Cr
//   p010le CbCr                   two 16-byte loads
// The arithmetic is packed 16-bit, two samples per dword (v_pk_min_u16, v_pk_add_u16, v_pk_lshrrev_b16), bytes are gathered
// with v_perm_b32; the 8-bit 4:2:2 mean is taken on four bytes of a dword at once.  Every clamp comes BEFORE its shift:
//     min((s + 2) >> 2, 255) = (min(s, 1021) + 2) >> 2           for s <= 1023
//     min((sa + sb + 4) >> 3, 255) = (min(sa + sb, 2043) + 4) >> 3   for sa, sb <= 1023
// (dev_scale.h: scale_clip8 tells what a shift followed by a clamp of neighbouring samples was compiled to).
//
// Alignment.  The library owns every pitch involved.  Raw staging rows are kFormatRawAlign = 32 bytes apart or a multiple,
// planes follow each other at pitch x rows, so lane g's loads at 8 g, 16 g or 32 g bytes of a row are aligned and, for the
// last lane of a row, may reach past the row's samples but not past its pitch: the allocation is pitch x rows.  The 8-bit
// destinations have the coded pitch W or W / 2 (W a multiple of 32) or the scaler's (a multiple of 16): 8-byte stores at
// 8 g are aligned.  Widths are only even (luma 34, 70; chroma 17, 35): where a row ends inside a lane's eight bytes they
// are stored one by one, so nothing is written outside the rectangle (the rule of scale_kernel's tail).
// No LDS, no division, no table.
#pragma once

#include "../../include/wrenc_format.h"

namespace wrenc {

constexpr int kFormatGroup = 8;      // output samples per lane
constexpr int kFormatRows = 4;       // rows (waves) per workgroup
constexpr int kFormatRawAlign = 32;  // raw staging pitch: a multiple of this
static_assert(kFormatRawAlign % 16 == 0 && kFormatRawAlign >= 2 * 2 * kFormatGroup,
              "a lane's widest read, 8 CbCr pairs of 16-bit words, is aligned and ends inside the row's pitch");
static_assert((32 / 2) % kFormatGroup == 0 && 16 % kFormatGroup == 0,
              "the coded chroma pitch (CTUs of 32) and the scaler's staging pitch keep 8-byte stores aligned");

__host__ __device__ inline size_t format_raw_pitch(size_t row_bytes) { return (row_bytes + kFormatRawAlign - 1) & ~(size_t)(kFormatRawAlign - 1); }

struct FormatArgs {
    const uint8_t* raw;     // the raw staging planes: one allocation
    uint8_t* dst;           // the 8-bit planes: a slot's originals (PicBufs::org[0]) or the scaler's staging planes
    size_t raw_off[3];      // byte offset of each raw plane ([2] unused by the two-plane formats)
    size_t dst_off[3];      // ... of Y, Cb, Cr in dst
    int raw_pitch[3];       // bytes, multiples of kFormatRawAlign
    int dst_pitch[2];       // luma and chroma
    int w, h;               // the picture: the context's source size
    int row_blocks[2];      // workgroups down a luma plane and down a chroma plane
};

typedef unsigned short FormatPk __attribute__((ext_vector_type(2)));

// two 16-bit words of a 10-bit format -> their two 10-bit values
template <bool HIGH>
__device__ __forceinline__ FormatPk format_s10(uint32_t v) {
    const FormatPk x = __builtin_bit_cast(FormatPk, v);
    if (HIGH) return x >> (unsigned short)6;
    return __builtin_elementwise_min(x, (FormatPk)(unsigned short)1023);
}
// ... -> two 8-bit samples, each in the low byte of its half
template <bool HIGH>
__device__ __forceinline__ uint32_t format_to8(uint32_t v) {
    const FormatPk s = __builtin_elementwise_min(format_s10<HIGH>(v), (FormatPk)(unsigned short)1021);
    return __builtin_bit_cast(uint32_t, (FormatPk)((s + (unsigned short)2) >> (unsigned short)2));
}
// the same of the mean of two rows (4:2:2, low-bit words)
__device__ __forceinline__ uint32_t format_mean10(uint32_t a, uint32_t b) {
    const FormatPk s = __builtin_elementwise_min((FormatPk)(format_s10<false>(a) + format_s10<false>(b)), (FormatPk)(unsigned short)2043);
    return __builtin_bit_cast(uint32_t, (FormatPk)((s + (unsigned short)4) >> (unsigned short)3));
}
// (a + b + 1) >> 1 of each of four bytes
__device__ __forceinline__ uint32_t format_mean8(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) >> 1) & 0x7F7F7F7Fu); }
// bytes 0 and 2 (1 and 3) of lo, then of hi
__device__ __forceinline__ uint32_t format_even(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x06040200u); }
__device__ __forceinline__ uint32_t format_odd(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x07050301u); }

template <bool HIGH>
__device__ __forceinline__ uint2 format_row10(const uint8_t* p) { // eight words -> eight bytes
    const uint4 v = *(const uint4*)p;
    return make_uint2(format_even(format_to8<HIGH>(v.x), format_to8<HIGH>(v.y)), format_even(format_to8<HIGH>(v.z), format_to8<HIGH>(v.w)));
}

// eight bytes at out, of which `left` (> 0) lie inside the row
__device__ __forceinline__ void format_store(uint8_t* out, uint2 v, int left) {
    if (left >= kFormatGroup) {
        *(uint2*)out = v;
    } else {
        for (int k = 0; k < left; ++k) out[k] = (uint8_t)((k < 4 ? v.x : v.y) >> (8 * (k & 3)));
    }
}

// F: the source format (wrenc_format.h), 1 .. 5.  Grid: x over groups of 64 lanes along a luma row, y over row_blocks[0]
// workgroups of luma rows, then row_blocks[1] of chroma rows once (interleaved: a lane makes Cb and Cr) or twice (planar).
template <int F>
__global__ __launch_bounds__(64 * kFormatRows) void convert_format_kernel(FormatArgs a) {
    static_assert(F >= 1 && F < WRENC_FORMAT_COUNT, "format 0 is the plain upload");
    constexpr bool kWide = F == WRENC_FORMAT_YUV420P10LE || F == WRENC_FORMAT_P010LE || F == WRENC_FORMAT_YUV422P10LE;
    constexpr bool kHigh = F == WRENC_FORMAT_P010LE;
    constexpr bool kPairs = F == WRENC_FORMAT_NV12 || F == WRENC_FORMAT_P010LE;
    constexpr bool k422 = F == WRENC_FORMAT_YUV422P || F == WRENC_FORMAT_YUV422P10LE;
    int by = (int)blockIdx.y, plane = 0;
    if (by >= a.row_blocks[0]) {
        by -= a.row_blocks[0];
        plane = 1;
        if (!kPairs && by >= a.row_blocks[1]) {
            by -= a.row_blocks[1];
            plane = 2;
        }
    }
    const int c = plane ? 1 : 0;
    const int g = (int)(blockIdx.x * 64 + threadIdx.x), r = by * kFormatRows + (int)threadIdx.y;
    const int left = (a.w >> c) - kFormatGroup * g;
    if (r >= (a.h >> c) || left <= 0) return;
    const int rp = a.raw_pitch[plane];
    const uint8_t* src = a.raw + a.raw_off[plane] + (size_t)(plane && k422 ? 2 * r : r) * rp;
    uint8_t* out = a.dst + a.dst_off[plane] + (size_t)r * a.dst_pitch[c] + kFormatGroup * g;
    if (!plane || (!kPairs && !k422)) { // a sample per sample
        const uint2 v = kWide ? format_row10<kHigh>(src + 16 * g) : *(const uint2*)(src + 8 * g);
        format_store(out, v, left);
    } else if (k422) {
        uint2 v;
        if (kWide) {
            const uint4 p = *(const uint4*)(src + 16 * g), q = *(const uint4*)(src + rp + 16 * g);
            v = make_uint2(format_even(format_mean10(p.x, q.x), format_mean10(p.y, q.y)), format_even(format_mean10(p.z, q.z), format_mean10(p.w, q.w)));
        } else {
            const uint2 p = *(const uint2*)(src + 8 * g), q = *(const uint2*)(src + rp + 8 * g);
            v = make_uint2(format_mean8(p.x, q.x), format_mean8(p.y, q.y));
        }
        format_store(out, v, left);
    } else { // CbCr pairs: n holds Cb0 Cr0 Cb1 Cr1 | ... as bytes
        uint4 n;
        if (kWide) {
            const uint4 p = *(const uint4*)(src + 32 * g), q = *(const uint4*)(src + 32 * g + 16);
            n = make_uint4(format_even(format_to8<kHigh>(p.x), format_to8<kHigh>(p.y)), format_even(format_to8<kHigh>(p.z), format_to8<kHigh>(p.w)),
                           format_even(format_to8<kHigh>(q.x), format_to8<kHigh>(q.y)), format_even(format_to8<kHigh>(q.z), format_to8<kHigh>(q.w)));
        } else {
            n = *(const uint4*)(src + 16 * g);
        }
        format_store(out, make_uint2(format_even(n.x, n.y), format_even(n.z, n.w)), left);
        format_store(out + (a.dst_off[2] - a.dst_off[1]), make_uint2(format_odd(n.x, n.y), format_odd(n.z, n.w)), left);
    }
}

} // namespace wrenc
