// dev_scale.h -- resampling of an uploaded picture from the context's source size to its visible size (include/wrenc_gpu.h:
// wrenc_gpu_set_source_size; the filter is defined in include/wrenc_scale.h, in integers, and met bit for bit).  The
// upload copies the caller's planes into the context's staging planes; this kernel writes the visible vw x vh rectangle
// of the slot's planes, at the coded pitch; dev_pad.h then fills the margin.
//
// One launch covers the three planes; a workgroup of 256 lanes makes one tile of kScaleTileW x kScaleTileH output
// samples of one plane in three steps:
//   load        the rows and columns of the staging plane that the tile's taps reach, into LDS: an item is one aligned dword
//               of one row (the staging pitch is a multiple of 16, the tile's first column a multiple of 4), consecutive
//               lanes along the row.  Row and column indices are clamped to the plane -- that is the filter's edge rule, and
//               it keeps every load inside the plane: a dword that reaches over either end of a row (source widths such as
//               70, 35 and 17 are no multiple of 4) is put together from single bytes at clamped columns.
//   horizontal  lane = output column, the four waves take the loaded rows in turn: sum k x over the column's taps (its
//               coefficients in registers, two per dword, for v_dot2_i32_i16) -> (sum + 32) >> 6 as int16 in LDS.
//   vertical    lane = four neighbouring columns of one output row: sum k t -> clip((sum + 2^17) >> 18) and one dword store;
//               where the visible width ends inside the dword (chroma 17, 35) the visible bytes are stored one by one, so
//               nothing is written outside the visible rectangle.
// The tables (first input index and 16 zero-padded coefficients per output sample, per axis and per luma / chroma) are built
// on the host once per context: no division here.  A tile reads staging samples and tables only and writes its own
// outputs only, so the result does not depend on the order of the tiles.
// LDS per workgroup: 96 x 288 input bytes + 96 x 64 int16 = 39 KB (four workgroups per CU); at 4:1 a tile uses 80 x 272 of
// the input part.
#pragma once
#include "scale_args.h" // ScaleAxis, ScaleArgs

namespace wrenc {

constexpr int kScaleTileW = 64, kScaleTileH = 16;
constexpr int kScaleSpanX = 288, kScaleSpanY = 96; // input columns / rows of a tile that the LDS holds
constexpr int kScaleCoefs = 16;                    // coefficients per output sample in the tables

__device__ __forceinline__ void scale_load_coefs(const int16_t* coef, int o, uint32_t cw[kScaleCoefs / 2]) {
    const uint4* p = (const uint4*)(coef + (size_t)o * kScaleCoefs);
    const uint4 a = p[0], b = p[1];
    cw[0] = a.x, cw[1] = a.y, cw[2] = a.z, cw[3] = a.w;
    cw[4] = b.x, cw[5] = b.y, cw[6] = b.z, cw[7] = b.w;
}

// clip(v >> 18, 0, 255).  Clamped first and then shifted as an unsigned value: written as a shift followed by the clamp,
// two neighbouring samples are compiled to one v_ashr_pk_u8_i32 whose result the compiler ORs with the other two bytes as
// if its upper half were zero, and on the device it was not (bytes 2 and 3 of every dword came out wrong).
__device__ __forceinline__ uint32_t scale_clip8(int v) { return (uint32_t)min(max(v, 0), (256 << 18) - 1) >> 18; }

__global__ __launch_bounds__(256) void scale_kernel(ScaleArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t in[kScaleSpanY * kScaleSpanX];
    __shared__ __attribute__((aligned(16))) int16_t mid[kScaleSpanY * kScaleTileW];
    int id = (int)blockIdx.x, plane = 0;
    if (id >= a.tiles[0]) {
        id -= a.tiles[0];
        plane = 1;
        if (id >= a.tiles[1]) {
            id -= a.tiles[1];
            plane = 2;
        }
    }
    const int c = plane ? 1 : 0;
    const ScaleAxis X = a.x[c], Y = a.y[c];
    const int ty = id / a.tiles_x[c], tx = id - ty * a.tiles_x[c];
    const int x0 = tx * kScaleTileW, y0 = ty * kScaleTileH;
    const int xb = X.tile_base[tx], yb = Y.tile_base[ty];
    const int tid = (int)threadIdx.x;

    // load: ny rows of nxd dwords from column xb (a multiple of 4, below 0 at the left edge) and row yb on
    const int nxd = (X.span + 3) >> 2, ny = Y.span;
    const uint8_t* src = a.src[plane];
    const int pitch = a.src_pitch[c];
    for (int it = tid; it < ny * nxd; it += 256) {
        const int r = it / nxd, d = it - r * nxd;
        const uint8_t* row = src + (size_t)min(max(yb + r, 0), Y.n_in - 1) * pitch;
        const int sx = xb + 4 * d;
        uint32_t v;
        if (sx >= 0 && sx + 3 < X.n_in) {
            v = *(const uint32_t*)(row + sx);
        } else {
            v = 0;
            for (int k = 0; k < 4; ++k) v |= (uint32_t)row[min(max(sx + k, 0), X.n_in - 1)] << (8 * k);
        }
        *(uint32_t*)(in + r * kScaleSpanX + 4 * d) = v;
    }
    __syncthreads();

    // horizontal: column x0 + lane of every loaded row
    {
        const int lx = tid & 63, ox = x0 + lx;
        if (ox < X.n_out) {
            uint32_t cw[kScaleCoefs / 2];
            scale_load_coefs(X.coef, ox, cw);
            const int off = X.first[ox] - xb;
            for (int r = tid >> 6; r < ny; r += 4) {
                const uint8_t* p = in + r * kScaleSpanX + off;
                int acc = 32;
#pragma unroll
                for (int j = 0; j < kScaleCoefs / 2; ++j)
                    if (2 * j < X.taps) acc = dot2(cw[j], (uint32_t)p[2 * j] | ((uint32_t)p[2 * j + 1] << 16), acc);
                mid[r * kScaleTileW + lx] = (int16_t)(acc >> 6);
            }
        }
    }
    __syncthreads();

    // vertical: columns x0 + gx .. + 3 of row y0 + (tid >> 4)
    {
        const int gx = (tid & 15) * 4, oy = y0 + (tid >> 4), left = X.n_out - (x0 + gx);
        if (oy < Y.n_out && left > 0) {
            uint32_t cw[kScaleCoefs / 2];
            scale_load_coefs(Y.coef, oy, cw);
            const int16_t* p = mid + (Y.first[oy] - yb) * kScaleTileW + gx;
            int acc0 = 1 << 17, acc1 = 1 << 17, acc2 = 1 << 17, acc3 = 1 << 17;
#pragma unroll
            for (int j = 0; j < kScaleCoefs / 2; ++j)
                if (2 * j < Y.taps) {
                    const uint2 m0 = *(const uint2*)(p + (2 * j) * kScaleTileW), m1 = *(const uint2*)(p + (2 * j + 1) * kScaleTileW);
                    acc0 = dot2(cw[j], (m0.x & 0xFFFFu) | (m1.x << 16), acc0);
                    acc1 = dot2(cw[j], (m0.x >> 16) | (m1.x & 0xFFFF0000u), acc1);
                    acc2 = dot2(cw[j], (m0.y & 0xFFFFu) | (m1.y << 16), acc2);
                    acc3 = dot2(cw[j], (m0.y >> 16) | (m1.y & 0xFFFF0000u), acc3);
                }
            const uint32_t v = scale_clip8(acc0) | (scale_clip8(acc1) << 8) | (scale_clip8(acc2) << 16) | (scale_clip8(acc3) << 24);
            const size_t wh = (size_t)a.W * a.H;
            uint8_t* out = a.dst + (plane ? wh + (size_t)(plane - 1) * (wh >> 2) : 0) + (size_t)oy * (a.W >> c) + x0 + gx;
            if (left >= 4) {
                *(uint32_t*)out = v;
            } else { // the visible width ends inside the dword: one to three bytes
                out[0] = (uint8_t)v;
                if (left > 1) out[1] = (uint8_t)(v >> 8);
                if (left > 2) out[2] = (uint8_t)(v >> 16);
            }
        }
    }
}

} // namespace wrenc
