// dev_complexity.h -- how hard a picture is to code, from its uploaded originals alone (include/wrenc_gpu.h:
// wrenc_gpu_download_complexity): per picture-aligned 8x8 block of every plane the unnormalised 2-D Hadamard transform
// (the +-1 matrix) of its 64 samples and act = sum |coefficient| over the 63 coefficients other than DC; per picture the
// planes' sums, and per CTU the sum over its 16 luma, 4 Cb and 4 Cr blocks.  All integers, all exact: act <= 130,560.
//
// Layout.  A lane owns TWO blocks at a time, one in each 16-bit half of its registers, so that all six butterfly stages
// of the 64-point transform are register-to-register v_pk_add_i16 / v_pk_sub_i16 (a coefficient is at most 64 x 255 =
// 16,320) and none crosses the halves: in the luma plane the block and the one below it, in the chroma planes the Cb and
// the Cr block at one position.  Per block a lane loads eight rows of 8 bytes (global_load_dwordx2, 512 contiguous bytes
// per wave instruction), nothing goes through LDS.  A wave is a STRIP of 16 CTUs (512 luma samples) of one CTU row: two
// rounds of luma (block rows 0 | 1 and 2 | 3 of the CTUs, lane = block column) and one of chroma (lanes 0..31 the upper,
// 32..63 the lower chroma block row, lane & 31 = block column), 24 KiB read once.  The last butterfly stage is never
// formed: |a + b| + |a - b| = 2 max(|a|, |b|), and of the pair that holds DC (= a + b >= 0) only |a - b| counts.
// Lanes beyond the plane's last block read that block again (no traffic, no divergent load) and own nothing.
// Every wave stores the 16 CTU sums of its strip and one {Y, Cb, Cr} triple at its own index; complexity_finish_kernel
// adds a picture's triples in index order: no atomics, the same figures in any slot, batch and run.
#pragma once

namespace wrenc {

constexpr int kCplxCtus = 16; // CTUs of a wave's strip

struct ComplexityPartial { // one wave, and (after the finish kernel) one picture: Y, Cb, Cr
    unsigned long long satd[3];
};

// waves per picture: CTU rows x strips
__host__ __device__ inline int cplx_strips(int W) { return ((W >> 5) + kCplxCtus - 1) / kCplxCtus; }
__host__ __device__ inline int cplx_waves(int W, int H) { return (H >> 5) * cplx_strips(W); }

typedef short Pk16 __attribute__((ext_vector_type(2)));
typedef unsigned short PkU16 __attribute__((ext_vector_type(2)));
typedef uint32_t Dwords2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) Dwords2* GlobalRow8;

struct BlockRows { // the 8 x 8 samples of two blocks
    Dwords2 a[8], b[8];
};
__device__ __forceinline__ void load_block_rows(BlockRows& r, const uint8_t* pa, const uint8_t* pb, int pitch) {
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        r.a[y] = *(GlobalRow8)(pa + (size_t)y * pitch);
        r.b[y] = *(GlobalRow8)(pb + (size_t)y * pitch);
    }
}

// act of block a (low 16 bits) and of block b (high 16 bits); each <= 130,560 does not fit 16 bits, so two words
__device__ __forceinline__ void act_pair(const BlockRows& r, uint32_t& act_a, uint32_t& act_b) {
    Pk16 v[64];
#pragma unroll
    for (int y = 0; y < 8; ++y)
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            // [a's sample, 0, b's sample, 0]
            const uint32_t sel = 0x0c040c00u | (uint32_t)(x & 3) << 16 | (uint32_t)(x & 3);
            v[8 * y + x] = __builtin_bit_cast(Pk16, __builtin_amdgcn_perm(r.b[y][x >> 2], r.a[y][x >> 2], sel));
        }
#pragma unroll
    for (int h = 1; h < 32; h <<= 1)
#pragma unroll
        for (int i = 0; i < 64; ++i)
            if (!(i & h)) {
                const Pk16 p = v[i], q = v[i | h];
                v[i] = p + q;
                v[i | h] = p - q;
            }
    // stage h = 32 folded into the sum: inputs within +-8160, so eight maxima fit 16 bits; the total is doubled at the end
    act_a = act_b = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        PkU16 part = {0, 0};
#pragma unroll
        for (int i = 8 * c; i < 8 * c + 8; ++i) {
            if (i == 0) continue; // the DC pair, below
            const Pk16 m = __builtin_elementwise_max(__builtin_elementwise_abs(v[i]), __builtin_elementwise_abs(v[i + 32]));
            part += __builtin_bit_cast(PkU16, m);
        }
        const uint32_t w = __builtin_bit_cast(uint32_t, part);
        act_a += w & 0xFFFFu;
        act_b += w >> 16;
    }
    const uint32_t dc = __builtin_bit_cast(uint32_t, __builtin_elementwise_abs(v[0] - v[32]));
    act_a = 2 * act_a + (dc & 0xFFFFu);
    act_b = 2 * act_b + (dc >> 16);
}

// One wave per (picture, CTU row, strip of kCplxCtus CTUs).  ctu_map: n_pics x CTUs of a picture, raster order.
__global__ __launch_bounds__(256) void complexity_kernel(const PicBufs* __restrict__ slots, int first_slot, int n_pics, int W, int H,
                                                         ComplexityPartial* __restrict__ partials, uint32_t* __restrict__ ctu_map) {
    const int strips = cplx_strips(W), per_pic = cplx_waves(W, H);
    const int id = uni((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (id >= n_pics * per_pic) return; // (the whole wave)
    const int pic = id / per_pic, rem = id - pic * per_pic;
    const int ctu_y = rem / strips, strip = rem - ctu_y * strips;
    const PicBufs& pb = slots[first_slot + pic];
    const uint8_t* org_y = pb.org[0];
    const uint8_t* org_cb = pb.org[1];
    const uint8_t* org_cr = pb.org[2];
    const int lane = (int)(threadIdx.x & 63);
    const int ctu_cols = W >> 5, cw = W >> 1;

    // luma: lane = block column of the strip
    const int bx = strip * (4 * kCplxCtus) + lane;
    const bool own_y = bx < (W >> 3);
    const uint8_t* py = org_y + (size_t)(32 * ctu_y) * W + 8 * min(bx, (W >> 3) - 1);
    // chroma: lane & 31 = block column, lane >> 5 = block row of the CTU row
    const int cx = strip * (2 * kCplxCtus) + (lane & 31);
    const bool own_c = cx < (W >> 4);
    const size_t c_at = (size_t)(16 * ctu_y + 8 * (lane >> 5)) * cw + 8 * min(cx, (W >> 4) - 1);

    BlockRows r0, r1, r2;
    load_block_rows(r0, py, py + (size_t)8 * W, W);
    load_block_rows(r1, py + (size_t)16 * W, py + (size_t)24 * W, W);
    load_block_rows(r2, org_cb + c_at, org_cr + c_at, cw);
    uint32_t y0, y1, y2, y3, cb, cr;
    act_pair(r0, y0, y1);
    act_pair(r1, y2, y3);
    act_pair(r2, cb, cr);
    uint32_t sum_y = own_y ? y0 + y1 + y2 + y3 : 0u; // <= 4 x 130,560
    const uint32_t sum_cb = own_c ? cb : 0u, sum_cr = own_c ? cr : 0u;

    // the CTUs of the strip: luma lanes 4c .. 4c + 3, chroma lanes 2c, 2c + 1, 32 + 2c, 33 + 2c
    uint32_t ctu_l = sum_y;
    ctu_l += (uint32_t)__shfl_xor((int)ctu_l, 1, 64);
    ctu_l += (uint32_t)__shfl_xor((int)ctu_l, 2, 64);
    uint32_t ctu_c = sum_cb + sum_cr;
    ctu_c += (uint32_t)__shfl_xor((int)ctu_c, 1, 64);
    ctu_c += (uint32_t)__shfl_xor((int)ctu_c, 32, 64);
    const uint32_t ctu_sum = ctu_l + (uint32_t)__shfl((int)ctu_c, lane >> 1, 64);
    const int ctu_x = strip * kCplxCtus + (lane >> 2);
    if ((lane & 3) == 0 && ctu_x < ctu_cols) ctu_map[(size_t)pic * ctu_cols * (H >> 5) + (size_t)ctu_y * ctu_cols + ctu_x] = ctu_sum;

    // the wave's triple (a lane holds at most 522,240: 32 bits suffice for the wave)
    uint32_t s0 = sum_y, s1 = sum_cb, s2 = sum_cr;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        s0 += (uint32_t)__shfl_xor((int)s0, d, 64);
        s1 += (uint32_t)__shfl_xor((int)s1, d, 64);
        s2 += (uint32_t)__shfl_xor((int)s2, d, 64);
    }
    if (lane == 0) partials[id] = ComplexityPartial{{s0, s1, s2}};
}

// A picture's triples added up in index order, one thread per plane.
__global__ __launch_bounds__(64) void complexity_finish_kernel(const ComplexityPartial* __restrict__ partials, int W, int H,
                                                               ComplexityPartial* __restrict__ sums) {
    const int plane = (int)threadIdx.x;
    if (plane >= 3) return;
    const int count = cplx_waves(W, H);
    const ComplexityPartial* p = partials + (size_t)blockIdx.x * count;
    unsigned long long s = 0;
    for (int i = 0; i < count; ++i) s += p[i].satd[plane];
    sums[blockIdx.x].satd[plane] = s;
}

} // namespace wrenc
