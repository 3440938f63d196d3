// dev_transform.h -- forward and inverse DCT-2 4..32 (transformer.rs)
// Part of the gfx950 device code of the RD-search path; see wrenc_dev.h for the overall model.
#pragma once

namespace wrenc {

// ---------------------------------------------------------------------------
// DCT-2 (transformer.rs).  Lane u = lane % N owns basis row T_N[u][.] in
// registers; G = 64/N lane groups walk the rows/columns; the other operand is
// read from LDS as a wave-broadcast.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int acc) { // v_dot2_i32_i16
    typedef short s2 __attribute__((ext_vector_type(2)));
    s2 va, vb;
    va.x = (short)(a & 0xFFFF);
    va.y = (short)(a >> 16);
    vb.x = (short)(b & 0xFFFF);
    vb.y = (short)(b >> 16);
    return __builtin_amdgcn_sdot2(va, vb, acc, false);
}

// forward: nb residual blocks in r1 ([blk][y][x] i16) -> coefficients in place, via r2;
// transformer.rs:2040-2378.  The i32 intermediate of all nb blocks goes through r2 at once when it fits its
// 2 KB, block after block otherwise (the two 16x16 blocks of a 32x32 CU's chroma pair).
// h: the intermediate's buffer of HBYTES bytes in LDS (r2 in the search; the micro-benchmark of the 32x32 v_dot2
// version brings its own, wrenc_gpu_test.hip).
template <int LG, int HBYTES>
__device__ void fwd_dct(Ctx c, int nb, int o1, LDS_AS int32_t* h) {
    constexpr int N = 1 << LG;
    constexpr int G = 64 / N;
    constexpr int HS = N + 1; // row stride of the intermediate
    const int u = LANE & (N - 1);
    const int g = LANE >> LG;
    uint32_t t[N / 2];
    {
        const CONST_AS uint32_t* src = (const CONST_AS uint32_t*)&c.k->dct[LG - 2][u][0];
#pragma unroll
        for (int k = 0; k < N / 2; ++k) t[k] = src[k];
    }
    constexpr int kFit = HBYTES / (N * HS * (int)sizeof(int32_t)); // blocks whose intermediate fits the buffer
    static_assert(kFit >= 1, "one block's stage-1 output must fit the buffer");
    const int per = nb <= kFit ? nb : 1; // blocks per round
#pragma unroll 1
    for (int b0 = 0; b0 < nb; b0 += per) {
        // stage 1: H[u][y] = (sum_x T[u][x] r[y][x] + d) >> (LG-1)   (:2139-2209); rows of the round's blocks
WRENC_UNROLL(WRENC_U_DCT)
        for (int yy = g; yy < per * N; yy += G) {
            const uint32_t* row = (const uint32_t*)&SH.r1[o1 + (b0 * N + yy) * N];
            int acc = 0;
#pragma unroll
            for (int k = 0; k < N / 2; ++k) acc = dot2(row[k], t[k], acc);
            const int blk = yy >> LG, y = yy & (N - 1);
            h[blk * (N * HS) + u * HS + y] = (acc + (1 << (LG - 2))) >> (LG - 1);
        }
        WSYNC();
        // stage 2: C[v][x] = (sum_y T[v][y] H[x][y] + d) >> (LG+6)  (:2246-2316); lane v = u
WRENC_UNROLL(WRENC_U_DCT)
        for (int xx = g; xx < per * N; xx += G) {
            const int blk = xx >> LG, x = xx & (N - 1);
            const LDS_AS int32_t* col = &h[blk * (N * HS) + x * HS];
            int acc = 0;
#pragma unroll
            for (int k = 0; k < N / 2; ++k) {
                // |T| <= 90 and |H| <= 46410: 24-bit multiplies are exact (v_mad_i32_i24)
                acc += __mul24((int)(short)(t[k] & 0xFFFF), col[2 * k]);
                acc += __mul24((int)t[k] >> 16, col[2 * k + 1]);
            }
            SH.r1[o1 + (b0 + blk) * (N * N) + u * N + x] = (int16_t)((acc + (1 << (LG + 5))) >> (LG + 6));
        }
        WSYNC();
    }
}

// inverse: nb transposed dequantised blocks in r2 ([blk][x][i], i16) -> residuals r1 ([blk][y][x]).  The
// intermediate V takes the place of the levels in r1 (dead once dequantised) and the second stage runs in
// place: a row of V is read whole by the 2^LG lanes that then write that row, and no other lane touches it.
// transformer.rs:2380-2737
template <int LG>
__device__ void inv_dct(Ctx c, int nb, int o1) {
    constexpr int N = 1 << LG;
    constexpr int G = 64 / N;
    const int u = LANE & (N - 1);
    const int g = LANE >> LG;
    const int16_t* dqt = (const int16_t*)SH.r2;
    int16_t* vbuf = SH.r1 + o1;
    uint32_t t[N / 2]; // Tt[u][i] = T_N[i][u]
    {
        const CONST_AS uint32_t* src = (const CONST_AS uint32_t*)&c.k->dct_t[LG - 2][u][0];
#pragma unroll
        for (int k = 0; k < N / 2; ++k) t[k] = src[k];
    }
    // stage 1 (vertical): V[y][x] = clamp16((sum_i T[i][y] d[i][x] + 64) >> 7); lane y = u
WRENC_UNROLL(WRENC_U_DCT)
    for (int xx = g; xx < nb * N; xx += G) {
        const uint32_t* col = (const uint32_t*)&dqt[xx * N]; // dT[blk][x][.]
        int acc = 0;
#pragma unroll
        for (int k = 0; k < N / 2; ++k) acc = dot2(col[k], t[k], acc);
        int v = (acc + 64) >> 7;
        v = min(max(v, -32768), 32767);
        const int blk = xx >> LG, x = xx & (N - 1);
        vbuf[blk * (N * N) + u * N + x] = (int16_t)v;
    }
    WSYNC();
    // stage 2 (horizontal): r[y][x] = (sum_i T[i][x] V[y][i] + 2048) >> 12; lane x = u
WRENC_UNROLL(WRENC_U_DCT)
    for (int yy = g; yy < nb * N; yy += G) {
        const uint32_t* row = (const uint32_t*)&vbuf[yy * N];
        uint32_t rv[N / 2];
#pragma unroll
        for (int k = 0; k < N / 2; ++k) rv[k] = row[k];
        WSYNC(); // the whole row is in registers before any lane overwrites an element of it
        int acc = 0;
#pragma unroll
        for (int k = 0; k < N / 2; ++k) acc = dot2(rv[k], t[k], acc);
        vbuf[yy * N + u] = (int16_t)((acc + 2048) >> 12);
    }
    WSYNC();
}

// ---------------------------------------------------------------------------
// MFMA EXPERIMENT (north_star: "MFMA tried only for the 32x32 separable int16 transform and kept only if
// rocprof shows a real win"): the forward 32x32 DCT-2 (transformer.rs:2040-2378) as five
// v_mfma_i32_32x32x32_i8.  Exact integer arithmetic: the basis fits signed bytes, the other operand is split
// into balanced base-256 digits (v = d0 + 256 d1 + 65536 d2, d0, d1 in [-128, 127]), one MFMA per digit,
// i32 accumulators recombined with shifts.
//   stage 1: Ht[y][u] = sum_x R[y][x] T[u][x]      A = digits of R (9 bits: 2 digits), B = T
//   stage 2: C[v][u]  = sum_y T[v][y] H[u][y]      A = T in accumulator k order, B = digits of Ht (17 bits: 3)
// The first stage's accumulators ARE the second stage's B operand (same lane, same k set), so the intermediate
// never goes through LDS.  wrenc_gpu_test_fwd_dct32 is its parity gate and micro-benchmark (tools/dct_bench.py)
// against the v_dot2 version (fwd_dct<5>); measurements and the decision to keep it in DESIGN.md.
// ---------------------------------------------------------------------------
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v16i_t __attribute__((ext_vector_type(16)));
typedef short s2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_digit1(uint32_t p) { // per i16 half: (v + 128) >> 8, arithmetic
    s2_t v;
    v.x = (short)(p & 0xFFFF);
    v.y = (short)(p >> 16);
    v = (v + (short)128) >> 8;
    return (uint32_t)(unsigned short)v.x | ((uint32_t)(unsigned short)v.y << 16);
}
// bytes b of four dwords -> one dword (byte k from dword k)
__device__ __forceinline__ uint32_t gather_byte(uint32_t a, uint32_t b, uint32_t c, uint32_t d, int byte) {
    const uint32_t sel = 0x0C0C0400u + 0x0101u * (uint32_t)byte; // [b(lo src), b(hi src), 0, 0]
    const uint32_t ab = __builtin_amdgcn_perm(b, a, sel);
    const uint32_t cd = __builtin_amdgcn_perm(d, c, sel);
    return __builtin_amdgcn_perm(cd, ab, 0x05040100u);           // [ab.b0, ab.b1, cd.b0, cd.b1]
}

__device__ __forceinline__ void fwd_dct32_mfma(Ctx c, int o1) {
    const int r = LANE & 31, h = LANE >> 5;
    const v4i_t tA = *(const CONST_AS v4i_t*)&c.k->dct32_a[r][16 * h];
    const v4i_t tP = *(const CONST_AS v4i_t*)&c.k->dct32_p[r][h][0];
    // ---- stage 1 ----
    const uint4 q0 = *(const uint4*)&SH.r1[o1 + r * 32 + 16 * h];
    const uint4 q1 = *(const uint4*)&SH.r1[o1 + r * 32 + 16 * h + 8];
    const uint32_t p[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    v4i_t lo, hi;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        lo[i] = (int)__builtin_amdgcn_perm(p[2 * i + 1], p[2 * i], 0x06040200u); // byte 0 of the four i16
        hi[i] = (int)__builtin_amdgcn_perm(pk_digit1(p[2 * i + 1]), pk_digit1(p[2 * i]), 0x06040200u);
    }
    // one accumulator set, digit after digit from the top: acc = (acc << 8) + digit product (16 live registers
    // instead of one set per digit: the search kernel has no registers to spare)
    v16i_t z = {};
    v16i_t acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(hi, tA, z, 0, 0, 0);
#pragma unroll
    for (int w = 0; w < 16; ++w) acc[w] = (acc[w] << 8) + (1 << 3); // (h + (1 << (LG - 2))) >> (LG - 1), LG = 5 (:2201-2209)
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(lo, tA, acc, 0, 0, 0);
    int H[16]; // Ht[y(w, h)][u = r], y(w, h) = 8 (w / 4) + 4 h + w % 4
#pragma unroll
    for (int w = 0; w < 16; ++w) H[w] = acc[w] >> 4;
    // ---- stage 2: digits of H straight from the registers ----
    v4i_t d0, d1, d2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t a = (uint32_t)H[4 * i], b = (uint32_t)H[4 * i + 1], cc = (uint32_t)H[4 * i + 2], d = (uint32_t)H[4 * i + 3];
        d0[i] = (int)gather_byte(a, b, cc, d, 0);                                     // sext8(v)
        d1[i] = (int)gather_byte(a + 128u, b + 128u, cc + 128u, d + 128u, 1);         // byte 1 of v + 128
        d2[i] = (int)gather_byte(a + 32896u, b + 32896u, cc + 32896u, d + 32896u, 2); // byte 2 of v + 128 + 32768
    }
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(tP, d2, z, 0, 0, 0);
#pragma unroll
    for (int w = 0; w < 16; ++w) acc[w] <<= 8;
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(tP, d1, acc, 0, 0, 0);
#pragma unroll
    for (int w = 0; w < 16; ++w) acc[w] = (acc[w] << 8) + (1 << 10); // (+ (1 << (LG + 5))) >> (LG + 6) (:2309-2316)
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(tP, d0, acc, 0, 0, 0);
    WSYNC(); // every lane has read its residuals before the coefficients overwrite them
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int v = 8 * (w >> 2) + 4 * h + (w & 3);
        SH.r1[o1 + v * 32 + r] = (int16_t)(acc[w] >> 11);
    }
    WSYNC();
}

// The inverse 32x32 transform (transformer.rs:2380-2737) the same way, four MFMAs.  16-bit operands (the dequantised
// coefficients, the clipped intermediate) go in as two bytes each: the signed high byte and the low byte minus 128
// (v = 256 hi + (lo - 128) + 128), so every product sum is short by 128 * sum_i T[i][n], a per-output constant that
// comes back together with the rounding offset (DevConst::idct32_k1 / k2).
//   stage 1: Vt[x][y] = sum_i dT[x][i] T[i][y]      A = bytes of the transposed dequantised block (r2), B = T
//   stage 2: Rt[x][y] = sum_i T[i][x] V[y][i]       A = T in accumulator k order, B = bytes of V straight from the
//                                                   first stage's accumulators (same lane, same k set)
// Residuals to r1[o1 ..] ([y][x]); nothing goes through LDS in between.
__device__ __forceinline__ void inv_dct32_mfma(Ctx c, int o1) {
    const int r = LANE & 31, h = LANE >> 5;
    const v4i_t tB = *(const CONST_AS v4i_t*)&c.k->idct32_b[r][16 * h];
    const v4i_t tP = *(const CONST_AS v4i_t*)&c.k->idct32_p[r][h][0];
    const int k1 = c.k->idct32_k1[r];
    // ---- stage 1 ----
    const int16_t* dqt = (const int16_t*)SH.r2;
    const uint4 q0 = *(const uint4*)&dqt[r * 32 + 16 * h];
    const uint4 q1 = *(const uint4*)&dqt[r * 32 + 16 * h + 8];
    const uint32_t p[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    v4i_t lo, hi;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        lo[i] = (int)(__builtin_amdgcn_perm(p[2 * i + 1], p[2 * i], 0x06040200u) ^ 0x80808080u); // low bytes - 128
        hi[i] = (int)__builtin_amdgcn_perm(p[2 * i + 1], p[2 * i], 0x07050301u);                 // high bytes, signed
    }
    v16i_t z = {};
    v16i_t acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(hi, tB, z, 0, 0, 0);
#pragma unroll
    for (int w = 0; w < 16; ++w) acc[w] = (acc[w] << 8) + k1; // + 128 S[y] + 64 (:2499-2543)
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(lo, tB, acc, 0, 0, 0);
    int V[16]; // V[y = r][x(w, h)], x(w, h) = 8 (w / 4) + 4 h + w % 4
#pragma unroll
    for (int w = 0; w < 16; ++w) V[w] = min(max(acc[w] >> 7, -32768), 32767);
    // ---- stage 2: bytes of V straight from the registers ----
    v4i_t d0, d1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t a = (uint32_t)V[4 * i], b = (uint32_t)V[4 * i + 1], cc = (uint32_t)V[4 * i + 2], d = (uint32_t)V[4 * i + 3];
        d0[i] = (int)(gather_byte(a, b, cc, d, 0) ^ 0x80808080u);
        d1[i] = (int)gather_byte(a, b, cc, d, 1);
    }
    const v16i_t k2 = *(const CONST_AS v16i_t*)&c.k->idct32_k2[h][0];
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(tP, d1, z, 0, 0, 0);
#pragma unroll
    for (int w = 0; w < 16; ++w) acc[w] = (acc[w] << 8) + k2[w]; // + 128 S[x] + 2048 (:2680-2737)
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(tP, d0, acc, 0, 0, 0);
    // lane (y = r, h): residuals at x = 8 q + 4 h + 0..3, q = 0..3
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint2 v;
        v.x = ((uint32_t)(acc[4 * q] >> 12) & 0xFFFFu) | ((uint32_t)(acc[4 * q + 1] >> 12) << 16);
        v.y = ((uint32_t)(acc[4 * q + 2] >> 12) & 0xFFFFu) | ((uint32_t)(acc[4 * q + 3] >> 12) << 16);
        *(uint2*)&SH.r1[o1 + r * 32 + 8 * q + 4 * h] = v;
    }
    WSYNC();
}

// ---------------------------------------------------------------------------
// 8x8 and 16x16 blocks the same way (the transforms of the leaf packs): 32 / N blocks share every MFMA, the basis
// operand of a first stage is block-diagonal over them, and the digits (forward) or bytes (inverse) of the data operand
// sit in the M dimension at rows m and m + 16, which are accumulators w and w + 8 of ONE lane, so they recombine without
// any lane exchange.  Lane (n = LANE & 31, h = LANE >> 5) of an accumulator holds column n, rows 8 (w / 4) + 4 h + w % 4;
// column n is (block n / N, index n % N).  What a first stage leaves in a lane is exactly that lane's share of the
// second stage's data operand, so nothing goes through LDS in between (r2 is not touched by the forward transforms).
// Cross products of different blocks meet zeros of the block-diagonal operand; rows that no block owns (N = 8: rows
// 8..15 and 24..31 of a first stage) repeat rows 0..7 and are not stored.  Blocks past nb carry zeros (a zero byte
// selector) and read a live block's address.  All 64 lanes run the operand gathers and the MFMAs under wave-uniform
// control; only the final stores sit under a lane predicate (the block of the lane's column exists).
//
// Bounds, S = max_u sum_x |T_N[u][x]| = 64 N (row 0), N <= 16 (tests/test_dct_mfma_model.py asserts them on the model):
//   forward, |r| <= 255: digits d0 in [-128, 127], d1 in [-1, 1]; per-digit sums <= 128 S = 131,072;
//     H = (sum + d) >> (LG - 1): |H| <= 255 * 64 N / (N / 2) = 32,640 (three digits: d0, d1 in [-128, 127], |d2| <= 1);
//     stage 2 per-digit sums <= 131,072; the recombined sum, and the chained accumulator before its last digit's product
//     (the sum less that product), <= 32,640 * 1024 + 131,072 + 2^10 < 2^25.1
//   inverse, any i16: bytes in [-128, 127]; per-byte sums <= 131,072; recombined (hi << 8) + lo + k <= 32,768 * 1024
//     + 128 * 1024 + 2048 < 2^25.1 in either stage; the clamp to i16 after stage 1 is the reference's
// ---------------------------------------------------------------------------
typedef int v2i_t __attribute__((ext_vector_type(2)));
constexpr uint32_t kSelLo = 0x06040200u, kSelHi = 0x07050301u, kSelZero = 0x0C0C0C0Cu; // v_perm: bytes 0 / 1 of four i16, zeros
static_assert(255 * 64 * 16 / 8 <= 32640 && 32640 + 128 + 32768 < (1 << 23), "H takes three balanced digits, the top one in [-1, 1]");
static_assert(32640ll * 1024 + (1 << 10) < (1ll << 31) && 32768ll * 1024 + 128 * 1024 + 2048 < (1ll << 31), "recombined sums stay in i32");

__device__ __forceinline__ uint32_t pk_add16(uint32_t p, uint32_t q) { // per i16 half, wrapping
    s2_t a, b;
    a.x = (short)(p & 0xFFFF);
    a.y = (short)(p >> 16);
    b.x = (short)(q & 0xFFFF);
    b.y = (short)(q >> 16);
    a = a + b;
    return (uint32_t)(unsigned short)a.x | ((uint32_t)(unsigned short)a.y << 16);
}
__device__ __forceinline__ long pack_i64(uint32_t lo, uint32_t hi) { return (long)(((unsigned long)hi << 32) | lo); }

// The data operand of a first stage: the lane's row (n % N) of the 32 / N blocks of its half, 16 samples of 16 bits, as
// the 16 bytes `sel` picks (kSelLo / kSelHi; a block past nb: zeros).  N = 16: block b0 + h; N = 8: blocks b0 + 2 h, + 1.
// src: [blk][row][col] i16.  add: added to each i16 before the pick (the forward transform's second digit), xm: xor'ed
// to the picked bytes of a live block (the inverse's "low byte minus 128").
template <int LG>
__device__ __forceinline__ v4i_t mfma_rows(const int16_t* src, int b0, int nb, int n, int h, uint32_t sel, uint32_t add,
                                           uint32_t xm) {
    constexpr int N = 1 << LG, NN = N * N;
    const int row = n & (N - 1), last = nb - 1;
    const int ba = b0 + (LG == 4 ? h : 2 * h), bb = LG == 4 ? ba : ba + 1;
    const uint4 q0 = *(const uint4*)&src[min(ba, last) * NN + row * N];
    const uint4 q1 = *(const uint4*)&src[min(bb, last) * NN + row * N + (LG == 4 ? 8 : 0)];
    const uint32_t sa = ba <= last ? sel : kSelZero, sb = bb <= last ? sel : kSelZero;
    const uint32_t xa = ba <= last ? xm : 0u, xb = bb <= last ? xm : 0u;
    v4i_t a;
    a[0] = (int)(__builtin_amdgcn_perm(pk_add16(q0.y, add), pk_add16(q0.x, add), sa) ^ xa);
    a[1] = (int)(__builtin_amdgcn_perm(pk_add16(q0.w, add), pk_add16(q0.z, add), sa) ^ xa);
    a[2] = (int)(__builtin_amdgcn_perm(pk_add16(q1.y, add), pk_add16(q1.x, add), sb) ^ xb);
    a[3] = (int)(__builtin_amdgcn_perm(pk_add16(q1.w, add), pk_add16(q1.z, add), sb) ^ xb);
    return a;
}

// forward (transformer.rs:2040-2378), LG = 3, 4: nb residual blocks in r1[o1 ..] ([blk][y][x] i16, |r| <= 255) ->
// coefficients in place ([blk][v][u]: the layout fwd_dct leaves).
//   stage 1: Ht[(d, y)][(blk, u)] = sum_x digit_d(R_blk[y][x]) T[u][x]     A = digits of R, rows 16 d + y; B = diag(T)
//   stage 2: C[v][(blk, u)] = sum_y T[v][y] H_blk[y][u]                    A = T in accumulator k order, B = digits of H
//     N = 16: three v_mfma_i32_32x32x16_i8 (k = the lane's 8 values of y), digit after digit from the top as at 32x32
//     N = 8: one v_mfma_i32_32x32x32_i8, k = (digit a, the lane's 4 values of y), rows 8 a + v: the three digit
//            products land in accumulators w, w + 4, w + 8
template <int LG>
__device__ __forceinline__ void fwd_dct_mfma(Ctx c, int nb, int o1) {
    static_assert(LG == 3 || LG == 4, "the 8x8 and 16x16 transforms");
    constexpr int N = 1 << LG, NN = N * N, PER = 32 / N, NH = N / 2;
    const int lane = LANE;
    const int n = lane & 31, h = lane >> 5;
    const v4i_t tB = *(const CONST_AS v4i_t*)&c.k->fdct_b[LG - 3][n][h][0];
    const int d = n >> 4;
    const v16i_t z = {};
#pragma unroll 1
    for (int b0 = 0; b0 < nb; b0 += PER) {
        // ---- stage 1: d0 = byte 0 of r (signed), d1 = byte 1 of r + 128 ----
        const v4i_t a = mfma_rows<LG>(&SH.r1[o1], b0, nb, n, h, d ? kSelHi : kSelLo, d ? 0x00800080u : 0u, 0u);
        v16i_t acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, tB, z, 0, 0, 0);
        uint32_t H[NH]; // Ht_blk[y(w, h)][u], y(w, h) = 8 (w / 4) + 4 h + w % 4
#pragma unroll
        for (int w = 0; w < NH; ++w) H[w] = (uint32_t)(((acc[w + 8] << 8) + acc[w] + (1 << (LG - 2))) >> (LG - 1)); // (:2201-2209)
        // ---- stage 2: digits of H straight from the registers ----
        if constexpr (LG == 4) {
            const long tP = *(const CONST_AS long*)&c.k->fdct16_p[n][h][0];
            const long d0 = pack_i64(gather_byte(H[0], H[1], H[2], H[3], 0), gather_byte(H[4], H[5], H[6], H[7], 0));
            const long d1 = pack_i64(gather_byte(H[0] + 128u, H[1] + 128u, H[2] + 128u, H[3] + 128u, 1),
                                     gather_byte(H[4] + 128u, H[5] + 128u, H[6] + 128u, H[7] + 128u, 1));
            const long d2 = pack_i64(gather_byte(H[0] + 32896u, H[1] + 32896u, H[2] + 32896u, H[3] + 32896u, 2),
                                     gather_byte(H[4] + 32896u, H[5] + 32896u, H[6] + 32896u, H[7] + 32896u, 2));
            acc = __builtin_amdgcn_mfma_i32_32x32x16_i8(tP, d2, z, 0, 0, 0); // (rows 16..31 of tP are zero: acc[8..15] stay 0)
#pragma unroll
            for (int w = 0; w < NH; ++w) acc[w] <<= 8;
            acc = __builtin_amdgcn_mfma_i32_32x32x16_i8(tP, d1, acc, 0, 0, 0);
#pragma unroll
            for (int w = 0; w < NH; ++w) acc[w] = (acc[w] << 8) + (1 << (LG + 5)); // (+ (1 << (LG + 5))) >> (LG + 6) (:2309-2316)
            acc = __builtin_amdgcn_mfma_i32_32x32x16_i8(tP, d0, acc, 0, 0, 0);
        } else {
            const v4i_t tP = *(const CONST_AS v4i_t*)&c.k->fdct8_p[n][h][0];
            v4i_t b;
            b[0] = (int)gather_byte(H[0], H[1], H[2], H[3], 0);
            b[1] = (int)gather_byte(H[0] + 128u, H[1] + 128u, H[2] + 128u, H[3] + 128u, 1);
            b[2] = (int)gather_byte(H[0] + 32896u, H[1] + 32896u, H[2] + 32896u, H[3] + 32896u, 2);
            b[3] = 0;
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(tP, b, z, 0, 0, 0);
#pragma unroll
            for (int w = 0; w < NH; ++w) acc[w] = (((acc[w + 8] << 8) + acc[w + 4]) << 8) + acc[w] + (1 << (LG + 5));
        }
        WSYNC(); // every lane has read its residuals before the coefficients overwrite them
        if (b0 + (n >> LG) < nb) {
            int16_t* out = &SH.r1[o1 + (b0 + (n >> LG)) * NN + (n & (N - 1))];
#pragma unroll
            for (int w = 0; w < NH; ++w) out[(8 * (w >> 2) + 4 * h + (w & 3)) * N] = (int16_t)(acc[w] >> (LG + 6));
        }
        WSYNC();
    }
}

// inverse (transformer.rs:2380-2737), LG = 3, 4: nb transposed dequantised blocks in r2 ([blk][x][i], any i16) ->
// residuals r1[o1 ..] ([blk][y][x]).  Bytes as in inv_dct32_mfma: v = 256 hi + (lo - 128) + 128.
//   stage 1: Vt[(b, x)][(blk, y)] = sum_i byte_b(dT_blk[x][i]) T[i][y]     A = bytes of dT, rows 16 b + x; B = diag(T)
//            V = clamp16(((hi << 8) + lo + 128 S[y] + 64) >> 7)            (idct_k1, S[y] = sum_i T[i][y])
//   stage 2: Rt[(b, x)][(blk, y)] = sum_i T[i][x] byte_b(V_blk[y][i])      A = T, k = (byte b, the lane's values of i),
//            rows 16 b + x; B = the lane's bytes of V; C = 128 S[x] + 2048 in rows b = 0 (idct16_k2 / idct8_k2)
//            N = 16: v_mfma_i32_32x32x32_i8 (8 values, 16 bytes); N = 8: v_mfma_i32_32x32x16_i8 (4 values, 8 bytes)
template <int LG>
__device__ __forceinline__ void inv_dct_mfma(Ctx c, int nb, int o1) {
    static_assert(LG == 3 || LG == 4, "the 8x8 and 16x16 transforms");
    constexpr int N = 1 << LG, NN = N * N, PER = 32 / N, NH = N / 2;
    const int lane = LANE;
    const int n = lane & 31, h = lane >> 5;
    const v4i_t tB = *(const CONST_AS v4i_t*)&c.k->idct_b[LG - 3][n][h][0];
    const int k1 = c.k->idct_k1[LG - 3][n];
    const int b = n >> 4;
    const v16i_t z = {};
    v16i_t k2 = {};
    if constexpr (LG == 4) {
        const v4i_t ka = *(const CONST_AS v4i_t*)&c.k->idct16_k2[h][0], kb = *(const CONST_AS v4i_t*)&c.k->idct16_k2[h][4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            k2[w] = ka[w];
            k2[4 + w] = kb[w];
        }
    } else {
        const v4i_t ka = *(const CONST_AS v4i_t*)&c.k->idct8_k2[h][0];
#pragma unroll
        for (int w = 0; w < 4; ++w) k2[w] = ka[w];
    }
#pragma unroll 1
    for (int b0 = 0; b0 < nb; b0 += PER) {
        // ---- stage 1 ----
        const v4i_t a = mfma_rows<LG>((const int16_t*)SH.r2, b0, nb, n, h, b ? kSelHi : kSelLo, 0u, b ? 0u : 0x80808080u);
        v16i_t acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, tB, z, 0, 0, 0);
        uint32_t V[NH]; // V_blk[y][x(w, h)], x(w, h) = 8 (w / 4) + 4 h + w % 4
#pragma unroll
        for (int w = 0; w < NH; ++w) V[w] = (uint32_t)min(max(((acc[w + 8] << 8) + acc[w] + k1) >> 7, -32768), 32767); // (:2499-2543)
        // ---- stage 2: bytes of V straight from the registers ----
        if constexpr (LG == 4) {
            const v4i_t tP = *(const CONST_AS v4i_t*)&c.k->idct16_p[n][h][0];
            v4i_t bv;
            bv[0] = (int)(gather_byte(V[0], V[1], V[2], V[3], 0) ^ 0x80808080u);
            bv[1] = (int)(gather_byte(V[4], V[5], V[6], V[7], 0) ^ 0x80808080u);
            bv[2] = (int)gather_byte(V[0], V[1], V[2], V[3], 1);
            bv[3] = (int)gather_byte(V[4], V[5], V[6], V[7], 1);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(tP, bv, k2, 0, 0, 0);
        } else {
            const long tP = *(const CONST_AS long*)&c.k->idct8_p[n][h][0];
            const long bv = pack_i64(gather_byte(V[0], V[1], V[2], V[3], 0) ^ 0x80808080u, gather_byte(V[0], V[1], V[2], V[3], 1));
            acc = __builtin_amdgcn_mfma_i32_32x32x16_i8(tP, bv, k2, 0, 0, 0);
        }
        // lane ((blk, y), h): residuals at x = 8 q + 4 h + 0..3 (:2680-2737)
        if (b0 + (n >> LG) < nb) {
            int16_t* out = &SH.r1[o1 + (b0 + (n >> LG)) * NN + (n & (N - 1)) * N + 4 * h];
#pragma unroll
            for (int q = 0; q < NH / 4; ++q) {
                int r[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = ((acc[4 * q + j + 8] << 8) + acc[4 * q + j]) >> 12;
                uint2 v;
                v.x = ((uint32_t)r[0] & 0xFFFFu) | ((uint32_t)r[1] << 16);
                v.y = ((uint32_t)r[2] & 0xFFFFu) | ((uint32_t)r[3] << 16);
                *(uint2*)&out[8 * q] = v;
            }
        }
        WSYNC();
    }
}

// ---------------------------------------------------------------------------
// 4x4 blocks in registers (the packed 4x4 passes of the leaf searches, dev_search.h): four blocks per wave,
// lane = (block LANE >> 4, sample LANE & 15, row-major), one value per lane in and out.  A 4x4 block lies inside one
// 16-lane DPP row, so the two stages of a transform exchange their operands between lanes and nothing goes through LDS:
//   the four lanes 4 y + 0..3 of a quad (one row of the block):  quad_perm broadcasts [k, k, k, k]
//   the four lanes 4 i + x at stride 4 (one column of the block):  row_ror:4 k
// The basis elements (64, 83, 36 and their signs) are the bytes of literals picked by the lane's x = LANE & 3 or
// y = (LANE >> 2) & 3: no table, no load.  Same sums, offsets, shifts and casts as fwd_dct<2> / inv_dct<2>.
// All 64 lanes must be enabled where these are called (a DPP read of a disabled lane is not that lane's value):
// idle rows carry zeros, and no call sits under a lane-divergent branch.
// ---------------------------------------------------------------------------
constexpr int kT4[4][4] = {{64, 64, 64, 64}, {83, 36, -36, -83}, {64, -64, -64, 64}, {36, -83, 83, -36}}; // T_4[u][x]
// row_ror:4 k hands lane j (of the stride-4 column) the value of lane (j - k) & 3 (the impulse cases of
// tests/test_gpu_blocks4_registers.py pin this direction: with the other one every off-diagonal coefficient moves)
constexpr int ror4_src(int j, int k) { return (j - k) & 3; }
enum { T4_FWD1, T4_FWD2, T4_INV1, T4_INV2 };
// the basis element that goes with operand k of a stage, for the lanes of index j = 0..3, as bytes j of one word
constexpr uint32_t t4_word(int stage, int k) {
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j) {
        const int o = ror4_src(j, k);
        const int t = stage == T4_FWD1   ? kT4[j][k]  // lane u = j, operand r[y][k]
                      : stage == T4_FWD2 ? kT4[j][o]  // lane v = j, operand H[x][o]
                      : stage == T4_INV1 ? kT4[o][j]  // lane y = j, operand d[o][x]
                                         : kT4[k][j]; // lane x = j, operand V[y][k]
        w |= (uint32_t)(t & 0xFF) << (8 * j);
    }
    return w;
}
template <int STAGE, int K>
__device__ __forceinline__ int t4_sel(int shift8) { // shift8 = 8 * (the lane's index j)
    constexpr uint32_t w = t4_word(STAGE, K);
    return (int)(int8_t)(w >> shift8);
}
// the sum over the four operands of a stage: the lanes of the quad (QUAD) or of the stride-4 column
template <int STAGE, bool QUAD>
__device__ __forceinline__ int t4_stage(int v, int shift8) {
    // |basis| <= 83 and |operand| < 2^23 (an i16, or stage 1 of the forward transform: <= 2 * 83 * 32768): exact in 24 bits
    const int v0 = QUAD ? dpp_mov<0x00>(v) : v;
    const int v1 = QUAD ? dpp_mov<0x55>(v) : dpp_mov<0x124>(v); // quad_perm [1,1,1,1] / row_ror:4
    const int v2 = QUAD ? dpp_mov<0xAA>(v) : dpp_mov<0x128>(v); // quad_perm [2,2,2,2] / row_ror:8
    const int v3 = QUAD ? dpp_mov<0xFF>(v) : dpp_mov<0x12C>(v); // quad_perm [3,3,3,3] / row_ror:12
    const int t0 = t4_sel<STAGE, 0>(shift8), t1 = t4_sel<STAGE, 1>(shift8), t2 = t4_sel<STAGE, 2>(shift8), t3 = t4_sel<STAGE, 3>(shift8);
    const int acc = M24(v0, t0) + M24(v1, t1) + M24(v2, t2) + M24(v3, t3);
    return acc;
}

// forward (transformer.rs:2040-2378 at 4x4): the lane's residual r[y][x] -> the lane's coefficient C[y][x] (C[v][x] on
// lane (v, x): the layout fwd_dct<2> leaves in r1)
__device__ __forceinline__ int fwd_dct4_reg(int res) {
#ifdef WRENC_EXP_SKIP_DCT
    return res;
#endif
    const int lane = lane_fresh();
    const int sx = 8 * (lane & 3), sy = 2 * (lane & 12);
    // stage 1 on lane (y, u): H[u][y] = (sum_x T[u][x] r[y][x] + 1) >> 1
    const int h = (t4_stage<T4_FWD1, true>(res, sx) + 1) >> 1;
    // stage 2 on lane (v, x): C[v][x] = (sum_y T[v][y] H[x][y] + 128) >> 8, H[x][y] from lane (y, x)
    return (int16_t)((t4_stage<T4_FWD2, false>(h, sy) + 128) >> 8);
}

// inverse (transformer.rs:2380-2737 at 4x4): the lane's dequantised coefficient d[y][x] -> the lane's residual r[y][x]
__device__ __forceinline__ int inv_dct4_reg(int deq) {
#ifdef WRENC_EXP_SKIP_DCT
    return deq;
#endif
    const int lane = lane_fresh();
    const int sx = 8 * (lane & 3), sy = 2 * (lane & 12);
    // stage 1 on lane (y, x): V[y][x] = clamp16((sum_i T[i][y] d[i][x] + 64) >> 7)
    int v = (t4_stage<T4_INV1, false>(deq, sy) + 64) >> 7;
    v = min(max(v, -32768), 32767);
    // stage 2 on lane (y, x): r[y][x] = (sum_i T[i][x] V[y][i] + 2048) >> 12
    return (int16_t)((t4_stage<T4_INV2, true>(v, sx) + 2048) >> 12);
}

// o1: where the blocks start in r1 (i16 units, a multiple of 2; of 8 for the MFMA versions' 16-byte row reads, which is
// what the search has: blocks start at multiples of 64).
// Which code runs at 8x8 and 16x16 (ARM, a literal: the branches fold away).  DCT_SEARCH, what every caller in the search
// passes: 16x16 as i8 MFMAs (fwd_dct_mfma / inv_dct_mfma, +3.0 % frames/s on the headline workload), 8x8 through the v_dot2
// templates -- the MFMA version of that size is exact, but faster in the micro-benchmark only from three blocks per
// group up, and its gain in the search (+0.2 %) did not clear the project's margin.  DCT_VDOT2 / DCT_MFMA: the building-block kernels (wrenc_gpu_test.hip)
// name the arm, for groups the digit scheme does not take (a residual outside +-255, an o1 that is no multiple of 8),
// for the parity tests of both versions at both sizes and for the micro-benchmark (tools/dct_bench.py).
enum { DCT_SEARCH, DCT_VDOT2, DCT_MFMA };
constexpr bool dct_runs_mfma(int arm, int lg) { return arm == DCT_MFMA || (arm == DCT_SEARCH && lg == 4); }
template <int ARM = DCT_SEARCH>
__device__ __forceinline__ void fwd_dct_lg(Ctx c, int lg, int nb, int o1 = 0) {
#ifdef WRENC_EXP_SKIP_DCT // instruction-count experiment only: the residual stays where the coefficients should be
    return;
#endif
    c = uni(c);
    lg = uni(lg);
    nb = uni(nb);
    o1 = uni(o1);
    LDS_AS int32_t* h = (LDS_AS int32_t*)SH.r2;
    constexpr int HB = (int)sizeof(SH.r2);
    switch (lg) {
    case 2: fwd_dct<2, HB>(c, nb, o1, h); break;
    case 3:
        if (!dct_runs_mfma(ARM, 3))
            fwd_dct<3, HB>(c, nb, o1, h);
        else
            fwd_dct_mfma<3>(c, nb, o1);
        break;
    case 4:
        if (!dct_runs_mfma(ARM, 4))
            fwd_dct<4, HB>(c, nb, o1, h);
        else
            fwd_dct_mfma<4>(c, nb, o1);
        break;
    default:
        // 32x32 (always a single luma block): the i8-MFMA version, kept on measurement (3.6x in the
        // micro-benchmark, +5.6 % frames/s at max-split-depth 0, +0.9 % at depth 2); its intermediate stays in the
        // accumulators, which is what lets r2 be 2 KB.
        fwd_dct32_mfma(c, o1);
        break;
    }
}
template <int ARM = DCT_SEARCH>
__device__ __forceinline__ void inv_dct_lg(Ctx c, int lg, int nb, int o1 = 0) {
#ifdef WRENC_EXP_SKIP_DCT
    return;
#endif
    c = uni(c);
    lg = uni(lg);
    nb = uni(nb);
    o1 = uni(o1);
    switch (lg) {
    case 2: inv_dct<2>(c, nb, o1); break;
    case 3:
        if (!dct_runs_mfma(ARM, 3))
            inv_dct<3>(c, nb, o1);
        else
            inv_dct_mfma<3>(c, nb, o1);
        break;
    case 4:
        if (!dct_runs_mfma(ARM, 4))
            inv_dct<4>(c, nb, o1);
        else
            inv_dct_mfma<4>(c, nb, o1);
        break;
    default:
#ifdef WRENC_IDCT32_VDOT2
        inv_dct<5>(c, nb, o1); // the comparison arm of the micro-benchmark (tools/dct_bench.py)
#else
        inv_dct32_mfma(c, o1); // 32x32 is always a single luma block
#endif
        break;
    }
}

} // namespace wrenc
