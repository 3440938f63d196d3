// dev_hash.h -- the decoded picture hash (include/wrenc_hash.h: MD5, CRC, checksum of H.274's decoded picture hash SEI) of
// the reconstruction a slot holds, taken on the device (include/wrenc_gpu.h: wrenc_gpu_download_hashes).  Each component
// is hashed over its coded plane, W x H luma and W/2 x H/2 chroma, a string of N = pw * ph bytes in raster order (the
// planes are tightly packed; pw is a multiple of 16 and N a multiple of 256).
//
// Layout (checksum and CRC).  The string is cut from its END into PIECES of kHashPiece = kHashLoads * 1024 bytes, one
// wave per piece: per load a lane reads 16 bytes (global_load_dwordx4), contiguous across the wave (1 KiB per load
// instruction), kHashLoads loads in flight; a lane's chunks are 1 KiB apart.  The first piece of a plane is short by
// pad = pieces * kHashPiece - N bytes: its lanes in front of the plane read byte 0 again and count as nothing (for the CRC:
// as zeros in front of the string, which leave a CRC that starts from 0 unchanged).  Every byte is read once.
// A wave leaves one 32-bit partial at its own index and hash_finish_kernel combines a plane's partials, one wave per
// (picture, plane), lane l taking partials l, l + 64, ... counted from the END in the same way: no atomics, the same
// bytes in any slot, any batch size and any run.
//
// Checksum: sum of byte ^ mask(x, y) modulo 2^32.  A 16-byte chunk lies inside one row at x = 0 mod 16, so its masks are
// c ^ i with c = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8) and i = 0 .. 15 the byte's place in the chunk: one xor and
// one v_dot4_u32_u8 per dword.  (x, y) of a lane's last chunk by one division, the others by stepping back 1 KiB.
// Partials and the finish are plain sums (any order gives the same 32 bits).
//
// CRC: linear over GF(2).  With crc0(M) = M(x) x^16 mod P (P = x^16 + x^12 + x^5 + 1; Python's crc_hqx(M, 0)):
//     crc0(A | B) = crc0(A) x^(8 |B|) + crc0(B)  (mod P),    SEI value = crc0(plane) + 0xFFFF x^(8 N + 16)  (mod P).
// A lane takes crc0 of its 16 bytes by four steps of four byte-table lookups (the running value goes into the next dword's
// first two bytes: x^32 per step), combines its chunks by Horner steps with x^(8 * 1024) (two more lookups: the 16-bit
// value's two bytes), and multiplies the result by its place in the wave, x^(128 (63 - lane)); the wave's partial is the
// xor of its lanes.  The finish does the same with the partials: Horner steps with x^(8 * 64 * kHashPiece) per lane, times
// x^(8 * kHashPiece * (63 - lane)), xor over the lanes, plus the term of the 0xFFFF start, which depends on N alone and
// comes from the host.  The six 256-entry tables and the lane multipliers depend on kHashPiece alone: hash_fill_tables
// builds them on the host once per context; a workgroup copies them to LDS (3.2 KB) and then takes pieces in a
// grid-stride loop, so the copy is paid once per workgroup and not once per piece.
//
// MD5: a serial chain, 64 steps per 64 bytes, each depending on the last: one LANE per (picture, plane), the luma planes
// of a call in waves of their own and the chroma planes behind them, so that a wave's lanes end together.  A lane's next
// 64 bytes are on their way while it works on the current ones.  N is a multiple of 64: the padding is always one
// block of its own (0x80, zeros, the length in bits).
#pragma once

#include "../../include/wrenc_hash.h"

namespace wrenc {

constexpr int kHashLoads = 4;                   // 16-byte loads per lane and piece; part of the layout the tests name
constexpr int kHashPiece = kHashLoads * 1024;   // bytes per wave

// how a plane (chroma = 0 luma, 1 Cb / Cr) of a W x H picture is dealt to waves
struct HashPlane {
    int pw, ph;
    int bytes;   // N
    int pieces;  // waves
    int pad;     // bytes the first piece is short of
};
__host__ __device__ inline HashPlane hash_plane(int W, int H, int chroma) {
    HashPlane p;
    p.pw = W >> chroma;
    p.ph = H >> chroma;
    p.bytes = p.pw * p.ph;
    p.pieces = (p.bytes + kHashPiece - 1) / kHashPiece;
    p.pad = p.pieces * kHashPiece - p.bytes;
    return p;
}

// a b mod P for polynomials below x^16 (bit i = x^i)
__host__ __device__ inline uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; --i) {
        r <<= 1;
        r ^= (r & 0x10000u) ? 0x11021u : 0u;
        r ^= ((b >> i) & 1u) ? a : 0u;
    }
    return r;
}
// x^e mod P
__host__ __device__ inline uint32_t crc_xpow(unsigned long long e) {
    uint32_t r = 1, base = 2;
    for (; e; e >>= 1) {
        if (e & 1) r = crc_mul(r, base);
        base = crc_mul(base, base);
    }
    return r;
}

// what the CRC kernels look up: tab[k][b] = b(x) x^(40 - 8 k) for byte k of a dword (k = 0 .. 3; x^16 of crc0 included),
// tab[4][b] = b(x) x^(8 * 1024 + 8) and tab[5][b] = b(x) x^(8 * 1024) for the high and low byte of a Horner step;
// lane_mul[l] = x^(128 (63 - l)); for the finish fin_lane_mul[l] = x^(8 kHashPiece (63 - l)) and fin_step = x^(8 * 64 * kHashPiece)
struct HashTables {
    uint16_t tab[6][256];
    uint16_t lane_mul[64];
    uint16_t fin_lane_mul[64];
    uint32_t fin_step;
    uint32_t reserved[3];
};
static_assert(sizeof(HashTables) % 16 == 0, "copied to LDS in 16-byte pieces");
constexpr int kHashLdsBytes = 6 * 256 * 2 + 64 * 2; // tab and lane_mul: what the piece kernel needs

inline void hash_fill_tables(HashTables& t) {
    const unsigned long long e[6] = {40, 32, 24, 16, 8 * 1024 + 8, 8 * 1024};
    for (int k = 0; k < 6; ++k) {
        const uint32_t m = crc_xpow(e[k]);
        for (uint32_t b = 0; b < 256; ++b) t.tab[k][b] = (uint16_t)crc_mul(m, b);
    }
    for (int l = 0; l < 64; ++l) {
        t.lane_mul[l] = (uint16_t)crc_xpow(128ull * (63 - l));
        t.fin_lane_mul[l] = (uint16_t)crc_xpow(8ull * kHashPiece * (63 - l));
    }
    t.fin_step = crc_xpow(8ull * 64 * kHashPiece);
    t.reserved[0] = t.reserved[1] = t.reserved[2] = 0;
}
// the term of the CRC's 0xFFFF start for a plane of N bytes
inline uint32_t hash_crc_start_term(int bytes) { return crc_mul(0xFFFFu, crc_xpow(8ull * (unsigned long long)bytes + 16)); }

// the plane and the piece (CRC, checksum) that wave `id` of a call works on; planes of a picture side by side: Y | Cb | Cr
struct HashWork {
    int pic, plane, piece;
    HashPlane P;
};
__device__ __forceinline__ HashWork hash_work(int id, const HashPlane& L, const HashPlane& C) {
    const int per_pic = L.pieces + 2 * C.pieces;
    HashWork w;
    w.pic = id / per_pic;
    int rem = id - w.pic * per_pic;
    w.plane = 0;
    if (rem >= L.pieces) {
        rem -= L.pieces;
        w.plane = 1;
        if (rem >= C.pieces) {
            rem -= C.pieces;
            w.plane = 2;
        }
    }
    w.piece = rem;
    w.P = w.plane ? C : L;
    return w;
}

// crc0 of a lane's 16 bytes (the byte at the lowest address is the first of the string)
__device__ __forceinline__ uint32_t crc_chunk(const uint16_t* tab, const Dwords4& d) {
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t w = d[k] ^ (acc >> 8) ^ ((acc & 0xFFu) << 8); // acc x^32: its high byte meets the dword's first byte
        acc = (uint32_t)tab[w & 0xFFu] ^ (uint32_t)tab[256 + ((w >> 8) & 0xFFu)] ^ (uint32_t)tab[512 + ((w >> 16) & 0xFFu)] ^
              (uint32_t)tab[768 + (w >> 24)];
    }
    return acc;
}

// One wave per (picture, plane, piece), in a grid-stride loop.  CRC: the partial is crc0 of the piece; else its checksum.
template <bool CRC>
__global__ __launch_bounds__(256) void hash_piece_kernel(const PicBufs* __restrict__ slots, int first_slot, int n_pics, int W, int H,
                                                         const HashTables* __restrict__ tables, uint32_t* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) uint16_t tab[kHashLdsBytes / 2];
    if (CRC) {
        if (threadIdx.x < kHashLdsBytes / 16) ((Dwords4*)tab)[threadIdx.x] = ((GlobalRow)tables)[threadIdx.x];
        __syncthreads();
    }
    const HashPlane L = hash_plane(W, H, 0), C = hash_plane(W, H, 1);
    const int total = n_pics * (L.pieces + 2 * C.pieces);
    const int lane = (int)(threadIdx.x & 63);
    for (int id = uni((int)(blockIdx.x * 4 + (threadIdx.x >> 6))); id < total; id += (int)gridDim.x * 4) { // (the whole wave)
        const HashWork w = hash_work(id, L, C);
        const uint8_t* rec = slots[first_slot + w.pic].rec[w.plane];
        // the lane's chunks at r0, r0 + 1024, ...; a negative offset lies in front of the plane
        const int r0 = w.piece * kHashPiece - w.P.pad + 16 * lane;
        Dwords4 d[kHashLoads];
#pragma unroll
        for (int j = 0; j < kHashLoads; ++j) d[j] = *(GlobalRow)(rec + max(r0 + 1024 * j, 0));
        uint32_t acc = 0;
        if (CRC) {
#pragma unroll
            for (int j = 0; j < kHashLoads; ++j) {
                const uint32_t c = r0 + 1024 * j >= 0 ? crc_chunk(tab, d[j]) : 0u;
                acc = (uint32_t)tab[1024 + (acc >> 8)] ^ (uint32_t)tab[1280 + (acc & 0xFFu)] ^ c;
            }
            acc = crc_mul(acc, tab[1536 + lane]);
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) acc ^= (uint32_t)__shfl_xor((int)acc, s, 64);
        } else {
            // (x, y) of the last chunk; the others 1024 bytes = qy rows and qx samples back.  A lane whose last chunk lies in
            // front of the plane has none inside it.
            const int last = r0 + 1024 * (kHashLoads - 1);
            const int qy = 1024 / w.P.pw, qx = 1024 - qy * w.P.pw;
            int y = max(last, 0) / w.P.pw, x = max(last, 0) - y * w.P.pw;
#pragma unroll
            for (int j = kHashLoads - 1; j >= 0; --j) {
                const uint32_t c = (uint32_t)((x ^ y ^ (x >> 8) ^ (y >> 8)) & 0xFF) * 0x01010101u;
                uint32_t s = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    s = __builtin_amdgcn_udot4(d[j][k] ^ c ^ (0x03020100u + 0x04040404u * (uint32_t)k), 0x01010101u, s, false);
                acc += r0 + 1024 * j >= 0 ? s : 0u;
                x -= qx;
                y -= qy;
                if (x < 0) {
                    x += w.P.pw;
                    --y;
                }
            }
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) acc += (uint32_t)__shfl_xor((int)acc, s, 64);
        }
        if (lane == 0) partials[id] = acc;
    }
}

// A plane's partials combined, one wave per (picture, plane): blockIdx.x the picture, blockIdx.y the plane.  The value
// goes to out[picture].value[plane] as the SEI carries it (CRC 2 bytes, checksum 4, big-endian, zeros behind).
// start_luma / start_chroma: hash_crc_start_term of the two plane sizes.
template <bool CRC>
__global__ __launch_bounds__(64) void hash_finish_kernel(const uint32_t* __restrict__ partials, int W, int H,
                                                         const HashTables* __restrict__ tables, uint32_t start_luma,
                                                         uint32_t start_chroma, wrenc_picture_hash* __restrict__ out) {
    const HashPlane L = hash_plane(W, H, 0), C = hash_plane(W, H, 1);
    const int plane = (int)blockIdx.y, lane = (int)threadIdx.x;
    const int count = plane ? C.pieces : L.pieces;
    const uint32_t* p = partials + (size_t)blockIdx.x * (L.pieces + 2 * C.pieces) + (plane ? L.pieces + (plane - 1) * C.pieces : 0);
    const int turns = (count + 63) / 64, pad = turns * 64 - count;
    const uint32_t step = CRC ? tables->fin_step : 0u;
    uint32_t acc = 0;
    for (int t = 0; t < turns; ++t) {
        const int i = t * 64 + lane - pad;
        const uint32_t v = i >= 0 ? p[max(i, 0)] : 0u;
        acc = CRC ? crc_mul(acc, step) ^ v : acc + v;
    }
    if (CRC) acc = crc_mul(acc, tables->fin_lane_mul[lane]);
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)acc, s, 64);
        acc = CRC ? acc ^ o : acc + o;
    }
    if (lane == 0) {
        Dwords4 v = {0u, 0u, 0u, 0u};
        if (CRC) {
            acc ^= plane ? start_chroma : start_luma;
            v[0] = (acc >> 8) | ((acc & 0xFFu) << 8);
        } else {
            v[0] = __builtin_bswap32(acc);
        }
        *(Dwords4*)out[blockIdx.x].value[plane] = v;
    }
}

// RFC 1321: one step a = b + ((a + f(b, c, d) + m + t) <<< s)
#define WRENC_MD5_STEP(f, a, b, c, d, m, s, t)     \
    {                                              \
        const uint32_t v_ = (a) + f(b, c, d) + (m) + (t); \
        (a) = (b) + ((v_ << (s)) | (v_ >> (32 - (s))));   \
    }
#define WRENC_MD5_F(x, y, z) (((x) & (y)) | (~(x) & (z)))
#define WRENC_MD5_G(x, y, z) (((x) & (z)) | ((y) & ~(z)))
#define WRENC_MD5_H(x, y, z) ((x) ^ (y) ^ (z))
#define WRENC_MD5_I(x, y, z) ((y) ^ ((x) | ~(z)))

__device__ __forceinline__ void md5_block(uint32_t st[4], const Dwords4 q[4]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
#define M(i) q[(i) >> 2][(i) & 3]
    WRENC_MD5_STEP(WRENC_MD5_F, a, b, c, d, M(0), 7, 0xd76aa478u)
    WRENC_MD5_STEP(WRENC_MD5_F, d, a, b, c, M(1), 12, 0xe8c7b756u)
    WRENC_MD5_STEP(WRENC_MD5_F, c, d, a, b, M(2), 17, 0x242070dbu)
    WRENC_MD5_STEP(WRENC_MD5_F, b, c, d, a, M(3), 22, 0xc1bdceeeu)
    WRENC_MD5_STEP(WRENC_MD5_F, a, b, c, d, M(4), 7, 0xf57c0fafu)
    WRENC_MD5_STEP(WRENC_MD5_F, d, a, b, c, M(5), 12, 0x4787c62au)
    WRENC_MD5_STEP(WRENC_MD5_F, c, d, a, b, M(6), 17, 0xa8304613u)
    WRENC_MD5_STEP(WRENC_MD5_F, b, c, d, a, M(7), 22, 0xfd469501u)
    WRENC_MD5_STEP(WRENC_MD5_F, a, b, c, d, M(8), 7, 0x698098d8u)
    WRENC_MD5_STEP(WRENC_MD5_F, d, a, b, c, M(9), 12, 0x8b44f7afu)
    WRENC_MD5_STEP(WRENC_MD5_F, c, d, a, b, M(10), 17, 0xffff5bb1u)
    WRENC_MD5_STEP(WRENC_MD5_F, b, c, d, a, M(11), 22, 0x895cd7beu)
    WRENC_MD5_STEP(WRENC_MD5_F, a, b, c, d, M(12), 7, 0x6b901122u)
    WRENC_MD5_STEP(WRENC_MD5_F, d, a, b, c, M(13), 12, 0xfd987193u)
    WRENC_MD5_STEP(WRENC_MD5_F, c, d, a, b, M(14), 17, 0xa679438eu)
    WRENC_MD5_STEP(WRENC_MD5_F, b, c, d, a, M(15), 22, 0x49b40821u)
    WRENC_MD5_STEP(WRENC_MD5_G, a, b, c, d, M(1), 5, 0xf61e2562u)
    WRENC_MD5_STEP(WRENC_MD5_G, d, a, b, c, M(6), 9, 0xc040b340u)
    WRENC_MD5_STEP(WRENC_MD5_G, c, d, a, b, M(11), 14, 0x265e5a51u)
    WRENC_MD5_STEP(WRENC_MD5_G, b, c, d, a, M(0), 20, 0xe9b6c7aau)
    WRENC_MD5_STEP(WRENC_MD5_G, a, b, c, d, M(5), 5, 0xd62f105du)
    WRENC_MD5_STEP(WRENC_MD5_G, d, a, b, c, M(10), 9, 0x02441453u)
    WRENC_MD5_STEP(WRENC_MD5_G, c, d, a, b, M(15), 14, 0xd8a1e681u)
    WRENC_MD5_STEP(WRENC_MD5_G, b, c, d, a, M(4), 20, 0xe7d3fbc8u)
    WRENC_MD5_STEP(WRENC_MD5_G, a, b, c, d, M(9), 5, 0x21e1cde6u)
    WRENC_MD5_STEP(WRENC_MD5_G, d, a, b, c, M(14), 9, 0xc33707d6u)
    WRENC_MD5_STEP(WRENC_MD5_G, c, d, a, b, M(3), 14, 0xf4d50d87u)
    WRENC_MD5_STEP(WRENC_MD5_G, b, c, d, a, M(8), 20, 0x455a14edu)
    WRENC_MD5_STEP(WRENC_MD5_G, a, b, c, d, M(13), 5, 0xa9e3e905u)
    WRENC_MD5_STEP(WRENC_MD5_G, d, a, b, c, M(2), 9, 0xfcefa3f8u)
    WRENC_MD5_STEP(WRENC_MD5_G, c, d, a, b, M(7), 14, 0x676f02d9u)
    WRENC_MD5_STEP(WRENC_MD5_G, b, c, d, a, M(12), 20, 0x8d2a4c8au)
    WRENC_MD5_STEP(WRENC_MD5_H, a, b, c, d, M(5), 4, 0xfffa3942u)
    WRENC_MD5_STEP(WRENC_MD5_H, d, a, b, c, M(8), 11, 0x8771f681u)
    WRENC_MD5_STEP(WRENC_MD5_H, c, d, a, b, M(11), 16, 0x6d9d6122u)
    WRENC_MD5_STEP(WRENC_MD5_H, b, c, d, a, M(14), 23, 0xfde5380cu)
    WRENC_MD5_STEP(WRENC_MD5_H, a, b, c, d, M(1), 4, 0xa4beea44u)
    WRENC_MD5_STEP(WRENC_MD5_H, d, a, b, c, M(4), 11, 0x4bdecfa9u)
    WRENC_MD5_STEP(WRENC_MD5_H, c, d, a, b, M(7), 16, 0xf6bb4b60u)
    WRENC_MD5_STEP(WRENC_MD5_H, b, c, d, a, M(10), 23, 0xbebfbc70u)
    WRENC_MD5_STEP(WRENC_MD5_H, a, b, c, d, M(13), 4, 0x289b7ec6u)
    WRENC_MD5_STEP(WRENC_MD5_H, d, a, b, c, M(0), 11, 0xeaa127fau)
    WRENC_MD5_STEP(WRENC_MD5_H, c, d, a, b, M(3), 16, 0xd4ef3085u)
    WRENC_MD5_STEP(WRENC_MD5_H, b, c, d, a, M(6), 23, 0x04881d05u)
    WRENC_MD5_STEP(WRENC_MD5_H, a, b, c, d, M(9), 4, 0xd9d4d039u)
    WRENC_MD5_STEP(WRENC_MD5_H, d, a, b, c, M(12), 11, 0xe6db99e5u)
    WRENC_MD5_STEP(WRENC_MD5_H, c, d, a, b, M(15), 16, 0x1fa27cf8u)
    WRENC_MD5_STEP(WRENC_MD5_H, b, c, d, a, M(2), 23, 0xc4ac5665u)
    WRENC_MD5_STEP(WRENC_MD5_I, a, b, c, d, M(0), 6, 0xf4292244u)
    WRENC_MD5_STEP(WRENC_MD5_I, d, a, b, c, M(7), 10, 0x432aff97u)
    WRENC_MD5_STEP(WRENC_MD5_I, c, d, a, b, M(14), 15, 0xab9423a7u)
    WRENC_MD5_STEP(WRENC_MD5_I, b, c, d, a, M(5), 21, 0xfc93a039u)
    WRENC_MD5_STEP(WRENC_MD5_I, a, b, c, d, M(12), 6, 0x655b59c3u)
    WRENC_MD5_STEP(WRENC_MD5_I, d, a, b, c, M(3), 10, 0x8f0ccc92u)
    WRENC_MD5_STEP(WRENC_MD5_I, c, d, a, b, M(10), 15, 0xffeff47du)
    WRENC_MD5_STEP(WRENC_MD5_I, b, c, d, a, M(1), 21, 0x85845dd1u)
    WRENC_MD5_STEP(WRENC_MD5_I, a, b, c, d, M(8), 6, 0x6fa87e4fu)
    WRENC_MD5_STEP(WRENC_MD5_I, d, a, b, c, M(15), 10, 0xfe2ce6e0u)
    WRENC_MD5_STEP(WRENC_MD5_I, c, d, a, b, M(6), 15, 0xa3014314u)
    WRENC_MD5_STEP(WRENC_MD5_I, b, c, d, a, M(13), 21, 0x4e0811a1u)
    WRENC_MD5_STEP(WRENC_MD5_I, a, b, c, d, M(4), 6, 0xf7537e82u)
    WRENC_MD5_STEP(WRENC_MD5_I, d, a, b, c, M(11), 10, 0xbd3af235u)
    WRENC_MD5_STEP(WRENC_MD5_I, c, d, a, b, M(2), 15, 0x2ad7d2bbu)
    WRENC_MD5_STEP(WRENC_MD5_I, b, c, d, a, M(9), 21, 0xeb86d391u)
#undef M
    st[0] += a;
    st[1] += b;
    st[2] += c;
    st[3] += d;
}
#undef WRENC_MD5_STEP
#undef WRENC_MD5_F
#undef WRENC_MD5_G
#undef WRENC_MD5_H
#undef WRENC_MD5_I

// waves of the MD5 pass over n pictures: the luma planes' lanes first, the chroma planes' (Cb and Cr of a picture side by
// side) in waves of their own behind them
__host__ __device__ inline int md5_luma_waves(int n) { return (n + 63) / 64; }
__host__ __device__ inline int md5_waves(int n) { return md5_luma_waves(n) + (2 * n + 63) / 64; }

// One lane per (picture, plane), one wave per workgroup.  The digest goes to out[picture].value[plane] in digest order.
__global__ __launch_bounds__(64) void hash_md5_kernel(const PicBufs* __restrict__ slots, int first_slot, int n_pics, int W, int H,
                                                      wrenc_picture_hash* __restrict__ out) {
    const int lane = (int)threadIdx.x, luma_waves = md5_luma_waves(n_pics);
    const bool chroma = (int)blockIdx.x >= luma_waves;
    const int idx = ((int)blockIdx.x - (chroma ? luma_waves : 0)) * 64 + lane;
    if (idx >= (chroma ? 2 * n_pics : n_pics)) return;
    const int pic = chroma ? idx >> 1 : idx, plane = chroma ? 1 + (idx & 1) : 0;
    const HashPlane P = hash_plane(W, H, chroma ? 1 : 0);
    const GlobalRow rec = (GlobalRow)slots[first_slot + pic].rec[plane];
    const int blocks = P.bytes >> 6;
    uint32_t st[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    Dwords4 cur[4], nxt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cur[k] = rec[k];
    for (int b = 0; b < blocks; ++b) {
        const int nb = min(b + 1, blocks - 1); // (the last turn loads its own block again)
#pragma unroll
        for (int k = 0; k < 4; ++k) nxt[k] = rec[(size_t)nb * 4 + k];
        md5_block(st, cur);
#pragma unroll
        for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
    }
    const unsigned long long bits = (unsigned long long)P.bytes * 8;
    const Dwords4 zero = {0u, 0u, 0u, 0u};
    cur[0] = Dwords4{0x80u, 0u, 0u, 0u};
    cur[1] = zero;
    cur[2] = zero;
    cur[3] = Dwords4{0u, 0u, (uint32_t)bits, (uint32_t)(bits >> 32)};
    md5_block(st, cur);
    *(Dwords4*)out[pic].value[plane] = Dwords4{st[0], st[1], st[2], st[3]};
}

} // namespace wrenc
