// dev_pk16.h -- sample rows as PAIRS of 16-bit values: a lane that holds four samples of a row as one dword runs the
// arithmetic on them two at a time (v_pk_add/sub/min/max/mad/ashrrev/lshrrev_i16, v_perm_b32) instead of one 32-bit
// operation per sample.  Plain C++ on two-element short vectors; every helper states the range it relies on, and
// tests/pk16_model.py holds each against the scalar formula it replaces (explicit i16 wrap-around).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef short pk16 __attribute__((ext_vector_type(2)));
typedef unsigned short upk16 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ pk16 pk16_from_bits(uint32_t w) { return __builtin_bit_cast(pk16, w); }
__device__ __forceinline__ uint32_t pk16_bits(pk16 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ pk16 pk16_splat(int v) { return pk16{(short)v, (short)v}; }
// a + b mod 2^16 per element (unsigned elements: a signed vector add that overflows would be undefined): v_pk_add_u16
__device__ __forceinline__ pk16 pk16_add_wrap(pk16 a, pk16 b) {
    return __builtin_bit_cast(pk16, __builtin_bit_cast(upk16, a) + __builtin_bit_cast(upk16, b));
}

// bytes 0, 1 / bytes 2, 3 of a dword of samples as two i16 (zero-extended): one v_perm_b32 each
__device__ __forceinline__ pk16 pk16_lo(uint32_t w) { return pk16_from_bits(__builtin_amdgcn_perm(0u, w, 0x0C010C00u)); }
__device__ __forceinline__ pk16 pk16_hi(uint32_t w) { return pk16_from_bits(__builtin_amdgcn_perm(0u, w, 0x0C030C02u)); }
// ... and back: the low bytes of four i16 (samples 0, 1 in a, 2, 3 in b) as one dword.  Exact for values 0..255.
__device__ __forceinline__ uint32_t pk16_pack(pk16 a, pk16 b) {
    return __builtin_amdgcn_perm(pk16_bits(b), pk16_bits(a), 0x06040200u);
}
// clamp to 0..255: v_pk_max_i16 + v_pk_min_i16, any i16 input
__device__ __forceinline__ pk16 pk16_clamp255(pk16 v) {
    return __builtin_elementwise_min(__builtin_elementwise_max(v, pk16_splat(0)), pk16_splat(255));
}

// a * b + c mod 2^16 per element (v_pk_mad_u16; the low 16 bits of a product do not depend on the signs)
__device__ __forceinline__ pk16 pk16_mad(pk16 a, pk16 b, pk16 c) {
    return __builtin_bit_cast(pk16, __builtin_bit_cast(upk16, a) * __builtin_bit_cast(upk16, b) + __builtin_bit_cast(upk16, c));
}
// positions x, x + 1 (x even, 0..30) as a pair
__device__ __forceinline__ pk16 pk16_positions(int x) { return pk16_from_bits((uint32_t)x * 0x10001u + 0x10000u); }

// PDPC weights of two positions (pdpc_w, dev_predict.h): 32 >> sh with sh = (2 x) >> n_scale, 0 once sh exceeds 5.
// Positions 0..31 and n_scale 0..2 give sh <= 62; v_pk_lshrrev_b16 takes four bits of a shift count, so sh is capped at
// 6, where 32 >> 6 = 0 as the rule demands.
__device__ __forceinline__ pk16 pk16_pdpc_w2(int n_scale, pk16 pos) {
    const upk16 sh = (__builtin_bit_cast(upk16, pos) << (unsigned short)1) >> (unsigned short)n_scale;
    const upk16 six = {6, 6}, w32 = {32, 32};
    return __builtin_bit_cast(pk16, w32 >> __builtin_elementwise_min(sh, six));
}

// The PDPC blend of the angular modes, (rs * w + (64 - w) * v + 32) >> 6 as i16 (w64 = 64 - w): w is one of 0, 1, 2, 4,
// 8, 16, 32 and v lies in 0..255; rs lies in -255..510 (mode 18 / 50: side - corner + v) or in 0..255 (the other modes),
// so the sum lies in -8,128..24,512, inside i16: the packed result equals the scalar (int16_t)(...) >> 6.
__device__ __forceinline__ pk16 pk16_pdpc_blend(pk16 rs, pk16 w, pk16 w64, pk16 v) {
    return pk16_mad(w64, v, pk16_mad(rs, w, pk16_splat(32))) >> (short)6;
}

// The same blend with what stays the same from row to row folded once: (s * w + v * wa + wc) >> 6, s the side reference
// (0..255).  Modes 18 / 50 blend rs = s - corner + v: (s - corner + v) w + (64 - w) v + 32 = s w + 64 v + (32 - corner w),
// so wa = 64 and wc = 32 - corner * w; the other modes have rs = s, wa = 64 - w, wc = 32.  The terms are added mod 2^16
// and the whole sum is the one above, inside i16.
__device__ __forceinline__ pk16 pk16_pdpc_blend_folded(pk16 s, pk16 w, pk16 v, pk16 wa, pk16 wc) {
    return pk16_mad(s, w, pk16_mad(v, wa, wc)) >> (short)6;
}

// Two PLANAR samples of row y at positions pos of an n x n block, n = 1 << lg <= 32 (a: the samples above them):
// ((n - 1 - y) a + (y + 1) lb + (n - 1 - x) l + (x + 1) an + n) >> (lg + 1), regrouped as a * ny + x * dl + k with
// ny = n - 1 - y, dl = an - l, k = (n - 1) l + an + (y + 1) lb + n.  The sum is at most 2 * 32 * 255 + 32 = 16,352 and
// never negative, so it is exact in 16 bits (products that leave i16 on the way wrap back) and the shift is logical;
// the result is at most 255: the reference's `as u8` changes nothing.
__device__ __forceinline__ pk16 pk16_planar2(pk16 a, pk16 pos, int ny, int dl, int k, int lg) {
    const pk16 t = pk16_mad(a, pk16_splat(ny), pk16_mad(pos, pk16_splat(dl), pk16_splat(k)));
    return __builtin_bit_cast(pk16, __builtin_bit_cast(upk16, t) >> (unsigned short)(lg + 1));
}
// The PDPC blend of PLANAR and DC, (l * wl + a * wt + (64 - wt - wl) * p + 32) >> 6: wl, wt <= 32 and every sample
// 0..255, so the weights are never negative, the sum is at most 64 * 255 + 32 = 16,352 and the result lies in 0..255 --
// the reference's clamp that follows changes nothing and is not computed.
__device__ __forceinline__ pk16 pk16_planar_dc_blend(pk16 a, pk16 p, pk16 wl, int l, int wt) {
    const pk16 t = pk16_mad(a, pk16_splat(wt), pk16_mad(wl, pk16_splat(l), pk16_splat(32)));
    return pk16_mad(pk16_splat(64 - wt) - wl, p, t) >> (short)6;
}

// Not here: the residual (emit_row4) and the reconstruction with its squared error (recon_row4) as pairs.  Both were
// built and measured: 29 -> 15 vector instructions per row of the reconstruction, and a
// headline gain inside the measurement's spread twice, so those rows stay scalar.
