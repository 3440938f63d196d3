// distcurve_quant.h -- the distortion curve's quantiser (include/wrenc_distcurve.h: l = (m + T / 2) / T, e = m - l T) without
// an integer division, as dev_distcurve.h's kernel runs it 64 times per coefficient.  Plain C++, for the device and for the
// host (tools/sanitize/rate_quality.cpp compares it with the definition at every m and every QP).
//
// T(q) is known at compile time, so the division is one multiplication by the constant 1 / T and one truncation, in
// binary32: m = 8 |c| <= 130,560 is exact there.  The quotient is taken half a unit up,
//     x = (m + T / 2 + 1/2) / T        (T / 2 the integer),
// which has the same floor as (m + T / 2) / T and lies at least 1 / (2 T) from every integer.  What the fused multiply-add
// fma(m, fl(1 / T), fl((T / 2 + 1/2) / T)) returns differs from x by at most 2^-23 (m / T + 1) -- one rounding of 1 / T, one
// of the sum, and the constant's -- and 2^-23 (130,560 + T) / T < 1 / (2 T) by a factor of 30: the truncation is the floor
// of the exact quotient for every m and every QP.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define WRENC_DQ_FN __host__ __device__ __forceinline__
#else
#define WRENC_DQ_FN inline
#endif

namespace wrenc {

constexpr int dq_step(int q) { // wrenc_distcurve_step
    constexpr int g[6] = {40, 45, 51, 57, 64, 72};
    return g[q % 6] << (q / 6);
}

// a product of factors within +-2^23: the full-rate 24-bit multiplier on the device (a 32-bit one runs at a quarter)
WRENC_DQ_FN int32_t dq_mul24(int32_t a, int32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

// e e of m = 8 |c|, given as a float, at QP Q.  l <= 3,265, T <= 58,368, l T <= m + T / 2 < 2^18, |e| <= 29,184.
template <int Q>
WRENC_DQ_FN uint32_t dq_error2(float mf) {
    constexpr int32_t T = dq_step(Q);
    constexpr float R = (float)(1.0 / T), B = (float)((T / 2 + 0.5) / T);
    const float l = __builtin_truncf(__builtin_fmaf(mf, R, B));
    // m - l T in binary32 as well: l T < 2^18 and the result are integers, the one rounding has nothing to round (an integer
    // multiply-add by a constant compiles to the 64-bit v_mad_u64_u32 here)
    const int32_t e = (int32_t)__builtin_fmaf(l, (float)-T, mf);
    return (uint32_t)dq_mul24(e, e);
}

} // namespace wrenc
