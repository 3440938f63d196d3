/* wrenc_distcurve.h -- the distortion curve of a picture (include/wrenc_gpu.h: wrenc_gpu_download_dist_curve): the squared
 * error that a uniform quantiser of every QP 0 .. 63 leaves in the picture's residual transform coefficients, taken from the
 * originals alone, in exact integers.  The table is QP-independent (it holds all 64 QPs); include/wrenc_rate_quality.h turns
 * it into a PSNR-at-QP prediction.
 *
 * Host only: no device, no threads, no I/O, no allocation.  libwrenc_gpu.so exports the definition as
 * wrenc_gpu_dist_curve_host; the device's kernel (wrenc_amd/csrc/dev_distcurve.h) meets it bit for bit;
 * tests/distcurve_ref.py restates it in Python.
 *
 * Coefficients.  Those of wrenc_ratecurve.h, by its own wrenc_ratecurve_block: every picture-aligned 8x8 block of every plane
 * of the coded picture, the best of DC / V / H from the neighbours' originals, the unnormalised 8x8 Hadamard transform of
 * the residual.  |c| <= 64 * 255 = 16,320.
 * Quantiser.  For q = 0 .. 63 the step is T(q) = g[q % 6] << (q / 6), g = {40, 45, 51, 57, 64, 72}: 64 * 2^((q - 4) / 6) to
 * within 1 %, the codec's step of 2^((q - 4) / 6) in the units of m = 8 |c| (the transform's gain of 8 per sample of an 8x8
 * block, times 8).  The level is l = (m + T / 2) / T (integer division: round to nearest, halves up) and the error
 * e = m - l T, so |e| <= min(m, T / 2): m <= 130,560, T <= T(63) = 57 << 10 = 58,368, |e| <= 29,184, e e < 2^30, and a
 * picture's sum fits 64 bits at any size the library accepts.
 * Output.  sse8[p][q] = sum e e over the coefficients of plane p = Y, Cb, Cr.  The predicted sample-domain SSE of the plane
 * at QP q is sse8 / 4096: the transform's 64 and the 8 x 8 of m.
 */
#ifndef WRENC_DISTCURVE_H
#define WRENC_DISTCURVE_H

#include "wrenc_ratecurve.h"

#define WRENC_DISTCURVE_QPS 64
#define WRENC_DISTCURVE_MAX_M (8 * WRENC_RATECURVE_MAX_MAGNITUDE) /* 130,560 */
#define WRENC_DISTCURVE_MAX_ERROR 29184                           /* T(63) / 2 */

typedef struct wrenc_dist_curve {
    uint64_t sse8[3][WRENC_DISTCURVE_QPS]; /* Y, Cb, Cr */
} wrenc_dist_curve;

/* The quantiser step of QP q = 0 .. 63 in the units of m = 8 |c|. */
static inline int32_t wrenc_distcurve_step(int q) {
    static const int32_t g[6] = {40, 45, 51, 57, 64, 72};
    return g[q % 6] << (q / 6);
}

/* The squared error of one coefficient c (|c| <= 16,320) at QP q. */
static inline uint64_t wrenc_distcurve_error(int c, int q) {
    const int32_t t = wrenc_distcurve_step(q), m = 8 * (c < 0 ? -c : c);
    const int32_t l = (m + t / 2) / t, e = m - l * t;
    return (uint64_t)((int64_t)e * e);
}

/* One plane of pw x ph samples (multiples of 8) into sse8[64], which is ADDED to. */
static inline void wrenc_distcurve_plane(const uint8_t* plane, size_t pitch, int pw, int ph, uint64_t sse8[WRENC_DISTCURVE_QPS]) {
    int16_t coef[64];
    for (int by = 0; by < ph / 8; ++by)
        for (int bx = 0; bx < pw / 8; ++bx) {
            wrenc_ratecurve_block(plane, pitch, bx, by, coef);
            for (int i = 0; i < 64; ++i)
                if (coef[i])
                    for (int q = 0; q < WRENC_DISTCURVE_QPS; ++q) sse8[q] += wrenc_distcurve_error(coef[i], q);
        }
}

/* A picture of w x h luma samples (multiples of 16, tightly packed planes).  0, or -1 for a bad size or a null pointer. */
static inline int wrenc_distcurve_picture(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int w, int h, wrenc_dist_curve* out) {
    if (!y || !cb || !cr || !out || w < 16 || h < 16 || (w & 15) || (h & 15)) return -1;
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < WRENC_DISTCURVE_QPS; ++q) out->sse8[p][q] = 0;
    wrenc_distcurve_plane(y, (size_t)w, w, h, out->sse8[0]);
    wrenc_distcurve_plane(cb, (size_t)(w / 2), w / 2, h / 2, out->sse8[1]);
    wrenc_distcurve_plane(cr, (size_t)(w / 2), w / 2, h / 2, out->sse8[2]);
    return 0;
}

#endif /* WRENC_DISTCURVE_H */
