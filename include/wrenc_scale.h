/* wrenc_scale.h -- the resampling filter of a scaling upload (include/wrenc_gpu.h: wrenc_gpu_set_source_size): the taps
 * of one output sample of one axis, in exact integers.
 *
 * Host only: no device, no threads, no I/O, no allocation.  libwrenc_gpu.so builds the device's tables from it and
 * exports it as wrenc_gpu_scale_taps; tests/scale_ref.py restates it in Python.
 *
 * Definition.  Each plane is resampled on its own, luma sw x sh -> vw x vh, each chroma plane sw/2 x sh/2 -> vw/2 x vh/2,
 * separably: all rows horizontally, then all columns vertically.  Samples are centre-aligned; the kernel is Catmull-Rom,
 * stretched by the ratio when shrinking.  For one axis n_in -> n_out and output index o:
 *     D = 2 n_out,  C = (2 o + 1) n_in - n_out  (the centre is C / D in input samples),  M = 2 max(n_in, n_out).
 * Taps: every integer i with N = |i D - C| < 2 M, ascending; i may lie outside the plane.  Weight times 2 M^3:
 *     N < M:        W = 3 N^3 - 5 N^2 M + 2 M^3
 *     M <= N < 2M:  W = -N^3 + 5 N^2 M - 8 N M^2 + 4 M^3
 * Coefficients, with T = sum W (> 0): k_i = floor((8192 W_i + T) / (2 T)), a floor division also for negative weights;
 * then 4096 - sum k_i is added to the tap with the largest W (the lowest i on a tie), so that they sum to 4096.
 * Taps at either end of the list whose coefficient came out as 0 are not listed (they add nothing to any sum): n_in ==
 * n_out, whose neighbours sit at N = M where W = 0, is the single tap 4096.
 * Edges: a tap outside [0, n_in - 1] reads the nearest edge sample.
 * Passes: horizontal t = (sum k x + 32) >> 6, an arithmetic shift, t a signed 16-bit intermediate; vertical
 * out = clip((sum k t + 2^17) >> 18, 0, 255).
 * Limits per axis: n_out <= 4 n_in and n_in <= 4 n_out, which keeps the open interval of the taps at most 16 samples
 * long: never more than 16 taps (WRENC_SCALE_MAX_TAPS leaves room for one more); and both at most WRENC_SCALE_MAX_SIZE,
 * up to which every intermediate fits 64 signed bits (8192 W at n = 16384 is below 2^61).
 */
#ifndef WRENC_SCALE_H
#define WRENC_SCALE_H

#include <stdint.h>

#define WRENC_SCALE_MAX_TAPS 17
#define WRENC_SCALE_MAX_SIZE 16384
#define WRENC_SCALE_UNITY 4096

static inline int64_t wrenc_scale_floor_div(int64_t a, int64_t b) { /* b > 0 */
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

/* The taps of output sample o: *first is the input index of coef[0] (it may be negative, and *first + *n_taps - 1 may
 * exceed n_in - 1: the edge rule), *n_taps their number (1 .. 16).  0, or -1 for sizes outside the limits, o outside
 * [0, n_out - 1] or a null pointer. */
static inline int wrenc_scale_taps(int n_in, int n_out, int o, int* first, int* n_taps, int16_t coef[WRENC_SCALE_MAX_TAPS]) {
    if (!first || !n_taps || !coef) return -1;
    if (n_in <= 0 || n_out <= 0 || n_in > WRENC_SCALE_MAX_SIZE || n_out > WRENC_SCALE_MAX_SIZE) return -1;
    if (n_out > 4 * n_in || n_in > 4 * n_out || o < 0 || o >= n_out) return -1;
    const int64_t D = 2 * (int64_t)n_out, C = (2 * (int64_t)o + 1) * n_in - n_out, M = 2 * (int64_t)(n_in > n_out ? n_in : n_out);
    const int64_t lo = wrenc_scale_floor_div(C - 2 * M, D) + 1;     /* the smallest i with i D > C - 2 M */
    const int64_t hi = -wrenc_scale_floor_div(-(C + 2 * M), D) - 1; /* the largest i with i D < C + 2 M */
    const int n = (int)(hi - lo + 1);
    if (n < 1 || n > WRENC_SCALE_MAX_TAPS) return -1;
    int64_t W[WRENC_SCALE_MAX_TAPS], k[WRENC_SCALE_MAX_TAPS], T = 0;
    int best = 0;
    for (int j = 0; j < n; ++j) {
        int64_t N = (lo + j) * D - C;
        if (N < 0) N = -N;
        W[j] = N < M ? 3 * N * N * N - 5 * N * N * M + 2 * M * M * M : -N * N * N + 5 * N * N * M - 8 * N * M * M + 4 * M * M * M;
        T += W[j];
        if (W[j] > W[best]) best = j;
    }
    if (T <= 0) return -1;
    int64_t sum = 0;
    for (int j = 0; j < n; ++j) {
        k[j] = wrenc_scale_floor_div(8192 * W[j] + T, 2 * T);
        sum += k[j];
    }
    k[best] += WRENC_SCALE_UNITY - sum;
    int a = 0, b = n;
    while (b - a > 1 && k[a] == 0) ++a;
    while (b - a > 1 && k[b - 1] == 0) --b;
    *first = (int)(lo + a);
    *n_taps = b - a;
    for (int j = a; j < b; ++j) coef[j - a] = (int16_t)k[j];
    return 0;
}

#endif /* WRENC_SCALE_H */
