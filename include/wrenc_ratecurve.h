/* wrenc_ratecurve.h -- the rate histogram of a picture (include/wrenc_gpu.h: wrenc_gpu_download_rate_hist): how many of its
 * residual transform coefficients have which magnitude, taken from the originals alone, in exact integers.  The histogram is
 * QP-independent; include/wrenc_rate.h turns it into a bytes-at-QP curve.
 *
 * Host only: no device, no threads, no I/O, no allocation.  libwrenc_gpu.so exports the definition as
 * wrenc_gpu_rate_hist_bin and wrenc_gpu_rate_hist_host; the device's kernel (wrenc_amd/csrc/dev_ratecurve.h) meets it bit
 * for bit; tests/ratecurve_ref.py restates it in Python.
 *
 * Blocks.  Every picture-aligned 8x8 block of every plane of the coded picture (Y at W x H, Cb and Cr at W/2 x H/2, W and H
 * multiples of 32), the margin of a padded picture included.  Block (bx, by) of a plane P has the samples
 * s(x, y) = P[8 by + y][8 bx + x], x, y = 0..7.
 * Prediction, from the ORIGINALS of the neighbours, so that no block depends on another:
 *     top(x)  = P[8 by - 1][8 bx + x]   exists when by > 0
 *     left(y) = P[8 by + y][8 bx - 1]   exists when bx > 0
 *     DC: every sample is d = (sum top + sum left + 8) >> 4 with both, (sum top + 4) >> 3 or (sum left + 4) >> 3 with
 *         one, 128 with neither
 *     V:  p(x, y) = top(x), only when top exists
 *     H:  p(x, y) = left(y), only when left exists
 *   The candidate with the least SAD = sum |s - p| wins; candidates are tried in the order DC, V, H and a later one wins
 *   only with a strictly smaller SAD.
 * Transform.  r = s - p (within +-255); c = H8 r H8, H8 the unnormalised 8x8 Hadamard matrix of +-1 (natural order; the
 * order does not matter to a histogram), DC included.  |c| <= 64 * 255 = 16,320: 16-bit arithmetic holds every stage.
 * Binning.  m = |c|.  bin(0) = 0; otherwise with e = floor(log2 m): bin = 1 + 4 e + the two bits of m below the leading
 * one (bits that m does not have read as 0: bin(1) = 1, bin(2) = 5, bin(3) = 7, bin(4) = 9, bin(7) = 12, bin(8) = 13).
 * bin(16,320) = 56 is the largest; a table has 64 entries, 57..63 stay 0.
 * Output.  count[p][b], 64-bit, p = Y, Cb, Cr: the number of coefficients of plane p in bin b.  sum_b count[p][b] is the
 * plane's sample count.
 */
#ifndef WRENC_RATECURVE_H
#define WRENC_RATECURVE_H

#include <stddef.h>
#include <stdint.h>

#define WRENC_RATECURVE_BINS 64
#define WRENC_RATECURVE_TOP_BIN 56
#define WRENC_RATECURVE_MAX_MAGNITUDE 16320

typedef struct wrenc_rate_hist {
    uint64_t count[3][WRENC_RATECURVE_BINS]; /* Y, Cb, Cr */
} wrenc_rate_hist;

/* The bin of a magnitude 0 .. 16,320. */
static inline int wrenc_ratecurve_bin(int m) {
    if (m <= 0) return 0;
    int e = 0;
    while ((m >> e) > 1) ++e;
    return 1 + 4 * e + (((m << 2) >> e) & 3);
}

/* The smallest magnitude of a bin 0 .. 56 (bins 2, 3, 4, 6 and 8 hold nothing: bits that 1, 2 and 3 do not have). */
static inline int wrenc_ratecurve_bin_floor(int bin) {
    if (bin <= 0) return 0;
    const int e = (bin - 1) >> 2, f = (bin - 1) & 3;
    return (int)(((4u + (unsigned)f) << e) >> 2);
}

/* The winning prediction of block (bx, by) of a plane of pw x ph samples: pred[8 y + x]. */
static inline void wrenc_ratecurve_predict(const uint8_t* plane, size_t pitch, int bx, int by, uint8_t pred[64]) {
    const uint8_t* s = plane + (size_t)(8 * by) * pitch + (size_t)(8 * bx);
    const int has_top = by > 0, has_left = bx > 0;
    int top[8] = {0}, left[8] = {0}, sum = 0;
    for (int i = 0; i < 8; ++i) {
        if (has_top) sum += top[i] = s[i - (ptrdiff_t)pitch];
        if (has_left) sum += left[i] = s[(size_t)i * pitch - 1];
    }
    const int dc = has_top && has_left ? (sum + 8) >> 4 : (has_top || has_left ? (sum + 4) >> 3 : 128);
    long sad_dc = 0, sad_v = 0, sad_h = 0;
    for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x) {
            const int v = s[(size_t)y * pitch + x];
            sad_dc += v > dc ? v - dc : dc - v;
            sad_v += v > top[x] ? v - top[x] : top[x] - v;
            sad_h += v > left[y] ? v - left[y] : left[y] - v;
        }
    int best = 0; /* DC, V, H */
    long least = sad_dc;
    if (has_top && sad_v < least) {
        best = 1;
        least = sad_v;
    }
    if (has_left && sad_h < least) best = 2;
    for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x) pred[8 * y + x] = (uint8_t)(best == 0 ? dc : (best == 1 ? top[x] : left[y]));
}

/* The 64 coefficients of block (bx, by). */
static inline void wrenc_ratecurve_block(const uint8_t* plane, size_t pitch, int bx, int by, int16_t coef[64]) {
    uint8_t pred[64];
    wrenc_ratecurve_predict(plane, pitch, bx, by, pred);
    const uint8_t* s = plane + (size_t)(8 * by) * pitch + (size_t)(8 * bx);
    for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x) coef[8 * y + x] = (int16_t)((int)s[(size_t)y * pitch + x] - (int)pred[8 * y + x]);
    for (int h = 1; h < 64; h <<= 1)
        for (int i = 0; i < 64; ++i)
            if (!(i & h)) {
                const int16_t p = coef[i], q = coef[i | h];
                coef[i] = (int16_t)(p + q);
                coef[i | h] = (int16_t)(p - q);
            }
}

/* One plane of pw x ph samples (multiples of 8) into count[64], which is ADDED to. */
static inline void wrenc_ratecurve_plane(const uint8_t* plane, size_t pitch, int pw, int ph, uint64_t count[WRENC_RATECURVE_BINS]) {
    int16_t coef[64];
    for (int by = 0; by < ph / 8; ++by)
        for (int bx = 0; bx < pw / 8; ++bx) {
            wrenc_ratecurve_block(plane, pitch, bx, by, coef);
            for (int i = 0; i < 64; ++i) ++count[wrenc_ratecurve_bin(coef[i] < 0 ? -coef[i] : coef[i])];
        }
}

/* A picture of w x h luma samples (multiples of 16, tightly packed planes).  0, or -1 for a bad size or a null pointer. */
static inline int wrenc_ratecurve_picture(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int w, int h, wrenc_rate_hist* out) {
    if (!y || !cb || !cr || !out || w < 16 || h < 16 || (w & 15) || (h & 15)) return -1;
    for (int p = 0; p < 3; ++p)
        for (int b = 0; b < WRENC_RATECURVE_BINS; ++b) out->count[p][b] = 0;
    wrenc_ratecurve_plane(y, (size_t)w, w, h, out->count[0]);
    wrenc_ratecurve_plane(cb, (size_t)(w / 2), w / 2, h / 2, out->count[1]);
    wrenc_ratecurve_plane(cr, (size_t)(w / 2), w / 2, h / 2, out->count[2]);
    return 0;
}

#endif /* WRENC_RATECURVE_H */
