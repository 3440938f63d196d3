/* wrenc_recon.h -- the reconstruction of a picture as it leaves the library (include/wrenc_gpu.h: wrenc_gpu_download_recon,
 * wrenc_gpu_download_recon_device): crop, interleave and conversion to RGB, in exact integers.  wrenc_rgb.h turned round.
 *
 * Host only: no device, no threads, no I/O, no allocation.  libwrenc_gpu.so exports the names, the layout, the coefficients
 * and the whole-picture converter as wrenc_gpu_recon_from_name, _recon_name, _recon_layout, _recon_coefficients and
 * _recon_convert_host; the device's kernels (wrenc_amd/csrc/dev_recon.h) meet the rules bit for bit; tests/recon_ref.py
 * restates them in Python.
 *
 * The output is a function of the VISIBLE reconstruction alone: the w x h luma plane and the w/2 x h/2 chroma planes a
 * decoder outputs behind the conformance window (w x h: the context's visible size, both even, at least 16).  The margin
 * of a padded context is never read.
 *
 * Output formats: ONE id space, of this header.  Ids 0 .. 4 are the RGB layouts of wrenc_rgb.h with their ids and names,
 * the two YUV outputs follow them (they are NOT the format ids of wrenc_format.h):
 *     id  name     planes                                                notes
 *     0   rgb24    one plane of packed R,G,B bytes, 3w bytes a row
 *     1   bgr24    one plane of packed B,G,R bytes
 *     2   rgb0     one plane of R,G,B,X, 4w bytes a row                  X is written as 255; "rgba" is an accepted alias
 *     3   bgr0     one plane of B,G,R,X                                  "bgra" is an accepted alias
 *     4   gbrp     three planes G, B, R of w x h bytes
 *     5   yuv420p  Y w x h, Cb w/2 x h/2, Cr w/2 x h/2                   the crop
 *     6   nv12     Y w x h, CbCr interleaved (w/2 pairs) x h/2
 * The frame layout is a wrenc_gpu_format_layout (wrenc_format.h), as for the sources.  RGB takes a matrix (bt709 = 0,
 * bt601 = 1) and a range (tv = 0, pc = 1), wrenc_rgb.h's ids; the YUV outputs read neither.
 *
 * Chroma upsampling: centre-sited, as the stream signals (both sps_chroma_*_collocated_flag are 0), bilinear, kept in
 * sixteenths and NOT rounded.  For luma position (x, y), with cw = w/2 and ch = h/2:
 *     i = x >> 1,  i' = clamp(i + ((x & 1) ? 1 : -1), 0, cw - 1)
 *     j = y >> 1,  j' = clamp(j + ((y & 1) ? 1 : -1), 0, ch - 1)
 *     C16 = 9 C(i, j) + 3 C(i', j) + 3 C(i, j') + C(i', j')                    0 .. 4080
 *
 * Conversion.  All arithmetic is 32-bit signed, >> is an arithmetic (floor) shift; each sample is rounded once:
 *     Yd = 16 (Y - yoff),  U = Cb16 - 2048,  V = Cr16 - 2048
 *     R = clip255((cy Yd + rv V        + (1 << 17)) >> 18)
 *     G = clip255((cy Yd + gu U + gv V + (1 << 17)) >> 18)
 *     B = clip255((cy Yd + bu U        + (1 << 17)) >> 18)
 * Coefficients, with Kr, Kb of the matrix, Kg = 1 - Kr - Kb, sy = 219/255, sc = 224/255 and yoff = 16 for tv, 1, 1 and 0
 * for pc:
 *     cy = round(2^14 / sy),  rv = round(2 (1 - Kr) / sc 2^14),  bu = round(2 (1 - Kb) / sc 2^14)
 *     gu = round(-2 Kb (1 - Kb) / (Kg sc) 2^14),  gv = round(-2 Kr (1 - Kr) / (Kg sc) 2^14)
 *                cy      rv      gu      gv       bu      yoff
 *     bt709 tv   19077   29372   -3494   -8731    34610   16
 *     bt709 pc   16384   25802   -3069   -7670    30402   0
 *     bt601 tv   19077   26149   -6419   -13320   33050   16
 *     bt601 pc   16384   22970   -5638   -11700   29032   0
 * What follows from the form:
 *   - Grey (Cb = Cr = 128 everywhere) gives U = V = 0 and so R = G = B exactly.
 *   - Every accumulator stays inside 32 bits: |cy Yd| <= 19077 * 16 * 255 < 2^27, |bu U| <= 34610 * 2048 < 2^27, and G has
 *     two chroma terms of the same sign at most.  bu of the tv tables does NOT fit a signed 16-bit operand.
 *   - Against the real-valued formula on the real-valued bilinear chroma the unclipped result is within
 *     0.5 + (255 + 128 + 128) / 2^15 < 0.516: half a step of the one rounding and half a unit of 2^-14 per coefficient.
 * No dithering, no gamma, no primaries conversion, no scaling.  The stream carries no VUI: matrix and range are the
 * caller's to know (wrenc_rgb.h).
 */
#ifndef WRENC_RECON_H
#define WRENC_RECON_H

#include "wrenc_rgb.h"

enum { WRENC_RECON_YUV420P = WRENC_RGB_COUNT, WRENC_RECON_NV12 = WRENC_RGB_COUNT + 1, WRENC_RECON_COUNT = WRENC_RGB_COUNT + 2 };

static inline int wrenc_recon_valid(int format) { return format >= 0 && format < WRENC_RECON_COUNT; }
static inline int wrenc_recon_is_rgb(int format) { return wrenc_rgb_valid(format); }

static inline const char* wrenc_recon_name(int format) {
    if (wrenc_recon_is_rgb(format)) return wrenc_rgb_name(format);
    return format == WRENC_RECON_YUV420P ? "yuv420p" : format == WRENC_RECON_NV12 ? "nv12" : NULL;
}

static inline int wrenc_recon_from_name(const char* name) { /* the id, or -1 */
    if (!name) return -1;
    if (!strcmp(name, "yuv420p")) return WRENC_RECON_YUV420P;
    if (!strcmp(name, "nv12")) return WRENC_RECON_NV12;
    return wrenc_rgb_from_name(name);
}

/* 0, or -1 for an unknown format, an odd w or h, w or h below 16, or a null pointer (the limits of wrenc_format_layout). */
static inline int wrenc_recon_layout(int format, int w, int h, struct wrenc_gpu_format_layout* out) {
    if (wrenc_recon_is_rgb(format)) return wrenc_rgb_layout(format, w, h, out);
    if (format == WRENC_RECON_YUV420P) return wrenc_format_layout(WRENC_FORMAT_YUV420P, w, h, out);
    if (format == WRENC_RECON_NV12) return wrenc_format_layout(WRENC_FORMAT_NV12, w, h, out);
    return -1;
}

/* cy rv gu gv bu | yoff.  0, or -1 for an unknown matrix or range or a null pointer. */
static inline int wrenc_recon_coefficients(int matrix, int range, int out[6]) {
    static const int table[WRENC_RGB_MATRIX_COUNT][WRENC_RGB_RANGE_COUNT][6] = {
        {{19077, 29372, -3494, -8731, 34610, 16}, {16384, 25802, -3069, -7670, 30402, 0}},
        {{19077, 26149, -6419, -13320, 33050, 16}, {16384, 22970, -5638, -11700, 29032, 0}}};
    if (!out || !wrenc_rgb_matrix_valid(matrix) || !wrenc_rgb_range_valid(range)) return -1;
    for (int i = 0; i < 6; ++i) out[i] = table[matrix][range][i];
    return 0;
}

/* the sample rules.  Chroma in sixteenths at luma position (x, y) of a cw x ch plane `c`, tightly packed */
static inline int wrenc_recon_chroma16(const uint8_t* c, int cw, int ch, int x, int y) {
    const int i = x >> 1, j = y >> 1;
    int i2 = i + ((x & 1) ? 1 : -1), j2 = j + ((y & 1) ? 1 : -1);
    i2 = i2 < 0 ? 0 : i2 > cw - 1 ? cw - 1 : i2;
    j2 = j2 < 0 ? 0 : j2 > ch - 1 ? ch - 1 : j2;
    const uint8_t *a = c + (size_t)j * (size_t)cw, *b = c + (size_t)j2 * (size_t)cw;
    return 9 * a[i] + 3 * a[i2] + 3 * b[i] + b[i2];
}
/* k: the six numbers of wrenc_recon_coefficients; y the luma sample, cb16 and cr16 the chroma in sixteenths; the unclipped
 * R, G, B before the clip (wrenc_recon_rgb clips them) */
static inline void wrenc_recon_rgb_unclipped(const int k[6], int y, int cb16, int cr16, int32_t rgb[3]) {
    const int32_t yd = 16 * (y - k[5]), u = cb16 - 2048, v = cr16 - 2048;
    rgb[0] = (int32_t)(k[0] * yd + k[1] * v + (1 << 17)) >> 18;
    rgb[1] = (int32_t)(k[0] * yd + k[2] * u + k[3] * v + (1 << 17)) >> 18;
    rgb[2] = (int32_t)(k[0] * yd + k[4] * u + (1 << 17)) >> 18;
}
static inline void wrenc_recon_rgb(const int k[6], int y, int cb16, int cr16, int rgb[3]) {
    int32_t t[3];
    wrenc_recon_rgb_unclipped(k, y, cb16, cr16, t);
    for (int q = 0; q < 3; ++q) rgb[q] = wrenc_rgb_clip255(t[q]);
}

/* The rules over a whole picture: y of w x h and cb, cr of w/2 x h/2 bytes, tightly packed (the visible reconstruction),
 * to planes and strides (bytes) as wrenc_recon_layout numbers them (a packed layout writes plane[0] alone, nv12 two
 * planes).  Only the bytes of the layout's rows are written.  matrix and range are not read for the YUV outputs.  0, or -1
 * for what the layout or the coefficients refuse, a null pointer that is used, or a stride smaller than the row. */
static inline int wrenc_recon_convert(int format, int matrix, int range, int w, int h, const uint8_t* y, const uint8_t* cb, const uint8_t* cr,
                                      uint8_t* const plane[3], const size_t stride[3]) {
    struct wrenc_gpu_format_layout lay;
    int k[6] = {0, 0, 0, 0, 0, 0};
    if (wrenc_recon_layout(format, w, h, &lay) || !plane || !stride || !y || !cb || !cr) return -1;
    if (wrenc_recon_is_rgb(format) && wrenc_recon_coefficients(matrix, range, k)) return -1;
    for (int p = 0; p < lay.n_planes; ++p)
        if (!plane[p] || stride[p] < lay.row_bytes[p]) return -1;
    const int cw = w / 2, ch = h / 2;
    if (!wrenc_recon_is_rgb(format)) {
        for (int r = 0; r < h; ++r) memcpy(plane[0] + (size_t)r * stride[0], y + (size_t)r * (size_t)w, (size_t)w);
        for (int r = 0; r < ch; ++r) {
            const uint8_t *b = cb + (size_t)r * (size_t)cw, *c = cr + (size_t)r * (size_t)cw;
            if (format == WRENC_RECON_NV12) {
                uint8_t* d = plane[1] + (size_t)r * stride[1];
                for (int i = 0; i < cw; ++i) d[2 * i] = b[i], d[2 * i + 1] = c[i];
            } else {
                memcpy(plane[1] + (size_t)r * stride[1], b, (size_t)cw);
                memcpy(plane[2] + (size_t)r * stride[2], c, (size_t)cw);
            }
        }
        return 0;
    }
    for (int py = 0; py < h; ++py)
        for (int px = 0; px < w; ++px) {
            int rgb[3], pl[3];
            size_t at[3];
            wrenc_recon_rgb(k, y[(size_t)py * (size_t)w + (size_t)px], wrenc_recon_chroma16(cb, cw, ch, px, py), wrenc_recon_chroma16(cr, cw, ch, px, py), rgb);
            wrenc_rgb_locate(format, px, pl, at);
            for (int q = 0; q < 3; ++q) plane[pl[q]][(size_t)py * stride[pl[q]] + at[q]] = (uint8_t)rgb[q];
            if (wrenc_rgb_pixel_bytes(format) == 4) plane[0][(size_t)py * stride[0] + 4 * (size_t)px + 3] = 255;
        }
    return 0;
}

#endif /* WRENC_RECON_H */
