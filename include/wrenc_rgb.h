/* wrenc_rgb.h -- RGB sources of an upload (include/wrenc_gpu.h: wrenc_gpu_set_source_rgb) and their conversion to the planar
 * 8-bit 4:2:0 Y'CbCr picture the rest of the library sees, in exact integers.  wrenc_format.h holds the YUV layouts and does
 * no colour or range conversion; colour conversion lives here.
 *
 * Host only: no device, no threads, no I/O, no allocation.  libwrenc_gpu.so exports the names, the layout, the coefficients
 * and the whole-picture converter as wrenc_gpu_rgb_from_name, _rgb_name, _rgb_layout, _rgb_coefficients and
 * _rgb_convert_host; the device's converter (wrenc_amd/csrc/dev_rgb.h) meets the rules bit for bit; tests/rgb_ref.py restates
 * them in Python.
 *
 * Layouts, named as ffmpeg names them; an id space of their own, separate from the format ids of wrenc_format.h.  w x h is
 * the size of the caller's pictures (the context's source size), both even, at least 16:
 *     id  name    planes                                               notes
 *     0   rgb24   one plane of packed R,G,B bytes, 3w bytes a row
 *     1   bgr24   one plane of packed B,G,R bytes
 *     2   rgb0    one plane of R,G,B,X, 4w bytes a row                 X is ignored; "rgba" is an accepted alias
 *     3   bgr0    one plane of B,G,R,X                                 "bgra" is an accepted alias
 *     4   gbrp    three planes G, B, R of w x h bytes
 * Matrix: bt709 = 0, bt601 = 1.  Range: tv = 0 (limited: Y' 16..235, chroma 16..240), pc = 1 (full).
 *
 * Rules.  All arithmetic is 32-bit, >> is an arithmetic shift; the offsets keep every accumulator non-negative.
 *     Y (x, y) = clip255((yr*R + yg*G + yb*B + (yoff << 14) + (1 << 13)) >> 14)       per pixel
 *     Cb(i, j) = clip255((br*SR + bg*SG + bb*SB + (128 << 16) + (1 << 15)) >> 16)     SR, SG, SB: the sums of the four
 *     Cr(i, j) = clip255((rr*SR + rg*SG + rb*SB + (128 << 16) + (1 << 15)) >> 16)     pixels (2i..2i+1, 2j..2j+1)
 * The 2x2 mean is the siting the stream itself signals (both sps_chroma_*_collocated_flag are 0); it is rounded once.
 * Coefficients, with Kr, Kb of the matrix, sy = 219/255 and sc = 224/255 for tv, 1 for pc:
 *     yr = round(Kr sy 2^14), yb = round(Kb sy 2^14), yg = round(sy 2^14) - yr - yb                    grey is exact
 *     bb = rr = round(sc 2^13), br = round(-Kr / (2 (1 - Kb)) sc 2^14), bg = -bb - br, Cr likewise     grey is exactly 128
 *                yr, yg, yb           br, bg, bb             rr, rg, rb             yoff
 *     bt709 tv   2991, 10064, 1016    -1649, -5547, 7196     7196, -6536, -660      16
 *     bt709 pc   3483, 11718, 1183    -1877, -6315, 8192     8192, -7441, -751      0
 *     bt601 tv   4207, 8260, 1604     -2428, -4768, 7196     7196, -6026, -1170     16
 *     bt601 pc   4899, 9617, 1868     -2765, -5427, 8192     8192, -6860, -1332     0
 * The clip is live only for pc chroma: pure red and pure blue reach 256 before it.
 * No dithering, no gamma, no primaries conversion.  Order: conversion comes BEFORE scaling, as for the YUV formats.
 * The stream carries no VUI, so matrix and range are NOT signalled in it: a player assumes what it assumes for untagged
 * video (usually bt709 tv at HD sizes, bt601 tv below); say the pair to the container or the player where it matters.
 */
#ifndef WRENC_RGB_H
#define WRENC_RGB_H

#include "wrenc_format.h"

enum { WRENC_RGB_RGB24 = 0, WRENC_RGB_BGR24 = 1, WRENC_RGB_RGB0 = 2, WRENC_RGB_BGR0 = 3, WRENC_RGB_GBRP = 4, WRENC_RGB_COUNT = 5 };
enum { WRENC_RGB_BT709 = 0, WRENC_RGB_BT601 = 1, WRENC_RGB_MATRIX_COUNT = 2 };
enum { WRENC_RGB_TV = 0, WRENC_RGB_PC = 1, WRENC_RGB_RANGE_COUNT = 2 };

static inline int wrenc_rgb_valid(int layout) { return layout >= 0 && layout < WRENC_RGB_COUNT; }
static inline int wrenc_rgb_matrix_valid(int matrix) { return matrix >= 0 && matrix < WRENC_RGB_MATRIX_COUNT; }
static inline int wrenc_rgb_range_valid(int range) { return range >= 0 && range < WRENC_RGB_RANGE_COUNT; }
static inline int wrenc_rgb_planar(int layout) { return layout == WRENC_RGB_GBRP; }
/* bytes of a pixel in the one plane of a packed layout; 1 for gbrp */
static inline int wrenc_rgb_pixel_bytes(int layout) { return layout == WRENC_RGB_GBRP ? 1 : layout >= WRENC_RGB_RGB0 ? 4 : 3; }

static inline const char* wrenc_rgb_name(int layout) {
    static const char* const names[WRENC_RGB_COUNT] = {"rgb24", "bgr24", "rgb0", "bgr0", "gbrp"};
    return wrenc_rgb_valid(layout) ? names[layout] : NULL;
}

static inline int wrenc_rgb_from_name(const char* name) { /* the id, or -1 */
    if (!name) return -1;
    for (int l = 0; l < WRENC_RGB_COUNT; ++l)
        if (!strcmp(name, wrenc_rgb_name(l))) return l;
    if (!strcmp(name, "rgba")) return WRENC_RGB_RGB0;
    if (!strcmp(name, "bgra")) return WRENC_RGB_BGR0;
    return -1;
}
static inline int wrenc_rgb_matrix_from_name(const char* name) { return !name ? -1 : !strcmp(name, "bt709") ? 0 : !strcmp(name, "bt601") ? 1 : -1; }
static inline int wrenc_rgb_range_from_name(const char* name) { return !name ? -1 : !strcmp(name, "tv") ? 0 : !strcmp(name, "pc") ? 1 : -1; }

/* 0, or -1 for an unknown layout, an odd w or h, w or h below 16, or a null pointer (the limits of wrenc_format_layout). */
static inline int wrenc_rgb_layout(int layout, int w, int h, struct wrenc_gpu_format_layout* out) {
    if (!out || !wrenc_rgb_valid(layout) || w < 16 || h < 16 || (w & 1) || (h & 1)) return -1;
    memset(out, 0, sizeof *out);
    out->bytes_per_sample = 1;
    out->n_planes = wrenc_rgb_planar(layout) ? 3 : 1;
    size_t at = 0;
    for (int p = 0; p < out->n_planes; ++p) {
        out->row_bytes[p] = (size_t)w * (size_t)wrenc_rgb_pixel_bytes(layout);
        out->rows[p] = (size_t)h;
        out->offset[p] = at;
        at += out->row_bytes[p] * out->rows[p];
    }
    out->frame_bytes = at;
    return 0;
}

/* yr yg yb | br bg bb | rr rg rb | yoff.  0, or -1 for an unknown matrix or range or a null pointer. */
static inline int wrenc_rgb_coefficients(int matrix, int range, int out[10]) {
    static const int table[WRENC_RGB_MATRIX_COUNT][WRENC_RGB_RANGE_COUNT][10] = {
        {{2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660, 16}, {3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751, 0}},
        {{4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170, 16}, {4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332, 0}}};
    if (!out || !wrenc_rgb_matrix_valid(matrix) || !wrenc_rgb_range_valid(range)) return -1;
    for (int i = 0; i < 10; ++i) out[i] = table[matrix][range][i];
    return 0;
}

static inline int wrenc_rgb_clip255(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : (int)v; }
/* the sample rules: k the ten numbers of wrenc_rgb_coefficients; sr, sg, sb the sums over a 2x2 block */
static inline int wrenc_rgb_luma(const int k[10], int r, int g, int b) {
    return wrenc_rgb_clip255((int32_t)(k[0] * r + k[1] * g + k[2] * b + (k[9] << 14) + (1 << 13)) >> 14);
}
static inline int wrenc_rgb_cb(const int k[10], int sr, int sg, int sb) {
    return wrenc_rgb_clip255((int32_t)(k[3] * sr + k[4] * sg + k[5] * sb + (128 << 16) + (1 << 15)) >> 16);
}
static inline int wrenc_rgb_cr(const int k[10], int sr, int sg, int sb) {
    return wrenc_rgb_clip255((int32_t)(k[6] * sr + k[7] * sg + k[8] * sb + (128 << 16) + (1 << 15)) >> 16);
}

/* Where R, G and B of pixel x of a row lie: the plane (of wrenc_rgb_layout's numbering) and the byte of the row. */
static inline void wrenc_rgb_locate(int layout, int x, int plane[3], size_t byte[3]) {
    if (wrenc_rgb_planar(layout)) { /* planes G, B, R */
        plane[0] = 2, plane[1] = 0, plane[2] = 1;
        byte[0] = byte[1] = byte[2] = (size_t)x;
        return;
    }
    const size_t at = (size_t)x * (size_t)wrenc_rgb_pixel_bytes(layout);
    const int swap = layout == WRENC_RGB_BGR24 || layout == WRENC_RGB_BGR0;
    plane[0] = plane[1] = plane[2] = 0;
    byte[0] = at + (swap ? 2 : 0), byte[1] = at + 1, byte[2] = at + (swap ? 0 : 2);
}

/* The rules over a whole picture: planes and strides (bytes) as wrenc_rgb_layout numbers them (a packed layout reads
 * plane[0] alone), y of w x h and cb, cr of w/2 x h/2 bytes, tightly packed.  0, or -1 for what the layout or the
 * coefficients refuse, a null pointer that is read, or a stride smaller than the row. */
static inline int wrenc_rgb_convert(int layout, int matrix, int range, int w, int h, const uint8_t* const plane[3], const size_t stride[3],
                                    uint8_t* y, uint8_t* cb, uint8_t* cr) {
    struct wrenc_gpu_format_layout lay;
    int k[10];
    if (wrenc_rgb_layout(layout, w, h, &lay) || wrenc_rgb_coefficients(matrix, range, k) || !plane || !stride || !y || !cb || !cr) return -1;
    for (int p = 0; p < lay.n_planes; ++p)
        if (!plane[p] || stride[p] < lay.row_bytes[p]) return -1;
    for (int j = 0; j < h / 2; ++j)
        for (int i = 0; i < w / 2; ++i) {
            int s[3] = {0, 0, 0};
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx) {
                    const int px = 2 * i + dx, py = 2 * j + dy;
                    int pl[3], c[3];
                    size_t at[3];
                    wrenc_rgb_locate(layout, px, pl, at);
                    for (int q = 0; q < 3; ++q) {
                        c[q] = plane[pl[q]][(size_t)py * stride[pl[q]] + at[q]];
                        s[q] += c[q];
                    }
                    y[(size_t)py * (size_t)w + (size_t)px] = (uint8_t)wrenc_rgb_luma(k, c[0], c[1], c[2]);
                }
            cb[(size_t)j * (size_t)(w / 2) + (size_t)i] = (uint8_t)wrenc_rgb_cb(k, s[0], s[1], s[2]);
            cr[(size_t)j * (size_t)(w / 2) + (size_t)i] = (uint8_t)wrenc_rgb_cr(k, s[0], s[1], s[2]);
        }
    return 0;
}

#endif /* WRENC_RGB_H */
