/* wrenc_format.h -- the pixel formats of an upload (include/wrenc_gpu.h: wrenc_gpu_set_source_format) and their conversion
 * to the planar 8-bit 4:2:0 picture the rest of the library sees, in exact integers.
 *
 * Host only: no device, no threads, no I/O, no allocation.  libwrenc_gpu.so exports the names and the layout as
 * wrenc_gpu_format_from_name, wrenc_gpu_format_name and wrenc_gpu_format_layout; the device's converter
 * (wrenc_amd/csrc/dev_format.h) meets the sample rules bit for bit; tests/format_ref.py restates them in Python.
 *
 * Formats, named as ffmpeg names them; the ids are stable and 0 is the plain behaviour.  w x h is the size of the caller's
 * pictures (the context's source size), both even:
 *     id  name         planes                                                   sample
 *     0   yuv420p      Y w x h, Cb w/2 x h/2, Cr w/2 x h/2                      u8
 *     1   nv12         Y w x h, CbCr interleaved (w/2 pairs) x h/2              u8
 *     2   yuv420p10le  as 0                                                     u16 little-endian, value in the low 10 bits
 *     3   p010le       as 1                                                     u16 little-endian, value in the HIGH 10 bits
 *     4   yuv422p      Y w x h, Cb w/2 x h, Cr w/2 x h                          u8
 *     5   yuv422p10le  as 4                                                     u16 little-endian, low 10 bits
 *
 * These are layouts of Y'CbCr samples: nothing here changes colour or range.  RGB sources, and with them the colour matrix
 * and the range, live in wrenc_rgb.h (wrenc_gpu_set_source_rgb), with layout ids of their own.
 *
 * Conversion, no dithering.
 *   The 10-bit value s of a word v:  low-bit formats s = min(v, 1023) -- stray high bits saturate, they do not wrap;
 *                                    p010le s = v >> 6 -- the low six bits are ignored.
 *   A sample at full chroma resolution (luma of every format, chroma of the 4:2:0 formats):
 *                                    8-bit formats the byte itself;  10-bit formats min((s + 2) >> 2, 255).
 *   4:2:2 chroma -> 4:2:0:           output row j is the mean of source rows 2j and 2j + 1 (the stream says
 *                                    sps_chroma_vertical_collocated_flag = 0: a 4:2:0 chroma row sits midway between two
 *                                    luma rows, and the two 4:2:2 rows sit on those luma rows):
 *                                    8-bit (a + b + 1) >> 1;  10-bit, rounded once from the 10-bit values,
 *                                    min((sa + sb + 4) >> 3, 255).
 * Order: conversion comes BEFORE scaling.  The scaler (wrenc_scale.h) takes the converted 8-bit planes of the source size:
 * its int16 intermediate is sized for 8-bit input.
 */
#ifndef WRENC_FORMAT_H
#define WRENC_FORMAT_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

enum {
    WRENC_FORMAT_YUV420P = 0,
    WRENC_FORMAT_NV12 = 1,
    WRENC_FORMAT_YUV420P10LE = 2,
    WRENC_FORMAT_P010LE = 3,
    WRENC_FORMAT_YUV422P = 4,
    WRENC_FORMAT_YUV422P10LE = 5,
    WRENC_FORMAT_COUNT = 6
};

/* A tightly packed frame of one format as it lies in a raw file: plane p is rows[p] rows of row_bytes[p] bytes from byte
 * offset[p] of the frame on.  Two-plane formats leave the third entry 0. */
struct wrenc_gpu_format_layout {
    int n_planes;          /* 2 or 3 */
    int bytes_per_sample;  /* 1 or 2 */
    size_t row_bytes[3];
    size_t rows[3];
    size_t offset[3];
    size_t frame_bytes;
};

static inline int wrenc_format_valid(int format) { return format >= 0 && format < WRENC_FORMAT_COUNT; }
static inline int wrenc_format_bytes(int format) { return format == WRENC_FORMAT_YUV420P10LE || format == WRENC_FORMAT_P010LE || format == WRENC_FORMAT_YUV422P10LE ? 2 : 1; }
static inline int wrenc_format_interleaved(int format) { return format == WRENC_FORMAT_NV12 || format == WRENC_FORMAT_P010LE; }
static inline int wrenc_format_is422(int format) { return format == WRENC_FORMAT_YUV422P || format == WRENC_FORMAT_YUV422P10LE; }

static inline const char* wrenc_format_name(int format) {
    static const char* const names[WRENC_FORMAT_COUNT] = {"yuv420p", "nv12", "yuv420p10le", "p010le", "yuv422p", "yuv422p10le"};
    return wrenc_format_valid(format) ? names[format] : NULL;
}

static inline int wrenc_format_from_name(const char* name) { /* the id, or -1 */
    if (!name) return -1;
    for (int f = 0; f < WRENC_FORMAT_COUNT; ++f)
        if (!strcmp(name, wrenc_format_name(f))) return f;
    return -1;
}

/* 0, or -1 for an unknown format, an odd w or h, w or h below 16, or a null pointer. */
static inline int wrenc_format_layout(int format, int w, int h, struct wrenc_gpu_format_layout* out) {
    if (!out || !wrenc_format_valid(format) || w < 16 || h < 16 || (w & 1) || (h & 1)) return -1;
    const size_t bps = (size_t)wrenc_format_bytes(format);
    const size_t chroma_rows = wrenc_format_is422(format) ? (size_t)h : (size_t)h / 2;
    memset(out, 0, sizeof *out);
    out->bytes_per_sample = (int)bps;
    out->row_bytes[0] = (size_t)w * bps;
    out->rows[0] = (size_t)h;
    if (wrenc_format_interleaved(format)) {
        out->n_planes = 2;
        out->row_bytes[1] = (size_t)w * bps; /* w/2 pairs */
        out->rows[1] = chroma_rows;
    } else {
        out->n_planes = 3;
        out->row_bytes[1] = out->row_bytes[2] = (size_t)(w / 2) * bps;
        out->rows[1] = out->rows[2] = chroma_rows;
    }
    size_t at = 0;
    for (int p = 0; p < out->n_planes; ++p) {
        out->offset[p] = at;
        at += out->row_bytes[p] * out->rows[p];
    }
    out->frame_bytes = at;
    return 0;
}

/* The sample rules, one word at a time (v: a byte of an 8-bit format, a 16-bit word of a 10-bit one). */
static inline int wrenc_format_s10(int format, int v) { return format == WRENC_FORMAT_P010LE ? (v & 0xFFFF) >> 6 : (v < 1023 ? v : 1023); }
static inline int wrenc_format_sample(int format, int v) {
    if (wrenc_format_bytes(format) == 1) return v;
    const int o = (wrenc_format_s10(format, v) + 2) >> 2;
    return o < 255 ? o : 255;
}
static inline int wrenc_format_chroma422(int format, int a, int b) { /* rows 2j and 2j + 1 of a 4:2:2 chroma plane */
    if (wrenc_format_bytes(format) == 1) return (a + b + 1) >> 1;
    const int o = (wrenc_format_s10(format, a) + wrenc_format_s10(format, b) + 4) >> 3;
    return o < 255 ? o : 255;
}

#endif /* WRENC_FORMAT_H */
