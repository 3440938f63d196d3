// ASan + UBSan over the source-format converter: the body of convert_format_kernel (wrenc_amd/csrc/dev_format.h) compiled
// for the host -- the HIP qualifiers defined away, blockIdx / threadIdx as globals walked over the launch's grid,
// v_perm_b32 restated -- against the scalar rules of include/wrenc_format.h, for every format at sizes whose rows end inside
// a lane's eight bytes.  The raw staging planes are a heap block of exactly pitch x rows bytes, so a read past them is an
// error the sanitizer reports; the destination is pre-filled, so a byte written outside the picture's rectangle shows.
// Stand-alone (tools/sanitize/run.sh builds it with clang++, for the vector types, and runs it); never loaded into Python.
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
static inline uint2 make_uint2(uint32_t a, uint32_t b) { return {a, b}; }
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return {a, b, c, d}; }
struct dim3e { unsigned x, y, z; };
static dim3e blockIdx, threadIdx;
static inline uint32_t emu_perm(uint32_t s0, uint32_t s1, uint32_t sel) {
    uint64_t both = ((uint64_t)s0 << 32) | s1;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) { unsigned k = (sel >> (8 * i)) & 0xFF; r |= (uint32_t)((both >> (8 * k)) & 0xFF) << (8 * i); }
    return r;
}
#define __builtin_amdgcn_perm emu_perm
#include "../../wrenc_amd/csrc/dev_format.h"
using namespace wrenc;

template <int F> int run(int w, int h, int dpitch_y, int dpitch_c, unsigned seed) {
    wrenc_gpu_format_layout lay;
    if (wrenc_format_layout(F, w, h, &lay)) return 1;
    srand(seed);
    size_t pitch[3] = {0, 0, 0}, off[3] = {0, 0, 0}, bytes = 0;
    for (int p = 0; p < 3; ++p) { pitch[p] = format_raw_pitch(lay.row_bytes[p]); off[p] = bytes; bytes += pitch[p] * lay.rows[p]; }
    uint8_t* raw = (uint8_t*)malloc(bytes);            // exact: ASan sees any read past pitch x rows
    for (size_t i = 0; i < bytes; ++i) raw[i] = (uint8_t)rand();
    // words at both ends of the range and just above 1023 are common
    for (size_t i = 0; i + 1 < bytes; i += 2) { int r = rand() % 8; if (r == 0) raw[i] = raw[i + 1] = 0xFF; else if (r == 1) raw[i] = raw[i + 1] = 0; else if (r == 2 && F != 3) { raw[i] = 0xFC + rand() % 4; raw[i + 1] = 3; } }
    const int ch = h / 2, cw = w / 2;
    size_t dbytes = (size_t)dpitch_y * h + 2 * (size_t)dpitch_c * ch;
    uint8_t* dst = (uint8_t*)malloc(dbytes);
    memset(dst, 0x5A, dbytes);
    FormatArgs a = {};
    a.raw = raw; a.dst = dst;
    for (int p = 0; p < 3; ++p) { a.raw_off[p] = off[p]; a.raw_pitch[p] = (int)pitch[p]; }
    a.dst_off[1] = (size_t)dpitch_y * h; a.dst_off[2] = a.dst_off[1] + (size_t)dpitch_c * ch;
    a.dst_pitch[0] = dpitch_y; a.dst_pitch[1] = dpitch_c; a.w = w; a.h = h;
    a.row_blocks[0] = (h + kFormatRows - 1) / kFormatRows; a.row_blocks[1] = (ch + kFormatRows - 1) / kFormatRows;
    unsigned gx = (w + 511) / 512, gy = a.row_blocks[0] + (lay.n_planes == 2 ? 1 : 2) * a.row_blocks[1];
    for (unsigned by = 0; by < gy; ++by) for (unsigned bx = 0; bx < gx; ++bx) for (unsigned ty = 0; ty < 4; ++ty) for (unsigned tx = 0; tx < 64; ++tx) {
        blockIdx = {bx, by, 0}; threadIdx = {tx, ty, 0};
        convert_format_kernel<F>(a);
    }
    int bad = 0;
    auto word = [&](int p, size_t row, size_t i) -> int { const uint8_t* q = raw + off[p] + row * pitch[p]; return lay.bytes_per_sample == 2 ? q[2 * i] | (q[2 * i + 1] << 8) : q[i]; };
    for (int p = 0; p < 3; ++p) {
        int pw = p ? cw : w, ph = p ? ch : h, dp = p ? dpitch_c : dpitch_y;
        for (int y = 0; y < ph; ++y) for (int x = 0; x < dp; ++x) {
            int got = dst[a.dst_off[p] + (size_t)y * dp + x], want;
            if (x >= pw) want = 0x5A;
            else if (!p) want = wrenc_format_sample(F, word(0, y, x));
            else if (wrenc_format_interleaved(F)) want = wrenc_format_sample(F, word(1, y, 2 * x + (p - 1)));
            else if (wrenc_format_is422(F)) want = wrenc_format_chroma422(F, word(p, 2 * y, x), word(p, 2 * y + 1, x));
            else want = wrenc_format_sample(F, word(p, y, x));
            if (got != want && bad++ < 5) printf("F%d %dx%d plane %d (%d,%d): got %d want %d\n", F, w, h, p, x, y, got, want);
        }
    }
    free(raw); free(dst);
    return bad;
}
template <int F> int all() {
    int bad = 0;
    bad += run<F>(32, 32, 32, 16, 1); bad += run<F>(34, 30, 64, 32, 2); bad += run<F>(70, 50, 96, 48, 3); bad += run<F>(70, 50, 80, 48, 4);
    bad += run<F>(64, 64, 64, 32, 5); bad += run<F>(1030, 18, 1056, 528, 6); bad += run<F>(16, 16, 32, 16, 7);
    return bad;
}
int main() {
    int bad = all<1>() + all<2>() + all<3>() + all<4>() + all<5>();
    if (bad) return 1;
    printf("format_convert: 5 formats x 7 sizes, clean\n");
    return 0;
}
