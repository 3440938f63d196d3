// dev_pad.h -- edge padding of a picture that is smaller than its coded size (include/wrenc_gpu.h:
// wrenc_gpu_set_visible_size).  The upload copies the visible vw x vh rectangle of each plane into the slot's planes of
// the coded size (whole CTUs); this kernel fills what is left, org(x, y) = org(min(x, vw - 1), min(y, vh - 1)), so that
// the margin never crosses the bus and the search sees an ordinary picture of the coded size.
//
// Per plane the margin is two pieces, and each item of work is one store:
//   right strip   rows 0 .. vh - 1, from the dword that holds column vw to the end of the row (at most 8 dwords): an item
//                 is one dword of one row, consecutive lanes along the row and then down the rows; its value is the row's
//                 last visible sample in every byte.  Where vw is no multiple of 4 the strip's first dword also holds
//                 visible samples: its margin bytes are stored one by one, so the kernel never writes a visible sample.
//   bottom strip  rows vh .. ph - 1 over the whole coded width: an item is 16 bytes of one row (rows and planes are 16-byte
//                 aligned: the pitch is a multiple of 16), consecutive lanes along the row; its value is the same 16 bytes of
//                 row vh - 1 with the bytes from column vw on replaced by that row's last visible sample.
// Every margin sample is computed from visible samples only, and the kernel loads visible samples only (a 16-byte piece of
// row vh - 1 that reaches into that row's own margin is put together from its visible dwords and bytes), so no item reads
// what another one writes and nothing depends on the order in which items run.  One launch covers the three planes; its
// size is the margin's, not the picture's (1920x1080 in 1920x1088: 1440 items).
#pragma once

namespace wrenc {

// how the margin of a plane (chroma = 0 luma, 1 Cb / Cr) is dealt to items
struct PadPlane {
    int pw, ph, vw, vh; // coded and visible size in samples
    int x_first;        // right strip: column of its first dword
    int row_dwords;     // ... dwords per row (0: no margin at the right)
    int right_items;
    int chunks;         // bottom strip: 16-byte pieces per row
    int bottom_items;
    int items;
};
__host__ __device__ inline PadPlane pad_plane(int W, int H, int VW, int VH, int chroma) {
    PadPlane p;
    p.pw = W >> chroma;
    p.ph = H >> chroma;
    p.vw = VW >> chroma;
    p.vh = VH >> chroma;
    p.x_first = p.vw & ~3;
    p.row_dwords = p.vw < p.pw ? (p.pw - p.x_first) >> 2 : 0;
    p.right_items = p.row_dwords * p.vh;
    p.chunks = p.pw >> 4;
    p.bottom_items = p.chunks * (p.ph - p.vh);
    p.items = p.right_items + p.bottom_items;
    return p;
}
__host__ __device__ inline int pad_items(int W, int H, int VW, int VH) {
    return pad_plane(W, H, VW, VH, 0).items + 2 * pad_plane(W, H, VW, VH, 1).items;
}

// the dword of row `src` from column x on (a multiple of 4) with the bytes at columns >= vw replaced by `edge`; only the
// visible bytes are loaded
__device__ __forceinline__ uint32_t pad_dword(const uint8_t* src, int x, int vw, uint32_t edge) {
    if (x + 4 <= vw) return *(const uint32_t*)(src + x);
    uint32_t v = edge * 0x01010101u;
    for (int k = 0; k < vw - x; ++k) v = (v & ~(0xFFu << (8 * k))) | ((uint32_t)src[x + k] << (8 * k));
    return v;
}

// org: a slot's originals, Y | Cb | Cr back to back at the coded size (PicBufs::org[0])
__global__ __launch_bounds__(256) void pad_edges_kernel(uint8_t* org, int W, int H, int VW, int VH) {
    int id = (int)(blockIdx.x * 256 + threadIdx.x);
    const size_t wh = (size_t)W * H;
    for (int plane = 0; plane < 3; ++plane) {
        const PadPlane P = pad_plane(W, H, VW, VH, plane ? 1 : 0);
        if (id >= P.items) {
            id -= P.items;
            continue;
        }
        uint8_t* base = org + (plane ? wh + (size_t)(plane - 1) * (wh >> 2) : 0);
        if (id < P.right_items) {
            const int y = id / P.row_dwords, x = P.x_first + 4 * (id - y * P.row_dwords);
            uint8_t* row = base + (size_t)y * P.pw;
            const uint8_t edge = row[P.vw - 1];
            if (x >= P.vw) {
                *(uint32_t*)(row + x) = edge * 0x01010101u;
            } else {
                for (int k = P.vw - x; k < 4; ++k) row[x + k] = edge; // the dword that column vw - 1 lies in
            }
        } else {
            id -= P.right_items;
            const int r = id / P.chunks, x = 16 * (id - r * P.chunks);
            const uint8_t* src = base + (size_t)(P.vh - 1) * P.pw;
            const uint32_t edge = src[P.vw - 1];
            uint4 v;
            if (x + 16 <= P.vw) {
                v = *(const uint4*)(src + x);
            } else {
                v.x = pad_dword(src, x, P.vw, edge);
                v.y = pad_dword(src, x + 4, P.vw, edge);
                v.z = pad_dword(src, x + 8, P.vw, edge);
                v.w = pad_dword(src, x + 12, P.vw, edge);
            }
            *(uint4*)(base + (size_t)(P.vh + r) * P.pw + x) = v;
        }
        return;
    }
}

} // namespace wrenc
