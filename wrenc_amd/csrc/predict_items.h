// predict_items.h -- the items of wrenc_gpu_test_predict (include/wrenc_gpu_test.h): what an item may be and how many
// bytes it puts out.  The one place that knows: the entry refuses a call through it before anything reaches the kernel,
// wrenc_gpu_test_predict_layout hands the offsets to callers, and test_predict_kernel names its kinds from here.
// Plain C++, no HIP: tools/sanitize/predict_items.cpp runs it on the host alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace wrenc {

// item = {x, y (luma samples, picture), log2 luma size, kind, mode word}
constexpr int kPredictItemInts = 5;
enum PredictKind : int {
    PK_LUMA = 0,       // predict_full of the luma block to scratch: n x n bytes
    PK_CHROMA = 1,     // ... of the Cb + Cr pair: 2 x (n/2)^2 bytes
    PK_LUMA4 = 2,      // the 4x4 luma block through predict4_lane: 16 bytes
    PK_SAD_LUMA = 4,   // SAD lists (sad_list_angular) over luma / the chroma pair / both: 16 u32
    PK_SAD_CHROMA = 5, //   mode word = first mode | entries << 8 | stride << 16
    PK_SAD_BOTH = 6,
    PK_SAD_CCLM = 7,   // the CCLM SAD list of the chroma pair (mode word 0): 16 u32
    PK_FULL_LUMA = 8,  // a full candidate into the recon tile: prediction bytes, then as many i16 residuals
    PK_FULL_CHROMA = 9,
    PK_PACK8 = 10,     // the luma blocks of an 8x8 pack, mode word = m0 | m1 << 8 | m2 << 16 | candidates << 24
    PK_PACK16 = 11,    // a 16x16 pack, luma and chroma pair, mode word = m0 | m1 << 8 | candidates << 24
};
// (dev_common.h, dev_predict.h: wrenc_gpu_test.hip asserts that these are LT_CCLM, T_CCLM and kNoMode)
constexpr int kItemModeMax = 66, kItemCclmFirst = 81, kItemCclmLast = 83, kItemNoMode = 255;

// the bytes an item of a W x H picture puts out, or 0 for an item that must not reach the kernel
inline size_t predict_item_bytes(int W, int H, const int32_t* q) {
    const int x = q[0], y = q[1], lg = q[2], kind = q[3], mode = q[4];
    if (lg < 2 || lg > 5) return 0;
    const int n = 1 << lg;
    if (x < 0 || y < 0 || x > W - n || y > H - n || (x & (n - 1)) || (y & (n - 1)) || mode < 0) return 0;
    const size_t nn = (size_t)n * n;
    const bool angular = mode <= kItemModeMax, cclm = mode >= kItemCclmFirst && mode <= kItemCclmLast;
    switch (kind) {
    case PK_LUMA: return angular ? nn : 0;
    case PK_CHROMA: return lg >= 3 && (angular || cclm) ? nn / 2 : 0;
    case PK_LUMA4: return lg == 2 && angular ? nn : 0;
    case PK_SAD_LUMA:
    case PK_SAD_CHROMA:
    case PK_SAD_BOTH: {
        const int m0 = mode & 255, entries = (mode >> 8) & 255, stride = mode >> 16;
        if (kind != PK_SAD_LUMA && lg < 3) return 0;
        return m0 >= 2 && m0 <= kItemModeMax && entries >= 1 && entries <= 16 && stride >= 1 && stride <= 64 ? 64 : 0;
    }
    case PK_SAD_CCLM: return lg >= 3 && mode == 0 ? 64 : 0;
    case PK_FULL_LUMA: return angular ? 3 * nn : 0;
    case PK_FULL_CHROMA: return lg >= 3 && (angular || cclm) ? 3 * nn / 2 : 0;
    case PK_PACK8:
    case PK_PACK16: {
        const int nc = mode >> 24, nc_max = kind == PK_PACK8 ? 3 : 2;
        if (lg != (kind == PK_PACK8 ? 3 : 4) || nc < 1 || nc > nc_max) return 0;
        for (int j = 0; j < nc; ++j) {
            const int m = (mode >> (8 * j)) & 255;
            if (m > kItemModeMax && m != kItemNoMode) return 0;
        }
        return 3 * (size_t)(kind == PK_PACK8 ? 64 : 384) * nc;
    }
    default: return 0;
    }
}

// offsets[i]: where item i's output starts, offsets[n_items]: the bytes of all of them (offsets: n_items + 1 values).
// Returns the index of the first item that is refused -- the kernel keeps 32-bit offsets, so an item that ends beyond
// 2^31 - 1 bytes is -- or -1 where every item is fine.
inline int predict_items_layout(int W, int H, int n_items, const int32_t* items, size_t* offsets) {
    size_t total = 0;
    for (int i = 0; i < n_items; ++i) {
        const size_t bytes = predict_item_bytes(W, H, items + (size_t)kPredictItemInts * i);
        offsets[i] = total;
        total += bytes;
        if (!bytes || total > (size_t)INT32_MAX) return i;
    }
    offsets[n_items] = total;
    return -1;
}

} // namespace wrenc
