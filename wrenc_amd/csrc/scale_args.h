// scale_args.h -- the arguments of the scaler's kernel (dev_scale.h) as plain data: a context keeps them between uploads
// (gpu_ctx.h), so every unit that knows the context knows them, with or without the kernel.
#pragma once
#include <stdint.h>

namespace wrenc {

// one axis of one plane size (luma or chroma)
struct ScaleAxis {
    const int* first;       // [n_out]: input index of the first tap (may be negative)
    const int16_t* coef;    // [n_out][kScaleCoefs]: zero behind the sample's own taps
    const int* tile_base;   // [tiles]: the smallest `first` of the tile's samples; x: rounded down to a multiple of 4
    int n_in, n_out;
    int taps;               // coefficients the passes run over: the longest list of the axis, rounded up to even
    int span;               // input samples from tile_base that a tile's taps reach at most (<= kScaleSpanX / kScaleSpanY)
};

struct ScaleArgs {
    ScaleAxis x[2], y[2];   // [0] luma, [1] chroma
    const uint8_t* src[3];  // staging planes
    int src_pitch[2];       // ... and their pitch, luma and chroma: multiples of 16
    uint8_t* dst;           // a slot's originals, Y | Cb | Cr back to back at the coded size (PicBufs::org[0])
    int W, H;               // the coded size
    int tiles_x[2], tiles[2]; // tiles per row and per plane, luma and chroma
};

} // namespace wrenc
