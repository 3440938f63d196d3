// wrenc_bitstream.cpp -- the C ABI of include/wrenc_bitstream.h, include/wrenc_bitstream_qp.h and include/wrenc_bitstream_window.h.
#include "../../../include/wrenc_bitstream_qp.h"
#include "../../../include/wrenc_bitstream_window.h"
#include "slice_data.h"

#include <cstring>

using namespace wrenc_host;

namespace {

thread_local long long g_last_slice_data_bits = 0;

bool size_ok(int width, int height, int qp) {
    return width >= 32 && height >= 32 && width % 32 == 0 && height % 32 == 0 && width <= 16384 &&
           height <= 16384 && qp >= 0 && qp <= 63;
}

// a visible size the coded size is the round-up of: even, at least 16 x 16 (one SSIM window per chroma plane)
bool window_ok(int width, int height, int vis_w, int vis_h) {
    return vis_w >= 16 && vis_h >= 16 && vis_w % 2 == 0 && vis_h % 2 == 0 && width == (vis_w + 31) / 32 * 32 &&
           height == (vis_h + 31) / 32 * 32;
}

int hand_over(const std::vector<uint8_t>& bytes, uint8_t* out, size_t cap, size_t* len) {
    if (len) *len = bytes.size();
    if (!out || cap < bytes.size()) return WRENC_BS_ENOSPC;
    memcpy(out, bytes.data(), bytes.size());
    return WRENC_BS_OK;
}

// picture header NAL + the slice's NAL (main.rs:307-313, :377-383), from either form of the record
int write_picture(int poc, const Slice& slice, int pps_qp, int slice_qp, uint8_t* out, size_t cap, size_t* len) {
    std::vector<uint8_t> stream;
    {
        BitWriter bw;
        write_picture_header(bw, poc);
        append_nal(stream, 9, NAL_PH, 0, bw.bytes());
    }
    // main.rs:380-382: let bins = slice_encoder.encode(&slice, &sh)
    const SliceHeader sh = {slice_qp, pps_qp};
    SliceEncoder slice_encoder;
    int rc = WRENC_BS_OK;
    const Bins bins = slice_encoder.encode(slice, sh, &rc);
    if (rc) return rc;
    g_last_slice_data_bits = slice_encoder.slice_data_bits();
    append_nal(stream, 9, NAL_IDR_W_RADL, 0, bins.bytes());
    return hand_over(stream, out, cap, len);
}

} // namespace

extern "C" {

size_t wrenc_bs_picture_bound(int width, int height) {
    // A level costs at most 32 escape bins + sign, everything else is far below one bit per sample on
    // top of that; emulation prevention adds at most one byte per two.
    if (width <= 0 || height <= 0) return 0;
    return (size_t)width * (size_t)height * 12 + 4096;
}

int wrenc_bs_write_parameter_sets(int width, int height, int qp, uint8_t* out, size_t cap, size_t* len) {
    return wrenc_bs_write_parameter_sets_window(width, height, width, height, qp, out, cap, len);
}

int wrenc_bs_write_parameter_sets_window(int width, int height, int vis_w, int vis_h, int qp, uint8_t* out, size_t cap,
                                         size_t* len) {
    if (!size_ok(width, height, qp)) return WRENC_BS_EINVAL;
    if ((vis_w != width || vis_h != height) && !window_ok(width, height, vis_w, vis_h)) return WRENC_BS_EINVAL;
    std::vector<uint8_t> stream;
    {
        BitWriter bw;
        write_vps(bw, width, height);
        append_nal(stream, 1, NAL_VPS, 0, bw.bytes()); // main.rs:232
    }
    {
        BitWriter bw;
        write_sps(bw, width, height, vis_w, vis_h);
        append_nal(stream, 9, NAL_SPS, 0, bw.bytes()); // main.rs:245
    }
    {
        BitWriter bw;
        write_pps(bw, width, height, qp);
        append_nal(stream, 9, NAL_PPS, 0, bw.bytes()); // main.rs:257
    }
    return hand_over(stream, out, cap, len);
}

int wrenc_bs_write_picture_qp(int width, int height, int pps_qp, int slice_qp, int poc, const wrenc_bs_record* rec,
                              uint8_t* out, size_t cap, size_t* len) {
    if (!size_ok(width, height, pps_qp) || slice_qp < 0 || slice_qp > 63 || poc < 0 || !rec || !rec->cu_log2_size ||
        !rec->luma_mode || !rec->chroma_mode || !rec->lev_y || !rec->lev_cb || !rec->lev_cr)
        return WRENC_BS_EINVAL;
    return write_picture(poc, Slice{width, height, rec, nullptr}, pps_qp, slice_qp, out, cap, len);
}

int wrenc_bs_write_picture(int width, int height, int qp, int poc, const wrenc_bs_record* rec, uint8_t* out,
                           size_t cap, size_t* len) {
    return wrenc_bs_write_picture_qp(width, height, qp, qp, poc, rec, out, cap, len);
}

int wrenc_bs_write_picture_tokens_qp(int width, int height, int pps_qp, int slice_qp, int poc, const wrenc_bs_tokens* tok,
                                     uint8_t* out, size_t cap, size_t* len) {
    if (!size_ok(width, height, pps_qp) || slice_qp < 0 || slice_qp > 63 || poc < 0 || !tok || !tok->cu_log2_size ||
        !tok->luma_mode || !tok->chroma_mode || !tok->pool || !tok->first_page)
        return WRENC_BS_EINVAL;
    const wrenc_bs_record maps = {tok->cu_log2_size, tok->luma_mode, tok->chroma_mode, nullptr, nullptr, nullptr};
    return write_picture(poc, Slice{width, height, &maps, tok}, pps_qp, slice_qp, out, cap, len);
}

int wrenc_bs_write_picture_tokens(int width, int height, int qp, int poc, const wrenc_bs_tokens* tok, uint8_t* out, size_t cap,
                                  size_t* len) {
    return wrenc_bs_write_picture_tokens_qp(width, height, qp, qp, poc, tok, out, cap, len);
}

long long wrenc_bs_last_slice_data_bits(void) { return g_last_slice_data_bits; }

} // extern "C"
