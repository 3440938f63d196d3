/* wrenc_bitstream_window.h -- pictures of any even size: the parameter sets with a conformance window.
 *
 * The encoder codes whole 32x32 CTUs.  A picture of another size is coded at the next multiple of the CTU size with its
 * last column and row replicated into the margin (include/wrenc_gpu.h, wrenc_gpu_set_visible_size) and the SPS tells the
 * decoder which rectangle to output.  Status codes and conventions are those of wrenc_bitstream.h.  (A header of its
 * own, like wrenc_bitstream_qp.h: tests/test_bitstream.py holds wrenc_bitstream.h to the five entries it has.) */
#ifndef WRENC_BITSTREAM_WINDOW_H
#define WRENC_BITSTREAM_WINDOW_H

#include "wrenc_bitstream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The parameter sets (VPS, SPS, PPS as wrenc_bs_write_parameter_sets writes them) for a picture of vis_w x vis_h coded
 * at coded_w x coded_h with its last column and row replicated into the margin (wrenc_gpu_set_visible_size): vis_w and
 * vis_h even and at least 16, the coded size exactly the round-up of each to a multiple of 32, else WRENC_BS_EINVAL.
 * VPS and PPS are those of wrenc_bs_write_parameter_sets(coded_w, coded_h, qp); the SPS has
 * sps_conformance_window_flag = 1 and the offsets left 0, right (coded_w - vis_w) / 2, top 0, bottom
 * (coded_h - vis_h) / 2 (chroma sample units, H.266 7.4.3.4), so a decoder outputs vis_w x vis_h.  The PPS keeps
 * pps_conformance_window_flag = 0: its picture size is the SPS's maximum size and the window is inferred (7.4.3.5).
 * Picture headers, slices and slice data are those of the coded size.  With the visible size equal to the coded size:
 * the bytes of wrenc_bs_write_parameter_sets. */
int wrenc_bs_write_parameter_sets_window(int coded_w, int coded_h, int vis_w, int vis_h, int qp, uint8_t* out, size_t cap,
                                         size_t* len);

#ifdef __cplusplus
}
#endif
#endif /* WRENC_BITSTREAM_WINDOW_H */
