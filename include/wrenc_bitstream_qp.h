/* wrenc_bitstream_qp.h -- per-picture QP entries of the host bitstream writer (include/wrenc_bitstream.h).
 *
 * A sequence's parameter sets carry one QP (wrenc_bs_write_parameter_sets: init_qp = max(qp, 26)); each slice header
 * carries its picture's offset from it.  These two writers are wrenc_bs_write_picture and wrenc_bs_write_picture_tokens
 * for a picture searched at `slice_qp` (wrenc_gpu_set_slot_qp, include/wrenc_gpu.h) in a sequence whose parameter sets
 * were written with `pps_qp`: the slice header carries slice_qp - max(pps_qp, 26), and the arithmetic coder initialises
 * its contexts at slice_qp.  WRENC_BS_EINVAL for a slice_qp outside 0..63.  With pps_qp == slice_qp the bytes are those
 * the entries of wrenc_bitstream.h write for qp = pps_qp.  Built into the same library.
 */
#ifndef WRENC_BITSTREAM_QP_H
#define WRENC_BITSTREAM_QP_H

#include "wrenc_bitstream.h"

#ifdef __cplusplus
extern "C" {
#endif

int wrenc_bs_write_picture_qp(int width, int height, int pps_qp, int slice_qp, int poc, const wrenc_bs_record* rec,
                              uint8_t* out, size_t cap, size_t* len);
int wrenc_bs_write_picture_tokens_qp(int width, int height, int pps_qp, int slice_qp, int poc, const wrenc_bs_tokens* tok,
                                     uint8_t* out, size_t cap, size_t* len);

#ifdef __cplusplus
}
#endif
#endif /* WRENC_BITSTREAM_QP_H */
