/* wrenc_rate_vbv.h -- the buffer model of the rate controller: its entry points (the model itself is described in
 * wrenc_rate.h, which includes this header).  Host only; built into libwrenc_host.so (wrenc_amd/csrc/host/rate_control.cpp). */
#ifndef WRENC_RATE_VBV_H
#define WRENC_RATE_VBV_H

#include "wrenc_rate.h"
#include "wrenc_ratecurve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WRENC_RATE_CURVE_DEAD 0.7
#define WRENC_RATE_CURVE_TAIL 0.125
#define WRENC_RATE_CURVE_BITS0 2.3
#define WRENC_RATE_CURVE_BITS1 0.87
#define WRENC_RATE_CURVE_CHROMA_WEIGHT 0.5
#define WRENC_RATE_VBV_SAFETY 0.85
#define WRENC_RATE_VBV_DECAY 0.9

/* P(q) of a histogram for q = 0 .. 63, in the model's bits (a = 1); non-increasing in q.  WRENC_RATE_EINVAL for a null
 * pointer. */
int wrenc_rate_curve(const wrenc_rate_hist* hist, double p[64]);
/* The prior of bytes ~ a * P(q) + c * CTUs (CTUs = ceil(width / 32) * ceil(height / 32)).  Any pointer may be NULL. */
void wrenc_rate_curve_prior(double* a, double* c);

/* Turns the buffer model on: bufsize_bits = B.  WRENC_RATE_EINVAL for a B that is not finite, smaller than one picture's
 * R = 8 * target_bytes or not larger than the parameter sets' 8 * header_bytes, and once a picture has been chosen. */
int wrenc_rate_enable_vbv(wrenc_rate* rc, double bufsize_bits);

/* The QPs of the next n pictures from their rate histograms, one QP per picture; allowance_bits (may be NULL) receives
 * what the walk expects the bucket to allow each.  The pictures count as chosen.  WRENC_RATE_EINVAL without
 * wrenc_rate_enable_vbv -- and wrenc_rate_choose returns it with. */
int wrenc_rate_choose_vbv(wrenc_rate* rc, int n, const wrenc_rate_hist* hist, int32_t* qp, double* allowance_bits);

/* The bits the oldest picture chosen and not yet reported may have: the bucket's fullness after every reported picture,
 * less the parameter sets for picture 0.  *bufsize_bits and *fullness_bits (may be NULL) receive B and that fullness. */
int wrenc_rate_vbv_allowance(const wrenc_rate* rc, double* allowance_bits, double* bufsize_bits, double* fullness_bits);

/* The oldest outstanding picture came back with actual_bytes at its QP and must fit allowance_bits: the QP to code it
 * again at -- the lowest one above its QP at which its own curve, scaled by actual / predicted, fits WRENC_RATE_VBV_SAFETY
 * of the allowance; qp_max if none does.  The picture's QP becomes *qp.  At qp_max already, *qp is qp_max again: the
 * caller keeps the picture as it is. */
int wrenc_rate_recode(wrenc_rate* rc, uint64_t actual_bytes, double allowance_bits, int32_t* qp);

#ifdef __cplusplus
}
#endif
#endif /* WRENC_RATE_VBV_H */
