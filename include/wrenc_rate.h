/* wrenc_rate.h -- rate control of an all-intra run: the QPs of a batch of pictures from their complexities.
 *
 * Host only: no device, no threads, no I/O.  Built into libwrenc_host.so (wrenc_amd/csrc/host/rate_control.cpp).
 * The caller measures every picture before it is searched (wrenc_gpu_download_complexity, include/wrenc_gpu.h), asks
 * wrenc_rate_choose for the batch's QPs, searches the pictures at them (wrenc_gpu_set_slot_qp) and reports the bytes of
 * the pictures' NAL units whenever they become known -- in a pipeline, some batches later.
 *
 * Model.  bytes of a picture ~ a * N * (C / N)^b * 2^(-QP / s), N = width * height, C = the picture's weighted plane sum
 * satd[0] + WRENC_RATE_CHROMA_WEIGHT * (satd[1] + satd[2]).  a, b, s start from a prior fitted on fixed-QP searches
 * (wrenc_rate_prior; DESIGN.md has the fit); b and s stay, a is replaced by (reported bytes) / (what a = 1 predicted for
 * them), the older reports counting half as much with every new one.  Below the mean QP of the reports the slope is not
 * the prior's but a steep one (bytes double every 3 QPs), so a first step towards more bytes is a short one; a report that
 * lies a QP or more below the earlier ones shows the slope between them, which then replaces the steep one, kept between
 * it and the prior's s.
 * Budget of a batch of n pictures: n * target + (target of everything chosen so far - its bytes) * n / window, where the
 * bytes of a picture chosen but not yet reported are the model's with the current a, and the window is the pictures
 * still to come including the batch, at most WRENC_RATE_WINDOW: at the end of the run the whole error is due.  Without
 * wrenc_rate_enable_vbv there is no buffer model: the target is the run's total.
 * QPs.  Pictures are independent, so the batch gets one QP -- or q for its first pictures and q + 1 for the rest, the
 * split whose predicted bytes come closest to the budget.  Complexity predicts bytes; it never makes a picture's QP differ
 * from its neighbours' by more than that.  QPs stay within [qp_min, qp_max]; a target out of reach pins the bound.
 * The same sequence of calls gives the same QPs.
 *
 * The buffer model, declared in wrenc_rate_vbv.h and off until wrenc_rate_enable_vbv; everything above stays as it is
 * without it.  A leaky bucket in bits: B the
 * buffer size, R = 8 * target_bytes the bits that arrive per picture, F_0 = B; picture i must satisfy bits_i <= F_i, and
 * F_(i+1) = min(B, F_i - bits_i + R).  The parameter sets (header_bytes) are charged to picture 0.  Only the cap is
 * modelled: no filler data, and no HRD syntax in the stream.
 * Its predictor is the picture's rate histogram (wrenc_gpu_download_rate_hist; include/wrenc_ratecurve.h), which, unlike
 * the complexity, knows the slope of the picture's own rate curve:
 *     P(q) = sum over planes and bins of weight * count * bits(rep(bin) / (8 * step(q))),  step(q) = 2^((q - 4) / 6),
 * weight 1 for Y and WRENC_RATE_CURVE_CHROMA_WEIGHT for Cb and Cr, rep(bin) the middle of the bin's magnitudes, 8 the gain
 * of the 8x8 Hadamard transform over an orthonormal one, and, with D = WRENC_RATE_CURVE_DEAD,
 *     bits(l) = WRENC_RATE_CURVE_TAIL * l / D inside the dead zone l < D (a coefficient that quantises to zero still costs
 *     its share of the significance flags), else WRENC_RATE_CURVE_BITS0 + WRENC_RATE_CURVE_BITS1 * log2(l / D)
 * -- wrenc_rate_curve.  bytes of a picture ~ a * P(q) + c * CTUs; a starts from a prior, wrenc_rate_curve_prior -- DESIGN.md
 * has the fit --, and follows the reports, an older picture counting WRENC_RATE_VBV_DECAY as much as the next.
 * wrenc_rate_choose_vbv gives every picture a QP of its own: walking the bucket forward from the reported pictures over
 * the predictions of those in flight and of the batch, the lowest QP whose predicted bytes fit both the picture's share
 * of the run's budget (above, an n-th of the batch's) and WRENC_RATE_VBV_SAFETY of what the bucket then allows.
 * Enforcement is the caller's, with wrenc_rate_vbv_allowance and wrenc_rate_recode: in picture order, a picture whose
 * bytes exceed its allowance is coded again at the QP wrenc_rate_recode returns, until it fits or the QP is qp_max, and
 * only then reported -- one picture per wrenc_rate_report call, so that the next allowance is known.
 */
#ifndef WRENC_RATE_H
#define WRENC_RATE_H

#include <stddef.h>
#include <stdint.h>

#include "wrenc_ratecurve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WRENC_RATE_CHROMA_WEIGHT 1.0
#define WRENC_RATE_WINDOW 64

enum wrenc_rate_status { WRENC_RATE_OK = 0, WRENC_RATE_EINVAL = -1 };

typedef struct wrenc_rate wrenc_rate;

typedef struct wrenc_rate_config {
    int32_t width, height;        /* luma samples */
    int32_t qp_min, qp_max;       /* 0 <= qp_min <= qp_max <= 63 */
    int64_t num_pictures;         /* of the run, > 0 */
    double target_bytes;          /* per picture, > 0 (kbit/s * 1000 / 8 / fps) */
    double header_bytes;          /* spent outside the pictures (parameter sets): counted against the total */
} wrenc_rate_config;

/* The prior: bytes ~ a * N * (C / N)^b * 2^(-QP / s).  Any pointer may be NULL. */
void wrenc_rate_prior(double* a, double* b, double* s);

/* WRENC_RATE_EINVAL for a field outside the ranges above. */
int wrenc_rate_create(const wrenc_rate_config* cfg, wrenc_rate** out);
void wrenc_rate_destroy(wrenc_rate* rc);

/* The QPs of the next n pictures (n >= 1) from their plane sums satd[3 * k + p] (wrenc_gpu_complexity::satd of picture
 * k): qp[k] is q for k < some split and q + 1 from it on.  The pictures count as chosen: their bytes are expected by
 * wrenc_rate_report in this order. */
int wrenc_rate_choose(wrenc_rate* rc, int n, const uint64_t* satd, int32_t* qp);

/* The bytes of the n oldest pictures chosen and not yet reported (WRENC_RATE_EINVAL if fewer are outstanding). */
int wrenc_rate_report(wrenc_rate* rc, int n, const uint64_t* bytes);

#ifdef __cplusplus
}
#endif

#include "wrenc_rate_vbv.h" /* the buffer model's entry points */

#endif /* WRENC_RATE_H */
