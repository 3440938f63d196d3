/* wrenc_rate_quality.h -- the quality controller: every picture gets the largest QP at which its luma PSNR is at or above a
 * target.  Host only; built into libwrenc_host.so (wrenc_amd/csrc/host/rate_quality.cpp).  No clock, no threads, no
 * allocation after wrenc_quality_create but for the batch's state; the same calls give the same answers.
 *
 * Predictor.  A picture's distortion curve (include/wrenc_distcurve.h; wrenc_gpu_download_dist_curve) predicts the luma SSE
 * sse8[0][q] / 4096 at every QP, so PSNR_pred(q) = 10 log10(255^2 W H / sse) over the CODED picture.  The search is not the
 * curve's quantiser (other predictions and block sizes, rate-distortion decisions, a dead zone), so the measured PSNR
 * differs by an offset of about a dB that moves slowly with content and QP: the controller keeps a running correction in
 * dB, WRENC_QUALITY_PRIOR at first (fitted on the CPU against reference searches of smooth and textured pictures at QP 20
 * .. 32: mean -0.9 dB, 0.8 dB rms about it), then an exponential average (weight WRENC_QUALITY_LEARN) of
 * measured - predicted over every reported coding.
 *
 * wrenc_quality_choose: per picture the largest QP in [qp_min, qp_max] with PSNR_pred(q) + correction >= target; qp_min
 * if there is none.  The pictures become the current batch, picture 0 .. n - 1 of wrenc_quality_report.
 *
 * wrenc_quality_report: a coding of a picture of the batch came back with the luma SSE sse_y over samples_y samples
 * (wrenc_gpu_metrics: the visible rectangle).  The answer is *accepted = 1 and in *next_qp the QP of the coding to keep, or
 * *accepted = 0 and the QP to code the picture again at, which was never tried for it.  With best = the largest tried QP
 * whose coding was at or above the target, and the picture's own offset = measured - predicted at the tried QP nearest to
 * the one asked about:
 *   - a best exists and best == qp_max, or best + 1 was tried (and so fell below the target), or
 *     PSNR_pred(best + 1) + offset < target: accepted, keep best.  Never on "close enough above the target": where a QP
 *     is worth 0.2 dB, any window wide enough to stop the search stops it QPs too low.
 *   - otherwise, the recodes used up (codings - 1 == max_recodes): accepted; keep best, or without one the lowest QP tried,
 *     and the picture counts as a MISS.
 *   - a best exists: next is the largest untried QP below the lowest failing QP above best whose PSNR_pred + offset is
 *     at or above the target, at least best + 1.
 *   - no best: with lo = the lowest QP tried, lo == qp_min is accepted as a miss; otherwise next is the largest QP below
 *     lo with PSNR_pred + offset >= target -- the deficit over the picture's own predicted slope, read off its curve, at
 *     least one QP -- or qp_min if there is none.
 * A report after a picture's acceptance, of a picture outside the batch or of a QP outside [qp_min, qp_max] is
 * WRENC_QUALITY_EINVAL.
 */
#ifndef WRENC_RATE_QUALITY_H
#define WRENC_RATE_QUALITY_H

#include "wrenc_distcurve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WRENC_QUALITY_OK 0
#define WRENC_QUALITY_EINVAL (-1)
#define WRENC_QUALITY_PRIOR (-0.9)
#define WRENC_QUALITY_LEARN 0.25
#define WRENC_QUALITY_MAX_RECODES 8

typedef struct wrenc_quality wrenc_quality;

/* NULL for a target that is not finite and positive, qp_min > qp_max, a QP outside 0 .. 63 or max_recodes outside
 * 0 .. WRENC_QUALITY_MAX_RECODES. */
wrenc_quality* wrenc_quality_create(double target_psnr_db, int qp_min, int qp_max, int max_recodes);
void wrenc_quality_destroy(wrenc_quality* q);

/* PSNR_pred(qp) of a curve for a coded picture of width x height, without any correction; +infinity for an SSE of 0. */
double wrenc_quality_predict(const wrenc_dist_curve* curve, int width, int height, int qp);

int wrenc_quality_choose(wrenc_quality* q, int n, const wrenc_dist_curve* curves, int width, int height, int32_t* qp);
int wrenc_quality_report(wrenc_quality* q, int picture, int qp, uint64_t sse_y, uint64_t samples_y, int32_t* next_qp, int* accepted);

/* The running correction in dB; the codings beyond every picture's first, and the misses, since wrenc_quality_create;
 * the codings of a picture of the current batch (0 outside it).  Any pointer may be NULL. */
double wrenc_quality_correction(const wrenc_quality* q);
void wrenc_quality_totals(const wrenc_quality* q, uint64_t* reencoded, uint64_t* misses);
int wrenc_quality_tries(const wrenc_quality* q, int picture);

#ifdef __cplusplus
}
#endif
#endif /* WRENC_RATE_QUALITY_H */
