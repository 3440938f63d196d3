// rate_quality.cpp -- the quality controller of include/wrenc_rate_quality.h (the rules are described there).
#include "../../../include/wrenc_rate_quality.h"

#include <cmath>
#include <new>
#include <vector>

namespace {

enum : uint8_t { kUntried = 0, kPassed = 1, kFailed = 2 };

struct Picture {
    double pred[64];   // PSNR_pred(q)
    double meas[64];   // of the tried QPs
    uint8_t tried[64];
    int tries = 0;
    bool done = false;
};

double psnr_db(double sse, double samples) { return sse <= 0.0 ? (double)INFINITY : 10.0 * std::log10(255.0 * 255.0 * samples / sse); }

} // namespace

struct wrenc_quality {
    double target, correction;
    int qp_min, qp_max, max_recodes;
    uint64_t reencoded, misses;
    std::vector<Picture> batch;
};

// PSNR_pred(x) + the picture's offset at the tried QP nearest to x (the lower one of two)
static double with_offset(const Picture& p, int x) {
    if (std::isinf(p.pred[x])) return p.pred[x];
    int near = -1;
    for (int d = 0; d < 64 && near < 0; ++d) {
        if (x - d >= 0 && p.tried[x - d]) near = x - d;
        else if (x + d < 64 && p.tried[x + d]) near = x + d;
    }
    const double offset = near < 0 || std::isinf(p.pred[near]) ? 0.0 : p.meas[near] - p.pred[near];
    return p.pred[x] + offset;
}

extern "C" {

wrenc_quality* wrenc_quality_create(double target_psnr_db, int qp_min, int qp_max, int max_recodes) {
    if (!std::isfinite(target_psnr_db) || target_psnr_db <= 0.0 || qp_min < 0 || qp_max > 63 || qp_min > qp_max || max_recodes < 0 ||
        max_recodes > WRENC_QUALITY_MAX_RECODES)
        return nullptr;
    wrenc_quality* q = new (std::nothrow) wrenc_quality();
    if (!q) return nullptr;
    q->target = target_psnr_db;
    q->correction = WRENC_QUALITY_PRIOR;
    q->qp_min = qp_min;
    q->qp_max = qp_max;
    q->max_recodes = max_recodes;
    q->reencoded = q->misses = 0;
    return q;
}

void wrenc_quality_destroy(wrenc_quality* q) { delete q; }

double wrenc_quality_predict(const wrenc_dist_curve* curve, int width, int height, int qp) {
    if (!curve || width <= 0 || height <= 0 || qp < 0 || qp > 63) return (double)NAN;
    return psnr_db((double)curve->sse8[0][qp] / 4096.0, (double)width * (double)height);
}

int wrenc_quality_choose(wrenc_quality* q, int n, const wrenc_dist_curve* curves, int width, int height, int32_t* qp) {
    if (!q || n < 0 || width <= 0 || height <= 0 || (n > 0 && (!curves || !qp))) return WRENC_QUALITY_EINVAL;
    q->batch.assign((size_t)n, Picture());
    for (int k = 0; k < n; ++k) {
        Picture& p = q->batch[(size_t)k];
        for (int x = 0; x < 64; ++x) {
            p.pred[x] = wrenc_quality_predict(&curves[k], width, height, x);
            p.meas[x] = 0.0;
            p.tried[x] = kUntried;
        }
        int pick = q->qp_min;
        for (int x = q->qp_max; x >= q->qp_min; --x)
            if (p.pred[x] + q->correction >= q->target) {
                pick = x;
                break;
            }
        qp[k] = pick;
    }
    return WRENC_QUALITY_OK;
}

int wrenc_quality_report(wrenc_quality* q, int picture, int qp, uint64_t sse_y, uint64_t samples_y, int32_t* next_qp, int* accepted) {
    if (!q || !next_qp || !accepted || picture < 0 || (size_t)picture >= q->batch.size() || qp < q->qp_min || qp > q->qp_max || samples_y == 0)
        return WRENC_QUALITY_EINVAL;
    Picture& p = q->batch[(size_t)picture];
    if (p.done || p.tried[qp]) return WRENC_QUALITY_EINVAL;
    const double psnr = psnr_db((double)sse_y, (double)samples_y);
    p.meas[qp] = psnr;
    p.tried[qp] = psnr >= q->target ? kPassed : kFailed;
    if (++p.tries > 1) ++q->reencoded;
    if (std::isfinite(psnr) && std::isfinite(p.pred[qp])) q->correction += WRENC_QUALITY_LEARN * (psnr - p.pred[qp] - q->correction);

    int best = -1, lo = 64;
    for (int x = 0; x < 64; ++x) {
        if (p.tried[x] == kPassed) best = x;
        if (p.tried[x] && x < lo) lo = x;
    }
    int keep = -1;
    if (best >= 0) {
        if (best == q->qp_max || p.tried[best + 1] == kFailed || with_offset(p, best + 1) < q->target) keep = best;
    } else if (lo == q->qp_min) {
        keep = lo;
    }
    if (keep < 0 && p.tries - 1 >= q->max_recodes) keep = best >= 0 ? best : lo;
    if (keep >= 0) {
        if (best < 0) ++q->misses;
        p.done = true;
        *next_qp = keep;
        *accepted = 1;
        return WRENC_QUALITY_OK;
    }
    int next;
    if (best >= 0) {
        int hi = q->qp_max + 1; // the lowest failing QP above best
        for (int x = q->qp_max; x > best; --x)
            if (p.tried[x] == kFailed) hi = x;
        next = best + 1;
        for (int x = hi - 1; x > best + 1; --x)
            if (!p.tried[x] && with_offset(p, x) >= q->target) {
                next = x;
                break;
            }
    } else {
        next = q->qp_min;
        for (int x = lo - 1; x > q->qp_min; --x)
            if (with_offset(p, x) >= q->target) {
                next = x;
                break;
            }
    }
    *next_qp = next;
    *accepted = 0;
    return WRENC_QUALITY_OK;
}

double wrenc_quality_correction(const wrenc_quality* q) { return q ? q->correction : (double)NAN; }

void wrenc_quality_totals(const wrenc_quality* q, uint64_t* reencoded, uint64_t* misses) {
    if (reencoded) *reencoded = q ? q->reencoded : 0;
    if (misses) *misses = q ? q->misses : 0;
}

int wrenc_quality_tries(const wrenc_quality* q, int picture) {
    return q && picture >= 0 && (size_t)picture < q->batch.size() ? q->batch[(size_t)picture].tries : 0;
}

} // extern "C"
