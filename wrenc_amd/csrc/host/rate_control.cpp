// rate_control.cpp -- include/wrenc_rate.h: the QPs of a batch from its pictures' complexities, a bytes-at-QP model
// whose scale follows the bytes reported so far; and the buffer model: a leaky bucket, a curve per picture from its rate
// histogram, a QP per picture, the QP to code a picture again at.  Plain doubles and libm, one thread, no state outside the object: the
// same calls give the same QPs.
#include <cmath>
#include <deque>
#include <new>
#include <vector>

#include "../../../include/wrenc_rate.h"

namespace {

// The prior: least squares over fixed-QP searches of the synthetic content at QP 17..47 (tools/rc_probe.py fit; the
// figures and the residuals are in DESIGN.md section 13).
constexpr double kPriorA = 0.01583;
constexpr double kPriorB = 1.017;
constexpr double kPriorS = 6.872;
// Below the QPs that reports cover the bytes are taken to double every kSteepS QPs, until reports at two QPs show the
// slope: the steepest content of the fit (smooth pictures below QP 26) doubles that fast, and spending four times a
// batch's budget costs three batches where spending a quarter of it costs three quarters of one.
constexpr double kSteepS = 3.0;

// The buffer model's prior, bytes ~ a P(q) + c CTUs: the same searches through the pictures' rate histograms
// (tools/rc_probe.py curve).
constexpr double kCurveA = 0.1370;
constexpr double kCurveC = 4.8;

// the middle of a bin's magnitudes (bins that hold nothing -- 2, 3, 4, 6, 8 -- never count)
double bin_rep(int bin) {
    if (bin <= 0) return 0.0;
    const int lo = wrenc_ratecurve_bin_floor(bin);
    int next = bin + 1;
    while (next <= WRENC_RATECURVE_TOP_BIN && wrenc_ratecurve_bin_floor(next) <= lo) ++next;
    const int hi = next <= WRENC_RATECURVE_TOP_BIN ? wrenc_ratecurve_bin_floor(next) : WRENC_RATECURVE_MAX_MAGNITUDE + 1;
    return 0.5 * (double)(lo + hi - 1);
}

double level_bits(double l) {
    if (l < WRENC_RATE_CURVE_DEAD) return WRENC_RATE_CURVE_TAIL * l / WRENC_RATE_CURVE_DEAD;
    return WRENC_RATE_CURVE_BITS0 + WRENC_RATE_CURVE_BITS1 * std::log2(l / WRENC_RATE_CURVE_DEAD);
}

} // namespace

struct wrenc_rate {
    wrenc_rate_config cfg;
    double samples;             // N
    struct picture {
        double base; // what a = 1 predicts for it at QP 0
        int qp;
        std::vector<double> curve; // the buffer model: P(q) of the picture, q = 0 .. 63
    };
    std::deque<picture> pending; // chosen, not yet reported
    long long chosen = 0;       // pictures chosen so far
    double reported_bytes = 0;  // ... and the bytes of those reported
    // reports, halved with every new one: a = fit_bytes / fit_unit (unit: a = 1 at the picture's QP), their mean QP
    // fit_qp / fit_n, and fit_base for the slope between them and the next report
    double fit_bytes = 0, fit_unit = 0, fit_base = 0, fit_qp = 0, fit_n = 0;
    double s_down = kSteepS;    // the slope below the reported QPs
    // the buffer model: off while bufsize is 0; the bucket after every reported picture; the reports behind a
    bool vbv = false;
    double bufsize = 0, fullness = 0;
    long long reported = 0;
    double curve_bytes = 0, curve_unit = 0;
    double ctus = 0;

    double curve_a() const { return curve_unit > 0 && curve_bytes > 0 ? curve_bytes / curve_unit : kCurveA; }
    double predict(const picture& p, int q) const { return curve_a() * p.curve[(size_t)q] + kCurveC * ctus; }
    double arrive() const { return 8.0 * cfg.target_bytes; } // R
    // the bucket after a picture of `bytes`, the `index`-th of the run (picture 0 carries the parameter sets)
    double drain(double f, double bytes, long long index) const {
        const double bits = 8.0 * (bytes + (index == 0 ? cfg.header_bytes : 0.0));
        return std::fmin(bufsize, f - bits + arrive());
    }

    // the model's 2^(-QP / s): the prior's slope, and s_down below the mean QP of the reports
    double scale(double q) const {
        double e = -q / kPriorS;
        if (fit_n > 0 && q < fit_qp / fit_n) e += (fit_qp / fit_n - q) * (1.0 / s_down - 1.0 / kPriorS);
        return std::exp2(e);
    }
};

void wrenc_rate_prior(double* a, double* b, double* s) {
    if (a) *a = kPriorA;
    if (b) *b = kPriorB;
    if (s) *s = kPriorS;
}

int wrenc_rate_create(const wrenc_rate_config* cfg, wrenc_rate** out) {
    if (!cfg || !out) return WRENC_RATE_EINVAL;
    if (cfg->width < 1 || cfg->height < 1 || cfg->qp_min < 0 || cfg->qp_max > 63 || cfg->qp_min > cfg->qp_max || cfg->num_pictures < 1 ||
        !(cfg->target_bytes > 0) || !std::isfinite(cfg->target_bytes) || !(cfg->header_bytes >= 0) || !std::isfinite(cfg->header_bytes))
        return WRENC_RATE_EINVAL;
    wrenc_rate* rc = new (std::nothrow) wrenc_rate;
    if (!rc) return WRENC_RATE_EINVAL;
    rc->cfg = *cfg;
    rc->samples = (double)cfg->width * cfg->height;
    rc->ctus = (double)((cfg->width + 31) / 32) * (double)((cfg->height + 31) / 32);
    *out = rc;
    return WRENC_RATE_OK;
}

void wrenc_rate_destroy(wrenc_rate* rc) { delete rc; }

int wrenc_rate_choose(wrenc_rate* rc, int n, const uint64_t* satd, int32_t* qp) {
    if (!rc || n < 1 || !satd || !qp || rc->vbv) return WRENC_RATE_EINVAL;
    const wrenc_rate_config& c = rc->cfg;
    // what a = 1 predicts for every picture at QP 0 (a flat picture still costs its CU syntax: one activity unit per block)
    std::vector<double> base((size_t)n);
    for (int k = 0; k < n; ++k) {
        const double cplx = (double)satd[3 * k] + WRENC_RATE_CHROMA_WEIGHT * ((double)satd[3 * k + 1] + (double)satd[3 * k + 2]);
        base[(size_t)k] = rc->samples * std::pow(std::fmax(cplx, rc->samples / 64.0) / rc->samples, kPriorB);
    }
    const double a = rc->fit_unit > 0 ? rc->fit_bytes / rc->fit_unit : kPriorA;
    // the budget: the batch's own target plus its share of the error so far
    double in_flight = 0;
    for (const wrenc_rate::picture& p : rc->pending) in_flight += p.base * rc->scale(p.qp);
    const double spent = c.header_bytes + rc->reported_bytes + a * in_flight;
    const double error = c.target_bytes * (double)rc->chosen - spent;
    long long window = c.num_pictures - rc->chosen;
    if (window > WRENC_RATE_WINDOW) window = WRENC_RATE_WINDOW;
    if (window < n) window = n;
    const double budget = c.target_bytes * n + error * (double)n / (double)window;
    const auto scale = [rc](int q) { return rc->scale(q); };
    double total = 0;
    for (double b : base) total += b;
    // q: the highest QP at which the whole batch still reaches the budget (qp_min if none does)
    int q = c.qp_min;
    while (q < c.qp_max && a * total * scale(q + 1) >= budget) ++q;
    int split = n; // pictures split .. n - 1 get q + 1
    if (q < c.qp_max && a * total * scale(q) > budget) {
        double best = std::fabs(a * total * scale(q) - budget), tail = 0;
        for (int m = n - 1; m >= 0; --m) {
            tail += base[(size_t)m];
            const double pred = a * ((total - tail) * scale(q) + tail * scale(q + 1));
            if (std::fabs(pred - budget) < best) {
                best = std::fabs(pred - budget);
                split = m;
            }
        }
    }
    for (int k = 0; k < n; ++k) {
        qp[k] = k < split ? q : q + 1;
        rc->pending.push_back({base[(size_t)k], qp[k], {}});
    }
    rc->chosen += n;
    return WRENC_RATE_OK;
}

int wrenc_rate_report(wrenc_rate* rc, int n, const uint64_t* bytes) {
    if (!rc || n < 1 || !bytes || (size_t)n > rc->pending.size()) return WRENC_RATE_EINVAL;
    if (rc->vbv) {
        for (int k = 0; k < n; ++k) {
            const wrenc_rate::picture p = rc->pending.front();
            rc->pending.pop_front();
            // a from the bytes beyond the constant; a picture smaller than the constant says nothing about a
            rc->curve_bytes = WRENC_RATE_VBV_DECAY * rc->curve_bytes + std::fmax((double)bytes[k] - kCurveC * rc->ctus, 0.0);
            rc->curve_unit = WRENC_RATE_VBV_DECAY * rc->curve_unit + p.curve[(size_t)p.qp];
            rc->fullness = rc->drain(rc->fullness, (double)bytes[k], rc->reported);
            rc->reported_bytes += (double)bytes[k];
            ++rc->reported;
        }
        return WRENC_RATE_OK;
    }
    double got = 0, base = 0, qp = 0;
    for (int k = 0; k < n; ++k) {
        got += (double)bytes[k];
        base += rc->pending[(size_t)k].base;
        qp += rc->pending[(size_t)k].qp;
    }
    // The slope between the earlier reports and this one, if it lies at least a QP below them: it replaces s_down,
    // kept between the steep slope and the prior's (a change of content between the two reads as a slope as well; the
    // bounds are what limits the harm).
    if (rc->fit_n > 0 && rc->fit_qp / rc->fit_n - qp / n >= 1.0) {
        const double rise = std::log2((got / base) / (rc->fit_bytes / rc->fit_base));
        const double seen = rise > 0 ? (rc->fit_qp / rc->fit_n - qp / n) / rise : kPriorS;
        rc->s_down = std::fmin(kPriorS, std::fmax(kSteepS, seen));
    }
    rc->fit_bytes *= 0.5;
    rc->fit_unit *= 0.5;
    rc->fit_base *= 0.5;
    rc->fit_qp *= 0.5;
    rc->fit_n *= 0.5;
    for (int k = 0; k < n; ++k) {
        const wrenc_rate::picture p = rc->pending.front();
        rc->pending.pop_front();
        rc->fit_bytes += (double)bytes[k];
        rc->fit_unit += p.base * std::exp2(-(double)p.qp / kPriorS);
        rc->fit_base += p.base;
        rc->fit_qp += p.qp;
        rc->fit_n += 1;
        rc->reported_bytes += (double)bytes[k];
    }
    return WRENC_RATE_OK;
}

int wrenc_rate_curve(const wrenc_rate_hist* hist, double p[64]) {
    if (!hist || !p) return WRENC_RATE_EINVAL;
    double rep[WRENC_RATECURVE_BINS] = {};
    for (int b = 1; b <= WRENC_RATECURVE_TOP_BIN; ++b) rep[b] = bin_rep(b);
    for (int q = 0; q < 64; ++q) {
        const double scale = 1.0 / (8.0 * std::exp2((q - 4) / 6.0));
        double sum = 0;
        for (int b = 1; b <= WRENC_RATECURVE_TOP_BIN; ++b) {
            const double n = (double)hist->count[0][b] + WRENC_RATE_CURVE_CHROMA_WEIGHT * ((double)hist->count[1][b] + (double)hist->count[2][b]);
            if (n > 0) sum += n * level_bits(rep[b] * scale);
        }
        p[q] = sum;
    }
    return WRENC_RATE_OK;
}

void wrenc_rate_curve_prior(double* a, double* c) {
    if (a) *a = kCurveA;
    if (c) *c = kCurveC;
}

int wrenc_rate_enable_vbv(wrenc_rate* rc, double bufsize_bits) {
    if (!rc || rc->chosen > 0 || !std::isfinite(bufsize_bits) || bufsize_bits < rc->arrive() || !(bufsize_bits > 8.0 * rc->cfg.header_bytes))
        return WRENC_RATE_EINVAL;
    rc->vbv = true;
    rc->bufsize = rc->fullness = bufsize_bits;
    return WRENC_RATE_OK;
}

int wrenc_rate_choose_vbv(wrenc_rate* rc, int n, const wrenc_rate_hist* hist, int32_t* qp, double* allowance_bits) {
    if (!rc || n < 1 || !hist || !qp || !rc->vbv) return WRENC_RATE_EINVAL;
    const wrenc_rate_config& c = rc->cfg;
    // the bucket and the bytes spent, walked from the reports over the predictions of the pictures in flight
    double f = rc->fullness, in_flight = 0;
    long long index = rc->reported;
    for (const wrenc_rate::picture& p : rc->pending) {
        const double bytes = rc->predict(p, p.qp);
        in_flight += bytes;
        f = rc->drain(f, bytes, index++);
    }
    // the batch's budget as wrenc_rate_choose draws it, an n-th of it for every picture
    const double spent = c.header_bytes + rc->reported_bytes + in_flight;
    const double error = c.target_bytes * (double)rc->chosen - spent;
    long long window = c.num_pictures - rc->chosen;
    if (window > WRENC_RATE_WINDOW) window = WRENC_RATE_WINDOW;
    if (window < n) window = n;
    const double share = c.target_bytes + error / (double)window;
    for (int k = 0; k < n; ++k, ++index) {
        wrenc_rate::picture p{0.0, c.qp_min, std::vector<double>(64)};
        wrenc_rate_curve(hist + k, p.curve.data());
        const double allowed = f - (index == 0 ? 8.0 * c.header_bytes : 0.0);
        const double cap = std::fmin(share, WRENC_RATE_VBV_SAFETY * allowed / 8.0);
        while (p.qp < c.qp_max && rc->predict(p, p.qp) > cap) ++p.qp;
        if (allowance_bits) allowance_bits[k] = allowed;
        qp[k] = p.qp;
        f = rc->drain(f, rc->predict(p, p.qp), index);
        rc->pending.push_back(std::move(p));
    }
    rc->chosen += n;
    return WRENC_RATE_OK;
}

int wrenc_rate_vbv_allowance(const wrenc_rate* rc, double* allowance_bits, double* bufsize_bits, double* fullness_bits) {
    if (!rc || !rc->vbv) return WRENC_RATE_EINVAL;
    if (allowance_bits) *allowance_bits = rc->fullness - (rc->reported == 0 ? 8.0 * rc->cfg.header_bytes : 0.0);
    if (bufsize_bits) *bufsize_bits = rc->bufsize;
    if (fullness_bits) *fullness_bits = rc->fullness;
    return WRENC_RATE_OK;
}

int wrenc_rate_recode(wrenc_rate* rc, uint64_t actual_bytes, double allowance_bits, int32_t* qp) {
    if (!rc || !rc->vbv || !qp || rc->pending.empty() || actual_bytes < 1 || !std::isfinite(allowance_bits)) return WRENC_RATE_EINVAL;
    wrenc_rate::picture& p = rc->pending.front();
    const double ratio = (double)actual_bytes / rc->predict(p, p.qp);
    const double cap = WRENC_RATE_VBV_SAFETY * allowance_bits / 8.0;
    int q = p.qp < rc->cfg.qp_max ? p.qp + 1 : rc->cfg.qp_max;
    while (q < rc->cfg.qp_max && ratio * rc->predict(p, q) > cap) ++q;
    *qp = p.qp = q;
    return WRENC_RATE_OK;
}
