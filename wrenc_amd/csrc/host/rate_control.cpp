// rate_control.cpp -- include/wrenc_rate.h: the QPs of a batch from its pictures' complexities, a bytes-at-QP model
// whose scale follows the bytes reported so far.  Plain doubles and libm, one thread, no state outside the object: the
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

} // namespace

struct wrenc_rate {
    wrenc_rate_config cfg;
    double samples;             // N
    struct picture {
        double base; // what a = 1 predicts for it at QP 0
        int qp;
    };
    std::deque<picture> pending; // chosen, not yet reported
    long long chosen = 0;       // pictures chosen so far
    double reported_bytes = 0;  // ... and the bytes of those reported
    // reports, halved with every new one: a = fit_bytes / fit_unit (unit: a = 1 at the picture's QP), their mean QP
    // fit_qp / fit_n, and fit_base for the slope between them and the next report
    double fit_bytes = 0, fit_unit = 0, fit_base = 0, fit_qp = 0, fit_n = 0;
    double s_down = kSteepS;    // the slope below the reported QPs

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
    *out = rc;
    return WRENC_RATE_OK;
}

void wrenc_rate_destroy(wrenc_rate* rc) { delete rc; }

int wrenc_rate_choose(wrenc_rate* rc, int n, const uint64_t* satd, int32_t* qp) {
    if (!rc || n < 1 || !satd || !qp) return WRENC_RATE_EINVAL;
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
        rc->pending.push_back({base[(size_t)k], qp[k]});
    }
    rc->chosen += n;
    return WRENC_RATE_OK;
}

int wrenc_rate_report(wrenc_rate* rc, int n, const uint64_t* bytes) {
    if (!rc || n < 1 || !bytes || (size_t)n > rc->pending.size()) return WRENC_RATE_EINVAL;
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
