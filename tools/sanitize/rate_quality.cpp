// ASan + UBSan over the host-only code of the quality mode: include/wrenc_distcurve.h (random, binary and flat pictures of a
// few sizes: no error above half a step or the coefficient, a flat plane all zeros), the kernel's division-free quantiser
// (wrenc_amd/csrc/distcurve_quant.h) against the definition at EVERY magnitude and QP, and include/wrenc_rate_quality.h in
// wrenc_amd/csrc/host/rate_quality.cpp (random curves and PSNR tables through the chooser and the reports, with the
// properties the program relies on: QPs within the bounds, no QP tried twice, an end within max_recodes, the kept coding the
// largest passing one tried; empty batches, qp_min == qp_max, max_recodes 0, an SSE of 0; the same calls the same answers)
// and the refusals.  Stand-alone (tools/sanitize/run.sh builds and runs it); never loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../../include/wrenc_rate_quality.h"
#include "../../wrenc_amd/csrc/distcurve_quant.h"

static int fail(const char* what, long a, long b) {
    fprintf(stderr, "rate_quality: %s (%ld, %ld)\n", what, a, b);
    return 1;
}

template <int Q>
static int quantiser_at() {
    if (wrenc::dq_step(Q) != wrenc_distcurve_step(Q)) return fail("step", Q, wrenc::dq_step(Q));
    for (int c = 0; c <= WRENC_RATECURVE_MAX_MAGNITUDE; ++c) {
        const uint64_t want = wrenc_distcurve_error(c, Q);
        if (wrenc::dq_error2<Q>((float)(8 * c)) != want) return fail("the kernel's quantiser", Q, c);
        if (want >= (1u << 30) || want > (uint64_t)WRENC_DISTCURVE_MAX_ERROR * WRENC_DISTCURVE_MAX_ERROR) return fail("error bound", Q, c);
    }
    return 0;
}
template <int... Q>
static int quantiser(std::integer_sequence<int, Q...>) {
    return (quantiser_at<Q>() | ...);
}

static int curves_of_pictures(std::mt19937_64& rng) {
    const int sizes[][2] = {{16, 16}, {32, 32}, {96, 64}, {48, 80}};
    for (const auto& s : sizes)
        for (int kind = 0; kind < 3; ++kind) {
            const int w = s[0], h = s[1];
            // exactly the planes on the heap: a read past them is an error the sanitizer reports
            std::vector<uint8_t> y((size_t)w * h), cb((size_t)w * h / 4), cr((size_t)w * h / 4);
            for (auto* pl : {&y, &cb, &cr})
                for (uint8_t& v : *pl) v = kind == 0 ? (uint8_t)rng() : (kind == 1 ? (uint8_t)(255 * (rng() & 1)) : (uint8_t)128);
            wrenc_dist_curve curve;
            if (wrenc_distcurve_picture(y.data(), cb.data(), cr.data(), w, h, &curve)) return fail("picture refused", w, h);
            for (int p = 0; p < 3; ++p)
                for (int q = 0; q < WRENC_DISTCURVE_QPS; ++q) {
                    const uint64_t half = (uint64_t)wrenc_distcurve_step(q) / 2, n = p ? y.size() / 4 : y.size();
                    if (curve.sse8[p][q] > n * half * half) return fail("an error above half a step", p, q);
                    if (kind == 2 && curve.sse8[p][q]) return fail("a flat plane with an error", p, q);
                }
            if (std::isnan(wrenc_quality_predict(&curve, w, h, 30)) || !std::isnan(wrenc_quality_predict(&curve, w, h, 64)))
                return fail("predict", w, h);
        }
    if (!wrenc_distcurve_picture(nullptr, nullptr, nullptr, 32, 32, nullptr)) return fail("null planes accepted", 0, 0);
    std::vector<uint8_t> y(24 * 16), c(12 * 8);
    wrenc_dist_curve curve;
    if (!wrenc_distcurve_picture(y.data(), c.data(), c.data(), 24, 16, &curve)) return fail("a width of 24 accepted", 0, 0);
    return 0;
}

// a curve whose luma row predicts psnr[q] for a picture of `samples` samples
static wrenc_dist_curve curve_of(const double psnr[64], double samples) {
    wrenc_dist_curve c = {};
    for (int q = 0; q < 64; ++q) c.sse8[0][q] = (uint64_t)std::llround(4096.0 * 255.0 * 255.0 * samples / std::pow(10.0, psnr[q] / 10.0));
    return c;
}

// one run of the controller on the seed's tables; the answers go into `trace`
static int controller(uint64_t seed, std::vector<double>& trace) {
    std::mt19937_64 rng(seed);
    const int w = 16 * (1 + (int)(rng() % 20)), h = 16 * (1 + (int)(rng() % 12));
    const double samples = (double)w * h;
    int qp_min = (int)(rng() % 40), qp_max = qp_min + (int)(rng() % (64 - qp_min));
    if (seed % 7 == 0) qp_max = qp_min;
    const int max_recodes = seed % 5 == 0 ? 0 : (int)(rng() % (WRENC_QUALITY_MAX_RECODES + 1));
    const double target = 30.0 + (double)(rng() % 150) / 10.0;
    wrenc_quality* q = wrenc_quality_create(target, qp_min, qp_max, max_recodes);
    if (!q) return fail("create", qp_min, qp_max);
    struct Owner { // (a failure below returns at once: no leak report on top of its message)
        wrenc_quality* q;
        ~Owner() { wrenc_quality_destroy(q); }
    } owner{q};
    int32_t next = 0;
    int accepted = 0;
    if (!wrenc_quality_report(q, 0, qp_min, 1, 1, &next, &accepted)) return fail("a report without a batch", 0, 0);
    for (int round = 0; round < 6; ++round) {
        const int batch = round == 2 ? 0 : 1 + (int)(rng() % 6);
        std::vector<wrenc_dist_curve> curves((size_t)batch);
        std::vector<std::vector<double>> truth((size_t)batch, std::vector<double>(64));
        for (int k = 0; k < batch; ++k) {
            double pred[64];
            const double top = 35.0 + (double)(rng() % 200) / 10.0, slope = 0.1 + (double)(rng() % 10) / 10.0, off = (double)(rng() % 60) / 10.0 - 3.0;
            for (int x = 0; x < 64; ++x) {
                pred[x] = top - slope * x;
                truth[(size_t)k][(size_t)x] = pred[x] + off + (double)(rng() % 100) / 100.0 - 0.5; // (not monotone where the slope is small)
            }
            curves[(size_t)k] = curve_of(pred, samples);
        }
        std::vector<int32_t> qps((size_t)batch + 1);
        if (wrenc_quality_choose(q, batch, batch ? curves.data() : nullptr, w, h, qps.data())) return fail("choose", round, batch);
        for (int k = 0; k < batch; ++k) {
            bool tried[64] = {};
            int qp = qps[(size_t)k], best = -1, lowest = 64, codings = 0;
            for (;;) {
                if (qp < qp_min || qp > qp_max) return fail("QP out of bounds", qp, k);
                if (tried[qp]) return fail("a QP tried twice", qp, k);
                tried[qp] = true;
                ++codings;
                const double psnr = truth[(size_t)k][(size_t)qp];
                // an SSE of 0 now and then: an infinite PSNR
                const uint64_t sse = rng() % 50 == 0 ? 0 : (uint64_t)std::llround(255.0 * 255.0 * samples / std::pow(10.0, psnr / 10.0));
                const bool pass = sse == 0 || 10.0 * std::log10(255.0 * 255.0 * samples / (double)sse) >= target;
                if (pass && qp > best) best = qp;
                if (qp < lowest) lowest = qp;
                if (wrenc_quality_report(q, k, qp, sse, (uint64_t)samples, &next, &accepted)) return fail("report", round, k);
                trace.push_back(next);
                trace.push_back(accepted);
                if (accepted) break;
                if (codings > max_recodes) return fail("more codings than max_recodes allows", codings, max_recodes);
                qp = next;
            }
            if (next != (best >= 0 ? best : lowest)) return fail("the kept coding", next, best);
            if (wrenc_quality_tries(q, k) != codings) return fail("tries", k, codings);
            if (!wrenc_quality_report(q, k, qp_min, 1, 1, &next, &accepted)) return fail("a report after acceptance", round, k);
        }
        trace.push_back(wrenc_quality_correction(q));
    }
    uint64_t reencoded = 0, misses = 0;
    wrenc_quality_totals(q, &reencoded, &misses);
    wrenc_quality_totals(q, nullptr, nullptr);
    trace.push_back((double)reencoded);
    trace.push_back((double)misses);
    if (max_recodes == 0 && reencoded) return fail("max_recodes 0, yet a recode", (long)reencoded, 0);
    return 0;
}

int main() {
    if (quantiser(std::make_integer_sequence<int, 64>())) return 1;
    std::mt19937_64 rng(2025);
    if (curves_of_pictures(rng)) return 1;
    if (wrenc_quality_create(NAN, 0, 63, 3) || wrenc_quality_create(37.0, 5, 4, 3) || wrenc_quality_create(37.0, 0, 64, 3) ||
        wrenc_quality_create(37.0, 0, 63, WRENC_QUALITY_MAX_RECODES + 1))
        return fail("a bad configuration accepted", 0, 0);
    wrenc_quality_destroy(nullptr);
    size_t answers = 0;
    for (uint64_t seed = 1; seed <= 300; ++seed) {
        std::vector<double> first, second;
        if (controller(seed, first) || controller(seed, second)) return 1;
        if (first != second) return fail("the same calls, other answers", (long)seed, 0);
        answers += first.size();
    }
    printf("rate_quality: ok, 64 x 16,321 quantiser steps, %zu answers over 300 seeds\n", answers);
    return 0;
}
