// ASan + UBSan over the host-only code of the buffer model: include/wrenc_ratecurve.h (random pictures of a few sizes: every
// coefficient lands in a bin of the table, the counts add up to the samples) and include/wrenc_rate_vbv.h in
// wrenc_amd/csrc/host/rate_control.cpp (random histograms and sizes through the chooser, the bucket and the re-encode step,
// with the properties the program relies on: QPs within the bounds, a re-encode QP above the picture's, a bucket that
// never holds more than its size, the same calls the same answers) and the refusals.  Stand-alone (tools/sanitize/run.sh
// builds and runs it); never loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/wrenc_rate.h"

static int fail(const char* what, long a, long b) {
    fprintf(stderr, "rate_vbv: %s (%ld, %ld)\n", what, a, b);
    return 1;
}

static wrenc_rate_hist random_hist(std::mt19937_64& rng, int w, int h) {
    wrenc_rate_hist out = {};
    const uint64_t samples[3] = {(uint64_t)w * h, (uint64_t)w * h / 4, (uint64_t)w * h / 4};
    const int centre = (int)(rng() % 50) + 1;
    for (int p = 0; p < 3; ++p) {
        uint64_t left = samples[p];
        for (int k = 0; k < 40 && left; ++k) {
            int b = centre + (int)(rng() % 13) - 6;
            b = b < 0 ? 0 : (b > WRENC_RATECURVE_TOP_BIN ? WRENC_RATECURVE_TOP_BIN : b);
            const uint64_t n = rng() % (left / 4 + 1);
            out.count[p][b] += n;
            left -= n;
        }
        out.count[p][0] += left;
    }
    return out;
}

static int histogram_of_pictures(std::mt19937_64& rng) {
    const int sizes[][2] = {{16, 16}, {32, 32}, {96, 64}, {48, 80}};
    for (const auto& s : sizes)
        for (int kind = 0; kind < 3; ++kind) {
            const int w = s[0], h = s[1];
            // exactly the planes on the heap: a read past them is an error the sanitizer reports
            std::vector<uint8_t> y((size_t)w * h), cb((size_t)w * h / 4), cr((size_t)w * h / 4);
            for (auto* pl : {&y, &cb, &cr})
                for (uint8_t& v : *pl) v = kind == 0 ? (uint8_t)rng() : (kind == 1 ? (uint8_t)(255 * (rng() & 1)) : (uint8_t)93);
            wrenc_rate_hist hist;
            if (wrenc_ratecurve_picture(y.data(), cb.data(), cr.data(), w, h, &hist)) return fail("picture refused", w, h);
            for (int p = 0; p < 3; ++p) {
                uint64_t sum = 0;
                for (int b = 0; b < WRENC_RATECURVE_BINS; ++b) {
                    if (b > WRENC_RATECURVE_TOP_BIN && hist.count[p][b]) return fail("a count beyond the top bin", p, b);
                    sum += hist.count[p][b];
                }
                if (sum != (p ? y.size() / 4 : y.size())) return fail("counts do not add up", p, (long)sum);
            }
            double curve[64];
            if (wrenc_rate_curve(&hist, curve)) return fail("curve refused", w, h);
            for (int q = 1; q < 64; ++q)
                if (!(curve[q] <= curve[q - 1]) || !(curve[q] >= 0)) return fail("curve rises", w, q);
        }
    for (int m = 0; m <= WRENC_RATECURVE_MAX_MAGNITUDE; ++m) {
        const int b = wrenc_ratecurve_bin(m);
        if (b < 0 || b > WRENC_RATECURVE_TOP_BIN || wrenc_ratecurve_bin_floor(b) > m) return fail("bin", m, b);
    }
    if (!wrenc_ratecurve_picture(nullptr, nullptr, nullptr, 32, 32, nullptr)) return fail("null planes accepted", 0, 0);
    return 0;
}

// one run of the controller on the seed's histograms and sizes; the answers go into `trace`
static int controller(uint64_t seed, std::vector<double>& trace) {
    std::mt19937_64 rng(seed);
    const int w = 352, h = 288, qp_max = 40 + (int)(rng() % 24), batch = 1 + (int)(rng() % 7);
    const double target = 500.0 + (double)(rng() % 20000), bufsize = 8.0 * target * (1.0 + (double)(rng() % 40) / 8.0);
    const wrenc_rate_config cfg = {w, h, (int32_t)(rng() % 20), qp_max, 96, target, 150.0};
    wrenc_rate* rc = nullptr;
    if (wrenc_rate_create(&cfg, &rc)) return fail("create", 0, 0);
    if (!wrenc_rate_enable_vbv(rc, 8.0 * target - 1.0) || !wrenc_rate_enable_vbv(rc, NAN)) return fail("a small buffer accepted", 0, 0);
    double allowance = 0, size = 0, fullness = 0;
    if (!wrenc_rate_vbv_allowance(rc, &allowance, &size, &fullness)) return fail("allowance without a buffer", 0, 0);
    if (bufsize <= 8.0 * 150.0) return wrenc_rate_destroy(rc), 0;
    if (wrenc_rate_enable_vbv(rc, bufsize)) return fail("enable", 0, 0);
    std::vector<wrenc_rate_hist> hists((size_t)batch);
    std::vector<int32_t> qps((size_t)batch);
    std::vector<double> allow((size_t)batch);
    uint64_t satd[3] = {1000000, 100000, 100000};
    if (!wrenc_rate_choose(rc, 1, satd, qps.data())) return fail("the complexity chooser with a buffer", 0, 0);
    for (int round = 0; round < 96 / batch; ++round) {
        for (auto& hst : hists) hst = random_hist(rng, w, h);
        if (wrenc_rate_choose_vbv(rc, batch, hists.data(), qps.data(), round & 1 ? allow.data() : nullptr)) return fail("choose", round, 0);
        for (int k = 0; k < batch; ++k) {
            if (qps[(size_t)k] < cfg.qp_min || qps[(size_t)k] > qp_max) return fail("QP out of bounds", round, qps[(size_t)k]);
            trace.push_back(qps[(size_t)k]);
            if (wrenc_rate_vbv_allowance(rc, &allowance, &size, &fullness)) return fail("allowance", round, k);
            if (size != bufsize || fullness > bufsize) return fail("bucket above its size", round, k);
            // a size between a tenth and ten times something plausible; over the allowance it is coded again
            uint64_t bytes = 1 + rng() % (uint64_t)(4.0 * target);
            int32_t q = qps[(size_t)k];
            for (int tries = 0; 8.0 * (double)bytes > allowance && tries < 64; ++tries) {
                int32_t next = 0;
                if (wrenc_rate_recode(rc, bytes, allowance, &next)) return fail("recode", round, k);
                if (next > qp_max || next < q || (next == q && q != qp_max)) return fail("recode QP", q, next);
                trace.push_back(next);
                if (next == q) break;
                bytes = 1 + bytes * 2 / 3; // (what a higher QP might give)
                q = next;
            }
            if (wrenc_rate_report(rc, 1, &bytes)) return fail("report", round, k);
            trace.push_back(fullness);
        }
    }
    uint64_t bytes = 1;
    int32_t q = 0;
    if (!wrenc_rate_report(rc, 1, &bytes) || !wrenc_rate_recode(rc, 100, 100.0, &q)) return fail("nothing outstanding, yet accepted", 0, 0);
    if (!wrenc_rate_choose_vbv(rc, 0, hists.data(), qps.data(), nullptr) || !wrenc_rate_choose_vbv(rc, 1, nullptr, qps.data(), nullptr))
        return fail("bad arguments accepted", 0, 0);
    wrenc_rate_destroy(rc);
    return 0;
}

int main() {
    std::mt19937_64 rng(2024);
    if (histogram_of_pictures(rng)) return 1;
    size_t answers = 0;
    for (uint64_t seed = 1; seed <= 200; ++seed) {
        std::vector<double> first, second;
        if (controller(seed, first) || controller(seed, second)) return 1;
        if (first != second) return fail("the same calls, other answers", (long)seed, 0);
        answers += first.size();
    }
    printf("rate_vbv: ok, %zu answers over 200 seeds\n", answers);
    return 0;
}
