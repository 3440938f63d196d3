// ASan + UBSan over include/wrenc_scale.h: every output index of a few size pairs, with the properties the device's tables
// rely on -- at most 16 taps, coefficients that sum to 4096 and fit 16 bits, the first tap within two stretched samples
// of the plane -- and the refusals.  Stand-alone (tools/sanitize/run.sh builds and runs it); never loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/wrenc_scale.h"

static int fail(const char* what, int n_in, int n_out, int o) {
    fprintf(stderr, "scale_taps: %s at %d -> %d, output %d\n", what, n_in, n_out, o);
    return 1;
}

int main() {
    const int pairs[][2] = {{16, 16}, {3840, 1920}, {2160, 1080}, {3840, 1280}, {8192, 2050}, {16384, 4096}, {4096, 16384}, {960, 1920},
                            {70, 34}, {50, 62}, {35, 17}, {17, 47}, {64, 16}, {16, 64}, {1, 4}, {4, 1}, {16384, 16384}};
    long taps_seen = 0;
    for (const auto& p : pairs) {
        const int n_in = p[0], n_out = p[1];
        for (int o = 0; o < n_out; ++o) {
            // exactly 17 coefficients on the heap: a write past them is an error the sanitizer reports
            std::vector<int16_t> coef(WRENC_SCALE_MAX_TAPS);
            int first = 0, n = 0;
            if (wrenc_scale_taps(n_in, n_out, o, &first, &n, coef.data())) return fail("refused", n_in, n_out, o);
            if (n < 1 || n > 16) return fail("tap count", n_in, n_out, o);
            long sum = 0;
            for (int j = 0; j < n; ++j) sum += coef[(size_t)j];
            if (sum != WRENC_SCALE_UNITY) return fail("sum", n_in, n_out, o);
            const long reach = 2L * (n_in > n_out ? (n_in + n_out - 1) / n_out : 1) + 1;
            if (first < -reach || first + n - 1 > n_in - 1 + reach) return fail("reach", n_in, n_out, o);
            if (n_in == n_out && (n != 1 || first != o)) return fail("identity", n_in, n_out, o);
            taps_seen += n;
        }
    }
    int first, n;
    int16_t coef[WRENC_SCALE_MAX_TAPS];
    const int refused[][3] = {{66, 16, 0}, {16, 66, 0}, {0, 16, 0}, {16, 0, 0}, {16, 16, 16}, {16, 16, -1}, {16386, 16386, 0}, {-4, -1, 0}};
    for (const auto& r : refused)
        if (wrenc_scale_taps(r[0], r[1], r[2], &first, &n, coef) != -1) return fail("not refused", r[0], r[1], r[2]);
    if (wrenc_scale_taps(16, 16, 0, nullptr, &n, coef) != -1) return fail("null pointer", 16, 16, 0);
    printf("scale_taps: %ld taps over %zu size pairs, clean\n", taps_seen, sizeof(pairs) / sizeof(pairs[0]));
    return 0;
}
