// ASan + UBSan over wrenc_amd/csrc/encode_plan.h: plan_encode over the sweep of tests/test_encode_plan.py (geometries, call
// sizes, QP patterns, schedules, wave slots at both sides of AUTO's thresholds, both depths), into ONE Plan as a context
// does, with the bounds the launch loop of wrenc_gpu_encode relies on checked per launch and every (picture, CTU) counted.
// Stand-alone (tools/sanitize/run.sh builds and runs it); never loaded into Python.
#include <cstdio>
#include <vector>

#include "../../wrenc_amd/csrc/encode_plan.h"

using namespace wrenc;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            fprintf(stderr, "encode_plan: line %d: %s (%dx%d CTUs, %d pictures, schedule %d, slots %lld)\n", __LINE__, #cond, cols, rows, n, \
                    schedule, slots);                                             \
            return 1;                                                             \
        }                                                                         \
    } while (0)

static const PlanBuild kBuild = {4, 4, 4, 50, 65}; // WPB, kTeam, kEncodeLanes and the two thresholds of the library's build

static std::vector<int> pattern(int which, int n) {
    std::vector<int> q((size_t)n, 32);
    if (which == 1)
        for (int i = 0; i < n; ++i) q[(size_t)i] = i % 2 ? 27 : 35;
    if (which == 2) { // five QPs, class sizes 3, 5, 2, 1 and the rest, dealt out of order
        const int qs[4] = {40, 22, 63, 0}, sizes[4] = {3, 5, 2, 1};
        std::vector<int> five;
        for (int k = 0; k < 4; ++k) five.insert(five.end(), (size_t)sizes[k], qs[k]);
        five.resize((size_t)n > five.size() ? (size_t)n : five.size(), 31);
        five.resize((size_t)n);
        q.clear();
        for (int i = 1; i < n; i += 2) q.push_back(five[(size_t)i]);
        for (int i = 0; i < n; i += 2) q.push_back(five[(size_t)i]);
    }
    return q;
}

static int check(const Plan& p, int cols, int rows, const std::vector<int>& qp, int schedule, long long slots) {
    const int n = (int)qp.size(), wpb = kBuild.wpb;
    const int n_list = p.mixed() ? (int)p.entries.size() : n;
    CHECK(p.groups.size() * (size_t)wpb == p.entries.size());
    CHECK(p.n_lanes >= 1 && p.n_lanes <= kBuild.lanes);
    std::vector<int> cover((size_t)n * cols * rows, 0);
    long long total = 0;
    for (const PlanLaunch& L : p.launches) {
        CHECK(L.lane >= 0 && L.lane < p.n_lanes && L.span >= 0 && L.span < p.n_spans);
        CHECK(L.count >= 1 && L.r_min >= 0 && L.r_min + L.count <= rows && L.grid >= 1);
        CHECK(L.first >= 0 && L.n >= 1 && L.first + L.n <= n_list);
        CHECK(L.qp >= -1 && L.qp < 64 && (L.qp >= 0 || (!L.team && p.mixed())));
        const int groups = L.grid / L.count;
        if (L.group >= 0) CHECK(!L.team && p.mixed() && L.group + groups <= (int)p.groups.size() && L.group * wpb == L.first);
        // the pictures it searches, padding left out
        for (int i = 0; i < L.n; ++i) {
            int pic = L.first + i;
            if (p.mixed()) {
                if (!L.team && i % wpb >= p.groups[(size_t)(L.group + i / wpb)].n_real) continue;
                pic = p.entries[(size_t)pic];
            }
            CHECK(pic >= 0 && pic < n && (!L.team || qp[(size_t)pic] == L.qp));
            for (int r = L.r_min; r < L.r_min + L.count; ++r) {
                const int c = L.diag - 2 * r;
                CHECK(c >= 0 && c < cols);
                ++cover[((size_t)pic * rows + r) * cols + c];
                ++total;
            }
        }
    }
    for (const int c : cover) CHECK(c == 1);
    long long ctus = 0;
    for (const PlanLaunch& L : p.launches) ctus += L.ctus;
    CHECK(ctus == total && total == (long long)n * cols * rows);
    return 0;
}

int main() {
    const int geo[][2] = {{1, 1}, {1, 2}, {1, 4}, {2, 1}, {2, 2}, {2, 4}, {3, 1}, {3, 2}, {3, 4}, {5, 1}, {5, 2}, {5, 4}, {120, 68}};
    const int pictures[] = {1, 3, 4, 5, 16, 17, 240};
    Plan p; // one, as in a context: refilled by every call
    int cases = 0;
    for (const auto& g : geo)
        for (const int n : pictures)
            for (int which = 0; which < 3; ++which)
                for (int d3 = 0; d3 < 2; ++d3)
                    for (int schedule = 0; schedule < 3; ++schedule)
                        for (int side = 0; side < 4; ++side) {
                            const int pct = d3 ? kBuild.team_below_pct_d3 : kBuild.team_below_pct, count = 1 + side / 2;
                            const long long slots = ((long long)n * count * 100 + pct - 1) / pct - side % 2;
                            if (slots < 1) continue;
                            const std::vector<int> qp = pattern(which, n);
                            plan_encode(p, g[0], g[1], qp.data(), n, schedule, slots, d3 != 0, kBuild);
                            if (check(p, g[0], g[1], qp, schedule, slots)) return 1;
                            ++cases;
                        }
    printf("encode_plan: %d plans clean\n", cases);
    return 0;
}
