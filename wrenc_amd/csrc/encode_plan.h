// encode_plan.h -- the launch schedule of one encode call as data (host code only, no HIP).  plan_encode decides everything
// wrenc_gpu_encode used to decide while it launched: which anti-diagonals run as teams, which pictures go to which lane,
// the order and padding of a mixed call's QP classes, and a lane's team launches per class.  wrenc_gpu_encode issues
// Plan::launches in order and the statistics entry points read the kept plan; tests/test_encode_plan.py holds the function
// against a restatement of the loop it replaced, tools/sanitize/encode_plan.cpp runs it under ASan and UBSan.
#pragma once
#include <vector>

namespace wrenc {

enum { kPlanAuto = 0, kPlanWave = 1, kPlanTeam = 2 }; // the values of wrenc_gpu_schedule (include/wrenc_gpu.h)

// how the library was built: waves per workgroup (WPB), waves per team (kTeam), streams of an encode call (kEncodeLanes)
// and AUTO's thresholds in percent of the wave slots (kTeamBelowSlotsPct, kTeamBelowSlotsPctDepth3)
struct PlanBuild {
    int wpb, team, lanes, team_below_pct, team_below_pct_d3;
};

struct PlanGroup { // WPB consecutive entries of a mixed call: one QP, n_real pictures and WPB - n_real entries of padding
    int qp, n_real;
};

struct PlanLaunch {
    int lane;  // the stream: 0 the context's own, l > 0 its extra lane l - 1
    int team;  // 1: ctu_search_team_kernel, 0: ctu_search_kernel
    int diag, r_min, count; // the anti-diagonal, its first CTU row and its number of CTUs (rows r with 0 <= diag - 2r < cols)
    int first, n; // the kernel's pictures: entries first .. first + n - 1 of the list (one QP: of the call's slots)
    int grid;  // workgroups
    int group; // wave kernel of a mixed call: the launch's first group; -1 otherwise
    int qp;    // the QP whose constant block the launch takes; -1: the groups name the blocks (wave kernel of a mixed call)
    int span;  // which (diagonal, lane) pair it belongs to, in issue order: the unit of the per-launch timing
    long long ctus; // CTU-pictures it searches, padding not counted
};

struct Plan {
    std::vector<int> entries;      // mixed call: the picture (index into the call) of every list entry, QP classes ascending,
                                   // each padded to whole groups by repeating its last picture; empty at one QP, which
                                   // runs its slots in place
    std::vector<PlanGroup> groups; // mixed call: one per WPB entries
    std::vector<PlanLaunch> launches; // in issue order
    int n_lanes = 0;
    int n_spans = 0;
    int schedule = kPlanWave; // what runs: WAVE, TEAM, or AUTO where some diagonals run as teams and some as waves
    bool mixed() const { return !entries.empty(); }
};

// qp[0 .. n_pictures - 1]: the QP (0..63) of each picture of the call, in slot order.  Clears and refills `p`; its vectors
// keep their capacity, so a context's plan stops allocating once the largest call has been seen.
inline void plan_encode(Plan& p, int cols, int rows, const int* qp, int n_pictures, int schedule, long long wave_slots, bool d3,
                        const PlanBuild& b) {
    p.entries.clear();
    p.groups.clear();
    p.launches.clear();
    bool mixed = false;
    for (int i = 1; i < n_pictures; ++i) mixed |= qp[i] != qp[0];
    if (mixed)
        for (int q = 0; q < 64; ++q) {
            int n_q = 0;
            for (int i = 0; i < n_pictures; ++i)
                if (qp[i] == q) {
                    p.entries.push_back(i);
                    ++n_q;
                }
            if (!n_q) continue;
            while (p.entries.size() % (size_t)b.wpb) p.entries.push_back(p.entries.back());
            for (int g = 0; g * b.wpb < n_q; ++g) p.groups.push_back(PlanGroup{q, n_q - g * b.wpb < b.wpb ? n_q - g * b.wpb : b.wpb});
        }
    const int n_entries = mixed ? (int)p.entries.size() : n_pictures;
    // Which schedule, decided PER ANTI-DIAGONAL: one wave per CTU fills the GPU only with thousands of CTUs runnable side by
    // side (pictures x CTUs of the diagonal); below that a team of kTeam waves per CTU shortens the CTU's chain of dependent
    // evaluations instead.  The thin first and last diagonals of a big batch run as teams, its wide ones as waves.
    // Pictures are dealt to lanes in units of WPB (the wave schedule's workgroup) whatever the schedule, so a picture stays
    // on one stream; a team launch covers its pictures in groups of WPB / kTeam.
    const int teams_per_group = b.wpb >= b.team ? b.wpb / b.team : 1;
    const int total_groups = (n_entries + b.wpb - 1) / b.wpb;
    const int ndiag = cols + 2 * (rows - 1);
    p.n_lanes = total_groups < b.lanes ? total_groups : b.lanes;
    p.n_spans = 0;
    int n_team_diags = 0, n_wave_diags = 0;
    for (int d = 0; d < ndiag; ++d) {
        int r_min = d - (cols - 1);
        r_min = r_min <= 0 ? 0 : (r_min + 1) / 2;
        int r_max = d / 2;
        if (r_max > rows - 1) r_max = rows - 1;
        const int count = r_max - r_min + 1;
        if (count <= 0) continue;
        const bool team = schedule == kPlanTeam || (schedule == kPlanAuto && (long long)n_pictures * count * 100 <=
                                                                                 wave_slots * (d3 ? b.team_below_pct_d3 : b.team_below_pct));
        ++(team ? n_team_diags : n_wave_diags);
        for (int l = 0; l < p.n_lanes; ++l) {
            const int g0 = (int)((long long)total_groups * l / p.n_lanes), g1 = (int)((long long)total_groups * (l + 1) / p.n_lanes);
            int lane_pics = (g1 - g0) * b.wpb;
            if (g0 * b.wpb + lane_pics > n_entries) lane_pics = n_entries - g0 * b.wpb;
            if (lane_pics <= 0) continue;
            PlanLaunch L = {l, team ? 1 : 0, d, r_min, count, g0 * b.wpb, lane_pics, 0, -1, qp[0], p.n_spans++, 0};
            if (!team) {
                L.grid = count * (g1 - g0);
                L.ctus = (long long)count * lane_pics;
                if (mixed) {
                    int lane_real = 0;
                    for (int g = g0; g < g1; ++g) lane_real += p.groups[(size_t)g].n_real;
                    L.group = g0, L.qp = -1, L.ctus = (long long)count * lane_real;
                }
                p.launches.push_back(L);
                continue;
            }
            // a call at one QP: one launch; a mixed call: one per QP class of the lane, its pictures only (a class's real
            // pictures are contiguous, its padding is at its end)
            for (int ga = g0; ga < g1;) {
                int gb = g1;
                if (mixed) {
                    L.qp = p.groups[(size_t)ga].qp;
                    L.first = ga * b.wpb;
                    L.n = 0;
                    for (gb = ga; gb < g1 && p.groups[(size_t)gb].qp == L.qp; ++gb) L.n += p.groups[(size_t)gb].n_real;
                }
                L.grid = count * ((L.n + teams_per_group - 1) / teams_per_group);
                L.ctus = (long long)count * L.n;
                p.launches.push_back(L);
                ga = gb;
            }
        }
    }
    p.schedule = n_wave_diags == 0 ? kPlanTeam : (n_team_diags == 0 ? kPlanWave : kPlanAuto);
}

} // namespace wrenc
