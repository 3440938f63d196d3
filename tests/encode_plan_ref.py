"""The launch schedule of an encode call, restated from the nested loop wrenc_gpu_encode consisted of before it was planned
(wrenc_amd/csrc/encode_plan.h): which kernel launches it issued, in order, with which arguments, and what it recorded for
the statistics.  The loop is kept in its old shape on purpose -- the list of a mixed call first, then diagonal by diagonal
and lane by lane, launching as it goes -- so that tests/test_encode_plan.py compares the planner with what the library did,
not with a second copy of the planner."""

AUTO, WAVE, TEAM = 0, 1, 2


def reference_plan(cols, rows, qps, schedule, wave_slots, depth3, wpb, team_waves, encode_lanes, pct, pct_depth3):
    """The same dict as wrenc_amd.gpu.encode_plan returns (without the build constants), plus launch_team and launch_ctus:
    per lane and diagonal (span), the kernel and the CTU-pictures the old code recorded for the statistics."""
    n_pictures = len(qps)
    launches, launch_team, launch_ctus = [], [], []

    def launch(lane, team, d, r_min, count, first, n, grid, group, qp, span, ctus):
        launches.append(dict(lane=lane, team=int(team), diag=d, r_min=r_min, count=count, first=first, n=n, grid=grid, group=group,
                             qp=qp, span=span, ctus=ctus))

    # the call's list: QP classes in ascending order, each padded to whole groups of WPB (padding repeats the class's last
    # picture); a call at one QP has none and runs its slots in place
    mixed = any(q != qps[0] for q in qps)
    entries, groups = [], []
    n_entries = n_pictures
    if mixed:
        for q in range(64):
            n_q = 0
            for s in range(n_pictures):
                if qps[s] == q:
                    entries.append(s)
                    n_q += 1
            if not n_q:
                continue
            while len(entries) % wpb:
                entries.append(entries[-1])
            g = 0
            while g * wpb < n_q:
                groups.append((q, min(n_q - g * wpb, wpb)))
                g += 1
        n_entries = len(entries)
    ndiag = cols + 2 * (rows - 1)
    per_group = wpb
    teams_per_group = wpb // team_waves if wpb >= team_waves else 1
    total_groups = (n_entries + per_group - 1) // per_group
    n_team_diags = n_wave_diags = 0
    n_lanes = min(total_groups, encode_lanes)
    spans = 0                                   # (the old code's `launches`: one per lane and diagonal)
    for d in range(ndiag):
        # rows r with 0 <= d - 2r < cols
        r_min = d - (cols - 1)
        r_min = 0 if r_min <= 0 else (r_min + 1) // 2
        r_max = min(d // 2, rows - 1)
        count = r_max - r_min + 1
        if count <= 0:
            continue
        team = schedule == TEAM or (schedule == AUTO and n_pictures * count * 100 <= wave_slots * (pct_depth3 if depth3 else pct))
        if team:
            n_team_diags += 1
        else:
            n_wave_diags += 1
        for l in range(n_lanes):
            g0, g1 = total_groups * l // n_lanes, total_groups * (l + 1) // n_lanes
            lane_first = g0 * per_group         # (+ the first slot for a call at one QP)
            lane_pics = (g1 - g0) * per_group
            if g0 * per_group + lane_pics > n_entries:
                lane_pics = n_entries - g0 * per_group
            if lane_pics <= 0:
                continue
            lane_real = lane_pics               # (without a mixed call's padding)
            if mixed:
                lane_real = sum(groups[g][1] for g in range(g0, g1))
            if team:
                # a call at one QP: one launch; a mixed call: one per QP class of the lane, its pictures only
                ga = g0
                while ga < g1:
                    kq, gb, first, n = qps[0], g1, lane_first, lane_pics
                    if mixed:
                        kq = groups[ga][0]
                        n = 0
                        gb = ga
                        while gb < g1 and groups[gb][0] == kq:
                            n += groups[gb][1]
                            gb += 1
                        first = ga * per_group
                    launch(l, True, d, r_min, count, first, n, count * ((n + teams_per_group - 1) // teams_per_group), -1, kq, spans,
                           count * n)
                    ga = gb
            else:
                # the wave kernel of a mixed call reads each group's constant block from the groups (qp -1)
                launch(l, False, d, r_min, count, lane_first, lane_pics, count * (g1 - g0), g0 if mixed else -1,
                       -1 if mixed else qps[0], spans, count * lane_real)
            launch_team.append(int(team))       # what the old code kept for the statistics, per lane and diagonal
            launch_ctus.append(count * lane_real)
            spans += 1
    ran =TEAM if n_wave_diags == 0 else (WAVE if n_team_diags == 0 else AUTO)
    return dict(launches=launches, entries=entries, groups=groups, n_launches=len(launches), n_entries=len(entries),
                n_groups=len(groups), n_lanes=n_lanes, n_spans=spans, schedule=ran, launch_team=launch_team, launch_ctus=launch_ctus)


def span_stats(plan):
    """What wrenc_gpu_last_encode_stats / _kernel_stats report of a call with this plan, timing apart: the number of
    launches they count (spans) and per kernel {"launches", "ctu_pictures"}."""
    out = {"n_launches": plan["n_spans"], "wave": {"launches": 0, "ctu_pictures": 0}, "team": {"launches": 0, "ctu_pictures": 0}}
    seen = set()
    for L in plan["launches"]:
        o = out["team" if L["team"] else "wave"]
        o["ctu_pictures"] += L["ctus"]
        if L["span"] not in seen:
            seen.add(L["span"])
            o["launches"] += 1
    return out
