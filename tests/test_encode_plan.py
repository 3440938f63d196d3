"""The launch plan of an encode call (wrenc_amd/csrc/encode_plan.h, through wrenc_gpu_test_plan; no device needed) against
the restatement of the loop it replaced (tests/encode_plan_ref.py), record by record, and the invariants the kernels rely
on -- held by the restatement alone first, then by the library's plan."""
import itertools

import numpy as np
import pytest

from encode_plan_ref import AUTO, TEAM, WAVE, reference_plan, span_stats

GEOMETRIES = [(c, r) for c in (1, 2, 3, 5) for r in (1, 2, 4)] + [(120, 68)]
PICTURES = (1, 3, 4, 5, 16, 17, 240)


def _qp_patterns(n):
    """One QP; two QPs interleaved; five QPs whose class sizes are no multiples of the workgroup's four pictures (where the
    call has pictures enough: 3, 5, 2, 1 and then the rest, dealt out of order)."""
    one = [32] * n
    two = [27 if i % 2 else 35 for i in range(n)]
    sizes = [3, 5, 2, 1]
    five = []
    for q, k in zip((40, 22, 63, 0), sizes):
        five += [q] * k
    five = (five + [31] * n)[:n]
    five = five[1::2] + five[0::2]          # classes not contiguous in slot order
    return [list(p) for p in dict.fromkeys(tuple(p) for p in (one, two, five))]


def _wave_slots(n, pct):
    """Both sides of AUTO's threshold n x count x 100 <= slots x pct for a diagonal of one CTU and of two."""
    out = []
    for count in (1, 2):
        at = -(-n * count * 100 // pct)     # the fewest slots at which the diagonal runs as teams
        out += [at, at - 1]
    return sorted(set(s for s in out if s >= 1))


def _true_diagonals(cols, rows):
    """{diagonal: rows of its CTUs} by enumeration: CTU (r, c) is on diagonal c + 2r."""
    diags = {}
    for r, c in itertools.product(range(rows), range(cols)):
        diags.setdefault(c + 2 * r, []).append(r)
    return diags


def _check_invariants(plan, cols, rows, qps, wpb, team_waves, diags):
    n = len(qps)
    entries, groups, mixed = plan["entries"], plan["groups"], bool(plan["entries"])
    assert mixed == (len(set(qps)) > 1)
    # every group of WPB entries holds one QP; a class's real pictures first, its padding repeats its last picture
    if mixed:
        assert len(entries) == wpb * len(groups)
        real = []
        for g, (q, n_real) in enumerate(groups):
            e = entries[g * wpb:(g + 1) * wpb]
            assert 1 <= n_real <= wpb and all(qps[i] == q for i in e)
            assert all(i == e[n_real - 1] for i in e[n_real:])
            real += e[:n_real]
        assert sorted(real) == list(range(n))
        assert [q for q, _ in groups] == sorted(q for q, _ in groups)
        for (qa, na), (qb, _) in zip(groups, groups[1:]):
            assert na == wpb or qa != qb            # only a class's last group is partial
    n_list = len(entries) if mixed else n
    lane_of = {}
    cover = np.zeros((n, cols + 2 * (rows - 1)), np.int64)
    teams_per_group = wpb // team_waves if wpb >= team_waves else 1
    total = 0
    for L in plan["launches"]:
        d, count = L["diag"], L["count"]
        assert diags[d] == list(range(L["r_min"], L["r_min"] + count))          # the diagonal's CTUs, all of them
        assert 0 <= L["first"] and L["n"] >= 1 and L["first"] + L["n"] <= n_list and L["first"] % wpb == 0
        listed = range(L["first"], L["first"] + L["n"])
        if L["team"]:
            # a team launch's pictures are one class's real pictures, and the block it takes is that class's
            pics = [entries[i] for i in listed] if mixed else list(listed)
            assert len(set(pics)) == len(pics) and all(qps[i] == L["qp"] for i in pics) and L["group"] == -1
            assert L["grid"] == count * -(-len(pics) // teams_per_group)
        elif mixed:
            g0, ng = L["group"], L["grid"] // count
            assert L["qp"] == -1 and g0 * wpb == L["first"] and ng * count == L["grid"] and L["n"] == ng * wpb
            pics = [i for g in range(g0, g0 + ng) for i in entries[g * wpb:g * wpb + groups[g][1]]]
        else:
            pics = list(listed)
            assert L["group"] == -1 and L["qp"] == qps[0] and L["grid"] == count * -(-L["n"] // wpb)
        assert L["ctus"] == count * len(pics)
        total += L["ctus"]
        for i in ([entries[j] for j in listed] if mixed else listed):            # padding included: it runs on that lane too
            assert lane_of.setdefault(i, L["lane"]) == L["lane"]                  # a picture appears on exactly one lane
        cover[pics, d] += 1
    assert 0 <= min(lane_of.values()) and max(lane_of.values()) == plan["n_lanes"] - 1
    # every (picture, CTU) is searched exactly once, padding not counted (a diagonal may be empty: 1 column, diagonal 1)
    assert np.all(cover[:, sorted(diags)] == 1) and cover.sum() == n * len(diags)
    assert total == n * cols * rows
    # spans: one per lane and diagonal, in issue order, one kernel each
    spans = [L["span"] for L in plan["launches"]]
    assert spans == sorted(spans) and set(spans) == set(range(plan["n_spans"]))
    for a, b in zip(plan["launches"], plan["launches"][1:]):
        if a["span"] == b["span"]:
            assert (a["lane"], a["diag"], a["team"]) == (b["lane"], b["diag"], b["team"]) == (a["lane"], a["diag"], 1)
    kinds = set(L["team"] for L in plan["launches"])
    assert plan["schedule"] == {(0,): WAVE, (1,): TEAM, (0, 1): AUTO}[tuple(sorted(kinds))]


@pytest.mark.parametrize("cols,rows", GEOMETRIES)
def test_plan_equals_the_loop_it_replaced(built, cols, rows):
    from wrenc_amd import gpu
    diags = _true_diagonals(cols, rows)
    build = None
    cases = 0
    for n in PICTURES:
        for qps in _qp_patterns(n):
            for depth3 in (False, True):
                for schedule in (AUTO, WAVE, TEAM):
                    # (WAVE and TEAM do not read the slots: one value)
                    for slots in (_wave_slots(n, 65 if depth3 else 50) if schedule == AUTO else [5120]):
                        got = gpu.encode_plan(cols, rows, qps, schedule, slots, depth3)
                        if build is None:
                            build = [got[k] for k in ("wpb", "team", "encode_lanes", "team_below_pct", "team_below_pct_depth3")]
                            assert build[3:] == [50, 65]        # what _wave_slots straddles
                        want = reference_plan(cols, rows, qps, schedule, slots, depth3, *build)
                        what = (n, qps[:8], depth3, schedule, slots)
                        _check_invariants(want, cols, rows, qps, build[0], build[1], diags)
                        for k in ("n_launches", "n_entries", "n_groups", "n_lanes", "n_spans", "schedule", "entries", "groups"):
                            assert got[k] == want[k], (k, what)
                        for i, (a, b) in enumerate(zip(got["launches"], want["launches"])):
                            assert a == b, (i, what)
                        _check_invariants(got, cols, rows, qps, build[0], build[1], diags)
                        # the statistics read from the plan are what the old code recorded per lane and diagonal
                        stats = span_stats(got)
                        assert stats["n_launches"] == len(want["launch_team"])
                        for kernel, flag in (("wave", 0), ("team", 1)):
                            assert stats[kernel]["launches"] == want["launch_team"].count(flag), what
                            assert stats[kernel]["ctu_pictures"] == sum(c for t, c in zip(want["launch_team"], want["launch_ctus"]) if t == flag)
                        if schedule == AUTO:
                            # the slots straddle the thresholds: a one-CTU diagonal is a team exactly at or above its own
                            first = got["launches"][0]
                            assert first["count"] == 1 and first["team"] == (n * 100 <= slots * (65 if depth3 else 50))
                        cases += 1
    assert cases >= 7 * 2 * (4 + 2)


def test_plan_refuses_what_an_encode_call_refuses(built):
    from wrenc_amd import gpu
    for args in ((0, 1, [32], AUTO, 5120, False), (1, 0, [32], AUTO, 5120, False), (1, 1, [64], AUTO, 5120, False),
                 (1, 1, [-1, 32], AUTO, 5120, False), (1, 1, [32], 3, 5120, False), (1, 1, [32], AUTO, 0, False)):
        with pytest.raises(gpu.WrencGpuError):
            gpu.encode_plan(*args)
