"""One iteration of a scored planner INSIDE interleaved call sequences (tests/session_ref.py: ("plan_iter", ...) and ("step", "decision"),
make_planner_script): lookahead_plan_sampled -> score_plans -> refit_plans -> draw_plans(index=top[:1]) between held steps, after a
step_skip with early and full envs, after a masked reset, on the beam after a select, and with its decision flown — every iteration held
to the oracle's flight of the same plans by tests/planner_ref.py::check_iteration, everything else compared after every operation.

CPU: the planner scripts of the fixed cases contain each of those placements (read off the oracle's record alone, where the stand-in of
tests/planner_ref.py takes the device's place).
GPU: the seven cases through Session(tree=True); only the case's lane-group width moves in the per-width launch records, the score and
refit records move by the number of plan_iter operations."""
import numpy as np
import pytest

import helpers as H
import session_ref as S

# The fixed cases of tests/test_call_sequences.py and tests/test_tree_sequences.py: one per lane-group width, B = two whole workgroups plus
# a part, time limits in the twenties, both auto_reset settings, normalised and raw, dt 1 and 0.3, keep_active once.
FIXED = [
    S.Case(1, H.ragged(1), True, True, 1.0, False, "random", 23, 3.0, 101),
    S.Case(2, H.ragged(2), False, False, 1.0, False, "random", 23, 5.0, 102),
    S.Case(3, H.ragged(3), True, True, 0.3, True, "random", 25, 5.0, 103),
    S.Case(8, H.ragged(8), True, False, 1.0, False, "random", 22, 5.0, 104),
    S.Case(16, H.ragged(16), False, True, 0.3, False, "lattice", 27, 13.0, 105),
    S.Case(33, H.ragged(33), True, True, 1.0, False, "lattice", 24, 3.0, 106),
    S.Case(64, H.ragged(64), True, False, 1.0, False, "lattice", 26, 3.0, 107),
]
IDS = ["N%d B%d %s %s dt%g %s%s" % (c.N, c.B, "reset" if c.auto_reset else "noreset", "norm" if c.normalize else "raw", c.dt, c.spawn,
                                   " keep" if c.keep_active else "") for c in FIXED]
PLACEMENTS = ("between two held steps", "directly after a step_skip with early and full envs", "after a masked reset of some envs",
              "on the beam after a select", "directly before its decision is flown, K steps, the last K - 1 held")


def _placements(rec):
    seen = set()
    for i, r in enumerate(rec):
        if r["op"][0] != "plan_iter":
            continue
        prev, nxt = rec[i - 1], rec[i + 1]
        if r["batch"] == "root" and prev["op"] == ("step", "held") and nxt["op"] == ("step", "held"):
            seen.add(PLACEMENTS[0])
        if prev["op"][0] == "skip" and prev["batch"] == r["batch"] and prev["early"] > 0 and prev["ran_all"] > 0:
            seen.add(PLACEMENTS[1])
        if prev["op"][0] == "reset" and prev["batch"] == r["batch"] and 0 < prev["selected"] < prev["of"] and r["t0_envs"] > 0:
            seen.add(PLACEMENTS[2])
        if r["batch"] == "beam" and prev["op"][0] == "select" and prev["op"][1] == "beam" and prev["selected"] > 0:
            seen.add(PLACEMENTS[3])
        if nxt["op"][:2] == ("step", "decision") and nxt["batch"] == r["batch"] and nxt["K"] == r["K"] and nxt["held_steps"] == r["K"] - 1 \
                and nxt["nonzero_rows"] > 0:
            seen.add(PLACEMENTS[4])
    return seen


def test_planner_scripts_contain_what_they_are_for():
    """Conditions on the INPUTS, on the oracle alone: every fixed case's script holds every placement; no iteration compares nothing
    (every candidate has an evaluated env); over the cases there are envs without a valid candidate, episodes that end inside an
    iteration's plans, both modes and a flown decision with zero rows (an env whose top is -1)."""
    total = dict(iters=0, none_valid=0, early=0, zero_rows=0, evaluated=0, pairs=0, ndw=0, envs=0)
    modes = set()
    for case in FIXED:
        script = S.make_planner_script(case)
        s = S.Session(case, device=False, tree=True)
        rec = s.run(script)
        missing = set(PLACEMENTS) - _placements(rec)
        assert not missing, (case, sorted(missing))
        for r in rec:
            if r["op"][0] == "plan_iter":
                assert min(r["evaluated_per_candidate"]) >= 1, (case, r["op"])
                modes.add(r["op"][1])
                total["iters"] += 1
                for k, name in (("none_valid", "none_valid"), ("early", "early"), ("evaluated", "evaluated"), ("pairs", "pairs"),
                                ("ndw", "non_decisive_winner"), ("envs", "evaluated_envs")):
                    total[k] += r[name]
            if r["op"][:2] == ("step", "decision"):
                total["zero_rows"] += s.b[r["batch"]].B - r["nonzero_rows"]
    print("planner sequences on the oracle: %s" % total)
    assert modes == {"elite", "softmax"} and total["none_valid"] > 0 and total["early"] > 0 and total["zero_rows"] > 0
    assert 2 * total["evaluated"] >= total["pairs"], total


def test_the_session_refuses_a_decision_nobody_made():
    s = S.Session(FIXED[3], device=False, tree=True)
    s.run([("step", "fresh")])
    with pytest.raises(S.IllegalScript, match="no plan_iter"):
        s.apply(("step", "decision"))
    with pytest.raises(S.IllegalScript, match="root or beam"):
        s.apply(("plan_iter", "elite", 3, 2, "child"))
    s.run([("plan_iter", "elite", 3, 2), ("step", "decision"), ("step", "held")])
    assert s.record[2]["K"] == S.ITER_KS[1] and np.array_equal(s.b["root"].prev_actions, s.b["root"].decision[0])


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", FIXED, ids=IDS)
def test_planner_sequence_matches_oracle(case):
    import time
    from atc_hip import lib
    t0 = time.time()
    W = H.lane_width(case.N)
    counters = {"skip": lib.skip_launch_counts, "traffic": lib.traffic_launch_counts, "lookahead": lib.lookahead_launch_counts,
                "plan": lib.plan_launch_counts, "plan_sampled": lib.plan_sampled_launch_counts, "plan_draw": lib.plan_draw_launch_counts,
                "branch": lib.branch_launch_counts, "select": lib.select_launch_counts, "score": lib.plan_score_launch_counts,
                "refit": lib.plan_refit_launch_counts}
    was = {k: fn() for k, fn in counters.items()}
    script = S.make_planner_script(case)
    iters = sum(op[0] == "plan_iter" for op in script)
    with H.launches() as gained:
        s = S.Session(case, tree=True)
        rec = s.run(script)
        s.env.synchronize()
        s.close()
    grew = {k: {w: n - was[k].get(w, 0) for w, n in fn().items() if n != was[k].get(w, 0)} for k, fn in counters.items()}
    stats = {k: max(r["stats"][k] for r in rec if "stats" in r) for k in ("score", "softmax", "refit")}
    print("planner sequence %s: %.1f s, %d iterations, largest error over its bar %s, launches %s, %s" % (
        case, time.time() - t0, iters, stats, dict(sorted(gained.items())), grew))
    assert gained and all(name.startswith("%d/" % W) for name in gained), gained
    for k in ("skip", "plan_sampled", "branch", "lookahead", "plan", "traffic"):      # counted per lane-group width: only the case's slot may move
        assert set(grew[k]) <= {W}, (k, grew[k])
    assert grew["skip"] and grew["branch"] and grew["select"]       # (select, draw, score and refit have one slot each, whatever the width)
    assert grew["plan_sampled"] == {W: iters} and not grew["lookahead"] and not grew["plan"]
    assert grew["score"] == {"score": iters} and grew["refit"] == {"refit": iters} and grew["plan_draw"] == {"draw": iters}, grew
    assert set(grew["traffic"]) <= {W} and (case.N == 1) == (not grew["traffic"])
