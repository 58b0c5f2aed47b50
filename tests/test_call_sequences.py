"""Interleaved calls against the oracle (tests/session_ref.py): step / held step / step_skip / rollout / reset / observe /
observe_traffic / set_state / set_last_action in scripted sequences, everything compared after every operation.

CPU: the scripts contain what they are for (asserted on the oracle's record alone); the session refuses an illegal held step.
GPU: every case through Session — outputs by the bars of tests/bars.py, the whole state bit for bit after each operation, the
launch record printed and confined to the case's lane-group width.

ATC_SEQ_CASES / ATC_SEQ_SEED widen the drawn part of the sweep (as ATC_FUZZ_* do for tests/test_fuzz_parity.py)."""
import os

import numpy as np
import pytest

import helpers as H
import session_ref as S

# One case per lane-group width, idle lanes where the width allows (3 in 4, 33 in 64); B = two whole workgroups plus a part; time
# limits in the twenties (22 or more: see session_ref.PREAMBLE) so that episodes end inside skips and rollouts; random entry where it does not put aircraft on top of each
# other at once (few aircraft), the slot lattice otherwise; both auto_reset settings, normalised and raw, dt 1 and 0.3, keep_active once.
FIXED = [
    S.Case(1, H.ragged(1), True, True, 1.0, False, "random", 23, 3.0, 101),
    S.Case(2, H.ragged(2), False, False, 1.0, False, "random", 23, 5.0, 102),
    S.Case(3, H.ragged(3), True, True, 0.3, True, "random", 25, 5.0, 103),
    S.Case(8, H.ragged(8), True, False, 1.0, False, "random", 22, 5.0, 104),
    S.Case(16, H.ragged(16), False, True, 0.3, False, "lattice", 27, 13.0, 105),
    S.Case(33, H.ragged(33), True, True, 1.0, False, "lattice", 24, 3.0, 106),
    S.Case(64, H.ragged(64), True, False, 1.0, False, "lattice", 26, 3.0, 107),
]


def _drawn():
    n, seed = int(os.environ.get("ATC_SEQ_CASES", "4")), int(os.environ.get("ATC_SEQ_SEED", "2024"))
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        N = int(rng.choice([1, 2, 3, 5, 8, 13, 16, 17, 33, 40, 64]))
        out.append(S.Case(N, H.ragged(N), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), float(rng.choice([1.0, 0.3])),
                          bool(rng.uniform() < 0.2), "random" if N <= 8 else "lattice", int(rng.integers(22, 30)),
                          float(rng.choice([3.0, 5.0, 13.0])), seed * 1000 + i))
    return out


CASES = FIXED + _drawn()
IDS = ["N%d B%d %s %s dt%g %s%s seed%d" % (c.N, c.B, "reset" if c.auto_reset else "noreset", "norm" if c.normalize else "raw", c.dt,
                                           c.spawn, " keep" if c.keep_active else "", c.seed) for c in CASES]


# ---------------------------------------------------------------------------------------------------------------- CPU
def _after(record, i, kinds):
    """the record of the nearest operation before i whose kind is in `kinds` and the kinds in between"""
    between = []
    for j in range(i - 1, -1, -1):
        if record[j]["op"][0] in kinds:
            return record[j], between
        between.append(record[j]["op"][0])
    return None, between


def test_scripts_contain_what_they_are_for():
    """Conditions on the INPUTS, on the oracle alone (tests/test_frame_skip.py::test_case_events_on_the_oracle): over the fixed cases
    the scripts hold every interaction the sequence test exists for — the GPU run cannot pass by flying nothing."""
    seen = set()
    stepping = ("step", "skip", "rollout")
    for case in FIXED:
        script = S.make_script(case)
        assert len(script) == S.LENGTH and tuple(script[:len(S.PREAMBLE)]) == S.PREAMBLE
        assert {op[1] for op in script if op[0] == "skip"} >= set(S.SKIP_KS)
        assert {op[2] for op in script if op[0] == "rollout"} == {1, 4} and {op[3] for op in script if op[0] == "rollout"} == {True, False}
        assert {op[1] for op in script if op[0] == "reset"} >= {"random", "zero", "one", "none"}
        rec = S.Session(case, device=False).run(script)
        wide_since = False      # a set_state (to a WIDE heading, among others) with no reset of all envs since
        for i, r in enumerate(rec):
            op = r["op"]
            if op == ("step", "held"):
                prev, between = _after(rec, i, stepping)
                if prev["op"][0] == "skip" and prev["early"] > 0 and prev["ran_all"] > 0 and not between:
                    seen.add("held step directly after a step_skip with early and full envs, auto_reset %s" % ("on" if case.auto_reset else "off"))
                if prev["op"][0] == "rollout" and prev["op"][2] == 4:
                    seen.add("held step after rollout(hold=4)")
                resets = [rec[j] for j in range(i - len(between), i) if rec[j]["op"][0] == "reset"]
                if any(0 < x["selected"] < x["of"] for x in resets) and r["t0_envs"] > 0:
                    seen.add("held step after a masked reset of some but not all envs")
                if between and set(between) == {"observe"} and prev["op"] == ("step", "held"):
                    seen.add("observe between two held steps")
            if op[0] == "set_state":
                wide_since = True
            if op[0] in ("rollout", "skip") and wide_since and r["wide_active"] > 0:
                seen.add("%s after set_state to a WIDE heading, aircraft under control" % op[0])
            if op[0] == "observe" and r["wide"] and r["handed_over"] and r["off_grid"]:
                seen.add("observe of WIDE + handed-over + off-grid aircraft")
            if op[0] == "reset" and op[1] not in ("none", "one") and r["hi_bit_clear_selected"]:
                seen.add("masked reset, N = %d, of an env whose mask bit >= 32 was clear" % case.N)
            if op[0] == "reset" and op[1] not in ("none", "one") and case.spawn == "random" and r["max_episode_selected"] >= 3 and 0 < r["selected"] < r["of"]:
                seen.add("masked reset under random entry of an env in episode >= 3")
            if op[0] in ("reset", "observe") and op[1] in ("zero", "one"):
                seen.add("all-%s mask (%s)" % (op[1], op[0]))
            if op[0] == "traffic" and r["short"]:
                seen.add("observe_traffic with fewer than K candidates")
    want = {"held step directly after a step_skip with early and full envs, auto_reset on",      # the early ones wait in their spawn state
            "held step directly after a step_skip with early and full envs, auto_reset off", "held step after rollout(hold=4)",
            "held step after a masked reset of some but not all envs", "observe between two held steps",
            "rollout after set_state to a WIDE heading, aircraft under control", "skip after set_state to a WIDE heading, aircraft under control",
            "observe of WIDE + handed-over + off-grid aircraft", "masked reset, N = 33, of an env whose mask bit >= 32 was clear",
            "masked reset, N = 64, of an env whose mask bit >= 32 was clear", "masked reset under random entry of an env in episode >= 3",
            "all-zero mask (reset)", "all-one mask (reset)", "all-zero mask (observe)", "observe_traffic with fewer than K candidates"}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("case", CASES[len(FIXED):], ids=IDS[len(FIXED):])
def test_drawn_scripts_are_legal_on_the_oracle(case):
    """every drawn case's script runs through the legality rule on the oracle alone, and something ends and something goes on in it"""
    rec = S.Session(case, device=False).run(S.make_script(case))
    assert sum(r.get("done", 0) for r in rec) > 0


def test_the_session_refuses_an_illegal_held_step():
    case = FIXED[2]
    for script, why in (
            ([("step", "held")], "no step"),
            ([("reset", "none"), ("observe", "none"), ("step", "held")], "no step"),
            ([("step", "fresh"), ("set_last_action",), ("step", "held")], "set_last_action"),
            ([("skip", 5), ("step", "held"), ("set_last_action",), ("reset", "one"), ("step", "held")], "set_last_action")):
        s = S.Session(case, device=False)
        with pytest.raises(S.IllegalScript, match=why):
            s.run(script)
        assert len(s.done_ops) == len(script) - 1, "the illegal step was not applied"
    # the rule itself: the same BITS (0.0 and -0.0 differ), a record written from outside, no step at all
    a = np.zeros((2, 3, 3), np.float32)
    assert S.held_is_legal(a, False, a.copy()) == (True, "")
    assert not S.held_is_legal(a, False, -a)[0] and not S.held_is_legal(a, True, a)[0] and not S.held_is_legal(None, False, a)[0]
    # legal: after a skip, a rollout, a reset, an observe, placed aircraft; a full repeat makes it legal again
    S.Session(case, device=False).run([("skip", 2), ("step", "held"), ("rollout", 4, 4, False), ("reset", "random"), ("set_state",),
                                       ("observe", "one"), ("step", "held"), ("set_last_action",), ("step", "repeat"), ("step", "held")])


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_call_sequence_matches_oracle(case):
    import time
    from atc_hip import lib
    t0 = time.time()
    W = H.lane_width(case.N)
    skip0, tr0 = lib.skip_launch_counts(), lib.traffic_launch_counts()
    with H.launches() as gained:
        s = S.Session(case)
        s.run(S.make_script(case))
        s.env.synchronize()
        s.close()
    grew = lambda now, was: {w: n - was.get(w, 0) for w, n in now.items() if n != was.get(w, 0)}   # noqa: E731
    skips, traffic = grew(lib.skip_launch_counts(), skip0), grew(lib.traffic_launch_counts(), tr0)
    print("call sequence %s: %.1f s, launches %s, skip %s, traffic %s" % (case, time.time() - t0, dict(sorted(gained.items())), skips, traffic))
    assert gained and all(name.startswith("%d/" % W) for name in gained), gained
    assert set(skips) == {W} and set(traffic) <= {W} and (case.N == 1) == (not traffic)
