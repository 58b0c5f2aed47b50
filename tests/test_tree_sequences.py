"""Look-ahead, plan, drawn plans, branch and select INSIDE interleaved call sequences (tests/session_ref.py, tree sessions): the calls a
planner makes — score between held steps, branch and hold the decision, fly the children on, keep a beam, commit, stash and restore —
against the oracle, everything compared after every operation, on three batches (root, child, beam).

CPU: the tree scripts contain what they are for and leave enough env-candidates evaluated (asserted on the oracle's record alone); drawn
scripts are legal; the session refuses a held step that a not-evaluated child cannot take; the plain scripts of tests/test_call_sequences.py
and their oracle records are what they were before Session learnt about batches (a digest).
GPU: every case through Session(tree=True); the launch record printed, confined to the case's lane-group width, every new entry point in it.

ATC_TREE_CASES / ATC_TREE_SEED widen the drawn part of the sweep."""
import hashlib
import os

import numpy as np
import pytest

import helpers as H
import session_ref as S
import skip_ref

# The fixed cases of tests/test_call_sequences.py (the digest below holds them to it): one per lane-group width, B = two whole workgroups
# plus a part — the smallest shapes at which the kernels' tile and candidate-group mapping still has a partial workgroup —, time limits
# in the twenties so that episodes end inside branches and plans, both auto_reset settings, normalised and raw, dt 1 and 0.3, keep_active once.
FIXED = [
    S.Case(1, H.ragged(1), True, True, 1.0, False, "random", 23, 3.0, 101),
    S.Case(2, H.ragged(2), False, False, 1.0, False, "random", 23, 5.0, 102),
    S.Case(3, H.ragged(3), True, True, 0.3, True, "random", 25, 5.0, 103),
    S.Case(8, H.ragged(8), True, False, 1.0, False, "random", 22, 5.0, 104),
    S.Case(16, H.ragged(16), False, True, 0.3, False, "lattice", 27, 13.0, 105),
    S.Case(33, H.ragged(33), True, True, 1.0, False, "lattice", 24, 3.0, 106),
    S.Case(64, H.ragged(64), True, False, 1.0, False, "lattice", 26, 3.0, 107),
]

# sha256 over make_script(case), the per-operation `done` counts and the final oracle state of the seven FIXED cases, taken before
# Session was generalised to named batches: the plain session tests mean what they meant
PLAIN_DIGEST = "7f11c0972eb38b5f0408c578d3037ab8bb8f79a60d6f8ab7aab2585dc9393ab8"


def _drawn():
    n, seed = int(os.environ.get("ATC_TREE_CASES", "2")), int(os.environ.get("ATC_TREE_SEED", "2025"))
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        N = int(rng.choice([2, 3, 5, 8, 13, 16, 17, 33, 40, 64]))
        out.append(S.Case(N, H.ragged(N), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), float(rng.choice([1.0, 0.3])),
                          bool(rng.uniform() < 0.2), "random" if N <= 8 else "lattice", int(rng.integers(22, 30)),
                          float(rng.choice([3.0, 5.0, 13.0])), seed * 1000 + i))
    return out


CASES = FIXED + _drawn()
IDS = ["N%d B%d %s %s dt%g %s%s seed%d" % (c.N, c.B, "reset" if c.auto_reset else "noreset", "norm" if c.normalize else "raw", c.dt,
                                           c.spawn, " keep" if c.keep_active else "", c.seed) for c in CASES]
STEPPING = ("step", "skip", "rollout")
SCORING = ("lookahead", "plan", "plan_sampled")


def _oracle_record(case):
    return S.Session(case, device=False, tree=True).run(S.make_tree_script(case))


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_plain_scripts_and_their_oracle_records_are_what_they_were():
    h = hashlib.sha256()
    for case in FIXED:
        script = S.make_script(case)
        s = S.Session(case, device=False)
        rec = s.run(script)
        h.update(repr(script).encode())
        h.update(repr([r.get("done", -1) for r in rec]).encode())
        for k in skip_ref.STATE:
            h.update(np.ascontiguousarray(getattr(s.orc, k)).tobytes())
    assert h.hexdigest() == PLAIN_DIGEST


def test_tree_scripts_contain_what_they_are_for():
    """Conditions on the INPUTS, on the oracle alone: over the fixed cases the tree scripts hold every interaction the sequence test
    exists for, and the GPU run cannot pass by comparing nothing — per scoring or branch operation every candidate has an evaluated env,
    per case at least half of all (candidate, env) pairs are evaluated.

    Evaluated / all (candidate, env) pairs of the scoring and branch operations of each fixed script, on the oracle (N: pairs):
        1: 39601 / 40596   2: 12742 / 13708   3: 9112 / 9834   8: 3237 / 3626   16: 1525 / 1702   33: 424 / 558   64: 338 / 414
    with the heading component wild in a fifth of the envs of a fresh action draw (session_ref.TREE_WILD_ENVS).  With the plain session's
    draw — a third of ALL heading components wild, each such target WIDE — an env of N aircraft is evaluated with probability 0.67^N after
    a fresh step: 4 % at N = 8, nothing from N = 16 on; hence the tree sessions' own draw."""
    seen = set()
    for case in FIXED:
        script = S.make_tree_script(case)
        assert len(script) == S.TREE_LENGTH and tuple(script[:len(S.TREE_PREAMBLE)]) == S.TREE_PREAMBLE
        rec = _oracle_record(case)
        on = "on" if case.auto_reset else "off"
        pairs = evaluated = 0
        shapes = []
        last_branch = None          # the record of the last branch into the child batch
        child_ops = set()           # what the children of the last branch with not-evaluated envs have been through since
        stash = None
        for i, r in enumerate(rec):
            op = r["op"]
            kind = op[0]
            prev = rec[i - 1] if i else None
            if kind in SCORING or kind == "branch":
                pairs, evaluated = pairs + r["pairs"], evaluated + r["evaluated"]
                assert min(r["evaluated_per_candidate"]) >= 1, (case, i, op)
            if kind in SCORING:
                assert 0 <= r["evaluated"] <= r["pairs"]
                shapes.append(r["shape"])
                if shapes.count(r["shape"]) >= 2 and len({s for s in shapes if s[0] == r["shape"][0]}) >= 2:
                    seen.add("a scoring shape (M, H, outputs) used twice and another one of the same call")
                nxt = rec[i + 1]["op"] if i + 1 < len(rec) else None
                if r["batch"] == "root" and prev["op"] == ("step", "held") and nxt == ("step", "held"):
                    seen.add("%s between two held steps" % kind)
                if prev["op"][0] == "skip" and prev.get("batch") == r["batch"] and prev["early"] > 0 and prev["ran_all"] > 0 and nxt == ("step", "held"):
                    seen.add("a scoring call directly after a step_skip with early and full envs, then a held step")
                if prev["op"][0] == "reset" and prev.get("batch") == r["batch"] and 0 < prev["selected"] < prev["of"] and r["t0_envs"] > 0 and nxt == ("step", "held"):
                    seen.add("a scoring call after a masked reset of some envs, then a held step")
                if r["early"] > 0:
                    seen.add("an episode ends inside a %s" % kind)
            if kind == "branch":
                last_branch, child_ops = r, set()
                nxt = rec[i + 1]["op"] if i + 1 < len(rec) else None
                if nxt == ("step", "branch", "child"):
                    assert r["not_evaluated"] == 0
                    if r["early"] > 0 and r["ran_all"] > 0:
                        seen.add("branch then a held step of the children with the branch's actions, early and full children, auto_reset %s" % on)
                if op[1] == "beam":
                    seen.add("a branch from the beam")
            if r.get("batch") == "child" and last_branch is not None:
                child_ops.add(kind if kind != "rollout" else ("rollout", op[2], op[3]))
                if last_branch["not_evaluated"] == 0 and child_ops >= {"skip", "reset", "observe", "traffic", ("rollout", 1, True),
                                                                         ("rollout", 4, False), ("rollout", 4, True), ("rollout", 1, False)}:
                    seen.add("children flown on: skip, rollout (hold 1 and 4, fast and full), masked reset, observe, traffic")
                if case.spawn == "random" and kind in STEPPING and r.get("hi_reset_episode", 0) >= 2:
                    seen.add("a child c >= B auto-reset under random entry at episode >= 2")
                if last_branch["not_evaluated"] > 0 and r.get("wide_envs", 0) > 0:
                    if op == ("step", "held", "child"):
                        seen.add("not-evaluated children (WIDE copies) take a held step with their source's actions")
                    if kind in ("observe", "traffic"):
                        seen.add("not-evaluated children (WIDE copies): %s" % kind)
                    if kind in ("skip", "rollout"):
                        seen.add("not-evaluated children (WIDE copies) flown on")
            if kind == "select":
                if op[3] in ("stash", "restore") and r["wide_selected"] > 0:
                    seen.add("select of WIDE rows, %s" % op[3])
                if r["hi_bit_clear_selected"] > 0:
                    seen.add("select, N = %d, of an env whose mask bit >= 32 was clear" % case.N)
                if op[3] == "stash":
                    stash = i
                if op[3] == "commit" and rec[i + 1]["op"] == ("step", "held"):
                    kinds = [x["op"][3] if x["op"][0] == "select" else x["op"][0] for x in rec[:i] if x["op"][0] in ("branch", "select")][-4:]
                    srcs = [x["op"][1] for x in rec[:i] if x["op"][0] == "branch"][-2:]
                    if kinds == ["branch", "beam", "branch", "beam"] and srcs == ["root", "beam"]:
                        seen.add("beam loop of two rounds, commit, the root holds the gathered actions")
                if op[3] == "edge" and r["out_of_range_under_mask"] == 3 and r["repeats"] > 0 and 0 < r["selected"] < r["of"]:
                    seen.add("select edges: repeated, -1, src.B and beyond-32-bit indices under a partial mask")
                if op[3] == "zero" and r["selected"] == 0:
                    seen.add("select under an all-zero mask")
                if op[3] == "beam" and r["repeats"] > 0:
                    seen.add("a beam with repeated children")
            if kind == "replay" and stash is not None and rec[i - 1]["op"][3] == "restore" and op[1] == stash + 1 and op[2] >= 6 and r["done"] > 0:
                seen.add("stash, fly on, restore, the same operations again")
        assert 2 * evaluated >= pairs, (case, evaluated, pairs)
    want = {"%s between two held steps" % k for k in SCORING} | {"an episode ends inside a %s" % k for k in SCORING} | {
        "a scoring call directly after a step_skip with early and full envs, then a held step",
        "a scoring call after a masked reset of some envs, then a held step",
        "a scoring shape (M, H, outputs) used twice and another one of the same call",
        "branch then a held step of the children with the branch's actions, early and full children, auto_reset on",
        "branch then a held step of the children with the branch's actions, early and full children, auto_reset off",
        "children flown on: skip, rollout (hold 1 and 4, fast and full), masked reset, observe, traffic",
        "a child c >= B auto-reset under random entry at episode >= 2",
        "not-evaluated children (WIDE copies) take a held step with their source's actions",
        "not-evaluated children (WIDE copies): observe", "not-evaluated children (WIDE copies): traffic",
        "not-evaluated children (WIDE copies) flown on",
        "select of WIDE rows, stash", "select of WIDE rows, restore",
        "select, N = 33, of an env whose mask bit >= 32 was clear", "select, N = 64, of an env whose mask bit >= 32 was clear",
        "a branch from the beam", "beam loop of two rounds, commit, the root holds the gathered actions", "a beam with repeated children",
        "stash, fly on, restore, the same operations again",
        "select edges: repeated, -1, src.B and beyond-32-bit indices under a partial mask", "select under an all-zero mask"}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("case", CASES[len(FIXED):], ids=IDS[len(FIXED):])
def test_drawn_tree_scripts_are_legal_on_the_oracle(case):
    """every drawn case's tree script runs through the legality rule on the oracle alone, something ends in it, and every scoring and
    branch operation has evaluated envs"""
    rec = _oracle_record(case)
    assert sum(r.get("done", 0) for r in rec) > 0
    assert all(min(r["evaluated_per_candidate"]) >= 1 for r in rec if "pairs" in r)


def test_the_session_refuses_a_held_step_a_child_cannot_take():
    case = FIXED[3]
    # a source with WIDE envs (wild heading targets): their children are byte copies, whose previous step is the SOURCE's — not the branch's
    s = S.Session(case, device=False, tree=True)
    s.run([("step", "fresh"), ("branch", "root", 5)])
    assert s.record[-1]["not_evaluated"] > 0
    with pytest.raises(S.IllegalScript, match="the actions differ"):
        s.apply(("step", "branch", "child"))
    assert len(s.done_ops) == 2, "the illegal step was not applied"
    s.run([("step", "held", "child"), ("step", "held", "child")])         # what they CAN hold: every env its own previous actions
    # a source that never stepped has not-evaluated children with no previous step at all; a tame source's children hold the branch's
    s = S.Session(case, device=False, tree=True)
    s.run([("set_state",), ("branch", "root", 2)])
    with pytest.raises(S.IllegalScript, match="no step"):
        s.apply(("step", "held", "child"))
    s = S.Session(case, device=False, tree=True)
    s.run([("step", "tame"), ("branch", "root", 5), ("step", "branch", "child"), ("select", "root", "child", "commit"), ("step", "held")])
    # a last-action record written in the source goes with the not-evaluated copies and with gathered envs
    s = S.Session(case, device=False, tree=True)
    s.run([("step", "fresh"), ("set_last_action",), ("select", "beam", "root", "stash")])
    with pytest.raises(S.IllegalScript, match="set_last_action"):
        s.apply(("step", "held", "beam"))
    # scoring calls change nothing about it; they and branch run on root or beam only; a plain session has no other batch
    s.run([("step", "repeat", "beam"), ("lookahead", 2, "fast", "beam"), ("plan", 2, 2, "all", "beam"), ("plan_sampled", 2, 2, True, "beam"),
           ("step", "held", "beam")])
    for bad in (("lookahead", 2, "fast", "child"), ("branch", "child", 2), ("select", "child", "root", "stash")):
        with pytest.raises(S.IllegalScript):
            s.apply(bad)
    with pytest.raises(S.IllegalScript, match="no batch"):
        S.Session(case, device=False).apply(("branch", "root", 2))
    # the rule itself, per env
    a = np.zeros((2, 3, 3), np.float32)
    b = a.copy()
    b[1, 2, 0] = -0.0
    assert S.held_is_legal(a, np.zeros(2, bool), a.copy(), np.ones(2, bool)) == (True, "")
    assert S.held_is_legal(a, False, b)[1].endswith("(env 1)") and not S.held_is_legal(a, np.array([False, True]), a)[0]
    assert not S.held_is_legal(a, False, a, np.array([True, False]))[0]


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tree_sequence_matches_oracle(case):
    import time
    from atc_hip import lib
    t0 = time.time()
    W = H.lane_width(case.N)
    counters = {"skip": lib.skip_launch_counts, "traffic": lib.traffic_launch_counts, "lookahead": lib.lookahead_launch_counts,
                "plan": lib.plan_launch_counts, "plan_sampled": lib.plan_sampled_launch_counts, "plan_draw": lib.plan_draw_launch_counts,
                "branch": lib.branch_launch_counts, "select": lib.select_launch_counts}
    was = {k: fn() for k, fn in counters.items()}
    with H.launches() as gained:
        s = S.Session(case, tree=True)
        s.run(S.make_tree_script(case))
        s.env.synchronize()
        s.close()
    grew = {k: {w: n - was[k].get(w, 0) for w, n in fn().items() if n != was[k].get(w, 0)} for k, fn in counters.items()}
    print("tree sequence %s: %.1f s, launches %s, %s" % (case, time.time() - t0, dict(sorted(gained.items())), grew))
    assert gained and all(name.startswith("%d/" % W) for name in gained), gained
    for k in ("skip", "lookahead", "plan", "plan_sampled", "branch"):      # counted per lane-group width: only the case's slot moved
        assert set(grew[k]) == {W}, (k, grew[k])
    assert set(grew["traffic"]) <= {W} and (case.N == 1) == (not grew["traffic"])
    assert grew["select"] and grew["plan_draw"], grew                       # (one slot each)
