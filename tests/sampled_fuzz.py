"""What the sweeps over the drawn-plan calls share (tests/test_fuzz_plan_sampled.py, tests/test_fuzz_planner.py): the first CASES cases
of tests/held_fuzz.py, flown as held_fuzz._fly flies them up to its plan call, and the numpy-drawn plans of that call flown on the oracle.
TEST INFRASTRUCTURE ONLY; importing it needs no GPU."""
import numpy as np

import bars
import held_fuzz as F
import helpers as H
import plan_draw_ref as P
import skip_ref as R

SEED0, CASES = 5000, 30
STD = 0.3


def inputs(seed):
    """(scn, comp, kw, rng) of a case: held_fuzz.case, and the random stream held_fuzz._fly draws the calls' actions from"""
    scn, comp, kw = F.case(seed)
    return scn, comp, kw, np.random.default_rng([kw["seed"], 0x464C59])


def fly_to_the_plan(env, orc, kw, rng, whole=False):
    """held_fuzz._fly up to its plan call, draw for draw: the flown calls on the oracle (and the env), auto-reset switched off where the
    case says so, the look-ahead's candidates drawn and dropped.  Returns (mean [H, B, N, 3] = the case's first plan, auto_reset); with
    whole=True all of the case's plans [M, H, B, N, 3] in the place of the first."""
    B, N, discrete, wild = kw["B"], kw["N"], kw["discrete"], kw["wild"]
    for K in kw["flown"]:
        a = F.draw_flown(rng, B, N, discrete, wild)
        R.skip_reference(orc, a, K)
        if env is not None:
            env.step_skip(a, K)
    auto_reset = not kw["auto_reset_off"]
    if not auto_reset:
        from oracle import oracle as O
        orc.params.mode &= ~O.M_AUTO_RESET
        if env is not None:
            H.set_auto_reset(env, False)
    if env is not None:
        bars.check_state(env, orc)
    F.draw_candidates(rng, (kw["lookahead"]["M"], B, N), discrete, wild)
    c = kw["plan"]
    cand = F.draw_candidates(rng, (c["M"], c["H"], B, N), discrete, wild)
    return (cand if whole else cand[0]), auto_reset


def key(kw):
    return dict(seed=kw["seed"], iteration=0, mean_first=True)


def oracle_side(orc, kw, mean, auto_reset, std=STD):
    """the numpy-drawn plans flown on the oracle (left as it was): (refs, ok [B], events, pairs not evaluated, pairs)"""
    c = kw["plan"]
    M, Hn, K = c["M"], c["H"], c["K"]
    plans = P.draw(mean, std, M, **key(kw))
    ok = ~R.wide_envs(orc)
    records = []
    refs = R.plan_references(orc, plans, K, records)
    ev = F._new_events()
    n = np.stack([r["n_steps"].astype(int) for r in refs])[:, ok]
    done = np.stack([r["done"].astype(bool) for r in refs])[:, ok]
    F._add_n(ev, n, done, K * Hn)
    if n.size:
        ev["differ"] += int((n.min(0) != n.max(0)).sum())
    for m in range(M):
        for alive, r in records[m]:
            F._add_block(ev, r, K, ok & alive, auto_reset)
    late = done & (n > K)
    ev["late_stop"] += int(late.sum())
    ev["late_reset"] += int(late.sum()) if auto_reset else 0
    return refs, ok, ev, M * int((~ok).sum()), M * kw["B"]
