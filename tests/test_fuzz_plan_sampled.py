"""The drawn-plan call (atc_lookahead_plan_sampled, k_plan_sampled) held directly to the fp32 oracle over the mode space of the held
sweep: the first CASES cases of tests/held_fuzz.py, drawn as it draws them (sector, lookup grid, timestep, shaping, normalisation,
separation minimum, keep_active, time limits that end episodes inside held blocks, wild flown actions, auto-reset switched off after
flying).  The case's flown step_skip calls are flown on both sides; its plan call is then flown as the SAMPLED call — mean = the case's
first plan, std = 0.3, the case's M, H, K, outputs and mapping — and compared with tests/skip_ref.py::plan_references on the oracle, fed
the numpy-drawn plans of tests/plan_draw_ref.py.  Every comparison is one of tests/bars.py.  Cases with discrete actions assert the
refusal instead.

A condition, not a measurement: at most 1 % of the sweep's (candidate, env) pairs may have n_steps == 0 (not evaluated: a WIDE heading
at the start of the call — drawn actions lie in [-1, 1] and make none).  The CPU twin flies the same cases on the oracle alone and asserts
that the oracle stays under the cap and that the cases hold early stops, resets inside a segment and conflicts.

On the oracle, CASES = 30: 17 cases are flown (13 have discrete actions and are refused), every lane-group width among them; 9 of their
1 829 pairs are not evaluated (0.49 %); they hold 1 031 early stops, 41 envs whose plans stop at different n_steps, 629 resets inside a
segment, 496 conflicts and 196 plans that end in a segment h >= 1."""
import functools

import numpy as np
import pytest

import bars
import held_fuzz as F
import helpers as H
from fuzz_space import make_env, make_oracle
from sampled_fuzz import CASES, SEED0, STD          # (the case's flying and its oracle side: tests/sampled_fuzz.py)
from sampled_fuzz import fly_to_the_plan as _fly_to_the_plan
from sampled_fuzz import inputs as _inputs
from sampled_fuzz import key as _key
from sampled_fuzz import oracle_side as _oracle_side

CAP = 0.01
EVENTS = ("early", "differ", "reset_in_block", "conflict", "late_stop", "late_reset")


@functools.lru_cache(maxsize=None)
def _oracle_record(seed):
    scn, comp, kw, rng = _inputs(seed)
    if kw["discrete"]:
        return None
    orc = make_oracle(comp, kw, auto_reset=True)
    mean, auto_reset = _fly_to_the_plan(None, orc, kw, rng)
    _, _, ev, left_out, pairs = _oracle_side(orc, kw, mean, auto_reset)
    return ev, left_out, pairs


def test_sweep_contains_what_it_is_for_on_the_oracle():
    recs = [r for r in (_oracle_record(SEED0 + i) for i in range(CASES)) if r is not None]
    assert 0 < len(recs) < CASES, "the sweep needs drawn cases and refused (discrete) ones"
    left_out, pairs = sum(r[1] for r in recs), sum(r[2] for r in recs)
    total = {n: sum(r[0][n] for r in recs) for n in EVENTS}
    print("cases flown %d of %d; pairs not evaluated %d of %d; events %s" % (len(recs), CASES, left_out, pairs, total))
    assert left_out <= CAP * pairs, (left_out, pairs)
    assert all(total.values()), total
    assert {H.lane_width(F.case(SEED0 + i)[2]["N"]) for i in range(CASES) if _oracle_record(SEED0 + i)} == set(F.WIDTHS)


_device_pairs = {}      # seed -> (pairs with n_steps == 0, pairs) of the cases flown on the device so far


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [SEED0 + i for i in range(CASES)])
def test_sampled_plan_matches_oracle(seed):
    import torch
    from atc_hip import lib
    scn, comp, kw, rng = _inputs(seed)
    c = kw["plan"]
    M, Hn, K, B, N = c["M"], c["H"], c["K"], kw["B"], kw["N"]
    print("sampled fuzz case", seed, type(scn).__name__, kw)
    env = make_env(scn, kw, auto_reset=True)
    try:
        if kw["discrete"]:      # only the continuous action space is drawn: both calls refuse, no launch record moves
            before = (lib.plan_sampled_launch_counts(), lib.plan_draw_launch_counts())
            mean = torch.zeros((Hn, B, N, 3), device=env.device)
            with pytest.raises(ValueError):
                env.lookahead_plan_sampled(mean, STD, K, M)
            with pytest.raises(ValueError):
                env.draw_plans(mean, STD, M)
            assert (lib.plan_sampled_launch_counts(), lib.plan_draw_launch_counts()) == before
            return
        orc = make_oracle(comp, kw, auto_reset=True)
        mean, auto_reset = _fly_to_the_plan(env, orc, kw, rng)
        refs, ok, _, _, pairs = _oracle_side(orc, kw, mean, auto_reset)
        snap = H.snapshot(env)
        before = lib.plan_sampled_launch_counts()
        lib.lookahead_set_mapping(c["mapping"])
        res = env.lookahead_plan_sampled(torch.as_tensor(mean, device=env.device), STD, K, M, outputs=c["outputs"], **_key(kw))
        lib.lookahead_set_mapping(0)
        assert set(res) == {"reward", "done", "n_steps"} | set(c["outputs"])
        got = {k: v.cpu().numpy() for k, v in res.items()}
        now = lib.plan_sampled_launch_counts()
        assert {w: n - before.get(w, 0) for w, n in now.items() if n != before.get(w, 0)} == {H.lane_width(N): 1}
        half = bars.half_range(comp)
        for m in range(M):
            g = {k: v[m] for k, v in got.items()}
            bars.check_candidate_outputs({k: v for k, v in g.items() if k != "seg_reward"}, refs[m], ok, half, tag=("sampled", seed, m))
            if "seg_reward" in g:
                bars.check_plan_segments(g["seg_reward"], refs[m], ok, K, tag=("sampled", seed, m))
        H.bytes_equal(env, snap)
        bars.check_state(env, orc)
        zero = int((got["n_steps"] == 0).sum())
        assert zero == M * int((~ok).sum()), "n_steps == 0 exactly for the envs that are WIDE at the start"
        _device_pairs[seed] = (zero, pairs)
    finally:
        lib.lookahead_set_mapping(0)
        env.close()


@pytest.mark.gpu
def test_device_sweep_stays_under_the_cap():
    """the cap over the sweep the cases above flew on the device (this module's tests run in order, in one process)"""
    flown = [SEED0 + i for i in range(CASES) if not F.case(SEED0 + i)[2]["discrete"]]
    assert sorted(_device_pairs) == flown, "run the module's sweep as a whole: the cap is the sweep's"
    zeros, total = (sum(v[i] for v in _device_pairs.values()) for i in (0, 1))
    print("sampled fuzz: pairs with n_steps == 0 on the device: %d of %d" % (zeros, total))
    assert zeros <= CAP * total, (zeros, total)
