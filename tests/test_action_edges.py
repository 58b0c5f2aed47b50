"""Non-finite and boundary ACTIONS on every kernel (tests/action_edges.py: the value table, the placement helper, the restated spec).

CPU (unmarked): the restated action stage of include/atc_step.h against the fp32 oracle for every table entry x component x action
space, held for 3 steps and then changed — flags, speed counts, altitude bits, exact heading counts, last_act, actions_taken and the
refusal penalty, all exact; every oracle output and state word finite; the placement helper's occurrence counts; the scripts the GPU
tests fly, on the oracle alone (their own conditions: a NaN altitude held, WIDE candidates present and at most a quarter).
GPU: the placed blocks through atc_step (fresh and held), atc_rollout, atc_rollout_hold, atc_step_skip, atc_lookahead,
atc_lookahead_plan and the single-env AtcGym, against the fp32 oracle through tests/bars.py / tests/skip_ref.py — no tolerance of its
own —, bars.check_state and a finiteness check after every call.

A NaN altitude action is REFUSED (include/atc_step.h "Non-finite actions").  Before that rule the kernels accepted it and their
held-step shortcut counted it once per block where the oracle counted it every step: test_flown_calls' held / hold / skip calls are
the ones that see it."""
import math

import numpy as np
import pytest

import action_edges as AE
import bars
import helpers as H
import session_ref
import skip_ref as R

NS = (1, 2, 3, 8, 16, 32, 33, 64)
FAR = H.FAR_A      # (20, 60) nm, 15 000 ft, 90 deg, 250 kt: inside LOWW, far above its floor


# ---------------------------------------------------------------------------------------------------------------- CPU
def _one_aircraft_oracle(B, discrete):
    from oracle import oracle as O
    comp = H.compiled("LOWW")
    orc = O.OracleEnv(comp, B, 1, O.make_params(dt=1.0, shaping=False, normalize=False, discrete=discrete), np.float32)
    for e in range(B):
        orc.set_state(e, 0, *FAR)
    return orc


def _hold(discrete):
    """the action that keeps FAR where it is (discrete: 250 kt, 15 000 ft, 90 deg as indices)"""
    return (15.0, 150.0, 90.0) if discrete else H.hold_action(FAR)


def _spec_state(orc, e):
    la = orc.last_act[e]
    lp = int(la[1]) if int(la[1]) not in (AE.I32_MIN, AE.I32_MAX) else int(orc.phi_wide[e, 1])
    return dict(v=int(np.uint32(orc.v_fix[e])), h=float(orc.h[e]), P=int(orc.phi_counts[e]), la_v=int(np.uint32(la[0])),
                la_h=float(la[2:4].copy().view(np.float64)[0]), la_P=lp, acts=int(orc.actions_taken[e]))


def _cases(discrete):
    return [(c, j) for c in range(3) for j in range(len(AE.table(discrete)[c]))]


@pytest.mark.parametrize("discrete", [False, True], ids=["continuous", "discrete"])
def test_restated_spec_agrees_with_the_fp32_oracle(discrete):
    tab, cases = AE.table(discrete), _cases(discrete)
    B = len(cases)
    orc = _one_aircraft_oracle(B, discrete)
    states = [_spec_state(orc, e) for e in range(B)]
    hold = _hold(discrete)
    seen = {"refused_v": 0, "refused_h": 0, "limit": 0, "wide": 0}
    for t in range(5):       # held for 3 steps, then changed (and the change held once)
        a = np.tile(np.array(hold, np.float32), (B, 1, 1))
        for e, (c, j) in enumerate(cases):
            a[e, 0, c] = tab[c][j].value if t < 3 else tab[c][j].follow
        orc.step(a)
        for e, (c, j) in enumerate(cases):
            st, tag = states[e], (tab[c][j].name, "component %d" % c, "step %d" % t)
            fl, pen = AE.spec_step(st, [float(x) for x in a[e, 0]], discrete)
            got = int(orc.flags[e, 0])
            assert got & ~(AE.F_INVALID_V | AE.F_INVALID_H | AE.F_PHI_LIMIT) == 0, ("an episode event in an action-stage case", tag, got)
            assert got == fl, ("flags", tag, got, fl)
            assert int(np.uint32(orc.v_fix[e])) == st["v"], ("speed counts", tag)
            assert np.float64(orc.h[e]).view(np.int64) == np.float64(st["h"]).view(np.int64), ("altitude bits", tag)
            assert int(orc.phi_counts[e]) == st["P"], ("heading counts", tag)
            ref = _spec_state(orc, e)
            assert (ref["la_v"], ref["la_P"]) == (st["la_v"], st["la_P"]), ("last_act speed / heading", tag)
            assert np.float64(ref["la_h"]).view(np.int64) == np.float64(st["la_h"]).view(np.int64), ("last_act altitude", tag)
            assert int(orc.last_act[e, 1]) == min(max(st["la_P"], AE.I32_MIN), AE.I32_MAX), ("last_act heading field", tag)
            assert ref["acts"] == st["acts"], ("actions_taken", tag, ref["acts"], st["acts"])
            want = np.float32(np.float32(-0.05) - np.float32(pen))
            assert np.float32(orc.ac_reward[e, 0]) == want, ("refusal penalty", tag, orc.ac_reward[e, 0], want)
            seen["refused_v"] += bool(fl & AE.F_INVALID_V)
            seen["refused_h"] += bool(fl & AE.F_INVALID_H)
            seen["limit"] += bool(fl & AE.F_PHI_LIMIT)
            seen["wide"] += not AE.I32_MIN < st["la_P"] < AE.I32_MAX
        # finite outputs and state, every entry, every step
        for name in ("obs", "raw_obs", "reward", "ac_reward", "h", "total_reward"):
            assert np.isfinite(getattr(orc, name)).all(), (name, "step %d" % t)
    assert all(v > 0 for v in seen.values()), seen


def test_the_table_holds_what_it_names():
    for discrete in (False, True):
        tab = AE.table(discrete)
        for c in range(3):
            names = [e.name for e in tab[c]]
            assert len(set(names)) == len(names)
            vals = [e.value for e in tab[c]]
            assert sum(math.isnan(v) for v in vals) == 3 and math.inf in vals and -math.inf in vals
            assert AE.FLT_MAX in vals and -AE.FLT_MAX in vals and AE.SUBNORMAL in vals and -AE.SUBNORMAL in vals
            assert any(v == 0 and math.copysign(1, v) < 0 for v in vals)
            assert all(AE.f32(v) == v or math.isnan(v) for e in tab[c] for v in (e.value, e.follow))
        by = {c: {e.name: e for e in tab[c]} for c in range(3)}
        sc = lambda n: AE.speed_counts(by[0][n].value, discrete)   # noqa: E731
        # (discrete: 100 kt is the action 0, its lower neighbour -2^-149 changes a float64 of 100 kt's magnitude by nothing: the ONE
        # rounding of the fma gives 100 kt again, accepted; the continuous -1 - 2^-23 decodes below 100 kt and is refused)
        assert sc("100 kt") == AE.V_MIN_FIX <= sc("100 kt +1 ulp") and (sc("100 kt -1 ulp") == AE.V_MIN_FIX if discrete else sc("100 kt -1 ulp") < AE.V_MIN_FIX)
        assert sc("300 kt") == AE.V_MAX_FIX and sc("300 kt +1 ulp") > AE.V_MAX_FIX >= sc("300 kt -1 ulp")
        assert sc("0 counts -1 ulp") == 0 and sc("2^32 counts") == 2 ** 32 - 1 and sc("2^32 counts +1 ulp") == 2 ** 32 - 1 > sc("2^32 counts -1 ulp") > AE.V_MAX_FIX
        at = lambda n: AE.altitude_target(by[1][n].value, discrete)   # noqa: E731
        assert at("0 ft") == 0.0 and at("0 ft -1 ulp") < 0.0 < at("0 ft +1 ulp")
        assert at("38000 ft") == 38000.0 and at("38000 ft -1 ulp") < 38000.0 < at("38000 ft +1 ulp")
        hc = lambda n: AE.heading_counts(by[2][n].value, discrete)   # noqa: E731
        assert hc("+2^31 counts -2 ulp")[0] < 2 ** 31 - 1 and by[2]["+2^31 counts"].wide and not by[2]["+2^31 counts -2 ulp"].wide
        assert hc("-2^31 counts +2 ulp")[0] > -2 ** 31 and by[2]["-2^31 counts"].wide and not by[2]["-2^31 counts +2 ulp"].wide
        assert hc("+2^52 counts +2 ulp") == (2 ** 52, True) and not hc("+2^52 counts -2 ulp")[1]
        assert hc("-2^52 counts -2 ulp") == (-2 ** 52, True) and not hc("-2^52 counts +2 ulp")[1]
        assert not by[2]["nan"].wide and hc("nan") == (0, False)
        for name, d in (("D-1", AE.DISCR_V - 1), ("D", AE.DISCR_V), ("-(D-1)", -(AE.DISCR_V - 1)), ("-D", -AE.DISCR_V)):
            e = by[0]["speed pair " + name]
            t1, t2 = AE.speed_counts(e.value, discrete), AE.speed_counts(e.follow, discrete)
            assert t2 - t1 == d and AE.V_MIN_FIX <= min(t1, t2) and max(t1, t2) <= AE.V_MAX_FIX, (name, t1, t2)
        for name, d in (("D-1", AE.DISCR_P - 1), ("D", AE.DISCR_P), ("-(D-1)", -(AE.DISCR_P - 1)), ("-D", -AE.DISCR_P)):
            e = by[2]["heading pair " + name]
            assert AE.heading_counts(e.follow, discrete)[0] - AE.heading_counts(e.value, discrete)[0] == d, name
        lo, hi = by[1]["altitude pair < 50 ft"], by[1]["altitude pair >= 50 ft"]
        assert abs(AE.altitude_target(lo.follow, discrete) - AE.altitude_target(lo.value, discrete)) < 50.0
        assert abs(AE.altitude_target(hi.follow, discrete) - AE.altitude_target(hi.value, discrete)) >= 50.0
        assert AE.bits(hi.follow) - AE.bits(lo.follow) in (1, -1)        # fp32 neighbours: either side of the threshold


@pytest.mark.parametrize("N", NS)
def test_placement_delivers_every_pair_everywhere(N):
    B = H.ragged(N)
    for discrete in (False, True):
        tab = AE.table(discrete)
        fam, in_free = AE.coverage(5, B, N, discrete, AE.n_values(discrete))
        assert in_free == 0
        for name, per_comp in fam.items():
            for c in range(3):
                assert (per_comp[c] >= 1).all(), (name, c, [tab[c][j].name for j in np.flatnonzero(per_comp[c] == 0)])
        p = AE.place(5, 0, B, N, discrete)
        assert (p.special[p.full_env] >= 0).all() and (p.special[0] >= 0).all() and (p.special[B - 1] >= 0).all()
        free = AE.free_envs(B, N)
        assert len(free) * H.lane_width(N) == 64 and (free[0] * H.lane_width(N)) % 64 == 0       # one whole wavefront
        ordinary = p.value[p.special < 0]
        assert np.isfinite(ordinary).all() and (np.abs(ordinary) <= (1.0 if not discrete else 380.0)).all()
        idx = p.special[..., 1]
        for e, k in zip(*np.nonzero(idx >= 0)):
            v, w = p.value[e, k, 1], tab[1][idx[e, k]].value
            assert AE.bits(float(v)) == AE.bits(w) or (math.isnan(v) and math.isnan(w))
        # restricted: WIDE heading values only where they are allowed
        q = AE.place(5, 0, B, N, discrete, wide_envs=[p.full_env])
        assert q.wide_env[q.full_env] and not np.delete(q.wide_env, q.full_env).any()


# ---------------------------------------------------------------------------------------------------------------- the scripts
def _setup(N, discrete, full, device):
    from oracle import oracle as O
    scn, comp = session_ref.setup(N)
    B = H.ragged(N)
    p = O.make_params(dt=1.0, discrete=discrete, auto_reset=True, random_entry=(N == 1), seed=9)
    orc = O.OracleEnv(comp, B, N, p, np.float32)
    env = None
    if device:
        from atc_hip.vec_env import AtcVecEnv
        from envs.atc import model
        env = AtcVecEnv(B, N, sim_parameters=model.SimParameters(1, discrete_action_space=discrete), scenario=scn, auto_reset=True,
                        spawn="random" if N == 1 else "lattice", seed=9, grid_cell=0.5, want_raw_obs=full, want_ac_reward=full,
                        want_min_sep=full, want_term_obs=full)
    return comp, B, orc, env


def _finite(env, orc, extra=()):
    """every output and state word: on the oracle, and on the device when there is one"""
    for name in ("obs", "reward", "h", "total_reward", "ep_return"):
        assert np.isfinite(getattr(orc, name)).all(), ("oracle", name)
    if env is None:
        return
    for name in ("obs", "reward", "raw_obs", "ac_reward", "min_sep", "term_obs", "h", "total_reward", "ep_return"):
        t = getattr(env, name)
        if t is not None:
            assert bool(env.torch.isfinite(t).all()), ("device", name)
    for name, t in extra:
        assert bool(env.torch.isfinite(t.float()).all()), ("device", name)


def _step_got(env, B, N, full):
    cpu = lambda t: t.cpu().numpy()   # noqa: E731
    got = {"flags": cpu(env.flags), "done": cpu(env.done), "obs": cpu(env.obs).reshape(B, N, 10), "reward": cpu(env.reward)}
    if full:
        got.update(raw_obs=cpu(env.raw_obs).reshape(B, N, 10), ac_reward=cpu(env.ac_reward), min_sep=cpu(env.min_sep),
                   term_obs=cpu(env.term_obs).reshape(B, N, 10))
    return got


def _nan_altitude_held(blocks):
    """aircraft-slots that carry a NaN altitude action in a block that is held"""
    return int(sum(np.isnan(b[..., 1]).sum() for b in blocks))


def _fly(N, discrete, full, device):
    """the flown calls of the issue's table on one env pair; returns the event record of the ORACLE side"""
    comp, B, orc, env = _setup(N, discrete, full, device)
    half = bars.half_range(comp)
    ev = {"held_nan_h": {}, "refused": 0, "limit": 0}
    try:
        blocks = iter(range(1000))
        P = lambda: AE.place(21, next(blocks) * 7, B, N, discrete)   # noqa: E731  (stride 7: the calls start at spread rotations)

        def after(tag):
            ev["refused"] += int((orc.flags & (H.F_INVALID_V | H.F_INVALID_H) != 0).sum())
            ev["limit"] += int((orc.flags & AE.F_PHI_LIMIT != 0).sum())
            if env is not None:
                try:
                    bars.check_state(env, orc)
                except AssertionError as e:
                    raise AssertionError("%s: state: %s" % (tag, e)) from e
            _finite(env, orc)

        def step(a, held, tag):
            orc.step(a)
            if env is not None:
                env.step(a, held=held)
                bars.check_step(_step_got(env, B, N, full), orc, True, half, tag)
            after(tag)

        # atc_step, no hint: 3 steps, the block redrawn each step (value, its follow-up, a new value)
        p = P()
        for t, a in enumerate((p.value, p.follow, P().value)):
            step(a, False, ("step", t))
        # atc_step with held=True: first step fresh, then 3 held
        p = P()
        ev["held_nan_h"]["held"] = _nan_altitude_held([p.value])
        step(p.value, False, ("held", 0))
        for t in range(1, 4):
            step(p.value, True, ("held", t))

        def rollout(a, hold, tag):
            T = a.shape[0] * hold
            out = None
            if env is not None:
                torch = env.torch
                names = [("obs", (B, N * 10), torch.float32), ("reward", (B,), torch.float32), ("done", (B,), torch.uint8),
                         ("flags", (B, N), torch.int16)]
                if full:
                    names += [("raw_obs", (B, N * 10), torch.float32), ("ac_reward", (B, N), torch.float32), ("min_sep", (B,), torch.float32),
                              ("term_obs", (B, N * 10), torch.float32)]
                bufs = {k: torch.zeros((T,) + s, dtype=d, device=env.device) for k, s, d in names}
                res = env.rollout(torch.as_tensor(a), out=bufs, hold=hold)
                out = {k: v.cpu().numpy() for k, v in res.items()}
                for k, v in res.items():
                    if v.dtype == torch.float32 and k != "term_obs":
                        assert bool(torch.isfinite(v).all()), (tag, k)
            term_before = orc.term_obs.copy()   # (a rollout's terminal observations go to its own [T, ...] buffers, not to the env's)
            for t in range(T):
                orc.step(a[t // hold])
                ev["refused"] += int((orc.flags & (H.F_INVALID_V | H.F_INVALID_H) != 0).sum()) if t < T - 1 else 0
                if out is not None:
                    got = {"flags": out["flags"][t], "done": out["done"][t], "obs": out["obs"][t].reshape(B, N, 10), "reward": out["reward"][t]}
                    if full:
                        got.update(raw_obs=out["raw_obs"][t].reshape(B, N, 10), ac_reward=out["ac_reward"][t], min_sep=out["min_sep"][t],
                                   term_obs=out["term_obs"][t].reshape(B, N, 10))
                    bars.check_step(got, orc, True, half, (tag, t))
            orc.term_obs[...] = term_before
            after(tag)

        # atc_rollout, T = 4
        p, q = P(), P()
        rollout(np.stack([p.value, p.follow, q.value, q.follow]), 1, "rollout")
        # atc_rollout_hold, T = 6, hold = 3
        p = P()
        ev["held_nan_h"]["rollout_hold"] = _nan_altitude_held([p.value])
        rollout(np.stack([p.value, p.follow]), 3, "rollout_hold")
        # atc_step_skip, K = 4
        p = P()
        ev["held_nan_h"]["skip"] = _nan_altitude_held([p.value])
        ref = R.skip_reference(orc, p.value, 4)
        if env is not None:
            env.step_skip(p.value, 4)
            got = _step_got(env, B, N, full)
            got["n_steps"] = env.frame_steps.cpu().numpy()
            bars.check_skip_outputs(got, ref, half, full, "skip")
        after("skip")
        # ... and one plain step on what they left
        step(P().follow, False, ("closing step", 0))
    finally:
        if env is not None:
            env.close()
    return ev


LOOK = dict(M=3, K=4)
PLAN = dict(M=2, H=2, K=3)


def _look(N, discrete, full, device):
    """atc_lookahead (mappings 0 / 1 / M) and atc_lookahead_plan from the reset state, candidates from the placement cycle with the WIDE
    heading values confined to two envs; returns the oracle-side record"""
    comp, B, orc, env = _setup(N, discrete, full, device)
    half = bars.half_range(comp)
    rec = {}
    try:
        probe = AE.place(33, 0, B, N, discrete)
        wide_envs = [probe.full_env, B - 1]
        assert len(wide_envs) * 4 <= B
        ok0 = ~R.wide_envs(orc)
        assert ok0.all()
        if env is not None:
            from atc_hip import lib
            snap = H.snapshot(env)
        for kernel, c in (("lookahead", LOOK), ("plan", PLAN)):
            M, K, Hn = c["M"], c["K"], c.get("H")
            pl = [AE.place(33, 11 * i + (0 if Hn is None else 5), B, N, discrete, wide_envs) for i in range(M * (Hn or 1))]
            # a look-ahead candidate is ONE held decision: the values; a plan's second segment changes every table value to its follow-up
            cand = np.stack([p.value for p in pl]) if Hn is None else \
                np.stack([np.stack([pl[m * Hn].value] + [pl[m * Hn + h].follow if h % 2 else pl[m * Hn + h].value for h in range(1, Hn)])
                          for m in range(M)])
            records = [] if Hn is not None else None
            refs = R.candidate_references(orc, cand, K) if Hn is None else R.plan_references(orc, cand, K, records)
            # which (candidate, env) pairs are not evaluated: a heading target beyond the 32-bit field in an executed step
            wide_pair = np.zeros((M, B), bool)
            for m in range(M):
                acts = cand[m][None] if Hn is None else cand[m]
                alive = np.ones(B, bool)
                for h in range(acts.shape[0]):
                    w = np.array([[AE.is_wide_target(float(a), discrete) for a in row] for row in acts[h][..., 2]]).any(axis=1)
                    wide_pair[m] |= alive & w
                    if records is not None:
                        alive = alive & ~records[m][h][1]["done"].astype(bool)
            n_wide = int(wide_pair.sum())
            assert 1 <= n_wide and 4 * n_wide <= M * B, (kernel, n_wide, M * B)
            rec[kernel] = (n_wide, M * B, int(sum(np.isnan(cand[..., 1][m][..., ~wide_pair[m], :]).sum() for m in range(M))))
            if env is None:
                continue
            outputs = (("flags", "min_sep", "ac_reward", "obs") if full else ()) + (("seg_reward",) if Hn is not None and full else ())
            for mapping in ((0, 1, M) if Hn is None else (0,)):
                lib.lookahead_set_mapping(mapping)
                try:
                    at = env.torch.as_tensor(cand, device=env.device)
                    res = env.lookahead(at, K, outputs=outputs) if Hn is None else env.lookahead_plan(at, K, outputs=outputs)
                finally:
                    lib.lookahead_set_mapping(0)
                got = {k: v.cpu().numpy() for k, v in res.items()}
                for m in range(M):
                    ok = ~wide_pair[m]
                    g = {k: v[m] for k, v in got.items()}
                    tag = (kernel, "mapping %d" % mapping, "candidate %d" % m)
                    bars.check_candidate_outputs({k: v for k, v in g.items() if k != "seg_reward"}, refs[m], ok, half, tag=tag)
                    if "seg_reward" in g:
                        bars.check_plan_segments(g["seg_reward"], refs[m], ok, K, tag=tag)
                    # the header's contract for a pair that is not evaluated, directly: n_steps == 0 and every returned word zero
                    assert not g["n_steps"][~ok].any() and not g["done"][~ok].any() and not g["reward"][~ok].view(np.uint32).any(), tag
                    for k, v in g.items():
                        rows = v.T[~ok] if k == "seg_reward" else v[~ok]
                        assert not np.ascontiguousarray(rows).view(np.uint8).any(), (k, tag)
                    assert (g["n_steps"][ok] > 0).all(), tag
                H.bytes_equal(env, snap)
                bars.check_state(env, orc)
                _finite(env, orc, extra=[(k, v) for k, v in res.items()])
    finally:
        if env is not None:
            env.close()
    return rec


_FORMS = [pytest.param(N, d, f, id="N%d-%s-%s" % (N, "discrete" if d else "continuous", "full" if f else "fast"))
          for N in NS for d in (False, True) for f in (False, True)]


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("discrete", [False, True], ids=["continuous", "discrete"])
def test_scripts_hold_their_own_conditions(N, discrete):
    """the GPU tests' scripts on the oracle alone: a NaN altitude is held in EACH of the held / hold / skip calls, targets are refused and clamped;
    WIDE candidate pairs exist and are at most a quarter (asserted inside _look), NaN altitudes take part in evaluated pairs"""
    ev = _fly(N, discrete, False, device=False)
    assert set(ev["held_nan_h"]) == {"held", "rollout_hold", "skip"} and all(n > 0 for n in ev["held_nan_h"].values()), ev
    assert ev["refused"] > 0 and ev["limit"] > 0, ev
    rec = _look(N, discrete, False, device=False)
    for kernel in ("lookahead", "plan"):
        assert rec[kernel][2] > 0, (kernel, rec)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("N,discrete,full", _FORMS)
def test_flown_calls(N, discrete, full):
    _fly(N, discrete, full, device=True)


@pytest.mark.gpu
@pytest.mark.parametrize("N,discrete,full", _FORMS)
def test_lookahead_calls(N, discrete, full):
    _look(N, discrete, full, device=True)


@pytest.mark.gpu
@pytest.mark.parametrize("persistent", [True, False], ids=["server", "packet"])
@pytest.mark.parametrize("discrete", [False, True], ids=["continuous", "discrete"])
def test_single_env_gym(discrete, persistent, monkeypatch, capsys):
    """Every table entry through the drop-in AtcGym (N = 1), held twice and then changed, against a one-env oracle: bars.check_step on
    every step, bars.check_state and finiteness of the device state after every entry.  persistent=True with the tight-loop window
    widened (as tests/test_dropin_boundary.py does: the oracle's step between two env steps is longer than 50 us) steps through the
    resident step server — asserted: the env is serving after at least two thirds of the steps, the share that file asks of a served
    run —, persistent=False through atc_step_packet alone."""
    from envs.atc import atc_gym, model, scenarios
    from oracle import oracle as O
    monkeypatch.setattr(atc_gym, "_TIGHT_GAP_S", 1.0)
    g = atc_gym.AtcGym(model.SimParameters(1, discrete_action_space=discrete), scenarios.LOWW(), persistent=persistent)
    comp = scenarios.compile_scenario(scenarios.LOWW())
    o1 = O.OracleEnv(comp, 1, 1, O.make_params(discrete=discrete, keep_active=True), np.float32)
    half = bars.half_range(comp)
    fetched = []
    fetch = g._launch_and_fetch
    g._launch_and_fetch = lambda: fetched.append(fetch()) or fetched[-1]     # (the step's flag word is not in what step() returns)
    n_served = n_steps = 0
    try:
        assert g._persistent == persistent
        o1.reset()      # (AtcGym.__init__ resets once more after its backend's first reset: atc_gym.py:60-61)
        bars.check_state(g._vec, o1)
        tab = AE.table(discrete)
        hold = (10.0, 120.0, 45.0) if discrete else (0.5, -0.2, -0.5)
        for c in range(3):
            for e in tab[c]:
                for t in range(3):
                    a = np.array(hold, np.float32)
                    a[c] = e.value if t < 2 else e.follow
                    s, r, d, info = g.step(a)
                    o1.step(a)
                    n_served, n_steps = n_served + bool(g._serving), n_steps + 1
                    tag = (e.name, c, t)
                    obs, raw, rew, dn, flags, timesteps, acts = fetched[-1]
                    assert np.isfinite(s).all() and np.isfinite(info["original_state"]).all() and np.isfinite(r), tag
                    got = {"flags": np.array([[flags]], np.uint16), "done": np.array([d], np.uint8), "obs": np.asarray(s).reshape(1, 1, 10),
                           "reward": np.array([r], np.float32)}
                    bars.check_step(got, o1, True, half, tag)
                    assert np.all(np.abs(info["original_state"] - o1.raw_obs[0, 0]) <= 1e-5 * half), tag      # (bars.check_step's raw bar)
                    assert (acts, timesteps) == (int(o1.actions_taken[0]), int(o1.timesteps[0])) == (g.actions_taken, g.timesteps), tag
                    if d:
                        g.reset()
                        o1.reset()
                vec = g._vec          # (settles: stops the server; the next step starts it again)
                bars.check_state(vec, o1)
                assert np.isfinite(vec.h.cpu().numpy()).all() and np.isfinite(vec.total_reward.cpu().numpy()).all(), e.name
        assert n_served * 3 >= n_steps * 2 if persistent else n_served == 0, (n_served, n_steps)
    finally:
        g.close()
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------------------------- g15: the reference
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_reference_fixture_of_the_finite_entries_and_inf_heading(dtype):
    """tests/golden/g15_action_edges.npz (recorded from the reference by tests/golden/generate_golden.py: every finite table entry and a
    +-Inf heading, held 3 steps, then changed) through both oracles at the bars of tests/test_oracle_golden.py.  The +-Inf-heading
    episodes pin what include/atc_step.h states: the fp32 path clamps the target (ATC_F_PHI_LIMIT on those steps, a flag the reference
    does not have) and counts the held target ONCE where the reference — abs(inf - inf) is NaN — counts it in every step; nothing else
    differs.  The float64 oracle is the reference as it is and counts like it."""
    from test_oracle_golden import OracleAdapter, _check_factory
    npz = H.golden_npz("g15_action_edges.npz")
    eps = H.episodes_of(npz)
    names = {(ep["discrete"], ep["component"], ep["edge"]) for ep in eps}
    for discrete in (False, True):     # the fixture is the table: every entry the reference can run, nothing else
        want = {(discrete, c, e.name) for c in range(3) for e in AE.table(discrete)[c]
                if math.isfinite(e.value) or (c == 2 and math.isinf(e.value))}
        assert want == {n for n in names if n[0] == discrete}
    stats = {"steps": 0}
    ad = OracleAdapter(dtype)
    pinned, edge_rows = 0, set()
    for ep in eps:
        check = _check_factory(npz, dtype, stats, ep)
        if ep["component"] == 2 and dtype == np.float32:
            def check(t, row, rec, inner=check, ep=ep):
                nonlocal pinned
                # ATC_F_PHI_LIMIT (a flag the reference does not have) exactly on the steps whose target lies beyond +-2^52 counts
                limit = AE.heading_counts(float(np.float32(npz["action"][row][2])), ep["discrete"])[1]
                assert bool(rec.flags & AE.F_PHI_LIMIT) == limit, (ep["edge"], t)
                rec.flags &= ~AE.F_PHI_LIMIT
                if ep["inf_heading"]:
                    assert limit == (t < 3)
                    assert rec.actions_taken == int(npz["actions_taken"][row]) - min(t, 2), (ep["edge"], t, rec.actions_taken)
                    rec.actions_taken = int(npz["actions_taken"][row])
                    pinned += 1
                inner(t, row, rec)
        if " pair " in ep["edge"] and ep["component"] != 1 and dtype == np.float32:
            # The discriminator pairs are built D-1 / D COUNTS apart (and D from the initial last_action).  Targets are truncated to counts
            # (include/atc_step.h): each truncation takes less than a count off, so a float64 difference just below the threshold can be
            # exactly D counts — counted here, not by the reference.  Only on such a step may the fp32 path be one action ahead; which
            # way IT decides is pinned exactly by test_restated_spec_agrees_with_the_fp32_oracle.
            c = ep["component"]
            D = (AE.DISCR_V, None, AE.DISCR_P)[c]
            fn = (lambda a, d=ep["discrete"]: AE.speed_counts(a, d)) if c == 0 else (lambda a, d=ep["discrete"]: AE.heading_counts(a, d)[0])
            track = {"prev": 0 if c == 0 else -180 * AE.Q, "ahead": 0}

            def check(t, row, rec, inner=check, ep=ep, fn=fn, D=D, track=track):
                tgt = fn(float(np.float32(npz["action"][row][ep["component"]])))
                ahead = rec.actions_taken - int(npz["actions_taken"][row])
                assert ahead - track["ahead"] in ((0, 1) if abs(tgt - track["prev"]) == D else (0,)), (ep["edge"], t, ahead)
                if ahead != track["ahead"]:
                    edge_rows.add((ep["discrete"], ep["edge"]))
                track.update(prev=tgt, ahead=ahead)
                rec.actions_taken = int(npz["actions_taken"][row])
                inner(t, row, rec)
        H.replay_episode(ad, npz, ep, check)
    assert stats["steps"] == len(npz["reward"]) and len(npz["reward"]) < 1000
    assert pinned == (16 if dtype == np.float32 else 0)
    # the episodes that hold "exactly D counts apart, below the reference's threshold in float64" (include/atc_step.h says g15 holds them)
    want_edges = {(False, "heading pair D"), (False, "heading pair -D"), (True, "speed pair D"), (True, "speed pair -D"),
                  (True, "heading pair -(D-1)"), (True, "heading pair D"), (True, "heading pair -D")}
    assert edge_rows == (want_edges if dtype == np.float32 else set()), sorted(edge_rows)
