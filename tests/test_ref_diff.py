"""The second link of the parity chain: the fp32 spec — and the kernels — against the float64, reference-faithful oracle over the fuzz's
mode space (tests/ref_diff.py draws, flies and compares; its docstring holds the bars, the tie rules and the word-9 rule).

CPU  ATC_REF_FUZZ_CASES cases (default 200) from seed ATC_REF_FUZZ_SEED (default 1000) on, both oracle instantiations in lock-step, each
     case's first 200 steps (python tests/ref_diff.py SEED0 CASES flies whole cases: profiles/ref_diff_sweep.txt).  No env of the default
     sweep may need a tie rule; at most one word-9 row per 50 000 env-steps may sit on the other side of the +-180 deg wrap; the sweep must
     contain what it is for.  Random actions never reach the corridor, so wins and hand-overs come from the ten hand-placed one-step
     situations of helpers.extension_known_answers, flown through the same comparator.  The two wrap ties the first sweep met (seeds 1067
     and 1199) and the wrap itself, headings placed ulps either side of the runway's reciprocal on two sectors, are pinned.
     The held references: tests/skip_ref.py's references of step_skip, lookahead and lookahead_plan built on the float64 oracle against the
     ones built on the fp32 oracle, on held_fuzz's 60 default configurations (ref_diff.fly_held).
GPU  40 drawn cases against the float64 oracle DIRECTLY, and against the fp32 oracle by tests/bars.py so that a failure names the link that
     broke: ATC_REF_GPU_CASES (default 28; ref_diff.gpu_case) of atc_step fast and full, atc_rollout, atc_rollout_hold at N = 1, 3, 16, 17,
     64, and ATC_REF_GPU_HELD (default 12; held_fuzz.case from seed 5000) of atc_step_skip, atc_lookahead and atc_lookahead_plan.  Integer
     words exact under the tie rules; the tie and wrap caps are asserted over the cases together.
tests/fuzz_debug.py --ref <seed> replays one CPU case and prints the first deviation."""
import functools
import os

import numpy as np
import pytest

import helpers as H
import ref_diff as D

SEED0 = int(os.environ.get("ATC_REF_FUZZ_SEED", "1000"))
CASES = int(os.environ.get("ATC_REF_FUZZ_CASES", "200"))
GPU_CASES = int(os.environ.get("ATC_REF_GPU_CASES", "28"))
GPU_HELD = int(os.environ.get("ATC_REF_GPU_HELD", "12"))
HELD_SEEDS = range(5000, 5060)
DEFAULT_SEEDS = range(1000, 1200)
SWEEP_STEPS = 200
WRAP_CAP = 1.0 / 50000          # word-9 rows on the other side of the wrap per env-step
PROPERTIES = ("LOWW", "LOWW_random", "SimpleScenario", "LOWWDense", "N=1", "N>16", "discrete", "continuous", "shaping off", "normalisation off",
              "sep_nm 0", "sep_nm 3", "sep_nm 5", "keep_active", "random entry", "non-dyadic dt", "out-of-space actions", "40-step limit",
              "no reset", "held actions") + tuple("grid " + g for g in ("None", "0.25", "0.5", "1.0", "0.125", "0.0625", "auto"))


@functools.lru_cache(maxsize=None)
def _record(seed):
    return D.fly(seed, max_steps=SWEEP_STEPS)


@pytest.mark.parametrize("seed", [SEED0 + i for i in range(CASES)])
def test_fp32_spec_follows_the_float64_oracle(seed):
    rec = _record(seed)
    assert rec["env_steps"] > 0
    assert not rec["excluded"], ("an env of the default sweep needed a tie rule", rec["ties"])


# ---------------------------------------------------------------------------------------------------------------- hand-placed situations
def _placed(name, params, t0, aircraft, dtype_pair=(np.float64, np.float32)):
    from oracle import oracle as O
    comp = H.compiled("LOWW")
    envs = []
    for dtype in dtype_pair:
        p = O.make_params(shaping=False, timestep_limit=params.get("timestep_limit", 6000), conflict_reward=params.get("conflict_reward", -200.0))
        env = O.OracleEnv(comp, 1, len(aircraft), p, dtype)
        env.timesteps[0] = t0
        for k, (state, _) in enumerate(aircraft):
            env.set_state(0, k, *state)
        envs.append(env)
    return comp, envs


@functools.lru_cache(maxsize=None)
def _placed_record():
    total = D.new_record()
    for name, params, t0, aircraft, exp in H.extension_known_answers():
        comp, (ref, spec) = _placed(name, params, t0, tuple(aircraft))
        cmp_ = D.Comparator(ref, comp, True, tag=name)
        act = np.array([a for _, a in aircraft], np.float32)[None]
        ref.step(act.astype(np.float64))
        spec.step(act)
        assert ref.flags[0].tolist() == exp["flags"] and bool(ref.done[0]) == exp["done"] and int(ref.active_mask[0]) == exp["mask_after"], name
        cmp_.step(D.outputs_of(spec), 0)
        cmp_.state(D.state_of(spec), 0)
        cmp_.rec["cases"] = 1
        D.merge(total, cmp_.rec)
    return total


def test_hand_placed_situations_through_the_comparator():
    """helpers.extension_known_answers — wins, a hand-over, conflicts, a below-MVA, an outside, time-outs, refusals, each ONE step from a
    placed state — in both instantiations: the float64 side gives the hand-computed flags, the fp32 spec follows it at the comparator's bars"""
    rec = _placed_record()
    assert not rec["excluded"] and rec["flags"]["won"] >= 5 and rec["handovers"] >= 2, rec


def test_default_sweep_contains_what_it_is_for():
    total = D.new_record()
    for seed in DEFAULT_SEEDS:
        D.merge(total, _record(seed))
    print("\n".join(D.report(total)))
    missing = [p for p in PROPERTIES if p not in total["props"]]
    assert not missing, missing
    assert not total["excluded"] and total["excluded_steps"] == 0, total["ties"]
    assert total["wrap9"] <= WRAP_CAP * total["env_steps"], (total["wrap9"], total["env_steps"])
    for name in ("below_mva", "timeout", "conflict", "outside"):
        assert total["flags"][name] > 0, name
    assert total["refused"] > 0 and total["resets"] > 0 and total["done"] > total["resets"]
    # random actions do not fly an approach: the wins and the hand-overs of the differential are the hand-placed ones
    placed = _placed_record()
    assert placed["flags"]["won"] >= 5 and placed["handovers"] >= 2, placed["flags"]


# ---------------------------------------------------------------------------------------------------------------- word 9 at the wrap
@pytest.mark.parametrize("seed,step,env,aircraft", [(1067, 33, 16, None), (1199, 37, 22, 9)])
def test_wrap_tie_of_the_first_sweep(seed, step, env, aircraft):
    """The two rows of the first sweep whose word 9 read +180 in the float64 instantiation and -180 in the fp32 spec: the float64 heading
    is a rounding BELOW the runway's reciprocal (159.99999999999997 deg for 340), where relative_angle gives 179.99999999999997 -> +180;
    the fixed-point heading is on or above it, where the reference's own formula gives -180 (include/atc_step.h)."""
    seen = []

    def probe(t, ref, spec):
        if t == step:
            N = ref.N
            seen.append((ref.raw_obs[env].copy(), spec.raw_obs[env].copy(), ref.phi.reshape(-1, N)[env].copy(), spec.phi.reshape(-1, N)[env].copy(),
                         ref.obs[env].copy(), spec.obs[env].copy()))

    comp = D.case(seed)[1]
    rec = D.fly(seed, max_steps=step + 1, probe=probe)
    assert rec["wrap9"] >= 1 and not rec["excluded"]
    raw64, raw32, phi64, phi32, obs64, obs32 = seen[0]
    k = np.flatnonzero((raw64[:, 9] == 180.0) & (raw32[:, 9] == -180.0))
    assert len(k) == 1 and (aircraft is None or k[0] == aircraft), k
    k = int(k[0])
    recip = (comp.corridor["phi_to_runway"] + 180.0) % 360.0
    off = lambda phi: (phi - recip) - 360.0 * np.rint((phi - recip) / 360.0)   # noqa: E731  (the heading relative to the reciprocal)
    assert -1e-9 < off(phi64[k]) < 0.0 and 0.0 <= off(phi32[k]) < 1e-6, (phi64[k], phi32[k], recip)
    assert abs(abs(obs64[k, 9] - obs32[k, 9]) - (2.0 if D.case(seed)[2]["normalize"] else 360.0)) < 1e-6   # the whole range apart


@pytest.mark.parametrize("sector", ["LOWW", "Simple"])
def test_word_9_either_side_of_the_reciprocal(sector):
    """Headings placed on the runway's reciprocal and ulps either side of it, held (target = the heading) and mid-turn (target 90 deg
    further: the step turns by 3 deg, so the start is placed 3 deg short): the float64 instantiation gives the reference's
    (phi - to_runway + 180) % 360 - 180 — +180 below the reciprocal, -180 on and above it.  The fp32 spec evaluates the same formula on
    the heading ROUNDED TO FP32 (fmaf(counts, 2^-23, 180): ulp 1.5e-5 deg at 160): every heading within half an fp32 ulp of the reciprocal
    reads -180, the counts just below it included, where the reference reads +180 (include/atc_step.h, "Observation word 9 at the wrap").
    An aircraft told to HOLD the reciprocal by a continuous action sits one count below it (the fp32 action, truncated to counts): the two
    instantiations then report opposite signs of the same angle on every step."""
    from oracle import oracle as O
    comp = H.compiled(sector)
    to_rwy = comp.corridor["phi_to_runway"]
    recip = (to_rwy + 180.0) % 360.0
    ulps = (-4, -1, 0, 1, 4)
    sides = []
    for turning in (False, True):
        for dtype in (np.float64, np.float32):
            env = O.OracleEnv(comp, 1, len(ulps), O.make_params(keep_active=True, sep_nm=0.0), dtype)
            act = np.zeros((1, len(ulps), 3), np.float32)
            for k, u in enumerate(ulps):
                target = recip + u * np.spacing(recip) if dtype == np.float64 else recip + u * 2.0 ** -23
                env.set_state(0, k, 20.0 + k, 60.0, 15000.0, target - (3.0 if turning else 0.0), 250.0)
                act[0, k] = H.hold_action((0, 0, 15000.0, recip + (90.0 if turning else 0.0), 250.0))
                if not turning:     # hold: the target is the heading itself up to the fp32 action's rounding (1e-5 deg) — keep it exact
                    act[0, k, 2] = np.float32(recip / 180.0 - 1.0)
            env.step(act.astype(dtype))
            phi = np.asarray(env.phi, np.float64)
            got = env.raw_obs[0, :, 9]
            for k, u in enumerate(ulps):
                if turning:
                    exact = (phi[k] - to_rwy + 180.0) % 360.0 - 180.0
                    assert dtype == np.float32 or got[k] == np.float32(exact), (sector, dtype, turning, u, phi[k], got[k])
                    assert got[k] == (180.0 if dtype(phi[k]) < recip else -180.0), (sector, dtype, u, phi[k], got[k])
            if not turning:   # every aircraft turned onto the fp32 action's heading: one value, on one side
                side = 180.0 if dtype(phi[0]) < recip else -180.0
                assert np.all(got == side) and np.all(phi == phi[0]) and 0.0 < recip - phi[0] < 1e-5, (sector, dtype, phi, got)
                sides.append(side)
    assert sides == [180.0, -180.0]      # float64, fp32: the held reciprocal reads +180 in the reference and -180 in the fp32 spec


# ---------------------------------------------------------------------------------------------------------------- the held references
@functools.lru_cache(maxsize=None)
def _held_record(seed):
    return D.fly_held(seed, device=False)


@pytest.mark.parametrize("seed", list(HELD_SEEDS))
def test_held_references_float64_against_fp32(seed):
    rec = _held_record(seed)
    assert all(rec["pairs"][k] + rec["excluded_pairs"] > 0 for k in D.HELD_KERNELS), rec["pairs"]


def test_held_references_sweep_stays_under_the_tie_cap():
    recs = [_held_record(seed) for seed in HELD_SEEDS]
    pairs = sum(sum(r["pairs"].values()) for r in recs)
    excluded = sum(r["excluded_pairs"] for r in recs)
    print("held references: %d (call, env) pairs compared, %d excluded as ties" % (pairs, excluded), [t for r in recs for t in r["ties"]])
    assert all(sum(r["pairs"][k] for r in recs) > 1000 for k in D.HELD_KERNELS)
    assert excluded <= D.EXCLUDED_CAP * (pairs + excluded), (excluded, pairs)


# ---------------------------------------------------------------------------------------------------------------- the kernels
@functools.lru_cache(maxsize=None)
def _gpu_record(i):
    return D.fly_kernel(i)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(GPU_CASES))
def test_kernels_follow_the_float64_oracle(i):
    scn, comp, kw = D.gpu_case(i)
    print("ref diff gpu case", i, type(scn).__name__, kw)
    rec, launched = _gpu_record(i)
    print("ref diff gpu case", i, "launched", launched, "excluded", rec["excluded"], "wrap9", rec["wrap9"],
          "largest deviations", {k: "%.2e" % v for k, v in rec["maxdev"].items()})
    W = H.lane_width(kw["N"])
    assert launched and all(name.startswith("%d/" % W) for name in launched), launched
    assert rec["env_steps"] + rec["excluded_steps"] == kw["B"] * kw["steps"], (rec["env_steps"], rec["excluded_steps"])


@pytest.mark.gpu
def test_kernel_cases_stay_under_the_tie_and_wrap_caps():
    total = D.new_record()
    for i in range(GPU_CASES):
        D.merge(total, _gpu_record(i)[0])
    print("\n".join(D.report(total)))
    assert not D.check_caps(total), D.check_caps(total)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [5000 + i for i in range(GPU_HELD)])
def test_held_kernels_follow_the_float64_oracle(seed):
    rec = D.fly_held(seed, device=True)
    print("ref diff held gpu case", seed, rec["pairs"], "excluded", rec["excluded_pairs"], rec["ties"],
          "largest deviations", {k: "%.2e" % v for k, v in rec["maxdev"].items()})
    assert all(rec["pairs"][k] + rec["excluded_pairs"] > 0 for k in D.HELD_KERNELS), rec["pairs"]
    assert rec["excluded_pairs"] <= max(1, D.EXCLUDED_CAP * sum(rec["pairs"].values())) and len(rec["ties"]) == len(set(rec["ties"]))


def test_gpu_cases_cover_every_form_and_width():
    """the drawn kernel cases, listed without a GPU: every (N, launch form) pair, fast and full outputs, every sector; the held cases reach
    every lane width"""
    import held_fuzz as F
    cases = [D.gpu_case(i) for i in range(28)]
    assert {(kw["N"], kw["form"]) for _, _, kw in cases} == {(n, f) for n in D.GPU_N for f in D.GPU_FORMS}
    assert {kw["full"] for _, _, kw in cases} == {False, True}
    assert {type(scn).__name__ for scn, _, _ in cases} == {"LOWW", "SimpleScenario", "LOWWDense"}
    assert all(kw["B"] <= 64 and kw["steps"] <= 120 and kw["steps"] % kw["chunk"] == 0 for _, _, kw in cases)
    held = [F.case(5000 + i)[2] for i in range(12)]
    assert {1, 16, 64} <= {H.lane_width(kw["N"]) for kw in held} and any(kw["N"] > 16 for kw in held), [kw["N"] for kw in held]
