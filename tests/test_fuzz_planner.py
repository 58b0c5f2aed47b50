"""One iteration of the scored planners — lookahead_plan_sampled -> score_plans -> refit_plans -> draw_plans(index=top[:1]), and
cem_plan_scored / mppi_plan_scored (atc_hip/cem.py) around them — held to a float64 evaluation of the ORACLE's flight of the same plans
(tests/planner_ref.py) over the mode space of the held sweep: the first CASES cases of tests/held_fuzz.py, flown exactly as
tests/test_fuzz_plan_sampled.py flies them (tests/sampled_fuzz.py), with the case's own M, H, K, std = STD and mean_first.  By seed the
cases alternate between ELITE (E in {1, min(3, M), M}) and SOFTMAX (two temperatures), gamma in {1, 0.9, 0} and top in {1, 5}.

Per continuous-action case, on the GPU: the chain of public calls checked by planner_ref.check_iteration; the env state byte-equal to a
snapshot and in step with the oracle; cem_plan_scored / mppi_plan_scored with iters = 1 and 2 equal to the chain of public calls word for
word; the decision flown with step_skip on the device and, as the numpy row of the same candidate, on the oracle, and the env still in
step.  Discrete-action cases: refit_plans refuses and no launch record moves; score_plans on the case's recorded seg_reward equals
tests/plan_score_ref.py — score, top and the ELITE weight bit for bit, the SOFTMAX weight within SOFTMAX_ULP_BAR of
float32(exp(float64(x))) (expf is the one inexact step of the contract: the rule of tests/test_plan_score.py).  One more GPU test runs
both planners and the chain of public calls on a side stream with a python-float std; another puts subnormal softmax weights through the
refit on the device.

WHAT THE SWEEP CANNOT HOLD.  The candidates of an env that is evaluated all have n_steps >= 1, and the oracle's rewards are finite, so over
flown envs validity is all or none: "fewer valid candidates than E" is met only by the envs with NO valid candidate (WIDE at the start),
and sum(weight) == min(E, valid) with 0 < valid < E is never flown.  test_partial_validity_on_the_stand_in puts that branch through
check_iteration with an oracle reward made infinite; on the device it is tests/test_plan_score.py's grid that holds it (the junk family).

CPU twins: the sweep contains what it is for; THE CAP, a condition on the inputs — at most 5 % of the evaluated envs non-decisive for the
winner, at most 5 % for the elite boundary (planner_ref: DECISIVE), asserted on the oracle alone and again over what the device flew —;
the checks have teeth: a stand-in device built from the oracle's rewards with the numpy restatements passes every case, and each of five
deliberate faults is caught by a case the test names.

STD.  The sweep was first drawn with std = 0.3, the std of tests/test_fuzz_plan_sampled.py.  It missed the cap: 70 of 766 evaluated envs
(9.14 %) were non-decisive for the winner, most of them in the cases with 16 .. 63 aircraft, where the bar of a score — 1e-5 of the summed
per-step reward scale of up to 20 steps — is a third of the spread std = 0.3 gives the candidates' scores.  The cap is a condition on the
inputs, so the inputs changed: std = 2.0 (most components of a drawn plan lie on the edge of the action space, candidate 0 stays the
mean) gives 21 of 766 (1.0 gives 32).

On the oracle, CASES = 30: 17 cases are flown and 13 (discrete actions) refused, every lane-group width among the flown; 1 820 evaluated
(candidate, env) pairs in 766 evaluated envs, 9 envs without a valid candidate; non-decisive for the winner 21 of 766 (2.74 %), for the
elite boundary 0 of 416 asked (0 %).  The stand-in's largest |score - score64| / bar is 0.012, its largest softmax distance over its bar
0.0061, its largest refit error over its bound 0.48.  On an MI355X: the same 17 / 13 cases, 1 820 pairs and shares (21 of 766, 0 of 416);
largest |score - score64| / bar 0.043, largest softmax distance over its bar 0.025, largest refit error over its bound 0.58.  The
mutations are caught by: late — 5013, 5023; plus1 — 5002, 5010, 5011, 5013, 5020, 5022, 5023, 5029; admit — 5020; ties — 5003, 5009,
5010, 5011, 5018, 5024; the unshifted refit — 5002, 5003, 5009, 5010, 5011, 5015, 5027, 5029.  The ratios are reported, not tuned."""
import functools

import numpy as np
import pytest

import bars
import held_fuzz as F
import helpers as H
import plan_draw_ref as P
import plan_refit_ref as RF
import plan_score_ref as S
import planner_ref as PR
import skip_ref as R
from fuzz_space import make_env, make_oracle
from sampled_fuzz import CASES, SEED0, fly_to_the_plan, inputs, key, oracle_side

CAP = 0.05
STD = 2.0           # (0.3, the std of tests/test_fuzz_plan_sampled.py, misses the cap: see the module docstring)
TEMPERATURES = (0.5, 5.0)
GAMMAS = (1.0, 0.9, 0.0)
TOPS = (1, 5)
SEEDS = [SEED0 + i for i in range(CASES)]


def _how(seed, M):
    """the scoring arguments of a case, alternating by seed (i % 2 and i % 3 are independent over the sweep)"""
    i = seed - SEED0
    how = dict(gamma=GAMMAS[i % 3], top=TOPS[(i // 3) % 2])
    if i % 2 == 0:
        return dict(how, mode="elite", elites=(1, min(3, M), M)[(i // 2) % 3])
    return dict(how, mode="softmax", temperature=TEMPERATURES[(i // 2) % 2])


def _merge(total, stats):
    for k, v in stats.items():
        total[k] = max(total.get(k, 0.0), v) if isinstance(v, float) else total.get(k, 0) + v


@functools.lru_cache(maxsize=None)
def _oracle_record(seed):
    """a continuous case on the oracle alone: everything check_iteration needs, and the case's events"""
    scn, comp, kw, rng = inputs(seed)
    if kw["discrete"]:
        return None
    c = kw["plan"]
    orc = make_oracle(comp, kw, auto_reset=True)
    mean, auto_reset = fly_to_the_plan(None, orc, kw, rng)
    refs, ok, ev, _, _ = oracle_side(orc, kw, mean, auto_reset, STD)
    plans = P.draw(mean, STD, c["M"], **key(kw))
    how = _how(seed, c["M"])
    ref = PR.reference(refs, ok, **how)
    n = ref["n_steps"]
    segs = -(-n // c["K"])
    events = dict(ev, fewer_than_E=int((ref["valid"].sum(0) < how.get("elites", 0)).sum()), none_valid=int((~ref["evaluated"]).sum()),
                  differ_n=int((ok & (n.min(0) != n.max(0))).sum()), nothing_behind=int(((n < c["K"] * c["H"]) & (segs == c["H"]))[:, ok].sum()),
                  zeros_behind=int((segs < c["H"])[:, ok].sum()))
    return dict(kw=kw, refs=refs, ok=ok, plans=plans, mean=mean, how=how, ref=ref, events=events, width=H.lane_width(kw["N"]))


def _flown():
    return [(s, r) for s, r in ((s, _oracle_record(s)) for s in SEEDS) if r is not None]


def _stand_in(rec, mutation=None):
    return PR.stand_in(rec["refs"], rec["ok"], rec["plans"], rec["mean"], STD, mutation=mutation, **rec["how"])


# ---------------------------------------------------------------------------------------------------------------- CPU twins
def test_sweep_contains_what_it_is_for_on_the_oracle():
    flown = _flown()
    assert 0 < len(flown) < CASES, "the sweep needs drawn cases and refused (discrete) ones"
    total = {k: sum(r["events"][k] for _, r in flown) for k in ("fewer_than_E", "none_valid", "differ_n", "zeros_behind", "nothing_behind", "early")}
    hows = [r["how"] for _, r in flown]
    print("planner fuzz: cases flown %d, refused %d; events %s" % (len(flown), CASES - len(flown), total))
    # an env with fewer valid candidates than E, one with none, candidates of an env stopping at different n_steps, an early stop with
    # zero segments behind it (and one inside the last segment, with nothing behind it), every lane-group width
    assert all(total.values()), total
    assert {r["width"] for _, r in flown} == set(F.WIDTHS)
    for name, values in (("gamma", GAMMAS), ("top", TOPS), ("mode", ("elite", "softmax"))):
        assert {h[name] for h in hows} == set(values), name
    assert {h["temperature"] for h in hows if h["mode"] == "softmax"} == set(TEMPERATURES)
    assert any(h.get("elites") == 1 for h in hows) and any(h.get("elites", 0) > 1 for h in hows)


def _shares(refs):
    ev, ndw, asked, nde = (sum(x) for x in zip(*(PR.shares(r) for r in refs)))
    return ev, ndw, asked, nde


def _under_the_cap(refs, where):
    ev, ndw, asked, nde = _shares(refs)
    print("planner fuzz, %s: evaluated pairs %d in %d evaluated envs; non-decisive for the winner %d of %d (%.2f %%), for the elite boundary "
          "%d of %d (%.2f %%)" % (where, sum(int(r["valid"].sum()) for r in refs), ev, ndw, ev, 100.0 * ndw / ev, nde, asked, 100.0 * nde / max(asked, 1)))
    assert ev > 0 and asked > 0
    assert ndw <= CAP * ev, (ndw, ev)
    assert nde <= CAP * asked, (nde, asked)


def test_oracle_sweep_stays_under_the_cap():
    """a condition on the INPUTS: were it to fail, the sweep's inputs (std, the temperatures, which E) change, never the cap"""
    _under_the_cap([r["ref"] for _, r in _flown()], "on the oracle")


def test_stand_in_passes_every_case():
    total = {}
    for seed, rec in _flown():
        _merge(total, PR.check_iteration(_stand_in(rec), rec["ref"], rec["plans"], rec["mean"], STD, tag=("stand-in", seed)))
    print("planner fuzz, the stand-in: %d pairs, largest |score - score64| / bar %.3g, softmax distance / bar %.3g, refit error / bound %.3g" % (
        total["pairs"], total["score"], total["softmax"], total["refit"]))
    assert total["pairs"] > 0 and total["softmax"] > 0 and total["refit"] > 0


@pytest.mark.parametrize("mutation", PR.MUTATIONS)
def test_check_iteration_catches(mutation):
    """late: the discount one segment late; plus1: gamma^(h + 1); admit: not-evaluated candidates admitted; ties: an exact tie to the
    higher number.  Each must raise on at least one case of the sweep, and the message names the case."""
    caught = {}
    for seed, rec in _flown():
        try:
            PR.check_iteration(_stand_in(rec, mutation), rec["ref"], rec["plans"], rec["mean"], STD, tag=("case", seed, mutation))
        except AssertionError as exc:
            assert str(seed) in str(exc), "the message does not name the case"
            caught[seed] = str(exc.args[0][0] if isinstance(exc.args[0], tuple) else exc)[:60]
    print("planner fuzz: mutation %r caught by cases %s" % (mutation, caught))
    assert caught, "no case of the sweep catches %r: the sweep is too weak" % mutation


def test_check_refit_catches_the_unshifted_form():
    """the fifth fault: at std = 1e-4 the refit about the unclamped mean in the E[a^2] - E[a]^2 form misses the summation bound, the
    restatement meets it, on the weights the case's own scoring gave"""
    caught = []
    for seed, rec in _flown():
        M = rec["plans"].shape[0]
        w = _stand_in(rec)["weight"]
        plans = P.draw(rec["mean"], 1e-4, M, **key(rec["kw"]))
        good = RF.refit(rec["mean"], 1e-4, M, w, draws=plans)
        PR.check_refit(good[0], good[1], rec["mean"], 1e-4, plans, w, tag=("case", seed, "std 1e-4"))
        bad = PR.naive_refit(rec["mean"], 1e-4, plans, w)
        try:
            PR.check_refit(bad[0], bad[1], rec["mean"], 1e-4, plans, w, tag=("case", seed, "unshifted"))
        except AssertionError as exc:
            assert str(seed) in str(exc)
            caught.append(seed)
    print("planner fuzz: the unshifted refit caught by cases %s" % caught)
    assert caught, "no case of the sweep catches the unshifted refit: the sweep is too weak"


def test_partial_validity_on_the_stand_in():
    """0 < valid < E, which no flown env shows (module docstring): an oracle reward of a case with M = 3 made infinite for candidate 1 in
    every other env.  The reference leaves the candidate out, the stand-in gives it weight 0, sum(weight) == 2 < E there, and admitting
    it is caught."""
    seed, rec = next((s, r) for s, r in _flown() if r["how"].get("elites") == 3 and r["plans"].shape[0] == 3)
    refs = [dict(r, seg_reward=np.array(r["seg_reward"], np.float64)) for r in rec["refs"]]
    hit = rec["ok"] & (np.arange(len(rec["ok"])) % 2 == 0)
    assert hit.any()
    refs[1]["seg_reward"][0, hit] = np.inf
    ref = PR.reference(refs, rec["ok"], **rec["how"])
    assert ((ref["valid"].sum(0) == 2) & hit).sum() == hit.sum() and not ref["valid"][1, hit].any()
    got = PR.stand_in(refs, rec["ok"], rec["plans"], rec["mean"], STD, **rec["how"])
    assert (got["weight"][:, hit].sum(0) == 2).all() and not got["weight"][1, hit].any()
    PR.check_iteration(got, ref, rec["plans"], rec["mean"], STD, tag=("partial validity", seed))
    bad = dict(got, weight=got["weight"].copy())
    bad["weight"][1, hit] = 1.0
    with pytest.raises(AssertionError, match="invalid candidate"):
        PR.check_iteration(bad, ref, rec["plans"], rec["mean"], STD, tag=("partial validity", seed))


def _subnormal_case():
    """mean, plans and seg_reward [M, 1, B] whose SOFTMAX weights at T = 0.5 run from just above FLT_MIN down to the smallest
    subnormal: candidate 0 — the clamped mean itself under mean_first, d == 0 exactly — wins with score 0, candidate m of env e scores
    -0.5 x with x from 86 (exp(-x) = 4.5e-38) to 103.2 (1.5e-45)"""
    M, Hn, B, N = 5, 2, 6, 3
    rng = np.random.default_rng(149)
    mean = rng.uniform(-0.6, 0.6, (Hn, B, N, 3)).astype(np.float32)
    k = dict(seed=77, iteration=2, mean_first=True)
    plans = P.draw(mean, 0.3, M, **k)
    x = np.linspace(86.0, 103.2, (M - 1) * B).reshape(M - 1, B)
    seg = np.zeros((M, 1, B), np.float32)
    seg[1:, 0] = (-0.5 * x).astype(np.float32)
    return M, mean, plans, seg, k


def test_check_refit_holds_subnormal_softmax_weights():
    """Weights among the subnormals participate (0 < w <= FLT_MAX), and with the winner at d == 0 the sums w d and w d^2 lie among the
    subnormals too, where fl(x op y) = (x op y)(1 + delta) does not hold: plan_refit_ref.bounds carries the absolute underflow terms, and
    the restatement meets it."""
    M, mean, plans, seg, k = _subnormal_case()
    w = np.asarray(S.plan_score(seg, None, "softmax", None, 0.5, 1.0, 1)["weight"]).astype(np.float32)
    sub = (w > 0) & (w < S.FLT_MIN)
    assert (w[0] == 1.0).all() and sub.sum() >= 0.8 * w[1:].size and RF.participates(w)[sub].all() and (w[1:] >= S.FLT_MIN).any()
    r64 = RF.refit64(mean, 0.3, M, w, draws=plans)
    assert (r64["A2"] * r64["W"] < S.FLT_MIN).all(), "the sum of w d^2 is not among the subnormals"
    new = RF.refit(mean, 0.3, M, w, draws=plans)
    worst = PR.check_refit(new[0], new[1], mean, 0.3, plans, w, tag="subnormal softmax weights")
    print("planner fuzz: subnormal softmax weights, the restatement: largest refit error over its bound %.3g" % worst)
    assert worst > 0


# ---------------------------------------------------------------------------------------------------------------- GPU
_device = {}      # seed -> (the case's reference with the device's own segment words, what check_iteration measured)


# every launch record of the library (helpers.launch_records), the ones this module indexes first
_records = functools.partial(H.launch_records, "plan_score", "plan_refit", "plan_sampled", "plan_draw")


def _same_words(got, want, what, tag):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want).reshape(np.shape(got))
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad[0]), "%s %r: %d words differ, first at %r: got %r want %r" % (
        what, tag, len(bad[0]), tuple(int(b[0]) for b in bad), got[bad][0], want[bad][0])


def _iteration(env, mean, std, K, M, seed, t, how):
    """one iteration by the public calls; returns numpy copies of everything (the calls' result tensors are reused by the next call)"""
    res = env.lookahead_plan_sampled(mean, std, K, M, seed=seed, iteration=t, mean_first=True, outputs=("seg_reward",))
    sc = env.score_plans(res["seg_reward"], res["n_steps"], **how)
    new_mean, new_std = env.refit_plans(mean, std, M, sc["weight"], seed=seed, iteration=t, mean_first=True)
    decision = env.draw_plans(mean, std, M, seed=seed, iteration=t, mean_first=True, index=sc["top"][:1])[0, 0]
    env.synchronize()
    got = {k: v.cpu().numpy() for k, v in dict(sc, seg_reward=res["seg_reward"], n_steps=res["n_steps"], new_mean=new_mean, new_std=new_std,
                                               decision=decision).items()}
    return got, new_mean, new_std


def _discrete_case(env, orc, kw, rng, seed):
    """refit_plans refuses and no launch record moves; score_plans on the case's recorded seg_reward equals tests/plan_score_ref.py"""
    import torch
    c = kw["plan"]
    M, Hn, K, B, N = c["M"], c["H"], c["K"], kw["B"], kw["N"]
    cand, _ = fly_to_the_plan(env, orc, kw, rng, whole=True)
    before = _records()
    with pytest.raises(ValueError):
        env.refit_plans(torch.zeros((Hn, B, N, 3), device=env.device), STD, M, torch.ones((M, B), device=env.device))
    assert _records() == before, "a refused refit moved a launch record"
    res = env.lookahead_plan(torch.as_tensor(cand, device=env.device), K, outputs=("seg_reward",))
    how = _how(seed, M)
    sc = env.score_plans(res["seg_reward"], res["n_steps"], **how)
    env.synchronize()
    now = _records()
    assert now[0].get("score", 0) == before[0].get("score", 0) + 1 and now[1] == before[1], "score_plans is one launch of its own record"
    want = S.plan_score(res["seg_reward"].cpu().numpy(), res["n_steps"].cpu().numpy(), how["mode"], how.get("elites"), how.get("temperature"),
                        how["gamma"], how["top"])
    _same_words(sc["score"].cpu().numpy(), want["score"], "score", seed)
    _same_words(sc["top"].cpu().numpy(), want["top"], "top", seed)
    w = sc["weight"].cpu().numpy()
    if how["mode"] == "elite":
        _same_words(w, want["weight"], "weight", seed)
    else:       # (expf is the one inexact step of the contract: tests/test_plan_score.py's rule)
        w64, okx = np.asarray(want["weight"], np.float64), ~np.isnan(want["x"])
        assert not w[~okx].view(np.uint32).any()
        small = okx & (w64 < S.FLT_MIN)
        assert (np.abs(w[small].astype(np.float64) - w64[small]) <= S.FLT_MIN).all()
        assert not (okx & ~small).any() or int(S.ulp_distance(w[okx & ~small], w64[okx & ~small]).max()) <= S.SOFTMAX_ULP_BAR


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("seed", SEEDS)
def test_planner_iteration_matches_oracle(seed):
    import torch
    from atc_hip import cem
    scn, comp, kw, rng = inputs(seed)
    c = kw["plan"]
    M, Hn, K, B, N = c["M"], c["H"], c["K"], kw["B"], kw["N"]
    how = _how(seed, M)
    print("planner fuzz case", seed, type(scn).__name__, kw, how)
    env = make_env(scn, kw, auto_reset=True)
    orc = make_oracle(comp, kw, auto_reset=True)
    try:
        if kw["discrete"]:
            _discrete_case(env, orc, kw, rng, seed)
            return
        mean, auto_reset = fly_to_the_plan(env, orc, kw, rng)
        refs, ok, _, _, _ = oracle_side(orc, kw, mean, auto_reset, STD)
        plans = P.draw(mean, STD, M, **key(kw))
        snap = H.snapshot(env)
        before = _records()
        tm = torch.as_tensor(mean, device=env.device)
        # 1. / 2. the chain of public calls, held to the oracle
        got, mean1, std1 = _iteration(env, tm, STD, K, M, kw["seed"], 0, how)
        now = _records()
        assert now[0].get("score", 0) - before[0].get("score", 0) == 1 and now[1].get("refit", 0) - before[1].get("refit", 0) == 1
        assert {w: n - before[2].get(w, 0) for w, n in now[2].items() if n != before[2].get(w, 0)} == {H.lane_width(N): 1} and now[4:] == before[4:]
        for m in range(M):
            bars.check_plan_segments(got["seg_reward"][m], refs[m], ok, K, tag=("planner", seed, m))
        ref = PR.reference(refs, ok, seg32=got["seg_reward"], **how)
        stats = PR.check_iteration(got, ref, plans, mean, STD, tag=("planner fuzz case", seed))
        # 3. nothing moved
        H.bytes_equal(env, snap)
        bars.check_state(env, orc)
        # 4. the planners are that chain, word for word, at one and at two iterations
        got2, _, _ = _iteration(env, mean1, std1, K, M, kw["seed"], 1, how)
        for iters, g in ((1, got), (2, got2)):
            if how["mode"] == "elite":
                res = cem.cem_plan_scored(env, tm, STD, K, M, iters, how["elites"], gamma=how["gamma"], seed=kw["seed"])
            else:
                res = cem.mppi_plan_scored(env, tm, STD, K, M, iters, how["temperature"], gamma=how["gamma"], seed=kw["seed"])
            env.synchronize()
            for name, t, want in zip(("mean", "std", "decision"), res, (g["new_mean"], g["new_std"], g["decision"])):
                _same_words(t.cpu().numpy(), want, name, ("planner against the chain of public calls", seed, iters))
        H.bytes_equal(env, snap)
        bars.check_state(env, orc)
        # 5. fly the decision: the device's own tensor on the device, the numpy row of the same candidate on the oracle
        t0 = got["top"][0].astype(np.int64)
        row = np.where((t0 >= 0)[:, None, None], plans[np.maximum(t0, 0), 0, np.arange(B)], np.float32(0))
        decision = env.draw_plans(tm, STD, M, index=torch.as_tensor(got["top"][:1], device=env.device), **key(kw))[0, 0]
        sref = R.skip_reference(orc, row, K)
        flown = F._skip_outputs(env, env.step_skip(decision, K), kw["full"])
        bars.check_skip_outputs(flown, sref, bars.half_range(comp), kw["full"], ("the decision flown", seed))
        bars.check_state(env, orc)
        _device[seed] = (ref, stats)
    finally:
        env.close()


@pytest.mark.gpu
def test_device_sweep_stays_under_the_cap():
    """the cap over the sweep the cases above flew on the device, decided on the device's own segment words (this module's tests run in
    order, in one process); the figures of the run"""
    flown = [s for s in SEEDS if not F.case(s)[2]["discrete"]]
    assert sorted(_device) == flown, "run the module's sweep as a whole: the cap is the sweep's"
    total = {}
    for _, stats in _device.values():
        _merge(total, stats)
    print("planner fuzz, the device: cases flown %d, refused %d; %d pairs, largest |score - score64| / bar %.3g, softmax distance / bar %.3g, "
          "refit error / bound %.3g" % (len(flown), CASES - len(flown), total["pairs"], total["score"], total["softmax"], total["refit"]))
    _under_the_cap([ref for ref, _ in _device.values()], "on the device")


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_planners_on_a_side_stream_with_a_cached_std():
    """cem_plan_scored and mppi_plan_scored, three iterations each, under torch.cuda.stream(side) with a python-float std, against the
    same calls on the default stream, bit for bit; between the two planners lookahead_plan_sampled with ANOTHER python-float std replaces
    the env's cached broadcast tensor while the launches that read the previous one may still be in flight.  The state stays byte-equal."""
    import held_tools as T
    import torch
    from atc_hip import cem
    N, B, K, Hn, M = 8, H.ragged(8), 3, 2, 8
    rng = np.random.default_rng(84)
    env = T.look_env(N, B)
    T.look_fly(env, rng)
    mean = torch.as_tensor(rng.uniform(-0.5, 0.5, (Hn, B, N, 3)).astype(np.float32), device=env.device)
    env.synchronize()
    snap = H.snapshot(env)

    def both():
        a = cem.cem_plan_scored(env, mean, 0.4, K, M, 3, 3, gamma=0.9, seed=9)
        # (the planners broadcast a float std themselves, atc_hip/cem.py::_start; the cached tensor is read by the public calls: one
        # iteration by them, four launches that read the 0.4 entry and are not waited for ...)
        res = env.lookahead_plan_sampled(mean, 0.4, K, M, seed=9)
        first = res["seg_reward"].clone()
        sc = env.score_plans(res["seg_reward"], res["n_steps"], elites=3, gamma=0.9, top=1)
        chain = list(env.refit_plans(mean, 0.4, M, sc["weight"], seed=9)) + [env.draw_plans(mean, 0.4, M, seed=9, index=sc["top"][:1])[0, 0].clone()]
        other = env.lookahead_plan_sampled(mean, 0.25, K, M, seed=9)["seg_reward"].clone()     # ... when 0.25 takes the entry's place
        b = cem.mppi_plan_scored(env, mean, 0.4, K, M, 3, 5.0, gamma=0.9, seed=9, std_min=0.02)
        again = env.lookahead_plan_sampled(mean, 0.4, K, M, seed=9)["seg_reward"].clone()
        return [first, other, again] + list(a) + list(b) + chain

    side = torch.cuda.Stream(device=env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        got = both()
    side.synchronize()
    H.bytes_equal(env, snap)
    got = [t.cpu().numpy() for t in got]
    want = both()
    env.synchronize()
    H.bytes_equal(env, snap)
    names = ("seg_reward std 0.4", "seg_reward std 0.25", "seg_reward std 0.4 again", "cem mean", "cem std", "cem decision", "mppi mean", "mppi std",
             "mppi decision", "chain mean", "chain std", "chain decision")
    assert len(got) == len(names)
    one = cem.cem_plan_scored(env, mean, 0.4, K, M, 1, 3, gamma=0.9, seed=9)       # the chain is the planner's first iteration
    for name, g, w in zip(names[9:], got[9:], one):
        _same_words(g, w.cpu().numpy(), name, "the chain with the cached std against cem_plan_scored(iters=1)")
    for name, g, w in zip(names, got, want):
        _same_words(g, w.cpu().numpy(), name, "side stream against the default stream")
    assert not np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    H.bytes_equal(env, snap)
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(60)
def test_refit_of_subnormal_softmax_weights_on_the_device():
    """_subnormal_case on the device: score_plans' own SOFTMAX weights (T = 0.5; below FLT_MIN the contract holds them to an absolute
    FLT_MIN only, so they are taken as they come), fed to refit_plans.  The result equals the restatement under those weights bit for
    bit — the kernel keeps subnormal products as numpy does — and meets the float64 moments within plan_refit_ref.bounds."""
    import held_tools as T
    import torch
    M, mean, plans, seg, k = _subnormal_case()
    Hn, B, N = mean.shape[:3]
    env = T.look_env(N, B)
    sc = env.score_plans(torch.as_tensor(seg, device=env.device), mode="softmax", temperature=0.5, top=1)
    w = sc["weight"].cpu().numpy()
    want = np.asarray(S.plan_score(seg, None, "softmax", None, 0.5, 1.0, 1)["weight"])
    sub = (w > 0) & (w < S.FLT_MIN)
    print("planner fuzz: subnormal softmax weights on the device: %d of %d weights subnormal (the restatement: %d), %d flushed to zero" % (
        sub.sum(), w.size, ((want > 0) & (want.astype(np.float32) < S.FLT_MIN)).sum(), ((w == 0) & (want.astype(np.float32) > 0)).sum()))
    assert (w[0] == 1.0).all() and (np.abs(w.astype(np.float64) - want)[want < S.FLT_MIN] <= S.FLT_MIN).all()
    new = env.refit_plans(torch.as_tensor(mean, device=env.device), 0.3, M, sc["weight"], **k)
    env.synchronize()
    got = [t.cpu().numpy() for t in new]
    ref = RF.refit(mean, 0.3, M, w, draws=plans)
    _same_words(got[0], ref[0], "new_mean", "subnormal weights against the restatement")
    _same_words(got[1], ref[1], "new_std", "subnormal weights against the restatement")
    worst = PR.check_refit(got[0], got[1], mean, 0.3, plans, w, tag="subnormal softmax weights on the device")
    print("planner fuzz: subnormal softmax weights on the device: largest refit error over its bound %.3g" % worst)
    env.close()
