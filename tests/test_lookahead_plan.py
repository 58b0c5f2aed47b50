"""Plan look-ahead (include/atc_step.h: atc_lookahead_plan; AtcVecEnv.lookahead_plan): M plans per env, each H action blocks held for
K steps one after the other, in one launch that never writes state.

CPU: the exported symbols and the 14 k_plan instantiations, the header's constants and atc_plan_out's field order against
atc_hip/layout.py and atc_hip/lib.py, the refusal order (K before H before M before the pointers) through ctypes with NULL pointers,
the launch record, the Python surface; the events of the oracle cases and of the grid's placed envs on the oracle alone.
GPU: every output BIT-IDENTICAL to the definition run on the product itself — env.step_skip chained over the segments on clones of
the six state tensors, an env leaving the chain at its first done (sums in a fixed order and integer words: no tolerance applies);
H = 1 against env.lookahead; the prefix property; WIDE headings; one case per width against tests/skip_ref.py on the oracle (the bars
of tests/bars.py); a scripted call sequence with and without plan calls in between; 65 536 x 16.

Inputs are valid only if the REFERENCE shows the events of _check_events; the test fails otherwise."""
import ctypes as C
import inspect
import re
import shutil
import subprocess

import numpy as np
import pytest

import bars
import held_tools as T
import helpers as H
import skip_ref as R
from atc_hip import layout as L
from held_tools import HEADER, LIB, TIME_LIMIT

OPTIONAL = ("seg_reward", "flags", "min_sep", "ac_reward", "obs")
LOOK_ALL = OPTIONAL[1:]     # atc_lookahead's optional outputs
ALL = OPTIONAL
WIDTH_N = (1, 2, 3, 8, 16, 32, 64)

# (N, M, H, K, auto_reset, spawn, normalize, outputs): every N of the grid, M in {1, 3}, H in {1, 2, 4}, K in {1, 3, 7}, each switch
# both ways, the fast form with and without seg_reward, and the full form with each optional output absent in at least one case
CASES = [
    (1, 3, 2, 3, True, "random", True, ("seg_reward",)),
    (1, 1, 4, 7, False, "lattice", False, ALL),
    (2, 3, 4, 3, True, "lattice", True, ("seg_reward", "flags")),
    (2, 1, 1, 1, True, "random", False, ()),
    (3, 3, 2, 7, True, "random", True, ALL),
    (3, 1, 4, 3, False, "lattice", True, ("seg_reward",)),
    (8, 3, 4, 7, True, "lattice", False, ("ac_reward",)),
    (8, 3, 1, 3, False, "random", True, ("seg_reward", "flags", "min_sep")),
    (16, 3, 4, 3, True, "lattice", True, ALL),
    (16, 3, 2, 7, True, "random", False, ("seg_reward",)),
    (16, 1, 2, 1, False, "lattice", True, ("seg_reward", "obs")),
    (32, 3, 2, 3, True, "lattice", True, ALL),
    (32, 3, 4, 7, False, "random", False, ()),
    (33, 3, 4, 7, True, "lattice", True, ("seg_reward", "flags", "ac_reward")),
    (33, 1, 2, 3, True, "random", False, ("seg_reward",)),
    (64, 3, 2, 3, True, "lattice", False, ALL),
    (64, 3, 4, 7, False, "lattice", True, ("seg_reward",)),
]
IDS = ["N%d M%d H%d K%d %s %s %s %s" % (c[0], c[1], c[2], c[3], "reset" if c[4] else "noreset", c[5], "norm" if c[6] else "raw",
                                        "+".join(c[7]) or "fast") for c in CASES]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_exports_and_kernel_symbols():
    from atc_hip import lib
    names = ("atc_lookahead_plan", "atc_plan_launch_counts")
    assert set(names) <= set(lib.EXPORTS)
    h = C.CDLL(LIB)
    for name in names:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    found = set(re.findall(r"\bvoid k_plan<(\d+), (true|false)>\(", text))
    assert found == {(str(w), f) for w in (1, 2, 4, 8, 16, 32, 64) for f in ("true", "false")}, found


def test_header_constants_match_layout():
    from atc_hip import lib
    text = open(HEADER).read()
    assert L.PLAN_MAX_H == int(re.search(r"#define ATC_PLAN_MAX_H (\d+)", text).group(1)) == 16
    assert L.PLAN_LAUNCH_SLOTS == int(re.search(r"ATC_PLAN_LAUNCH_SLOTS = (\d+)", text).group(1)) == 7
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22
    body = re.search(r"typedef struct atc_plan_out \{(.*?)\} atc_plan_out_t;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == list(lib.PLAN_FIELDS) == [f[0] for f in lib.AtcPlanOut._fields_]
    assert names == ["reward", "done", "n_steps", "seg_reward", "flags", "ac_reward", "min_sep", "obs"]


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    call = lambda K, Hn, M, out=None: h.atc_lookahead_plan(None, 1, 1, K, Hn, M, None, None, out, None, None)   # noqa: E731
    for K in (0, 256, -3):
        for Hn in (0, 1, 17):      # K is looked at before H and M
            for M in (0, 1, 65):
                assert call(K, Hn, M) == -1 and b"K (" in h.atc_last_error() and b"255" in h.atc_last_error()
    for Hn in (0, 17, -1):
        for M in (0, 1, 65):       # H is looked at before M
            assert call(1, Hn, M) == -1 and b"H (" in h.atc_last_error() and b"16" in h.atc_last_error()
    for M in (0, 65, -1):
        assert call(255, 16, M) == -1 and b"M (" in h.atc_last_error() and b"64" in h.atc_last_error()
    assert call(1, 1, 1) == -1 and b"null" in h.atc_last_error()          # K, H and M in range: now the pointers, `out` first
    out = lib.AtcPlanOut()
    assert call(255, 16, 64, C.byref(out)) == -1 and b"reward" in h.atc_last_error()
    word = (C.c_float * 1)()
    out.reward = C.cast(word, C.c_void_p)                                  # reward set, done NULL
    assert call(1, 1, 1, C.byref(out)) == -1 and b"done" in h.atc_last_error()
    out.done = C.cast(word, C.c_void_p)                                    # both set: the next refusal is atc_step's (actions NULL)
    assert call(1, 1, 1, C.byref(out)) == -1 and b"null pointer" in h.atc_last_error() and b"reward" not in h.atc_last_error()


def test_launch_record_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    buf = (C.c_uint64 * L.PLAN_LAUNCH_SLOTS)(*([99] * L.PLAN_LAUNCH_SLOTS))
    assert h.atc_plan_launch_counts(buf, L.PLAN_LAUNCH_SLOTS) == 0
    assert h.atc_plan_launch_counts(None, 7) == -1
    assert isinstance(lib.plan_launch_counts(), dict)
    assert all(v != 99 for v in buf)


def test_python_surface():
    from atc_hip import sb_adapter
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import atc_gym
    sig = inspect.signature(AtcVecEnv.lookahead_plan)
    assert list(sig.parameters) == ["self", "actions", "K", "outputs"]
    assert sig.parameters["outputs"].default == ("seg_reward", "flags", "min_sep")
    assert AtcVecEnv.PLAN_OUTPUTS == OPTIONAL
    sig = inspect.signature(AtcVecEnv.lookahead)
    assert list(sig.parameters) == ["self", "actions", "K", "outputs"] and sig.parameters["outputs"].default == ("flags", "min_sep")
    assert not hasattr(sb_adapter.AtcSBVecEnv, "lookahead_plan")    # deliberately out of scope
    assert not hasattr(atc_gym.AtcGym, "lookahead_plan")


# ------------------------------------------------------------------------------------------------- the oracle cases' inputs
ORACLE_M, ORACLE_H, ORACLE_K = 2, 3, 4


def _oracle_case(N):
    """device-independent part of the oracle case of width N: (scn, comp, kw, B, seed)"""
    scn, comp = T.skip_setup(N)
    # (time limit: 4 steps are flown, so an env that was never reset stops in the plan's last segment; conflicts end others earlier)
    return scn, comp, dict(T.skip_plan(N), timestep_limit=14), T.look_ragged(N), 8642 + N


def _oracle_inputs(rng, B, N):
    """the flown calls' actions and the plans: headings inside the action space (a WIDE target is not evaluated: its own test)"""
    flown = []
    for Kf in (3, 1):
        a = T.skip_actions(rng, B, N)
        a[..., 2] = np.clip(a[..., 2], -1.0, 1.0)
        flown.append((a, Kf))
    cand = T.skip_actions(rng, ORACLE_M * ORACLE_H * B, N).reshape(ORACLE_M, ORACLE_H, B, N, 3)
    cand[..., 2] = np.clip(cand[..., 2], -1.0, 1.0)
    return flown, cand


_oracle_chain, _oracle_refs = R.plan_chain, R.plan_references   # (the definition on the oracle: shared with tests/held_fuzz.py)


@pytest.mark.parametrize("N", WIDTH_N)
def test_oracle_case_events_on_the_oracle(N):
    """A condition on the INPUTS of the oracle cases, checked without a GPU: an env-candidate stops before the plan's end, and one
    does so in a segment h >= 1 (whole plans without a done: the equality grid's events)."""
    scn, comp, kw, B, seed = _oracle_case(N)
    orc = T.skip_oracle(comp, B, N, True, seed, **kw)
    flown, cand = _oracle_inputs(np.random.default_rng(seed), B, N)
    for a, Kf in flown:
        R.skip_reference(orc, a, Kf)
    n = np.stack([r["n_steps"] for r in _oracle_refs(orc, cand, ORACLE_K)])
    assert (n < ORACLE_H * ORACLE_K).any(), "no env-candidate stops early"
    assert ((n > ORACLE_K) & (n < ORACLE_H * ORACLE_K)).any(), "no env-candidate stops in a segment h >= 1"


def _grid_inputs(case):
    """the plans of a grid case as the GPU test draws them (the same generator, the same order of draws)"""
    import torch
    N, M, Hn, K = CASES[case][:4]
    B = T.look_ragged(N)
    rng = np.random.default_rng(2000 + 7 * case)
    T.look_draw(rng, 200 // 10, B, N)                      # (_fly's draw)
    actions = torch.as_tensor(T.look_draw(rng, M, Hn, B, N))
    return actions.numpy(), _place_plans(actions, M, Hn)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_placed_envs_show_their_events_on_the_oracle(case):
    """A condition on the INPUTS of the grid cases, checked without a GPU: the two placed envs — alone in their env, so a one-aircraft
    oracle flies them — do what _check_events asks of them.  Env 0: plan 0 ends in segment 0, plan 2 runs all H K steps, the late plan
    reaches segment 1 with its altitude target refused then accepted and its speed target accepted then refused.  The last env: every
    plan ends in segment 1 by the time limit."""
    from envs.atc import scenarios
    from oracle import oracle as O
    N, M, Hn, K, auto_reset, spawn = CASES[case][:6]
    if "grid" not in H._compiled:
        H._compiled["grid"] = scenarios.compile_scenario(T.look_scenario(), grid_cell=0.5)
    comp = H._compiled["grid"]
    actions, late = _grid_inputs(case)
    x, y, _, phi, v = H.FAR_A
    floor = float(O.OracleQueries(comp, np.float32).mva([x], [y])[0])

    def fly(e, state, t0, m):
        orc = O.OracleEnv(comp, 1, 1, O.make_params(auto_reset=auto_reset, random_entry=spawn == "random", seed=11,
                                                    timestep_limit=TIME_LIMIT, sep_nm=5.0), np.float32)
        orc.reset()
        orc.set_state(0, 0, *state)
        orc.set_last_action(0, 0, [state[4], state[2], state[3]])
        orc.timesteps[0] = t0
        n, flags = 0, []
        for h in range(Hn):
            r = R.skip_reference(orc, actions[m, h, e:e + 1, :1], K)
            n += int(r["n_steps"][0])
            flags.append(int(r["flags"][0, 0]))
            if r["done"][0]:
                return n, True, flags
        return n, False, flags

    start = (x, y, floor + 100.0, phi, v)
    if Hn > 1:
        n, done, flags = fly(0, start, 5, late)
        assert n > K
        assert flags[0] & H.F_INVALID_H and not flags[0] & H.F_INVALID_V and flags[1] & H.F_INVALID_V and not flags[1] & H.F_INVALID_H
    if M > 1 and K >= 3:
        assert fly(0, start, 5, 0)[:2] == (3, True)
        assert fly(0, start, 5, 2)[:2] == (Hn * K, False)
    if Hn > 1 and K >= 3:
        for m in range(M):
            n, done, _ = fly(actions.shape[2] - 1, H.FAR_B, TIME_LIMIT - K - 2, m)
            assert done and K < n <= 2 * K, (m, n, done)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _place_plans(actions, M, Hn):
    """env 0 (tests/held_tools.py::look_fly: aircraft 0 alone under control, a step above its MVA floor, far from the time limit):
    its plans stop in different segments, and aircraft 0's altitude / speed targets are refused in one segment and accepted in the
    next, in each order.  `late` is the plan that holds its altitude in segment 0 (refused target) and descends from segment 1 on; it
    flies east into an area with a lower floor, so it reaches segment 1 but need not end there: _place_timeout ends plans there."""
    late = 0 if M == 1 else 1
    if M > 1:
        actions[0, :, 0, 0, 1] = -0.9             # plan 0 descends at once: ends in segment 0
        actions[2, :, 0, 0, 1] = 0.9              # plan 2 climbs throughout: runs the whole plan
        actions[2, :, 0, 0, 0] = 0.3
    if Hn > 1:
        actions[late, 0, 0, 0, 1] = 2.5           # altitude: refused in segment 0 (the aircraft keeps its altitude) ...
        actions[late, 1:, 0, 0, 1] = -0.9         # ... accepted from segment 1
        actions[late, 0, 0, 0, 0] = 0.3           # speed: accepted in segment 0 ...
        actions[late, 1, 0, 0, 0] = 2.5           # ... refused in segment 1
    return late


def _place_timeout(env, K):
    """The last env: aircraft 0 alone under control, high above every floor (helpers.FAR_B), two steps short of the time limit at the
    end of segment 0 — every plan of it ends in segment 1 (K >= 2), whatever its actions."""
    e = env.B - 1
    env.set_state(e, 0, *H.FAR_B)
    env.set_last_action(e, 0, [H.FAR_B[4], H.FAR_B[2], H.FAR_B[3]])
    env.env[e, L.ENV_TIMESTEPS] = TIME_LIMIT - K - 2
    env.env[e, L.ENV_MASK_LO] = 1
    env.stats[e, L.STAT_MASK_HI] = 0
    env.synchronize()


def _check_events(ref, N, M, Hn, K, auto_reset, late):
    n = ref["n_steps"].numpy().astype(int)
    done = ref["done"].numpy().astype(bool)
    fl = ref["flags"].numpy().astype(np.uint16)
    seg = ref["seg_reward"].numpy()
    sfl = ref["seg_flags"].numpy().astype(np.uint16)
    segs = -(-n // K)            # executed segments
    print("events: n_steps %d..%d, segments run %s, done %d of %d" % (n.min(), n.max(), np.bincount(segs.ravel(), minlength=Hn + 1).tolist(),
                                                                      done.sum(), done.size))
    assert n.min() >= 1 and n.max() <= Hn * K
    assert (n == Hn * K).any(), "no env-candidate that runs all H K steps"
    for m, e in zip(*np.nonzero(segs < Hn)):
        assert done[m, e] and not seg[m, segs[m, e]:, e].view(np.uint32).any()
    if auto_reset:
        assert done.any(), "no look-ahead reset"
    if N > 1:
        assert (fl & H.F_CONFLICT).any(), "no conflict flag"
        assert (fl & H.F_INACTIVE).any(), "no handed-over aircraft"
    if Hn > 1 and K >= 3:      # (one step of descent from 100 ft above the floor does not end an episode: K = 1 shows the rest)
        if M > 1:
            assert (segs.min(0) != segs.max(0)).any(), "no env whose candidates stop in different segments"
        assert (done[:, -1] & (segs[:, -1] == 2)).all(), "the last env's plans do not end in segment 1 (h >= 1)"
        assert not seg[:, 2:, -1].view(np.uint32).any()      # (zero seg_reward behind the stop, where H > 2)
    if Hn > 1:                 # the refusal verdict is per segment: refused -> accepted (altitude), accepted -> refused (speed)
        assert segs[late, 0] >= 2, "env 0's late plan does not reach segment 1"
        assert sfl[late, 0, 0, 0] & H.F_INVALID_H and not sfl[late, 0, 0, 0] & H.F_INVALID_V
        assert sfl[late, 1, 0, 0] & H.F_INVALID_V and not sfl[late, 1, 0, 0] & H.F_INVALID_H


def _cpu(res):
    return {k: v.cpu() for k, v in res.items()}


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N,M,Hn,K,auto_reset,spawn,normalize,outputs", CASES, ids=IDS)
def test_plan_equals_chained_step_skip_on_copies(N, M, Hn, K, auto_reset, spawn, normalize, outputs):
    import torch
    from atc_hip import lib
    case = CASES.index((N, M, Hn, K, auto_reset, spawn, normalize, outputs))
    B = T.look_ragged(N)
    rng = np.random.default_rng(2000 + 7 * case)
    env = T.look_env(N, B, spawn, normalize)
    T.look_fly(env, rng)
    _place_timeout(env, K)
    H.set_auto_reset(env, auto_reset)
    actions = torch.as_tensor(T.look_draw(rng, M, Hn, B, N), device=env.device)
    late = _place_plans(actions, M, Hn)
    ref = T.chained_skip_reference(env, actions, K)
    _check_events(ref, N, M, Hn, K, auto_reset, late)
    ref.pop("seg_flags")
    snap = H.snapshot(env)
    before = (lib.plan_launch_counts(), lib.lookahead_launch_counts(), lib.skip_launch_counts(), lib.launch_counts(), lib.traffic_launch_counts())
    got = T.guarded_call(env, "plan", actions, K, outputs, n_steps=(case % 4 != 3))
    assert set(got) >= {"reward", "done"} | set(outputs)
    T.assert_equal(got, ref, "guarded")
    H.bytes_equal(env, snap)
    now = lib.plan_launch_counts()
    W = H.lane_width(N)
    assert {w: n - before[0].get(w, 0) for w, n in now.items() if n != before[0].get(w, 0)} == {W: 1}
    assert (lib.lookahead_launch_counts(), lib.skip_launch_counts(), lib.launch_counts(), lib.traffic_launch_counts()) == before[1:]
    # the Python surface: the same numbers, env outputs untouched; every candidate mapping; a permuted candidate axis; M = 1
    bound = {k: getattr(env, k).clone() for k in ("obs", "reward", "done", "flags")}
    perm = torch.as_tensor(rng.permutation(M), device=env.device)
    try:
        for cpg in (1, 2, M, 0):
            lib.lookahead_set_mapping(cpg)
            res = env.lookahead_plan(actions.view(M, Hn, B, N * 3), K, outputs=outputs)
            assert set(res) == {"reward", "done", "n_steps"} | set(outputs)
            assert res["reward"].shape == (M, B) and res["n_steps"].dtype == torch.int16
            assert "seg_reward" not in res or res["seg_reward"].shape == (M, Hn, B)
            T.assert_equal(_cpu(res), ref, ("python", cpg))
            first = env.lookahead_plan(actions, K, outputs=outputs)
            assert all(first[k].data_ptr() == res[k].data_ptr() for k in res), "output tensors are allocated once per (M, H, outputs)"
            p = env.lookahead_plan(actions[perm], K, outputs=outputs)
            T.assert_equal(_cpu(p), {k: v[perm.cpu()] for k, v in ref.items()}, ("permuted", cpg))
            one = env.lookahead_plan(actions[:1], K, outputs=outputs)
            T.assert_equal(_cpu(one), {k: v[:1] for k, v in ref.items()}, ("M = 1", cpg))
    finally:
        lib.lookahead_set_mapping(0)
    for k, v in bound.items():
        assert torch.equal(getattr(env, k), v), k
    H.bytes_equal(env, snap)
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N", WIDTH_N)
def test_one_segment_is_lookahead(N):
    """H == 1 reproduces env.lookahead bit for bit in every shared output, n_steps' values included; both forms."""
    import torch
    B, M, K = T.look_ragged(N), 3, 6
    rng = np.random.default_rng(300 + N)
    env = T.look_env(N, B, "lattice", True)
    T.look_fly(env, rng)
    actions = torch.as_tensor(T.look_draw(rng, M, B, N), device=env.device)
    actions[0, 0, 0, 1], actions[1, 0, 0, 1] = -0.9, 0.9
    for outs in (LOOK_ALL, ()):
        look = {k: v.clone().cpu() for k, v in env.lookahead(actions, K, outputs=outs).items()}
        plan = _cpu(env.lookahead_plan(actions[:, None], K, outputs=outs + ("seg_reward",)))
        assert (look["n_steps"].numpy() != K).any() and (look["n_steps"].numpy() == K).any()
        assert np.array_equal(plan["n_steps"].numpy().astype(int), look["n_steps"].numpy().astype(int))
        T.assert_equal({k: plan[k] for k in look if k != "n_steps"}, look, ("H = 1", outs))
        T.assert_equal({"seg_reward": plan["seg_reward"][:, 0]}, {"seg_reward": look["reward"]}, ("H = 1 seg", outs))
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N", [1, 16, 64])
def test_prefix_property(N):
    import torch
    B, M, Hn, K = T.look_ragged(N), 3, 4, 3
    rng = np.random.default_rng(500 + N)
    env = T.look_env(N, B, "random", True)
    T.look_fly(env, rng)
    _place_timeout(env, K)      # (the last env's plans end in segment 1; env 0's plan 0 in segment 0, its plan 2 not at all)
    actions = torch.as_tensor(T.look_draw(rng, M, Hn, B, N), device=env.device)
    _place_plans(actions, M, Hn)
    whole = {k: v.clone().cpu() for k, v in env.lookahead_plan(actions, K, outputs=("seg_reward",)).items()}
    segs = -(-whole["n_steps"].numpy().astype(int) // K)
    ended_by = lambda h: torch.as_tensor((segs < h) | ((segs == h) & whole["done"].numpy().astype(bool)))   # noqa: E731
    assert ended_by(1).any() and ended_by(2).any() and not ended_by(3).all()
    for h in (1, 2, 3):
        part = _cpu(env.lookahead_plan(actions[:, :h].contiguous(), K, outputs=("seg_reward",)))
        T.assert_equal({"seg_reward": part["seg_reward"]}, {"seg_reward": whole["seg_reward"][:, :h].contiguous()}, ("prefix", h))
        mask = ended_by(h)
        T.assert_equal({k: part[k] for k in ("reward", "done", "n_steps")}, whole, ("prefix rows", h), mask=mask)
        assert bool((part["n_steps"][~mask] == h * K).all())
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N", [1, 16, 33])
def test_wide_headings_are_not_evaluated(N):
    import torch
    B, M, Hn, K = T.look_ragged(N), 3, 3, 4
    rng = np.random.default_rng(177 + N)
    env = T.look_env(N, B, "lattice", True)
    T.look_fly(env, rng, steps=40)
    e_wide = B - 1
    env.set_state(e_wide, N - 1, *H.FAR_B[:3], 500.0, H.FAR_B[4])    # 500 deg: beyond the 32-bit heading field
    assert int(env.phi_fix[e_wide * N + N - 1]) == L.I32_MAX
    actions = torch.as_tensor(T.look_draw(rng, M, Hn, B, N), device=env.device)
    actions[1, 0, 3, 0, 2] = 3.0          # candidate 1, env 3: a heading target of 720 deg in segment 0
    actions[2, 1, 4, 0, 2] = 3.0          # candidate 2, env 4: ... in segment 1
    for e in (3, 4):                      # (both envs run into segment 1: aircraft 0 alone under control, far from everything)
        env.env[e, L.ENV_TIMESTEPS] = 5
        env.env[e, L.ENV_MASK_LO] = 1
        env.stats[e, L.STAT_MASK_HI] = 0
        env.set_state(e, 0, *H.FAR_B[:3], 90.0, H.FAR_B[4])
        env.set_last_action(e, 0, [H.FAR_B[4], H.FAR_B[2], 90.0])
    env.synchronize()
    bad = torch.zeros((M, B), dtype=torch.bool)
    bad[:, e_wide] = True
    bad[1, 3] = True
    bad[2, 4] = True
    ref = T.chained_skip_reference(env, actions, K)    # (step_skip evaluates WIDE headings: its rows of `bad` are not compared)
    ref.pop("seg_flags")
    assert int(ref["n_steps"][2, 4]) > K, "env 4 does not reach the segment with the WIDE target"
    snap = H.snapshot(env)
    got = T.guarded_call(env, "plan", actions, K, ALL)
    H.bytes_equal(env, snap)
    swap = lambda d: {k: (v.transpose(1, 2) if k == "seg_reward" else v) for k, v in d.items()}   # noqa: E731  ([M, B, H]: the mask's axes first)
    T.assert_equal(swap(got), swap(ref), "evaluated", mask=~bad)
    for k, v in swap(got).items():
        assert not bool(v[bad].contiguous().view(torch.uint8 if v.dtype == torch.uint8 else torch.int32 if v.dtype == torch.float32 else torch.int16).any()), k
    assert bool((got["n_steps"][~bad] >= 1).all())
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("N", WIDTH_N)
def test_plan_against_the_oracle(N):
    """A second reference, one case per width: chained tests/skip_ref.py calls on the CPU oracle from a snapshot, under the bars of
    tests/bars.py.  M = 2, H = 3, K = 4 under a time limit of 14 steps: envs stop early (asserted)."""
    import torch
    scn, comp, kw, B, seed = _oracle_case(N)
    M, Hn, K = ORACLE_M, ORACLE_H, ORACLE_K
    env = T.skip_env(scn, B, N, True, seed, True, **kw)
    orc = T.skip_oracle(comp, B, N, True, seed, **kw)
    flown, cand = _oracle_inputs(np.random.default_rng(seed), B, N)
    for a, Kf in flown:
        R.skip_reference(orc, a, Kf)
        env.step_skip(a, Kf)
    bars.check_state(env, orc)
    wide0 = R.wide_envs(orc)
    assert not wide0.all()
    ok = ~wide0
    res = env.lookahead_plan(torch.as_tensor(cand, device=env.device), K, outputs=ALL)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    early = 0
    for m, ref in enumerate(_oracle_refs(orc, cand, K)):
        bars.check_candidate_outputs({k: v[m] for k, v in got.items() if k != "seg_reward"}, ref, ok, bars.half_range(comp), tag=(N, m))
        bars.check_plan_segments(got["seg_reward"][m], ref, ok, K, tag=(N, m))
        early += int((ref["n_steps"][ok] < Hn * K).sum())
    assert early > 0
    bars.check_state(env, orc)
    env.close()


def _plans(env):
    """the lookahead_plan calls of both forms that tests/held_tools.py::scripted makes between its calls"""
    import torch
    cand = torch.as_tensor(T.look_draw(np.random.default_rng(10), 3, 3, env.B, env.N), device=env.device)

    def plan():
        env.lookahead_plan(cand, 4, outputs=ALL)
        env.lookahead_plan(cand[:2, :2].contiguous(), 3, outputs=("seg_reward",))
    return plan


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_plans_between_calls_change_nothing():
    import torch
    plain, mixed = T.scripted(), T.scripted(_plans)
    assert len(plain) == len(mixed)
    for j, (a, b) in enumerate(zip(plain, mixed)):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), j
    assert any(bool(t.any()) for t in plain if t.dtype == torch.uint8)    # an episode ended inside the script


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_full_size_batch():
    """65 536 x 16, M = 2, H = 2, K = 4: the first 256 envs against the chain on a 256-env twin, the state bytes of all of them; the envs
    beyond 256 by properties.  (The exact check of the tile decode past one chunk, on every env: tests/test_candidate_tiles.py.)"""
    import torch
    B, N, M, Hn, K = 65536, 16, 2, 2, 4
    rng = np.random.default_rng(3)
    env = T.look_env(N, B, "lattice", True, seed=3, timestep_limit=30)
    small = T.look_env(N, 256, "lattice", True, seed=3, timestep_limit=30)
    a0 = T.look_draw(rng, 3, B, N)
    env.rollout(torch.as_tensor(a0, device=env.device), hold=9)
    small.rollout(torch.as_tensor(a0[:, :256].copy(), device=env.device), hold=9)
    for k in H.STATE:     # envs are independent and the sampler is keyed by the env index: the small env IS the first 256
        rows = 256 * N if getattr(env, k).shape[0] == B * N else 256
        assert torch.equal(getattr(env, k)[:rows], getattr(small, k))
    actions = torch.as_tensor(T.look_draw(rng, M, Hn, B, N), device=env.device)
    ref = T.chained_skip_reference(small, actions[:, :, :256].contiguous(), K)
    ref.pop("seg_flags")
    assert ref["done"].any() and (ref["n_steps"] > K).any()
    snap = H.snapshot(env)
    first = lambda res: {k: (v[:, :, :256] if k == "seg_reward" else v[:, :256]).contiguous().cpu() for k, v in res.items()}   # noqa: E731
    res = env.lookahead_plan(actions, K, outputs=ALL)
    T.assert_equal(first(res), ref, "full size")
    fast = env.lookahead_plan(actions, K, outputs=("seg_reward",))
    T.assert_equal(first(fast), ref, "full size, fast form")
    H.bytes_equal(env, snap)
    n = res["n_steps"]
    assert bool(((n >= 1) & (n <= Hn * K)).all()) and bool((n[res["done"] == 0] == Hn * K).all())
    env.close()
    small.close()
