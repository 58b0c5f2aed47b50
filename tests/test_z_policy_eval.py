"""The policy evaluation (include/atc_step.h: atc_policy_eval; AtcVecEnv.evaluate_policy; atc_hip.evaluate).

CPU: header <-> atc_hip/layout.py <-> ctypes (ATC_EVAL_*, the struct's size and field order, both symbols, ABI 22, LAUNCH_SLOTS 57); one
kernel per (W, K) in the code object; the refusals in their order with atc_last_error() naming the argument, the two of the call's own
and the overlap rule included; refused calls move no launch record; tests/policy_eval_ref.py on a hand-written case and against its
float64 twin.
GPU, bit for bit, on twin envs: the record equals policy_eval_ref folded over rollout_policy_ends' arrays; the state and obs_last equal the
twin's state and obs[-1]; two launches of T / 2 equal one; clear=False adds to the record it is given and clear=True ignores it;
obs_last = NULL changes nothing else; only the call's own launch record moves; an episode that began before the launch counts in full.
test_the_runs_contain_what_they_are_meant_to_test asserts, on what the runs produced, that the events the cases are built for did occur.
(The module's name sorts it behind the existing test modules for the reason given in tests/test_z_policy_ends.py's docstring.)
Per-instantiation coverage — every (W, K) this call is compiled for, each against its oracle — lives in tests/test_z_policy_matrix.py."""
import ctypes as C
import functools
import re
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import policy_eval_ref as V
import policy_ref as P
from atc_hip import layout as L
from held_tools import HEADER, LIB, struct_fields

NAMES = ("atc_policy_eval", "atc_policy_eval_launch_counts")
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
KS = (0, 1, 2, 4)
EVAL_NAMES = ("EPISODES", "WINS", "END_BELOW_MVA", "END_OUTSIDE", "END_CONFLICT", "END_TIMEOUT", "STEPS", "RETURN_SUM", "RETURN_SQ", "RETURN_MIN",
              "RETURN_MAX", "FLAGS_OR", "LAUNCH_STEPS")


# ---------------------------------------------------------------------------------------------------------------- CPU: the ABI
def test_exports_and_one_kernel_per_width_and_k():
    from atc_hip import lib
    assert set(NAMES) <= set(lib.EXPORTS)
    h = lib.load()
    for name in NAMES:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    assert {(int(w), int(k)) for w, k in re.findall(r"\bk_policy_eval<(\d+), (\d+)>\(", text)} == {(w, k) for w in WIDTHS for k in KS}


def test_header_constants_struct_and_argtypes():
    from atc_hip import lib
    text = open(HEADER).read()
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22 and L.LAUNCH_SLOTS == 57
    for i, name in enumerate(EVAL_NAMES):
        assert getattr(L, "EVAL_" + name) == int(re.search(r"\bATC_EVAL_%s = (\d+)," % name, text).group(1)) == i == getattr(V, name), name
    assert L.EVAL_WORDS == int(re.search(r"\bATC_EVAL_WORDS = (\d+)", text).group(1)) == 16 == V.WORDS
    assert L.EVAL_CLEAR == int(re.search(r"#define ATC_EVAL_CLEAR (\d+)u", text).group(1)) == 1
    assert L.POLICY_EVAL_LAUNCH_SLOTS == int(re.search(r"ATC_POLICY_EVAL_LAUNCH_SLOTS = (\d+)", text).group(1)) == 28 == 4 * len(WIDTHS)
    assert (V.F_BELOW_MVA, V.F_OUTSIDE, V.F_WON, V.F_TIMEOUT, V.F_CONFLICT) == (L.F_BELOW_MVA, L.F_OUTSIDE, L.F_WON, L.F_TIMEOUT, L.F_CONFLICT)
    out = struct_fields(text, "atc_policy_eval_out")
    assert out == [["int32_t", "*record"], ["float", "*obs_last"], ["uint32_t", "flags"]]
    assert [f[1].lstrip("*") for f in out] == list(lib.POLICY_EVAL_OUT_FIELDS) == [f[0] for f in lib.AtcPolicyEvalOut._fields_]
    assert [f[1] for f in lib.AtcPolicyEvalOut._fields_] == [C.c_void_p, C.c_void_p, C.c_uint32] and C.sizeof(lib.AtcPolicyEvalOut) == 24
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    decl = re.search(r"^int atc_policy_eval\((.*?)\);", text, flags=re.S | re.M).group(1)
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "B", "N", "T", "hold", "st", "obs0", "pol", "out", "p", "stream"]
    ptr = {"atc_state_t": lib.AtcState, "atc_policy_traffic_t": lib.AtcPolicyTraffic, "atc_policy_eval_out_t": lib.AtcPolicyEvalOut, "atc_params_t": lib.AtcParams}
    want = [ci if a.startswith("int ") else next((C.POINTER(t) for n, t in ptr.items() if n in a), vp) for a in args]
    assert list(h.atc_policy_eval.argtypes) == want and h.atc_policy_eval.restype is ci
    assert lib.LAUNCH_RECORDS["atc_policy_eval_launch_counts"] == (28, lib._width_k0) and callable(lib.policy_eval_launch_counts)
    from atc_hip.vec_env import AtcVecEnv
    import atc_hip
    assert callable(AtcVecEnv.evaluate_policy) and callable(atc_hip.evaluate.summary) and callable(atc_hip.evaluate.evaluate)


def _records():
    from atc_hip import lib
    return lib.launch_records()


def _call(h, T=1, hold=1, B=1, N=1, s=None, st=None, obs0=None, pol=None, out=None, p=None):
    return h.atc_policy_eval(s, B, N, T, hold, st, obs0, pol, out, p, None)


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    err = h.atc_last_error
    at = lambda k: 0x1000000 * (k + 1)      # noqa: E731
    # a zeroed stand-in for the sector handle: the dt check reads its host copy of the constants, nothing else looks inside before a launch
    sector = C.create_string_buffer(1 << 20)
    pol = lib.AtcPolicyTraffic(at(1), 64, 0, 0, 0, 0, 0)
    out = lib.AtcPolicyEvalOut(at(2), None, 0)
    st, p = H.fake_state(), lib.make_params()
    p.mode |= L.M_AUTO_RESET
    p.mode &= ~(L.M_DISCRETE | L.M_ACTIONS_HELD)
    ok = dict(s=C.cast(sector, C.c_void_p), st=C.byref(st), obs0=C.c_void_p(at(7)), pol=C.byref(pol), out=C.byref(out), p=C.byref(p))
    # 1. T and hold, before any pointer is looked at
    for T, hold in ((0, 1), (1, 0), (4, -2)):
        assert _call(h, T, hold) == -1 and b"T >= 1" in err() and b"hold >= 1" in err()
    for T, hold in ((5, 2), (7, 3)):
        assert _call(h, T, hold, **ok) == -1 and b"multiple of hold" in err()
    # 2. the pointers, in atc_rollout_policy_ends' order, out->record where its required outputs stand
    assert _call(h, 6, 3) == -1 and b"null pointer: pol " in err() and b"atc_policy_traffic_t" in err()
    now = lib.AtcPolicyTraffic(None, 7, 0xff, 0, 0, 0, 3)
    assert _call(h, **dict(ok, pol=C.byref(now))) == -1 and b"null pointer: pol->w" in err()
    assert _call(h, **dict(ok, obs0=None, out=None)) == -1 and b"null pointer: obs0" in err()
    assert _call(h, **dict(ok, out=None)) == -1 and b"null pointer: out " in err() and b"atc_policy_eval_out_t" in err()
    bad = lib.AtcPolicyTraffic(at(1), 32, 2, 0, 0, 0, 3)
    o = lib.AtcPolicyEvalOut(None, at(3), 0xff)
    assert _call(h, **dict(ok, out=C.byref(o), pol=C.byref(bad))) == -1 and b"atc_policy_eval_out_t.record" in err()
    # 3. n_hidden, traffic_k, the policy's flag bits — with everything later wrong as well (s NULL, B = 0)
    assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"n_hidden" in err()
    for k in (3, 5, 8, -1):
        bad = lib.AtcPolicyTraffic(at(1), 64, 2, 0, 0, 0, k)
        assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"pol->traffic_k" in err() and b"0, 1, 2 or 4" in err()
    for k in KS:
        bad = lib.AtcPolicyTraffic(at(1), 64, 2, 0, 0, 0, k)
        assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"pol->flags" in err()
    # 4. the argument errors of atc_rollout_hold
    for kw in (dict(s=None), dict(st=None), dict(p=None)):
        assert _call(h, B=0, **dict(ok, **kw)) == -1 and err().endswith(b": null pointer")
    for B, N in ((0, 1), (1, 0), (1, 65)):
        assert _call(h, B=B, N=N, **ok) == -1 and b"B >= 1" in err()
    unknown = lib.AtcPolicyEvalOut(at(2), None, 2)
    q = lib.make_params()
    q.mode = (p.mode | L.M_DISCRETE | L.M_ACTIONS_HELD) & ~L.M_AUTO_RESET
    q.dt = 0.0
    assert _call(h, **dict(ok, p=C.byref(q), out=C.byref(unknown))) == -1 and b"dt must be > 0" in err()
    q.dt = p.dt
    # 5. the mode: DISCRETE, ACTIONS_HELD, then the call's own two — AUTO_RESET missing, unknown bits in out->flags
    assert _call(h, **dict(ok, p=C.byref(q), out=C.byref(unknown))) == -1 and b"ATC_M_DISCRETE" in err()
    q.mode &= ~L.M_DISCRETE
    assert _call(h, **dict(ok, p=C.byref(q), out=C.byref(unknown))) == -1 and b"ATC_M_ACTIONS_HELD" in err()
    q.mode &= ~L.M_ACTIONS_HELD
    assert _call(h, **dict(ok, p=C.byref(q), out=C.byref(unknown))) == -1 and b"ATC_M_AUTO_RESET is required" in err()
    assert _call(h, **dict(ok, out=C.byref(unknown))) == -1 and b"atc_policy_eval_out_t.flags has unknown bits" in err()
    # 6. the overlap rule (B = 3, N = 5: record 192 bytes, obs_last and obs0 600; st->env 48 bytes at 0x500000, st->ac 240 at 0x200000)
    shape = dict(B=3, N=5)
    for rec, last, a, b in ((at(7) + 599, None, b"out->record", b"obs0"), (at(7) - 191, None, b"out->record", b"obs0"), (at(2), at(2) + 191, b"out->record", b"out->obs_last"),
                            (at(2), at(7) + 599, b"out->obs_last", b"obs0"), (0x500000 + 47, None, b"out->record", b"st->env"), (at(2), 0x200000 - 599, b"out->obs_last", b"st->ac"),
                            (0x600000 + 95, None, b"out->record", b"st->stats"), (at(2), 0x700000 + 479, b"out->obs_last", b"st->phi_wide")):
        o = lib.AtcPolicyEvalOut(rec, last, L.EVAL_CLEAR)
        assert _call(h, **dict(ok, out=C.byref(o), **shape)) == -1 and b"overlaps" in err() and a in err() and b in err(), (hex(rec), err())
    assert _records() == before, "a refused call moved a launch record"


def test_launch_record_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    buf = (C.c_uint64 * 30)(*([99] * 30))
    assert h.atc_policy_eval_launch_counts(buf, 30) == 0
    assert all(v != 99 for v in buf[:28]) and all(v == 99 for v in buf[28:])
    assert h.atc_policy_eval_launch_counts(None, 1) == -1
    assert isinstance(lib.policy_eval_launch_counts(), dict)


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatement
def test_policy_eval_ref_on_a_hand_case():
    """hold plays no part in the record: two ends of env 0 at steps 1 and 2 (one held block of a caller), a carried-in episode, a carried-in record"""
    Wn, Tm, Cf, Mv = V.F_WON, V.F_TIMEOUT, V.F_CONFLICT, V.F_BELOW_MVA
    reward = np.array([[1.5, -1.0], [2.0, 0.25], [-4.0, 0.5], [8.0, 0.125]], np.float32)
    done = np.array([[0, 0], [1, 0], [1, 0], [0, 0]], np.uint8)
    flags = np.zeros((4, 2, 2), np.uint16)
    flags[1, 0] = [Tm, Tm | 256]
    flags[2, 0] = [Cf | Mv, 16]
    flags[3, 1] = [Wn, 0]                     # env 1: aircraft 0 handed over, no end
    carried = V.initial(2)
    carried[0, :7] = [10, 3, 1, 0, 2, 4, 70]
    cf = carried.view(np.float32)
    cf[0, V.RETURN_SUM], cf[0, V.RETURN_SQ], cf[0, V.RETURN_MIN], cf[0, V.RETURN_MAX] = 100.0, 2000.0, -7.0, 31.0
    carried[0, V.FLAGS_OR], carried[0, V.LAUNCH_STEPS], carried[0, 13:] = 0x200, 90, (0, 0, 0)
    rec = V.fold(reward, done, flags, t0=[5, 2], r0=[10.0, -3.0], record=carried)
    w = V.words(rec)
    # env 0: the carried episode ends at step 1 with length 5 + 2 and return 10 + 1.5 + 2 (a time limit), the next at step 2 with length 1 and return -4
    assert [int(w[n][0]) for n in ("episodes", "wins", "end_below_mva", "end_outside", "end_conflict", "end_timeout", "steps")] == [12, 3, 2, 0, 3, 5, 78]
    assert (float(w["return_sum"][0]), float(w["return_sq"][0]), float(w["return_min"][0]), float(w["return_max"][0])) == (100.0 + 13.5 - 4.0, 2000.0 + 182.25 + 16.0, -7.0, 31.0)
    assert int(w["flags_or"][0]) == 0x200 | Tm | 256 | Cf | Mv | 16 and int(w["launch_steps"][0]) == 94
    # env 1: no end — the cleared record's values, MIN / MAX +-inf
    assert [int(w[n][1]) for n in ("episodes", "wins", "steps", "flags_or", "launch_steps")] == [0, 0, 0, Wn, 4]
    assert float(w["return_min"][1]) == np.inf and float(w["return_max"][1]) == -np.inf and float(w["return_sum"][1]) == 0.0
    # a win: the only aircraft under control is handed over and the env ends (mask0); keep_active: any F_WON at the ending step
    done[3, 1] = 1
    assert V.words(V.fold(reward, done, flags, [0, 0], [0.0, 0.0], mask0=[3, 1]))["wins"].tolist() == [0, 1]
    assert V.words(V.fold(reward, done, flags, [0, 0], [0.0, 0.0], mask0=[3, 3]))["wins"].tolist() == [0, 0]
    assert V.words(V.fold(reward, done, flags, [0, 0], [0.0, 0.0], keep_active=True))["wins"].tolist() == [0, 1]
    # two halves on one record equal the whole
    first = V.fold(reward[:2], done[:2], flags[:2], [5, 2], [10.0, -3.0], record=carried)
    second = V.fold(reward[2:], done[2:], flags[2:], [0, 4], [0.0, np.float32(np.float32(-3.0 - 1.0) + np.float32(0.25))], record=first)
    assert np.array_equal(second, V.fold(reward, done, flags, [5, 2], [10.0, -3.0], record=carried))


def test_policy_eval_ref_float32_sums_against_the_float64_twin():
    """RETURN_SUM and RETURN_SQ of the restatement against float64 sums over the SAME float32 returns (the restatement's own, through
    returns=): n sequential float32 adds of n terms err by at most n u sum|term| (u = 2^-24), so |SUM - twin| <= n u sum|r|; the squares are
    each rounded once more, u r^2 apiece, so |SQ - twin| <= (n + 1) u sum r^2.  Each return itself — a running float32 sum over the
    episode's m steps — is held to the float64 sum of its rewards within m u sum|reward|.  Values carried in take part like any term."""
    rng = np.random.default_rng(11)
    T, B = 400, 6
    reward = rng.normal(0.0, 50.0, (T, B)).astype(np.float32)
    done = (rng.random((T, B)) < 0.1).astype(np.uint8)
    flags = np.zeros((T, B, 1), np.uint16)
    u = 2.0 ** -24
    for carried in (None, V.fold(reward[:50], done[:50], flags[:50], np.zeros(B, int), np.zeros(B))):
        rets = []
        a32 = V.words(V.fold(reward, done, flags, np.zeros(B, int), np.zeros(B), record=carried, returns=rets))
        c = V.words(V.initial(B) if carried is None else carried)
        for e in range(B):
            ends = np.flatnonzero(done[:, e])
            mine = [(m, r) for env, m, r in rets if env == e]
            assert len(mine) == len(ends) > 5 and all(isinstance(r, np.float32) for _, r in mine)
            for i, (m, r) in enumerate(mine):
                first = ends[i - 1] + 1 if i else 0
                steps = reward[first:ends[i] + 1, e].astype(np.float64)
                assert m == len(steps) and abs(float(r) - steps.sum()) <= m * u * np.abs(steps).sum(), (e, i)
            r64 = np.array([float(r) for _, r in mine])
            had = int(c["episodes"][e])
            n = len(r64) + (1 if had else 0)          # the carried sum is one more term
            s0, q0 = float(c["return_sum"][e]), float(c["return_sq"][e])
            err_sum = abs(float(a32["return_sum"][e]) - (s0 + r64.sum()))
            err_sq = abs(float(a32["return_sq"][e]) - (q0 + (r64 ** 2).sum()))
            bound_sum = n * u * (abs(s0) + np.abs(r64).sum())
            bound_sq = (n + 1) * u * (q0 + (r64 ** 2).sum())
            print(e, "sum", err_sum, "<=", bound_sum, " sq", err_sq, "<=", bound_sq)
            assert err_sum <= bound_sum and err_sq <= bound_sq, (e, err_sum, bound_sum, err_sq, bound_sq)
            assert float(a32["return_min"][e]) == min(r64.min(), float(c["return_min"][e])) and float(a32["return_max"][e]) == max(r64.max(), float(c["return_max"][e]))
            assert int(a32["episodes"][e]) == had + len(ends) and int(a32["steps"][e]) == int(c["steps"][e]) + ends[-1] + 1
    # the all-float64 fold (dtype=) is the same fold: its integer words agree
    a64 = V.fold(reward, done, flags, np.zeros(B, int), np.zeros(B), dtype=np.float64)
    assert np.array_equal(a64["ints"][:, :7], V.fold(reward, done, flags, np.zeros(B, int), np.zeros(B)).astype(np.int64)[:, :7])


# ---------------------------------------------------------------------------------------------------------------- GPU
T = 48
SEED, DECISION0 = 0x1234567890ABCDEF, 0xFFFFFFFA
# (B, N, timestep_limit, hold, K, deterministic)
CASES = ((5, 3, 7, 1, 0, False), (5, 3, 5, 8, 1, True), (3, 16, 7, 4, 2, False), (2, 64, 7, 4, 4, True), (300, 1, 7, 3, 0, False), (2, 2, 6000, 1, 0, True))
JUNK = 0x5A5A5A5A


def _make(B, N, tl):
    if tl == 6000:      # the set-up of test_z_policy_ends.py's hand-over test, aircraft 1 of env 0 out of control: aircraft 0's hand-over wins env 0
        from atc_hip.vec_env import AtcVecEnv
        from envs.atc import model, scenarios
        env = AtcVecEnv(B, N, sim_parameters=model.SimParameters(1), scenario=scenarios.LOWW(random_entrypoints=True), auto_reset=True, seed=3, timestep_limit=tl)
        for e in range(B):
            env.set_state(e, 0, 48.9, 31.9, 3300.0, 345.0, 200.0)
            env.set_state(e, 1, 20.0, 60.0, 15000.0, 90.0, 250.0)
        env.env[0, L.ENV_MASK_LO] &= ~0b10
    else:
        env = H.policy_env(dict(normalize=True, shaping=True, auto_reset=True, timestep_limit=tl, spawn="lattice"), B, N)
        if N > 32:
            env.stats[1, L.STAT_MASK_HI] = 0          # env 1 flies its low 32 aircraft only: the high mask word
    env.observe()
    env.synchronize()
    return env


def _weights(tl, K, device):
    import torch
    if tl == 6000:      # a constant policy (W3 = 0, b3 = the targets) that flies aircraft 0 into the final-approach corridor
        parts = P.split(P.random_weights(np.random.default_rng(5), 1.0, (0.0, 0.0, 0.0), True))
        parts["b3"] = np.array([0.0, 2 * 2700.0 / 38000.0 - 1, 2 * 345.0 / 360.0 - 1], np.float32)
        return torch.as_tensor(P.pack(*[parts[n] for n, _ in P.SHAPES]), device=device)
    return torch.as_tensor(P.random_weights(np.random.default_rng([17, K]), 1.0, (-0.5, -1.0, 0.25), False, K), device=device)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _run(B, N, tl, hold, K, det):
    import torch
    from atc_hip import lib
    A, Bv = _make(B, N, tl), _make(B, N, tl)
    for k in H.STATE + ("obs",):
        assert torch.equal(getattr(A, k), getattr(Bv, k)), k
    snap, obs0 = H.snapshot(A), A.obs.clone()
    w = _weights(tl, K, A.device)
    kw = dict(traffic=K, hold=hold, seed=SEED, deterministic=det)
    state = lambda env: {k: getattr(env, k).cpu().numpy() for k in H.STATE}      # noqa: E731
    res = dict(mask0=[int(m) for m in A.active_mask.cpu().numpy()], env0=A.env.cpu().numpy().copy(), win_bits0=A.stats[:, L.STAT_WIN_BITS].cpu().numpy().copy())
    # 1, 2, 6: one launch of T on A; rollout_policy_ends on the twin
    before = lib.launch_records()
    full = A.evaluate_policy(w, T, decision0=DECISION0, obs0=obs0, **kw)
    A.synchronize()
    after = lib.launch_records()
    res["gained"] = {g: {k: v - before[g].get(k, 0) for k, v in after[g].items() if v != before[g].get(k, 0)} for g in after}
    res["gained"] = {g: v for g, v in res["gained"].items() if v}
    assert torch.equal(obs0, Bv.obs), "evaluate_policy wrote to the obs0 it was given"
    res["full"], res["stA"] = _np(full), state(A)
    twin = Bv.rollout_policy_ends(w, T, K, hold=hold, seed=SEED, decision0=DECISION0, deterministic=det, obs0=obs0.clone())
    Bv.synchronize()
    res["twin"], res["stB"] = _np({k: twin[k] for k in ("obs", "reward", "done", "flags")}), state(Bv)
    # 3: two launches of T / 2 on one record
    H.restore(A, snap)
    h = T // 2
    first = A.evaluate_policy(w, h, decision0=DECISION0, obs0=obs0, **kw)
    res["first"], res["st_first"] = _np(first), state(A)
    second = A.evaluate_policy(w, h, decision0=DECISION0 + h // hold, obs0=first["obs_last"], record=first["record"].clone(), clear=False, **kw)
    A.synchronize()
    res["halves"], res["st_halves"] = _np(second), state(A)
    # 4: clear=False on a record holding the first run's words; clear=True on a record full of junk
    H.restore(A, snap)
    carried = A.evaluate_policy(w, T, decision0=DECISION0, obs0=obs0, record=full["record"].clone(), clear=False, **kw)
    H.restore(A, snap)
    junk = A.evaluate_policy(w, T, decision0=DECISION0, obs0=obs0, record=torch.full((B, L.EVAL_WORDS), JUNK, dtype=torch.int32, device=A.device), clear=True, **kw)
    A.synchronize()
    res["carried"], res["junk"] = _np(carried), _np(junk)
    # 5: obs_last = NULL, through the library itself
    H.restore(A, snap)
    rec = torch.full((B, L.EVAL_WORDS), JUNK, dtype=torch.int32, device=A.device)
    x0 = obs0.clone()
    o = lib.AtcPolicyEvalOut(A._ptr(rec), None, L.EVAL_CLEAR)
    pol = lib.AtcPolicyTraffic(A._ptr(w), L.POLICY_HIDDEN, L.POLICY_DETERMINISTIC if det else 0, SEED, DECISION0, 0, K)
    with torch.cuda.device(A.device):
        lib.check(lib.load().atc_policy_eval(A.sector.handle, B, N, T, hold, C.byref(A._state), A._ptr(x0), C.byref(pol), C.byref(o), C.byref(A.params), A._stream()))
    A.synchronize()
    res["no_last"], res["st_no_last"] = rec.cpu().numpy(), state(A)
    # 7: episodes that began before the launch — three steps of rollout() on both, then the evaluation against the twin's arrays
    for env in (A, Bv):
        H.restore(env, snap)
    zeros = torch.zeros((3, B, N, 3), dtype=torch.float32, device=A.device)
    pre = [env.rollout(zeros.clone()) for env in (A, Bv)]
    A.synchronize()
    assert torch.equal(pre[0]["obs"], pre[1]["obs"])
    res["env3"], res["mask3"] = A.env.cpu().numpy().copy(), [int(m) for m in A.active_mask.cpu().numpy()]
    x3 = pre[0]["obs"][-1].clone()
    late = A.evaluate_policy(w, T, decision0=DECISION0, obs0=x3, **kw)
    twin3 = Bv.rollout_policy_ends(w, T, K, hold=hold, seed=SEED, decision0=DECISION0, deterministic=det, obs0=x3.clone())
    A.synchronize()
    res["late"], res["twin3"] = _np(late), _np({k: twin3[k] for k in ("obs", "reward", "done", "flags")})
    res["st_late"], res["st_twin3"] = state(A), state(Bv)
    for env in (A, Bv):
        env.close()
    return res


def _fold(arrays, env_words, mask0, record=None):
    t0 = env_words[:, L.ENV_TIMESTEPS]
    r0 = np.ascontiguousarray(env_words[:, L.ENV_TOTAL_REWARD]).view(np.float32)
    return V.fold(arrays["reward"], arrays["done"], arrays["flags"], t0, r0, record=record, mask0=mask0)


_cases = pytest.mark.parametrize("B,N,tl,hold,K,det", CASES, ids=["%dx%d-limit%d-hold%d-K%d-%s" % (c[:5] + ("mean" if c[5] else "drawn",)) for c in CASES])


def _same(a, b):
    return np.array_equal(H.bits(a), H.bits(b))


@pytest.mark.gpu
@_cases
def test_record_state_and_obs_last_bit_for_bit(B, N, tl, hold, K, det):
    r = _run(B, N, tl, hold, K, det)
    tag = (B, N, tl, hold, K, det)
    full, twin = r["full"], r["twin"]
    # 1. the record: the restatement folded over rollout_policy_ends' arrays on the twin
    want = _fold(twin, r["env0"], r["mask0"])
    for e in range(min(B, 8)):
        print(tag, e, {n: v[e] for n, v in V.words(full["record"]).items()})
    assert np.array_equal(full["record"], want), (tag, np.argwhere(full["record"] != want)[:8])
    assert np.all(full["record"][:, 13:] == 0) and np.all(full["record"][:, L.EVAL_LAUNCH_STEPS] == T)
    # ... and WINS is what the step shifted into the per-episode record
    rec = V.words(full["record"])
    few = (r["win_bits0"] == 0) & (rec["episodes"] <= 10)
    pop = np.array([bin(int(v) & 0x3ff).count("1") for v in r["stA"]["stats"][:, L.STAT_WIN_BITS]])
    assert few.any() and np.array_equal(rec["wins"][few], pop[few]), tag
    # 2. the state and obs_last: the twin's state and obs[-1]
    for k in H.STATE:
        assert _same(r["stA"][k], r["stB"][k]), (tag, k)
    assert _same(full["obs_last"].reshape(-1), twin["obs"][-1].reshape(-1)), tag
    # 3. two launches of T / 2 equal one launch of T
    assert np.array_equal(r["halves"]["record"], full["record"]), (tag, np.argwhere(r["halves"]["record"] != full["record"])[:8])
    assert _same(r["halves"]["obs_last"], full["obs_last"]), tag
    assert _same(r["first"]["obs_last"].reshape(-1), twin["obs"][T // 2 - 1].reshape(-1)), tag
    for k in H.STATE:
        assert _same(r["st_halves"][k], r["stA"][k]), (tag, "halves", k)
    # 4. clear=False adds to what the record holds; clear=True ignores it
    assert np.array_equal(r["carried"]["record"], _fold(twin, r["env0"], r["mask0"], record=full["record"])), tag
    assert np.all(r["carried"]["record"][:, L.EVAL_LAUNCH_STEPS] == 2 * T)
    assert np.array_equal(r["junk"]["record"], full["record"]), tag
    # 5. obs_last = NULL leaves the record and the state as they are
    assert np.array_equal(r["no_last"], full["record"]), tag
    for k in H.STATE:
        assert _same(r["st_no_last"][k], r["stA"][k]), (tag, "obs_last NULL", k)
    # 6. only the call's own launch record moved, by one
    assert r["gained"] == {"atc_policy_eval_launch_counts": {(H.lane_width(N), K): 1}}, (tag, r["gained"])
    # 7. an episode that began before the launch counts in full
    assert (r["env3"][:, L.ENV_TIMESTEPS] == 3).any()
    assert np.array_equal(r["late"]["record"], _fold(r["twin3"], r["env3"], r["mask3"])), tag
    for k in H.STATE:
        assert _same(r["st_late"][k], r["st_twin3"][k]), (tag, "late", k)
    assert _same(r["late"]["obs_last"].reshape(-1), r["twin3"]["obs"][-1].reshape(-1)), tag


@pytest.mark.gpu
def test_the_runs_contain_what_they_are_meant_to_test():
    seen = set()
    for c in CASES:
        B, N, tl, hold, K, det = c
        r = _run(*c)
        done = r["twin"]["done"] != 0
        flags = r["twin"]["flags"].view(np.uint16)
        rec = V.words(r["full"]["record"])
        seen_or = np.bitwise_or.reduce(flags, axis=2)
        hard = V.F_BELOW_MVA | V.F_OUTSIDE | V.F_CONFLICT
        if hold > 1 and (done.reshape(T // hold, hold, B).sum(axis=1) >= 2).any():
            seen.add("two ends inside one block")
        if (done & ((seen_or & V.F_TIMEOUT) == 0)).any():
            seen.add("an end that is not a time limit")
        if (done & ((seen_or & V.F_TIMEOUT) != 0) & ((seen_or & hard) == 0)).any():
            seen.add("a time-limit end")
        if (rec["wins"] > 0).any():
            seen.add("a win")
        none = rec["episodes"] == 0
        if none.any() and np.all(rec["return_min"][none] == np.inf) and np.all(rec["return_max"][none] == -np.inf):
            seen.add("an env with no end: MIN / MAX stay +-inf")
        if ((r["st_first"]["env"][:, L.ENV_TIMESTEPS] > 0) & done[T // 2:].any(axis=0)).any():
            seen.add("an episode carried across the T / 2 split")
        if N > 32 and (r["mask0"][1] >> 32) == 0 and (r["mask0"][0] >> 32) != 0:
            seen.add("the high mask word")
    want = {"two ends inside one block", "an end that is not a time limit", "a time-limit end", "a win", "an env with no end: MIN / MAX stay +-inf",
            "an episode carried across the T / 2 split", "the high mask word"}
    assert seen == want, want - seen


@pytest.mark.gpu
def test_summary_against_numpy_float64():
    import torch
    from atc_hip import evaluate
    recs = np.concatenate([_run(*c)["carried"]["record"] for c in CASES[:3]])
    got = evaluate.summary(torch.as_tensor(recs).cuda())
    w = V.words(recs)
    n = int(w["episodes"].astype(np.int64).sum())
    assert n > 0 and got["episodes"] == n and got["steps"] == int(w["launch_steps"].astype(np.int64).sum())
    s, sq = w["return_sum"].astype(np.float64).sum(), w["return_sq"].astype(np.float64).sum()
    want = {"win_ratio": w["wins"].astype(np.int64).sum() / n, "mean_return": s / n, "std_return": np.sqrt(max(sq / n - (s / n) ** 2, 0.0)),
            "min_return": float(w["return_min"].min()), "max_return": float(w["return_max"].max()), "mean_length": w["steps"].astype(np.int64).sum() / n}
    for name in ("below_mva", "outside", "conflict", "timeout"):
        want["end_" + name] = w["end_" + name].astype(np.int64).sum() / n
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12 * max(1.0, abs(v)), (k, got[k], v)
    assert got["flags_or"] == int(np.bitwise_or.reduce(w["flags_or"].view(np.uint32)))
    assert all(isinstance(v, (int, float)) for v in got.values())
    empty = evaluate.summary(torch.as_tensor(V.initial(3)).cuda())
    assert empty["episodes"] == 0 and np.isnan(empty["win_ratio"]) and empty["min_return"] == np.inf and empty["max_return"] == -np.inf


@pytest.mark.gpu
def test_evaluate_runs_until_every_env_has_its_episodes():
    import torch
    from atc_hip import evaluate
    B, N, tl, hold, K = 5, 3, 7, 2, 0
    A, Bv = _make(B, N, tl), _make(B, N, tl)
    w = _weights(tl, K, A.device)
    summ, rec = evaluate.evaluate(A, w, episodes_per_env=2, chunk=6, hold=hold, seed=SEED, decision0=DECISION0, deterministic=False)
    assert int(rec[:, L.EVAL_EPISODES].min()) >= 2
    total = int(rec[0, L.EVAL_LAUNCH_STEPS])
    assert total % 6 == 0 and torch.all(rec[:, L.EVAL_LAUNCH_STEPS] == total) and summ == evaluate.summary(rec)
    # one chunk earlier some env had not finished two: the loop stopped at the first chunk that could
    one = Bv.evaluate_policy(w, total, hold=hold, seed=SEED, decision0=DECISION0, deterministic=False)
    assert torch.equal(one["record"], rec)
    for k in H.STATE:
        assert _same(getattr(A, k).cpu().numpy(), getattr(Bv, k).cpu().numpy()), k
    # max_steps ends it early, on a chunk boundary
    H.restore(A, H.snapshot(Bv))
    summ2, rec2 = evaluate.evaluate(A, w, episodes_per_env=10 ** 6, chunk=6, max_steps=20, hold=hold)
    assert summ2["steps"] == B * 18 and int(rec2[:, L.EVAL_EPISODES].min()) < 10 ** 6
    A.close()
    Bv.close()
