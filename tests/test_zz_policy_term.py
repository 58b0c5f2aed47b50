"""The policy rollout with terminal traffic records (include/atc_step.h: atc_rollout_policy_term; AtcVecEnv.rollout_policy_term) and
atc_hip.ppo.collect_bootstrap_traffic.

CPU: the symbol and exactly the 21 instantiations k_rollout_policy_term<W, K>; header <-> atc_hip/layout.py <-> ctypes, ABI 22; every refusal
through ctypes in the header's order with made-up pointers — the time increment comes last, so the overlap rule of term_traffic is reached
without a sector —; the Python refusals ahead of any library call; collect_bootstrap_traffic on a stand-in env: the row layout of the one
forward, the split into values / boot, boot read only where trunc is set.
GPU, bit for bit, one case per (W, K) on tests/policy_term_tools.py's rig: every other output and the state equal rollout_policy_ends(traffic=K)
on a twin env, with term_traffic given and NULL; term_traffic equals observe_traffic() on the terminal state, obtained from envs the call never
touched; rows of blocks that did not end keep the sentinel; the call without auto-reset likewise; two launches of T / 2 equal one; out=
allocates nothing; touching ranges pass and one byte of overlap is refused; collect_bootstrap_traffic equals the calls written out by hand,
its ret differs from collect(traffic=K)'s exactly where a truncation reaches, and one ppo.update on its dict equals update on the
hand-assembled dict.  test_the_runs_contain_what_they_are_meant_to_test asserts per width the events the rig is built for.
(Sorted behind the other modules on purpose, like tests/test_z_policy_ends.py.)"""
import ctypes as C
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import helpers as H
import policy_ends_ref as E
import policy_term_tools as TT
from atc_hip import layout as L
from held_tools import HEADER, LIB, struct_fields

FAKE = C.c_void_p(0x100000)
WIDTHS, KS = TT.WIDTHS, TT.KS
EVENTS = {"an end on a block's first step", "an end on a block's middle step", "an end on a block's last step", "a pure time-limit end",
          "an end by another cause", "an aircraft not under control at its end"}


# ---------------------------------------------------------------------------------------------------------------- CPU: the ABI
def test_export_and_exactly_21_instantiations():
    from atc_hip import lib
    names = ("atc_rollout_policy_term", "atc_rollout_policy_term_launch_counts")
    assert set(names) <= set(lib.EXPORTS)
    h = lib.load()
    for name in names:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    found = sorted((int(w), int(k)) for w, k in set(re.findall(r"\bk_rollout_policy_term<(\d+), (\d+)>\(", text)))
    assert found == sorted((w, k) for w in WIDTHS for k in KS) and len(found) == 21


def test_header_layout_and_ctypes_agree():
    from atc_hip import lib
    text = open(HEADER).read()
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22
    assert L.ROLLOUT_POLICY_TERM_LAUNCH_SLOTS == int(re.search(r"ATC_ROLLOUT_POLICY_TERM_LAUNCH_SLOTS = (\d+)", text).group(1)) == 21 == len(WIDTHS) * len(KS)
    out = struct_fields(text, "atc_policy_term_out")
    assert all(f[1].startswith("*") for f in out)
    assert [f[1].lstrip("*") for f in out] == list(lib.POLICY_TERM_OUT_FIELDS) == [f[0] for f in lib.AtcPolicyTermOut._fields_]
    assert lib.POLICY_TERM_OUT_FIELDS == lib.POLICY_ENDS_OUT_FIELDS + ("term_traffic",)
    assert [tuple(f) for f in out[:10]] == [tuple(f) for f in struct_fields(text, "atc_policy_ends_out")]      # atc_policy_ends_out_t's fields, then the pointer
    assert out[10][0] == "float" and C.sizeof(lib.AtcPolicyTermOut) == 88
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    decl = re.search(r"^int atc_rollout_policy_term\((.*?)\);", text, flags=re.S | re.M).group(1)
    ends = re.search(r"^int atc_rollout_policy_ends\((.*?)\);", text, flags=re.S | re.M).group(1)
    strip = lambda d: [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", d, flags=re.S).split(",")]      # noqa: E731
    args = strip(decl)
    assert args == [a.replace("atc_policy_ends_out_t", "atc_policy_term_out_t") for a in strip(ends)]      # atc_rollout_policy_ends' argument list
    ptr = {"atc_state_t": lib.AtcState, "atc_policy_traffic_t": lib.AtcPolicyTraffic, "atc_policy_term_out_t": lib.AtcPolicyTermOut, "atc_params_t": lib.AtcParams}
    want = [ci if a.startswith("int ") else next((C.POINTER(t) for n, t in ptr.items() if n in a), vp) for a in args]
    assert list(h.atc_rollout_policy_term.argtypes) == want and h.atc_rollout_policy_term.restype is ci
    slots, name = lib.LAUNCH_RECORDS["atc_rollout_policy_term_launch_counts"]
    assert slots == 21 and [name(s) for s in (0, 1, 2, 3, 20)] == [(1, 1), (1, 2), (1, 4), (2, 1), (64, 4)]
    # a record of its own: the existing records keep their slot counts
    assert lib.LAUNCH_RECORDS["atc_rollout_policy_ends_launch_counts"][0] == 28 and lib.LAUNCH_RECORDS["atc_rollout_policy_traffic_launch_counts"][0] == 21
    buf = (C.c_uint64 * 23)(*([99] * 23))
    assert h.atc_rollout_policy_term_launch_counts(buf, 23) == 0 and all(v != 99 for v in buf[:21]) and buf[21] == buf[22] == 99
    assert h.atc_rollout_policy_term_launch_counts(None, 1) == -1 and isinstance(lib.rollout_policy_term_launch_counts(), dict)


def _call(h, T=1, hold=1, B=1, N=1, s=None, st=None, obs0=None, pol=None, out=None, p=None):
    return h.atc_rollout_policy_term(s, B, N, T, hold, st, obs0, pol, out, p, None)


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = lib.launch_records()
    err = h.atc_last_error
    at = lambda k: 0x1000000 * (k + 1)      # noqa: E731
    pol = lib.AtcPolicyTraffic(at(1), 64, 0, 0, 0, 0, 2)
    out = lib.AtcPolicyTermOut(at(2), at(3), at(4), at(5), at(6), None, None, None, None, None, None)
    st, p = H.fake_state(), lib.make_params()
    ok = dict(s=FAKE, st=C.byref(st), obs0=C.c_void_p(at(7)), pol=C.byref(pol), out=C.byref(out), p=C.byref(p))
    # 1. T and hold, before any pointer is looked at
    for T, hold in ((0, 1), (1, 0), (4, -2)):
        assert _call(h, T, hold) == -1 and b"T >= 1" in err() and b"hold >= 1" in err()
    assert _call(h, 5, 2, **ok) == -1 and b"multiple of hold" in err()
    # 2. the pointers, in atc_rollout_policy_ends' order
    assert _call(h, 6, 3) == -1 and b"null pointer: pol " in err() and b"atc_policy_traffic_t" in err()
    now = lib.AtcPolicyTraffic(None, 7, 0xff, 0, 0, 0, 3)
    assert _call(h, **dict(ok, pol=C.byref(now))) == -1 and b"null pointer: pol->w" in err()
    assert _call(h, **dict(ok, obs0=None, out=None)) == -1 and b"null pointer: obs0" in err()
    assert _call(h, **dict(ok, out=None)) == -1 and b"null pointer: out " in err() and b"atc_policy_term_out_t" in err()
    for k in range(4):
        o = lib.AtcPolicyTermOut(*[None if j == k else at(2 + j) for j in range(4)], None, None, None, None, None, None, at(9))
        assert _call(h, **dict(ok, out=C.byref(o))) == -1 and b"atc_policy_term_out_t.obs, .reward, .done and .flags" in err()
    o = lib.AtcPolicyTermOut(at(2), at(3), at(4), at(5), None, at(6), None, None, None, None, at(9))
    bad = lib.AtcPolicyTraffic(at(1), 32, 2, 0, 0, 0, 3)
    assert _call(h, **dict(ok, out=C.byref(o), pol=C.byref(bad))) == -1 and b"atc_policy_term_out_t.action" in err()
    # 3. n_hidden, traffic_k (0 refused as well), the flag bits — with everything later wrong as well (s NULL, B = 0)
    assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"n_hidden" in err()
    for k in (0, 3, 5, 8, -1):
        bad = lib.AtcPolicyTraffic(at(1), 64, 2, 0, 0, 0, k)
        assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"pol->traffic_k must be 1, 2 or 4" in err()
    for k in KS:
        bad = lib.AtcPolicyTraffic(at(1), 64, 2, 0, 0, 0, k)
        assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"pol->flags" in err()
    # 4. the argument errors of atc_rollout_hold that need no sector, then the mode
    for kw in (dict(s=None), dict(st=None), dict(p=None)):
        assert _call(h, B=0, **dict(ok, **kw)) == -1 and err().endswith(b": null pointer")
    for B, N in ((0, 1), (1, 0), (1, 65)):
        assert _call(h, B=B, N=N, **ok) == -1 and b"B >= 1" in err()
    null_field = H.fake_state()
    null_field.alt = None
    assert _call(h, **dict(ok, st=C.byref(null_field))) == -1 and b"null field" in err()
    for bit, word in ((L.M_DISCRETE, b"ATC_M_DISCRETE"), (L.M_ACTIONS_HELD, b"ATC_M_ACTIONS_HELD")):
        pm = lib.make_params()
        pm.mode |= bit
        pm.dt = -1.0      # (the time increment is wrong as well: it comes last)
        assert _call(h, **dict(ok, p=C.byref(pm))) == -1 and word in err()
    # 5. atc_rollout_policy_ends' overlap rule, then term_traffic's — B = 3, N = 5, T = 8, hold = 2, K = 2: D = 4, term_traffic 3840 bytes
    shape = dict(B=3, N=5, T=8, hold=2)
    bn, t, d, K = 15, 8, 4, 2
    size = d * bn * K * 32
    sizes = {"pol->w": L.policy_words(K) * 4, "obs0": bn * 40, "out->obs": t * bn * 40, "out->reward": t * 3 * 4, "out->done": t * 3, "out->flags": t * bn * 2,
             "out->action": d * bn * 12, "out->logp": d * bn * 4, "out->traffic": size, "out->term_obs": d * bn * 40, "out->term_flags": d * 3 * 2,
             "out->control": d * bn, "st->ac": bn * 16, "st->alt": bn * 8, "st->last_act": bn * 16, "st->env": 3 * L.ENV_WORDS * 4, "st->stats": 3 * L.STAT_WORDS * 4,
             "st->phi_wide": bn * 32}
    where = {"pol->w": at(1), "obs0": at(7), "out->obs": at(2), "out->reward": at(3), "out->done": at(4), "out->flags": at(5), "out->action": at(6), "out->logp": at(10),
             "out->traffic": at(11), "out->term_obs": at(12), "out->term_flags": at(13), "out->control": at(14)}
    where.update({"st->" + n: getattr(st, n) for n in ("ac", "alt", "last_act", "env", "stats", "phi_wide")})
    assert set(where) == set(sizes) and len(sizes) == 18
    bad_dt = lib.make_params()
    bad_dt.dt = -1.0

    def placed(term_traffic, **swap):
        o = lib.AtcPolicyTermOut(at(2), at(3), at(4), at(5), at(6), at(10), at(11), at(12), at(13), at(14), term_traffic)
        for k, v in swap.items():
            setattr(o, k, v)
        return _call(h, **dict(ok, out=C.byref(o), p=C.byref(bad_dt), **shape))
    assert placed(at(20), term_obs=at(11) + size - 1) == -1 and b"out->term_obs overlaps out->traffic" in err()      # the older rule comes first
    for name, base in where.items():
        for ptr in (base - size + 1, base, base + sizes[name] - 1):      # one byte at either end, and the same start
            assert placed(ptr) == -1 and b"overlaps" in err() and b"out->term_traffic" in err() and name.encode() in err(), (name, err())
        for ptr in (base - size, base + sizes[name]):      # ranges that only touch pass the rule: refused by what comes LAST, the time increment
            assert placed(ptr) == -1 and b"dt must be > 0" in err(), (name, err())
    # 6. the time increment, last — with term_traffic NULL as well
    assert placed(None) == -1 and b"dt must be > 0" in err()
    assert lib.launch_records() == before, "a refused call moved a launch record"


# ---------------------------------------------------------------------------------------------------------------- CPU: Python
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was reached: %s" % name)


def _python_env(B=2, N=3):
    """what AtcVecEnv._rollout_policy reads of an env, on the CPU, with a library that fails the test when touched"""
    import torch
    from atc_hip.vec_env import AtcVecEnv
    env = types.SimpleNamespace(torch=torch, B=B, N=N, device=torch.device("cpu"), obs=torch.zeros((B, N * 10)), _lib=_NoLibrary(), host_mapped=False)
    env._step_rows = lambda T: AtcVecEnv._step_rows(env, T)
    return env, AtcVecEnv


def test_python_refusals_come_before_any_library_call():
    import torch
    env, AtcVecEnv = _python_env()
    w = {k: torch.zeros(L.policy_words(k)) for k in (0, 1, 2, 4)}
    with pytest.raises(ValueError, match="traffic must be one of"):
        AtcVecEnv.rollout_policy_term(env, w[0], 6, 0, hold=3)      # a K = 0 policy
    with pytest.raises(ValueError, match="traffic must be one of"):
        AtcVecEnv.rollout_policy_term(env, w[2], 6, 3, hold=3)
    with pytest.raises(ValueError, match="%d words" % L.policy_words(2)):
        AtcVecEnv.rollout_policy_term(env, w[4], 6, 2, hold=3)      # a policy packed for another K
    with pytest.raises(ValueError, match="obs0"):
        AtcVecEnv.rollout_policy_term(env, w[2], 6, 2, hold=3, obs0=torch.zeros(7))
    good = lambda: dict(AtcVecEnv._step_rows(env, 6), action=torch.zeros((2, 2, 3, 3)), term_traffic=torch.zeros((2, 2, 3, 2, 8)))      # noqa: E731
    for bad in (torch.zeros((2, 2, 3, 4, 8)), torch.zeros((2, 2, 3, 2, 8), dtype=torch.float64), torch.zeros((2, 2, 3, 2, 16))[..., ::2], np.zeros((2, 2, 3, 2, 8), np.float32)):
        with pytest.raises(ValueError, match="term_traffic"):
            AtcVecEnv.rollout_policy_term(env, w[2], 6, 2, hold=3, out=dict(good(), term_traffic=bad))
    with pytest.raises(ValueError, match="term_obs"):
        AtcVecEnv.rollout_policy_term(env, w[2], 6, 2, hold=3, out=dict(good(), term_obs=torch.zeros((2, 2, 3, 9))))
    # with good arguments the next thing the method does is reach for the library
    with pytest.raises(AssertionError, match="the library was reached"):
        AtcVecEnv.rollout_policy_term(env, w[2], 6, 2, hold=3, out=good())


def test_collect_bootstrap_keeps_refusing_traffic_and_the_new_call_refuses_k0():
    from atc_hip import ppo
    with pytest.raises(ValueError, match="terminal state are not produced"):
        ppo.collect_bootstrap(None, None, None, 6, hold=3, traffic=2)
    for K in (0, 3):
        with pytest.raises(ValueError, match="collect_bootstrap_traffic"):
            ppo.collect_bootstrap_traffic(None, None, None, 6, K, hold=3)


@pytest.mark.parametrize("K,per_decision", ((1, False), (2, True), (4, False)))
def test_collect_bootstrap_traffic_on_a_stand_in(K, per_decision):
    import torch
    import gae_boot_ref
    from atc_hip import policy, ppo
    B, N, T, hold = 4, 3, 12, 3
    D = T // hold
    s = TT.synthetic(K, B, N, T, hold, K)
    env = TT.StandIn(B, N, K, s)
    seen = []

    def value_fn(rows):
        seen.append(rows.clone())
        return rows.sum(dim=-1) * 0.25 + rows[..., 3]      # any function of the whole row, one value per aircraft
    res = ppo.collect_bootstrap_traffic(env, "w", value_fn, T, K, hold=hold, gamma=0.97, lam=0.9, seed=5, decision0=7, per_decision=per_decision)
    assert [c[0] for c in env.calls] == ["rollout_policy_term", "observe_traffic", "gae_boot"] and env.calls[0][1:] == (T, K, hold, 5, 7)
    assert env.calls[2][1:] == (hold, 0.97, 0.9, per_decision) and torch.equal(env.obs0_seen, s["obs0"].reshape(B, N * 10))
    # ONE forward over [2 D + 1, B, N, 10 + 7 K]: value_rows' D + 1 rows, then input_rows(term_obs, term_traffic)
    assert len(seen) == 1 and tuple(seen[0].shape) == (2 * D + 1, B, N, 10 + 7 * K)
    own = torch.stack([s["obs0"]] + [s["obs"][d * hold - 1].reshape(B, N, 10) for d in range(1, D + 1)])
    records = torch.cat([s["traffic"], s["traffic_final"][None]])
    want = torch.cat([torch.cat([own, records[..., :7].reshape(D + 1, B, N, 7 * K)], dim=-1), policy.input_rows(s["term_obs"], s["term_traffic"])])
    assert torch.equal(seen[0], want)
    ended = s["term_flags"] != 0
    assert ended.any() and (~ended).any() and not seen[0][D + 1:][~ended].any(), "rows of blocks that did not end are zeros"
    # the split, and what gae_boot was given
    v = value_fn(want)
    seen.pop()
    assert torch.equal(res["values"], v[:D + 1]) and torch.equal(res["boot"], v[D + 1:]) and tuple(res["boot"].shape) == (D, B, N)
    trunc = ppo.truncated(s["term_flags"])
    assert torch.equal(res["trunc"], trunc) and trunc.any() and (ended & (trunc == 0)).any()
    for k in ("reward", "done", "values", "boot", "trunc"):
        assert torch.equal(env.gae_args[k], res[k]), k
    for k in ("traffic", "term_traffic", "term_obs", "term_flags", "control", "action", "logp", "obs"):
        assert res[k] is s[k], k
    # boot is read only where trunc is set: NaN everywhere else changes nothing
    kw = dict(hold=hold, gamma=0.97, lam=0.9, per_decision=per_decision)
    a = gae_boot_ref.gae_boot(s["reward"].numpy(), s["done"].numpy(), res["values"].numpy(), res["boot"].numpy(), trunc.numpy(), **kw)
    poisoned = np.where((trunc.numpy() != 0)[:, :, None], res["boot"].numpy(), np.float32(np.nan))
    b = gae_boot_ref.gae_boot(s["reward"].numpy(), s["done"].numpy(), res["values"].numpy(), poisoned, trunc.numpy(), **kw)
    for k in ("adv", "ret"):
        assert np.array_equal(H.bits(a[k]), H.bits(b[k])) and np.array_equal(H.bits(res[k].numpy()), H.bits(np.asarray(a[k]))), k
    # ... and where it is set it matters
    c = gae_boot_ref.gae_boot(s["reward"].numpy(), s["done"].numpy(), res["values"].numpy(), res["boot"].numpy() + 1.0, trunc.numpy(), **kw)
    assert (np.asarray(c["ret"]) != np.asarray(a["ret"])).reshape(D, B, -1).any(axis=2)[trunc.numpy() != 0].all()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _same(a, b):
    return np.array_equal(H.bits(a), H.bits(b))


@pytest.mark.gpu
@pytest.mark.parametrize("W,K", [(W, K) for W in WIDTHS for K in KS], ids=["W%d-K%d" % (W, K) for W in WIDTHS for K in KS])
def test_instantiation(W, K):
    r = TT.rig(W, K)
    B, N, full = r["B"], r["N"], r["full"]
    tag = (W, K)
    assert r["same_dict"] and r["gained"] == {"atc_rollout_policy_term_launch_counts": {(W, K): 1}}, (tag, r["gained"])
    # 1. every other output and the state: rollout_policy_ends(traffic=K) on a twin env; term_traffic NULL: the same bits again
    for k in TT.OUT_KEYS:
        assert _same(full[k], r["ends"][k]), (tag, k)
        assert _same(r["null"][k], r["ends"][k]), (tag, "NULL", k)
    assert "term_traffic" not in r["null"]
    for k in H.STATE:
        assert _same(r["state"][k], r["state_ends"][k]) and _same(r["state_null"][k], r["state_ends"][k]), (tag, k)
    # 2. the records: observe_traffic() on the terminal state, from envs the call never touched; other rows keep the sentinel
    assert _same(r["ref_obs"], full["obs"]), (tag, "the replay that the terminal states come from is this run")
    t_end = E.ending_steps(full["done"], TT.HOLD)
    assert np.array_equal(t_end >= 0, full["term_flags"].view(np.uint16) != 0)
    got, want = full["term_traffic"], r["want"]
    assert (t_end >= 0).any() and (t_end < 0).any()
    assert np.all(want[t_end < 0] == np.float32(TT.SENTINEL)) and not np.any(want[t_end >= 0] == np.float32(TT.SENTINEL))
    assert _same(got, want), (tag, np.argwhere(H.bits(got) != H.bits(want))[:5])
    present = want[t_end >= 0][..., 0] == 1.0
    print("W %d K %d: %d ended blocks compared, %d of %d terminal records present" % (W, K, int((t_end >= 0).sum()), int(present.sum()), present.size))
    assert N == 1 or present.any()
    # ... and the call without auto-reset
    nr = r["noreset"]
    t2 = E.ending_steps(nr["done"], TT.HOLD)
    assert (t2 >= 0).any() and _same(nr["term_traffic"], r["want_noreset"]), (tag, "no auto-reset")
    # 4. two launches of T / 2 equal one
    for k in TT.OUT_KEYS + ("term_traffic",):
        assert _same(r["halves"][k], full[k]), (tag, "halves", k)
    for k in ("ac", "alt", "last_act", "env", "stats"):
        assert _same(r["state_halves"][k], r["state"][k]), (tag, "halves", k)


@pytest.mark.gpu
def test_the_runs_contain_what_they_are_meant_to_test():
    for W in WIDTHS:
        seen = set()
        for K in KS:
            seen |= TT.events(TT.rig(W, K))
        want = EVENTS | ({"the high mask word"} if W == 64 else set())
        assert seen == want, (W, want - seen, seen - want)


@pytest.mark.gpu
def test_out_allocates_nothing_and_overlap_is_refused_by_the_byte():
    import torch
    K, N, B = 2, 3, 5
    env = TT.make(B, N)
    w = torch.as_tensor(TT.P.random_weights(np.random.default_rng([17, K]), 1.0, TT.LOG_STD, False, K), device=env.device)
    snap, obs0 = H.snapshot(env), env.obs.clone()
    kw = dict(hold=TT.HOLD, seed=TT.SEED, decision0=TT.DECISION0)
    out = TT.fresh(env, K)
    x0 = obs0.clone()
    env.synchronize()
    torch.cuda.reset_peak_memory_stats(env.device)
    before = torch.cuda.memory_allocated(env.device)
    got = env.rollout_policy_term(w, TT.T, K, obs0=x0, out=out, **kw)
    env.synchronize()
    assert got is out and torch.cuda.max_memory_allocated(env.device) == before == torch.cuda.memory_allocated(env.device)
    want = {k: v.clone() for k, v in got.items()}
    # control [D, B, N] bytes and term_traffic in ONE allocation: touching passes, one shared byte is refused
    n_c, n_t = TT.D * B * N, TT.D * B * N * K * 8 * 4
    lo = 64
    assert n_c <= lo
    hi = lo + n_t
    pool = torch.zeros(hi + lo, dtype=torch.uint8, device=env.device)
    records = pool[lo:hi].view(torch.float32).view(TT.D, B, N, K, 8)
    for control, fine in ((pool[lo - n_c:lo], True), (pool[hi:hi + n_c], True), (pool[lo + 1 - n_c:lo + 1], False), (pool[hi - 1:hi - 1 + n_c], False)):
        H.restore(env, snap)
        records.fill_(TT.SENTINEL)      # (rows of blocks that did not end keep what they hold, as in `want`)
        o = dict(TT.fresh(env, K), control=control.view(TT.D, B, N), term_traffic=records)
        if fine:
            res = env.rollout_policy_term(w, TT.T, K, obs0=obs0.clone(), out=o, **kw)
            env.synchronize()
            assert H.same_bytes(want, res)
        else:
            with pytest.raises(RuntimeError, match="out->term_traffic overlaps out->control"):
                env.rollout_policy_term(w, TT.T, K, obs0=obs0.clone(), out=o, **kw)
            H.bytes_equal(env, snap)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", (2, 4))
def test_collect_bootstrap_traffic_on_the_device(K):
    import torch
    import ppo_value_ref as PV
    from atc_hip import policy, ppo
    B, N, T, hold = 40, 5, 24, 3
    D = T // hold
    envs = [TT.make(B, N, traffic=K, timestep_limit=7) for _ in range(3)]      # (env 2 is won at the first step: a block that ends and is no truncation)
    dev = envs[0].device
    w = torch.as_tensor(TT.P.random_weights(np.random.default_rng([18, K]), 1.0, TT.LOG_STD, False, K), device=dev)
    vw = torch.as_tensor(PV.random_weights(np.random.default_rng([19, K]), 1.0, K), device=dev)
    kw = dict(hold=hold, gamma=0.99, lam=0.95, seed=3, decision0=11)
    res = ppo.collect_bootstrap_traffic(envs[0], w, ppo.critic(envs[0], vw), T, K, **kw)
    # the calls written out by hand, on a twin
    env = envs[1]
    x0 = env.obs.clone()
    out = env.rollout_policy_term(w, T, K, hold=hold, seed=3, decision0=11, obs0=x0)
    rows = torch.cat([ppo.value_rows(env, out, x0, hold=hold, traffic=K), policy.input_rows(out["term_obs"], out["term_traffic"])])
    assert tuple(rows.shape) == (2 * D + 1, B, N, 10 + 7 * K)
    v = env.value_forward(vw, rows.contiguous())
    values, boot = v[:D + 1].contiguous(), v[D + 1:].contiguous()
    trunc = ppo.truncated(out["term_flags"])
    hand = dict(out, values=values, boot=boot, trunc=trunc)
    hand.update(env.gae_boot(out["reward"], out["done"], values, boot, trunc, hold=hold, gamma=0.99, lam=0.95))
    env.synchronize()
    assert set(res) == set(hand) and {"traffic", "term_traffic", "boot", "trunc", "adv", "ret", "values", "control"} <= set(res)
    assert H.same_bytes(res, hand)
    # against collect(traffic=K): ret differs exactly in the blocks with trunc set and in those upstream of them through lambda
    plain = ppo.collect(envs[2], w, ppo.critic(envs[2], vw), T, traffic=K, **kw)
    envs[2].synchronize()
    for k in ("obs", "reward", "done", "action", "logp", "traffic", "values"):
        assert torch.equal(res[k], plain[k]), k
    tr, ended = trunc.cpu().numpy() != 0, res["term_flags"].cpu().numpy() != 0
    reach = np.zeros((D, B), bool)      # block d's return reads a bootstrapped value: its own, or through blocks that did not end
    for d in range(D - 1, -1, -1):
        reach[d] = tr[d] | (~ended[d] & (reach[d + 1] if d + 1 < D else False))
    differs = (H.bits(res["ret"].cpu().numpy()) != H.bits(plain["ret"].cpu().numpy())).reshape(D, B, -1).any(axis=2)
    print("K %d: %d truncated blocks, %d reached upstream, %d ended otherwise" % (K, int(tr.sum()), int((reach & ~tr).sum()), int((ended & ~tr).sum())))
    assert tr.any() and (reach & ~tr).any() and (~reach).any()
    assert np.array_equal(differs, reach), np.argwhere(differs != reach)[:5]
    # one update on the dict equals update on the hand-assembled dict
    after = []
    for e, c in ((envs[0], res), (envs[1], dict(hand, obs0=x0))):
        w2, vw2 = w.clone(), vw.clone()
        perm = torch.stack([torch.randperm(D * B * N, generator=torch.Generator().manual_seed(5)) for _ in range(2)]).to(torch.int32).to(dev)
        upd = ppo.update(e, c, w2, vw2, ppo.adam_state(e, w2, vw2), epochs=2, minibatches=3, perm=perm)
        e.synchronize()
        after.append(dict(upd, w=w2, vw=vw2))
    assert H.same_bytes(after[0], after[1]) and not torch.equal(after[0]["w"], w) and not torch.equal(after[0]["vw"], vw)
    for env in envs:
        env.close()
