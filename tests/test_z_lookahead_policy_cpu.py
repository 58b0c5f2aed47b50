"""atc_lookahead_policy without a GPU (include/atc_step.h; AtcVecEnv.lookahead_policy, atc_hip/shield.py, atc_hip.ppo.mc_returns): the symbol,
the struct and the argtypes across the header, atc_hip/layout.py and atc_hip/lib.py with ATC_ABI_VERSION unchanged; every refusal through
ctypes, in the header's order, with NULL and made-up pointers — no launch is made; the launch record; the Python surface and its refusals
before any library call; tests/lookahead_policy_ref.py's fold against a float64 fold on random arrays, with the first done in every position
of a segment."""
import ctypes as C
import inspect
import re
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import lookahead_policy_ref as R
from atc_hip import layout as L
from held_tools import HEADER, LIB, struct_fields

NAMES = ("atc_lookahead_policy", "atc_lookahead_policy_launch_counts")
RECORD = NAMES[1]
FAKE = C.c_void_p(0x100000)     # a made-up pointer: a call that is refused never follows it
WIDTHS = (1, 2, 4, 8, 16, 32, 64)


def _at(k):
    return 0x10000000 * (k + 1)      # made-up ranges 256 MiB apart


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_exports_and_kernel_symbols():
    from atc_hip import lib
    assert set(NAMES) <= set(lib.EXPORTS)
    h = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    got = {(int(w), f) for w, f in re.findall(r"\bk_lookahead_policy<(\d+), (true|false)>\(", text)}
    assert got == {(w, f) for w in WIDTHS for f in ("true", "false")}


def test_header_struct_and_argtypes():
    from atc_hip import lib
    text = open(HEADER).read()
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22      # a new entry point: the ABI number stays
    assert L.LOOKAHEAD_POLICY_LAUNCH_SLOTS == int(re.search(r"ATC_LOOKAHEAD_POLICY_LAUNCH_SLOTS = (\d+)", text).group(1)) == 7
    o = struct_fields(text, "atc_lookahead_policy_out")
    plan = struct_fields(text, "atc_plan_out")
    assert [x[1].lstrip("*") for x in o] == list(lib.LOOKAHEAD_POLICY_FIELDS) == [x[0] for x in lib.AtcLookaheadPolicyOut._fields_]
    assert o[:len(plan)] == plan and [x[1] for x in o[len(plan):]] == ["*flown", "*logp"] and all(x[0] == "float" for x in o[len(plan):])
    assert C.sizeof(lib.AtcLookaheadPolicyOut) == 80 and all(t is C.c_void_p for _, t in lib.AtcLookaheadPolicyOut._fields_)
    decl = re.search(r"^int atc_lookahead_policy\((.*?)\);", text, flags=re.S | re.M).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "B", "N", "K", "H", "M", "st", "obs0", "first", "pol", "out", "p", "stream"]
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    ptr = {"atc_state_t": lib.AtcState, "atc_policy_t": lib.AtcPolicy, "atc_lookahead_policy_out_t": lib.AtcLookaheadPolicyOut, "atc_params_t": lib.AtcParams}
    want = [ci if a.startswith("int ") else next((C.POINTER(t) for n, t in ptr.items() if n in a), vp) for a in args]
    assert list(h.atc_lookahead_policy.argtypes) == want and h.atc_lookahead_policy.restype is ci
    assert list(getattr(h, RECORD).argtypes) == [C.POINTER(C.c_uint64), ci]
    slots, slot_name = lib.LAUNCH_RECORDS[RECORD]
    assert slots == 7 and [slot_name(i) for i in range(7)] == list(WIDTHS) and callable(lib.lookahead_policy_launch_counts)


def test_launch_record_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    buf = (C.c_uint64 * 9)(*([99] * 9))
    assert getattr(h, RECORD)(buf, 9) == 0
    assert all(v != 99 for v in buf[:7]) and all(v == 99 for v in buf[7:])
    assert getattr(h, RECORD)(None, 1) == -1
    assert RECORD in lib.launch_records() and isinstance(lib.lookahead_policy_launch_counts(), dict)


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = lib.launch_records()
    err = h.atc_last_error
    HELD, DISCRETE = L.M_ACTIONS_HELD, L.M_DISCRETE

    def call(B=0, N=0, K=0, Hh=0, M=0, **a):      # (every count wrong unless given: the pointers are looked at first)
        return h.atc_lookahead_policy(a.get("s"), B, N, K, Hh, M, a.get("st"), a.get("obs0"), a.get("first"), a.get("pol"), a.get("out"), a.get("p"), None)
    bad_pol = lib.AtcPolicy(_at(1), 32, 0xfe, 0, 0, 0)      # n_hidden and the flag bits wrong
    out = lib.AtcLookaheadPolicyOut(*([_at(1)] * 10))       # every output ON the weights: the first of the overlap refusals
    st = H.fake_state()
    p_bad = lib.make_params(discrete=True)
    p_bad.mode |= HELD
    ok = dict(s=FAKE, st=C.byref(st), obs0=C.c_void_p(_at(2)), pol=C.byref(bad_pol), out=C.byref(out), p=C.byref(p_bad))
    # 1. the pointers in their order, each with everything behind it wrong as well
    assert call() == -1 and b"null pointer: pol " in err()
    assert call(**dict(ok, pol=None)) == -1 and b"null pointer: pol " in err()
    now = lib.AtcPolicy(None, 7, 0xff, 0, 0, 0)
    assert call(**dict(ok, pol=C.byref(now))) == -1 and b"null pointer: pol->w" in err()
    assert call(**dict(ok, out=None)) == -1 and b"null pointer: out " in err()
    for k in (0, 1):
        o = lib.AtcLookaheadPolicyOut(*[None if j == k else _at(1) for j in range(10)])
        assert call(**dict(ok, out=C.byref(o))) == -1 and b"atc_lookahead_policy_out_t.reward and .done" in err()
    assert call(**dict(ok, obs0=None)) == -1 and b"null pointer: obs0" in err()
    for kw in (dict(s=None), dict(st=None), dict(p=None)):
        assert call(**dict(ok, **kw)) == -1 and err().endswith(b": null pointer"), err()
    assert call(**dict(ok, obs0=None, first=C.c_void_p(_at(3)), s=None)) == -1 and err().endswith(b": null pointer")      # (obs0 may be NULL where first is given)
    hole = H.fake_state()
    hole.alt = None
    assert call(**dict(ok, st=C.byref(hole))) == -1 and b"null field" in err()
    # 2. K, H, M
    for K in (0, -1, 256):
        assert call(K=K, **ok) == -1 and b"K (" in err() and b"255" in err()
    for Hh in (0, -1, 17):
        assert call(K=255, Hh=Hh, **ok) == -1 and b"H (" in err() and b"16" in err()
    for M in (0, -1, 1025):
        assert call(K=1, Hh=16, M=M, **ok) == -1 and b"M (" in err() and b"1024" in err()
    good = dict(K=3, Hh=4, M=1024)
    # 3. the mode: ATC_M_DISCRETE, then ATC_M_ACTIONS_HELD
    assert call(**good, **ok) == -1 and b"ATC_M_DISCRETE" in err()
    p_held = lib.make_params()
    p_held.mode |= HELD
    assert call(**good, **dict(ok, p=C.byref(p_held))) == -1 and b"ATC_M_ACTIONS_HELD" in err()
    # 4. the policy's fields
    p = lib.make_params()
    assert not p.mode & (HELD | DISCRETE)
    ok["p"] = C.byref(p)
    assert call(**good, **ok) == -1 and b"n_hidden" in err()
    for fl in (2, 3, 0x80000000):
        pol = lib.AtcPolicy(_at(1), 64, fl, 0, 0, 0)
        assert call(**good, **dict(ok, pol=C.byref(pol))) == -1 and b"pol->flags" in err()
    # 5. the batch shape, B * N for one launch, M * B * N for the key
    pol = lib.AtcPolicy(_at(1), 64, L.POLICY_DETERMINISTIC, 5, 9, 0)
    ok["pol"] = C.byref(pol)
    for B, N in ((0, 1), (-1, 1), (1, 0), (1, 65)):
        assert call(B=B, N=N, **good, **ok) == -1 and b"B >= 1" in err()
    assert call(B=1 << 21, N=64, **good, **ok) == -1 and b"too large" in err()
    assert call(B=1 << 16, N=64, **good, **ok) == -1 and b"M*B*N" in err()          # 2^22 aircraft x 1024 candidates = 2^32
    assert call(B=3, N=64, **dict(good, M=1025), **ok) == -1 and b"M (" in err()
    # 6. the overlap rule, on pointer values: the weights against every output first (`out` above has every output ON the weights) ...
    Bn, Nn, Kk, Hh, M = 3, 2, 3, 4, 5
    assert call(B=Bn, N=Nn, K=Kk, Hh=Hh, M=M, **ok) == -1 and b"pol->w overlaps out->reward" in err()
    bn, mb, mbn = Bn * Nn, M * Bn, M * Bn * Nn
    outs = dict(reward=mb * 4, done=mb, n_steps=mb * 2, seg_reward=mb * Hh * 4, flags=mbn * 2, ac_reward=mbn * 4, min_sep=mb * 4, obs=mbn * 40, flown=mbn * Hh * 12,
                logp=mbn * Hh * 4)
    assert list(outs) == list(lib.LOOKAHEAD_POLICY_FIELDS)
    state = dict(zip(("ac", "alt", "last_act", "env", "stats", "phi_wide"), (bn * 16, bn * 8, bn * 16, Bn * L.ENV_WORDS * 4, Bn * L.STAT_WORDS * 4, bn * 32)))
    ins = {"pol->w": (_at(1), L.POLICY_WORDS * 4), "obs0": (_at(2), bn * 40), "first": (_at(3), mbn * 12)}
    for k, (n, size) in enumerate(state.items()):
        ins["st->" + n] = (getattr(st, n), size)
    base = {n: _at(20 + k) for k, n in enumerate(outs)}

    def run(ptrs, with_first):
        o = lib.AtcLookaheadPolicyOut(*[ptrs[n] for n in outs])
        return call(B=Bn, N=Nn, K=Kk, Hh=Hh, M=M, **dict(ok, out=C.byref(o), first=C.c_void_p(_at(3)) if with_first else None))
    n = 0
    for j, b in enumerate(outs):
        # ... then each output against every input it may not share a byte with, and against every output in front of it
        others = dict(ins, **{"out->" + a: (base[a], outs[a]) for a in list(outs)[:j]})
        for a, (ptr, size) in others.items():
            for off in (0, size - 1, -(outs[b] - 1)):
                for with_first in (False, True):
                    if (a == "first" and not with_first) or (a == "obs0" and with_first):      # (an input that is not read is not a range)
                        continue
                    assert run(dict(base, **{b: ptr + off}), with_first) == -1 and b"overlaps" in err() and a.encode() in err() and b.encode() in err(), (a, b, off, err())
                    n += 1
    assert n == sum((9 + j) * 3 * 2 - 2 * 3 for j in range(10))
    # (the last check, the time increment, reads the sector: it and ranges that only touch are in the GPU file)
    assert lib.launch_records() == before, "a refused call moved a launch record"


def test_python_surface():
    from atc_hip import ppo, shield
    from atc_hip.sb_adapter import AtcSBVecEnv
    from atc_hip.vec_env import AtcVecEnv
    sig = inspect.signature(AtcVecEnv.lookahead_policy)
    assert list(sig.parameters) == ["self", "weights", "K", "H", "first", "M", "seed", "decision0", "deterministic", "obs0", "outputs", "out"]
    kw = list(sig.parameters)[4:]
    assert [sig.parameters[k].default for k in kw] == [None, None, 0, 0, False, None, ("flags", "min_sep"), None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kw)
    assert not hasattr(AtcSBVecEnv, "lookahead_policy")
    sig = inspect.signature(shield.policy_shield)
    assert list(sig.parameters) == ["env", "w", "M", "K", "H", "veto", "seed", "decision", "gamma"]
    assert sig.parameters["veto"].default == L.F_CONFLICT | L.F_BELOW_MVA and sig.parameters["gamma"].default == 1.0
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("veto", "seed", "decision", "gamma"))
    assert list(inspect.signature(ppo.mc_returns).parameters)[:6] == ["env", "w", "M", "K", "H", "gamma"]
    # no existing signature changed
    assert list(inspect.signature(AtcVecEnv.lookahead_plan).parameters) == ["self", "actions", "K", "outputs"]
    assert list(inspect.signature(AtcVecEnv._candidate_results).parameters)[:5] == ["self", "cache_name", "lead", "outputs", "plan"]


class _NoLibrary:
    """an env stand-in whose library handle fails the test when anything is called through it"""
    B, N, traffic_k, host_mapped = 3, 2, 0, False

    class _lib:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    _lib = _lib()

    class sector:
        handle = None

    class params:
        mode = 0

    def __init__(self):
        import torch
        self.torch = torch
        self.device = torch.device("cpu")
        self.obs = torch.zeros(self.B, self.N * 10)


def test_lookahead_policy_refuses_before_any_library_call():
    import torch
    from atc_hip.vec_env import AtcVecEnv
    env = _NoLibrary()
    w0 = torch.zeros(L.policy_words(0))

    def refused(match, w=w0, K=3, Hh=2, **kw):
        with pytest.raises(ValueError, match=match):
            AtcVecEnv.lookahead_policy(env, w, K, Hh, **kw)
    for K in (0, 256):
        refused("K", K=K, M=2)
    for Hh in (0, 17):
        refused("H", Hh=Hh, M=2)
    for k in L.POLICY_TRAFFIC_K:      # a packed traffic policy: out of scope, and the message says so
        refused("traffic", w=torch.zeros(L.policy_words(k)), M=2)
    for w in (w0.double(), torch.zeros(2 * L.policy_words(0))[::2], np.zeros(L.policy_words(0), np.float32)):
        refused("weights", w=w, M=2)
    refused("M is required")
    for M in (0, 1025):
        refused("M", M=M)
    refused("obs0", M=2, obs0=torch.zeros(5))
    refused("first", first=torch.zeros(3))
    refused("M", first=torch.zeros(2, 3, 2, 3), M=3)
    refused("outputs", M=2, outputs=("flags", "value"))
    refused("out", M=2, out={"reward": torch.zeros(2, 3)})      # done is missing
    refused(r"out\['flown'\]", M=2, out={"reward": torch.zeros(2, 3), "done": torch.zeros(2, 3, dtype=torch.uint8), "flown": torch.zeros(2, 3, 2, 3)})
    refused("out", M=2, out={"reward": torch.zeros(2, 3), "done": torch.zeros(2, 3, dtype=torch.uint8), "value": torch.zeros(2)})
    env.params.mode = L.M_DISCRETE
    refused("discrete", M=2)
    env.params.mode = 0
    good = {"reward": torch.zeros(2, 3), "done": torch.zeros(2, 3, dtype=torch.uint8), "seg_reward": torch.zeros(2, 2, 3), "flown": torch.zeros(2, 2, 3, 2, 3),
            "logp": torch.zeros(2, 2, 3, 2)}
    with pytest.raises(AssertionError, match="the library was called"):
        AtcVecEnv.lookahead_policy(env, w0, 3, 2, M=2, out=good)


# ---------------------------------------------------------------------------------------------------------------- the fold
def _loop_fold(reward, done, K, Hh):
    """the definition, one column at a time, in float32 scalars"""
    T, Cn = reward.shape
    seg, tot, dn, n = np.zeros((Hh, Cn), np.float32), np.zeros(Cn, np.float32), np.zeros(Cn, np.uint8), np.zeros(Cn, np.int64)
    for c in range(Cn):
        total, stop = None, False
        for h in range(Hh):
            if stop:
                break
            acc = None
            for j in range(K):
                t = h * K + j
                acc = reward[t, c] if acc is None else np.float32(acc + reward[t, c])
                n[c] += 1
                dn[c] = done[t, c]
                if done[t, c]:
                    stop = True
                    break
            seg[h, c] = acc
            total = acc if total is None else np.float32(total + acc)
        tot[c] = total
    return seg, tot, dn, n


@pytest.mark.parametrize("K,Hh", [(3, 1), (3, 4), (1, 5), (5, 2)])
def test_fold_cuts_pads_and_sums(K, Hh):
    rng = np.random.default_rng([K, Hh])
    T = K * Hh
    # a column per position of the first done — every step of the plan: the first step, mid-segment, a segment's last step, the plan's last
    # step — then one without a done, then random ones; later dones behind the first are there to be ignored
    firsts = list(range(T)) + [None] + [int(t) for t in rng.integers(0, T, 40)]
    Cn = len(firsts)
    reward = (rng.normal(size=(T, Cn)) * 10.0 ** rng.integers(-3, 4, (T, Cn))).astype(np.float32)
    reward[0, 1::3] = np.float32(-0.0)
    done = rng.random((T, Cn)) < 0.3
    for c, t in enumerate(firsts):
        done[:t if t is not None else T, c] = False
        if t is not None:
            done[t, c] = True
    got = R.fold(reward, done, K, Hh)
    seg, tot, dn, n = _loop_fold(reward, done, K, Hh)
    want_n = np.array([T if t is None else t + 1 for t in firsts])
    assert np.array_equal(got["n_steps"], want_n) and np.array_equal(n, want_n)
    if Hh > 1 and K > 1:      # the positions the issue names are all among the columns
        pos = {(t // K, t % K) for t in firsts if t is not None}
        assert {(0, 0), (0, K - 1), (1, K // 2) if K > 2 else (1, 0), (Hh - 1, K - 1)} <= pos
    assert np.array_equal(H.bits(got["seg_reward"]), H.bits(seg)) and np.array_equal(H.bits(got["reward"]), H.bits(tot))
    assert np.array_equal(got["done"], dn) and np.array_equal(got["done"], np.array([t is not None for t in firsts], np.uint8))
    # zeros behind the cut, +0 exactly
    for c, nn in enumerate(want_n):
        ran = -(-int(nn) // K)
        assert not H.bits(got["seg_reward"][ran:, c]).any()
    # against the float64 fold: sequential float32 sums of k terms are within (k - 1) eps sum |r| of it
    f64 = R.fold64(reward, done, K, Hh)
    eps = float(np.finfo(np.float32).eps)
    run = np.arange(T)[:, None] < want_n[None, :]
    mag = np.where(run, np.abs(reward.astype(np.float64)), 0.0)
    seg_mag = mag.reshape(Hh, K, Cn).sum(axis=1)
    assert np.array_equal(f64["n_steps"], want_n)
    assert np.all(np.abs(got["seg_reward"] - f64["seg_reward"]) <= K * eps * seg_mag)
    assert np.all(np.abs(got["reward"] - f64["reward"]) <= (K + Hh) * eps * seg_mag.sum(axis=0))
    # the helpers next to it
    flags = rng.integers(0, 1 << 16, (T, Cn, 2)).astype(np.int16)
    of = R.or_flags(flags, want_n)
    for c, nn in enumerate(want_n):
        assert np.array_equal(of[c], np.bitwise_or.reduce(flags[:nn, c].astype(np.int64) & 0xffff, axis=0).astype(np.uint16))
        assert np.array_equal(R.last_rows(flags, want_n)[c], flags[nn - 1, c])
    assert np.allclose(R.discounted(seg, 0.5), sum(seg[h].astype(np.float64) * 0.5 ** h for h in range(Hh)))
