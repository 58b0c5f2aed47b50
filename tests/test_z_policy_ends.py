"""The policy rollout with episode ends (include/atc_step.h: atc_rollout_policy_ends; AtcVecEnv.rollout_policy_ends) and atc_gae_boot's ABI.

CPU: header <-> atc_hip/layout.py <-> ctypes (struct sizes and field order, ATC_TERM_ENDED, the slot counts, ABI 22); both symbols; the
refusals in their order with atc_last_error() naming the argument; every other launch record stays still; tests/gae_boot_ref.py against
its float64 twin within tests/gae_ref.py's running bound, and equal to gae_ref where trunc is all zero.
GPU, bit for bit: every old output equals the call without the three outputs on a twin env; term_obs rows equal
rollout(clamp(action), hold) with term_obs requested on a twin, at each block's ending step; unwritten rows keep the sentinel; term_flags
and control equal tests/policy_ends_ref.py; two launches of T / 2 equal one; each of the three outputs left out leaves the others
unchanged; the state afterwards equals the twin's.  test_the_runs_contain_what_they_are_meant_to_test asserts, on what the runs produced,
that the events the cases are built for did occur.
(The module's name sorts it behind the existing test modules on purpose: tests/test_rollout_policy_traffic.py's overlap refusals depend
on where the allocator places that test's buffers next to the env's state arrays, which every GPU test run before it shifts.)
Per-instantiation coverage — every (W, K) this call is compiled for, each against its oracle — lives in tests/test_z_policy_matrix.py."""
import ctypes as C
import functools
import re
import shutil
import subprocess

import numpy as np
import pytest

import gae_boot_ref as GB
import gae_ref as G
import helpers as H
import policy_ends_ref as E
import policy_ref as P
from atc_hip import layout as L
from held_tools import HEADER, LIB, struct_fields

NAMES = ("atc_rollout_policy_ends", "atc_rollout_policy_ends_launch_counts", "atc_gae_boot", "atc_gae_boot_launch_counts")
FAKE = C.c_void_p(0x100000)
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
KS = (0, 1, 2, 4)


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
    assert {(int(w), int(k)) for w, k in re.findall(r"\bk_rollout_policy_ends<(\d+), (\d+)>\(", text)} == {(w, k) for w in WIDTHS for k in KS}
    assert len(re.findall(r"\bk_gae_boot\(", text)) == 1


def test_header_constants_structs_and_argtypes():
    from atc_hip import lib
    text = open(HEADER).read()
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22      # new entry points: the ABI number stays
    assert L.TERM_ENDED == int(re.search(r"#define ATC_TERM_ENDED (0x[0-9a-fA-F]+)u", text).group(1), 16) == 0x8000 == E.TERM_ENDED
    all_flags = L.F_BELOW_MVA | L.F_OUTSIDE | L.F_WON | L.F_TIMEOUT | L.F_INVALID_V | L.F_INVALID_H | L.F_CONFLICT | L.F_NOISE | L.F_INACTIVE | L.F_PHI_LIMIT
    assert all_flags < (1 << 10) and not all_flags & L.TERM_ENDED          # the defined flag bits end at bit 9
    assert L.ROLLOUT_POLICY_ENDS_LAUNCH_SLOTS == int(re.search(r"ATC_ROLLOUT_POLICY_ENDS_LAUNCH_SLOTS = (\d+)", text).group(1)) == 28 == 4 * len(WIDTHS)
    assert L.GAE_BOOT_LAUNCH_SLOTS == int(re.search(r"ATC_GAE_BOOT_LAUNCH_SLOTS = (\d+)", text).group(1)) == 1
    assert L.policy_words(0) == L.POLICY_WORDS == 5062
    out = struct_fields(text, "atc_policy_ends_out")
    assert all(f[1].startswith("*") for f in out)
    assert [f[1].lstrip("*") for f in out] == list(lib.POLICY_ENDS_OUT_FIELDS) == [f[0] for f in lib.AtcPolicyEndsOut._fields_]
    assert list(lib.POLICY_ENDS_OUT_FIELDS[:7]) == list(lib.POLICY_TRAFFIC_OUT_FIELDS) and lib.POLICY_ENDS_OUT_FIELDS[7:] == ("term_obs", "term_flags", "control")
    assert [f[0] for f in out[7:]] == ["float", "uint16_t", "uint8_t"] and C.sizeof(lib.AtcPolicyEndsOut) == 80
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    for fn, names in (("atc_rollout_policy_ends", ["s", "B", "N", "T", "hold", "st", "obs0", "pol", "out", "p", "stream"]),
                      ("atc_gae_boot", ["s", "B", "NV", "D", "hold", "reward", "done", "values", "adv_next", "boot", "trunc", "g", "out", "stream"])):
        decl = re.search(r"^int %s\((.*?)\);" % fn, text, flags=re.S | re.M).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        args = [" ".join(a.split()) for a in decl.split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
        ptr = {"atc_state_t": lib.AtcState, "atc_policy_traffic_t": lib.AtcPolicyTraffic, "atc_policy_ends_out_t": lib.AtcPolicyEndsOut, "atc_params_t": lib.AtcParams,
               "atc_gae_t": lib.AtcGae, "atc_gae_out_t": lib.AtcGaeOut}
        want = [ci if a.startswith("int ") else next((C.POINTER(t) for n, t in ptr.items() if n in a), vp) for a in args]
        assert list(getattr(h, fn).argtypes) == want and getattr(h, fn).restype is ci
    assert lib.LAUNCH_RECORDS["atc_rollout_policy_ends_launch_counts"][0] == 28 and lib.LAUNCH_RECORDS["atc_gae_boot_launch_counts"] == (1, "gae_boot")
    assert [lib._width_k0(s) for s in (0, 1, 2, 3, 4, 27)] == [(1, 0), (1, 1), (1, 2), (1, 4), (2, 0), (64, 4)]


def _records():
    from atc_hip import lib
    return lib.launch_records()


def _call(h, T=1, hold=1, B=1, N=1, s=None, st=None, obs0=None, pol=None, out=None, p=None):
    return h.atc_rollout_policy_ends(s, B, N, T, hold, st, obs0, pol, out, p, None)


def test_rollout_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    err = h.atc_last_error
    at = lambda k: 0x1000000 * (k + 1)      # noqa: E731
    pol = lib.AtcPolicyTraffic(at(1), 64, 0, 0, 0, 0, 0)
    out = lib.AtcPolicyEndsOut(at(2), at(3), at(4), at(5), at(6), None, None, None, None, None)
    st, p = H.fake_state(), lib.make_params()
    ok = dict(s=FAKE, st=C.byref(st), obs0=C.c_void_p(at(7)), pol=C.byref(pol), out=C.byref(out), p=C.byref(p))
    # 1. T and hold, before any pointer is looked at
    for T, hold in ((0, 1), (1, 0), (4, -2)):
        assert _call(h, T, hold) == -1 and b"T >= 1" in err() and b"hold >= 1" in err()
    for T, hold in ((5, 2), (7, 3)):
        assert _call(h, T, hold, **ok) == -1 and b"multiple of hold" in err()
    # 2. the pointers, in atc_rollout_policy_traffic's order
    assert _call(h, 6, 3) == -1 and b"null pointer: pol " in err() and b"atc_policy_traffic_t" in err()
    now = lib.AtcPolicyTraffic(None, 7, 0xff, 0, 0, 0, 3)
    assert _call(h, **dict(ok, pol=C.byref(now))) == -1 and b"null pointer: pol->w" in err()
    assert _call(h, **dict(ok, obs0=None, out=None)) == -1 and b"null pointer: obs0" in err()
    assert _call(h, **dict(ok, out=None)) == -1 and b"null pointer: out " in err() and b"atc_policy_ends_out_t" in err()
    for k in range(4):
        o = lib.AtcPolicyEndsOut(*[None if j == k else at(2 + j) for j in range(4)], None, None, None, None, None, None)
        assert _call(h, **dict(ok, out=C.byref(o))) == -1 and b"atc_policy_ends_out_t.obs, .reward, .done and .flags" in err()
    o = lib.AtcPolicyEndsOut(at(2), at(3), at(4), at(5), None, at(6), None, None, None, None)
    bad = lib.AtcPolicyTraffic(at(1), 32, 2, 0, 0, 0, 3)
    assert _call(h, **dict(ok, out=C.byref(o), pol=C.byref(bad))) == -1 and b"atc_policy_ends_out_t.action" in err()
    # 3. n_hidden, traffic_k, the flag bits, then traffic with traffic_k == 0 — with everything later wrong as well (s NULL, B = 0)
    bad = lib.AtcPolicyTraffic(at(1), 32, 2, 0, 0, 0, 3)
    assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"n_hidden" in err()
    for k in (3, 5, 8, -1):
        bad = lib.AtcPolicyTraffic(at(1), 64, 2, 0, 0, 0, k)
        assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"pol->traffic_k" in err() and b"0, 1, 2 or 4" in err()
    for k in KS:
        bad = lib.AtcPolicyTraffic(at(1), 64, 2, 0, 0, 0, k)
        assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"pol->flags" in err()
    with_traffic = lib.AtcPolicyEndsOut(at(2), at(3), at(4), at(5), at(6), None, at(8), None, None, None)
    assert _call(h, B=0, **dict(ok, s=None, out=C.byref(with_traffic))) == -1 and b"atc_policy_ends_out_t.traffic must be NULL" in err()
    # 4. the argument errors of atc_rollout_hold, as far as they need no sector (traffic_k == 0 accepted up to here)
    for kw in (dict(s=None), dict(st=None), dict(p=None)):
        assert _call(h, B=0, **dict(ok, **kw)) == -1 and err().endswith(b": null pointer")
    for B, N in ((0, 1), (1, 0), (1, 65)):
        assert _call(h, B=B, N=N, **ok) == -1 and b"B >= 1" in err()
    assert _records() == before, "a refused call moved a launch record"


def test_gae_boot_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    err = h.atc_last_error
    at = lambda k: 0x100000 + k * 0x1000000     # noqa: E731
    g = lib.AtcGae(0.99, 0.95, 0, 0)
    out = lib.AtcGaeOut(at(4), at(5), None, None, None)
    ptrs = ("s", "reward", "done", "values", "g", "out")
    ok = dict(s=FAKE, reward=C.c_void_p(at(1)), done=C.c_void_p(at(2)), values=C.c_void_p(at(3)), g=C.byref(g), out=C.byref(out))

    def call(B=1, NV=1, D=1, hold=1, adv_next=None, boot=None, trunc=None, **kw):
        a = dict.fromkeys(ptrs)
        a.update(kw)
        return h.atc_gae_boot(a["s"], B, NV, D, hold, a["reward"], a["done"], a["values"], adv_next, boot, trunc, a["g"], a["out"], None)
    assert call(D=0, hold=0, NV=0, B=0) == -1 and b"D (" in err()
    assert call(hold=256, NV=0, B=0) == -1 and b"hold" in err()
    assert call(NV=65, B=0) == -1 and b"NV (" in err()
    assert call(B=0, **ok) == -1 and b"B >= 1" in err()
    for j, name in enumerate(ptrs):
        assert call(**{k: ok[k] for k in ptrs[:j]}) == -1 and re.search(rb"null pointer: %s\b" % name.encode(), err()), (name, err())
    bad = lib.AtcGae(np.nan, np.inf, 4, 0)
    o = lib.AtcGaeOut(at(4), None, None, None, None)
    assert call(**dict(ok, g=C.byref(bad), out=C.byref(o)), boot=C.c_void_p(at(6))) == -1 and b"null pointer: out->ret" in err()
    # one of boot and trunc without the other: behind the NULL checks, ahead of the flags
    assert call(**dict(ok, g=C.byref(bad)), boot=C.c_void_p(at(6))) == -1 and b"null pointer: trunc" in err()
    assert call(**dict(ok, g=C.byref(bad)), trunc=C.c_void_p(at(7))) == -1 and b"null pointer: boot" in err()
    assert call(**dict(ok, g=C.byref(bad)), boot=C.c_void_p(at(6)), trunc=C.c_void_p(at(7))) == -1 and b"flags" in err()
    gg = lib.AtcGae(np.inf, 0.5, 3, 0)
    assert call(**dict(ok, g=C.byref(gg)), boot=C.c_void_p(at(6)), trunc=C.c_void_p(at(7))) == -1 and b"gamma" in err()
    # both arrays join the overlap rule (B = 3, NV = 5, D = 4, hold = 2: boot 240 bytes, trunc 12)
    shape = dict(B=3, NV=5, D=4, hold=2)
    for other, size in (("reward", 96), ("done", 24), ("values", 300)):
        for off in (0, size - 1):
            assert call(**dict(ok, **shape), boot=C.c_void_p(ok[other].value + off), trunc=C.c_void_p(at(7))) == -1 and b"overlaps" in err() and b"boot" in err() and other.encode() in err()
            assert call(**dict(ok, **shape), boot=C.c_void_p(at(6)), trunc=C.c_void_p(ok[other].value + off)) == -1 and b"overlaps" in err() and b"trunc" in err() and other.encode() in err()
    assert call(**dict(ok, **shape), boot=C.c_void_p(at(4) + 239), trunc=C.c_void_p(at(7))) == -1 and b"adv overlaps boot" in err()
    assert call(**dict(ok, **shape), boot=C.c_void_p(at(6)), trunc=C.c_void_p(at(6) + 239)) == -1 and b"boot overlaps trunc" in err()
    assert _records() == before, "a refused call moved a launch record"


def test_launch_records_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    buf = (C.c_uint64 * 30)(*([99] * 30))
    assert h.atc_rollout_policy_ends_launch_counts(buf, 30) == 0
    assert all(v != 99 for v in buf[:28]) and all(v == 99 for v in buf[28:])
    buf = (C.c_uint64 * 3)(*([99] * 3))
    assert h.atc_gae_boot_launch_counts(buf, 3) == 0 and buf[0] != 99 and buf[1] == buf[2] == 99
    assert h.atc_gae_boot_launch_counts(None, 1) == -1 and h.atc_rollout_policy_ends_launch_counts(None, 1) == -1
    assert isinstance(lib.rollout_policy_ends_launch_counts(), dict) and isinstance(lib.gae_boot_launch_counts(), dict)


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatements
def _gae_inputs(seed, D, hold, B, NV, per_column):
    rng = np.random.default_rng(seed)
    T = D * hold
    reward = rng.normal(0.0, 50.0, (T, B, NV) if per_column else (T, B)).astype(np.float32)
    done = (rng.random((T, B)) < 0.3).astype(np.uint8)
    values = rng.normal(0.0, 100.0, (D + 1, B, NV)).astype(np.float32)
    boot = rng.normal(0.0, 100.0, (D, B, NV)).astype(np.float32)
    trunc = (rng.random((D, B)) < 0.5).astype(np.uint8)
    return reward, done, values, boot, trunc


@pytest.mark.parametrize("D,hold,per_decision,per_column", ((1, 1, False, False), (5, 3, False, True), (17, 20, False, False), (5, 3, True, False), (17, 1, True, True)))
def test_gae_boot_ref_against_its_float64_twin_and_gae_ref(D, hold, per_decision, per_column):
    reward, done, values, boot, trunc = _gae_inputs([7, D, hold], D, hold, 9, 3, per_column)
    kw = dict(hold=hold, gamma=0.99, lam=0.95, per_decision=per_decision)
    a32 = GB.gae_boot(reward, done, values, boot, trunc, with_bound=True, **kw)
    a64 = GB.gae_boot(reward, done, values, boot, trunc, dtype=np.float64, **kw)
    for name in ("adv", "ret"):
        dev = np.abs(a32[name].astype(np.float64) - a64[name])
        assert np.all(dev <= a32[name + "_bound"]), (name, float((dev / np.maximum(a32[name + "_bound"], 1e-300)).max()))
    assert np.array_equal(a32["block_done"], a64["block_done"]) and np.array_equal(a32["block_steps"], a64["block_steps"])
    term = done.reshape(D, hold, 9).any(axis=1) & (trunc != 0)
    assert D == 1 or (term.any() and (~term).any())
    # a float64 loop over one column, written from the header's text
    e, k = (np.argwhere(term.any(axis=0))[0][0] if term.any() else 0), 1
    A_next, V = 0.0, values.astype(np.float64)
    gam = float(np.float32(0.99))
    Gfull = gam if per_decision else gam ** hold
    for d in range(D - 1, -1, -1):
        g, R, ended = 1.0, 0.0, False
        for j in range(hold):
            r = float(reward[d * hold + j, e, k] if per_column else reward[d * hold + j, e])
            if j == 0:
                R = r
            else:
                g = g if per_decision else g * gam
                R = R + r * g
            if done[d * hold + j, e]:
                ended = True
                break
        if ended and trunc[d, e]:
            A = R + (g * gam) * float(boot[d, e, k]) - V[d, e, k]
        elif ended:
            A = R - V[d, e, k]
        else:
            A = R + Gfull * V[d + 1, e, k] - V[d, e, k] + Gfull * float(np.float32(0.95)) * A_next
        assert abs(A - a64["adv"][d, e, k]) <= 1e-9 * max(1.0, abs(A)), (d, A, a64["adv"][d, e, k])
        A_next = A
    # trunc all zero (and NULL / NULL): gae_ref, bit for bit, whatever boot holds
    ref = G.gae(reward, done, values, **kw)
    for other in (GB.gae_boot(reward, done, values, np.full_like(boot, np.nan), np.zeros_like(trunc), **kw), GB.gae_boot(reward, done, values, None, None, **kw)):
        for name in ref:
            assert np.array_equal(G.words(other[name]), G.words(ref[name])), name
    sp = GB.split(reward, done, values, boot, trunc, **kw)
    for name in ref:
        assert np.array_equal(G.words(sp[name]), G.words(a32[name])), name


def test_policy_ends_ref_on_a_hand_case():
    W, T_, C_ = E.F_WON, E.F_TIMEOUT, 64
    flags = np.zeros((6, 2, 2), np.uint16)
    done = np.zeros((6, 2), np.uint8)
    flags[1, 0] = [T_, T_ | 256]
    done[1, 0] = 1          # env 0: a time limit in the middle of block 0 (hold = 3) ...
    flags[2, 0] = [C_, 0]
    done[2, 0] = 1          # ... and a second end in the same block, which nothing reads
    flags[4, 1] = [W, 0]    # env 1: aircraft 0 handed over at step 4, no end
    assert E.ending_steps(done, 3).tolist() == [[1, -1], [-1, -1]]
    tf = E.term_flags(flags, done, 3)
    assert tf.tolist() == [[0x8000 | T_ | 256, 0], [0, 0]] and E.truncated(tf).tolist() == [[1, 0], [0, 0]]
    assert E.truncated(np.array([0x8000 | T_ | C_, 0x8000 | C_, 0x8000 | T_ | W])).tolist() == [0, 0, 1]
    c = E.control([0b01, 0b11], flags, done, 3, 2)
    assert c.tolist() == [[[1, 0], [1, 1]], [[1, 1], [1, 1]]]
    c = E.control([0b11, 0b11], flags, done, 1, 2)
    assert c[5].tolist() == [[1, 1], [0, 1]] and c[4].tolist() == [[1, 1], [1, 1]]
    c = E.control([0b01, 0b11], flags, done, 3, 2, auto_reset=False)
    assert c[1].tolist() == [[1, 0], [1, 1]]


# ---------------------------------------------------------------------------------------------------------------- GPU
SHAPES = ((5, 3), (70, 1), (3, 16), (2, 33))      # W = 4 with idle lanes, several envs a wavefront; W = 1 over two wavefronts; 16; 64 with the high mask word
T = 30
SEED, DECISION0 = 0x1234567890ABCDEF, 0xFFFFFFFA
SENTINEL = -12345.5
OLD = ("obs", "reward", "done", "flags", "action", "logp")
CASES = [(B, N, tl, hold, K, True) for B, N in SHAPES for tl in (2, 7) for hold in (1, 3, 5) for K in (0, 2)] + [(5, 3, 7, 3, 0, False)]


def _make(B, N, tl, auto_reset):
    cfg = dict(normalize=True, shaping=True, auto_reset=auto_reset, timestep_limit=tl, spawn="lattice")
    env = H.policy_env(cfg, B, N)
    # a few aircraft not under control at decision 0
    lo = env.env[:, L.ENV_MASK_LO].clone()
    if N > 1:
        lo[0] &= ~0b10
        lo[B - 1] &= ~0b01
        env.env[:, L.ENV_MASK_LO] = lo
    if N > 32:
        env.stats[1, L.STAT_MASK_HI] = 0          # aircraft 32 of env 1: the high mask word
    env.observe()
    env.synchronize()
    return env


@functools.lru_cache(maxsize=None)
def _run(B, N, tl, hold, K, auto_reset):
    import torch
    from atc_hip import lib
    A, Bv, Cv = _make(B, N, tl, auto_reset), _make(B, N, tl, auto_reset), _make(B, N, tl, auto_reset)
    for k in H.STATE + ("obs",):
        assert torch.equal(getattr(A, k), getattr(Bv, k)), k
    snap, obs0 = H.snapshot(A), A.obs.clone()
    mask0 = [int(m) for m in A.active_mask.cpu().numpy()]
    w = torch.as_tensor(P.random_weights(np.random.default_rng([17, K]), 1.0, (-0.5, -1.0, 0.25), False, K), device=A.device)
    D = T // hold

    def fresh():
        return {"term_obs": torch.full((D, B, N, 10), SENTINEL, dtype=torch.float32, device=A.device),
                "term_flags": torch.full((D, B), 0x5A5A, dtype=torch.int16, device=A.device), "control": torch.full((D, B, N), 7, dtype=torch.uint8, device=A.device)}

    def ends(env, T_, dec0, x0, extra):
        out = env._step_rows(T_)
        d = T_ // hold
        out["action"] = torch.empty((d, B, N, 3), dtype=torch.float32, device=env.device)
        out["logp"] = torch.empty((d, B, N), dtype=torch.float32, device=env.device)
        if K:
            out["traffic"] = torch.empty((d, B, N, K, 8), dtype=torch.float32, device=env.device)
        out.update(extra)
        return env.rollout_policy_ends(w, T_, K, hold=hold, seed=SEED, decision0=dec0, obs0=x0, out=out)
    before = lib.launch_records()
    full = ends(A, T, DECISION0, obs0.clone(), fresh())
    A.synchronize()
    after = lib.launch_records()
    gained = {g: {k: v - before[g].get(k, 0) for k, v in after[g].items() if v != before[g].get(k, 0)} for g in after}
    res = dict(full={k: v.cpu().numpy() for k, v in full.items()}, stA={k: getattr(A, k).cpu().numpy() for k in H.STATE}, gained={g: v for g, v in gained.items() if v},
               mask0=mask0)
    # the twin: the call without the three outputs
    if K:
        old = Bv.rollout_policy_traffic(w, T, K, hold=hold, seed=SEED, decision0=DECISION0, obs0=obs0.clone())
    else:
        old = Bv.rollout_policy(w, T, hold=hold, seed=SEED, decision0=DECISION0, obs0=obs0.clone())
    Bv.synchronize()
    res["old"] = {k: v.cpu().numpy() for k, v in old.items()}
    res["stB"] = {k: getattr(Bv, k).cpu().numpy() for k in H.STATE}
    # the per-step rollout on the clamped actions, with term_obs requested
    rows = Cv._step_rows(T)
    rows["term_obs"] = torch.full((T, B, N * 10), SENTINEL, dtype=torch.float32, device=Cv.device)
    ref = Cv.rollout(full["action"].clamp(-1.0, 1.0), out=rows, hold=hold)
    Cv.synchronize()
    res["ref"] = {k: v.cpu().numpy() for k, v in ref.items()}
    # two launches of T / 2 (where T / 2 is a multiple of hold)
    if (T // 2) % hold == 0:
        H.restore(A, snap)
        h = T // 2
        f = fresh()
        first = ends(A, h, DECISION0, obs0.clone(), {k: v[:h // hold] for k, v in f.items()})
        second = ends(A, h, DECISION0 + h // hold, first["obs"][-1].clone(), {k: v[h // hold:] for k, v in f.items()})
        A.synchronize()
        res["halves"] = {k: np.concatenate([first[k].cpu().numpy(), second[k].cpu().numpy()]) for k in first}
        res["st_halves"] = {k: getattr(A, k).cpu().numpy() for k in H.STATE}
    # each of the three left out
    res["without"] = {}
    for name in ("term_obs", "term_flags", "control"):
        H.restore(A, snap)
        f = fresh()
        del f[name]
        got = ends(A, T, DECISION0, obs0.clone(), f)
        A.synchronize()
        res["without"][name] = {k: v.cpu().numpy() for k, v in got.items()}
    for env in (A, Bv, Cv):
        env.close()
    return res


_cases = pytest.mark.parametrize("B,N,tl,hold,K,auto_reset", CASES, ids=["%dx%d-limit%d-hold%d-K%d-%s" % (c[:5] + ("reset" if c[5] else "noreset",)) for c in CASES])


@pytest.mark.gpu
@_cases
def test_ends_outputs_and_everything_else_bit_for_bit(B, N, tl, hold, K, auto_reset):
    r = _run(B, N, tl, hold, K, auto_reset)
    full, old, ref = r["full"], r["old"], r["ref"]
    D = T // hold
    tag = (B, N, tl, hold, K, auto_reset)
    # every old output and the state equal the call without the three outputs
    for k in OLD + (("traffic",) if K else ()):
        assert np.array_equal(H.bits(full[k]), H.bits(old[k])), (tag, k)
    for k in H.STATE:
        assert np.array_equal(H.bits(r["stA"][k]), H.bits(r["stB"][k])), (tag, k)
    assert r["gained"] == {"atc_rollout_policy_ends_launch_counts": {(H.lane_width(N), K): 1}}, (tag, r["gained"])
    # term_flags and control: the reference on the per-step arrays
    t_end = E.ending_steps(full["done"], hold)
    assert np.array_equal(full["term_flags"].view(np.uint16), E.term_flags(full["flags"], full["done"], hold)), tag
    want_c = E.control(r["mask0"], full["flags"], full["done"], hold, N, auto_reset=auto_reset)
    assert np.array_equal(full["control"], want_c), (tag, np.argwhere(full["control"] != want_c)[:5])
    # term_obs: the per-step rollout's term_obs at each block's ending step (its obs without an auto-reset); other rows keep the sentinel
    src = ref["term_obs"] if auto_reset else ref["obs"]
    assert np.array_equal(H.bits(ref["obs"]), H.bits(full["obs"])), tag
    want = np.full((D, B, N, 10), SENTINEL, np.float32)
    for d in range(D):
        for e in range(B):
            if t_end[d, e] >= 0:
                want[d, e] = src[t_end[d, e], e].reshape(N, 10)
    assert np.array_equal(H.bits(full["term_obs"]), H.bits(want)), (tag, np.argwhere(H.bits(full["term_obs"]) != H.bits(want))[:5])
    # two launches of T / 2 equal one
    if "halves" in r:
        for k in full:
            assert np.array_equal(H.bits(r["halves"][k]), H.bits(full[k])), (tag, "halves", k)
        for k in ("ac", "alt", "last_act", "env", "stats"):
            assert np.array_equal(H.bits(r["st_halves"][k]), H.bits(r["stA"][k])), (tag, "halves", k)
    # each of the three left out: the others unchanged
    for name, got in r["without"].items():
        assert name not in got
        for k in got:
            assert np.array_equal(H.bits(got[k]), H.bits(full[k])), (tag, "without " + name, k)


@pytest.mark.gpu
def test_the_runs_contain_what_they_are_meant_to_test():
    seen = set()
    for c in CASES:
        B, N, tl, hold, K, auto_reset = c
        full = _run(*c)["full"]
        D = T // hold
        done = full["done"].reshape(D, hold, B) != 0
        tf = full["term_flags"].view(np.uint16)
        t_end = E.ending_steps(full["done"], hold)
        trunc = E.truncated(tf) != 0
        if hold > 1 and (trunc & (t_end % hold > 0) & (t_end % hold < hold - 1) & (t_end >= 0)).any():
            seen.add("a time-limit end in the middle of a block")
        if hold > 1 and ((t_end >= 0) & (t_end % hold == hold - 1)).any():
            seen.add("an end on a block's last step")
        if tl < hold and (done.sum(axis=1) >= 2).any():
            seen.add("two ends inside one block, timestep_limit < hold")
        if ((tf != 0) & ~trunc).any():
            seen.add("an end that is not a time limit")
        if (tf == 0).any():
            seen.add("a block with no end")
        if (full["control"][0] == 0).any():
            seen.add("an aircraft not under control at decision 0")
        if N > 32 and full["control"][0, 1, 32] == 0:
            seen.add("the high mask word")
    want = {"a time-limit end in the middle of a block", "an end on a block's last step", "two ends inside one block, timestep_limit < hold",
            "an end that is not a time limit", "a block with no end", "an aircraft not under control at decision 0", "the high mask word"}
    assert seen == want, want - seen


@pytest.mark.gpu
def test_an_aircraft_handed_over_during_the_call_leaves_control():
    """one aircraft flown into the final-approach corridor by a constant policy (W3 = 0, b3 = the targets): handed over, not done"""
    import torch
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import model, scenarios
    env = AtcVecEnv(2, 2, sim_parameters=model.SimParameters(1), scenario=scenarios.LOWW(random_entrypoints=True), auto_reset=True, seed=3, timestep_limit=6000)
    for e in range(2):
        env.set_state(e, 0, 48.9, 31.9, 3300.0, 345.0, 200.0)
        env.set_state(e, 1, 20.0, 60.0, 15000.0, 90.0, 250.0)
    env.observe()
    env.synchronize()
    mask0 = [int(m) for m in env.active_mask.cpu().numpy()]
    parts = P.split(P.random_weights(np.random.default_rng(5), 1.0, (0.0, 0.0, 0.0), True))
    parts["b3"] = np.array([0.0, 2 * 2700.0 / 38000.0 - 1, 2 * 345.0 / 360.0 - 1], np.float32)
    w = torch.as_tensor(P.pack(*[parts[n] for n, _ in P.SHAPES]), device=env.device)
    out = env.rollout_policy_ends(w, 60, 0, hold=3, deterministic=True)
    env.synchronize()
    flags, done, control = out["flags"].cpu().numpy(), out["done"].cpu().numpy(), out["control"].cpu().numpy()
    won = (flags.view(np.uint16)[:, :, 0] & E.F_WON) != 0
    assert won.any() and not done[won.argmax(axis=0)[0], 0], "no aircraft was handed over"
    assert np.array_equal(control, E.control(mask0, flags, done, 3, 2))
    assert control[0].all() and (control[:, :, 0] == 0).any() and control[:, :, 1].all()
    env.close()
