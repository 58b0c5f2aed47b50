"""Advantages and returns of a collection (include/atc_step.h: atc_gae; AtcVecEnv.gae; atc_hip/ppo.py: collect): the per-decision block
fold and the GAE recurrence in one launch.

CPU: the exports and the one kernel symbol; structs, macros and argtypes across the header, atc_hip/layout.py and atc_hip/lib.py; the
refusal order through ctypes with NULL and made-up pointers; AtcVecEnv.gae's own refusals on a stand-in without a library;
tests/gae_ref.py (the numpy restatement) against a plain scalar loop written from the header's text on hand cases; the float32
restatement against its float64 twin within the running error bound derived in tests/gae_ref.py; the split property.
GPU: adv, ret and the three block outputs BIT-IDENTICAL to the restatement over the shapes, (D, hold), (gamma, lam), done rates, both
flags and adv_next given / NULL rotating through the cases, into pattern-filled buffers with guard rows; the split; out= without an
allocation; NaNs behind a block's first done; a NaN in values; the launch records; the refusals behind the pointer checks; end to end
behind rollout_policy, and atc_hip.ppo.collect against the three calls made by hand (once with traffic=2)."""
import ctypes as C
import functools
import inspect
import re
import shutil
import subprocess

import numpy as np
import pytest

import gae_ref as G
import helpers as H
import policy_ref as P
import policy_traffic_ref as PT
from atc_hip import layout as L
from held_tools import GUARD, HEADER, LIB

NAMES = ("atc_gae", "atc_gae_launch_counts")
FAKE = C.c_void_p(0x100000)     # a made-up pointer: a call that is refused never follows it
PATTERN = 0xA5                  # the byte output buffers hold before a call
_records = functools.partial(H.launch_records, "gae")


# ---------------------------------------------------------------------------------------------------------------- CPU: the ABI
def test_exports_and_one_kernel_symbol():
    from atc_hip import lib
    assert set(NAMES) <= set(lib.EXPORTS)
    h = lib.load()      # (the binding's own handle: it loads torch's HIP runtime first, so a run of this module alone has one runtime)
    for name in NAMES:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    assert len(re.findall(r"\bk_gae\(", text)) == 1
    assert open(LIB, "rb").read().count(b"_Z5k_gaeiiiiPKfPKhS0_S0_7atc_gae11atc_gae_out\0") >= 1      # ... and in the embedded code object


def _struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [" ".join(d.split()).replace("* ", " *").rsplit(" ", 1) for d in body.split(";") if d.strip()]


def test_header_constants_structs_and_argtypes():
    from atc_hip import lib
    text = open(HEADER).read()
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, text).group(1))      # noqa: E731
    assert (L.GAE_PER_DECISION, L.GAE_REWARD_PER_COLUMN, L.GAE_MAX_NV) == (define("ATC_GAE_PER_DECISION"), define("ATC_GAE_REWARD_PER_COLUMN"), define("ATC_GAE_MAX_NV")) == (1, 2, 64)
    assert L.GAE_LAUNCH_SLOTS == int(re.search(r"ATC_GAE_LAUNCH_SLOTS = (\d+)", text).group(1)) == 1
    assert L.SKIP_MAX == int(re.search(r"ATC_SKIP_MAX = (\d+)", text).group(1)) == 255
    assert L.ABI_VERSION == 22 and define("ATC_ABI_VERSION") == 22          # a new entry point: the ABI number stays
    scalar = {"float": C.c_float, "uint32_t": C.c_uint32}
    g = _struct_fields(text, "atc_gae")
    assert [f[1] for f in g] == list(lib.GAE_FIELDS) == [f[0] for f in lib.AtcGae._fields_]
    assert [scalar[f[0]] for f in g] == [f[1] for f in lib.AtcGae._fields_] and C.sizeof(lib.AtcGae) == 16
    o = _struct_fields(text, "atc_gae_out")
    assert [f[1].lstrip("*") for f in o] == list(lib.GAE_OUT_FIELDS) == [f[0] for f in lib.AtcGaeOut._fields_]
    assert all(f[1].startswith("*") for f in o) and [f[0] for f in o] == ["float", "float", "float", "uint8_t", "uint8_t"]
    assert all(f[1] is C.c_void_p for f in lib.AtcGaeOut._fields_) and C.sizeof(lib.AtcGaeOut) == 40
    decl = re.search(r"^int atc_gae\((.*?)\);", text, flags=re.S | re.M).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "B", "NV", "D", "hold", "reward", "done", "values", "adv_next", "g", "out", "stream"]
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    want = [ci if a.startswith("int ") else C.POINTER(lib.AtcGae) if "atc_gae_t" in a else C.POINTER(lib.AtcGaeOut) if "atc_gae_out_t" in a else vp for a in args]
    assert list(h.atc_gae.argtypes) == want
    assert h.atc_gae.restype is ci and h.atc_gae_launch_counts.restype is ci
    assert list(h.atc_gae_launch_counts.argtypes) == [C.POINTER(C.c_uint64), ci]
    assert callable(lib.gae_launch_counts) and lib.LAUNCH_RECORDS["atc_gae_launch_counts"] == (1, "gae")


ARGS = ("s", "reward", "done", "values", "g", "out")      # the pointers that may not be NULL, in the order they are looked at


def _gae_call(h):
    def call(B=1, NV=1, D=1, hold=1, adv_next=None, **kw):
        a = dict.fromkeys(ARGS)
        a.update(kw)
        return h.atc_gae(a["s"], B, NV, D, hold, a["reward"], a["done"], a["values"], adv_next, a["g"], a["out"], None)
    return call


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    at = lambda k: 0x100000 + k * 0x1000000     # noqa: E731  (made-up ranges 16 MiB apart)
    g = lib.AtcGae(0.99, 0.95, 0, 0)
    out = lib.AtcGaeOut(at(4), at(5), None, None, None)
    ok = dict(s=FAKE, reward=C.c_void_p(at(1)), done=C.c_void_p(at(2)), values=C.c_void_p(at(3)), g=C.byref(g), out=C.byref(out))
    call, err = _gae_call(h), h.atc_last_error
    # 1. D, 2. hold, 3. NV, 4. B: before any pointer is looked at, each with every later one wrong as well
    for D in (0, -1):
        assert call(D=D, hold=0, NV=0, B=0) == -1 and b"D (" in err()
    for hold in (0, 256, -1):
        assert call(hold=hold, NV=0, B=0) == -1 and b"hold" in err() and b"255" in err()
    for NV in (0, 65, -1):
        assert call(NV=NV, B=0) == -1 and b"NV (" in err() and b"64" in err()
    for B in (0, -3):
        assert call(B=B, **ok) == -1 and b"B >= 1" in err()
    for hold, NV in ((1, 1), (255, 64)):      # accepted as far as the first pointer check
        assert call(hold=hold, NV=NV) == -1 and b"null pointer: s" in err()
    # 5. the pointers, in their order: with every earlier one given and every later one NULL, the first NULL is the one named
    for j, name in enumerate(ARGS):
        named = re.compile(rb"null pointer: %s\b" % name.encode())
        assert call(**{k: ok[k] for k in ARGS[:j]}) == -1 and named.search(err()), (name, err())
        assert call(**dict(ok, **{name: None})) == -1 and named.search(err()), (name, err())
    bad = lib.AtcGae(np.nan, np.inf, 4, 0)      # (everything behind the pointers is wrong as well)
    for o, word in ((lib.AtcGaeOut(None, None, None, None, None), b"out->adv"), (lib.AtcGaeOut(at(4), None, None, None, None), b"out->ret")):
        assert call(**dict(ok, g=C.byref(bad), out=C.byref(o))) == -1 and b"null pointer: " + word in err()
    # 6. flags, 7. gamma, lam, 8. the overlap rule: host checks on the two structs and on pointer values
    assert call(**dict(ok, g=C.byref(bad))) == -1 and b"flags" in err()
    for gm, lm, word in ((np.nan, np.inf, b"gamma"), (np.inf, 0.5, b"gamma"), (0.5, np.nan, b"lam"), (0.5, -np.inf, b"lam")):
        gg = lib.AtcGae(gm, lm, 3, 0)
        assert call(**dict(ok, g=C.byref(gg), reward=ok["done"])) == -1 and word in err()
    assert _records() == before, "a refused call moved a launch record"


def _overlap_pairs(call, err, base, B, NV, D, hold, per_column):
    """every pair of the nine arrays once: equal pointers, then the last / first bytes shared; ranges that only touch are accepted"""
    from atc_hip import lib
    Cn, T = B * NV, D * hold
    rc = Cn if per_column else B
    size = dict(reward=T * rc * 4, done=T * B, values=(D + 1) * Cn * 4, adv_next=Cn * 4, adv=D * Cn * 4, ret=D * Cn * 4, block_reward=D * rc * 4,
                block_done=D * B, block_steps=D * B)
    names = list(size)
    g = lib.AtcGae(0.9, 0.9, L.GAE_REWARD_PER_COLUMN if per_column else 0, 0)

    def run(p):
        o = lib.AtcGaeOut(*[p[n] for n in lib.GAE_OUT_FIELDS])
        return call(B=B, NV=NV, D=D, hold=hold, adv_next=C.c_void_p(p["adv_next"]), s=base["s"], reward=C.c_void_p(p["reward"]), done=C.c_void_p(p["done"]),
                    values=C.c_void_p(p["values"]), g=C.byref(g), out=C.byref(o))
    n = 0
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for off in (0, size[a] - 1, -(size[b] - 1)):
                assert run(dict(base, **{b: base[a] + off})) == -1 and b"overlaps" in err() and a.encode() in err() and b.encode() in err(), (a, b, off)
                n += 1
    return n, run, size


def test_overlap_rule_on_pointer_values():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    base = dict(s=FAKE, **{n: 0x100000 + (k + 1) * 0x1000000 for k, n in enumerate(("reward", "done", "values", "adv_next") + lib.GAE_OUT_FIELDS)})
    n, _, _ = _overlap_pairs(_gae_call(h), h.atc_last_error, base, 3, 5, 4, 2, True)
    m, _, _ = _overlap_pairs(_gae_call(h), h.atc_last_error, base, 3, 5, 4, 2, False)
    assert n == m == 36 * 3 and _records() == before


def test_launch_record_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    buf = (C.c_uint64 * 8)(*([99] * 8))
    assert h.atc_gae_launch_counts(buf, 8) == 0
    assert buf[0] != 99 and all(v == 99 for v in buf[1:])
    assert h.atc_gae_launch_counts(None, 1) == -1
    assert isinstance(lib.gae_launch_counts(), dict)


def test_python_surface():
    from atc_hip import ppo
    from atc_hip.vec_env import AtcVecEnv
    sig = inspect.signature(AtcVecEnv.gae)
    assert list(sig.parameters) == ["self", "reward", "done", "values", "hold", "gamma", "lam", "per_decision", "adv_next", "out"]
    assert [sig.parameters[k].default for k in ("hold", "gamma", "lam", "per_decision", "adv_next", "out")] == [1, 0.99, 0.95, False, None, None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("per_decision", "adv_next", "out"))
    sig = inspect.signature(ppo.collect)
    assert list(sig.parameters) == ["env", "weights", "value_fn", "T", "hold", "traffic", "gamma", "lam", "seed", "decision0", "obs0", "per_decision"]
    assert "observe_traffic()" in ppo.collect.__doc__
    for word in ("time-limit", "not under control", "normalisation"):
        assert word in AtcVecEnv.gae.__doc__, word


class _NoLibrary:
    """an env stand-in whose library handle fails the test when anything is called through it"""
    B, N = 3, 2

    class _lib:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    _lib = _lib()

    def __init__(self):
        import torch
        self.torch = torch
        self.device = torch.device("cpu")


def test_the_method_refuses_before_any_library_call():
    import torch
    from atc_hip.vec_env import AtcVecEnv
    env = _NoLibrary()
    B, NV, D, hold = 3, 2, 4, 2
    ok = dict(reward=torch.zeros(D * hold, B), done=torch.zeros(D * hold, B, dtype=torch.uint8), values=torch.zeros(D + 1, B, NV))

    def refused(match, hold=hold, **kw):
        with pytest.raises(ValueError, match=match):
            AtcVecEnv.gae(env, **dict(ok, **{k: v for k, v in kw.items() if k in ok}), hold=hold, **{k: v for k, v in kw.items() if k not in ok})
    for h in (0, 256, -1):
        refused("hold", hold=h)
    for v in (torch.zeros(D + 1, B + 1, NV), torch.zeros(1, B, NV), torch.zeros(D + 1), torch.zeros(D + 1, B, NV, 1), np.zeros((D + 1, B, NV), np.float32)):
        refused("values", values=v)
    refused("NV", values=torch.zeros(D + 1, B, 65))
    refused("values", values=torch.zeros(D + 1, B, NV, dtype=torch.float64))
    refused("values", values=torch.zeros(D + 1, NV, B).transpose(1, 2))
    refused("values", values=torch.zeros(D + 1, B, NV, device="meta"))
    for r in (torch.zeros(D * hold + 1, B), torch.zeros(D * hold, B, NV + 1), torch.zeros(D * hold), torch.zeros(D * hold, B, dtype=torch.float64),
              torch.zeros(B, D * hold).t(), torch.zeros(D * hold, B, device="meta")):
        refused("reward", reward=r)
    for d in (torch.zeros(D * hold, B), torch.zeros(D * hold, B, NV, dtype=torch.uint8), torch.zeros(D * hold, B, dtype=torch.bool),
              torch.zeros(B, D * hold, dtype=torch.uint8).t()):
        refused("done", done=d)
    refused("gamma", gamma=float("nan"))
    refused("gamma", gamma=1e39)
    refused("lam", lam=float("inf"))
    refused("adv_next", adv_next=torch.zeros(B))
    refused("adv_next", adv_next=torch.zeros(B, NV, dtype=torch.float64))
    good = dict(adv=torch.zeros(D, B, NV), ret=torch.zeros(D, B, NV))
    refused("out", out=[good["adv"], good["ret"]])
    refused("out", out=dict(adv=good["adv"]))
    refused("out", out=dict(good, values=good["adv"]))
    refused(r"out\['ret'\]", out=dict(good, ret=torch.zeros(D, B)))
    refused(r"out\['block_reward'\]", out=dict(good, block_reward=torch.zeros(D, B, NV)))
    refused(r"out\['block_done'\]", out=dict(good, block_done=torch.zeros(D, B)))
    refused(r"out\['block_steps'\]", out=dict(good, block_steps=torch.zeros(D, B + 1, dtype=torch.uint8)))
    with pytest.raises(AssertionError, match="the library was called"):      # ... and a call that passes them all goes to the library
        AtcVecEnv.gae(env, **ok, hold=hold, out=good)


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatement
def _scalar(reward, done, values, hold, gamma, lam, per_decision=False, adv_next=None):
    """the header's text as a plain loop on numpy float32 scalars, one column at a time"""
    f = np.float32
    values = np.asarray(values, f)
    D, B, NV = values.shape[0] - 1, values.shape[1], values.shape[2]
    reward = np.asarray(reward, f)
    per_column = reward.ndim == 3
    gam, lm = f(gamma), f(lam)
    adv, ret = np.zeros((D, B, NV), f), np.zeros((D, B, NV), f)
    br = np.zeros((D, B, NV) if per_column else (D, B), f)
    bd, bs = np.zeros((D, B), np.uint8), np.zeros((D, B), np.uint8)
    with np.errstate(all="ignore"):
        Gc = f(1.0)
        for _ in range(hold):
            Gc = f(Gc * gam)
        if per_decision:
            Gc = gam
        c = f(Gc * lm)
        for e in range(B):
            for k in range(NV):
                rw = (lambda t: reward[t, e, k]) if per_column else (lambda t: reward[t, e])      # noqa: E731
                A_next = f(0.0) if adv_next is None else f(adv_next[e, k])
                for d in range(D - 1, -1, -1):
                    t0 = d * hold
                    g, R, n, term = f(1.0), f(rw(t0)), 1, done[t0, e] != 0
                    j = 1
                    while j < hold and not term:
                        if per_decision:
                            R = f(R + rw(t0 + j))
                        else:
                            g = f(g * gam)
                            R = f(R + f(rw(t0 + j) * g))
                        n += 1
                        term = done[t0 + j, e] != 0
                        j += 1
                    if term:
                        A = f(R - values[d, e, k])
                    else:
                        delta = f(f(R + f(Gc * values[d + 1, e, k])) - values[d, e, k])
                        A = f(delta + f(c * A_next))
                    adv[d, e, k], ret[d, e, k], A_next = A, f(A + values[d, e, k]), A
                    if per_column:
                        br[d, e, k] = R
                    else:
                        br[d, e] = R
                    bd[d, e], bs[d, e] = term, n
    return {"adv": adv, "ret": ret, "block_reward": br, "block_done": bd, "block_steps": bs}


KEYS = ("adv", "ret", "block_reward", "block_done", "block_steps")


def _same(got, ref, tag):
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, k, a.shape, b.shape, a.dtype, b.dtype)
        bad = np.argwhere(G.words(a) != G.words(b))
        assert len(bad) == 0, "%s: %s differs in %d words, first at %s: %r != %r" % (tag, k, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def _hand(dones, hold, B=2, NV=2, seed=0, per_column=False):
    """rewards and values of small integers and halves (every sum below is exact or nearly so) with the given done steps [(t, e)]"""
    rng = np.random.default_rng(seed)
    done = np.asarray(dones, np.uint8)
    T = done.shape[0]
    D = T // hold
    reward = rng.uniform(-3, 3, (T, B, NV) if per_column else (T, B)).astype(np.float32)
    values = rng.uniform(-3, 3, (D + 1, B, NV)).astype(np.float32)
    return reward, done, values


def _dones(T, B, at):
    d = np.zeros((T, B), np.uint8)
    for t, e in at:
        d[t, e] = 1
    return d


def test_restatement_equals_the_scalar_loop_on_hand_cases():
    cases = {
        "hold 1, textbook": (_dones(6, 2, [(2, 0), (5, 1)]), 1, 0.99, 0.95),
        "a done in the middle of a block": (_dones(8, 2, [(1, 0), (6, 1)]), 4, 0.9, 0.8),
        "a done at the first and at the last step of a block": (_dones(8, 2, [(0, 0), (4, 1), (7, 0), (3, 1)]), 4, 0.9, 0.8),
        "two dones in one block": (_dones(8, 2, [(1, 0), (3, 0), (4, 1), (5, 1)]), 4, 0.9, 0.8),
        "gamma 0": (_dones(6, 2, [(2, 0)]), 3, 0.0, 0.5),
        "lam 0": (_dones(6, 2, [(4, 1)]), 2, 0.9, 0.0),
        "lam 1, gamma 1, no done": (_dones(6, 2, []), 2, 1.0, 1.0),
    }
    for name, (done, hold, gamma, lam) in cases.items():
        for per_column in (False, True):
            for per_decision in (False, True):
                reward, _, values = _hand(done, hold, per_column=per_column, seed=len(name))
                for nxt in (None, np.full((2, 2), 0.75, np.float32)):
                    got = G.gae(reward, done, values, hold, gamma, lam, per_decision, nxt)
                    _same(got, _scalar(reward, done, values, hold, gamma, lam, per_decision, nxt), name)
    # what the cases are about, on the restatement itself
    reward, done, values = _hand(_dones(8, 2, [(1, 0), (3, 0)]), 4)
    got = G.gae(reward, done, values, 4, 0.9, 0.8)
    assert got["block_steps"][0, 0] == 2 and got["block_done"][0, 0] == 1 and got["block_steps"][0, 1] == 4 and got["block_done"][0, 1] == 0
    assert got["block_reward"][0, 0] == np.float32(reward[0, 0] + np.float32(reward[1, 0] * np.float32(0.9)))
    assert np.array_equal(got["adv"][0, 0], got["block_reward"][0, 0] - values[0, 0])          # a block that ended: A = R - V[d]
    first, last = G.gae(*_hand(_dones(4, 1, [(0, 0)]), 4, B=1), 4, 0.9, 0.8), G.gae(*_hand(_dones(4, 1, [(3, 0)]), 4, B=1), 4, 0.9, 0.8)
    assert first["block_steps"][0, 0] == 1 and last["block_steps"][0, 0] == 4 and first["block_done"][0, 0] == last["block_done"][0, 0] == 1
    # lam = 0: adv is delta;  lam = 1 = gamma without dones: ret is the reward-to-go plus V[D] (small integers: every sum is exact)
    rng = np.random.default_rng(5)
    reward = rng.integers(-3, 4, (6, 2)).astype(np.float32)
    values = rng.integers(-3, 4, (4, 2, 2)).astype(np.float32)
    none = _dones(6, 2, [])
    got = G.gae(reward, none, values, 2, 1.0, 0.0)
    R = reward.reshape(3, 2, 2).sum(axis=1)[:, :, None]
    assert np.array_equal(got["adv"], R + values[1:] - values[:-1])
    got = G.gae(reward, none, values, 2, 1.0, 1.0)
    to_go = np.cumsum(R[::-1], axis=0)[::-1]
    assert np.array_equal(got["ret"], to_go + values[3][None])
    got = G.gae(reward, none, values, 2, 0.0, 0.5)          # gamma = 0: nothing behind a block's first reward counts
    assert np.array_equal(got["adv"], reward[0::2][:, :, None] - values[:-1]) and np.array_equal(got["block_steps"], np.full((3, 2), 2, np.uint8))


# ---- the synthetic cases: rewards and values uniform in [-3, 3], dones Bernoulli or forced onto the block boundaries
SHAPES = ((3, 1), (7, 5), (5, 13), (40, 16), (4, 64), (130, 1))      # (B, NV): 65 columns at (5, 13) — an env straddles the wavefront boundary
RUNS = ((1, 1), (2, 1), (7, 3), (5, 20), (3, 255))                   # (D, hold)
GAMMA_LAM = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.5), (0.9, 0.0))
RATES = (0.0, 0.05, 0.5, 1.0, "boundary")
N_CASES = 30


@functools.lru_cache(maxsize=None)
def _case(k):
    B, NV = SHAPES[k % 6]
    D, hold = RUNS[k % 5]
    gamma, lam = GAMMA_LAM[k % 4]
    rate = RATES[(k + k // 5) % 5]
    per_decision, per_column, given = bool((k // 2) % 2), bool((k // 3) % 2), bool((k // 4 + k) % 2)
    rng = np.random.default_rng([2024, k])
    T = D * hold
    reward = rng.uniform(-3, 3, (T, B, NV) if per_column else (T, B)).astype(np.float32)
    values = rng.uniform(-3, 3, (D + 1, B, NV)).astype(np.float32)
    if rate == "boundary":
        done = np.zeros((T, B), np.uint8)
        done[hold - 1::hold] = rng.uniform(size=(D, B)) < 0.5
    else:
        done = (rng.uniform(size=(T, B)) < rate).astype(np.uint8) * np.uint8(rng.integers(1, 256))      # (any non-zero byte is a done)
    adv_next = rng.uniform(-3, 3, (B, NV)).astype(np.float32) if given else None
    c = dict(k=k, B=B, NV=NV, D=D, hold=hold, gamma=gamma, lam=lam, rate=rate, per_decision=per_decision, per_column=per_column, reward=reward,
             done=done, values=values, adv_next=adv_next)
    c["ref"] = G.gae(reward, done, values, hold, gamma, lam, per_decision, adv_next, with_bound=True)
    return c


def _tag(c):
    return "case %(k)d B=%(B)d NV=%(NV)d D=%(D)d hold=%(hold)d gamma=%(gamma)g lam=%(lam)g rate=%(rate)s per_decision=%(per_decision)s per_column=%(per_column)s" % c


def test_the_cases_cover_what_they_claim():
    cases = [_case(k) for k in range(N_CASES)]
    assert {(c["B"], c["NV"]) for c in cases} == set(SHAPES) and {(c["D"], c["hold"]) for c in cases} == set(RUNS)
    assert {(c["gamma"], c["lam"]) for c in cases} == set(GAMMA_LAM) and {c["rate"] for c in cases} == set(RATES)
    assert {(c["per_decision"], c["per_column"], c["adv_next"] is None) for c in cases} == {(a, b, n) for a in (False, True) for b in (False, True) for n in (False, True)}
    two = steps = 0
    for rate in (0.05, 0.5):
        early = 0
        for c in cases:
            if c["rate"] != rate or c["hold"] == 1:
                continue
            blocks = c["done"].reshape(c["D"], c["hold"], c["B"]) != 0
            early += int(blocks[:, :-1].any(axis=1).sum())
            two += int((blocks.sum(axis=1) >= 2).sum())
            assert np.array_equal(c["ref"]["block_steps"] < c["hold"], blocks[:, :-1].any(axis=1))
        assert early > 0, rate
    assert two > 0
    for c in cases:
        steps += len(np.unique(c["ref"]["block_steps"])) > 1
        if c["rate"] == "boundary":
            assert np.all(c["ref"]["block_steps"] == c["hold"]) and c["ref"]["block_done"].any() and not c["ref"]["block_done"].all()
    assert steps > 0


def test_float32_restatement_within_the_running_bound_of_the_float64_twin():
    worst = 0.0
    for k in range(N_CASES):
        c = _case(k)
        twin = G.gae(c["reward"], c["done"], c["values"], c["hold"], c["gamma"], c["lam"], c["per_decision"], c["adv_next"], dtype=np.float64)
        for key in ("adv", "ret"):
            dev = np.abs(c["ref"][key].astype(np.float64) - twin[key])
            bound = c["ref"][key + "_bound"]
            assert np.all(np.isfinite(bound)) and np.all(dev <= bound), (_tag(c), key, float((dev / np.maximum(bound, 1e-300)).max()))
            nz = bound > 0
            if nz.any():
                worst = max(worst, float((dev[nz] / bound[nz]).max()))
            assert np.all(dev[~nz] == 0)
        for key in ("block_done", "block_steps"):
            assert np.array_equal(c["ref"][key], twin[key])
    print("float32 restatement against the float64 twin: largest deviation / bound = %.4f" % worst)
    assert 0 < worst <= 1


def test_split_property_on_the_restatement():
    for k in range(N_CASES):
        c = _case(k)
        got = G.split(c["reward"], c["done"], c["values"], hold=c["hold"], adv_next=c["adv_next"], gamma=c["gamma"], lam=c["lam"], per_decision=c["per_decision"])
        _same(got, c["ref"], _tag(c))


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _env(B, N=1, traffic=0, cfg=False):
    """an env of B: atc_gae reads nothing of it but the device.  cfg: the normalised, shaped, auto-reset, time-limit-4 configuration of
    tests/test_rollout_policy.py, in which envs end and reset inside a held block"""
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import model, scenarios
    env = AtcVecEnv(B, N, sim_parameters=model.SimParameters(1, reward_shaping=True, normalize_state=True), scenario=scenarios.LOWWDense(), auto_reset=True,
                    spawn="lattice", seed=11, grid_cell=0.5, timestep_limit=4 if cfg else 6000, sep_nm=5.0 if N <= 8 else 13.0 if N <= 16 else 3.0,
                    traffic=traffic)
    env.synchronize()
    return env


def _dev(env, a):
    import torch
    return None if a is None else torch.as_tensor(a, device=env.device)


def _guarded(env, c, names=KEYS):
    """pattern-filled output buffers with GUARD rows in front and behind: (the out= dict of the middle rows, the whole buffers)"""
    import torch
    B, NV, D = c["B"], c["NV"], c["D"]
    shape = {"adv": (B, NV), "ret": (B, NV), "block_reward": (B, NV) if c["per_column"] else (B,), "block_done": (B,), "block_steps": (B,)}
    whole = {n: torch.full((D + 2 * GUARD,) + shape[n], PATTERN, dtype=torch.uint8 if n in ("block_done", "block_steps") else torch.float32, device=env.device)
             for n in names}
    for n in names:
        if whole[n].dtype == torch.float32:
            whole[n].view(torch.uint8).fill_(PATTERN)
    return {n: t[GUARD:GUARD + D] for n, t in whole.items()}, whole


def _run(env, c, out=None, **over):
    a = dict(c, **over)
    return env.gae(_dev(env, a["reward"]), _dev(env, a["done"]), _dev(env, a["values"]), hold=a["hold"], gamma=a["gamma"], lam=a["lam"],
                   per_decision=a["per_decision"], adv_next=_dev(env, a["adv_next"]), out=out)


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(N_CASES))
def test_every_word_equals_the_restatement(k):
    import torch
    c = _case(k)
    env = _env(c["B"])
    out, whole = _guarded(env, c)
    before = _records()
    got = _run(env, c, out=out)
    torch.cuda.synchronize()
    after = _records()
    assert all(got[n] is out[n] for n in KEYS)
    _same(_host(got), c["ref"], _tag(c))
    for n, t in whole.items():      # nothing in front of or behind the D rows was written
        edge = torch.cat([t[:GUARD], t[GUARD + c["D"]:]]).contiguous().view(torch.uint8)
        assert bool((edge == PATTERN).all()), (_tag(c), n)
    assert after[0] == {"gae": before[0].get("gae", 0) + 1} and after[1:] == before[1:], "only atc_gae_launch_counts moves"
    # without out=: the same words in fresh tensors of the documented shapes
    _same(_host(_run(env, c)), c["ref"], _tag(c) + " (no out)")


@pytest.mark.gpu
def test_two_calls_split_at_half_equal_one():
    for k in (2, 3, 4, 7, 13, 24):
        c = _case(k)
        env = _env(c["B"])
        D, hold, h = c["D"], c["hold"], c["D"] // 2
        assert h >= 1
        late = _run(env, c, reward=c["reward"][h * hold:], done=c["done"][h * hold:], values=c["values"][h:])
        early = env.gae(_dev(env, c["reward"][:h * hold]), _dev(env, c["done"][:h * hold]), _dev(env, c["values"][:h + 1]), hold=hold, gamma=c["gamma"],
                        lam=c["lam"], per_decision=c["per_decision"], adv_next=late["adv"][0].contiguous())
        early, late = _host(early), _host(late)
        _same({n: np.concatenate([early[n], late[n]]) for n in KEYS}, c["ref"], _tag(c))


@pytest.mark.gpu
def test_out_carries_the_buffers_and_nothing_is_allocated():
    import torch
    c = _case(9)
    env = _env(c["B"])
    args = [_dev(env, c[n]) for n in ("reward", "done", "values")]
    nxt = _dev(env, c["adv_next"])
    out, _ = _guarded(env, c)
    call = lambda o: env.gae(*args, hold=c["hold"], gamma=c["gamma"], lam=c["lam"], per_decision=c["per_decision"], adv_next=nxt, out=o)      # noqa: E731
    call(out)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(env.device)
    got = call(out)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(env.device) == before
    assert all(got[n] is out[n] for n in KEYS)
    _same(_host(got), c["ref"], _tag(c))
    # the block outputs are stored only where out names them
    two, whole = _guarded(env, c, ("adv", "ret", "block_steps"))
    got = call(two)
    assert set(got) == {"adv", "ret", "block_steps"}
    for n in got:
        assert np.array_equal(G.words(got[n].cpu().numpy()), G.words(c["ref"][n])), n
    with pytest.raises(RuntimeError, match="overlaps"):
        call(dict(out, ret=out["adv"]))
    with pytest.raises(ValueError, match="values"):
        env.gae(args[0], args[1], args[2].cpu(), hold=c["hold"])


@pytest.mark.gpu
def test_words_behind_a_blocks_first_done_reach_no_output():
    hit = 0
    for k in (7, 8, 13, 14, 19, 22):
        c = _case(k)
        if c["hold"] == 1:
            continue
        env = _env(c["B"])
        D, hold, B = c["D"], c["hold"], c["B"]
        blocks = c["done"].reshape(D, hold, B) != 0
        behind = (np.cumsum(blocks, axis=1) - blocks) > 0                    # steps after the block's first done
        behind = behind.reshape(D * hold, B)
        hit += int(behind.sum())
        reward = c["reward"].copy()
        reward[behind] = np.nan
        done = c["done"].copy()
        done[behind] ^= 0xFF                                               # a done becomes 0 there, everything else 0xFF
        _same(_host(_run(env, c, reward=reward, done=done)), c["ref"], _tag(c))
    assert hit > 100


@pytest.mark.gpu
def test_a_nan_in_values_is_the_quiet_nan_where_the_restatement_has_one():
    c = _case(13)
    env = _env(c["B"])
    values = c["values"].copy()
    rng = np.random.default_rng(3)
    values[rng.uniform(size=values.shape) < 0.1] = np.float32(np.nan)
    values.view(np.uint32)[np.isnan(values)] = 0xFFC12345                 # (a signalling-free NaN with a sign and a payload)
    ref = G.gae(c["reward"], c["done"], values, c["hold"], c["gamma"], c["lam"], c["per_decision"], c["adv_next"])
    got = _host(_run(env, c, values=values))
    _same(got, ref, _tag(c))
    for n in ("adv", "ret"):
        nan = np.isnan(ref[n])
        assert nan.any() and not nan.all() and np.all(G.words(got[n])[nan] == G.QNAN) and not np.isnan(got[n][~nan]).any()


@pytest.mark.gpu
def test_refusals_behind_the_pointer_checks_on_the_device():
    import torch
    from atc_hip import lib
    h = lib.load()
    B, NV, D, hold = 3, 5, 4, 2
    env = _env(B)
    Cn, T = B * NV, D * hold
    pool = torch.zeros(9 * 4096, dtype=torch.uint8, device=env.device)      # nine ranges 4 KiB apart, each larger than any array here
    names = ("reward", "done", "values", "adv_next") + lib.GAE_OUT_FIELDS
    base = dict(s=env.sector.handle, **{n: pool.data_ptr() + 4096 * k for k, n in enumerate(names)})
    call, err = _gae_call(h), h.atc_last_error
    before = _records()
    out = lib.AtcGaeOut(*[base[n] for n in lib.GAE_OUT_FIELDS])
    ptrs = dict(s=base["s"], reward=C.c_void_p(base["reward"]), done=C.c_void_p(base["done"]), values=C.c_void_p(base["values"]), out=C.byref(out))
    with torch.cuda.device(env.device):
        for flags in (4, 8, 0x80000000, 7):
            g = lib.AtcGae(np.nan, np.nan, flags, 0)
            assert call(B=B, NV=NV, D=D, hold=hold, g=C.byref(g), **ptrs) == -1 and b"flags" in err()
        for gm, lm, word in ((np.nan, 0.5, b"gamma"), (np.inf, np.nan, b"gamma"), (-np.inf, 0.5, b"gamma"), (0.5, np.nan, b"lam"), (0.5, np.inf, b"lam")):
            g = lib.AtcGae(gm, lm, 3, 0)
            assert call(B=B, NV=NV, D=D, hold=hold, g=C.byref(g), **dict(ptrs, done=ptrs["reward"])) == -1 and word in err()
        for per_column in (False, True):
            n, run, size = _overlap_pairs(call, err, base, B, NV, D, hold, per_column)
            assert n == 36 * 3
        assert _records() == before, "a refused call moved a launch record"
        # ranges that only touch are accepted: the nine arrays packed back to back
        at, packed = pool.data_ptr(), {}
        for n in names:
            packed[n] = at
            at += size[n]
        assert run(dict(base, **packed)) == 0, err()
        torch.cuda.synchronize()
    assert _records()[0] == {"gae": before[0].get("gae", 0) + 1}


# ---- end to end behind the policy rollout
def _critic(rows):
    """a fixed linear map of the input words (the ten own words, and the traffic words where the rows have them), one value per aircraft"""
    import torch
    w = torch.linspace(-0.5, 0.5, rows.shape[-1], dtype=torch.float32, device=rows.device)
    return (rows * w).sum(dim=-1) + 0.25


def _rows(env, out, obs0, hold):
    import torch
    T = out["obs"].shape[0]
    D = T // hold
    own = torch.cat([obs0.reshape(1, env.B, env.N, L.OBS_DIM), out["obs"].reshape(D, hold, env.B, env.N, L.OBS_DIM)[:, hold - 1]])
    return own


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", ((7, 5), (40, 16)))
def test_end_to_end_behind_rollout_policy_and_collect(B, N):
    import torch
    from atc_hip import ppo
    w = P.random_weights(np.random.default_rng([17, 1]), 1.0, (-0.5, -1.0, 0.25))
    A, Bv = _env.__wrapped__(B, N, cfg=True), _env.__wrapped__(B, N, cfg=True)      # two envs built alike: one for the calls by hand, one for collect
    start = [(H.snapshot(e), e.obs.clone()) for e in (A, Bv)]
    wd = torch.as_tensor(w, device=A.device)
    any_done = inside = 0
    for T, hold in ((6, 1), (6, 3)):
        for per_decision in (False, True):
            for e, (snap, obs) in zip((A, Bv), start):
                H.restore(e, snap)
                e.obs.copy_(obs)
            obs0 = A.obs.clone()
            out = A.rollout_policy(wd, T, hold=hold, seed=5, decision0=3, obs0=obs0)
            values = _critic(_rows(A, out, obs0, hold)).contiguous()
            assert tuple(values.shape) == (T // hold + 1, B, N)
            got = A.gae(out["reward"], out["done"], values, hold=hold, gamma=0.99, lam=0.95, per_decision=per_decision)
            ref = G.gae(out["reward"].cpu().numpy(), out["done"].cpu().numpy(), values.cpu().numpy(), hold, 0.99, 0.95, per_decision)
            _same(_host(got), ref, "end to end (%d, %d) T=%d hold=%d" % (B, N, T, hold))
            done = out["done"].cpu().numpy().reshape(T // hold, hold, B) != 0
            any_done += int(done.sum())
            inside += int(done[:, :-1].any(axis=1).sum()) if hold > 1 else 0
            res = ppo.collect(Bv, wd, _critic, T, hold=hold, gamma=0.99, lam=0.95, seed=5, decision0=3, per_decision=per_decision)
            for n in ("obs", "reward", "done", "flags", "action", "logp"):
                assert torch.equal(res[n], out[n]), n
            assert np.array_equal(G.words(res["values"].cpu().numpy()), G.words(values.cpu().numpy()))
            _same(_host({n: res[n] for n in KEYS}), ref, "collect (%d, %d) T=%d hold=%d" % (B, N, T, hold))
    assert any_done > 0 and inside > 0, "no env ended inside a held block"


@pytest.mark.gpu
def test_collect_with_traffic_equals_the_three_calls_by_hand():
    import torch
    from atc_hip import policy, ppo
    B, N, K, T, hold = 7, 5, 2, 6, 3
    w = PT.random_weights(np.random.default_rng([17, 2]), K)
    A, Bv = _env.__wrapped__(B, N, traffic=K, cfg=True), _env.__wrapped__(B, N, traffic=K, cfg=True)
    wd = torch.as_tensor(w, device=A.device)
    obs0 = A.obs.clone()
    out = A.rollout_policy_traffic(wd, T, K, hold=hold, seed=5, decision0=3, obs0=obs0)
    rows = policy.input_rows(_rows(A, out, obs0, hold), torch.cat([out["traffic"], A.observe_traffic().reshape(1, B, N, K, L.TRAFFIC_DIM)]))
    assert tuple(rows.shape) == (T // hold + 1, B, N, L.policy_in(K))
    values = _critic(rows).contiguous()
    got = A.gae(out["reward"], out["done"], values, hold=hold, gamma=0.99, lam=0.95)
    ref = G.gae(out["reward"].cpu().numpy(), out["done"].cpu().numpy(), values.cpu().numpy(), hold, 0.99, 0.95)
    _same(_host(got), ref, "by hand, traffic")
    res = ppo.collect(Bv, torch.as_tensor(w, device=Bv.device), _critic, T, hold=hold, traffic=K, gamma=0.99, lam=0.95, seed=5, decision0=3)
    for n in ("obs", "reward", "done", "flags", "action", "logp", "traffic"):
        assert torch.equal(res[n], out[n]), n
    assert np.array_equal(G.words(res["values"].cpu().numpy()), G.words(values.cpu().numpy()))
    _same(_host({n: res[n] for n in KEYS}), ref, "collect, traffic")
    with pytest.raises(ValueError, match="traffic"):
        ppo.collect(_env(B), wd, _critic, T, hold=hold, traffic=K)
