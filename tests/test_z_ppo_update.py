"""The update half of a PPO iteration in the library (include/atc_step.h: atc_adv_normalise, atc_adam_step; AtcVecEnv.adv_normalise,
AtcVecEnv.adam_step; atc_hip/ppo.py: adam_state, update): the advantages normalised without a host read, and the gradient-norm clip, the
entropy term and Adam on both packed tensors in one launch.

CPU: the four declarations, exports, launch records, constants, structs and argtypes across the header, atc_hip/layout.py and atc_hip/lib.py
(ABI 22, 57 step slots); the refusals of both entry points through ctypes with made-up pointers; tests/ppo_update_ref.py (the numpy restatement
in the kernels' order) against plain numpy float64 mean / std(ddof=1) within 1e-12, and against clip_grad_norm_ + torch.optim.Adam in float64
over 6 steps on two tensors: within 1e-6 of the largest |w| with float32 stores, within 1e-12 with float64 stores; the entropy window; the
NaN skip.
GPU: adv_normalise and adam_step against the restatement BIT FOR BIT on every stored word; the statistics of adv_normalise against the
float64 values within 4 x the deviation of torch's own float32 mean / std / scale on the same data (printed before it is asserted);
ppo_policy_grad on (out_adv, 0, 1) against (adv, mean, scale): the same bits; ppo.update against the same calls issued by hand, its
permutations, its launch records; ppo.update with every host synchronisation turned into an error.

Measured on an MI355X: every word of out_adv, stats, w, m and v equal to the restatement; adv_normalise's mean, scale and std deviation / bar
at most 0.25 (the bar is 4 x torch's deviation, so 0.25 is where both round the same value) — DESIGN.md section 3r."""
import ctypes as C
import functools
import inspect
import re

import numpy as np
import pytest

import helpers as H
import policy_ref as P
import ppo_update_ref as U
import ppo_value_ref as PV
from atc_hip import layout as L
from held_tools import HEADER, struct_fields

NAMES = ("atc_adv_normalise", "atc_adv_normalise_launch_counts", "atc_adam_step", "atc_adam_step_launch_counts")
RECORDS = {"atc_adv_normalise_launch_counts": 1, "atc_adam_step_launch_counts": 2}
FAKE = C.c_void_p(0x100000)
INF = float("inf")
SENTINEL = -12345.5
LOG_STD = L.POLICY_WORDS - 3


def _same(a, b):
    """two arrays equal bit for bit"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _records():
    from atc_hip import lib
    return lib.launch_records()


def _moved(before, after):
    """{getter: {slot: count}} of what moved between two launch_records()"""
    out = {}
    for getter in after:
        d = {k: v - before[getter].get(k, 0) for k, v in after[getter].items() if v != before[getter].get(k, 0)}
        if d:
            out[getter] = d
    return out


def _at(k):
    return 0x100000 + k * 0x10000000      # made-up ranges 256 MiB apart


# ---------------------------------------------------------------------------------------------------------------- CPU: the ABI
def test_header_exports_records_and_layout_agree():
    from atc_hip import lib, policy
    text = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(atc_\w+)\(", text, flags=re.M))
    assert set(NAMES) <= declared and set(NAMES) <= set(lib.EXPORTS) and set(lib.EXPORTS) == declared | {"atc_last_error"}
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, text).group(1))      # noqa: E731
    assert L.ABI_VERSION == 22 and define("ATC_ABI_VERSION") == 22 and L.LAUNCH_SLOTS == 57
    for n in ("ADV_TILE", "ADV_MAX_WG", "ADV_DEFAULT_WG", "ADV_STATS", "ADAM_BLOCK", "ADAM_MAX_WORDS", "ADAM_STATS"):
        assert getattr(L, n) == define("ATC_" + n), n
    assert (L.ADV_TILE, L.ADV_MAX_WG, L.ADV_DEFAULT_WG, L.ADV_STATS) == (U.TILE, U.MAX_WG, U.DEFAULT_WG, U.ADV_STATS) == (256, 1024, 256, 4)
    assert (L.ADAM_BLOCK, L.ADAM_MAX_WORDS, L.ADAM_STATS) == (U.ADAM_BLOCK, U.ADAM_MAX_WORDS, U.ADAM_STATS) == (1024, 65536, 4)
    for k, n in enumerate(("N", "MEAN", "SCALE", "STD")):
        assert define("ATC_ADV_STAT_" + n) == getattr(L, "ADV_STAT_" + n) == k
    for k, n in enumerate(("NORM", "COEF", "SKIPPED", "STEP")):
        assert define("ATC_ADAM_STAT_" + n) == getattr(L, "ADAM_STAT_" + n) == k
    assert (U.STAT_N, U.STAT_MEAN, U.STAT_SCALE, U.STAT_STD) == (U.ASTAT_NORM, U.ASTAT_COEF, U.ASTAT_SKIPPED, U.ASTAT_STEP) == tuple(range(4))
    assert L.ADV_NORMALISE_LAUNCH_SLOTS == int(re.search(r"ATC_ADV_NORMALISE_LAUNCH_SLOTS = (\d+)", text).group(1)) == 1
    assert L.ADAM_STEP_LAUNCH_SLOTS == int(re.search(r"ATC_ADAM_STEP_LAUNCH_SLOTS = (\d+)", text).group(1)) == 2
    assert [L.adv_workgroups(R) for R in (1, 256, 257, 256 * 256, 10 ** 7)] == [U.workgroups(R) for R in (1, 256, 257, 256 * 256, 10 ** 7)] == [1, 1, 2, 256, 256]
    assert L.adv_workgroups(10 ** 7, 3) == 3
    ctype = {"float": C.c_float, "int32_t": C.c_int32, "double": C.c_double}
    for struct, fields, cls, size in (("atc_adv_norm", lib.ADV_NORM_FIELDS, lib.AtcAdvNorm, 8), ("atc_adam", lib.ADAM_FIELDS, lib.AtcAdam, 48)):
        f = struct_fields(text, struct)
        assert [x[1] for x in f] == list(fields) == [x[0] for x in cls._fields_], struct
        assert [ctype[x[0]] for x in f] == [x[1] for x in cls._fields_] and C.sizeof(cls) == size, struct
    o = struct_fields(text, "atc_adv_norm_out")
    assert [x[1].lstrip("*") for x in o] == list(lib.ADV_NORM_OUT_FIELDS) == [x[0] for x in lib.AtcAdvNormOut._fields_] == ["out_adv", "stats", "scratch"]
    assert [x[0] for x in o] == ["float", "float", "double"] and all(x[1].startswith("*") for x in o) and C.sizeof(lib.AtcAdvNormOut) == 24
    t = struct_fields(text, "atc_adam_tensor")
    assert [x[1].lstrip("*") for x in t] == list(lib.ADAM_TENSOR_FIELDS) == [x[0] for x in lib.AtcAdamTensor._fields_]
    assert [x[1].startswith("*") for x in t] == [True] * 4 + [False] * 5 and C.sizeof(lib.AtcAdamTensor) == 56
    assert [ctype[x[0]] for x in t[4:]] == [x[1] for x in lib.AtcAdamTensor._fields_[4:]]
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    assert list(h.atc_adv_normalise.argtypes) == [vp, ci, vp, vp, C.POINTER(lib.AtcAdvNorm), C.POINTER(lib.AtcAdvNormOut), vp]
    assert list(h.atc_adam_step.argtypes) == [vp, ci, C.POINTER(lib.AtcAdamTensor), C.POINTER(lib.AtcAdam), vp, vp]
    for name in NAMES:
        assert hasattr(h, name) and getattr(h, name).restype is ci, name
    for name, slots in RECORDS.items():
        assert lib.LAUNCH_RECORDS[name][0] == slots and list(getattr(h, name).argtypes) == [C.POINTER(C.c_uint64), ci]
        buf = (C.c_uint64 * 4)(*([99] * 4))
        assert getattr(h, name)(buf, 4) == 0 and all(v != 99 for v in buf[:slots]) and all(v == 99 for v in buf[slots:])
        assert getattr(h, name)(None, 1) == -1 and name in lib.launch_records()
    assert lib.LAUNCH_RECORDS["atc_adv_normalise_launch_counts"][1] == "adv_normalise"
    assert [lib.LAUNCH_RECORDS["atc_adam_step_launch_counts"][1](i) for i in range(2)] == [1, 2]
    assert isinstance(lib.adv_normalise_launch_counts(), dict) and isinstance(lib.adam_step_launch_counts(), dict)
    assert policy.offsets(0)["log_std"][0] == LOG_STD


def test_python_surface():
    from atc_hip import ppo
    from atc_hip.vec_env import AtcVecEnv
    sig = inspect.signature(AtcVecEnv.adv_normalise)
    assert list(sig.parameters) == ["self", "adv", "mask", "eps", "workgroups", "out"]
    assert [sig.parameters[k].default for k in ("mask", "eps", "workgroups", "out")] == [None, 1e-8, 0, None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("eps", "workgroups", "out"))
    sig = inspect.signature(AtcVecEnv.adam_step)
    assert list(sig.parameters) == ["self", "tensors", "lr", "step", "beta1", "beta2", "eps", "max_norm", "out"]
    assert [sig.parameters[k].default for k in ("beta1", "beta2", "eps", "max_norm", "out")] == [0.9, 0.999, 1e-5, 0.0, None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[2:])
    assert list(inspect.signature(ppo.adam_state).parameters) == ["env", "w", "vw"]
    sig = inspect.signature(ppo.update)
    assert list(sig.parameters) == ["env", "collected", "w", "vw", "state", "epochs", "minibatches", "clip", "vclip", "lr", "ent_coef", "vf_coef", "max_grad_norm", "eps",
                                    "perm", "seed"]
    assert [p.default for p in list(sig.parameters.values())[5:]] == [4, 4, 0.2, 0.2, 3e-4, 0.0, 0.5, 0.5, 1e-5, None, 0]
    # what was there stays as it was
    assert list(inspect.signature(ppo.policy_grad).parameters) == ["env", "collected", "weights", "index", "clip", "normalise", "workgroups", "out"]
    assert inspect.signature(ppo.policy_grad).parameters["normalise"].default is True
    assert "update" in ppo.__doc__ and "adam_state" in ppo.__doc__
    # update() reads no device value on the host: none of the calls that do stands in its source
    src = inspect.getsource(ppo.update) + inspect.getsource(ppo.adam_state)
    for word in ("float(", ".item(", ".cpu(", ".tolist(", "bool(", ".nonzero(", ".numpy("):
        assert word not in src.replace("float(ent_coef)", ""), word


def _adv_call(h, R=5, mask=None, **kw):
    a = dict.fromkeys(("s", "adv", "g", "out"))
    a.update(kw)
    return h.atc_adv_normalise(a["s"], R, a["adv"], mask, a["g"], a["out"], None)


def test_adv_normalise_refusals_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    err = h.atc_last_error
    g = lib.AtcAdvNorm(1e-8, 0)
    out = lib.AtcAdvNormOut(_at(3), _at(4), _at(5))
    ok = dict(s=FAKE, adv=C.c_void_p(_at(1)), g=C.byref(g), out=C.byref(out))
    ptrs = ("s", "adv", "g", "out")
    for j, name in enumerate(ptrs):
        named = re.compile(rb"null pointer: %s\b" % name.encode())
        assert _adv_call(h, 0, **{k: ok[k] for k in ptrs[:j]}) == -1 and named.search(err()), (name, err())
        assert _adv_call(h, 0, **dict(ok, **{name: None})) == -1 and named.search(err()), (name, err())
    for o, word in ((lib.AtcAdvNormOut(None, None, None), b"out->stats"), (lib.AtcAdvNormOut(None, _at(4), None), b"out->scratch")):
        assert _adv_call(h, 0, **dict(ok, out=C.byref(o))) == -1 and b"null pointer: " + word in err(), err()
    for R in (0, -1):
        assert _adv_call(h, R, **dict(ok, g=C.byref(lib.AtcAdvNorm(-1.0, -1)))) == -1 and b"R (" in err()
    for eps in (-1e-8, float("nan"), INF):
        assert _adv_call(h, 5, **dict(ok, g=C.byref(lib.AtcAdvNorm(eps, -1)))) == -1 and b"eps" in err(), eps
    for wg in (-1, 1025):
        assert _adv_call(h, 5, **dict(ok, g=C.byref(lib.AtcAdvNorm(0.0, wg)))) == -1 and b"workgroups" in err() and b"1024" in err()
    # the overlap rule on pointer values; out_adv == adv is the one pair let through, and only as equal pointers
    R, G = 600, 3
    size = dict(adv=R * 4, mask=R, out_adv=R * 4, stats=16, scratch=G * 24)
    base = {n: _at(k + 1) for k, n in enumerate(size)}
    gk = lib.AtcAdvNorm(1e-8, G)

    def run(p):
        o = lib.AtcAdvNormOut(p["out_adv"], p["stats"], p["scratch"])
        return _adv_call(h, R, mask=C.c_void_p(p["mask"]), s=FAKE, adv=C.c_void_p(p["adv"]), g=C.byref(gk), out=C.byref(o))
    names, n = list(size), 0
    for b in ("out_adv", "stats", "scratch"):
        for a in names[:names.index(b)]:
            for off in (0, size[a] - 1, -(size[b] - 1)):
                if (a, b, off) == ("adv", "out_adv", 0):
                    continue
                assert run(dict(base, **{b: base[a] + off})) == -1 and b"overlaps" in err() and a.encode() in err() and b.encode() in err(), (a, b, off, err())
                n += 1
    assert n == (2 + 3 + 4) * 3 - 1
    assert _records() == before, "a refused call moved a launch record"


def _tensor(k, words=10, **kw):
    from atc_hip import lib
    f = dict(w=_at(1 + 4 * k), grad=_at(2 + 4 * k), m=_at(3 + 4 * k), v=_at(4 + 4 * k), words=words, grad_scale=1.0, add_first=0, add_count=0, add_value=0.0)
    f.update(kw)
    return lib.AtcAdamTensor(*[f[n] for n in lib.ADAM_TENSOR_FIELDS])


def test_adam_step_refusals_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    err = h.atc_last_error
    good = lib.AtcAdam(3e-4, 0.9, 0.999, 1e-5, 0.5, 1)
    stats = C.c_void_p(_at(20))

    def call(tensors, g=good, n=None, s=FAKE, st=stats):
        arr = (lib.AtcAdamTensor * max(len(tensors), 1))(*tensors)
        return h.atc_adam_step(s, len(tensors) if n is None else n, arr if tensors else None, None if g is None else C.byref(g), st, None)
    two = [_tensor(0), _tensor(1)]
    assert call(two, s=None) == -1 and b"null pointer: s" in err()
    assert call([], n=3) == -1 and b"null pointer: t" in err()
    assert call(two, g=None, n=3) == -1 and b"null pointer: g" in err()
    assert call(two, n=3, st=None) == -1 and b"null pointer: stats" in err()
    for n in (0, 3, -1):
        assert call([_tensor(0, words=0)] * 2, n=n) == -1 and b"n_tensors" in err(), n
    for name in ("w", "grad", "m", "v"):
        assert call([_tensor(0), _tensor(1, **{name: None, "words": 0})]) == -1 and b"tensor 1" in err() and b"null pointer" in err(), name
    for words in (0, -3, 65537):
        assert call([_tensor(0, words=words, add_count=-1)]) == -1 and b"words of tensor 0" in err(), words
    for first, count in ((0, -1), (-1, 1), (8, 3), (10, 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert call([_tensor(0), _tensor(1, add_first=first, add_count=count)], g=lib.AtcAdam(3e-4, 0.9, 0.999, 1e-5, 0.5, 0)) == -1 and b"window of tensor 1" in err(), (first, count)
    assert call([_tensor(0, add_first=7, add_count=3, grad_scale=INF)], g=lib.AtcAdam(3e-4, 0.9, 0.999, 1e-5, 0.5, 0)) == -1 and b"grad_scale" in err()   # (7 .. 9 is inside)
    assert call([_tensor(0, add_first=99, add_count=0, add_value=float("nan"))]) == -1 and b"add_value" in err()      # (a window of 0 words lies anywhere)
    for step in (0, -1):
        assert call(two, g=lib.AtcAdam(float("nan"), 0.9, 0.999, 1e-5, 0.5, step)) == -1 and b"step" in err()
    for lr in (float("nan"), INF, -1e-3):
        assert call(two, g=lib.AtcAdam(lr, 0.9, 0.999, -1.0, 0.5, 1)) == -1 and b"lr" in err()
    for eps in (float("nan"), INF, -1e-5):
        assert call(two, g=lib.AtcAdam(3e-4, 1.0, 0.999, eps, 0.5, 1)) == -1 and b"eps" in err()
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, float("nan")), (float("nan"), 0.5)):
        assert call(two, g=lib.AtcAdam(3e-4, b1, b2, 1e-5, float("nan"), 1)) == -1 and b"beta" in err()
    assert call(two, g=lib.AtcAdam(3e-4, 0.9, 0.999, 1e-5, float("nan"), 1)) == -1 and b"max_norm" in err()
    # every pair of the nine arrays, at both ends of the ranges
    names = [(k, n) for k in (0, 1) for n in ("w", "grad", "m", "v")]
    n = 0
    for j, (kb, b) in enumerate(names):
        for ka, a in names[:j]:
            for off in (0, 39, -39):
                t = [dict(), dict()]
                t[kb][b] = getattr(two[ka], a) + off
                assert call([_tensor(0, **t[0]), _tensor(1, **t[1])]) == -1 and b"overlaps" in err(), (ka, a, kb, b, off)
                assert b"%s of tensor %d" % (a.encode(), ka) in err() and b"%s of tensor %d" % (b.encode(), kb) in err(), err()
                n += 1
    for k, a in names:
        for off in (0, 39, -15):
            assert call(two, st=C.c_void_p(getattr(two[k], a) + off)) == -1 and b"overlaps stats" in err(), (k, a, off)
    assert n == 28 * 3
    assert _records() == before, "a refused call moved a launch record"


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatement
ADV_R = (1, 2, 255, 256, 257, 3 * 256 * 2 + 1)


def _adv_data(R, seed=0):
    rng = np.random.default_rng([41, R, seed])
    return (rng.normal(0.3, 2.0, R) * rng.choice([0.1, 1.0, 30.0], R)).astype(np.float32)


@pytest.mark.parametrize("G", (0, 1, 3))
@pytest.mark.parametrize("R", ADV_R)
def test_adv_restatement_equals_numpy_moments(R, G):
    a = _adv_data(R)
    rng = np.random.default_rng([42, R])
    for mask in (None, (rng.random(R) < 0.6).astype(np.uint8)):
        if mask is not None and R > 2:
            mask[:2] = 1
        ref = U.adv_normalise(a, mask, 1e-8, G)
        sel = a.astype(np.float64) if mask is None else a.astype(np.float64)[mask != 0]
        assert ref["n"] == sel.size == ref["stats"][U.STAT_N]
        if sel.size == 0:
            assert not ref["stats"].any() and not ref["adv"].any()
            continue
        assert abs(ref["mean"] - sel.mean()) <= 1e-12 * abs(sel.mean())
        if sel.size > 1:
            assert abs(ref["std"] - sel.std(ddof=1)) <= 1e-12 * sel.std(ddof=1)
            z = ((sel - sel.mean()) / (sel.std(ddof=1) + 1e-8))
            got = ref["adv"].astype(np.float64) if mask is None else ref["adv"].astype(np.float64)[mask != 0]
            assert np.max(np.abs(got - z)) <= 4e-7 * np.max(np.abs(z)) + 4e-7 * abs(sel.mean()) / sel.std(ddof=1)      # (float32: the shift, the difference, the product)
        if mask is not None:
            assert not ref["adv"][mask == 0].any()
    assert U.adv_moments(a, None, G).shape == (U.workgroups(R, G), 3)


def test_adv_restatement_edges():
    a = _adv_data(300)
    none = U.adv_normalise(a, np.zeros(300, np.uint8), 1e-8, 2)
    assert not none["stats"].any() and not none["adv"].any() and none["adv"].dtype == np.float32 and none["stats"].dtype == np.float32
    one = np.zeros(300, np.uint8)
    one[271] = 1
    for eps in (1e-8, 2.0 ** -10):      # (1e-8 rounded to float32 still gives float32(1e8))
        ref = U.adv_normalise(a, one, eps, 0)
        assert ref["n"] == 1 and ref["std"] == 0.0 and ref["stats"][U.STAT_STD] == 0 and ref["stats"][U.STAT_MEAN] == a[271]
        assert ref["stats"][U.STAT_SCALE] == np.float32(1.0 / eps) and not ref["adv"].any()      # (its own advantage is the mean)
    lone = U.adv_normalise(a[:1], None, 1e-8, 0)
    assert lone["stats"].tolist() == [1.0, float(a[0]), float(np.float32(1e8)), 0.0] and lone["adv"].tolist() == [0.0]
    dirty = a.copy()
    dirty[one == 0] = np.nan
    assert _same(U.adv_normalise(dirty, one, 1e-8, 0)["adv"], U.adv_normalise(a, one, 1e-8, 0)["adv"])
    # another G is another order of the same sums; the shape is kept
    assert np.allclose(U.adv_normalise(a, None, 1e-8, 1)["adv"], U.adv_normalise(a, None, 1e-8, 2)["adv"], rtol=1e-6, atol=1e-6)
    assert U.adv_normalise(a.reshape(3, 50, 2), None, 1e-8, 0)["adv"].shape == (3, 50, 2)


WORDS2 = (L.POLICY_WORDS, L.VALUE_WORDS)
ADAM = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_norm=1000.0)      # a bound between the two gains' norms (about 80 and 8e4)
ENT, VF = 0.01, 0.5


@functools.lru_cache(maxsize=None)
def _adam_inputs(words=WORDS2, steps=6, seed=0):
    """(initial tensors, the gradients of each step): gains 1 and 1e3 in turn, so that the clip engages on every second step"""
    rng = np.random.default_rng([43, seed] + list(words))
    t0 = [dict(w=rng.normal(0, 0.3, n).astype(np.float32), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32)) for n in words]
    grads = [[(rng.normal(0, 1, n) * (1.0 if s % 2 == 0 else 1e3)).astype(np.float32) for n in words] for s in range(steps)]
    return t0, grads


def _extras(k, words):
    """the policy carries the entropy window on its last three words, the critic the value coefficient"""
    if k == 0:
        return dict(add=(words - 3, 3, -ENT)) if words >= 3 else {}
    return dict(grad_scale=VF)


def _run_ref(words=WORDS2, steps=6, store=np.float32, seed=0, **kw):
    """the restatement over `steps` steps: [(tensors after the step, stats)]"""
    t0, grads = _adam_inputs(words, steps, seed)
    cur = [dict(t, **_extras(k, words[k])) for k, t in enumerate(t0)]
    if store is np.float64:
        cur = [dict(t, w=t["w"].astype(np.float64), m=t["m"].astype(np.float64), v=t["v"].astype(np.float64)) for t in cur]
    out = []
    for s in range(steps):
        cur = [dict(t, grad=grads[s][k]) for k, t in enumerate(cur)]
        cur, stats = U.adam_step(cur, step=s + 1, store=store, **dict(ADAM, **kw))
        out.append((cur, stats))
    return out


def test_adam_restatement_equals_torch_adam_in_float64():
    import torch
    t0, grads = _adam_inputs()
    params = [torch.tensor(t["w"].astype(np.float64), requires_grad=True) for t in t0]
    opt = torch.optim.Adam(params, lr=ADAM["lr"], betas=(ADAM["beta1"], ADAM["beta2"]), eps=ADAM["eps"])
    ref32, ref64 = _run_ref(), _run_ref(store=np.float64)
    clipped = []
    for s in range(6):
        for k, p in enumerate(params):
            g = torch.tensor(grads[s][k].astype(np.float64))
            if k == 0:
                g[-3:] += np.float64(np.float32(-ENT))
            else:
                g = g * VF
            p.grad = g
        norm = float(torch.nn.utils.clip_grad_norm_(params, ADAM["max_norm"]))
        opt.step()
        clipped.append(norm > ADAM["max_norm"])
        for k, p in enumerate(params):
            w = p.detach().numpy()
            top = np.max(np.abs(w))
            d64, d32 = np.max(np.abs(ref64[s][0][k]["w"] - w)) / top, np.max(np.abs(ref32[s][0][k]["w"].astype(np.float64) - w)) / top
            assert d64 <= 1e-12 and d32 <= 1e-6, (s, k, d64, d32)
            assert ref32[s][0][k]["w"].dtype == np.float32 and ref64[s][0][k]["w"].dtype == np.float64
        for ref in (ref32, ref64):
            assert abs(float(ref[s][1][U.ASTAT_NORM]) - norm) <= 1e-6 * norm and ref[s][1][U.ASTAT_SKIPPED] == 0 and ref[s][1][U.ASTAT_STEP] == s + 1
            assert (ref[s][1][U.ASTAT_COEF] < 1.0) == clipped[-1]
    assert clipped == [False, True] * 3      # the clip engages on some steps and not on others
    assert np.max(np.abs(ref32[5][0][0]["w"] - t0[0]["w"])) > 1e-4      # ... and the weights moved


def test_adam_restatement_window_and_nan_skip():
    t0, grads = _adam_inputs()
    base = [dict(t, grad=grads[0][k]) for k, t in enumerate(t0)]
    plain = np.concatenate([U.effective_grad(t) for t in base])
    with_window = np.concatenate([U.effective_grad(dict(t, **_extras(k, WORDS2[k]))) for k, t in enumerate(base)])
    moved = np.flatnonzero(plain != with_window)
    assert set(range(LOG_STD, LOG_STD + 3)) <= set(moved.tolist()) and np.all(with_window[LOG_STD:LOG_STD + 3] - plain[LOG_STD:LOG_STD + 3] == np.float64(np.float32(-ENT)))
    assert np.all(moved[3:] >= L.POLICY_WORDS) and np.all(with_window[L.POLICY_WORDS:] == VF * plain[L.POLICY_WORDS:])      # the rest of what moved is the critic's scale
    only = np.concatenate([U.effective_grad(dict(base[0], add=(LOG_STD, 3, -ENT))), U.effective_grad(base[1])])
    assert np.flatnonzero(only != plain).tolist() == [LOG_STD, LOG_STD + 1, LOG_STD + 2]
    for bad in (np.nan, np.inf, -np.inf):
        g = grads[0][1].copy()
        g[17] = bad
        held = [dict(t, grad=(g if k else grads[0][0])) for k, t in enumerate(t0)]
        new, stats = U.adam_step(held, step=1, **ADAM)
        assert stats[U.ASTAT_SKIPPED] == 1 and stats[U.ASTAT_COEF] == 0 and not np.isfinite(stats[U.ASTAT_NORM])
        for k in (0, 1):
            for n in ("w", "m", "v"):
                assert _same(new[k][n], t0[k][n]), (bad, k, n)
    # without a bound the coefficient is 1 whatever the norm
    for off in (0.0, -1.0, INF):
        assert _run_ref(steps=2, max_norm=off)[1][1][U.ASTAT_COEF] == 1.0


# ---------------------------------------------------------------------------------------------------------------- GPU
CFG = dict(normalize=True, shaping=True, auto_reset=True, timestep_limit=7, spawn="lattice")


@functools.lru_cache(maxsize=None)
def _env():
    return H.policy_env(CFG, 8, 4)


def _t(env, a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a), device=env.device)
    return t if dtype is None else t.to(dtype)


ADV_GPU_R = (1, 2, 255, 256, 257, 1537)
ADV_KINDS = ("plain", "mask", "none", "one", "nan", "inplace", "stats-only")


def _adv_case(R, kind):
    a = _adv_data(R, 1)
    rng = np.random.default_rng([44, R])
    mask = None
    if kind in ("mask", "nan", "inplace"):
        mask = (rng.random(R) < 0.6).astype(np.uint8)
        mask[0] = 1
        if R > 1:
            mask[R - 1] = 0
    elif kind == "none":
        mask = np.zeros(R, np.uint8)
    elif kind == "one":
        mask = np.zeros(R, np.uint8)
        mask[R // 2] = 1
    if kind == "nan":
        a = a.copy()
        a[mask == 0] = np.nan
    return a, mask


@pytest.mark.gpu
@pytest.mark.parametrize("G", (0, 1, 3))
@pytest.mark.parametrize("R", ADV_GPU_R)
def test_adv_normalise_equals_the_restatement_bit_for_bit(R, G):
    import torch
    from atc_hip import lib
    env = _env()
    worst = 0.0
    for kind in ADV_KINDS:
        a, mask = _adv_case(R, kind)
        ref = U.adv_normalise(a, mask, 1e-8, G)
        ad, md = _t(env, a), None if mask is None else _t(env, mask)
        before = _records()
        stats = torch.full((5,), SENTINEL, device=env.device)
        scratch = torch.empty((L.adv_workgroups(R, G), 3), dtype=torch.float64, device=env.device)
        if kind == "inplace":
            res = env.adv_normalise(ad, md, workgroups=G, out={"adv": ad, "stats": stats[:4], "scratch": scratch})
            assert res["adv"] is ad and "scratch" not in res
        elif kind == "stats-only":      # out_adv omitted: the entry point through ctypes with a NULL
            g, o = lib.AtcAdvNorm(1e-8, G), lib.AtcAdvNormOut(None, stats.data_ptr(), scratch.data_ptr())
            with torch.cuda.device(env.device):
                assert env._lib.atc_adv_normalise(env.sector.handle, R, ad.data_ptr(), None, C.byref(g), C.byref(o), env._stream()) == 0
            res = {"stats": stats[:4]}
        else:
            res = env.adv_normalise(ad, md, workgroups=G, out={"stats": stats[:4], "scratch": scratch})
            assert res["adv"].data_ptr() != ad.data_ptr() and res["adv"].shape == ad.shape
        env.synchronize()
        assert _moved(before, _records()) == {"atc_adv_normalise_launch_counts": {"adv_normalise": 1}}
        got = {k: v.cpu().numpy() for k, v in res.items()}
        assert _same(got["stats"], ref["stats"]), (kind, got["stats"], ref["stats"])
        assert float(stats[4]) == SENTINEL and _same(scratch.cpu().numpy(), ref["scratch"])
        if "adv" in got:
            assert _same(got["adv"], ref["adv"]), (kind, np.flatnonzero(got["adv"] != ref["adv"])[:5])
            if mask is not None:
                assert not got["adv"][mask == 0].any()
        if kind in ("none",):
            assert not got["stats"].any() and not got["adv"].any()
        if kind == "one":
            assert got["stats"].tolist() == [1.0, float(a[R // 2]), 1e8, 0.0]
        # the statistics against the float64 values: the bar is 4 x the deviation of torch's own float32 reductions on the same data
        sel = a.astype(np.float64) if mask is None else a.astype(np.float64)[mask != 0]
        if sel.size >= 2:
            t32 = torch.as_tensor(a if mask is None else a[mask != 0], device=env.device)
            want = {U.STAT_MEAN: sel.mean(), U.STAT_STD: sel.std(ddof=1), U.STAT_SCALE: 1.0 / (sel.std(ddof=1) + np.float64(np.float32(1e-8)))}
            theirs = {U.STAT_MEAN: float(t32.mean()), U.STAT_STD: float(t32.std()), U.STAT_SCALE: float(1.0 / (t32.std() + 1e-8))}
            for q, name in ((U.STAT_MEAN, "mean"), (U.STAT_SCALE, "scale"), (U.STAT_STD, "std")):
                dev, bar = abs(float(got["stats"][q]) - want[q]), 4.0 * abs(theirs[q] - want[q])
                print("R %d G %d %s: %s deviation %.3e, bar %.3e (4 x torch float32's %.3e)" % (R, G, kind, name, dev, bar, bar / 4))
                assert dev <= bar, (kind, name, dev, bar)
                worst = max(worst, dev / bar if bar > 0 else 0.0)
    print("R %d G %d: largest deviation / bar %.3f" % (R, G, worst))
    # without out=: fresh tensors, the same bits; any shape
    a, mask = _adv_case(R, "mask")
    free = env.adv_normalise(_t(env, a).reshape(1, R, 1), _t(env, mask), workgroups=G)
    env.synchronize()
    ref = U.adv_normalise(a, mask, 1e-8, G)
    assert tuple(free["adv"].shape) == (1, R, 1) and _same(free["adv"].cpu().numpy().reshape(-1), ref["adv"]) and _same(free["stats"].cpu().numpy(), ref["stats"])


@pytest.mark.gpu
def test_adv_normalise_with_all_buffers_allocates_nothing_and_refuses_overlap():
    import torch
    env = _env()
    a, mask = _adv_case(1537, "mask")
    ad, md = _t(env, a), _t(env, mask)
    out = {"adv": torch.empty_like(ad), "stats": torch.empty(4, device=env.device), "scratch": torch.empty((3, 3), dtype=torch.float64, device=env.device)}
    env.adv_normalise(ad, md, workgroups=3, out=out)
    env.synchronize()
    torch.cuda.reset_peak_memory_stats(env.device)
    held = torch.cuda.memory_allocated(env.device)
    first = {k: v.clone() for k, v in out.items()}
    held2 = torch.cuda.memory_allocated(env.device)
    torch.cuda.reset_peak_memory_stats(env.device)
    env.adv_normalise(ad, md, workgroups=3, out=out)
    env.synchronize()
    assert held2 > held and torch.cuda.memory_allocated(env.device) == held2 == torch.cuda.max_memory_allocated(env.device)
    for k in out:      # the same inputs and the same G: the same bits
        assert torch.equal(out[k].view(torch.int32), first[k].view(torch.int32)), k
    before = _records()
    big = torch.zeros(1537 + 8, device=env.device)
    with pytest.raises(RuntimeError, match="adv overlaps out_adv"):
        env.adv_normalise(big[:1537], md, out={"adv": big[1:1538]})
    with pytest.raises(RuntimeError, match="out_adv overlaps stats"):
        env.adv_normalise(ad, md, out={"adv": big[:1537], "stats": big[1536:1540]})
    with pytest.raises(ValueError, match=r"out\['scratch'\]"):
        env.adv_normalise(ad, md, workgroups=3, out={"scratch": torch.empty((2, 3), dtype=torch.float64, device=env.device)})
    with pytest.raises(ValueError, match=r"out\['scratch'\]"):
        env.adv_normalise(ad, md, workgroups=3, out={"scratch": torch.empty((3, 3), device=env.device)})
    with pytest.raises(ValueError, match="mask"):
        env.adv_normalise(ad, md[:-1].contiguous())
    with pytest.raises(ValueError, match="adv"):
        env.adv_normalise(ad.double())
    env.synchronize()
    assert _records() == before


@functools.lru_cache(maxsize=None)
def _collection():
    """one small collect_bootstrap result (B = 8, N = 4, T = 16, hold 2) with the policy and the critic it was made with"""
    import torch
    from atc_hip import ppo
    env = _env()
    w = _t(env, P.random_weights(np.random.default_rng([45, 0]), 1.0, (-0.5, -1.0, 0.25), False, 0))
    vw = _t(env, PV.random_weights(np.random.default_rng([45, 1]), 1.0, 0))
    res = ppo.collect_bootstrap(env, w, ppo.critic(env, vw), 16, hold=2, seed=5, decision0=3)
    res = dict(res, obs0=env._collected_obs0[1])      # (kept with the dict: other tests collect on the same env)
    env.synchronize()
    assert tuple(res["adv"].shape) == (8, 8, 4) and 0 < int(res["control"].sum()) and bool(torch.isfinite(res["adv"]).all())
    return env, res, w, vw


@pytest.mark.gpu
def test_policy_grad_on_normalised_advantages_equals_shift_and_scale():
    from atc_hip import ppo
    env, res, w, vw = _collection()
    normed = env.adv_normalise(res["adv"], res["control"])
    env.synchronize()
    stats = normed["stats"].cpu().numpy()      # (read back for this test only)
    assert stats[0] == float(res["control"].sum()) and stats[3] > 0
    a = ppo.policy_grad(env, dict(res, adv=normed["adv"]), w, normalise=False)
    own = ppo.value_rows(env, res, res["obs0"], hold=2)[:-1]
    b = env.ppo_policy_grad(w, own, res["action"], res["logp"], res["adv"], mask=res["control"], adv_shift=float(stats[1]), adv_scale=float(stats[2]))
    env.synchronize()
    for k in ("grad", "stats", "logp"):
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert x.view(np.int32).tolist() == y.view(np.int32).tolist(), k
    assert float(a["grad"].abs().max()) > 0 and float(a["stats"][0]) == stats[0]
    # ... and ppo.policy_grad's own normalisation (three torch reductions) is the same shift and scale within float32
    c = ppo.policy_grad(env, res, w)
    env.synchronize()
    assert float((c["grad"] - a["grad"]).abs().max()) <= 1e-4 * float(a["grad"].abs().max())


ADAM_GPU = (("two", WORDS2, {}), ("two-no-clip", WORDS2, dict(max_norm=0.0)), ("two-inf", WORDS2, dict(max_norm=INF)), ("one-1", (1,), {}), ("one-1023", (1023,), {}),
            ("one-1024", (1024,), {}), ("one-1025", (1025,), dict(max_norm=-1.0)), ("one-policy", (L.POLICY_WORDS,), {}))


@pytest.mark.gpu
@pytest.mark.parametrize("name,words,kw", ADAM_GPU, ids=[c[0] for c in ADAM_GPU])
def test_adam_step_equals_the_restatement_bit_for_bit(name, words, kw):
    import torch
    env = _env()
    t0, grads = _adam_inputs(words, 6, 0)
    ref = _run_ref(words, 6, np.float32, 0, **kw)
    dev = [{n: _t(env, t[n]) for n in ("w", "m", "v")} for t in t0]
    for k, d in enumerate(dev):
        d["grad"] = torch.empty(words[k], device=env.device)
        x = _extras(k, words[k])
        if "add" in x:
            d["add"] = x["add"]
        if "grad_scale" in x:
            d["grad_scale"] = x["grad_scale"]
    stats = torch.full((5,), SENTINEL, device=env.device)
    for s in range(6):
        for k, d in enumerate(dev):
            d["grad"].copy_(_t(env, grads[s][k]))
        before = _records()
        held = torch.cuda.memory_allocated(env.device)
        got = env.adam_step(dev, step=s + 1, out=stats[:4], **dict(ADAM, **kw))
        env.synchronize()
        assert got.data_ptr() == stats.data_ptr()
        if s:      # (the first call lets go of the tensors the env kept alive for the call before it)
            assert torch.cuda.memory_allocated(env.device) == held
        assert _moved(before, _records()) == {"atc_adam_step_launch_counts": {len(words): 1}}
        for k, d in enumerate(dev):
            for n in ("w", "m", "v"):
                x, y = d[n].cpu().numpy(), ref[s][0][k][n]
                assert _same(x, y), (name, s, k, n, int((x != y).sum()), np.flatnonzero(x != y)[:4])
            assert _same(d["grad"].cpu().numpy(), grads[s][k])
        st, want = got.cpu().numpy(), ref[s][1]
        for q in (U.ASTAT_NORM, U.ASTAT_COEF):
            assert abs(float(st[q]) - float(want[q])) <= float(np.spacing(np.abs(want[q]))), (name, s, q, st, want)      # within 1 ulp of the restatement's float32
        assert st[U.ASTAT_SKIPPED] == 0 and st[U.ASTAT_STEP] == s + 1 and float(stats[4]) == SENTINEL
        if len(words) == 2 and not kw:
            assert (st[U.ASTAT_COEF] < 1.0) == (s % 2 == 1)
    if kw:
        assert all(r[1][U.ASTAT_COEF] == 1.0 for r in ref)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", (float("nan"), INF))
def test_adam_step_skips_a_gradient_that_is_not_finite(bad):
    env = _env()
    t0, grads = _adam_inputs(WORDS2, 6, 0)
    after = _run_ref(steps=1)[0][0]      # one good step first, so that m and v hold something
    g = [grads[1][0].copy(), grads[1][1].copy()]
    g[1][4000] = bad
    dev = [dict({n: _t(env, after[k][n]) for n in ("w", "m", "v")}, grad=_t(env, g[k]), **_extras(k, WORDS2[k])) for k in (0, 1)]
    got = env.adam_step(dev, step=2, **ADAM)
    env.synchronize()
    st = got.cpu().numpy()
    _, want = U.adam_step([dict(after[k], grad=g[k]) for k in (0, 1)], step=2, **ADAM)
    assert st[U.ASTAT_SKIPPED] == 1 and st[U.ASTAT_COEF] == 0 and st[U.ASTAT_STEP] == 2 and np.array_equal(st, want, equal_nan=True)
    for k in (0, 1):
        for n in ("w", "m", "v"):
            assert _same(dev[k][n].cpu().numpy(), after[k][n]), (k, n)


@pytest.mark.gpu
def test_adam_step_refusals_launch_nothing():
    import torch
    env = _env()
    z = lambda n=64: torch.zeros(n, device=env.device)      # noqa: E731
    one = dict(w=z(), grad=z(), m=z(), v=z())
    before = _records()
    with pytest.raises(RuntimeError, match="w of tensor 0 overlaps m of tensor 0"):
        env.adam_step([dict(one, m=one["w"])], lr=1e-3, step=1)
    big = z(100)
    with pytest.raises(RuntimeError, match="m of tensor 0 overlaps w of tensor 1"):
        env.adam_step([dict(one, m=big[:64]), dict(one, w=big[36:], grad=z(), v=z(), m=z())], lr=1e-3, step=1)
    with pytest.raises(ValueError, match="step"):
        env.adam_step([one], lr=1e-3, step=0)
    with pytest.raises(ValueError, match="1 or 2"):
        env.adam_step([one, dict(w=z(), grad=z(), m=z(), v=z()), dict(w=z(), grad=z(), m=z(), v=z())], lr=1e-3, step=1)
    for add in ((62, 3, -0.01), (-1, 1, -0.01), (64, 1, 0.5)):
        with pytest.raises(ValueError, match="inside the tensor"):
            env.adam_step([dict(one, add=add)], lr=1e-3, step=1)
    # ... and the library's own refusals of the same, through ctypes
    from atc_hip import lib
    t = (lib.AtcAdamTensor * 3)(*[lib.AtcAdamTensor(*[z().data_ptr() for _ in range(4)], 64, 1.0, 0, 0, 0.0) for _ in range(3)])
    st = z(4)
    call = lambda n, g: env._lib.atc_adam_step(env.sector.handle, n, t, C.byref(g), st.data_ptr(), env._stream())      # noqa: E731
    err = env._lib.atc_last_error
    assert call(3, lib.AtcAdam(1e-3, 0.9, 0.999, 1e-5, 0.5, 1)) == -1 and b"n_tensors" in err()
    assert call(2, lib.AtcAdam(1e-3, 0.9, 0.999, 1e-5, 0.5, 0)) == -1 and b"step" in err()
    t[1].add_first, t[1].add_count = 62, 3
    assert call(2, lib.AtcAdam(1e-3, 0.9, 0.999, 1e-5, 0.5, 1)) == -1 and b"window of tensor 1" in err()
    with pytest.raises(ValueError, match=r"tensors\[0\]\['m'\]"):
        env.adam_step([dict(one, m=z(63))], lr=1e-3, step=1)
    with pytest.raises(ValueError, match="beta"):
        env.adam_step([one], lr=1e-3, step=1, beta1=1.0)
    env.synchronize()
    assert _records() == before and not any(float(v.abs().max()) for v in one.values())


def _clone_state(env, w, vw):
    from atc_hip import ppo
    w2, vw2 = w.clone(), vw.clone()
    return w2, vw2, ppo.adam_state(env, w2, vw2)


UPDATE = dict(clip=0.2, vclip=0.3, lr=1e-3, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, eps=1e-5)


@pytest.mark.gpu
def test_update_equals_the_same_calls_issued_by_hand():
    import torch
    from atc_hip import ppo
    env, res, w, vw = _collection()
    R, E, M = 8 * 8 * 4, 2, 2
    gen = torch.Generator().manual_seed(9)
    perm = torch.stack([torch.randperm(R, generator=gen) for _ in range(E)]).to(torch.int32).to(env.device)
    w1, vw1, state = _clone_state(env, w, vw)
    assert state["t"] == 0 and not any(float(t.abs().max()) for t in state["m"] + state["v"])
    before = _records()
    got = ppo.update(env, res, w1, vw1, state, epochs=E, minibatches=M, perm=perm, **UPDATE)
    env.synchronize()
    moved = _moved(before, _records())
    assert moved == {"atc_adv_normalise_launch_counts": {"adv_normalise": 1}, "atc_ppo_policy_grad_launch_counts": {0: E * M},
                     "atc_ppo_value_grad_launch_counts": {0: E * M}, "atc_adam_step_launch_counts": {2: E * M}}, moved
    assert sum(sum(d.values()) for d in moved.values()) == 1 + E * M * (1 + 1 + 1)
    assert state["t"] == E * M
    assert {k: tuple(v.shape) for k, v in got.items()} == {"policy_stats": (E, M, 8), "value_stats": (E, M, 8), "adam_stats": (E, M, 4), "adv_stats": (4,)}
    # by hand
    w2, vw2 = w.clone(), vw.clone()
    m = [torch.zeros_like(w2), torch.zeros_like(vw2)]
    v = [torch.zeros_like(w2), torch.zeros_like(vw2)]
    normed = env.adv_normalise(res["adv"], res["control"])
    mb = dict(res, adv=normed["adv"])
    step = 0
    for e in range(E):
        for k in range(M):
            index = perm[e][k * R // M:(k + 1) * R // M].contiguous()
            pg = ppo.policy_grad(env, mb, w2, index=index, clip=UPDATE["clip"], normalise=False)
            vg = ppo.value_grad(env, res, vw2, index=index, clip=UPDATE["vclip"])
            step += 1
            st = env.adam_step([dict(w=w2, grad=pg["grad"], m=m[0], v=v[0], add=(LOG_STD, 3, -UPDATE["ent_coef"])),
                                dict(w=vw2, grad=vg["grad"], m=m[1], v=v[1], grad_scale=UPDATE["vf_coef"])],
                               lr=UPDATE["lr"], step=step, eps=UPDATE["eps"], max_norm=UPDATE["max_grad_norm"])
            env.synchronize()
            for name, mine, theirs in (("policy_stats", got["policy_stats"][e, k], pg["stats"]), ("value_stats", got["value_stats"][e, k], vg["stats"]),
                                       ("adam_stats", got["adam_stats"][e, k], st)):
                assert torch.equal(mine.contiguous().view(torch.int32), theirs.view(torch.int32)), (name, e, k)
            assert float(st[L.ADAM_STAT_SKIPPED]) == 0 and float(st[L.ADAM_STAT_STEP]) == step
    bits = lambda t: t.view(torch.int32)      # noqa: E731
    assert torch.equal(bits(got["adv_stats"]), bits(normed["stats"]))
    for name, mine, theirs in (("w", w1, w2), ("vw", vw1, vw2), ("m0", state["m"][0], m[0]), ("m1", state["m"][1], m[1]), ("v0", state["v"][0], v[0]), ("v1", state["v"][1], v[1])):
        assert torch.equal(bits(mine), bits(theirs)), name
    assert not torch.equal(w1, w) and not torch.equal(vw1, vw)
    assert float(got["policy_stats"][0, 0, L.PPO_STAT_N]) + float(got["policy_stats"][0, 1, L.PPO_STAT_N]) == float(got["adv_stats"][0])
    # the log_std words moved by the entropy term too: without it another result
    w3, vw3, state3 = _clone_state(env, w, vw)
    ppo.update(env, res, w3, vw3, state3, epochs=E, minibatches=M, perm=perm, **dict(UPDATE, ent_coef=0.0))
    env.synchronize()
    assert not torch.equal(w3[LOG_STD:], w1[LOG_STD:])


@pytest.mark.gpu
def test_update_draws_its_permutations_from_the_seed():
    import torch
    from atc_hip import ppo
    env, res, w, vw = _collection()
    runs = []
    for seed in (3, 3, 4):
        w1, vw1, state = _clone_state(env, w, vw)
        got = ppo.update(env, res, w1, vw1, state, epochs=2, minibatches=2, seed=seed, **UPDATE)
        env.synchronize()
        runs.append((w1, vw1, got))
    bits = lambda t: t.contiguous().view(torch.int32)      # noqa: E731
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(bits(runs[0][1]), bits(runs[1][1]))
    for k in runs[0][2]:
        assert torch.equal(bits(runs[0][2][k]), bits(runs[1][2][k])), k
    assert not torch.equal(runs[0][0], runs[2][0]) and not torch.equal(runs[0][2]["policy_stats"], runs[2][2]["policy_stats"])
    # a second update goes on counting, and makes no buffer of its own
    w1, vw1, state = _clone_state(env, w, vw)
    ppo.update(env, res, w1, vw1, state, epochs=1, minibatches=2, seed=1, **UPDATE)
    kept = (set(state["rows"]), set(state["adv"]))
    got = ppo.update(env, res, w1, vw1, state, epochs=1, minibatches=2, seed=2, **UPDATE)
    env.synchronize()
    assert state["t"] == 4 and got["adam_stats"][0, :, L.ADAM_STAT_STEP].tolist() == [3.0, 4.0] and (set(state["rows"]), set(state["adv"])) == kept


@pytest.mark.gpu
def test_update_only_enqueues():
    """after one warm-up call, update() with every synchronising call of torch's turned into an error"""
    import torch
    from atc_hip import ppo
    env, res, w, vw = _collection()
    w1, vw1, state = _clone_state(env, w, vw)
    perm = torch.stack([torch.randperm(256) for _ in range(2)]).to(torch.int32).to(env.device)
    ppo.update(env, res, w1, vw1, state, epochs=2, minibatches=2, seed=1, **UPDATE)
    env.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError):      # the mode is live in this build: a host read is refused
            float(w1[0])
        ppo.update(env, res, w1, vw1, state, epochs=2, minibatches=2, seed=2, **UPDATE)
        ppo.update(env, res, w1, vw1, state, epochs=2, minibatches=2, perm=perm, **UPDATE)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    env.synchronize()
    assert state["t"] == 12 and bool(torch.isfinite(w1).all())
