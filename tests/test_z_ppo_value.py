"""The critic in the library (include/atc_step.h: atc_value_forward, atc_ppo_value_grad; AtcVecEnv.value_forward, AtcVecEnv.ppo_value_grad;
atc_hip/value.py; atc_hip/ppo.py: critic, value_grad): V of R rows in one launch, and the clipped PPO value loss with its gradient with
respect to the packed critic in one call, no activation written to memory.

CPU: the exports and one kernel symbol per K for both kernels; constants, structs and argtypes across the header, atc_hip/layout.py and
atc_hip/lib.py; the refusal order of both entry points through ctypes with NULL and made-up pointers; the launch records; the Python surface
and its refusals before any library call; atc_hip.value's offsets / pack_mlp / from_torch against an nn.Sequential; tests/ppo_value_ref.py
(the float64 restatement) against torch.autograd in float64 with the loss written as 0.5 * torch.maximum((v - ret)^2, (vc - ret)^2), for
every K, with and without mask and index, for clip 0.2 and inf, within 1e-10 of each part's largest word; what the GPU cases contain: every
finite-clip case has a row inside the clip range, one outside whose gradient flows and one that is cut, none within 1e-4 of |delta| = clip
and none outside with |e^2 - ec^2| < 1e-4 max(e^2, ec^2).  (The R = 1 case cannot hold three kinds of row: it is the clip = inf case.)
GPU: value_forward against the float64 restatement within 4 x the float32 twin's own deviation (floor 1e-6 x the largest |V|); every part of
grad, the five means of stats and value within the twin bars, n and the cut count exact, max |v - v_old| within value's bar — the measured
deviation / bar is printed before it is asserted —; value bit for bit value_forward's output on the rows the tiles hold; two runs bit for
bit; G = 1 against G = 3; NaNs in the rows that take no part; a mask of zeros; the value sentinel; clip = inf; out= without an allocation;
the refusals that need a device; end to end behind collect_bootstrap / collect(traffic=2) with ppo.critic and the SAME weights.

Measured on an MI355X, largest kernel deviation / bar over the cases below: W1 0.43, b1 0.46, W2 0.32, b2 0.40, W3 0.28, b3 0.83, the five means
0.26, value 0.32, max |v - v_old| 0.29, value_forward 0.26, the collection's values and boot 0.29."""
import ctypes as C
import functools
import inspect
import re
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import policy_ref as P
import ppo_value_ref as PV
from atc_hip import layout as L
from held_tools import HEADER, LIB, struct_fields

NAMES = ("atc_value_forward", "atc_value_forward_launch_counts", "atc_ppo_value_grad", "atc_ppo_value_grad_launch_counts")
RECORDS = ("atc_value_forward_launch_counts", "atc_ppo_value_grad_launch_counts")
FAKE = C.c_void_p(0x100000)
KS = (0, 1, 2, 4)
INF = float("inf")
SENTINEL = -12345.5
PTRS = ("s", "w", "obs_rows", "v_old", "ret", "g", "out")      # the pointers that may not be NULL, in the order they are looked at


def _same(a, b):
    """two arrays equal bit for bit"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _records():
    from atc_hip import lib
    return lib.launch_records()


# ---------------------------------------------------------------------------------------------------------------- CPU: the ABI
def test_exports_and_one_kernel_symbol_per_k():
    from atc_hip import lib
    assert set(NAMES) <= set(lib.EXPORTS)
    h = lib.load()
    for name in NAMES:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    for K in KS:
        assert len(re.findall(r"\bvoid k_value_forward<%d>\(" % K, text)) == 1, K
        assert len(re.findall(r"\bvoid k_ppo_value_grad<%d>\(" % K, text)) == 1, K
    assert len(re.findall(r"\bk_ppo_value_grad_reduce\(", text)) == 1
    blob = open(LIB, "rb").read()
    for K in KS:      # ... and in the embedded code object
        assert blob.count(b"_Z15k_value_forwardILi%dEEviPKfS1_Pf\0" % K) >= 1, K
        assert blob.count(b"_Z16k_ppo_value_gradILi%dEEviiPKfS1_S1_S1_S1_PKhPKifPfS6_\0" % K) >= 1, K
    assert blob.count(b"_Z23k_ppo_value_grad_reduceiiPKfPfS1_\0") >= 1


def _decl(text, name):
    decl = re.search(r"^int %s\((.*?)\);" % name, text, flags=re.S | re.M).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return [" ".join(a.split()) for a in decl.split(",")]


def test_header_constants_structs_and_argtypes():
    from atc_hip import lib, value
    text = open(HEADER).read()
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, text).group(1))      # noqa: E731
    assert re.search(r"#define ATC_VALUE_WORDS\(K\) \(4289 \+ 64 \* ATC_POLICY_TRAFFIC_IN\(K\)\)", text)
    assert [L.value_words(K) for K in KS] == [PV.words(K) for K in KS] == [4929, 5377, 5825, 6721] and L.VALUE_WORDS == 4929
    assert [L.value_words(K) for K in KS] == [L.policy_words(K) - 2 * 64 - 2 - 3 for K in KS]      # the policy without two head rows and log_std
    assert L.PPO_VALUE_STATS == define("ATC_PPO_VALUE_STATS") == PV.STATS == 8
    stat = ("N", "LOSS", "CUT", "V", "RET", "RET2", "ERR2", "DV_MAX")
    assert [define("ATC_PPO_VSTAT_" + n) for n in stat] == [getattr(L, "PPO_VSTAT_" + n) for n in stat] == list(range(8))
    assert (PV.STAT_N, PV.STAT_LOSS, PV.STAT_CUT, PV.STAT_V, PV.STAT_RET, PV.STAT_RET2, PV.STAT_ERR2, PV.STAT_DV_MAX) == tuple(range(8))
    assert L.VALUE_FORWARD_LAUNCH_SLOTS == int(re.search(r"ATC_VALUE_FORWARD_LAUNCH_SLOTS = (\d+)", text).group(1)) == 4
    assert L.PPO_VALUE_GRAD_LAUNCH_SLOTS == int(re.search(r"ATC_PPO_VALUE_GRAD_LAUNCH_SLOTS = (\d+)", text).group(1)) == 4
    assert L.ABI_VERSION == 22 and define("ATC_ABI_VERSION") == 22 and L.LAUNCH_SLOTS == 57      # new entry points: the ABI number stays
    g = struct_fields(text, "atc_ppo_value_grad")
    assert [f[1] for f in g] == list(lib.PPO_VALUE_GRAD_FIELDS) == [f[0] for f in lib.AtcPpoValueGrad._fields_] == ["clip", "workgroups"]
    assert [{"float": C.c_float, "int32_t": C.c_int32}[f[0]] for f in g] == [f[1] for f in lib.AtcPpoValueGrad._fields_] and C.sizeof(lib.AtcPpoValueGrad) == 8
    o = struct_fields(text, "atc_ppo_value_grad_out")
    assert [f[1].lstrip("*") for f in o] == list(lib.PPO_VALUE_GRAD_OUT_FIELDS) == [f[0] for f in lib.AtcPpoValueGradOut._fields_]
    assert all(f[1].startswith("*") and f[0] == "float" for f in o) and C.sizeof(lib.AtcPpoValueGradOut) == 32
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    args = _decl(text, "atc_ppo_value_grad")
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "R_src", "R", "traffic_k", "w", "obs_rows", "traffic", "v_old", "ret", "mask", "index", "g", "out", "stream"]
    want = [ci if a.startswith("int ") else C.POINTER(lib.AtcPpoValueGrad) if "atc_ppo_value_grad_t" in a else
            C.POINTER(lib.AtcPpoValueGradOut) if "atc_ppo_value_grad_out_t" in a else vp for a in args]
    assert list(h.atc_ppo_value_grad.argtypes) == want
    args = _decl(text, "atc_value_forward")
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "R", "traffic_k", "w", "x", "values", "stream"]
    assert list(h.atc_value_forward.argtypes) == [ci if a.startswith("int ") else vp for a in args]
    for name in NAMES:
        assert getattr(h, name).restype is ci
    for name in RECORDS:
        assert list(getattr(h, name).argtypes) == [C.POINTER(C.c_uint64), ci]
        slots, slot_name = lib.LAUNCH_RECORDS[name]
        assert slots == 4 and [slot_name(i) for i in range(4)] == [0, 1, 2, 4]
    assert callable(lib.value_forward_launch_counts) and callable(lib.ppo_value_grad_launch_counts)
    assert [n for n, _ in value.shapes(0)] == list(PV.PART_NAMES) and [value.shapes(K) for K in KS] == [PV.shapes(K) for K in KS]
    section = text[text.index("PPO POLICY GRADIENT"):]
    assert "atc_ppo_value_grad" in section[:section.index("#define ATC_PPO_GRAD_MAX_WG")]      # what the policy call leaves out now points here


def _at(k):
    return 0x100000 + k * 0x10000000      # made-up ranges 256 MiB apart


def _call(h, R_src=1, R=1, K=0, traffic=None, mask=None, index=None, **kw):
    a = dict.fromkeys(PTRS)
    a.update(kw)
    return h.atc_ppo_value_grad(a["s"], R_src, R, K, a["w"], a["obs_rows"], traffic, a["v_old"], a["ret"], mask, index, a["g"], a["out"], None)


def test_value_grad_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    err = h.atc_last_error
    g = lib.AtcPpoValueGrad(0.2, 0)
    out = lib.AtcPpoValueGradOut(_at(10), _at(11), None, _at(12))
    ok = dict(s=FAKE, w=C.c_void_p(_at(1)), obs_rows=C.c_void_p(_at(2)), v_old=C.c_void_p(_at(3)), ret=C.c_void_p(_at(4)), g=C.byref(g), out=C.byref(out))
    # 1. the pointers in their order, with everything behind them wrong as well (K = 3, R = 0, R_src = 0)
    for j, name in enumerate(PTRS):
        named = re.compile(rb"null pointer: %s\b" % name.encode())
        assert _call(h, 0, 0, 3, **{k: ok[k] for k in PTRS[:j]}) == -1 and named.search(err()), (name, err())
        assert _call(h, 0, 0, 3, **dict(ok, **{name: None})) == -1 and named.search(err()), (name, err())
    bad = lib.AtcPpoValueGrad(float("nan"), -1)
    for o, word in ((lib.AtcPpoValueGradOut(None, None, None, None), b"out->grad"), (lib.AtcPpoValueGradOut(_at(10), None, None, None), b"out->stats"),
                    (lib.AtcPpoValueGradOut(_at(10), _at(11), None, None), b"out->scratch")):
        assert _call(h, 0, 0, 3, **dict(ok, g=C.byref(bad), out=C.byref(o))) == -1 and b"null pointer: " + word in err(), err()
    # 2. traffic_k, 3. R_src, R, index, 4. clip, 5. workgroups, 6. traffic iff K > 0: each with every later one wrong as well
    for K in (3, -1, 5, 8):
        assert _call(h, 0, 0, K, **dict(ok, g=C.byref(bad))) == -1 and b"traffic_k" in err()
    assert _call(h, 0, 5, 1, **dict(ok, g=C.byref(bad))) == -1 and b"R_src" in err()
    assert _call(h, 5, 0, 1, **dict(ok, g=C.byref(bad))) == -1 and b"R (" in err()
    assert _call(h, 5, 4, 1, **dict(ok, g=C.byref(bad))) == -1 and b"index is NULL" in err()
    assert _call(h, 5, 4, 1, index=C.c_void_p(_at(6)), **dict(ok, g=C.byref(bad))) == -1 and b"clip" in err()      # (with an index R may differ)
    for clip in (float("nan"), 0.0, -0.1, -INF):
        assert _call(h, 5, 5, 1, **dict(ok, g=C.byref(lib.AtcPpoValueGrad(clip, -1)))) == -1 and b"clip" in err(), clip
    for clip in (0.2, INF):      # +inf passes the clip check: the next refusal is the workgroups'
        for wg in (-1, 1025):
            assert _call(h, 5, 5, 1, **dict(ok, g=C.byref(lib.AtcPpoValueGrad(clip, wg)))) == -1 and b"workgroups" in err() and b"1024" in err()
    shared = C.byref(lib.AtcPpoValueGradOut(_at(10), _at(10), None, _at(10)))
    assert _call(h, 5, 5, 1, **dict(ok, g=C.byref(lib.AtcPpoValueGrad(INF, 1024)), out=shared)) == -1 and b"traffic is required" in err()
    assert _call(h, 5, 5, 0, traffic=C.c_void_p(_at(7)), **dict(ok, out=shared)) == -1 and b"traffic must be NULL" in err()
    # 7. the overlap rule, on pointer values: every output against every input and every other output; the inputs may share
    R_src, R, K, G = 9, 7, 2, 3
    words = L.value_words(K)
    size = dict(w=words * 4, obs_rows=R_src * 40, traffic=R_src * K * 32, v_old=R_src * 4, ret=R_src * 4, mask=R_src, index=R * 4,
                grad=words * 4, stats=32, value=R * 4, scratch=G * (words + 8) * 4)
    base = {n: _at(k + 1) for k, n in enumerate(size)}
    gk = lib.AtcPpoValueGrad(0.2, G)

    def run(p):
        o = lib.AtcPpoValueGradOut(p["grad"], p["stats"], p["value"], p["scratch"])
        return _call(h, R_src, R, K, traffic=C.c_void_p(p["traffic"]), mask=C.c_void_p(p["mask"]), index=C.c_void_p(p["index"]), s=FAKE, w=C.c_void_p(p["w"]),
                     obs_rows=C.c_void_p(p["obs_rows"]), v_old=C.c_void_p(p["v_old"]), ret=C.c_void_p(p["ret"]), g=C.byref(gk), out=C.byref(o))
    names, outputs, n = list(size), ("grad", "stats", "value", "scratch"), 0
    for b in outputs:
        for a in names[:names.index(b)]:
            for off in (0, size[a] - 1, -(size[b] - 1)):
                assert run(dict(base, **{b: base[a] + off})) == -1 and b"overlaps" in err() and a.encode() in err() and b.encode() in err(), (a, b, off, err())
                n += 1
    assert n == (7 + 8 + 9 + 10) * 3
    assert _records() == before, "a refused call moved a launch record"


def test_value_forward_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    err = h.atc_last_error
    ptrs = ("s", "w", "x", "values")
    ok = dict(s=FAKE, w=C.c_void_p(_at(1)), x=C.c_void_p(_at(2)), values=C.c_void_p(_at(3)))
    call = lambda R, K, **a: h.atc_value_forward(a.get("s"), R, K, a.get("w"), a.get("x"), a.get("values"), None)      # noqa: E731
    for j, name in enumerate(ptrs):      # the pointers in their order, with R and K wrong as well
        named = re.compile(rb"null pointer: %s\b" % name.encode())
        assert call(0, 3, **{k: ok[k] for k in ptrs[:j]}) == -1 and named.search(err()), (name, err())
        assert call(0, 3, **dict(ok, **{name: None})) == -1 and named.search(err()), (name, err())
    for R in (0, -1):
        assert call(R, 3, **ok) == -1 and b"R (" in err()
    for K in (3, -1, 5, 8):
        assert call(7, K, **dict(ok, values=ok["x"])) == -1 and b"traffic_k" in err()
    R, K = 7, 2
    size = dict(x=R * L.policy_in(K) * 4, w=L.value_words(K) * 4)
    for a in ("x", "w"):
        for off in (0, size[a] - 1, -(R * 4 - 1)):
            assert call(R, K, **dict(ok, values=C.c_void_p(ok[a].value + off))) == -1 and b"overlaps" in err() and a.encode() in err() and b"values" in err(), (a, off, err())
    assert _records() == before, "a refused call moved a launch record"


def test_launch_records_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    for name in RECORDS:
        buf = (C.c_uint64 * 8)(*([99] * 8))
        assert getattr(h, name)(buf, 8) == 0
        assert all(v != 99 for v in buf[:4]) and all(v == 99 for v in buf[4:])
        assert getattr(h, name)(None, 1) == -1
        assert name in lib.launch_records()
    assert isinstance(lib.value_forward_launch_counts(), dict) and isinstance(lib.ppo_value_grad_launch_counts(), dict)


def test_python_surface():
    from atc_hip import ppo
    from atc_hip.vec_env import AtcVecEnv
    sig = inspect.signature(AtcVecEnv.value_forward)
    assert list(sig.parameters) == ["self", "weights", "rows", "out"] and sig.parameters["out"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(AtcVecEnv.ppo_value_grad)
    assert list(sig.parameters) == ["self", "weights", "obs_rows", "v_old", "ret", "traffic", "mask", "index", "clip", "workgroups", "out"]
    kw = ("traffic", "mask", "index", "clip", "workgroups", "out")
    assert [sig.parameters[k].default for k in kw] == [None, None, None, 0.2, 0, None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kw)
    sig = inspect.signature(ppo.value_grad)
    assert list(sig.parameters) == ["env", "collected", "weights", "index", "clip", "workgroups", "out"]
    assert [sig.parameters[k].default for k in ("index", "clip", "workgroups", "out")] == [None, 0.2, 0, None]
    assert list(inspect.signature(ppo.critic).parameters) == ["env", "weights"]
    assert "ppo_value_grad" in AtcVecEnv.ppo_policy_grad.__doc__ and "value_grad" in ppo.__doc__ and "critic" in ppo.__doc__
    # no keyword of collect changes
    names = ["env", "weights", "value_fn", "T", "hold", "traffic", "gamma", "lam", "seed", "decision0", "obs0", "per_decision"]
    assert list(inspect.signature(ppo.collect).parameters) == names == list(inspect.signature(ppo.collect_bootstrap).parameters)


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


def test_ppo_value_grad_refuses_before_any_library_call():
    import torch
    from atc_hip.vec_env import AtcVecEnv
    env = _NoLibrary()
    Rs, K = 12, 2
    ok = dict(weights=torch.zeros(L.value_words(0)), obs_rows=torch.zeros(Rs, 10), v_old=torch.zeros(Rs), ret=torch.zeros(Rs))

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            AtcVecEnv.ppo_value_grad(env, **dict(ok, **{k: v for k, v in kw.items() if k in ok}), **{k: v for k, v in kw.items() if k not in ok})
    for w in (torch.zeros(L.value_words(2)), torch.zeros(L.policy_words(0)), torch.zeros(L.value_words(0), dtype=torch.float64), np.zeros(L.value_words(0), np.float32),
              torch.zeros(2 * L.value_words(0))[::2], torch.zeros(L.value_words(0), device="meta")):
        refused("weights", weights=w)
    refused("weights", traffic=torch.zeros(Rs, K, 8))      # (the ten-word critic with a traffic critic's rows)
    for t in (torch.zeros(Rs, 3, 8), torch.zeros(Rs, K, 7), torch.zeros(K, 8), np.zeros((Rs, K, 8), np.float32)):
        refused("traffic", traffic=t)
    wk = torch.zeros(L.value_words(K))
    refused("traffic", weights=wk, traffic=torch.zeros(Rs + 1, K, 8))
    refused("traffic", weights=wk, traffic=torch.zeros(Rs, K, 8, dtype=torch.float64))
    for x in (torch.zeros(Rs, 9), torch.zeros(0, 10), torch.zeros(Rs, 10, dtype=torch.float64), torch.zeros(10, Rs).t(), np.zeros((Rs, 10), np.float32)):
        refused("obs_rows", obs_rows=x)
    refused("v_old", v_old=torch.zeros(Rs + 1))
    refused("v_old", v_old=torch.zeros(Rs, dtype=torch.float64))
    refused("ret", ret=torch.zeros(Rs - 1))
    refused("ret", ret=torch.zeros(2 * Rs)[::2])
    refused("mask", mask=torch.zeros(Rs, dtype=torch.bool))
    refused("mask", mask=torch.zeros(Rs + 1, dtype=torch.uint8))
    refused("index", index=torch.zeros(4, dtype=torch.int64))
    refused("index", index=torch.zeros(0, dtype=torch.int32))
    refused("index", index=torch.zeros(2, 2, dtype=torch.int32))
    for clip in (0.0, -1.0, float("nan"), -INF, 1e-60):
        refused("clip", clip=clip)
    for wg in (-1, L.PPO_GRAD_MAX_WG + 1):
        refused("workgroups", workgroups=wg)
    words = L.value_words(0)
    good = dict(grad=torch.zeros(words), stats=torch.zeros(8), value=torch.zeros(Rs), scratch=torch.zeros(1, words + 8))
    refused("out", out=[good["grad"]])
    refused("out", out=dict(good, logp=good["grad"]))
    refused(r"out\['grad'\]", out=dict(good, grad=torch.zeros(words + 1)))
    refused(r"out\['stats'\]", out=dict(good, stats=torch.zeros(8, dtype=torch.float64)))
    refused(r"out\['value'\]", out=dict(good, value=torch.zeros(Rs + 1)))
    refused(r"out\['value'\]", out=dict(good, value=torch.zeros(5)), index=torch.zeros(4, dtype=torch.int32))
    refused(r"out\['scratch'\]", out=dict(good, scratch=torch.zeros(2, words + 8)))      # (12 rows are one tile: G = 1)
    refused(r"out\['scratch'\]", out=dict(good), workgroups=3)
    for clip in (0.2, INF, 1e39):      # ... and a call that passes them all goes to the library (1e39 is +inf in float32)
        with pytest.raises(AssertionError, match="the library was called"):
            AtcVecEnv.ppo_value_grad(env, **ok, clip=clip, out=good)


def test_value_forward_refuses_before_any_library_call():
    import torch
    from atc_hip import ppo
    from atc_hip.vec_env import AtcVecEnv
    env = _NoLibrary()
    w0, w2 = torch.zeros(L.value_words(0)), torch.zeros(L.value_words(2))
    for rows in (torch.zeros(5, 9), torch.zeros(5, 31), torch.zeros(0, 10), torch.zeros(()), np.zeros((5, 10), np.float32)):
        with pytest.raises(ValueError, match="rows"):
            AtcVecEnv.value_forward(env, w0, rows)
    for rows in (torch.zeros(5, 10, dtype=torch.float64), torch.zeros(10, 5).t(), torch.zeros(5, 10, device="meta")):
        with pytest.raises(ValueError, match="rows"):
            AtcVecEnv.value_forward(env, w0, rows)
    for w in (w2, torch.zeros(L.policy_words(0)), w0.double(), torch.zeros(2 * L.value_words(0))[::2]):
        with pytest.raises(ValueError, match="weights"):
            AtcVecEnv.value_forward(env, w, torch.zeros(4, 3, 10))
    with pytest.raises(ValueError, match="weights"):      # K is taken from IN: 24 words are K = 2
        AtcVecEnv.value_forward(env, w0, torch.zeros(4, 24))
    for out in (torch.zeros(12), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(3, 4).t(), np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError, match="out"):
            AtcVecEnv.value_forward(env, w0, torch.zeros(4, 3, 10), out=out)
    for w, rows in ((w0, torch.zeros(4, 3, 10)), (w2, torch.zeros(7, 24)), (w0, torch.zeros(10))):
        with pytest.raises(AssertionError, match="the library was called"):
            AtcVecEnv.value_forward(env, w, rows, out=torch.zeros(tuple(rows.shape[:-1])))
    env.value_forward = lambda w, rows, out=None: ("called", w, tuple(rows.shape), rows.is_contiguous())      # ppo.critic hands its rows on
    assert ppo.critic(env, w0)(torch.zeros(5, 3, 2, 10)) == ("called", w0, (5, 3, 2, 10), True)
    assert ppo.critic(env, w0)(torch.zeros(10, 6, 5).permute(2, 1, 0))[2:] == ((5, 6, 10), True)


@pytest.mark.parametrize("K", KS)
def test_value_offsets_and_pack_mlp_round_trip_against_a_torch_module(K):
    import torch
    from torch import nn
    from atc_hip import value
    torch.manual_seed(5 + K)
    n_in = L.policy_in(K)
    net = nn.Sequential(nn.Linear(n_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1))
    w = value.from_torch(net, traffic=K)
    assert w.dtype == torch.float32 and tuple(w.shape) == (L.value_words(K),) and w.is_contiguous()
    off = value.offsets(K)
    assert list(off) == list(PV.PART_NAMES) and off["W1"] == (0, (64, n_in)) and off["b3"] == (L.value_words(K) - 1, (1,))
    lin = list(net)[0::2]
    for name, t in zip(PV.PART_NAMES, (lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias)):
        at, shape = off[name]
        assert torch.equal(w[at:at + t.numel()].reshape(shape), t.detach()), name
        assert np.array_equal(PV.split(w.numpy(), K)[name], t.detach().numpy()), name
    x = torch.randn(33, n_in)
    v = PV.forward(w.numpy(), x.numpy(), K, np.float64)
    assert np.max(np.abs(v - net.double()(x.double()).detach().numpy()[:, 0])) <= 1e-12
    with pytest.raises(ValueError, match="W3"):
        value.pack_mlp(lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight.reshape(64), lin[2].bias, traffic=K)
    with pytest.raises(ValueError, match="Sequential"):
        value.from_torch(nn.Sequential(nn.Linear(n_in, 64), nn.ReLU(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)), traffic=K)
    with pytest.raises(ValueError, match="traffic"):
        value.shapes(3)


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatement
def _torch_grad(case):
    """(grad, means, value) of the contract through torch.autograd in float64, the loss written with torch.maximum / torch.clamp"""
    import torch
    K = int(case["K"])
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in PV.split(case["w"], K).items()}
    src, part = PV._select(case)
    rows = torch.tensor(PV.input_rows(case["obs_rows"], case.get("traffic"), K)[src][part].astype(np.float64))
    v_old = torch.tensor(np.asarray(case["v_old"], np.float64).reshape(-1)[src][part])
    ret = torch.tensor(np.asarray(case["ret"], np.float64).reshape(-1)[src][part])
    clip = float(np.float32(case["clip"]))
    v = (torch.tanh(torch.tanh(rows @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"]) @ p["W3"].T + p["b3"])[:, 0]
    vc = v_old + torch.clamp(v - v_old, -clip, clip)
    loss = 0.5 * torch.maximum((v - ret) ** 2, (vc - ret) ** 2)
    loss.sum().div(int(part.sum())).backward()
    grad = np.concatenate([p[name].grad.numpy().reshape(-1) for name in PV.PART_NAMES])
    means = [float(t.detach().mean()) for t in (loss, v, ret, ret ** 2, (ret - v) ** 2)]
    return grad, means, v.detach().numpy(), float((v.detach() - v_old).abs().max())


@pytest.mark.parametrize("clip", (0.2, INF))
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mask,index", ((False, False), (True, False), (False, True), (True, True)))
def test_float64_restatement_equals_torch_autograd(K, mask, index, clip):
    case = PV.make_case(100 + K, 150, K=K, gain=1.0, raw=False, mask=mask, index=index, clip=clip)
    ref = PV.evaluate(case, np.float64)
    grad, means, v, dmax = _torch_grad(case)
    assert 0 < ref["n"] <= 150 and (ref["n"] < 150) == (mask or index)
    assert (ref["n_cut"] > 0) == (clip != INF)
    g_ref, g_t = PV.split(ref["grad"], K), PV.split(grad, K)
    for name in PV.PART_NAMES:
        top = np.max(np.abs(g_t[name]))
        assert top > 0 and np.max(np.abs(g_ref[name] - g_t[name])) <= 1e-10 * top, (name, np.max(np.abs(g_ref[name] - g_t[name])), top)
    for q, m in zip(PV.MEANS, means):
        assert abs(ref["stats"][q] - m) <= 1e-10 * max(1.0, abs(m)), q
    assert ref["stats"][PV.STAT_N] == ref["n"] and ref["stats"][PV.STAT_CUT] == ref["n_cut"] / ref["n"]
    assert abs(ref["stats"][PV.STAT_DV_MAX] - dmax) <= 1e-10 * dmax
    assert np.max(np.abs(ref["value"][ref["part"]] - v)) <= 1e-10 * np.max(np.abs(v))
    assert np.all(np.isnan(ref["value"][~ref["part"]]))


def test_a_nan_value_stays_a_nan_in_the_restatement():
    L_, dv, cut, inside, d, e2, ec2 = PV.loss_terms(np.array([np.nan, 1.0]), np.array([0.0, 0.0]), np.array([0.5, 0.5]), 0.2)
    assert np.isnan(L_[0]) and np.isnan(dv[0]) and not cut[0] and not inside[0]
    assert L_[1] == 0.5 * 0.25 and dv[1] == 0.5 and not cut[1]      # outside, e^2 = 0.25 >= ec^2 = 0.09: it flows


# the GPU cases: (seed, R, G, K, gain, raw, mask, index, clip)
CASES = ((1, 1, 1, 0, 1.0, False, False, False, INF), (2, 63, 2, 1, 8.0, False, True, False, 0.2), (3, 64, 1, 2, 1.0, True, False, True, 0.2),
         (4, 65, 3, 4, 1.0, False, True, True, 0.2), (5, 130, 2, 0, 8.0, True, True, True, 0.2), (6, 300, 3, 4, 8.0, True, True, True, 0.2),
         (7, 300, 1, 2, 1.0, False, False, False, 0.2), (8, 300, 3, 1, 1.0, True, True, False, 0.2), (9, 65, 2, 0, 1.0, False, False, True, 0.2),
         (10, 130, 3, 0, 1.0, False, True, True, INF), (11, 64, 3, 1, 1.0, False, False, False, 0.2))
_ids = ["R%d-G%d-K%d-gain%g%s%s%s-clip%g" % (c[1:5] + ("-raw" if c[5] else "", "-mask" if c[6] else "", "-index" if c[7] else "", c[8])) for c in CASES]
_cases = pytest.mark.parametrize("case_id", range(len(CASES)), ids=_ids)


@functools.lru_cache(maxsize=None)
def _case(case_id):
    """the case, its float64 restatement, its float32 twin and the bars: computed once, shared, never written to"""
    seed, R, G, K, gain, raw, mask, index, clip = CASES[case_id]
    case = PV.make_case(seed, R, K=K, gain=gain, raw=raw, mask=mask, index=index, clip=clip)
    ref64, ref32 = PV.evaluate(case, np.float64), PV.evaluate(case, np.float32)
    return case, ref64, ref32, PV.bars(case, ref64, ref32), G


def test_the_cases_cover_what_they_claim():
    assert {c[1] for c in CASES} == {1, 63, 64, 65, 130, 300} and {c[2] for c in CASES} == {1, 2, 3} and {c[3] for c in CASES} == set(KS)
    assert {c[4] for c in CASES} == {1.0, 8.0} and {c[5] for c in CASES} == {False, True} and {c[8] for c in CASES} == {0.2, INF}
    masked = out_of_range = wide = repeated = 0
    for i, c in enumerate(CASES):
        case, ref64, ref32, bars, G = _case(i)
        part = ref64["part"]
        assert np.array_equal(part, ref32["part"]) and np.array_equal(ref64["cut"], ref32["cut"]) and np.array_equal(ref64["inside"], ref32["inside"]), c
        if c[8] != INF:
            near, tie = PV.margins(case, ref64)
            assert near >= PV.CLIP_MARGIN and tie >= PV.TIE_MARGIN, (c, near, tie)      # no row may take another branch in float32: none is excused
            clip = np.float64(np.float32(c[8]))
            inside = part & (np.abs(ref64["delta"]) < clip)
            flows = part & (np.abs(ref64["delta"]) > clip) & ~ref64["cut"]
            assert inside.sum() >= 1 and flows.sum() >= 1 and ref64["cut"].sum() >= 1, (c, inside.sum(), flows.sum(), ref64["cut"].sum())
        else:
            assert ref64["n_cut"] == 0 and ref64["n"] >= 1
        src, _ = PV._select(case)
        if case["mask"] is not None:
            masked += int((case["mask"] == 0).sum())
        if case["index"] is not None:
            idx = case["index"].astype(np.int64)
            out_of_range += int(((idx < 0) | (idx >= case["R_src"])).sum())
            repeated += int(len(idx) - len(np.unique(idx)))
        x = PV.input_rows(case["obs_rows"], case["traffic"], case["K"])[src][part]
        wide += int((np.abs(x).max(axis=1) > 4.0).sum()) if x.size else 0
        assert not c[5] or np.abs(x).max() > 1e4, c      # raw rows carry 1.5e4-magnitude words
    assert min(masked, out_of_range, wide, repeated) > 0, (masked, out_of_range, wide, repeated)
    # partial tiles, a workgroup that loops (tiles > G) and workgroups with unequal loads (tiles % G != 0)
    assert any(c[1] % 64 for c in CASES) and any(-(-c[1] // 64) > c[2] for c in CASES) and any(-(-c[1] // 64) % c[2] for c in CASES if c[2] > 1)


# ---------------------------------------------------------------------------------------------------------------- GPU
CFG = dict(normalize=True, shaping=True, auto_reset=True, timestep_limit=7, spawn="lattice")


@functools.lru_cache(maxsize=None)
def _env():
    return H.policy_env(CFG, 2, 1)


def _dev(case, env):
    import torch
    t = lambda v: None if v is None else torch.as_tensor(np.ascontiguousarray(v), device=env.device)      # noqa: E731
    return dict(weights=t(case["w"]), obs_rows=t(case["obs_rows"]), v_old=t(case["v_old"]), ret=t(case["ret"]), traffic=t(case["traffic"]), mask=t(case["mask"]),
                index=t(case["index"]))


def _call_gpu(env, case, G, dev=None, out=None):
    d = _dev(case, env) if dev is None else dev
    res = env.ppo_value_grad(d["weights"], d["obs_rows"], d["v_old"], d["ret"], traffic=d["traffic"], mask=d["mask"], index=d["index"], clip=case["clip"],
                             workgroups=G, out=out)
    env.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _hold(got, ref64, bars, K, tag):
    """every part of grad, the means of stats and value within its bar of the float64 restatement; n and the cut count exact; max |v - v_old|
    within value's bar.  Prints deviation / bar."""
    worst = {}
    g, r = PV.split(got["grad"].astype(np.float64), K), PV.split(ref64["grad"], K)
    for name in PV.PART_NAMES:
        worst[name] = float(np.max(np.abs(g[name] - r[name]))) / bars[name][0] if bars[name][0] > 0 else 0.0
    n = ref64["n"]
    assert got["stats"][PV.STAT_N] == n, (tag, got["stats"])
    if n:
        assert round(float(got["stats"][PV.STAT_CUT]) * n) == ref64["n_cut"] and abs(got["stats"][PV.STAT_CUT] - ref64["n_cut"] / n) <= 1e-6, (tag, got["stats"], ref64["n_cut"])
        sel = list(PV.MEANS)
        worst["stats"] = float(np.max(np.abs(got["stats"][sel].astype(np.float64) - ref64["stats"][sel]))) / bars["stats"][0]
        part = ref64["part"]
        worst["value"] = float(np.max(np.abs(got["value"][part].astype(np.float64) - ref64["value"][part]))) / bars["value"][0]
        worst["max |dv|"] = abs(float(got["stats"][PV.STAT_DV_MAX]) - ref64["stats"][PV.STAT_DV_MAX]) / bars["value"][0]
    print("%s: kernel deviation / bar: %s" % (tag, ", ".join("%s %.3f" % kv for kv in worst.items())))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad, {k: bars.get(k, bars["value"]) for k in bad})
    return worst


FORWARD = ((0, 1), (3, 65), (4, 167), (5, 337), (6, 300), (7, 300))      # (case whose source rows are taken, how many of them)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id,R", FORWARD, ids=["%s-rows%d" % (_ids[c], r) for c, r in FORWARD])
def test_value_forward_within_the_twin_bar(case_id, R):
    import torch
    from atc_hip import lib
    case = _case(case_id)[0]
    K = case["K"]
    env = _env()
    x = np.ascontiguousarray(PV.input_rows(case["obs_rows"], case["traffic"], K)[:R])
    assert x.shape == (R, L.policy_in(K))
    bar, dev, v64 = PV.forward_bar(case["w"], x, K)
    before, others = lib.value_forward_launch_counts().get(K, 0), {k: v for k, v in lib.launch_records().items() if k != "atc_value_forward_launch_counts"}
    w, xd = torch.as_tensor(case["w"], device=env.device), torch.as_tensor(x, device=env.device)
    got = env.value_forward(w, xd)
    env.synchronize()
    assert lib.value_forward_launch_counts().get(K, 0) == before + 1
    assert {k: v for k, v in lib.launch_records().items() if k != "atc_value_forward_launch_counts"} == others
    assert got.shape == (R,) and got.dtype == torch.float32
    worst = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - v64))) / bar
    print("%s rows %d: value_forward deviation / bar %.3f (bar %.3e, twin deviation %.3e)" % (_ids[case_id], R, worst, bar, dev))
    assert worst <= 1.0
    # out=: the same bits, nothing allocated, and one word more is left alone
    buf = torch.full((R + 1,), SENTINEL, device=env.device)
    torch.cuda.synchronize(env.device)
    held = torch.cuda.memory_allocated(env.device)
    res = env.value_forward(w, xd, out=buf[:R])
    env.synchronize()
    assert torch.cuda.memory_allocated(env.device) == held and res.data_ptr() == buf.data_ptr()
    assert torch.equal(res.view(torch.int32), got.view(torch.int32)) and float(buf[R]) == SENTINEL
    if R >= 60:      # a [2 D + 1, B, N, IN] input returns [2 D + 1, B, N]
        shaped = env.value_forward(w, xd[:60].reshape(5, 3, 4, -1))
        env.synchronize()
        assert tuple(shaped.shape) == (5, 3, 4)
        if not CASES[case_id][5]:      # (a wavefront of fewer rows may sum its first layer otherwise where raw rows stand; rows within 4 never differ)
            assert torch.equal(shaped.reshape(-1).view(torch.int32), got[:60].view(torch.int32))


@pytest.mark.gpu
@_cases
def test_grad_stats_and_value_within_the_twin_bars(case_id):
    import torch
    case, ref64, ref32, bars, G = _case(case_id)
    env = _env()
    from atc_hip import lib
    K = case["K"]
    before = lib.ppo_value_grad_launch_counts().get(K, 0)
    others = {k: v for k, v in lib.launch_records().items() if k != "atc_ppo_value_grad_launch_counts"}
    d = _dev(case, env)
    words = L.value_words(K)
    out = dict(grad=torch.full((words,), SENTINEL, device=env.device), stats=torch.full((8,), SENTINEL, device=env.device),
               value=torch.full((case["R"],), SENTINEL, device=env.device), scratch=torch.full((G, words + 8), SENTINEL, device=env.device))
    got = _call_gpu(env, case, G, d, out)
    assert lib.ppo_value_grad_launch_counts().get(K, 0) == before + 1
    assert {k: v for k, v in lib.launch_records().items() if k != "atc_ppo_value_grad_launch_counts"} == others
    _hold(got, ref64, bars, K, _ids[case_id])
    assert np.all(got["value"][~ref64["part"]] == np.float32(SENTINEL)), "a row that takes no part had its value written"
    assert not np.any(got["value"][ref64["part"]] == np.float32(SENTINEL))
    if case["clip"] == INF:
        assert got["stats"][PV.STAT_CUT] == 0.0
    # the same inputs and the same G: the same bits
    again = _call_gpu(env, case, G, d, out)
    for k in ("grad", "stats", "value"):
        assert _same(got[k], again[k]), k
    # without out=, and with the library's own G
    free = _call_gpu(env, case, 0, d)
    assert np.all(np.isnan(free["value"][~ref64["part"]]))
    if L.ppo_grad_workgroups(case["R"]) == G:
        assert _same(free["grad"], got["grad"]) and _same(free["stats"], got["stats"])
    _hold(free, ref64, bars, K, _ids[case_id] + " (G = 0)")


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", (3, 5, 6, 8), ids=lambda i: _ids[i])
def test_value_equals_value_forward_bit_for_bit(case_id):
    """value of the grad call against value_forward on the rows its tiles hold — gathered through index, the rows that take no part as zeros —
    and, without an index or a mask, on the source rows as they lie"""
    import torch
    case, ref64, ref32, bars, G = _case(case_id)
    env = _env()
    got = _call_gpu(env, case, G)
    src, part = PV._select(case)
    rows = PV.input_rows(case["obs_rows"], case["traffic"], case["K"])
    x = np.ascontiguousarray(np.where(part[:, None], rows[src], 0).astype(np.float32))
    fwd = env.value_forward(torch.as_tensor(case["w"], device=env.device), torch.as_tensor(x, device=env.device))
    env.synchronize()
    fwd = fwd.cpu().numpy()
    assert part.sum() > 0 and _same(got["value"][part], fwd[part])
    if case["index"] is None and case["mask"] is None:
        assert _same(got["value"], fwd)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", (4, 5, 6), ids=lambda i: _ids[i])
def test_one_workgroup_and_three_agree_within_the_bars(case_id):
    case, ref64, ref32, bars, _ = _case(case_id)
    env = _env()
    d = _dev(case, env)
    one, three = _call_gpu(env, case, 1, d), _call_gpu(env, case, 3, d)
    _hold(one, ref64, bars, case["K"], _ids[case_id] + " G=1")
    _hold(three, ref64, bars, case["K"], _ids[case_id] + " G=3")
    assert _same(one["value"], three["value"]) and all(one["stats"][q] == three["stats"][q] for q in (PV.STAT_N, PV.STAT_CUT, PV.STAT_DV_MAX))
    a, b = PV.split(one["grad"].astype(np.float64), case["K"]), PV.split(three["grad"].astype(np.float64), case["K"])
    for name in PV.PART_NAMES:
        assert np.max(np.abs(a[name] - b[name])) <= 2.0 * bars[name][0], name      # (each is within one bar of the restatement)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", (3, 5), ids=lambda i: _ids[i])
def test_nans_in_rows_that_take_no_part_change_no_bit(case_id):
    case, ref64, ref32, bars, G = _case(case_id)
    env = _env()
    clean = _call_gpu(env, case, G)
    src, part = PV._select(case)
    used = np.zeros(case["R_src"], bool)
    used[src[part]] = True
    assert (~used).sum() > 0
    dirty = dict(case)
    for k in ("obs_rows", "v_old", "ret", "traffic"):
        if case[k] is not None:
            v = case[k].copy()
            v[~used] = np.nan
            dirty[k] = v
    got = _call_gpu(env, dirty, G)
    for k in ("grad", "stats"):
        assert _same(clean[k], got[k]), k
    assert _same(clean["value"][ref64["part"]], got["value"][ref64["part"]]) and np.all(np.isnan(got["value"][~ref64["part"]]))


@pytest.mark.gpu
def test_a_mask_of_zeros_and_indices_all_out_of_range():
    import torch
    case, ref64, ref32, bars, G = _case(8)
    env = _env()
    none = dict(case, mask=np.zeros(case["R_src"], np.uint8))
    for c in (none, dict(case, index=np.full(case["R"], case["R_src"], np.int32)), dict(case, index=np.full(case["R"], -5, np.int32))):
        d = _dev(c, env)
        out = dict(value=torch.full((case["R"],), SENTINEL, device=env.device))
        got = _call_gpu(env, c, G, d, out)
        assert np.all(got["grad"] == 0) and np.all(got["stats"] == 0) and got["grad"].shape == (L.value_words(case["K"]),)
        assert np.all(got["value"] == np.float32(SENTINEL))


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", (4, 6), ids=lambda i: _ids[i])
def test_clip_inf_is_the_plain_squared_error(case_id):
    case, _, _, _, G = _case(case_id)
    env = _env()
    plain = dict(case, clip=INF)
    ref64, ref32 = PV.evaluate(plain, np.float64), PV.evaluate(plain, np.float32)
    v = ref64["value"][ref64["part"]]
    ret = np.asarray(case["ret"], np.float64)[PV._select(case)[0]][ref64["part"]]
    assert ref64["n_cut"] == 0 and abs(ref64["stats"][PV.STAT_LOSS] - 0.5 * np.mean((v - ret) ** 2)) <= 1e-12 * ref64["stats"][PV.STAT_LOSS]
    assert abs(ref64["stats"][PV.STAT_LOSS] - 0.5 * ref64["stats"][PV.STAT_ERR2]) <= 1e-12 * ref64["stats"][PV.STAT_LOSS]
    got = _call_gpu(env, plain, G)
    assert got["stats"][PV.STAT_CUT] == 0.0
    _hold(got, ref64, PV.bars(plain, ref64, ref32), case["K"], _ids[case_id] + " with clip = inf")


@pytest.mark.gpu
def test_out_with_all_four_buffers_allocates_nothing():
    import torch
    case, ref64, ref32, bars, G = _case(5)
    env = _env()
    d = _dev(case, env)
    words = L.value_words(case["K"])
    out = dict(grad=torch.empty(words, device=env.device), stats=torch.empty(8, device=env.device), value=torch.empty(case["R"], device=env.device),
               scratch=torch.empty((G, words + 8), device=env.device))
    pos = [d[k] for k in ("weights", "obs_rows", "v_old", "ret")]
    kw = dict(traffic=d["traffic"], mask=d["mask"], index=d["index"], clip=case["clip"], workgroups=G, out=out)
    env.ppo_value_grad(*pos, **kw)
    env.synchronize()
    torch.cuda.reset_peak_memory_stats(env.device)
    before = torch.cuda.memory_allocated(env.device)
    res = env.ppo_value_grad(*pos, **kw)
    env.synchronize()
    assert torch.cuda.memory_allocated(env.device) == before and torch.cuda.max_memory_allocated(env.device) == before
    assert res["grad"] is out["grad"] and res["stats"] is out["stats"] and res["value"] is out["value"] and "scratch" not in res


@pytest.mark.gpu
def test_refusals_that_need_a_device():
    import torch
    case, ref64, ref32, bars, G = _case(5)      # K = 4, with a mask and an index
    env = _env()
    d = _dev(case, env)
    pos = [d[k] for k in ("weights", "obs_rows", "v_old", "ret")]
    kw = dict(traffic=d["traffic"], mask=d["mask"], index=d["index"])
    before = _records()
    with pytest.raises(ValueError, match="weights"):
        env.ppo_value_grad(d["weights"].cpu(), *pos[1:], **kw)
    with pytest.raises(ValueError, match="mask"):
        env.ppo_value_grad(*pos, **dict(kw, mask=d["mask"].cpu()))
    with pytest.raises(ValueError, match="weights"):      # the rows say K = 4, the array K = 0
        env.ppo_value_grad(d["weights"][:L.value_words(0)].contiguous(), *pos[1:], **kw)
    words = L.value_words(case["K"])
    with pytest.raises(ValueError, match=r"out\['scratch'\]"):
        env.ppo_value_grad(*pos, **kw, workgroups=2, out=dict(scratch=torch.zeros((3, words + 8), device=env.device)))
    with pytest.raises(ValueError, match=r"out\['scratch'\]"):
        env.ppo_value_grad(*pos, **kw, workgroups=2, out=dict(scratch=torch.zeros((2, words + 7), device=env.device)))
    big = torch.zeros(words + 8 + case["R"], device=env.device)
    for out, a, b in ((dict(grad=d["weights"]), "w", "grad"), (dict(value=d["ret"][:case["R"]]), "ret", "value"),
                      (dict(grad=big[:words], stats=big[words - 1:words + 7]), "grad", "stats"), (dict(stats=big[:8], value=big[7:7 + case["R"]]), "stats", "value")):
        with pytest.raises(RuntimeError, match="%s overlaps %s" % (a, b)):
            env.ppo_value_grad(*pos, **kw, out=out)
    x = torch.zeros((5, L.policy_in(4)), device=env.device)
    with pytest.raises(ValueError, match="rows"):
        env.value_forward(d["weights"], x.cpu())
    with pytest.raises(ValueError, match="out"):
        env.value_forward(d["weights"], x, out=torch.zeros(5))
    with pytest.raises(RuntimeError, match="x overlaps values"):
        env.value_forward(d["weights"], x, out=x.reshape(-1)[3:8])
    env.synchronize()
    assert _records() == before


E2E = ((4, 4, 1, 0), (4, 4, 2, 0), (3, 4, 2, 0), (4, 4, 1, 2), (4, 4, 2, 2))      # (B, N, hold, K): K = 0 through collect_bootstrap, K = 2 through collect(traffic=2)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,hold,K", E2E, ids=["%dx%d-hold%d-K%d" % c for c in E2E])
def test_end_to_end_behind_the_collection_with_the_same_critic(B, N, hold, K):
    """collect_bootstrap (collect(traffic=2)) with ppo.critic -> ppo.value_grad with the SAME critic (a time limit of 7 ends episodes inside
    the collection): values and boot equal an nn.Sequential float64 forward on the same rows within the forward bar; value equals
    values[:-1] bit for bit where control is 1, max |v - v_old| is 0 and no row is cut.  (The raw observation behind an auto-reset exceeds 4:
    the wavefronts that hold one sum their first layer in float64, in the collection's forward and in the gradient's tiles alike.)"""
    import torch
    from torch import nn
    from atc_hip import ppo, value
    env = H.policy_env(CFG, B, N, traffic=K)
    D = 8 if hold == 1 else 4      # (T = 8 steps against a limit of 7)
    T = D * hold
    w = torch.as_tensor(P.random_weights(np.random.default_rng([23, K]), 1.0, (-0.5, -1.0, 0.25), False, K), device=env.device)
    torch.manual_seed(7 + K)
    n_in = L.policy_in(K)
    net = nn.Sequential(nn.Linear(n_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1))
    vw = value.from_torch(net, device=env.device, traffic=K)
    obs0 = env.obs.clone()
    if K:
        res = ppo.collect(env, w, ppo.critic(env, vw), T, hold=hold, traffic=K, seed=99, decision0=7)
    else:
        res = ppo.collect_bootstrap(env, w, ppo.critic(env, vw), T, hold=hold, seed=99, decision0=7)
    assert tuple(res["values"].shape) == (D + 1, B, N) and tuple(res["ret"].shape) == (D, B, N) and bool(res["done"].any())
    if K:
        rows = torch.cat([ppo.value_rows(env, res, obs0, hold=hold)[:-1], res["traffic"][..., :7].reshape(D, B, N, 7 * K)], dim=-1)      # (the D decisions' rows)
        stored = res["values"][:-1]
    else:
        rows = torch.cat([ppo.value_rows(env, res, obs0, hold=hold), res["term_obs"].reshape(D, B, N, 10)], dim=0)
        stored = torch.cat([res["values"], res["boot"]], dim=0)
        assert tuple(res["boot"].shape) == (D, B, N)
    x = rows.cpu().numpy().reshape(-1, n_in)
    within = bool(np.abs(x).max() <= 4.0)      # every wavefront sums its first layer in float32, however its rows are grouped
    print("end to end %dx%d hold %d K %d: largest input word %.4g" % (B, N, hold, K, np.abs(x).max()))
    bar, dev, v64 = PV.forward_bar(vw.cpu().numpy(), x, K)
    ref = net.double()(torch.as_tensor(x, dtype=torch.float64)).detach().numpy()[:, 0]
    assert np.max(np.abs(ref - v64)) <= 1e-12
    worst = float(np.max(np.abs(stored.cpu().numpy().reshape(-1).astype(np.float64) - ref))) / bar
    print("end to end %dx%d hold %d K %d: values (and boot) deviation / bar %.3f" % (B, N, hold, K, worst))
    assert worst <= 1.0
    got = ppo.value_grad(env, res, vw, clip=0.2)
    env.synchronize()
    control = res["control"].bool().reshape(-1) if "control" in res else torch.ones(D * B * N, dtype=torch.bool, device=env.device)
    assert 0 < int(control.sum()) == int(got["stats"][PV.STAT_N])
    old = res["values"][:-1].reshape(-1)
    assert torch.equal(got["value"][control].view(torch.int32), old[control].view(torch.int32))
    assert bool(torch.isnan(got["value"][~control]).all())
    assert float(got["stats"][PV.STAT_DV_MAX]) == 0.0 and float(got["stats"][PV.STAT_CUT]) == 0.0 and float(got["grad"].abs().max()) > 0
    # the gradient on the collection within the bars of the restatement
    case = dict(K=K, w=vw.cpu().numpy(), obs_rows=x[:D * B * N, :10].copy(), traffic=res["traffic"].cpu().numpy().reshape(-1, K, 8) if K else None,
                v_old=old.cpu().numpy(), ret=res["ret"].cpu().numpy().reshape(-1), clip=0.2, mask=control.cpu().numpy().astype(np.uint8) if "control" in res else None,
                index=None, R=D * B * N, R_src=D * B * N)
    ref64, ref32 = PV.evaluate(case, np.float64), PV.evaluate(case, np.float32)
    _hold({k: v.cpu().numpy() for k, v in got.items()}, ref64, PV.bars(case, ref64, ref32), K, "end to end %dx%d hold %d K %d" % (B, N, hold, K))
    mb = torch.randperm(D * B * N, device=env.device).to(torch.int32)[:40].contiguous()
    part = ppo.value_grad(env, res, vw, index=mb, clip=INF)
    env.synchronize()
    assert part["value"].shape == (40,) and int(part["stats"][PV.STAT_N]) == int(control[mb.long()].sum())
    sel = control[mb.long()]
    if within:
        assert torch.equal(part["value"][sel].view(torch.int32), old[mb.long()][sel].view(torch.int32))
    env.close()
