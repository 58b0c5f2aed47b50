"""The PPO policy loss and gradient in one call (include/atc_step.h: atc_ppo_policy_grad; AtcVecEnv.ppo_policy_grad; atc_hip/ppo.py:
policy_grad): forward, clipped surrogate and backward of the 10 + 7 K -> 64 -> 64 -> 3 policy per row, the weight gradients summed over
the rows, no activation written to memory.

CPU: the exports and one kernel symbol per K; constants, structs and argtypes across the header, atc_hip/layout.py and atc_hip/lib.py; the
refusal order through ctypes with NULL and made-up pointers; the launch record; the Python surface and its refusals before any library call;
tests/ppo_grad_ref.py (the float64 restatement) against torch.autograd in float64 with the loss written with torch.minimum / torch.clamp,
for every K, with and without mask and index, within 1e-10 of each part's largest word; the surrogate on a clip boundary and at A = 0; what
the GPU cases contain, and that none of their rows lies within 1e-4 of a clip boundary or has |A| < 1e-6.
GPU: every part of grad, stats and logp against the float64 restatement within 4 x the float32 twin's own deviation (floor 1e-6 x the
part's largest word), n and the cut count exact, mean (logp_old - logp) and max |logp - logp_old| within logp's bar (they are differences
of logp words: ppo_grad_ref.STATS_OF_LOGP) — the measured deviation / bar is printed before it is asserted —; two runs bit for bit;
G = 1 against G = 3; NaNs in the rows that take no part; a mask of zeros; the logp sentinel; out= without an allocation; the refusals that
need a device; end to end behind rollout_policy_ends and gae_boot with the SAME weights, K = 0 and K = 2.

Measured on an MI355X, largest kernel deviation / bar over the cases below: W1 0.36, b1 0.49, W2 0.35, b2 0.42, W3 0.38, b3 0.54, log_std 0.46,
mean loss and mean ratio 0.34, KL and max |dlogp| 0.12, logp 0.39."""
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
import ppo_grad_ref as PG
from atc_hip import layout as L
from held_tools import HEADER, LIB, struct_fields

NAMES = ("atc_ppo_policy_grad", "atc_ppo_policy_grad_launch_counts")
FAKE = C.c_void_p(0x100000)
KS = (0, 1, 2, 4)
SENTINEL = -12345.5
PTRS = ("s", "w", "obs_rows", "action", "logp_old", "adv", "g", "out")      # the pointers that may not be NULL, in the order they are looked at


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
        assert len(re.findall(r"\bvoid k_ppo_grad<%d>\(" % K, text)) == 1, K
    assert len(re.findall(r"\bk_ppo_grad_reduce\(", text)) == 1
    blob = open(LIB, "rb").read()
    for K in KS:      # ... and in the embedded code object
        assert blob.count(b"_Z10k_ppo_gradILi%dEEviiPKfS1_S1_S1_S1_S1_PKhPKi12atc_ppo_gradPfS7_\0" % K) >= 1, K
    assert blob.count(b"_Z17k_ppo_grad_reduceiiPKfPfS1_\0") >= 1


def test_header_constants_structs_and_argtypes():
    from atc_hip import lib
    text = open(HEADER).read()
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, text).group(1))      # noqa: E731
    assert (L.PPO_GRAD_MAX_WG, L.PPO_GRAD_DEFAULT_WG, L.PPO_GRAD_STATS) == (define("ATC_PPO_GRAD_MAX_WG"), define("ATC_PPO_GRAD_DEFAULT_WG"), define("ATC_PPO_GRAD_STATS")) == (1024, 512, 8)
    stat = ("N", "LOSS", "KL", "CUT", "RATIO", "DLOGP_MAX")
    assert [define("ATC_PPO_STAT_" + n) for n in stat] == [getattr(L, "PPO_STAT_" + n) for n in stat] == list(range(6))
    assert (PG.STAT_N, PG.STAT_LOSS, PG.STAT_KL, PG.STAT_CUT, PG.STAT_RATIO, PG.STAT_DLOGP_MAX) == tuple(range(6)) and PG.STATS == L.PPO_GRAD_STATS
    assert L.PPO_GRAD_LAUNCH_SLOTS == int(re.search(r"ATC_PPO_GRAD_LAUNCH_SLOTS = (\d+)", text).group(1)) == 4
    assert L.ABI_VERSION == 22 and define("ATC_ABI_VERSION") == 22 and L.LAUNCH_SLOTS == 57      # a new entry point: the ABI number stays
    assert [L.ppo_grad_workgroups(R) for R in (1, 64, 65, 512 * 64, 512 * 64 + 1, 2 ** 31 - 1)] == [1, 1, 2, 512, 512, 512]
    assert L.ppo_grad_workgroups(10, 7) == 7
    scalar = {"float": C.c_float, "uint32_t": C.c_uint32, "int32_t": C.c_int32}
    g = struct_fields(text, "atc_ppo_grad")
    assert [f[1] for f in g] == list(lib.PPO_GRAD_FIELDS) == [f[0] for f in lib.AtcPpoGrad._fields_]
    assert [scalar[f[0]] for f in g] == [f[1] for f in lib.AtcPpoGrad._fields_] and C.sizeof(lib.AtcPpoGrad) == 24
    o = struct_fields(text, "atc_ppo_grad_out")
    assert [f[1].lstrip("*") for f in o] == list(lib.PPO_GRAD_OUT_FIELDS) == [f[0] for f in lib.AtcPpoGradOut._fields_]
    assert all(f[1].startswith("*") and f[0] == "float" for f in o) and C.sizeof(lib.AtcPpoGradOut) == 32
    decl = re.search(r"^int atc_ppo_policy_grad\((.*?)\);", text, flags=re.S | re.M).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "R_src", "R", "w", "obs_rows", "traffic", "action", "logp_old", "adv", "mask", "index", "g", "out", "stream"]
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    want = [ci if a.startswith("int ") else C.POINTER(lib.AtcPpoGrad) if "atc_ppo_grad_t" in a else C.POINTER(lib.AtcPpoGradOut) if "atc_ppo_grad_out_t" in a else vp
            for a in args]
    assert list(h.atc_ppo_policy_grad.argtypes) == want
    assert h.atc_ppo_policy_grad.restype is ci and h.atc_ppo_policy_grad_launch_counts.restype is ci
    assert list(h.atc_ppo_policy_grad_launch_counts.argtypes) == [C.POINTER(C.c_uint64), ci]
    slots, name = lib.LAUNCH_RECORDS["atc_ppo_policy_grad_launch_counts"]
    assert slots == 4 and [name(i) for i in range(4)] == [0, 1, 2, 4] and callable(lib.ppo_policy_grad_launch_counts)
    for word in ("entropy bonus", "value loss", "optimiser"):      # what is not in the call is said in the header
        assert word in text[text.index("PPO POLICY GRADIENT"):], word


def _at(k):
    return 0x100000 + k * 0x10000000      # made-up ranges 256 MiB apart


def _call(h, R_src=1, R=1, traffic=None, mask=None, index=None, **kw):
    a = dict.fromkeys(PTRS)
    a.update(kw)
    return h.atc_ppo_policy_grad(a["s"], R_src, R, a["w"], a["obs_rows"], traffic, a["action"], a["logp_old"], a["adv"], mask, index, a["g"], a["out"], None)


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    err = h.atc_last_error
    g = lib.AtcPpoGrad(0, 0.2, 0.0, 1.0, 0, 0)
    out = lib.AtcPpoGradOut(_at(10), _at(11), None, _at(12))
    ok = dict(s=FAKE, w=C.c_void_p(_at(1)), obs_rows=C.c_void_p(_at(2)), action=C.c_void_p(_at(3)), logp_old=C.c_void_p(_at(4)), adv=C.c_void_p(_at(5)),
              g=C.byref(g), out=C.byref(out))
    # 1. the pointers in their order, with everything behind them wrong as well (R = 0, R_src = 0)
    for j, name in enumerate(PTRS):
        named = re.compile(rb"null pointer: %s\b" % name.encode())
        assert _call(h, 0, 0, **{k: ok[k] for k in PTRS[:j]}) == -1 and named.search(err()), (name, err())
        assert _call(h, 0, 0, **dict(ok, **{name: None})) == -1 and named.search(err()), (name, err())
    bad = lib.AtcPpoGrad(3, float("nan"), 0.0, 1.0, -1, 0)
    for o, word in ((lib.AtcPpoGradOut(None, None, None, None), b"out->grad"), (lib.AtcPpoGradOut(_at(10), None, None, None), b"out->stats"),
                    (lib.AtcPpoGradOut(_at(10), _at(11), None, None), b"out->scratch")):
        assert _call(h, 0, 0, **dict(ok, g=C.byref(bad), out=C.byref(o))) == -1 and b"null pointer: " + word in err(), err()
    # 2. traffic_k, 3. R_src, R, index, 4. clip, 5. workgroups, 6. traffic iff K > 0: each with every later one wrong as well
    for K in (3, -1, 5, 8):
        assert _call(h, 0, 0, **dict(ok, g=C.byref(lib.AtcPpoGrad(K, float("nan"), 0.0, 1.0, -1, 0)))) == -1 and b"traffic_k" in err()
    nan_clip = C.byref(lib.AtcPpoGrad(1, float("nan"), 0.0, 1.0, -1, 0))
    assert _call(h, 0, 5, **dict(ok, g=nan_clip)) == -1 and b"R_src" in err()
    assert _call(h, 5, 0, **dict(ok, g=nan_clip)) == -1 and b"R (" in err()
    assert _call(h, 5, 4, **dict(ok, g=nan_clip)) == -1 and b"index is NULL" in err()
    assert _call(h, 5, 4, index=C.c_void_p(_at(6)), **dict(ok, g=nan_clip)) == -1 and b"clip" in err()      # (with an index R may differ)
    for clip in (float("nan"), float("inf"), 0.0, -0.1):
        assert _call(h, 5, 5, **dict(ok, g=C.byref(lib.AtcPpoGrad(1, clip, 0.0, 1.0, -1, 0)))) == -1 and b"clip" in err(), clip
    for wg in (-1, 1025):
        assert _call(h, 5, 5, **dict(ok, g=C.byref(lib.AtcPpoGrad(1, 0.2, 0.0, 1.0, wg, 0)))) == -1 and b"workgroups" in err() and b"1024" in err()
    assert _call(h, 5, 5, **dict(ok, g=C.byref(lib.AtcPpoGrad(1, 0.2, 0.0, 1.0, 1024, 0)), out=C.byref(lib.AtcPpoGradOut(_at(10), _at(10), None, _at(10))))) == -1 \
        and b"traffic is required" in err()
    assert _call(h, 5, 5, traffic=C.c_void_p(_at(7)), **dict(ok, out=C.byref(lib.AtcPpoGradOut(_at(10), _at(10), None, _at(10))))) == -1 and b"traffic must be NULL" in err()
    # 7. the overlap rule, on pointer values: every output against every input and every other output; the inputs may share
    R_src, R, K, G = 9, 7, 2, 3
    words = L.policy_words(K)
    size = dict(w=words * 4, obs_rows=R_src * 40, traffic=R_src * K * 32, action=R_src * 12, logp_old=R_src * 4, adv=R_src * 4, mask=R_src, index=R * 4,
                grad=words * 4, stats=32, logp_new=R * 4, scratch=G * (words + 8) * 4)
    base = {n: _at(k + 1) for k, n in enumerate(size)}
    gk = lib.AtcPpoGrad(K, 0.2, 0.0, 1.0, G, 0)

    def run(p):
        o = lib.AtcPpoGradOut(p["grad"], p["stats"], p["logp_new"], p["scratch"])
        return _call(h, R_src, R, traffic=C.c_void_p(p["traffic"]), mask=C.c_void_p(p["mask"]), index=C.c_void_p(p["index"]), s=FAKE, w=C.c_void_p(p["w"]),
                     obs_rows=C.c_void_p(p["obs_rows"]), action=C.c_void_p(p["action"]), logp_old=C.c_void_p(p["logp_old"]), adv=C.c_void_p(p["adv"]),
                     g=C.byref(gk), out=C.byref(o))
    names, outputs, n = list(size), ("grad", "stats", "logp_new", "scratch"), 0
    for b in outputs:
        for a in names[:names.index(b)]:
            for off in (0, size[a] - 1, -(size[b] - 1)):
                assert run(dict(base, **{b: base[a] + off})) == -1 and b"overlaps" in err() and a.encode() in err() and b.encode() in err(), (a, b, off, err())
                n += 1
    assert n == (8 + 9 + 10 + 11) * 3
    assert _records() == before, "a refused call moved a launch record"


def test_launch_record_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    buf = (C.c_uint64 * 8)(*([99] * 8))
    assert h.atc_ppo_policy_grad_launch_counts(buf, 8) == 0
    assert all(v != 99 for v in buf[:4]) and all(v == 99 for v in buf[4:])
    assert h.atc_ppo_policy_grad_launch_counts(None, 1) == -1
    assert isinstance(lib.ppo_policy_grad_launch_counts(), dict)
    assert "atc_ppo_policy_grad_launch_counts" in lib.launch_records()


def test_python_surface():
    from atc_hip import ppo
    from atc_hip.vec_env import AtcVecEnv
    sig = inspect.signature(AtcVecEnv.ppo_policy_grad)
    assert list(sig.parameters) == ["self", "weights", "obs_rows", "action", "logp_old", "adv", "traffic", "mask", "index", "clip", "adv_shift", "adv_scale",
                                    "workgroups", "out"]
    kw = ("traffic", "mask", "index", "clip", "adv_shift", "adv_scale", "workgroups", "out")
    assert [sig.parameters[k].default for k in kw] == [None, None, None, 0.2, 0.0, 1.0, 0, None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kw)
    sig = inspect.signature(ppo.policy_grad)
    assert list(sig.parameters)[:6] == ["env", "collected", "weights", "index", "clip", "normalise"]
    assert sig.parameters["index"].default is None and sig.parameters["normalise"].default is True
    for word in ("entropy bonus", "value loss", "optimiser"):
        assert word in AtcVecEnv.ppo_policy_grad.__doc__, word
    with pytest.raises(ValueError, match="traffic=0"):      # existing behaviour stays
        ppo.collect_bootstrap(None, None, None, 4, traffic=2)


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
    Rs, K = 12, 2
    ok = dict(weights=torch.zeros(L.policy_words(0)), obs_rows=torch.zeros(Rs, 10), action=torch.zeros(Rs, 3), logp_old=torch.zeros(Rs), adv=torch.zeros(Rs))

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            AtcVecEnv.ppo_policy_grad(env, **dict(ok, **{k: v for k, v in kw.items() if k in ok}), **{k: v for k, v in kw.items() if k not in ok})
    for w in (torch.zeros(L.policy_words(2)), torch.zeros(L.policy_words(0), dtype=torch.float64), np.zeros(L.policy_words(0), np.float32),
              torch.zeros(2 * L.policy_words(0))[::2], torch.zeros(L.policy_words(0), device="meta")):
        refused("weights", weights=w)
    refused("weights", traffic=torch.zeros(Rs, K, 8))      # (the ten-word array with a traffic policy's rows)
    for t in (torch.zeros(Rs, 3, 8), torch.zeros(Rs, K, 7), torch.zeros(K, 8), np.zeros((Rs, K, 8), np.float32)):
        refused("traffic", traffic=t)
    wk = torch.zeros(L.policy_words(K))
    refused("traffic", weights=wk, traffic=torch.zeros(Rs + 1, K, 8))
    refused("traffic", weights=wk, traffic=torch.zeros(Rs, K, 8, dtype=torch.float64))
    for x in (torch.zeros(Rs, 9), torch.zeros(0, 10), torch.zeros(Rs, 10, dtype=torch.float64), torch.zeros(10, Rs).t(), np.zeros((Rs, 10), np.float32)):
        refused("obs_rows", obs_rows=x)
    for a in (torch.zeros(Rs, 2), torch.zeros(Rs + 1, 3), torch.zeros(Rs, 3, dtype=torch.float64), torch.zeros(3, Rs).t()):
        refused("action", action=a)
    refused("logp_old", logp_old=torch.zeros(Rs + 1))
    refused("logp_old", logp_old=torch.zeros(Rs, dtype=torch.float64))
    refused("adv", adv=torch.zeros(Rs - 1))
    refused("adv", adv=torch.zeros(2 * Rs)[::2])
    refused("mask", mask=torch.zeros(Rs, dtype=torch.bool))
    refused("mask", mask=torch.zeros(Rs + 1, dtype=torch.uint8))
    refused("index", index=torch.zeros(4, dtype=torch.int64))
    refused("index", index=torch.zeros(0, dtype=torch.int32))
    refused("index", index=torch.zeros(2, 2, dtype=torch.int32))
    for clip in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        refused("clip", clip=clip)
    for wg in (-1, L.PPO_GRAD_MAX_WG + 1):
        refused("workgroups", workgroups=wg)
    words = L.policy_words(0)
    good = dict(grad=torch.zeros(words), stats=torch.zeros(8), logp=torch.zeros(Rs), scratch=torch.zeros(1, words + 8))
    refused("out", out=[good["grad"]])
    refused("out", out=dict(good, values=good["grad"]))
    refused(r"out\['grad'\]", out=dict(good, grad=torch.zeros(words + 1)))
    refused(r"out\['stats'\]", out=dict(good, stats=torch.zeros(8, dtype=torch.float64)))
    refused(r"out\['logp'\]", out=dict(good, logp=torch.zeros(Rs + 1)))
    refused(r"out\['logp'\]", out=dict(good, logp=torch.zeros(5)), index=torch.zeros(4, dtype=torch.int32))
    refused(r"out\['scratch'\]", out=dict(good, scratch=torch.zeros(2, words + 8)))      # (12 rows are one tile: G = 1)
    refused(r"out\['scratch'\]", out=dict(good), workgroups=3)
    with pytest.raises(AssertionError, match="the library was called"):      # ... and a call that passes them all goes to the library
        AtcVecEnv.ppo_policy_grad(env, **ok, out=good)


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatement
def _torch_grad(case):
    """(grad, stats[:6], logp) of the contract through torch.autograd in float64, the loss written with torch.minimum / torch.clamp"""
    import torch
    K = int(case["K"])
    parts = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in P.split(case["w"], K).items()}
    src, part = PG._select(case)
    rows = torch.tensor(PG.input_rows(case["obs_rows"], case.get("traffic"), K)[src][part].astype(np.float64))
    u = torch.tensor(np.asarray(case["action"], np.float64).reshape(-1, 3)[src][part])
    lp_old = torch.tensor(np.asarray(case["logp_old"], np.float64).reshape(-1)[src][part])
    adv = torch.tensor(np.asarray(case["adv"], np.float64).reshape(-1)[src][part])
    clip, shift, scale = (float(np.float32(case[k])) for k in ("clip", "adv_shift", "adv_scale"))
    h1 = torch.tanh(rows @ parts["W1"].T + parts["b1"])
    h2 = torch.tanh(h1 @ parts["W2"].T + parts["b2"])
    mu = h2 @ parts["W3"].T + parts["b3"]
    d = (u - mu) / torch.exp(parts["log_std"])
    logp = (-0.5 * d * d - parts["log_std"]).sum(-1) - P.LOGP_C
    ratio = torch.exp(logp - lp_old)
    A = (adv - shift) * scale
    loss = -torch.minimum(ratio * A, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * A)
    n = int(part.sum())
    loss.sum().div(n).backward()
    grad = np.concatenate([parts[name].grad.numpy().reshape(-1) for name in PG.PART_NAMES])
    stats = [n] + [float(v.detach()) for v in (loss.mean(), (lp_old - logp).mean(), ratio.sum() * 0, ratio.mean(), (logp - lp_old).abs().max())]
    return grad, stats, logp.detach().numpy()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mask,index", ((False, False), (True, False), (False, True), (True, True)))
def test_float64_restatement_equals_torch_autograd(K, mask, index):
    case = PG.make_case(100 + K, 150, K=K, gain=1.0, log_std=-0.5, raw=False, mask=mask, index=index)
    if not index:      # a row with A exactly 0: adv equal to the shift
        case["adv"][3] = np.float32(case["adv_shift"])
        if mask:
            case["mask"][3] = 1
    ref = PG.evaluate(case, np.float64)
    if not index:
        assert ref["A"][3] == 0.0 and ref["part"][3]
    grad, stats, logp = _torch_grad(case)
    assert ref["n_cut"] > 0 and 0 < ref["n"] < 150 or not (mask or index)
    g_ref, g_t = PG.parts(ref["grad"], K), PG.parts(grad, K)
    for name in PG.PART_NAMES:
        top = np.max(np.abs(g_t[name]))
        assert top > 0 and np.max(np.abs(g_ref[name] - g_t[name])) <= 1e-10 * top, (name, np.max(np.abs(g_ref[name] - g_t[name])), top)
    for q in (PG.STAT_N, PG.STAT_LOSS, PG.STAT_KL, PG.STAT_RATIO, PG.STAT_DLOGP_MAX):
        assert abs(ref["stats"][q] - stats[q]) <= 1e-10 * max(1.0, abs(stats[q])), q
    assert ref["stats"][PG.STAT_CUT] == ref["n_cut"] / ref["n"] and np.all(ref["stats"][6:] == 0)
    assert np.max(np.abs(ref["logp"][ref["part"]] - logp)) <= 1e-10 * np.max(np.abs(logp))
    assert np.all(np.isnan(ref["logp"][~ref["part"]]))


def test_surrogate_on_a_clip_boundary_and_at_zero_advantage():
    """ratio exactly 1 - clip and 1 + clip, both signs of A, and A = 0: the restatement's rule equals what torch.minimum plus torch.clamp
    autograd yields (boundaries inclusive; minimum splits a tie in halves, clamp passes its bounds)"""
    import torch
    clip = float(np.float32(0.25))      # 0.75 and 1.25 are exact
    ratio = np.array([0.75, 1.25, 0.75, 1.25, 1.0, 0.5, 2.0, 0.75, 1.25, np.nextafter(1.25, 2), np.nextafter(0.75, 0), np.nextafter(1.25, 2), np.nextafter(0.75, 0)])
    A = np.array([1.5, 1.5, -1.5, -1.5, 0.0, 0.0, 0.0, 0.0, -0.0, 1.5, -1.5, -1.5, 1.5])
    loss, flows = PG.surrogate(ratio, A, clip)
    r = torch.tensor(ratio, requires_grad=True)
    lt = -torch.minimum(r * torch.tensor(A), torch.clamp(r, 1.0 - clip, 1.0 + clip) * torch.tensor(A))
    lt.sum().backward()
    assert np.array_equal(loss, lt.detach().numpy())
    assert np.array_equal(np.where(flows, -A, 0.0), r.grad.numpy())
    assert list(flows[:4]) == [True] * 4 and list(flows[9:]) == [False, False, True, True]


# the GPU cases: (seed, R, G, K, gain, log_std, raw, mask, index)
CASES = ((1, 1, 1, 0, 1.0, 0.0, False, False, False), (2, 63, 2, 1, 8.0, -2.0, False, True, False), (3, 64, 1, 2, 1.0, -2.0, True, False, True),
         (4, 65, 3, 4, 1.0, 0.0, False, True, True), (5, 300, 1, 0, 8.0, 0.0, True, True, True), (6, 300, 3, 4, 8.0, -2.0, True, True, True),
         (7, 300, 2, 2, 1.0, 0.0, False, False, False), (8, 300, 3, 1, 1.0, -2.0, True, True, False), (9, 65, 2, 0, 1.0, -2.0, False, False, True),
         (10, 300, 3, 0, 1.0, 0.0, False, True, True), (11, 64, 3, 1, 1.0, 0.0, False, False, False))
_ids = ["R%d-G%d-K%d-gain%g-ls%g%s%s%s" % (c[1:6] + ("-raw" if c[6] else "", "-mask" if c[7] else "", "-index" if c[8] else "")) for c in CASES]
_cases = pytest.mark.parametrize("case_id", range(len(CASES)), ids=_ids)


@functools.lru_cache(maxsize=None)
def _case(case_id):
    """the case, its float64 restatement, its float32 twin and the bars: computed once, shared, never written to"""
    seed, R, G, K, gain, ls, raw, mask, index = CASES[case_id]
    case = PG.make_case(seed, R, K=K, gain=gain, log_std=ls, raw=raw, mask=mask, index=index)
    ref64, ref32 = PG.evaluate(case, np.float64), PG.evaluate(case, np.float32)
    return case, ref64, ref32, PG.bars(case, ref64, ref32), G


def test_the_cases_cover_what_they_claim():
    assert {c[1] for c in CASES} == {1, 63, 64, 65, 300} and {c[2] for c in CASES} == {1, 2, 3} and {c[3] for c in CASES} == set(KS)
    assert {c[4] for c in CASES} == {1.0, 8.0} and {c[5] for c in CASES} == {0.0, -2.0} and {c[6] for c in CASES} == {False, True}
    cut_hi = cut_lo = masked = out_of_range = wide = repeated = 0
    for i, c in enumerate(CASES):
        case, ref64, ref32, bars, G = _case(i)
        near, flat = PG.margins(case, ref64)
        assert near >= PG.RATIO_MARGIN and flat >= PG.ADV_MARGIN, (c, near, flat)      # no row may fall on the other side in float32: none is excused
        assert np.array_equal(ref64["part"], ref32["part"]) and np.array_equal(ref64["cut"], ref32["cut"]), c
        r = ref64["ratio"][ref64["part"]]
        if r.size > 50:
            assert r.min() < 0.6 and r.max() > 1.7, (c, r.min(), r.max())      # the ratios spread over [0.5, 2]
        cut_hi += int((ref64["cut"] & (ref64["ratio"] > 1.2)).sum())
        cut_lo += int((ref64["cut"] & (ref64["ratio"] < 0.8)).sum())
        src, part = PG._select(case)
        if case["mask"] is not None:
            masked += int((case["mask"] == 0).sum())
        if case["index"] is not None:
            idx = case["index"].astype(np.int64)
            out_of_range += int(((idx < 0) | (idx >= case["R_src"])).sum())
            repeated += int(len(idx) - len(np.unique(idx)))
        x = PG.input_rows(case["obs_rows"], case["traffic"], case["K"])[src][part]
        wide += int((np.abs(x).max(axis=1) > 4.0).sum()) if x.size else 0
        assert not c[6] or np.abs(x).max() > 1e4, c      # raw rows carry 1.5e4-magnitude words
    assert min(cut_hi, cut_lo, masked, out_of_range, wide, repeated) > 0, (cut_hi, cut_lo, masked, out_of_range, wide, repeated)
    # partial tiles, a workgroup that loops (tiles > G) and workgroups with unequal loads (tiles % G != 0)
    assert any(c[1] % 64 for c in CASES) and any(-(-c[1] // 64) > c[2] for c in CASES) and any(-(-c[1] // 64) % c[2] for c in CASES if c[2] > 1)


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _env():
    return H.policy_env(dict(normalize=True, shaping=True, auto_reset=True, timestep_limit=7, spawn="lattice"), 2, 1)


def _dev(case, env):
    import torch
    t = lambda v: None if v is None else torch.as_tensor(np.ascontiguousarray(v), device=env.device)      # noqa: E731
    return dict(weights=t(case["w"]), obs_rows=t(case["obs_rows"]), action=t(case["action"]), logp_old=t(case["logp_old"]), adv=t(case["adv"]),
                traffic=t(case["traffic"]), mask=t(case["mask"]), index=t(case["index"]))


def _call_gpu(env, case, G, dev=None, out=None):
    d = _dev(case, env) if dev is None else dev
    pos = [d[k] for k in ("weights", "obs_rows", "action", "logp_old", "adv")]
    res = env.ppo_policy_grad(*pos, traffic=d["traffic"], mask=d["mask"], index=d["index"], clip=case["clip"], adv_shift=case["adv_shift"],
                              adv_scale=case["adv_scale"], workgroups=G, out=out)
    env.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _hold(got, ref64, bars, K, tag):
    """every part of grad, stats and logp within its bar of the float64 restatement; n and the cut count exact.  Prints deviation / bar."""
    worst = {}
    g, r = PG.parts(got["grad"].astype(np.float64), K), PG.parts(ref64["grad"], K)
    for name in PG.PART_NAMES:
        worst[name] = float(np.max(np.abs(g[name] - r[name]))) / bars[name][0] if bars[name][0] > 0 else 0.0
    n = ref64["n"]
    assert got["stats"][PG.STAT_N] == n and np.all(got["stats"][6:] == 0), (tag, got["stats"])
    if n:
        assert round(float(got["stats"][PG.STAT_CUT]) * n) == ref64["n_cut"] and abs(got["stats"][PG.STAT_CUT] - ref64["n_cut"] / n) <= 1e-6, (tag, got["stats"], ref64["n_cut"])
        for name, sel, bar in (("stats", [PG.STAT_LOSS, PG.STAT_RATIO], bars["stats"][0]), ("kl and max |dlogp|", list(PG.STATS_OF_LOGP), bars["logp"][0])):
            worst[name] = float(np.max(np.abs(got["stats"][sel].astype(np.float64) - ref64["stats"][sel]))) / bar
        part = ref64["part"]
        worst["logp"] = float(np.max(np.abs(got["logp"][part].astype(np.float64) - ref64["logp"][part]))) / bars["logp"][0]
    print("%s: kernel deviation / bar: %s" % (tag, ", ".join("%s %.3f" % kv for kv in worst.items())))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad, {k: bars[k] for k in bad})
    return worst


@pytest.mark.gpu
@_cases
def test_grad_stats_and_logp_within_the_twin_bars(case_id):
    import torch
    case, ref64, ref32, bars, G = _case(case_id)
    env = _env()
    from atc_hip import lib
    before = lib.ppo_policy_grad_launch_counts().get(case["K"], 0)
    others = {k: v for k, v in lib.launch_records().items() if k != "atc_ppo_policy_grad_launch_counts"}
    d = _dev(case, env)
    words = L.policy_words(case["K"])
    out = dict(grad=torch.full((words,), SENTINEL, device=env.device), stats=torch.full((8,), SENTINEL, device=env.device),
               logp=torch.full((case["R"],), SENTINEL, device=env.device), scratch=torch.full((G, words + 8), SENTINEL, device=env.device))
    got = _call_gpu(env, case, G, d, out)
    assert lib.ppo_policy_grad_launch_counts().get(case["K"], 0) == before + 1
    assert {k: v for k, v in lib.launch_records().items() if k != "atc_ppo_policy_grad_launch_counts"} == others
    _hold(got, ref64, bars, case["K"], _ids[case_id])
    assert np.all(got["logp"][~ref64["part"]] == np.float32(SENTINEL)), "a row that takes no part had its logp written"
    assert not np.any(got["logp"][ref64["part"]] == np.float32(SENTINEL))
    # the same inputs and the same G: the same bits
    again = _call_gpu(env, case, G, d, out)
    for k in ("grad", "stats", "logp"):
        assert _same(got[k], again[k]), k
    # without out=, and with the library's own G
    free = _call_gpu(env, case, 0, d)
    assert np.all(np.isnan(free["logp"][~ref64["part"]]))
    if L.ppo_grad_workgroups(case["R"]) == G:
        assert _same(free["grad"], got["grad"]) and _same(free["stats"], got["stats"])
    _hold(free, ref64, bars, case["K"], _ids[case_id] + " (G = 0)")


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", (4, 5, 7), ids=lambda i: _ids[i])
def test_one_workgroup_and_three_agree_within_the_bars(case_id):
    case, ref64, ref32, bars, _ = _case(case_id)
    env = _env()
    d = _dev(case, env)
    one, three = _call_gpu(env, case, 1, d), _call_gpu(env, case, 3, d)
    _hold(one, ref64, bars, case["K"], _ids[case_id] + " G=1")
    _hold(three, ref64, bars, case["K"], _ids[case_id] + " G=3")
    assert _same(one["logp"], three["logp"]) and one["stats"][0] == three["stats"][0] and one["stats"][3] == three["stats"][3]
    a, b = PG.parts(one["grad"].astype(np.float64), case["K"]), PG.parts(three["grad"].astype(np.float64), case["K"])
    for name in PG.PART_NAMES:
        assert np.max(np.abs(a[name] - b[name])) <= 2.0 * bars[name][0], name      # (each is within one bar of the restatement)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", (3, 5), ids=lambda i: _ids[i])
def test_nans_in_rows_that_take_no_part_change_no_bit(case_id):
    case, ref64, ref32, bars, G = _case(case_id)
    env = _env()
    clean = _call_gpu(env, case, G)
    src, part = PG._select(case)
    used = np.zeros(case["R_src"], bool)
    used[src[part]] = True
    assert (~used).sum() > 0
    dirty = dict(case)
    for k in ("obs_rows", "action", "logp_old", "adv", "traffic"):
        if case[k] is not None:
            v = case[k].copy()
            v[~used] = np.nan
            dirty[k] = v
    got = _call_gpu(env, dirty, G)
    for k in ("grad", "stats"):
        assert _same(clean[k], got[k]), k
    assert _same(clean["logp"][ref64["part"]], got["logp"][ref64["part"]]) and np.all(np.isnan(got["logp"][~ref64["part"]]))


@pytest.mark.gpu
def test_a_mask_of_zeros_and_indices_all_out_of_range():
    import torch
    case, ref64, ref32, bars, G = _case(9)
    env = _env()
    none = dict(case, mask=np.zeros(case["R_src"], np.uint8))
    for c in (none, dict(case, index=np.full(case["R"], case["R_src"], np.int32)), dict(case, index=np.full(case["R"], -5, np.int32))):
        d = _dev(c, env)
        out = dict(logp=torch.full((case["R"],), SENTINEL, device=env.device))
        got = _call_gpu(env, c, G, d, out)
        assert np.all(got["grad"] == 0) and np.all(got["stats"] == 0) and got["grad"].shape == (L.policy_words(case["K"]),)
        assert np.all(got["logp"] == np.float32(SENTINEL))


@pytest.mark.gpu
def test_out_with_all_four_buffers_allocates_nothing():
    import torch
    case, ref64, ref32, bars, G = _case(5)
    env = _env()
    d = _dev(case, env)
    words = L.policy_words(case["K"])
    out = dict(grad=torch.empty(words, device=env.device), stats=torch.empty(8, device=env.device), logp=torch.empty(case["R"], device=env.device),
               scratch=torch.empty((G, words + 8), device=env.device))
    pos = [d[k] for k in ("weights", "obs_rows", "action", "logp_old", "adv")]
    kw = dict(traffic=d["traffic"], mask=d["mask"], index=d["index"], clip=case["clip"], adv_shift=case["adv_shift"], adv_scale=case["adv_scale"], workgroups=G, out=out)
    env.ppo_policy_grad(*pos, **kw)
    env.synchronize()
    torch.cuda.reset_peak_memory_stats(env.device)
    before = torch.cuda.memory_allocated(env.device)
    res = env.ppo_policy_grad(*pos, **kw)
    env.synchronize()
    assert torch.cuda.memory_allocated(env.device) == before and torch.cuda.max_memory_allocated(env.device) == before
    assert res["grad"] is out["grad"] and res["stats"] is out["stats"] and res["logp"] is out["logp"] and "scratch" not in res


@pytest.mark.gpu
def test_refusals_that_need_a_device():
    import torch
    case, ref64, ref32, bars, G = _case(5)      # K = 4, with a mask and an index
    env = _env()
    d = _dev(case, env)
    pos = [d[k] for k in ("weights", "obs_rows", "action", "logp_old", "adv")]
    kw = dict(traffic=d["traffic"], mask=d["mask"], index=d["index"])
    before = _records()
    with pytest.raises(ValueError, match="weights"):
        env.ppo_policy_grad(d["weights"].cpu(), *pos[1:], **kw)
    with pytest.raises(ValueError, match="mask"):
        env.ppo_policy_grad(*pos, **dict(kw, mask=d["mask"].cpu()))
    with pytest.raises(ValueError, match="weights"):      # the rows say K = 4, the array K = 0
        env.ppo_policy_grad(d["weights"][:L.policy_words(0)].contiguous(), *pos[1:], **kw)
    words = L.policy_words(case["K"])
    big = torch.zeros(words + 8 + case["R"], device=env.device)
    for out, a, b in ((dict(grad=d["weights"]), "w", "grad"), (dict(logp=d["adv"][:case["R"]]), "adv", "logp_new"),
                      (dict(grad=big[:words], stats=big[words - 1:words + 7]), "grad", "stats"), (dict(stats=big[:8], logp=big[7:7 + case["R"]]), "stats", "logp_new")):
        with pytest.raises(RuntimeError, match="%s overlaps %s" % (a, b)):
            env.ppo_policy_grad(*pos, **kw, out=out)
    env.synchronize()
    assert _records() == before


E2E = ((7, 5, 1), (7, 5, 3), (40, 16, 1), (40, 16, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,hold", E2E, ids=["%dx%d-hold%d" % c for c in E2E])
@pytest.mark.parametrize("K", (0, 2))
def test_end_to_end_behind_the_collection_with_the_same_weights(B, N, hold, K):
    """rollout_policy_ends -> gae_boot -> ppo.policy_grad with the SAME weights (a time limit of 7 ends episodes inside blocks): no row is
    cut, grad within the bars of the restatement, and logp agrees with the stored one as closely as the restatement itself does"""
    import torch
    from atc_hip import ppo
    env = H.policy_env(dict(normalize=True, shaping=True, auto_reset=True, timestep_limit=7, spawn="lattice"), B, N)
    D = 8 if hold == 1 else 4      # (T = 8 and 12 steps against a limit of 7)
    T = D * hold
    w = torch.as_tensor(P.random_weights(np.random.default_rng([23, K]), 1.0, (-0.5, -1.0, 0.25), False, K), device=env.device)
    obs0 = env.obs.clone()
    out = env.rollout_policy_ends(w, T, K, hold=hold, seed=99, decision0=7, obs0=obs0)
    rows = ppo.value_rows(env, out, obs0, hold=hold)
    critic = lambda x: torch.tanh(x.sum(-1) * 0.05)      # noqa: E731
    values, boot = critic(rows).contiguous(), critic(out["term_obs"]).contiguous()
    g = env.gae_boot(out["reward"], out["done"], values, boot, ppo.truncated(out["term_flags"]), hold=hold, gamma=0.99, lam=0.95)
    col = dict(out, obs0=obs0, **g)
    got = ppo.policy_grad(env, col, w, clip=0.2, normalise=True)
    env.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    control = out["control"].cpu().numpy().reshape(-1)
    done = out["done"].cpu().numpy().reshape(D, hold, B)
    assert done.any() and (hold == 1 or done[:, :-1].any()), "no episode ended (inside a block)"
    assert 0 < control.sum()
    adv = g["adv"].cpu().numpy().reshape(-1).astype(np.float64)
    sel = adv[control != 0]
    case = dict(K=K, w=w.cpu().numpy(), obs_rows=rows[:-1].cpu().numpy().reshape(-1, 10), traffic=out["traffic"].cpu().numpy().reshape(-1, K, 8) if K else None,
                action=out["action"].cpu().numpy().reshape(-1, 3), logp_old=out["logp"].cpu().numpy().reshape(-1), adv=g["adv"].cpu().numpy().reshape(-1), clip=0.2,
                mask=control, index=None, R=D * B * N, R_src=D * B * N)
    a_t = g["adv"][out["control"].bool()]      # the two scalars as ppo.policy_grad computes them
    case["adv_shift"], case["adv_scale"] = float(a_t.mean()), float(1.0 / (a_t.std() + 1e-8))
    assert abs(case["adv_shift"] - sel.mean()) <= 1e-5 * max(1.0, abs(sel.mean()))
    ref64, ref32 = PG.evaluate(case, np.float64), PG.evaluate(case, np.float32)
    bars = PG.bars(case, ref64, ref32)
    assert ref64["n"] == int((control != 0).sum()) and ref64["n_cut"] == 0
    assert got["stats"][PG.STAT_CUT] == 0.0
    _hold(got, ref64, bars, K, "end to end %dx%d hold %d K %d" % (B, N, hold, K))
    part = ref64["part"]
    stored = case["logp_old"][part].astype(np.float64)
    own_gap = float(np.max(np.abs(ref64["logp"][part] - stored)))
    gap = float(np.max(np.abs(got["logp"][part].astype(np.float64) - stored)))
    print("|logp_new - stored logp| = %.3e; the float64 restatement's own gap %.3e (+ LOGP_BAR %.1e)" % (gap, own_gap, P.LOGP_BAR))
    assert gap <= own_gap + P.LOGP_BAR
    assert np.all(np.isnan(got["logp"][~part]))
    env.close()


@pytest.mark.gpu
def test_policy_grad_on_the_dict_collect_bootstrap_returns():
    import torch
    from atc_hip import ppo
    B, N, hold, D = 7, 5, 3, 4
    env = H.policy_env(dict(normalize=True, shaping=True, auto_reset=True, timestep_limit=7, spawn="lattice"), B, N)
    w = torch.as_tensor(P.random_weights(np.random.default_rng(31), 1.0, (-0.5, -1.0, 0.25)), device=env.device)
    obs0 = env.obs.clone()
    res = ppo.collect_bootstrap(env, w, lambda x: torch.tanh(x.sum(-1) * 0.05), D * hold, hold=hold, seed=5)
    assert "obs0" not in res
    got = ppo.policy_grad(env, res, w)                                  # the row of decision 0: the copy the collection kept
    by_hand = ppo.policy_grad(env, dict(res, obs0=obs0), w)
    mb = torch.randperm(D * B * N, device=env.device).to(torch.int32)[:100].contiguous()
    part = ppo.policy_grad(env, res, w, index=mb, normalise=False)
    env.synchronize()
    for k in ("grad", "stats", "logp"):
        assert torch.equal(got[k].view(torch.int32), by_hand[k].view(torch.int32)), k
    n = int(res["control"].sum())
    assert got["stats"][0] == n and got["stats"][3] == 0 and float(got["grad"].abs().max()) > 0
    assert part["stats"][0] == int(res["control"].reshape(-1)[mb.long()].sum()) and part["logp"].shape == (100,)
    with pytest.raises(ValueError, match="obs0"):
        ppo.policy_grad(env, {k: v.clone() for k, v in res.items()}, w)
    env.close()
