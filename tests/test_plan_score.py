"""Scoring and ranking of drawn plans (include/atc_step.h: atc_plan_score; AtcVecEnv.score_plans; atc_hip/cem.py: cem_plan_scored,
mppi_plan_scored): the discounted score, the strict total order, the refit weights and the best R candidate numbers in one launch.

CPU: the exports and the kernel symbol; the constants and the argtypes across the header, atc_hip/layout.py and atc_hip/lib.py; the
whole refusal order through ctypes with NULL and made-up pointers; the launch record; tests/plan_score_ref.py (the numpy restatement)
against a plain scalar loop written from the header's text, on ties, +-0, NaN / +-Inf rewards, n_steps zeros, an env with no valid
candidate and elites beyond the number of valid candidates.
GPU: every word of score, of the ELITE weight and of top BIT-IDENTICAL to the restatement over B x M x H with the elites, R, gamma and
five score families rotating through the cases, into pattern-filled buffers with guard rows; n_steps=None against all-ones; the SOFTMAX
weight within SOFTMAX_ULP_BAR of float32(exp(float64(x))), x restated exactly; refusals, touching ranges, out=, the launch records and
the env state; cem_plan_scored and mppi_plan_scored against the same loops written with the restatements; an env that is not evaluated.

THE SOFTMAX BAR.  No file of the ROCm installation documents an ulp bound for the device library's expf (none under its share/doc or
among its markdown / text files speaks of one), so the bar follows the other rule: the largest ulp distance measured over this file's own
softmax inputs in one device run — printed by test_softmax_weight_within_the_bar before it asserts — was MEASURED_MAX_ULP, and the bar
is twice that.  Weights whose reference is below FLT_MIN are compared by absolute difference <= FLT_MIN; the best candidate's weight
must be exactly 1."""
import ctypes as C
import functools
import inspect
import re
import shutil
import subprocess

import numpy as np
import pytest

import held_tools as T
import helpers as H
import plan_draw_ref as P
import plan_refit_ref as R
import plan_score_ref as S
from atc_hip import layout as L
from held_tools import GUARD, HEADER, LIB

NAMES = ("atc_plan_score", "atc_plan_score_launch_counts")
FAKE = C.c_void_p(0x100000)     # a made-up pointer: a call that is refused never follows it
PATTERN = 0xA5                  # the byte output buffers hold before a call
MEASURED_MAX_ULP = S.MEASURED_MAX_ULP        # largest distance seen over this file's softmax inputs on an MI355X
SOFTMAX_ULP_BAR = S.SOFTMAX_ULP_BAR          # (both kept in tests/plan_score_ref.py, where tests/planner_ref.py takes the same bar from)


# ---------------------------------------------------------------------------------------------------------------- CPU: the ABI
def test_exports_and_kernel_symbol():
    from atc_hip import lib
    assert set(NAMES) <= set(lib.EXPORTS)
    h = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bk_plan_score\(", text)


def test_header_constants_struct_and_argtypes():
    from atc_hip import lib
    text = open(HEADER).read()
    assert L.SCORE_MAX_TOP == int(re.search(r"#define ATC_SCORE_MAX_TOP (\d+)", text).group(1)) == 64
    assert L.PLAN_SCORE_LAUNCH_SLOTS == int(re.search(r"ATC_PLAN_SCORE_LAUNCH_SLOTS = (\d+)", text).group(1)) == 1
    assert (L.SCORE_ELITE, L.SCORE_SOFTMAX) == (int(re.search(r"ATC_SCORE_ELITE = (\d+)", text).group(1)),
                                                int(re.search(r"ATC_SCORE_SOFTMAX = (\d+)", text).group(1))) == (0, 1)
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22
    body = re.search(r"typedef struct atc_plan_score \{(.*?)\} atc_plan_score_t;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.split() for d in body.split(";") if d.strip()]
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "float": C.c_float}
    assert [(f[1], ctype[f[0]]) for f in fields] == list(lib.AtcPlanScore._fields_)
    assert [f[1] for f in fields] == list(lib.PLAN_SCORE_FIELDS) and C.sizeof(lib.AtcPlanScore) == 16
    decl = re.search(r"^int atc_plan_score\((.*?)\);", text, flags=re.S | re.M).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "B", "H", "M", "seg_reward", "n_steps", "sc", "score", "weight", "top", "R", "stream"]
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    want = [ci if a.startswith("int ") else C.POINTER(lib.AtcPlanScore) if "atc_plan_score_t" in a else vp for a in args]
    assert list(h.atc_plan_score.argtypes) == want
    assert h.atc_plan_score.restype is ci and h.atc_plan_score_launch_counts.restype is ci
    assert list(h.atc_plan_score_launch_counts.argtypes) == [C.POINTER(C.c_uint64), ci]
    assert callable(lib.plan_score_launch_counts)


# every launch record of the library (helpers.launch_records), the ones this module indexes first
_records = functools.partial(H.launch_records, "plan_score", "plan_refit", "plan_sampled", "plan_draw")


ARGS = ("s", "seg_reward", "sc", "score", "weight")      # the pointers that may not be NULL, in the order they are looked at


def _score_call(h):
    def call(Hn, M, R=0, B=1, n_steps=None, top=None, **kw):
        a = dict.fromkeys(ARGS)
        a.update(kw)
        return h.atc_plan_score(a["s"], B, Hn, M, a["seg_reward"], n_steps, a["sc"], a["score"], a["weight"], top, R, None)
    return call


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    at = lambda k: C.c_void_p(0x100000 + k * 0x1000000)     # noqa: E731  (made-up ranges 16 MiB apart: no overlap at these shapes)
    elite, soft = lib.AtcPlanScore(L.SCORE_ELITE, 1, 0.5, 0.0), lib.AtcPlanScore(L.SCORE_SOFTMAX, 0, 0.5, 2.0)
    ok = dict(s=FAKE, seg_reward=at(1), sc=C.byref(elite), score=at(2), weight=at(3))
    call, err = _score_call(h), h.atc_last_error
    # 1. H, 2. M, 3. R: before any pointer is looked at
    for Hn in (0, 17, -1):
        for M in (0, 1, 1025):
            assert call(Hn, M, R=99) == -1 and b"H (" in err() and b"16" in err()
    for M in (0, 1025, -1, 1 << 20):
        assert call(16, M, R=99) == -1 and b"M (" in err() and b"1024" in err()
    for Rn in (-1, 65, 1 << 20):
        assert call(1, 1, R=Rn) == -1 and b"R (" in err() and b"64" in err()
    assert call(1, 1, R=1) == -1 and b"R (" in err() and b"top" in err()
    assert call(1, 1, R=64, **ok) == -1 and b"R (" in err() and b"top" in err()
    for M, Rn in ((1, 0), (65, 0), (1024, 64)):        # accepted as far as the first pointer check (R > M included)
        assert call(1, M, R=Rn, top=at(4)) == -1 and b"null pointer: s" in err()
    # 4. the pointers, in their order: with every earlier one given and every later one NULL, the first NULL is the one named
    for j, name in enumerate(ARGS):
        named = re.compile(rb"null pointer: %s\b" % name.encode())      # (\b: "s" is not "seg_reward", "sc" or "score")
        assert call(1, 1, **{k: ok[k] for k in ARGS[:j]}) == -1 and named.search(err()), (name, err())
        assert call(1, 1, **dict(ok, **{name: None})) == -1 and named.search(err()), (name, err())
    # 5. mode, 6. elites, 7. gamma, 8. temperature, 9. B — each with every later item wrong as well
    bad_later = dict(B=0)
    sc = lib.AtcPlanScore(2, 0, np.nan, -1.0)
    assert call(1, 4, **dict(ok, sc=C.byref(sc)), **bad_later) == -1 and b"mode" in err()
    for E in (0, 5, -1):
        sc = lib.AtcPlanScore(L.SCORE_ELITE, E, np.inf, 0.0)
        assert call(1, 4, **dict(ok, sc=C.byref(sc)), **bad_later) == -1 and b"elites" in err()
    sc = lib.AtcPlanScore(L.SCORE_SOFTMAX, 0, 0.5, 1.0)      # (elites is not looked at in SOFTMAX mode)
    assert call(1, 4, **dict(ok, sc=C.byref(sc)), **bad_later) == -1 and b"B >= 1" in err()
    for g in (np.nan, np.inf, -np.inf):
        for mode in (L.SCORE_ELITE, L.SCORE_SOFTMAX):
            sc = lib.AtcPlanScore(mode, 1, g, -1.0)
            assert call(1, 4, **dict(ok, sc=C.byref(sc)), **bad_later) == -1 and b"gamma" in err()
    for temp in (0.0, -0.0, -1.0, np.nan, np.inf):
        sc = lib.AtcPlanScore(L.SCORE_SOFTMAX, 0, 0.5, temp)
        assert call(1, 4, **dict(ok, sc=C.byref(sc)), **bad_later) == -1 and b"temperature" in err()
    sc = lib.AtcPlanScore(L.SCORE_ELITE, 4, -0.5, np.nan)      # (temperature is not looked at in ELITE mode)
    assert call(1, 4, **dict(ok, sc=C.byref(sc)), **bad_later) == -1 and b"B >= 1" in err()
    for B in (0, -3):       # B before the overlap rule
        assert call(1, 4, B=B, **dict(ok, weight=ok["score"])) == -1 and b"B >= 1" in err()
    # 10. the overlap rule (pointer values only), every pair once: equal pointers, then the last / first word shared
    Hn, M, B, Rn = 2, 4, 3, 5
    size = dict(seg_reward=M * Hn * B * 4, n_steps=M * B * 2, score=M * B * 4, weight=M * B * 4, top=Rn * B * 4)
    base = dict(ok, n_steps=at(5), top=at(6), sc=C.byref(soft))
    names = list(size)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for off in (0, size[a] - 2, -(size[b] - 2)):
                kw = dict(base, **{b: C.c_void_p(base[a].value + off)})
                assert call(Hn, M, R=Rn, B=B, **kw) == -1 and b"overlaps" in err() and a.encode() in err() and b.encode() in err(), (a, b, off)
    # top's range is not looked at with R == 0, n_steps' not when it is NULL
    assert call(Hn, M, R=0, B=0, **dict(base, top=base["score"])) == -1 and b"B >= 1" in err()
    assert _records() == before, "a refused call moved a launch record"


def test_launch_record_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    buf = (C.c_uint64 * 8)(*([99] * 8))
    assert h.atc_plan_score_launch_counts(buf, 8) == 0
    assert buf[0] != 99 and all(v == 99 for v in buf[1:])
    assert h.atc_plan_score_launch_counts(None, 1) == -1
    assert isinstance(lib.plan_score_launch_counts(), dict)


def test_python_surface():
    from atc_hip import cem
    from atc_hip.vec_env import AtcVecEnv
    sig = inspect.signature(AtcVecEnv.score_plans)
    assert list(sig.parameters) == ["self", "seg_reward", "n_steps", "mode", "elites", "temperature", "gamma", "top", "out"]
    assert [sig.parameters[k].default for k in ("n_steps", "mode", "elites", "temperature", "gamma", "top", "out")] == [None, "elite", None, None, 1.0, 1, None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("mode", "elites", "temperature", "gamma", "top", "out"))
    sig = inspect.signature(cem.cem_plan_scored)
    assert list(sig.parameters) == list(inspect.signature(cem.cem_plan).parameters)
    assert [sig.parameters[k].default for k in ("gamma", "seed")] == [1.0, 0]
    assert list(inspect.signature(cem.mppi_plan_scored).parameters) == list(inspect.signature(cem.mppi_plan).parameters)
    for f in (cem.cem_plan_scored, cem.mppi_plan_scored):
        for word in ("NOT EVALUATED", "LOWER candidate number", "running product"):
            assert word in f.__doc__, (f.__name__, word)


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatement
def _scalar(seg, n_steps, mode, elites, temperature, gamma, top):
    """the header's text as a plain loop on numpy float32 scalars, one env at a time, the order by repeated selection of the best
    remaining candidate (no sort)"""
    f = np.float32
    M, Hn, B = seg.shape
    score = np.zeros((M, B), f)
    weight = np.zeros((M, B), np.float64)
    tp = np.full((top, B), -1, np.int32)
    with np.errstate(all="ignore"):
        for e in range(B):
            ok = []
            for m in range(M):
                s, g = f(seg[m, 0, e]), f(1.0)
                for h in range(1, Hn):
                    g = f(g * f(gamma))
                    s = f(s + f(f(seg[m, h, e]) * g))
                score[m, e] = s if s == s else S.QUIET_NAN
                if (n_steps is None or n_steps[m, e] != 0) and abs(s) <= S.FLT_MAX:
                    ok.append(m)
            ranked = []
            while ok:
                best = ok[0]
                for m in ok[1:]:
                    if score[m, e] > score[best, e]:       # (strictly: an equal score stays behind the lower number; -0 > +0 is False)
                        best = m
                ranked.append(best)
                ok.remove(best)
            for r, m in enumerate(ranked[:top]):
                tp[r, e] = m
            for pos, m in enumerate(ranked):
                if mode == "elite":
                    weight[m, e] = 1.0 if pos < elites else 0.0
                else:
                    x = f(f(score[m, e] - score[ranked[0], e]) / f(temperature))
                    weight[m, e] = np.exp(np.float64(x))
    return score, weight, tp


def _hard_seg(rng, M, Hn, B):
    """[M, H, B] float32 and n_steps [M, B]: a few distinct values so that most candidates tie, +-0, NaN / +-Inf rewards, n_steps zeros,
    env 1 (B > 1) without a valid candidate, env 2 (B > 2) with all candidates equal"""
    seg = rng.choice(np.array([-2.0, -1.0, 0.0, -0.0, 1.0], np.float32), (M, Hn, B))
    hit = rng.uniform(size=seg.shape) < 0.06
    seg[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(hit.sum()))
    n_steps = rng.integers(0, 4, (M, B)).astype(np.uint16)
    if B > 1:
        n_steps[: M // 2, 1] = 0
        seg[M // 2:, 0, 1] = np.nan
    if B > 2:
        seg[:, :, 2] = -0.0
        seg[::2, 0, 2] = 0.0
        n_steps[:, 2] = 3
    return seg, n_steps


def test_restatement_equals_a_scalar_loop():
    rng = np.random.default_rng(41)
    seen_short = seen_tie = False
    for M, Hn, B in ((1, 1, 1), (2, 1, 4), (9, 3, 6), (40, 4, 5)):
        seg, n_steps = _hard_seg(rng, M, Hn, B)
        for gamma in (1.0, 0.95, 0.0, -0.5):
            for ns in (n_steps, None):
                for mode, E, temp, top in (("elite", 1, None, 0), ("elite", min(3, M), None, 5), ("elite", M, None, 64), ("softmax", None, 0.7, 1)):
                    got = S.plan_score(seg, ns, mode, E, temp, gamma, top)
                    score, weight, tp = _scalar(seg, ns, mode, E, temp, gamma, top)
                    assert np.array_equal(got["score"].view(np.uint32), score.view(np.uint32))
                    assert np.array_equal(got["top"], tp) and got["top"].dtype == np.int32 and got["top"].shape == (top, B)
                    assert np.array_equal(np.asarray(got["weight"], np.float64), weight), (M, Hn, B, gamma, mode, E)
                    ok = S.valid(got["score"], ns)
                    assert not np.asarray(got["weight"])[~ok].any()
                    if mode == "elite":
                        assert got["weight"].dtype == np.float32 and np.array_equal(got["weight"].sum(0), np.minimum(E, ok.sum(0)))
                        seen_short = seen_short or bool((ok.sum(0) < E).any())
                    else:
                        for e in range(B):
                            if ok[:, e].any():
                                assert got["weight"][got["top"][0, e], e] == 1.0 and got["weight"][:, e].max() == 1.0
                    for e in range(B):       # a tie at the head of the order went to the lower number
                        ms = np.nonzero(ok[:, e])[0]
                        if top and len(ms) > 1 and (got["score"][ms, e] == got["score"][ms, e].max()).sum() > 1:
                            assert got["top"][0, e] == ms[got["score"][ms, e] == got["score"][ms, e].max()][0]
                            seen_tie = True
                    if B > 1 and ns is not None:
                        assert not np.asarray(got["weight"])[:, 1].any() and (got["top"][:, 1] == -1).all()       # the env with no valid candidate
                    if B > 2 and top:
                        assert got["top"][0, 2] == 0 and (top < 2 or M < 2 or got["top"][1, 2] == 1)               # +0 and -0 tie: candidate numbers ascending
    assert seen_short and seen_tie


# ---------------------------------------------------------------------------------------------------------------- the grid's inputs
GRID_B, GRID_M, GRID_H = (1, 5, 70, 257), (1, 2, 8, 65, 1024), (1, 4, 16)
FAMILIES = ("continuous", "three", "equal", "hole", "junk")
GAMMAS, RS, TEMPS = (1.0, 0.95, 0.0, -0.5), (0, 1, 5, 64), (0.5, 5.0, 100.0)


def _family(family, rng, M, Hn, B):
    """seg [M, H, B] float32 and n_steps [M, B] uint16 (a tenth of the candidates not evaluated, every third env none in `hole`)"""
    if family == "three":
        seg = rng.choice(np.array([-3.0, -1.5, 0.0], np.float32), (M, Hn, B))
    elif family == "equal":
        seg = np.broadcast_to(rng.normal(-5.0, 3.0, (1, Hn, B)).astype(np.float32), (M, Hn, B)).copy()
    else:
        seg = rng.normal(-5.0, 10.0, (M, Hn, B)).astype(np.float32)
    n_steps = np.where(rng.uniform(size=(M, B)) < 0.1, 0, rng.integers(1, 4081, (M, B))).astype(np.uint16)
    if family == "hole":
        n_steps[:, 1::3] = 0
    if family == "junk":
        hit = rng.uniform(size=seg.shape) < 0.08
        seg[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 3e38, -3e38], np.float32), int(hit.sum()))
    return seg, n_steps


def _grid_cases():
    i = 0
    for B in GRID_B:
        for M in GRID_M:
            if M == 1024 and B > 70:
                continue
            for Hn in GRID_H:
                rng = np.random.default_rng(10000 * B + 10 * M + Hn)
                family, gamma, top = FAMILIES[i % 5], GAMMAS[i % 4], RS[(i // 3) % 4]
                elites = (1, min(3, M), M)[(i // 2) % 3]
                seg, n_steps = _family(family, rng, M, Hn, B)
                yield dict(B=B, M=M, H=Hn, family=family, gamma=gamma, top=top, elites=elites, temperature=TEMPS[i % 3], seg=seg, n_steps=n_steps,
                           none=i % 4 == 1)
                i += 1


def test_grid_covers_every_value_the_cases_name():
    cases = list(_grid_cases())
    for key, values in (("B", GRID_B), ("M", GRID_M), ("H", GRID_H), ("family", FAMILIES), ("gamma", GAMMAS), ("top", RS)):
        assert {c[key] for c in cases} == set(values), key
    assert any(c["top"] > c["M"] for c in cases) and any(c["elites"] == c["M"] > 3 for c in cases) and any(c["elites"] == 3 for c in cases)
    assert any(c["M"] == 1024 and c["B"] == 70 for c in cases) and not any(c["M"] == 1024 and c["B"] > 70 for c in cases)
    ties = short = empty = 0
    for c in cases:
        ref = S.plan_score(c["seg"], c["n_steps"], "elite", c["elites"], None, c["gamma"], c["top"])
        ok = S.valid(ref["score"], c["n_steps"])
        short += int((ok.sum(0) < c["elites"]).any())
        empty += int((~ok.any(0)).any())
        ties += int(any(len(np.unique(ref["score"][ok[:, e], e])) < ok[:, e].sum() for e in range(c["B"])))
    assert ties > 10 and short > 5 and empty > 3


# ---------------------------------------------------------------------------------------------------------------- GPU
def _guarded(env, c, mode, n_steps):
    """atc_plan_score through ctypes into PATTERN-filled outputs with GUARD rows of [B] in front and behind; n_steps: "given", "none", "ones\""""
    import torch
    from atc_hip import lib
    B, M, Hn, Rn = c["B"], c["M"], c["H"], c["top"]
    dev = env.device
    seg = torch.as_tensor(c["seg"], device=dev)
    ns = None if n_steps == "none" else torch.as_tensor((c["n_steps"] if n_steps == "given" else np.ones_like(c["n_steps"])).view(np.int16), device=dev)
    rows = {"score": M, "weight": M, "top": max(Rn, 1)}
    bufs = {k: torch.full(((r + 2 * GUARD) * B * 4,), PATTERN, dtype=torch.uint8, device=dev) for k, r in rows.items()}
    inner = {k: bufs[k][GUARD * B * 4:] for k in bufs}
    sc = lib.AtcPlanScore(L.SCORE_ELITE if mode == "elite" else L.SCORE_SOFTMAX, c["elites"] if mode == "elite" else 0, c["gamma"],
                          c["temperature"] if mode == "softmax" else 0.0)
    lib.check(lib.load().atc_plan_score(env.sector.handle, B, Hn, M, seg.data_ptr(), None if ns is None else ns.data_ptr(), C.byref(sc),
                                        inner["score"].data_ptr(), inner["weight"].data_ptr(), inner["top"].data_ptr() if Rn else None, Rn,
                                        torch.cuda.current_stream().cuda_stream))
    env.synchronize()
    out = {}
    for k, r in rows.items():
        used = (Rn if k == "top" else r) * B * 4
        raw = bufs[k].cpu().numpy()
        assert (raw[:GUARD * B * 4] == PATTERN).all() and (raw[GUARD * B * 4 + used:] == PATTERN).all(), "%s: bytes outside the result overwritten" % k
        out[k] = raw[GUARD * B * 4:GUARD * B * 4 + used].view(np.int32 if k == "top" else np.float32).reshape(-1, B)
    return out


def _same_words(got, want, name, tag):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (name, tag, got.shape, want.shape)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad[0]), "%s %r: %d words differ, first at %r: got %r want %r" % (
        name, tag, len(bad[0]), tuple(int(b[0]) for b in bad), got[bad][0], want[bad][0])


def _softmax_check(got_w, ref, tag):
    """the SOFTMAX weight against float32(exp(float64(x))): the largest ulp distance among references >= FLT_MIN (returned), absolute
    difference <= FLT_MIN below that, exactly 0 for invalid candidates and exactly 1 for the best"""
    want = np.asarray(ref["weight"], np.float64)
    okx = ~np.isnan(ref["x"])
    assert not got_w[~okx].view(np.uint32).any(), ("an invalid candidate's weight is not +0", tag)
    B = got_w.shape[1]
    for e in range(B):
        if ref["top"].shape[0] and ref["top"][0, e] >= 0:
            assert got_w[ref["top"][0, e], e] == 1.0, ("the best candidate's weight is not exactly 1", tag, e)
    assert (got_w[okx] >= 0).all() and (got_w[okx] <= 1.0).all(), tag
    small = okx & (want < S.FLT_MIN)
    assert (np.abs(got_w[small].astype(np.float64) - want[small]) <= S.FLT_MIN).all(), tag
    big = okx & ~small
    return int(S.ulp_distance(got_w[big], want[big]).max()) if big.any() else 0


@pytest.fixture(scope="module")
def score_env():
    env = T.look_env(3, 5)
    env.synchronize()
    yield env
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_score_elite_weight_and_top_equal_the_restatement(score_env):
    """ELITE mode over the whole grid, every word of score, weight and top bit for bit; the scenario handle only names the device, so one
    env serves every B.  Only the score record moves and the env state stays byte-identical."""
    env = score_env
    snap = H.snapshot(env)
    start = _records()
    n = 0
    for c in _grid_cases():
        tag = {k: c[k] for k in ("B", "M", "H", "family", "gamma", "top", "elites")}
        ref = S.plan_score(c["seg"], c["n_steps"], "elite", c["elites"], None, c["gamma"], c["top"])
        got = _guarded(env, c, "elite", "given")
        n += 1
        for k in ("score", "weight", "top"):
            _same_words(got[k], ref[k], k, tag)
        if c["none"]:
            ones, none = _guarded(env, c, "elite", "ones"), _guarded(env, c, "elite", "none")
            n += 2
            ref1 = S.plan_score(c["seg"], None, "elite", c["elites"], None, c["gamma"], c["top"])
            for k in ("score", "weight", "top"):
                _same_words(none[k], ones[k], k, ("n_steps=None against all ones", tag))
                _same_words(none[k], ref1[k], k, ("n_steps=None", tag))
    now = _records()
    assert now[0] == {"score": start[0].get("score", 0) + n} and now[1:] == start[1:], "only the score's launch record moves"
    H.bytes_equal(env, snap)


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_softmax_weight_within_the_bar(score_env):
    """SOFTMAX mode over the whole grid: score and top bit for bit, the weight within SOFTMAX_ULP_BAR ulps of float32(exp(float64(x)))
    with x restated exactly.  The largest distance seen is printed before it is held to the bar."""
    env = score_env
    worst, where = 0, None
    for c in _grid_cases():
        tag = {k: c[k] for k in ("B", "M", "H", "family", "gamma", "top", "temperature")}
        ref = S.plan_score(c["seg"], c["n_steps"], "softmax", None, c["temperature"], c["gamma"], c["top"])
        got = _guarded(env, c, "softmax", "given")
        _same_words(got["score"], ref["score"], "score", tag)
        _same_words(got["top"], ref["top"], "top", tag)
        d = _softmax_check(got["weight"], dict(ref, top=S.plan_score(c["seg"], c["n_steps"], "softmax", None, c["temperature"], c["gamma"], 1)["top"]), tag)
        if d > worst:
            worst, where = d, tag
    print("softmax weight: largest distance to float32(exp(float64(x))) = %d ulp at %r (bar %d)" % (worst, where, SOFTMAX_ULP_BAR))
    assert worst <= SOFTMAX_ULP_BAR, (worst, where)


@pytest.mark.gpu
@pytest.mark.timeout(60)
def test_python_arguments_refusals_and_touching_ranges(score_env):
    import torch
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import model
    env = score_env
    B, M, Hn = env.B, 8, 4
    rng = np.random.default_rng(7)
    seg_np, ns_np = _family("three", rng, M, Hn, B)
    seg, ns = torch.as_tensor(seg_np, device=env.device), torch.as_tensor(ns_np.view(np.int16), device=env.device)
    ref = S.plan_score(seg_np, ns_np, "elite", 3, None, 0.9, 5)
    res = env.score_plans(seg, ns, elites=3, gamma=0.9, top=5)
    env.synchronize()
    assert set(res) == {"score", "weight", "top"} and res["top"].dtype == torch.int32 and tuple(res["top"].shape) == (5, B)
    for k in res:
        _same_words(res[k].cpu().numpy(), ref[k], k, "score_plans")
    assert set(env.score_plans(seg, ns, elites=3, top=0)) == {"score", "weight"}
    soft = env.score_plans(seg, mode="softmax", temperature=2.0, gamma=0.9)
    env.synchronize()
    _softmax_check(soft["weight"].cpu().numpy(), S.plan_score(seg_np, None, "softmax", None, 2.0, 0.9, 1), "score_plans softmax")
    # out=: written in place, nothing allocated; ranges that only touch are accepted (one buffer: score | weight | top, back to back)
    flat = torch.empty(2 * M * B + 5 * B, dtype=torch.float32, device=env.device)
    out = {"score": flat[:M * B].view(M, B), "weight": flat[M * B:2 * M * B].view(M, B), "top": flat[2 * M * B:].view(torch.int32).view(5, B)}
    env.synchronize()
    torch.cuda.reset_peak_memory_stats(env.device)
    held = torch.cuda.memory_allocated(env.device)
    back = env.score_plans(seg, ns, elites=3, gamma=0.9, top=5, out=out)
    env.synchronize()
    assert torch.cuda.max_memory_allocated(env.device) == held, "score_plans(out=) allocated device memory"
    for k in out:
        assert back[k].data_ptr() == out[k].data_ptr()
        _same_words(back[k].cpu().numpy(), ref[k], k, "out=, touching ranges")
    # ValueError: shape, dtype, device, the library's refusals mirrored
    for bad in (dict(seg_reward=seg[:, :, :3]), dict(seg_reward=seg.double()), dict(seg_reward=seg.cpu()), dict(seg_reward=seg.transpose(0, 1)),
                dict(seg_reward=seg[0]), dict(seg_reward=seg.repeat(1, 5, 1)[:, :17].contiguous()), dict(n_steps=ns[:4]), dict(n_steps=ns.int()),
                dict(n_steps=ns.cpu()), dict(elites=0), dict(elites=M + 1), dict(elites=None), dict(mode="softmax"), dict(mode="softmax", temperature=0.0),
                dict(mode="softmax", temperature=float("inf")), dict(mode="rank"), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(top=-1),
                dict(top=65), dict(out={"score": out["score"]}), dict(out=dict(out, top=out["top"][:1])), dict(out=dict(out, weight=out["weight"].double())),
                dict(out=dict(out, score=out["score"].cpu())), dict(out=(out["score"], out["weight"]))):
        kw = dict(dict(seg_reward=seg, n_steps=ns, elites=3, top=5), **bad)
        with pytest.raises(ValueError):
            env.score_plans(kw.pop("seg_reward"), kw.pop("n_steps"), **kw)
    # the overlap rule, refused by the library: no record moves
    before = _records()
    with pytest.raises(RuntimeError, match="overlaps"):
        env.score_plans(seg, ns, elites=3, top=5, out=dict(out, weight=out["score"]))
    with pytest.raises(RuntimeError, match="overlaps"):
        env.score_plans(seg, ns, elites=3, top=5, out=dict(out, weight=flat[M * B - 1:2 * M * B - 1].view(M, B)))
    with pytest.raises(RuntimeError, match="overlaps"):
        env.score_plans(seg, None, elites=3, top=0, out={"score": seg[:2].view(M, B), "weight": out["weight"]})
    assert _records() == before
    # a discrete-action env: the method reads no action
    denv = AtcVecEnv(B, 2, sim_parameters=model.SimParameters(1, discrete_action_space=True), scenario=T.look_scenario(), grid_cell=0.5)
    denv.reset()
    dres = denv.score_plans(seg.to(denv.device), ns.to(denv.device), elites=3, gamma=0.9, top=5)
    denv.synchronize()
    for k in dres:
        _same_words(dres[k].cpu().numpy(), ref[k], k, "a discrete-action env")
    denv.close()


def _small_planner_env(rng):
    env = T.look_env(3, 5)
    T.look_fly(env, rng)
    return env


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_cem_plan_scored_equals_the_loop_on_the_restatements():
    """Three CEM iterations against the same loop written with plan_draw_ref, the library's own lookahead_plan for the rewards,
    plan_score_ref and plan_refit_ref: mean, std and decision bit for bit"""
    import torch
    from atc_hip import cem
    B, N, K, Hn, M, E, gamma = 5, 3, 3, 2, 8, 3, 0.9
    rng = np.random.default_rng(61)
    env = _small_planner_env(rng)
    mean0 = torch.as_tensor(rng.uniform(-0.5, 0.5, (Hn, B, N, 3)).astype(np.float32), device=env.device)
    snap = H.snapshot(env)
    with pytest.raises(ValueError):
        cem.cem_plan_scored(env, mean0, 0.4, K, M, 0, E)
    with pytest.raises(ValueError):
        cem.cem_plan_scored(env, mean0, 0.4, K, M, 1, M + 1)
    before = _records()
    got = cem.cem_plan_scored(env, mean0, 0.4, K, M, 3, E, gamma=gamma, seed=12)
    env.synchronize()
    now = _records()
    assert now[0].get("score", 0) - before[0].get("score", 0) == 3 and now[1].get("refit", 0) - before[1].get("refit", 0) == 3
    assert sum(now[2].values()) - sum(before[2].values()) == 3 and now[3].get("draw", 0) - before[3].get("draw", 0) == 1 and now[4:] == before[4:]
    H.bytes_equal(env, snap)
    mean, std = mean0.cpu().numpy(), np.full(mean0.shape, 0.4, np.float32)
    for t in range(3):
        plans = P.draw(mean, std, M, seed=12, iteration=t)
        res = env.lookahead_plan(torch.as_tensor(plans, device=env.device), K, outputs=("seg_reward",))
        env.synchronize()
        ref = S.plan_score(res["seg_reward"].cpu().numpy(), res["n_steps"].cpu().numpy(), "elite", E, None, gamma, 1)
        assert (ref["weight"].sum(0) == E).all()
        best = plans[ref["top"][0], 0, np.arange(B)]
        mean, std = R.refit(mean, std, M, ref["weight"], seed=12, iteration=t, draws=plans)
    _same_words(got[0].cpu().numpy(), mean, "mean", "cem_plan_scored")
    _same_words(got[1].cpu().numpy(), std, "std", "cem_plan_scored")
    assert got[2].shape == (B, N, 3)
    _same_words(got[2].cpu().numpy(), best, "best_first_decision", "cem_plan_scored")
    H.bytes_equal(env, snap)
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_mppi_plan_scored_equals_the_loop_on_the_restatements():
    """Two MPPI iterations: the device's own softmax weights — each held to the bar against plan_score_ref — are fed to the restated
    refit, and the result is compared bit for bit (the tighter of the two forms the comparison could take)"""
    import torch
    from atc_hip import cem
    B, N, K, Hn, M, temp, gamma, floor = 5, 3, 3, 2, 8, 5.0, 0.9, 0.02
    rng = np.random.default_rng(62)
    env = _small_planner_env(rng)
    mean0 = torch.as_tensor(rng.uniform(-0.5, 0.5, (Hn, B, N, 3)).astype(np.float32), device=env.device)
    snap = H.snapshot(env)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(iters=0)):
        with pytest.raises(ValueError):
            cem.mppi_plan_scored(env, mean0, 0.4, K, M, **dict(dict(iters=1, temperature=temp), **bad))
    got = cem.mppi_plan_scored(env, mean0, 0.4, K, M, 2, temp, gamma=gamma, seed=5, std_min=floor)
    env.synchronize()
    H.bytes_equal(env, snap)
    mean, std = mean0.cpu().numpy(), np.full(mean0.shape, 0.4, np.float32)
    spread = []
    for t in range(2):
        plans = P.draw(mean, std, M, seed=5, iteration=t)
        res = env.lookahead_plan(torch.as_tensor(plans, device=env.device), K, outputs=("seg_reward",))
        dev = env.score_plans(res["seg_reward"], res["n_steps"], mode="softmax", temperature=temp, gamma=gamma, top=1)
        env.synchronize()
        ref = S.plan_score(res["seg_reward"].cpu().numpy(), res["n_steps"].cpu().numpy(), "softmax", None, temp, gamma, 1)
        w = dev["weight"].cpu().numpy()
        _same_words(dev["score"].cpu().numpy(), ref["score"], "score", t)
        _same_words(dev["top"].cpu().numpy(), ref["top"], "top", t)
        assert _softmax_check(w, ref, ("mppi", t)) <= SOFTMAX_ULP_BAR
        spread.append(int((w > 0).sum(0).max()))
        best = plans[ref["top"][0], 0, np.arange(B)]
        mean, std = R.refit(mean, std, M, w, seed=5, iteration=t, draws=plans)
        std = np.maximum(std, np.float32(floor))
    assert min(spread) > 1, "in every env the softmax weight sits on one candidate"
    _same_words(got[0].cpu().numpy(), mean, "mean", "mppi_plan_scored")
    _same_words(got[1].cpu().numpy(), std, "std", "mppi_plan_scored")
    _same_words(got[2].cpu().numpy(), best, "best_first_decision", "mppi_plan_scored")
    H.bytes_equal(env, snap)
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_cem_plan_scored_leaves_out_what_was_not_evaluated():
    """An env with a WIDE heading at the start of the call, placed as test_plan_sampled.py places it: under that rule NONE of the env's
    candidates is evaluated — candidate 1 among them —, every one scores 0 and the older loop makes `elites` of them the elites.
    cem_plan_scored leaves them all out: weight 0, top -1, and the env keeps its distribution, while its neighbours refit as ever."""
    import torch
    from atc_hip import cem
    B, N, K, Hn, M, E = 5, 3, 3, 2, 8, 3
    rng = np.random.default_rng(63)
    env = T.look_env(N, B)
    T.look_fly(env, rng, steps=40)
    e_wide = B - 2
    env.set_state(e_wide, N - 1, *H.FAR_B[:3], 500.0, H.FAR_B[4])    # 500 deg: beyond the 32-bit heading field
    env.synchronize()
    assert int(env.phi_fix[e_wide * N + N - 1]) == L.I32_MAX
    mean0 = torch.as_tensor(rng.uniform(-0.5, 0.5, (Hn, B, N, 3)).astype(np.float32), device=env.device)
    res = env.lookahead_plan_sampled(mean0, 0.4, K, M, seed=3, iteration=0)
    sc = env.score_plans(res["seg_reward"], res["n_steps"], elites=E, top=2)
    env.synchronize()
    n_steps, weight, top = res["n_steps"].cpu().numpy(), sc["weight"].cpu().numpy(), sc["top"].cpu().numpy()
    assert n_steps[1, e_wide] == 0 and not n_steps[:, e_wide].any() and n_steps[:, :e_wide].all()
    assert not weight[:, e_wide].any() and (top[:, e_wide] == -1).all()
    others = [e for e in range(B) if e != e_wide]
    assert (weight[:, others].sum(0) == E).all() and (top[:, others] >= 0).all()
    assert not sc["score"].cpu().numpy()[:, e_wide].any(), "a candidate that was not evaluated scores 0, which the older loop ranks"
    new = cem.cem_plan_scored(env, mean0, 0.4, K, M, 1, E, seed=3)
    old = cem.cem_plan_launch(env, mean0, 0.4, K, M, 1, E, seed=3)
    env.synchronize()
    assert torch.equal(new[0][:, e_wide], mean0[:, e_wide]) and bool((new[1][:, e_wide] == np.float32(0.4)).all()) and not bool(new[2][e_wide].any())
    assert not torch.equal(old[1][:, e_wide], new[1][:, e_wide]), "the older loop refits the env from candidates that never flew"
    assert not torch.equal(new[1][:, others], torch.full_like(new[1][:, others], 0.4))
    env.close()
