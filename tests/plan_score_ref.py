"""atc_plan_score (include/atc_step.h) restated in numpy: the discounted score in np.float32, operation by operation; validity; the
strict total order (score descending, equal scores to the lower candidate number, -0 as +0) by a stable sort; the ELITE weights; top;
and the SOFTMAX argument x in fp32 with exp of it in float64 — expf is the one inexact step of the contract, so the device's weight is
held to float32(exp(float64(x))) within a bar (ulp_distance), never bit for bit."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny
MAX_TOP = 64
QUIET_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
# THE SOFTMAX BAR (derived in tests/test_plan_score.py's docstring): twice the largest ulp distance of the device's expf measured over
# that file's softmax inputs on an MI355X.  One bar for every test that holds a softmax weight.
MEASURED_MAX_ULP = 1
SOFTMAX_ULP_BAR = 2 * MEASURED_MAX_ULP


def score(seg, gamma):
    """[M, B] float32 from seg [M, H, B]: seg[:, 0] assigned, then + seg[:, h] * g_h with g_h the fp32 running product of gamma"""
    seg = np.asarray(seg, np.float32)
    gamma = np.float32(gamma)
    s = seg[:, 0].copy()
    g = np.float32(1.0)
    with np.errstate(all="ignore"):
        for h in range(1, seg.shape[1]):
            g = np.float32(g * gamma)
            s = (s + (seg[:, h] * g).astype(np.float32)).astype(np.float32)
    s[np.isnan(s)] = QUIET_NAN          # (the header's one NaN: hosts and devices differ in the sign of a computed NaN)
    return s


def valid(s, n_steps=None):
    """[M, B] bool: evaluated (n_steps != 0, or no n_steps) and the score finite"""
    with np.errstate(invalid="ignore"):
        ok = np.abs(s) <= FLT_MAX
    if n_steps is not None:
        ok = ok & (np.asarray(n_steps) != 0)
    return ok


def order(s, ok):
    """per env the list of its valid candidate numbers, first in the order first: a stable sort on -score (with -0 normalised), so
    that equal scores keep ascending candidate number"""
    out = []
    for e in range(s.shape[1]):
        ms = np.nonzero(ok[:, e])[0]
        key = -(s[ms, e].astype(np.float64) + 0.0)        # (float64 holds every float32 exactly; + 0.0 turns -0 into +0)
        key = np.where(key == 0.0, 0.0, key)
        out.append(ms[np.argsort(key, kind="stable")])
    return out


def plan_score(seg, n_steps=None, mode="elite", elites=None, temperature=None, gamma=1.0, top=1):
    """{"score", "weight", "top", "x"}: score [M, B] float32; weight [M, B] — ELITE: float32, exact; SOFTMAX: float64 exp(float64(x));
    top [top, B] int32 (always present, possibly with 0 rows); x [M, B] float32, the softmax argument (NaN where the candidate is invalid
    or the mode is ELITE)."""
    seg = np.asarray(seg, np.float32)
    M, _, B = seg.shape
    s = score(seg, gamma)
    ok = valid(s, n_steps)
    ranks = order(s, ok)
    tp = np.full((int(top), B), -1, np.int32)
    x = np.full((M, B), np.nan, np.float32)
    w = np.zeros((M, B), np.float32 if mode == "elite" else np.float64)
    for e, ms in enumerate(ranks):
        n = min(int(top), len(ms))
        tp[:n, e] = ms[:n]
        if not len(ms):
            continue
        if mode == "elite":
            w[ms[:min(int(elites), len(ms))], e] = 1.0
        else:
            with np.errstate(all="ignore"):
                d = (s[ms, e] - s[ms[0], e]).astype(np.float32)
                x[ms, e] = (d / np.float32(temperature)).astype(np.float32)
                w[ms, e] = np.exp(x[ms, e].astype(np.float64))
    return {"score": s, "weight": w, "top": tp, "x": x}


def ulp_distance(got, want64):
    """distance in float32 ulps between got (float32) and float32(want64), counted on the ordered integer image of the bits; only
    meaningful where both are finite and >= 0 (weights are)"""
    a = np.asarray(got, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(want64).astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)
