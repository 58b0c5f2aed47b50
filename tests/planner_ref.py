"""One iteration of a scored planner — draw -> score -> rank / weigh -> refit -> pick the decision — held to a float64 evaluation of the
ORACLE's flight of the same plans.  TEST INFRASTRUCTURE ONLY; needs no GPU.

tests/plan_score_ref.py and tests/plan_refit_ref.py restate the kernels' own definitions and share every decision the kernels made (where
the discount starts, what counts as evaluated, what is read behind a stop, which way a tie goes).  Nothing here does: the inputs are the
per-candidate references of tests/skip_ref.py::plan_references (the oracle's seg_reward — fp32 words, every one exact in float64 —, its
seg_reward_scale and n_steps), the fp32 plans of tests/plan_draw_ref.py::draw and the mask `ok` of envs that are not WIDE at the start.

  reference(refs, ok, gamma, mode, ...)     score64, valid, bar, order, winner, the two decisive flags, softmax64
  check_iteration(got, ref, plans, ...)     a device iteration (or a stand-in for one) against it; returns what it measured
  check_refit(...)                          the refit part alone: float64 moments under the device's own weights, plan_refit_ref.bounds
  stand_in(...)                             an iteration built from the oracle's rewards with the numpy restatements, and its mutations

THE BAR OF A SCORE, derived, not measured:  bar[m, e] = sum_h |gamma|^h 1e-5 seg_reward_scale[m, h, e]  +  2 H 2^-24 sum_h |gamma^h seg64[m, h, e]|.
The first term is what bars.check_plan_segments grants each segment the score is a combination of; the second covers the fp32
evaluation: the discount of segment h is a running product (the rounding of gamma and h - 1 products), the term one product and the
left-to-right sum one addition per segment, at most 2 H roundings on any term.

DECISIVE.  A pair (a before b in the float64 order) is decided when score64[a] - score64[b] > bar[a] + bar[b], or when the two float64
scores are exactly equal and the fp32 segment words that enter the score (those with gamma^h != 0) are equal word for word — then the
documented tie rule (the lower candidate number) decides.  The winner is decisive when it is decided against EVERY other valid candidate
(the runner-up's bar need not be the largest, so the runner-up alone would not do); the elite boundary when every candidate of the first
E is decided against every candidate behind them.  An env with at most one valid candidate (at most E, for the boundary) is decisive.
A non-decisive env is never left unchecked: what the device chose must then lie within the bars of what the oracle chose.
  winner     dev[top0] >= dev[w] and |dev - score64| <= bar give score64[top0] >= score64[w] - bar[top0] - bar[w].
  boundary   E candidates have score64 >= s_E (the oracle's E-th score), so the device's E-th largest score is >= s_E - max bar of those
             E; the candidates from position E on have score64 <= s_E, so it is <= s_E + max bar of those.  A member therefore has
             score64 >= s_E - bar[member] - (the first maximum), a valid non-member score64 <= s_E + bar[it] + (the second).
  top[r]     dev[top[r]] >= dev[top[r + 1]] gives score64[top[r]] + bar[top[r]] + bar[top[r + 1]] >= score64[top[r + 1]]; a decided tie
             must stand in ascending candidate number."""
import numpy as np

import plan_refit_ref as RF
import plan_score_ref as S

U = 2.0 ** -24


def reference(refs, ok, gamma, mode, elites=None, temperature=None, top=1, seg32=None):
    """refs: plan_references' M dicts; ok [B] bool.  seg32 [M, H, B] float32: the fp32 segment inputs whose words decide what an exact
    tie means (default: the oracle's own, rounded to fp32 — they are fp32 words already)."""
    M, ok = len(refs), np.asarray(ok, bool)
    seg64 = np.stack([np.asarray(r["seg_reward"], np.float64) for r in refs])                     # [M, H, B]
    scale = np.stack([np.asarray(r["seg_reward_scale"], np.float64) for r in refs])
    n_steps = np.stack([np.asarray(r["n_steps"]).astype(np.int64) for r in refs])
    Hn, B = seg64.shape[1], seg64.shape[2]
    g = float(gamma) ** np.arange(Hn)                                                             # (0.0 ** 0 == 1.0)
    terms = g[None, :, None] * seg64
    score64 = terms.sum(1)
    bar = (np.abs(g)[None, :, None] * 1e-5 * scale).sum(1) + 2 * Hn * U * np.abs(terms).sum(1)
    valid = ok[None, :] & np.isfinite(score64)
    words = np.ascontiguousarray(seg64.astype(np.float32) if seg32 is None else np.asarray(seg32, np.float32)).view(np.uint32)[:, g != 0, :]
    ref = dict(M=M, H=Hn, B=B, ok=ok, gamma=float(gamma), mode=mode, elites=elites, temperature=temperature, top=int(top), seg64=seg64,
               n_steps=n_steps, score64=score64, bar=bar, valid=valid, words=words)
    order, winner = [], np.full(B, -1, np.int64)
    win_dec, elite_dec = np.ones(B, bool), np.ones(B, bool)
    for e in range(B):
        ms = np.nonzero(valid[:, e])[0]
        o = ms[np.argsort(-score64[ms, e], kind="stable")]         # descending; an exact float64 tie keeps the lower number first
        order.append(o)
        if len(o):
            winner[e] = o[0]
            win_dec[e] = all(decided(ref, o[0], j, e) for j in o[1:])
            if mode == "elite" and len(o) > elites:
                elite_dec[e] = all(decided(ref, i, j, e) for i in o[:elites] for j in o[elites:])
    soft = np.zeros((M, B))
    if mode == "softmax":
        for e in range(B):
            o = order[e]
            if len(o):
                soft[o, e] = np.exp((score64[o, e] - score64[o[0], e]) / float(temperature))
    ref.update(order=order, winner=winner, winner_decisive=win_dec, elite_decisive=elite_dec, softmax64=soft,
               evaluated=np.array([len(o) > 0 for o in order]))
    return ref


def tied(ref, a, b, e):
    """an exact float64 tie on equal fp32 words: the tie rule decides"""
    return ref["score64"][a, e] == ref["score64"][b, e] and np.array_equal(ref["words"][a, :, e], ref["words"][b, :, e])


def decided(ref, a, b, e):
    """a stands before b in env e's float64 order: is that order decided (module docstring)?"""
    s, bar = ref["score64"], ref["bar"]
    return bool(s[a, e] - s[b, e] > bar[a, e] + bar[b, e]) or (tied(ref, a, b, e) and a < b)


def shares(ref):
    """(evaluated envs, of them non-decisive for the winner, envs an elite boundary is asked of, of them non-decisive)"""
    ev = ref["evaluated"]
    asked = ev if ref["mode"] == "elite" else np.zeros_like(ev)
    return int(ev.sum()), int((ev & ~ref["winner_decisive"]).sum()), int(asked.sum()), int((asked & ~ref["elite_decisive"]).sum())


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_refit(new_mean, new_std, mean, std, plans, weight, tag=None):
    """refit_plans' results under `weight` (the device's own) against the float64 moments of the fp32 plans under those weights upcast,
    within plan_refit_ref.bounds; envs with no participant keep the input rows bit for bit.  Returns the largest error over its bound."""
    mean = np.asarray(mean, np.float32)
    M = plans.shape[0]
    std = np.ascontiguousarray(np.broadcast_to(np.asarray(std, np.float32), mean.shape))
    new_mean, new_std = (np.asarray(x, np.float32).reshape(mean.shape) for x in (new_mean, new_std))
    weight = np.asarray(weight, np.float32)
    some = RF.participates(weight).any(0)
    assert np.array_equal(_words(new_mean[:, ~some]), _words(mean[:, ~some])), ("an env with no participant lost its mean", tag)
    assert np.array_equal(_words(new_std[:, ~some]), _words(std[:, ~some])), ("an env with no participant lost its std", tag)
    if not some.any():
        return 0.0
    r64 = RF.refit64(mean, std, M, weight, draws=plans)
    worst = 0.0
    for name, got, want, bound in zip(("new_mean", "new_std"), (new_mean, new_std), (r64["mean"], r64["std"]), RF.bounds(M, r64)):
        err = np.abs(got.astype(np.float64) - want)[:, some]
        bound = bound[:, some]
        ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
        worst = max(worst, float(ratio.max()))
        assert np.all(err <= bound), ("refit: %s beyond the summation bound of float64" % name, tag, float(ratio.max()))
    return worst


def check_iteration(got, ref, plans, mean, std, tag=None):
    """got: score, weight [M, B] float32; top [R, B] (R >= 1); new_mean, new_std [H, B, N, 3] — refit_plans under got["weight"], out of
    place —; decision [B, N, 3] = draw_plans(index=top[:1])[0, 0]; optionally seg_reward [M, H, B], the words the score was computed
    from.  Raises AssertionError naming `tag`; returns dict(score, softmax, refit: the largest observed error over its bar; pairs)."""
    score, weight = np.asarray(got["score"], np.float32), np.asarray(got["weight"], np.float32)
    top = np.asarray(got["top"]).astype(np.int64)
    M, B, ok, valid, s64, bar = ref["M"], ref["B"], ref["ok"], ref["valid"], ref["score64"], ref["bar"]
    assert score.shape == weight.shape == (M, B) and top.shape == (ref["top"], B) and ref["top"] >= 1, (tag, score.shape, top.shape)
    decision = np.asarray(got["decision"], np.float32).reshape(B, -1, 3)
    stats = dict(score=0.0, softmax=0.0, refit=0.0, pairs=int(valid.sum()))
    # ---- the score
    with np.errstate(invalid="ignore"):          # (an invalid candidate's score64 is not finite; only valid pairs are compared)
        err = np.abs(score.astype(np.float64) - s64)
    if valid.any():
        stats["score"] = float((err[valid] / bar[valid]).max())
    assert np.all(err[valid] <= bar[valid]), ("score beyond its bar", tag, stats["score"], [int(x[0]) for x in np.nonzero(valid & ~(err <= bar))])
    for name, a in (("score", score), ("weight", weight)) + ((("seg_reward", np.asarray(got["seg_reward"], np.float32)),) if "seg_reward" in got else ()):
        assert not _words(a[..., ~ok]).any(), ("an env that is not evaluated: %s is not zero" % name, tag)
    assert (top[:, ~ok] == -1).all(), ("an env that is not evaluated: top is not -1 down the column", tag)
    assert not _words(weight[~valid]).any(), ("an invalid candidate has a weight", tag)
    # ---- the order, the winner, the weights
    for e in range(B):
        o, col = ref["order"][e], top[:, e]
        k = min(len(col), len(o))
        assert (col[k:] == -1).all() and (col[:k] >= 0).all() and (col[:k] < M).all() and len(set(col[:k].tolist())) == k and valid[col[:k], e].all(), \
            ("top names something else than min(top, valid) distinct valid candidates", tag, e, col.tolist(), o.tolist())
        t0 = int(col[0])
        want_row = plans[t0, 0, e] if t0 >= 0 else np.zeros_like(plans[0, 0, e])
        assert np.array_equal(_words(decision[e]), _words(want_row)), ("the decision is not the first action of plan top[0]", tag, e, t0)
        if not len(o):
            continue
        w0 = int(o[0])
        if ref["winner_decisive"][e]:
            assert t0 == w0, ("winner", tag, e, t0, w0, s64[:, e].tolist(), bar[:, e].tolist())
        else:
            assert s64[t0, e] >= s64[w0, e] - bar[t0, e] - bar[w0, e], ("winner beyond the bars of the oracle's", tag, e, t0, w0)
        for r in range(k - 1):
            a, b = int(col[r]), int(col[r + 1])
            assert s64[a, e] + bar[a, e] + bar[b, e] >= s64[b, e], ("top is not a descending order to within the bars", tag, e, r, col.tolist())
            assert not (tied(ref, a, b, e) and a > b), ("an exact tie stands in descending candidate number", tag, e, r, col.tolist())
        w = weight[:, e]
        if ref["mode"] == "elite":
            E = int(ref["elites"])
            assert np.isin(w, (0.0, 1.0)).all() and w.sum() == min(E, len(o)), ("elite weights", tag, e, w.tolist())
            members = np.nonzero(w == 1.0)[0]
            assert all(w[col[r]] == 1.0 for r in range(min(k, E))), ("top's first E are not the elites", tag, e)
            if ref["elite_decisive"][e]:
                assert set(members.tolist()) == set(o[:E].tolist()), ("elite set", tag, e, members.tolist(), o[:E].tolist())
            else:
                s_e, lo, hi = s64[o[E - 1], e], bar[o[:E], e].max(), bar[o[E - 1:], e].max()
                for m in o:
                    if w[m] == 1.0:
                        assert s64[m, e] >= s_e - bar[m, e] - lo, ("an elite beyond the bars below the oracle's E-th score", tag, e, int(m))
                    else:
                        assert s64[m, e] <= s_e + bar[m, e] + hi, ("a candidate left out beyond the bars above the oracle's E-th score", tag, e, int(m))
        else:
            T = float(ref["temperature"])
            assert w[t0] == 1.0, ("the winner's weight is not exactly 1", tag, e)
            bw = max(bar[w0, e], bar[t0, e])
            for m in o:
                if m == t0:
                    continue
                w64 = ref["softmax64"][m, e]
                if w64 < S.FLT_MIN:
                    allowed = float(S.FLT_MIN)
                else:
                    allowed = w64 * np.expm1((bar[m, e] + bw) / T) + S.SOFTMAX_ULP_BAR * float(np.spacing(np.float32(w64)))
                dist = abs(float(w[m]) - w64)
                stats["softmax"] = max(stats["softmax"], dist / allowed)
                assert dist <= allowed, ("softmax weight", tag, e, int(m), float(w[m]), w64, dist / allowed)
    # ---- the refit under the device's own weights
    stats["refit"] = check_refit(got["new_mean"], got["new_std"], mean, std, plans, weight, tag)
    return stats


# ---------------------------------------------------------------------------------------------------------------- a stand-in device
MUTATIONS = ("late", "plus1", "admit", "ties")


def stand_in(refs, ok, plans, mean, std, gamma, mode, elites=None, temperature=None, top=1, mutation=None):
    """`got` of check_iteration from the ORACLE's seg_reward rounded to fp32 (zeros and n_steps == 0 outside ok, as the device returns
    them) run through plan_score_ref and plan_refit_ref.  mutation: None, or one deliberate fault —
      late    the discount starts one segment late (1, 1, gamma, gamma^2, ...)          plus1   segment h is discounted gamma^(h + 1)
      admit   candidates that were not evaluated are admitted (n_steps ignored)         ties    exact ties go to the HIGHER number"""
    assert mutation is None or mutation in MUTATIONS, mutation
    f = np.float32
    seg = np.stack([np.asarray(r["seg_reward"]).astype(f) for r in refs])
    n = np.stack([np.asarray(r["n_steps"]).astype(np.uint16) for r in refs])
    seg[:, :, ~ok], n[:, ~ok] = 0, 0
    M, Hn, B = seg.shape
    use, g_use, n_use = seg, gamma, (None if mutation == "admit" else n)
    if mutation in ("late", "plus1"):
        g, s = (f(1.0), seg[:, 0].copy()) if mutation == "late" else (f(gamma), (seg[:, 0] * f(gamma)).astype(f))
        for h in range(1, Hn):
            if mutation == "plus1":
                g = f(g * f(gamma))
            s = (s + (seg[:, h] * g).astype(f)).astype(f)
            if mutation == "late":
                g = f(g * f(gamma))
        use, g_use = s[:, None, :], 1.0
    if mutation == "ties":
        use, n_use = use[::-1], n_use[::-1]
    res = S.plan_score(use, n_use, mode, elites, temperature, g_use, top)
    score, weight, tp = res["score"], np.asarray(res["weight"]).astype(f), res["top"].astype(np.int64)
    if mutation == "ties":
        score, weight, tp = score[::-1], weight[::-1], np.where(tp >= 0, M - 1 - tp, -1)
    new_mean, new_std = RF.refit(mean, std, M, weight, draws=plans)
    t0 = tp[0]
    decision = np.where((t0 >= 0)[:, None, None], plans[np.maximum(t0, 0), 0, np.arange(B)], f(0))
    return dict(score=np.ascontiguousarray(score), weight=np.ascontiguousarray(weight), top=tp, new_mean=new_mean, new_std=new_std,
                decision=decision, seg_reward=seg)


def naive_refit(mean, std, plans, weight):
    """the fifth fault: the refit about the UNCLAMPED mean in the E[a^2] - E[a]^2 form, fp32 (what plan_refit_ref.refit's shift avoids)"""
    f = np.float32
    wb = np.where(RF.participates(weight), weight, 0).astype(f)[:, None, :, None, None]
    a = np.asarray(plans, f)
    with np.errstate(all="ignore"):
        Wt = wb.sum(0, dtype=f)
        mu = ((wb * a).sum(0, dtype=f) / Wt).astype(f)
        sd = np.sqrt(np.fmax(((wb * a * a).sum(0, dtype=f) / Wt).astype(f) - (mu * mu).astype(f), f(0))).astype(f)
    some = np.broadcast_to(RF.participates(weight).any(0)[None, :, None, None], a.shape[1:])
    mean = np.asarray(mean, f)
    return np.where(some, mu, mean).astype(f), np.where(some, sd, np.broadcast_to(np.asarray(std, f), mean.shape)).astype(f)
