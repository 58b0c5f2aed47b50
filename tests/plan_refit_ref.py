"""atc_plan_refit (include/atc_step.h) restated in numpy: the weighted mean and standard deviation of the drawn plans about the clamped
mean, float32 throughout, one rounding per operation, sequential in the candidate number — every word the kernel writes, bit for bit.
TEST INFRASTRUCTURE ONLY; needs no GPU.

  participates(weight)                         0 < w <= FLT_MAX (NaN, zero, negative, infinite: out)
  refit(mean, std, M, weight, ...)             (new_mean, new_std) [H, B, N, 3] float32; an env with no participant keeps `into`
  refit64(mean, std, M, weight, ...)           the same two moments evaluated in float64 on the float32 draws, with the quantities the
                                               error bound of the float32 loop is written in
  bounds(M, r64)                               that bound: (on the mean, on the standard deviation)"""
import numpy as np

import plan_draw_ref as P

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
U = 2.0 ** -24          # the unit roundoff of float32
ETA = 2.0 ** -149       # the smallest positive float32: what a product or quotient that underflows may be off by, absolutely


def participates(weight):
    w = np.asarray(weight, F32)
    with np.errstate(invalid="ignore"):
        return (w > 0) & (w <= FLT_MAX)


def _inputs(mean, std, M, weight):
    mean = np.asarray(mean, F32)
    std = np.broadcast_to(np.asarray(std, F32), mean.shape)
    weight = np.asarray(weight, F32)
    assert mean.ndim == 4 and mean.shape[3] == 3 and weight.shape == (M, mean.shape[1]), (mean.shape, weight.shape)
    return mean, std, weight


def refit(mean, std, M, weight, seed=0, iteration=0, mean_first=True, into=None, draws=None):
    """into: (mean_rows, std_rows) that envs with no participating candidate keep (default: the inputs).  draws: the plans
    [M, H, B, N, 3] of this key, where the caller has them already (plan_draw_ref.draw's, or AtcVecEnv.draw_plans' rows)."""
    mean, std, weight = _inputs(mean, std, M, weight)
    part = participates(weight)                                   # [M, B]
    ctr = P.clamp(mean)
    s1, s2 = np.zeros(mean.shape, F32), np.zeros(mean.shape, F32)
    W = np.zeros(mean.shape, F32)
    a_all = P.draw(mean, std, M, seed=seed, iteration=iteration, mean_first=mean_first) if draws is None else np.asarray(draws, F32)
    assert a_all.shape == (M,) + mean.shape, a_all.shape
    with np.errstate(all="ignore"):
        for m in range(M):
            if not part[m].any():
                continue
            on = np.broadcast_to(part[m][None, :, None, None], mean.shape)
            w = np.broadcast_to(np.where(part[m], weight[m], F32(0))[None, :, None, None], mean.shape).astype(F32)
            d = (a_all[m] - ctr).astype(F32)
            t = (w * d).astype(F32)
            s1 = np.where(on, (s1 + t).astype(F32), s1)
            s2 = np.where(on, (s2 + (t * d).astype(F32)).astype(F32), s2)
            W = np.where(on, (W + w).astype(F32), W)
        q = (s1 / W).astype(F32)
        new_mean = (ctr + q).astype(F32)
        new_std = np.sqrt(np.fmax(((s2 / W).astype(F32) - (q * q).astype(F32)).astype(F32), F32(0))).astype(F32)
    keep_mean, keep_std = (mean, std) if into is None else (np.asarray(into[0], F32).reshape(mean.shape), np.asarray(into[1], F32).reshape(mean.shape))
    some = np.broadcast_to(part.any(0)[None, :, None, None], mean.shape)
    return np.where(some, new_mean, keep_mean).astype(F32), np.where(some, new_std, keep_std).astype(F32)


def refit64(mean, std, M, weight, seed=0, iteration=0, mean_first=True, draws=None):
    """The weighted mean and standard deviation of the float32 draws in float64 (envs with no participant: NaN), and A1 = sum |w d| / W,
    A2 = sum w d^2 / W with d = a - ctr: what the float32 loop's rounding errors are proportional to.  draws: as in refit()."""
    mean, std, weight = _inputs(mean, std, M, weight)
    part = participates(weight)
    w = np.where(part, weight, 0).astype(np.float64)[:, None, :, None, None]                    # [M, 1, B, 1, 1]
    a = P.draw(mean, std, M, seed=seed, iteration=iteration, mean_first=mean_first) if draws is None else np.asarray(draws, F32)
    assert a.shape == (M,) + mean.shape, a.shape
    a = a.astype(np.float64)
    d = a - P.clamp(mean).astype(np.float64)[None]
    with np.errstate(all="ignore"):
        Wt = w.sum(0)
        mu = (w * a).sum(0) / Wt
        sd = np.sqrt((w * (a - mu[None]) ** 2).sum(0) / Wt)
        return dict(mean=mu, std=sd, A1=(w * np.abs(d)).sum(0) / Wt, A2=(w * d * d).sum(0) / Wt, q=(w * d).sum(0) / Wt,
                    W=np.broadcast_to(Wt, mu.shape))


def gamma(n):
    return n * U / (1.0 - n * U)


def bounds(M, r64):
    """The float32 loop against refit64, by the standard model fl(x op y) = (x op y)(1 + delta), |delta| <= U:
    a term of s1 carries the roundings of d, of t and of at most M additions, W those of at most M additions, the quotient one more:
    |q^ - q| <= gamma(2 M + 3) A1 =: eq, and the mean adds the rounding of ctr + q.  A term of s2 carries one rounding more than one of
    s1 (all terms >= 0), so |s2/W^ - A2| <= gamma(2 M + 4) A2; q q carries 2 |q| eq + eq^2 and its own rounding; the subtraction one
    more.  With ev the sum of these, |sqrt(v^) - sqrt(v)| <= min(sqrt(ev), ev / sqrt(v)), and the square root rounds once.
    UNDERFLOW.  Weights down to the smallest subnormal participate (a softmax gives them), and then w d and (w d) d lie among the
    subnormals, where that model does not hold: a product or quotient there is fl(x op y) = (x op y)(1 + delta) + eta with
    |eta| <= ETA (sums and differences of float32 numbers are exact where they underflow, and a square root never underflows).  Each of
    the at most M terms of s1 carries one eta, and the quotient one more: eq grows by (M ETA / W)(1 + gamma(2 M + 3)) + ETA.  A term
    (w d) d of s2 carries |d| <= 2 times the eta of w d and one of its own, 3 ETA, and the quotient one more: ev grows by
    (3 M ETA / W)(1 + gamma(2 M + 4)) + ETA, and by one more ETA for the product q q."""
    A1, A2, q, sd = r64["A1"], r64["A2"], np.abs(r64["q"]), r64["std"]
    W = r64["W"]
    with np.errstate(all="ignore"):
        eq = gamma(2 * M + 3) * A1 + (M * ETA / W) * (1 + gamma(2 * M + 3)) + ETA
        e_mean = eq + U * (np.abs(r64["mean"]) + eq)
        ev = gamma(2 * M + 4) * A2 + 2 * q * eq + eq * eq + U * (q * q + 2 * q * eq + eq * eq) + U * (A2 + q * q) * (1 + gamma(2 * M + 6)) \
            + (3 * M * ETA / W) * (1 + gamma(2 * M + 4)) + 2 * ETA
        e_std = np.minimum(np.sqrt(ev), np.where(sd > 0, ev / sd, np.inf))
    return e_mean, e_std + U * (sd + e_std)
