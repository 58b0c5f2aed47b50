"""The PPO policy loss and gradient (include/atc_step.h: atc_ppo_policy_grad) restated in numpy.  TEST INFRASTRUCTURE ONLY; needs no GPU.

  evaluate(case, dtype)      the contract in float64 (dtype=np.float64: matrix products, no particular order), or its float32 twin
                             (dtype=np.float32), which follows the kernel's order: the first layer an fmaf chain over the inputs — in
                             float64 for a tile of 64 rows that holds a participating input above 4 —, the second layer in four partial
                             sums, the data gradients as fmaf chains, and the weight gradients added row by row in float32.  Returns
                             {"grad": packed float array, "stats": [8], "logp": [R] (NaN where the row does not participate), "part", "cut":
                             bool [R], "ratio", "A": [R]}.
  parts(grad, K)             the seven parts of a packed gradient by name (policy_ref.split)
  bars(case)                 {part: (bar, twin deviation, largest float64 word)} for W1 .. log_std, "stats" (mean L and mean ratio; the two
                             statistics of logp - logp_old are held to "logp", see STATS_OF_LOGP) and "logp": 4 x the twin's
                             largest deviation from float64 on the same inputs, floored at 1e-6 x the part's largest float64 word
                             (section 3k's rule for mu: the reference sets the bar, never the kernel)
  make_case(...)             rows drawn on the CPU with a fixed seed; see there
  margins(case)              (smallest |ratio - (1 +- clip)|, smallest |A|) over the participating rows in float64
"""
import numpy as np

import policy_ref as P

STATS = 8
STAT_N, STAT_LOSS, STAT_KL, STAT_CUT, STAT_RATIO, STAT_DLOGP_MAX = range(6)
TILE = 64
PART_NAMES = tuple(n for n, _ in P.SHAPES)
RATIO_MARGIN, ADV_MARGIN = 1e-4, 1e-6
# The statistics that are sums or maxima of logp - logp_old with unit coefficients: a float32 logp of magnitude 10 is a multiple of 9.5e-7, so
# these two words carry logp's absolute error whatever their own size (with unchanged weights they are 1e-6 themselves) and are held to
# logp's bar; mean L and mean ratio have the bar of their own size.
STATS_OF_LOGP = (STAT_KL, STAT_DLOGP_MAX)


def parts(grad, K=0):
    return P.split(np.asarray(grad), K)


def input_rows(obs_rows, traffic, K):
    obs_rows = np.asarray(obs_rows)
    if not K:
        return obs_rows.reshape(-1, P.IN)
    tr = np.asarray(traffic).reshape(obs_rows.reshape(-1, P.IN).shape[0], K, 8)
    return np.concatenate([obs_rows.reshape(-1, P.IN), tr[:, :, :P.RECORD_INPUTS].reshape(-1, K * P.RECORD_INPUTS)], axis=1)


def _select(case):
    """(src [R] clipped into range, part [R] bool): which source row each row evaluates and whether it participates"""
    R_src = np.asarray(case["obs_rows"]).reshape(-1, P.IN).shape[0]
    index = case.get("index")
    if index is None:
        src, part = np.arange(R_src), np.ones(R_src, bool)
    else:
        idx = np.asarray(index).astype(np.int64)
        part = (idx >= 0) & (idx < R_src)
        src = np.where(part, idx, 0)
    if case.get("mask") is not None:
        part = part & (np.asarray(case["mask"]).reshape(-1)[src] != 0)
    return src, part


def surrogate(ratio, A, clip):
    """(L, flows) of the contract, elementwise in the dtype of `ratio`: L = -min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A); the gradient
    flows through the unclipped term, dL/dratio = -A, iff (A >= 0 and ratio <= 1 + clip) or (A < 0 and ratio >= 1 - clip), and is 0 otherwise"""
    f = ratio.dtype.type
    lo, hi = f(1.0) - f(clip), f(1.0) + f(clip)
    clamped = np.where(ratio < lo, lo, np.where(ratio > hi, hi, ratio)).astype(f)
    t1, t2 = ratio * A, clamped * A
    return -np.where(t1 < t2, t1, t2), np.where(A >= 0, ~(ratio > hi), ~(ratio < lo))


def _fma32(a, b, s):
    """fmaf on float32 arrays: the product is exact in float64, one rounding to float64 and one to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + s.astype(np.float64)).astype(np.float32)


def _forward32(p, x, part):
    """h1, h2, mu in the kernel's order; x: [R, IN] float32 with the rows that do not participate zeroed"""
    f = np.float32
    R, n_in = x.shape
    W1, W2, W3 = p["W1"], p["W2"], p["W3"]
    s = np.broadcast_to(p["b1"], (R, P.HIDDEN)).astype(f)
    for c in range(n_in):
        s = _fma32(W1[None, :, c], x[:, c:c + 1], s)
    wide = np.zeros(R, bool)       # the tiles whose first layer is summed in float64
    big = ~(np.abs(x).max(axis=1) <= 4.0)
    for t0 in range(0, R, TILE):
        wide[t0:t0 + TILE] = big[t0:t0 + TILE].any()
    if wide.any():
        sd = np.broadcast_to(p["b1"].astype(np.float64), (R, P.HIDDEN)).copy()
        for c in range(n_in):
            sd = W1[None, :, c].astype(np.float64) * x[:, c:c + 1].astype(np.float64) + sd
        s = np.where(wide[:, None], sd.astype(f), s)
    h1 = np.tanh(s).astype(f)
    acc = [np.broadcast_to(p["b2"], (R, P.HIDDEN)).astype(f)] + [np.zeros((R, P.HIDDEN), f) for _ in range(3)]
    for c in range(0, P.HIDDEN, 4):
        for q in range(4):
            acc[q] = _fma32(W2[None, :, c + q], h1[:, c + q:c + q + 1], acc[q])
    h2 = np.tanh((acc[0] + acc[1]) + (acc[2] + acc[3])).astype(f)
    mu = np.broadcast_to(p["b3"], (R, P.ACT)).astype(f)
    for j in range(P.HIDDEN):
        mu = _fma32(W3[None, :, j], h2[:, j:j + 1], mu)
    return h1, h2, mu


def evaluate(case, dtype=np.float64):
    K = int(case.get("K", 0))
    f = dtype
    twin = dtype == np.float32
    p = {k: v.astype(f) for k, v in P.split(case["w"], K).items()}
    src, part = _select(case)
    R = src.shape[0]
    rows = input_rows(case["obs_rows"], case.get("traffic"), K)
    x = np.where(part[:, None], rows[src], 0).astype(f)
    u = np.where(part[:, None], np.asarray(case["action"]).reshape(-1, 3)[src], 0).astype(f)
    lp_old = np.where(part, np.asarray(case["logp_old"]).reshape(-1)[src], 0).astype(f)
    adv = np.where(part, np.asarray(case["adv"]).reshape(-1)[src], 0).astype(f)
    clip, shift, scale = (f(np.float32(case.get(k, d))) for k, d in (("clip", 0.2), ("adv_shift", 0.0), ("adv_scale", 1.0)))
    with np.errstate(all="ignore"):
        if twin:
            h1, h2, mu = _forward32(p, x, part)
        else:
            h1 = np.tanh(x @ p["W1"].T + p["b1"])
            h2 = np.tanh(h1 @ p["W2"].T + p["b2"])
            mu = h2 @ p["W3"].T + p["b3"]
        ls = p["log_std"]
        sigma = np.exp(ls).astype(f)
        d = ((u - mu) / sigma).astype(f)
        lp = np.zeros(R, f)
        for c in range(3):
            lp = (lp + (f(-0.5) * (d[:, c] * d[:, c]) - ls[c])).astype(f)
        logp = (lp - f(P.LOGP_C)).astype(f)
        dlogp = (logp - lp_old).astype(f)
        ratio = np.exp(dlogp).astype(f)
        A = ((adv - shift) * scale).astype(f)
        loss, flows = surrogate(ratio, A, clip)
        gl = np.where(flows, -(A * ratio), 0).astype(f)
        dmu = np.where(part[:, None], gl[:, None] * (d / sigma), 0).astype(f)
        dls = np.where(part[:, None], gl[:, None] * (d * d - f(1.0)), 0).astype(f)
        one = f(1.0)
        if twin:
            dh2 = np.zeros((R, P.HIDDEN), f)
            for k in range(3):
                dh2 = _fma32(p["W3"][None, k, :], dmu[:, k:k + 1], dh2)
            dz2 = (dh2 * (one - h2 * h2)).astype(f)
            dh1 = np.zeros((R, P.HIDDEN), f)
            for j in range(P.HIDDEN):
                dh1 = _fma32(p["W2"][None, j, :], dz2[:, j:j + 1], dh1)
            dz1 = (dh1 * (one - h1 * h1)).astype(f)
            g = {"W1": np.zeros_like(p["W1"]), "b1": np.zeros_like(p["b1"]), "W2": np.zeros_like(p["W2"]), "b2": np.zeros_like(p["b2"]),
                 "W3": np.zeros_like(p["W3"])}
            for r in range(R):      # row by row, in the kernel's order (one workgroup)
                if not part[r // TILE * TILE:(r // TILE + 1) * TILE].any():
                    continue
                g["W3"] = _fma32(dmu[r][:, None], h2[r][None, :], g["W3"])
                g["W2"] = _fma32(dz2[r][:, None], h1[r][None, :], g["W2"])
                g["b2"] = (g["b2"] + dz2[r]).astype(f)
                g["W1"] = _fma32(dz1[r][:, None], x[r][None, :], g["W1"])
                g["b1"] = (g["b1"] + dz1[r]).astype(f)
            g["b3"] = dmu.astype(np.float64).sum(0).astype(f)
            g["log_std"] = dls.astype(np.float64).sum(0).astype(f)
        else:
            dz2 = (dmu @ p["W3"]) * (one - h2 * h2)
            dz1 = (dz2 @ p["W2"]) * (one - h1 * h1)
            g = {"W1": dz1.T @ x, "b1": dz1.sum(0), "W2": dz2.T @ h1, "b2": dz2.sum(0), "W3": dmu.T @ h2, "b3": dmu.sum(0), "log_std": dls.sum(0)}
        n = int(part.sum())
        grad = np.concatenate([np.asarray(g[name], f).reshape(-1) for name in PART_NAMES])
        stats = np.zeros(STATS, f)
        if n:
            grad = (grad / f(n)).astype(f)
            acc = np.float64 if twin else f
            stats[:6] = [n, loss[part].astype(acc).sum() / n, (-dlogp[part]).astype(acc).sum() / n, int((part & ~flows).sum()) / n,
                         ratio[part].astype(acc).sum() / n, np.abs(dlogp[part]).max()]
        else:
            grad = np.zeros_like(grad)
    return {"grad": grad, "stats": stats, "logp": np.where(part, logp, np.nan).astype(f), "part": part, "cut": part & ~flows, "ratio": ratio, "A": A,
            "n": n, "n_cut": int((part & ~flows).sum())}


def bars(case, ref64=None, ref32=None):
    K = int(case.get("K", 0))
    ref64 = evaluate(case, np.float64) if ref64 is None else ref64
    ref32 = evaluate(case, np.float32) if ref32 is None else ref32
    out = {}
    g64, g32 = parts(ref64["grad"], K), parts(ref32["grad"].astype(np.float64), K)
    for name in PART_NAMES:
        top = float(np.max(np.abs(g64[name])))
        dev = float(np.max(np.abs(g32[name] - g64[name])))
        out[name] = (max(4.0 * dev, 1e-6 * top), dev, top)
    own = [STAT_LOSS, STAT_RATIO]      # (n and the cut count are exact; KL and max |dlogp| are differences of logp words: STATS_OF_LOGP)
    for name, a, b in (("stats", ref32["stats"][own].astype(np.float64), ref64["stats"][own]),
                       ("logp", ref32["logp"][ref64["part"]].astype(np.float64), ref64["logp"][ref64["part"]])):
        top = float(np.max(np.abs(b))) if b.size else 0.0
        dev = float(np.max(np.abs(a - b))) if b.size else 0.0
        out[name] = (max(4.0 * dev, 1e-6 * top), dev, top)
    return out


def margins(case, ref64=None):
    ref = evaluate(case, np.float64) if ref64 is None else ref64
    part = ref["part"]
    if not part.any():
        return np.inf, np.inf
    clip = np.float64(np.float32(case.get("clip", 0.2)))
    r = ref["ratio"][part]
    return float(np.minimum(np.abs(r - (1.0 - clip)), np.abs(r - (1.0 + clip))).min()), float(np.abs(ref["A"][part]).min())


def make_case(seed, R, K=0, gain=1.0, log_std=0.0, raw=False, mask=False, index=False, clip=0.2, normalise=True):
    """One case of R rows to evaluate.  Weights N(0, 1 / fan_in) x gain, log_std the same for the three components; input words U(-1, 1),
    with raw=True a third of the rows carry words of magnitude up to 1.5e4 (the unnormalised observation); actions mu + sigma z; logp_old
    such that the ratios spread over [0.5, 2]; adv N(0.3, 2) with shift and scale its masked mean and 1 / std (normalise=True).
    mask=True: a quarter of the source rows are masked out.  index=True: R_src = R + 37 source rows, index a random draw of them with
    repeats plus, for R > 8, entries out of range (-1, R_src, 2^31 - 1, -2^31) at fixed places.  Rows whose float64 ratio lies within 1e-4 of a clip
    boundary have logp_old nudged, rows with |A| < 1e-6 have adv nudged, until none is left: in float32 a row may then not fall on the
    other side of a boundary."""
    rng = np.random.default_rng(seed)
    R_src = R + 37 if index else R
    n_in = P.n_in(K)
    w = P.random_weights(rng, gain=gain, log_std=(log_std,) * 3, K=K)
    xin = rng.uniform(-1.0, 1.0, (R_src, n_in)).astype(np.float32)
    if raw:
        rows = rng.random(R_src) < 1.0 / 3.0
        rows[0] = True
        scale = np.where(rng.random((R_src, n_in)) < 0.3, 1.5e4, 40.0)
        xin = np.where(rows[:, None], (xin * scale).astype(np.float32), xin)
    obs_rows = np.ascontiguousarray(xin[:, :P.IN])
    traffic = None
    if K:
        traffic = np.zeros((R_src, K, 8), np.float32)
        traffic[:, :, :P.RECORD_INPUTS] = xin[:, P.IN:].reshape(R_src, K, P.RECORD_INPUTS)
        traffic[:, :, 7] = rng.integers(0, 64, (R_src, K)).astype(np.float32)      # the slot: not an input
    mu = P.mlp(w, xin, K, np.float64)
    z = rng.normal(0.0, 1.0, (R_src, 3))
    action = (mu + np.exp(log_std) * z).astype(np.float32)
    d = (action.astype(np.float64) - mu) / np.exp(np.float64(np.float32(log_std)))
    logp = P.logp64(d, np.full(3, np.float32(log_std), np.float64))
    target = np.exp(rng.uniform(np.log(0.5), np.log(2.0), R_src))
    logp_old = (logp - np.log(target)).astype(np.float32)
    adv = rng.normal(0.3, 2.0, R_src).astype(np.float32)
    case = {"K": K, "w": w, "obs_rows": obs_rows, "traffic": traffic, "action": action, "logp_old": logp_old, "adv": adv, "clip": clip,
            "mask": None, "index": None, "adv_shift": 0.0, "adv_scale": 1.0, "R": R, "R_src": R_src}
    if mask:
        m = (rng.random(R_src) >= 0.25).astype(np.uint8)
        case["mask"] = m
    if index:
        idx = rng.integers(0, R_src, R).astype(np.int32)
        if R > 8:
            for at, bad in zip(range(1, R, R // 4), (-1, R_src, 2 ** 31 - 1, -2 ** 31)):
                idx[at] = bad
            idx[-1] = idx[0]      # a repeated row
        case["index"] = idx
    if normalise:
        _, part = _select(case)
        src, _ = _select(case)
        a = adv[src][part].astype(np.float64)
        if a.size > 1 and a.std() > 0:
            case["adv_shift"], case["adv_scale"] = float(np.float32(a.mean())), float(np.float32(1.0 / (a.std() + 1e-8)))
    for _ in range(50):
        ref = evaluate(case, np.float64)
        src, part = _select(case)
        c = np.float64(np.float32(clip))
        near = part & (np.minimum(np.abs(ref["ratio"] - (1.0 - c)), np.abs(ref["ratio"] - (1.0 + c))) < 2.0 * RATIO_MARGIN)
        flat = part & (np.abs(ref["A"]) < 2.0 * ADV_MARGIN)
        if not near.any() and not flat.any():
            break
        case["logp_old"][src[near]] += np.float32(1e-3)
        case["adv"][src[flat]] += np.float32(1e-3)
    return case
