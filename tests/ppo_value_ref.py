"""The critic's forward and the PPO value loss and gradient (include/atc_step.h: atc_value_forward, atc_ppo_value_grad) restated in numpy.
TEST INFRASTRUCTURE ONLY; needs no GPU.

  split(w, K), pack(...)     the six parts of the packed critic by name, [out, in]
  forward(w, x, K, dtype)    V of rows x [R, 10 + 7 K]: float64 (matrix products), or the float32 twin in the kernel's order (wavefronts of 64
                             consecutive rows decide on the float64 first layer)
  evaluate(case, dtype)      the contract in float64 (dtype=np.float64: matrix products, no particular order), or its float32 twin
                             (dtype=np.float32), which follows the kernel's order with ONE workgroup: the first layer an fmaf chain over the
                             inputs — in float64 for a tile of 64 rows that holds a participating input above 4 —, the second layer in four
                             partial sums, the head an fmaf chain, the data gradients as fmaf chains, the weight gradients added row by row
                             in float32, and db3 and the statistics as float32 sums per lane (rows l, l + 64, ...) folded over the lanes in
                             float64.  Returns {"grad", "stats": [8], "value": [R] (NaN where the row does not participate), "part", "cut",
                             "inside": bool [R], "delta", "e2", "ec2": [R], "n", "n_cut"}.
  bars(case)                 {part: (bar, twin deviation, largest float64 word)} for W1 .. b3, "stats" (the five means) and "value": 4 x the
                             twin's largest deviation from float64 on the same inputs, floored at 1e-6 x the part's largest float64 word.  n
                             and the cut count are exact; max |v - v_old| is a difference of float32 words and is held to "value"'s bar.
  make_case(...)             rows drawn on the CPU with a fixed seed; see there
  margins(case)              (smallest ||delta| - clip|, smallest |e^2 - ec^2| / max(e^2, ec^2) over the rows outside) over the participating
                             rows in float64
"""
import numpy as np

import policy_ref as P
from ppo_grad_ref import TILE, _fma32, _select, input_rows

STATS = 8
STAT_N, STAT_LOSS, STAT_CUT, STAT_V, STAT_RET, STAT_RET2, STAT_ERR2, STAT_DV_MAX = range(8)
MEANS = (STAT_LOSS, STAT_V, STAT_RET, STAT_RET2, STAT_ERR2)
PART_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
CLIP_MARGIN, TIE_MARGIN = 1e-4, 1e-4
HIDDEN = P.HIDDEN


def words(K=0):
    return 4289 + HIDDEN * P.n_in(K)


def shapes(K=0):
    return (("W1", (HIDDEN, P.n_in(K))), ("b1", (HIDDEN,)), ("W2", (HIDDEN, HIDDEN)), ("b2", (HIDDEN,)), ("W3", (1, HIDDEN)), ("b3", (1,)))


def split(w, K=0):
    w = np.asarray(w).reshape(-1)
    assert w.size == words(K)
    parts, at = {}, 0
    for name, shape in shapes(K):
        n = int(np.prod(shape))
        parts[name] = w[at:at + n].reshape(shape)
        at += n
    return parts


parts = split


def pack(W1, b1, W2, b2, W3, b3, K=0):
    vals = [np.asarray(v, np.float32) for v in (W1, b1, W2, b2, W3, b3)]
    for (name, shape), v in zip(shapes(K), vals):
        assert v.shape == shape, name
    return np.concatenate([v.reshape(-1) for v in vals])


def random_weights(rng, gain=1.0, K=0):
    """N(0, 1 / fan_in) times `gain` (a gain of 8 saturates tanh); biases N(0, 0.1) times gain"""
    g = lambda o, i: (rng.normal(0.0, 1.0, (o, i)) * gain / np.sqrt(i)).astype(np.float32)      # noqa: E731
    b = lambda n: (rng.normal(0.0, 0.1, n) * gain).astype(np.float32)      # noqa: E731
    return pack(g(HIDDEN, P.n_in(K)), b(HIDDEN), g(HIDDEN, HIDDEN), b(HIDDEN), g(1, HIDDEN), b(1), K)


def _hidden32(p, x):
    """h1, h2 in the kernel's order; x: [R, IN] float32 (rows that do not participate zeroed by the caller)"""
    f = np.float32
    R, n_in = x.shape
    W1, W2 = p["W1"], p["W2"]
    s = np.broadcast_to(p["b1"], (R, HIDDEN)).astype(f)
    for c in range(n_in):
        s = _fma32(W1[None, :, c], x[:, c:c + 1], s)
    wide = np.zeros(R, bool)       # the wavefronts whose first layer is summed in float64
    big = ~(np.abs(x).max(axis=1) <= 4.0)
    for t0 in range(0, R, TILE):
        wide[t0:t0 + TILE] = big[t0:t0 + TILE].any()
    if wide.any():
        sd = np.broadcast_to(p["b1"].astype(np.float64), (R, HIDDEN)).copy()
        for c in range(n_in):
            sd = W1[None, :, c].astype(np.float64) * x[:, c:c + 1].astype(np.float64) + sd
        s = np.where(wide[:, None], sd.astype(f), s)
    h1 = np.tanh(s).astype(f)
    acc = [np.broadcast_to(p["b2"], (R, HIDDEN)).astype(f)] + [np.zeros((R, HIDDEN), f) for _ in range(3)]
    for c in range(0, HIDDEN, 4):
        for q in range(4):
            acc[q] = _fma32(W2[None, :, c + q], h1[:, c + q:c + q + 1], acc[q])
    h2 = np.tanh((acc[0] + acc[1]) + (acc[2] + acc[3])).astype(f)
    return h1, h2


def _head32(p, h2):
    v = np.broadcast_to(p["b3"], (h2.shape[0],)).astype(np.float32)
    for j in range(HIDDEN):
        v = _fma32(np.broadcast_to(p["W3"][0, j], v.shape), h2[:, j], v)
    return v


def forward(w, x, K=0, dtype=np.float64):
    p = {k: v.astype(dtype) for k, v in split(w, K).items()}
    x = np.asarray(x).reshape(-1, P.n_in(K)).astype(dtype)
    with np.errstate(all="ignore"):
        if dtype == np.float32:
            return _head32(p, _hidden32(p, x)[1])
        h1 = np.tanh(x @ p["W1"].T + p["b1"])
        h2 = np.tanh(h1 @ p["W2"].T + p["b2"])
        return (h2 @ p["W3"].T + p["b3"])[:, 0]


def loss_terms(v, v_old, ret, clip):
    """(L, dL/dv, cut, inside, delta, e2, ec2) of the contract, elementwise in the dtype of v"""
    f = v.dtype.type
    clip = f(clip)
    e, d = v - ret, v - v_old
    cl = np.where(d < -clip, -clip, np.where(d > clip, clip, d)).astype(f)
    ec = (v_old + cl) - ret
    e2, ec2 = e * e, ec * ec
    inside = np.abs(d) <= clip
    cut = (np.abs(d) > clip) & (e2 < ec2)
    return f(0.5) * np.where(cut, ec2, e2), np.where(cut, f(0), e), cut, inside, d, e2, ec2


def _lane_fold(values, part, tiles_run, integer=False):
    """float32 sums per lane over the tiles a single workgroup runs (a row that does not participate adds nothing), folded in float64"""
    R = values.shape[0]
    lanes = np.zeros(TILE, np.float32)
    for t0 in range(0, R, TILE):
        if not tiles_run[t0 // TILE]:
            continue
        v, m = values[t0:t0 + TILE], part[t0:t0 + TILE]
        k = v.shape[0]
        lanes[:k] = np.where(m, (lanes[:k] + v).astype(np.float32), lanes[:k])
    return np.float32(lanes.astype(np.float64).sum())


def evaluate(case, dtype=np.float64):
    K = int(case.get("K", 0))
    f = dtype
    twin = dtype == np.float32
    p = {k: v.astype(f) for k, v in split(case["w"], K).items()}
    src, part = _select(case)
    R = src.shape[0]
    rows = input_rows(case["obs_rows"], case.get("traffic"), K)
    x = np.where(part[:, None], rows[src], 0).astype(f)
    v_old = np.where(part, np.asarray(case["v_old"]).reshape(-1)[src], 0).astype(f)
    ret = np.where(part, np.asarray(case["ret"]).reshape(-1)[src], 0).astype(f)
    clip = f(np.float32(case.get("clip", 0.2)))
    one = f(1.0)
    n = int(part.sum())
    with np.errstate(all="ignore"):
        if twin:
            h1, h2 = _hidden32(p, x)
            v = _head32(p, h2)
        else:
            h1 = np.tanh(x @ p["W1"].T + p["b1"])
            h2 = np.tanh(h1 @ p["W2"].T + p["b2"])
            v = (h2 @ p["W3"].T + p["b3"])[:, 0]
        loss, dldv, cut, inside, delta, e2, ec2 = loss_terms(v, v_old, ret, clip)
        cut = cut & part
        dv = np.where(part, dldv, 0).astype(f)
        err2 = (ret - v) * (ret - v)
        if twin:
            tiles_run = [bool(part[t0:t0 + TILE].any()) for t0 in range(0, R, TILE)]
            dh2 = (p["W3"][0][None, :] * dv[:, None]).astype(f)
            dz2 = (dh2 * (one - h2 * h2)).astype(f)
            dh1 = np.zeros((R, HIDDEN), f)
            for j in range(HIDDEN):
                dh1 = _fma32(p["W2"][None, j, :], dz2[:, j:j + 1], dh1)
            dz1 = (dh1 * (one - h1 * h1)).astype(f)
            g = {"W1": np.zeros_like(p["W1"]), "b1": np.zeros_like(p["b1"]), "W2": np.zeros_like(p["W2"]), "b2": np.zeros_like(p["b2"]),
                 "W3": np.zeros_like(p["W3"])}
            for r in range(R):      # row by row, in the kernel's order (one workgroup)
                if not tiles_run[r // TILE]:
                    continue
                g["W3"] = _fma32(np.broadcast_to(dv[r], (1, HIDDEN)), h2[r][None, :], g["W3"])
                g["W2"] = _fma32(dz2[r][:, None], h1[r][None, :], g["W2"])
                g["b2"] = (g["b2"] + dz2[r]).astype(f)
                g["W1"] = _fma32(dz1[r][:, None], x[r][None, :], g["W1"])
                g["b1"] = (g["b1"] + dz1[r]).astype(f)
            every = np.ones(R, bool)
            g["b3"] = np.array([_lane_fold(dv, every, tiles_run)], f)
            sums = {q: _lane_fold(a.astype(f), part, tiles_run) for q, a in ((STAT_LOSS, loss), (STAT_V, v), (STAT_RET, ret), (STAT_RET2, ret * ret), (STAT_ERR2, err2))}
        else:
            dz2 = (dv[:, None] * p["W3"]) * (one - h2 * h2)
            dz1 = (dz2 @ p["W2"]) * (one - h1 * h1)
            g = {"W1": dz1.T @ x, "b1": dz1.sum(0), "W2": dz2.T @ h1, "b2": dz2.sum(0), "W3": dv[None, :] @ h2, "b3": dv.sum(keepdims=True)}
            sums = {q: a[part].sum() for q, a in ((STAT_LOSS, loss), (STAT_V, v), (STAT_RET, ret), (STAT_RET2, ret * ret), (STAT_ERR2, err2))}
        grad = np.concatenate([np.asarray(g[name], f).reshape(-1) for name in PART_NAMES])
        stats = np.zeros(STATS, f)
        n_cut = int(cut.sum())
        if n:
            grad = (grad / f(n)).astype(f)
            stats[STAT_N] = n
            stats[STAT_CUT] = f(n_cut) / f(n)
            for q, s in sums.items():
                stats[q] = f(s) / f(n)
            stats[STAT_DV_MAX] = np.fmax.reduce(np.abs(delta[part]), initial=f(0))
        else:
            grad = np.zeros_like(grad)
    return {"grad": grad, "stats": stats, "value": np.where(part, v, np.nan).astype(f), "part": part, "cut": cut, "inside": inside & part, "delta": delta,
            "e2": e2, "ec2": ec2, "n": n, "n_cut": n_cut}


def bars(case, ref64=None, ref32=None):
    K = int(case.get("K", 0))
    ref64 = evaluate(case, np.float64) if ref64 is None else ref64
    ref32 = evaluate(case, np.float32) if ref32 is None else ref32
    out = {}
    g64, g32 = split(ref64["grad"], K), split(ref32["grad"].astype(np.float64), K)
    for name in PART_NAMES:
        top = float(np.max(np.abs(g64[name])))
        dev = float(np.max(np.abs(g32[name] - g64[name])))
        out[name] = (max(4.0 * dev, 1e-6 * top), dev, top)
    own = list(MEANS)
    for name, a, b in (("stats", ref32["stats"][own].astype(np.float64), ref64["stats"][own]),
                       ("value", ref32["value"][ref64["part"]].astype(np.float64), ref64["value"][ref64["part"]])):
        top = float(np.max(np.abs(b))) if b.size else 0.0
        dev = float(np.max(np.abs(a - b))) if b.size else 0.0
        out[name] = (max(4.0 * dev, 1e-6 * top), dev, top)
    return out


def forward_bar(w, x, K=0):
    """(bar, deviation, V in float64) of the forward alone: 4 x the twin's largest deviation, floored at 1e-6 x the largest |V|"""
    v64 = forward(w, x, K, np.float64)
    dev = float(np.max(np.abs(forward(w, x, K, np.float32).astype(np.float64) - v64)))
    return max(4.0 * dev, 1e-6 * float(np.max(np.abs(v64)))), dev, v64


def margins(case, ref64=None):
    ref = evaluate(case, np.float64) if ref64 is None else ref64
    part = ref["part"]
    clip = np.float64(np.float32(case.get("clip", 0.2)))
    if not part.any() or not np.isfinite(clip):
        return np.inf, np.inf
    d = np.abs(ref["delta"][part])
    outside = d > clip
    e2, ec2 = ref["e2"][part][outside], ref["ec2"][part][outside]
    tie = float((np.abs(e2 - ec2) / np.maximum(e2, ec2)).min()) if outside.any() else np.inf
    return float(np.abs(d - clip).min()), tie


def make_case(seed, R, K=0, gain=1.0, raw=False, mask=False, index=False, clip=0.2):
    """One case of R rows to evaluate.  Weights N(0, 1 / fan_in) x gain; input words U(-1, 1), with raw=True a third of the rows carry words
    of magnitude up to 1.5e4 (the unnormalised observation); v_old = V + noise and ret = V + noise, each noise of magnitude U(0.05, 1) with
    a random sign, so that rows inside the clip range, rows outside whose gradient flows and rows that are cut all occur.
    mask=True: a quarter of the source rows are masked out.  index=True: R_src = R + 37 source rows, index a random draw of them with
    repeats plus, for R > 8, entries out of range (-1, R_src, 2^31 - 1, -2^31) at fixed places.  Rows whose float64 |delta| lies within
    2e-4 of clip, and rows outside with |e^2 - ec^2| < 2e-4 max(e^2, ec^2), have v_old (ret) nudged until none is left: in float32 a row
    may then not fall on the other side of a branch."""
    rng = np.random.default_rng(seed)
    R_src = R + 37 if index else R
    n_in = P.n_in(K)
    w = random_weights(rng, gain=gain, K=K)
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
    v = forward(w, xin, K, np.float64)
    noise = lambda: rng.uniform(0.05, 1.0, R_src) * rng.choice((-1.0, 1.0), R_src)      # noqa: E731
    v_old = (v + noise()).astype(np.float32)
    ret = (v + noise()).astype(np.float32)
    case = {"K": K, "w": w, "obs_rows": obs_rows, "traffic": traffic, "v_old": v_old, "ret": ret, "clip": clip, "mask": None, "index": None,
            "R": R, "R_src": R_src}
    if mask:
        case["mask"] = (rng.random(R_src) >= 0.25).astype(np.uint8)
    if index:
        idx = rng.integers(0, R_src, R).astype(np.int32)
        if R > 8:
            for at, bad in zip(range(1, R, R // 4), (-1, R_src, 2 ** 31 - 1, -2 ** 31)):
                idx[at] = bad
            idx[-1] = idx[0]      # a repeated row
        case["index"] = idx
    c = np.float64(np.float32(clip))
    if np.isfinite(c):
        for _ in range(50):
            ref = evaluate(case, np.float64)
            src, part = _select(case)
            d = np.abs(ref["delta"])
            near = part & (np.abs(d - c) < 2.0 * CLIP_MARGIN)
            tie = part & (d > c) & (np.abs(ref["e2"] - ref["ec2"]) < 2.0 * TIE_MARGIN * np.maximum(ref["e2"], ref["ec2"]))
            if not near.any() and not tie.any():
                break
            case["v_old"][src[near]] += np.float32(1e-3)
            case["ret"][src[tie]] += np.float32(1e-2)
    return case
