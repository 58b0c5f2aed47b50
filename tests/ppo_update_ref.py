"""numpy restatement of atc_adv_normalise and atc_adam_step (include/atc_step.h) IN THE KERNELS' OPERATION ORDER: float64 arithmetic, every
product and every sum rounded on its own, each stored word rounded to float32 once.  The kernels (csrc/atc_ppo_update.inc) are held to it bit
for bit (tests/test_z_ppo_update.py); the restatement itself is held to plain numpy moments and to torch.optim.Adam in float64 there.

adv_normalise: G workgroups take the tiles of 256 rows g, g + G, ...; lane l adds its row of each tile in tile order (n, S, S2); lane 0 adds
the 256 lanes' triples in lane order; the G triples are added in the order of g.
adam_step: one workgroup of 1 024 lanes over the concatenated words; lane l adds ge^2 over j = l, l + 1024, ...; the 1 024 sums are added in
lane order."""
import numpy as np

TILE, DEFAULT_WG, MAX_WG = 256, 256, 1024
ADV_STATS = 4
STAT_N, STAT_MEAN, STAT_SCALE, STAT_STD = range(4)
ADAM_BLOCK, ADAM_MAX_WORDS, ADAM_STATS = 1024, 65536, 4
ASTAT_NORM, ASTAT_COEF, ASTAT_SKIPPED, ASTAT_STEP = range(4)


def workgroups(R, G=0):
    return int(G) if G else min((int(R) + TILE - 1) // TILE, DEFAULT_WG)


def _fold(columns):
    """the rows of a float64 [k, lanes] array added in row order per lane, then the lanes in lane order: one python float"""
    lanes = np.zeros(columns.shape[1], np.float64)
    for row in columns:
        lanes = lanes + row
    total = 0.0
    for x in lanes.tolist():
        total += x
    return total


def adv_moments(adv, mask=None, G=0):
    """[G, 3] float64: the partial triples {n, S, S2} as k_adv_moments writes them"""
    a = np.asarray(adv, np.float32).reshape(-1)
    R = a.size
    part = np.ones(R, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    G = workgroups(R, G)
    tiles = (R + TILE - 1) // TILE
    pad = tiles * TILE - R
    ad = np.concatenate([np.where(part, a, np.float32(0)).astype(np.float64), np.zeros(pad)]).reshape(tiles, TILE)
    pd = np.concatenate([part.astype(np.float64), np.zeros(pad)]).reshape(tiles, TILE)
    out = np.zeros((G, 3), np.float64)
    for g in range(G):
        mine = slice(g, tiles, G)
        if ad[mine].shape[0]:
            out[g] = (_fold(pd[mine]), _fold(ad[mine]), _fold(ad[mine] * ad[mine]))
    return out


def adv_normalise(adv, mask=None, eps=1e-8, G=0):
    """{"adv": float32 of adv's shape, "stats": float32 [4], "n", "mean", "std": the float64 values, "scratch": [G, 3]}"""
    a = np.asarray(adv, np.float32)
    part = np.ones(a.size, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    scratch = adv_moments(a, mask, G)
    n = S = S2 = 0.0
    for g in range(scratch.shape[0]):
        n += float(scratch[g, 0])
        S += float(scratch[g, 1])
        S2 += float(scratch[g, 2])
    mean = std = 0.0
    shift = scale = np.float32(0)
    if n > 0:
        mean = S / n
        var = 0.0
        if n > 1:
            c = S2 - S * mean
            var = (c if c > 0.0 else 0.0) / (n - 1.0)
        std = float(np.sqrt(np.float64(var)))
        shift = np.float32(mean)
        with np.errstate(over="ignore", divide="ignore"):
            scale = np.float32(np.float64(1.0) / (np.float64(std) + np.float64(np.float32(eps))))
    with np.errstate(invalid="ignore", over="ignore"):
        z = (np.where(part, a.reshape(-1), np.float32(0)) - shift) * scale
    out = np.where(part & (n > 0), z, np.float32(0)).astype(np.float32).reshape(a.shape)
    stats = np.array([np.float32(n), shift, scale, np.float32(std)], np.float32)
    return {"adv": out, "stats": stats, "n": n, "mean": mean, "std": std, "scratch": scratch}


def effective_grad(t):
    """float64 [words]: grad_scale * grad + the add window's value"""
    g = np.asarray(t["grad"]).astype(np.float64).reshape(-1)
    ge = np.float64(np.float32(t.get("grad_scale", 1.0))) * g
    first, count, value = t.get("add") or (0, 0, 0.0)
    add = np.zeros(g.size, np.float64)
    add[first:first + count] = np.float64(np.float32(value))
    return ge + add


def grad_norm(tensors):
    """(norm, total) of the effective gradients of all tensors, summed as k_adam_step sums them"""
    ge = np.concatenate([effective_grad(t) for t in tensors])
    sq = ge * ge
    pad = -sq.size % ADAM_BLOCK
    total = _fold(np.concatenate([sq, np.zeros(pad)]).reshape(-1, ADAM_BLOCK))
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(np.float64(total))), total


def adam_step(tensors, lr, step, beta1=0.9, beta2=0.999, eps=1e-5, max_norm=0.0, store=np.float32):
    """One atc_adam_step on `tensors` (a list of dicts "w", "grad", "m", "v" and optionally "grad_scale", "add" = (first, count, value)):
    returns (new tensors — the same dicts with w, m, v replaced, arrays of dtype `store` —, stats float32 [4]).  store=np.float64 keeps the
    stored words unrounded: the restatement without the float32 stores."""
    assert 1 <= len(tensors) <= 2 and step >= 1
    lr, beta1, beta2, eps, max_norm = (float(x) for x in (lr, beta1, beta2, eps, max_norm))
    norm, _ = grad_norm(tensors)
    finite = bool(np.isfinite(norm))
    coef = 1.0
    if 0.0 < max_norm < float("inf"):
        c = max_norm / (norm + 1e-6)
        coef = c if c < 1.0 else 1.0
    stats = np.array([np.float32(norm), np.float32(coef) if finite else 0.0, 0.0 if finite else 1.0, np.float32(step)], np.float32)
    if not finite:
        return [dict(t) for t in tensors], stats
    c1, c2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    step_size, root_c2 = lr / c1, float(np.sqrt(np.float64(c2)))
    out = []
    for t in tensors:
        gc = effective_grad(t) * coef
        m = (beta1 * np.asarray(t["m"]).astype(np.float64) + (1.0 - beta1) * gc).astype(store)
        v = (beta2 * np.asarray(t["v"]).astype(np.float64) + ((1.0 - beta2) * gc) * gc).astype(store)
        denom = np.sqrt(v.astype(np.float64)) / root_c2 + eps
        w = (np.asarray(t["w"]).astype(np.float64) - step_size * (m.astype(np.float64) / denom)).astype(store)
        out.append(dict(t, w=w, m=m, v=v))
    return out, stats
