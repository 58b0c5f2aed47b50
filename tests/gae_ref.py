"""atc_gae (include/atc_step.h) restated in numpy: the block fold and the recurrence in np.float32, operation by operation in the header's
order (numpy rounds every float32 product and sum once and fuses nothing), vectorised over the columns only — the loops over d and j
are the header's.  gae(..., dtype=np.float64) is the TWIN: the same operations on the same inputs (gamma and lam as the float32 values
the library reads) in float64.

THE RUNNING ERROR BOUND (gae(..., with_bound=True), float32 only).  Every fp32 operation returns fl(x) = x (1 + e) with |e| <= u = 2^-24
(round to nearest; results here stay far above the subnormals), so it adds at most u |fl(x)| to the error its operands carry.  To first
order in u the deviation of an output word from the exact evaluation of the same formula is therefore at most

    u * S,    S = the sum of the magnitudes of every ROUNDED intermediate in the word's dependency chain:

the running products g_j (not g_1 = 1.0f * gamma, which is exact), each r * g and each partial sum R of the word's block (R = r_{t0} is
assigned, not rounded); for a block that did not end its episode G's products, G * V[d+1], R + G V[d+1], delta, c (with G's chain),
c * A_next and the whole chain of A_next; A itself; for ret also A + V[d].  S is accumulated next to the values, per element, from the
float32 intermediates the restatement actually produced — it is not a fixed number.  The float64 twin's own rounding is 2^-29 of that
and is left out.  (The inputs are exact in both evaluations; `term` and n are integers and agree.)"""
import numpy as np

QNAN = 0x7FC00000
U = 2.0 ** -24


def words(a):
    """the 32-bit (float32) or 8-bit words of an array, to compare bit for bit"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


def _stored(a):
    """a float32 result as the library stores it: every NaN is the quiet NaN 0x7FC00000"""
    a = np.array(a, dtype=np.float32)
    a.view(np.uint32)[np.isnan(a)] = QNAN
    return a


def constants(hold, gamma, lam, per_decision=False, dtype=np.float32):
    """(G, c, S_G, S_c): the two launch constants and the magnitude sums of their rounded intermediates"""
    f = dtype
    gam, lm = f(np.float32(gamma)), f(np.float32(lam))
    with np.errstate(all="ignore"):
        G, S_G = gam, 0.0
        if not per_decision:
            g = f(1.0)
            for j in range(int(hold)):
                g = f(g * gam)
                S_G += abs(float(g)) if j else 0.0       # (1.0f * gamma is exact)
            G = g
        c = f(G * lm)
    return G, c, S_G, S_G + abs(float(c))


def gae(reward, done, values, hold=1, gamma=0.99, lam=0.95, per_decision=False, adv_next=None, dtype=np.float32, with_bound=False):
    """reward [T, B] or [T, B, NV] (the shape selects the per-column reward), done [T, B], values [D + 1, B, NV] or [D + 1, B], T = D * hold,
    adv_next None or [B, NV] / [B].  Returns {"adv", "ret": values' shape with D rows, "block_reward": [D, B] ([D, B, NV] per column),
    "block_done", "block_steps": [D, B] uint8}; in float32 the NaNs are stored as QNAN.  with_bound: also "adv_bound", "ret_bound"."""
    f = dtype
    values = np.asarray(values)
    flat = values.ndim == 2
    V = values.reshape(values.shape[0], values.shape[1], -1).astype(f)
    D, B, NV = V.shape[0] - 1, V.shape[1], V.shape[2]
    hold = int(hold)
    T = D * hold
    reward = np.asarray(reward)
    per_column = reward.ndim == 3
    r = reward.reshape(T, B, NV if per_column else 1).astype(f)
    dn = (np.asarray(done).reshape(T, B) != 0)[:, :, None]
    gam = f(np.float32(gamma))
    G, c, S_G, S_c = constants(hold, gamma, lam, per_decision, f)
    A_next = np.zeros((B, NV), f) if adv_next is None else np.asarray(adv_next).reshape(B, NV).astype(f)
    S_next = np.zeros((B, NV))
    adv, ret = np.zeros((D, B, NV), f), np.zeros((D, B, NV), f)
    adv_b, ret_b = np.zeros((D, B, NV)), np.zeros((D, B, NV))
    block_reward = np.zeros((D, B, r.shape[2]), f)
    block_done, block_steps = np.zeros((D, B), np.uint8), np.zeros((D, B), np.uint8)
    mag = lambda x: np.abs(x.astype(np.float64))      # noqa: E731
    with np.errstate(all="ignore"):
        for d in range(D - 1, -1, -1):
            t0 = d * hold
            # the block
            g = np.ones_like(r[t0])
            R = r[t0].copy()
            n = np.ones((B, 1), np.int64)
            term = dn[t0].copy()
            S_g, S_R = np.zeros(R.shape), np.zeros(R.shape)
            for j in range(1, hold):
                is_open = ~term
                if per_decision:
                    R1 = R + r[t0 + j]
                    S_R1 = S_R + mag(R1)
                else:
                    g1 = g * gam
                    S_g1 = S_g + (mag(g1) if j > 1 else 0.0)
                    p = r[t0 + j] * g1
                    R1 = R + p
                    S_R1 = S_R + S_g1 + mag(p) + mag(R1)
                    g = np.where(is_open, g1, g)
                    S_g = np.where(is_open, S_g1, S_g)
                R = np.where(is_open, R1, R)
                S_R = np.where(is_open, S_R1, S_R)
                n = np.where(is_open, n + 1, n)
                term = np.where(is_open, dn[t0 + j], True)
            # the recurrence
            Vd, Vn = V[d], V[d + 1]
            A_t = R - Vd
            gv = G * Vn
            s1 = R + gv
            delta = s1 - Vd
            ca = c * A_next
            A_o = delta + ca
            A = np.where(term, A_t, A_o).astype(f)
            S_A = np.where(term, S_R + mag(A_t), S_R + S_G + mag(gv) + mag(s1) + mag(delta) + S_c + S_next + mag(ca) + mag(A_o))
            rt = A + Vd
            adv[d], ret[d] = A, rt
            adv_b[d], ret_b[d] = U * S_A, U * (S_A + mag(rt))
            block_reward[d], block_done[d], block_steps[d] = R, term[:, 0], n[:, 0]
            A_next, S_next = A, S_A
    if f is np.float32:
        adv, ret, block_reward = _stored(adv), _stored(ret), _stored(block_reward)
    shape = (D, B) if flat else (D, B, NV)
    res = {"adv": adv.reshape(shape), "ret": ret.reshape(shape), "block_reward": block_reward.reshape(shape if per_column else (D, B)),
           "block_done": block_done, "block_steps": block_steps}
    if with_bound:
        res["adv_bound"], res["ret_bound"] = adv_b.reshape(shape), ret_b.reshape(shape)
    return res


def split(reward, done, values, hold=1, adv_next=None, **kw):
    """the header's SPLITTING: decisions D/2 .. D-1 first, then 0 .. D/2-1 with adv_next = the first call's adv row 0; the two results joined"""
    D = np.asarray(values).shape[0] - 1
    h = D // 2
    late = gae(reward[h * hold:], done[h * hold:], values[h:], hold=hold, adv_next=adv_next, **kw)
    if h == 0:
        return late
    early = gae(reward[:h * hold], done[:h * hold], values[:h + 1], hold=hold, adv_next=late["adv"][0], **kw)
    return {k: np.concatenate([early[k], late[k]], axis=0) for k in late}
