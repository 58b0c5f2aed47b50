"""atc_gae_boot (include/atc_step.h) restated in numpy, in the style of tests/gae_ref.py (which restates atc_gae and stays as it is): the
block fold and the recurrence in np.float32 — or in float64, the TWIN — operation by operation in the header's order, vectorised over the
columns only.  What atc_gae_boot adds to atc_gae, with g the running product at the block's last counted step:

    term and trunc[d][e] != 0:  Gn = g * gamma;  delta = (R + (Gn * boot[d][i])) - V[d][i];  A = delta

THE RUNNING ERROR BOUND is gae_ref's, extended by the same rule (u times the sum of the magnitudes of every rounded intermediate in the
word's chain): a bootstrapped block's chain is R's, g's, Gn (not where it is 1.0f * gamma, which is exact), Gn * boot, R + Gn boot and
delta = A."""
import numpy as np

from gae_ref import U, _stored, constants


def gae_boot(reward, done, values, boot=None, trunc=None, hold=1, gamma=0.99, lam=0.95, per_decision=False, adv_next=None, dtype=np.float32,
             with_bound=False):
    """gae_ref.gae's arguments plus boot [D, B, NV] / [D, B] and trunc [D, B]; both None is atc_gae.  Returns gae_ref.gae's dict."""
    f = dtype
    assert (boot is None) == (trunc is None)
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
    if boot is None:
        bt, tr = np.zeros((D, B, NV), f), np.zeros((D, B, 1), bool)
    else:
        bt, tr = np.asarray(boot).reshape(D, B, NV).astype(f), (np.asarray(trunc).reshape(D, B) != 0)[:, :, None]
    gam = f(np.float32(gamma))
    G, c, S_G, S_c = constants(hold, gamma, lam, per_decision, f)
    A_next = np.zeros((B, NV), f) if adv_next is None else np.asarray(adv_next).reshape(B, NV).astype(f)
    S_next = np.zeros((B, NV))
    adv, ret = np.zeros((D, B, NV), f), np.zeros((D, B, NV), f)
    adv_b, ret_b = np.zeros((D, B, NV)), np.zeros((D, B, NV))
    block_reward = np.zeros((D, B, r.shape[2]), f)
    block_done, block_steps = np.zeros((D, B), np.uint8), np.zeros((D, B), np.uint8)
    mag = lambda x: np.abs(np.asarray(x).astype(np.float64))      # noqa: E731
    with np.errstate(all="ignore"):
        for d in range(D - 1, -1, -1):
            t0 = d * hold
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
            Vd, Vn = V[d], V[d + 1]
            A_t = R - Vd
            # the bootstrapped end: one more product of the running discount, from where the block stopped counting
            Gn = g * gam
            gb = Gn * bt[d]
            sb = R + gb
            A_b = sb - Vd
            S_b = S_R + S_g + np.where(g != 1, mag(Gn), 0.0) + mag(gb) + mag(sb) + mag(A_b)
            gv = G * Vn
            s1 = R + gv
            delta = s1 - Vd
            ca = c * A_next
            A_o = delta + ca
            booted = term & tr[d]
            A = np.where(booted, A_b, np.where(term, A_t, A_o)).astype(f)
            S_A = np.where(booted, S_b, np.where(term, S_R + mag(A_t), S_R + S_G + mag(gv) + mag(s1) + mag(delta) + S_c + S_next + mag(ca) + mag(A_o)))
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


def split(reward, done, values, boot, trunc, hold=1, adv_next=None, **kw):
    """the header's SPLITTING with boot and trunc split by decision: D/2 .. D-1 first, then 0 .. D/2-1 with adv_next = the first call's adv row 0"""
    D = np.asarray(values).shape[0] - 1
    h = D // 2
    late = gae_boot(reward[h * hold:], done[h * hold:], values[h:], boot[h:], trunc[h:], hold=hold, adv_next=adv_next, **kw)
    if h == 0:
        return late
    early = gae_boot(reward[:h * hold], done[:h * hold], values[:h + 1], boot[:h], trunc[:h], hold=hold, adv_next=late["adv"][0], **kw)
    return {k: np.concatenate([early[k], late[k]], axis=0) for k in late}
