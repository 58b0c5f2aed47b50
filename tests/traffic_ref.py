"""numpy reference of the traffic observation (include/atc_step.h: atc_observe_traffic) and the state families its tests run on.

The reference works from the state's own formats — position counts, float64 altitudes, exact heading counts, speed counts, the
active masks, the position grid's origin / exponent:
  - fp32 positions as every formula sees them: (float)(origin + fix 2^-k), one rounding;
  - the ordering key d2 = fma(dx, dx, dy * dy) evaluated EXACTLY as the contract defines it: the fp32 product dy * dy, then the fma
    with ONE rounding — integer arithmetic per pair (a float64 shortcut can round twice);
  - the features in float64 from the same fp32 dx, dy, h and the exact heading and speed.
Nothing here touches the GPU or the library.
"""
import math

import numpy as np

from atc_hip import layout as L

TURN = 360 << 23          # a full turn in heading counts
KMAX = L.TRAFFIC_MAX_K


def _round_f32(n, s):
    """n / 2^s (n >= 0 an integer) rounded to the nearest float32, ties to even — returned as a Python float (exact)"""
    if n == 0:
        return 0.0
    e = max(n.bit_length() - 1 - s, -126)   # floor(log2) of the value, or the subnormal exponent
    sh = s + e - 23                          # the result is r * 2^(e - 23), r the value in units of its last place
    if sh <= 0:
        r = n << -sh
    else:
        r, rem, half = n >> sh, n & ((1 << sh) - 1), 1 << (sh - 1)
        if rem > half or (rem == half and (r & 1)):
            r += 1
    return math.ldexp(float(r), e - 23)


def fma_sq_f32(dx, p):
    """fma(dx, dx, p) in float32 with ONE rounding, dx and p float32 values (p >= 0)"""
    n1, d1 = float(dx).as_integer_ratio()
    n2, d2 = float(p).as_integer_ratio()
    s1, s2 = d1.bit_length() - 1, d2.bit_length() - 1
    s = max(2 * s1, s2)
    return _round_f32(((n1 * n1) << (s - 2 * s1)) + (n2 << (s - s2)), s)


def positions_f32(fix, origin, k):
    return (np.asarray(fix, np.int64).astype(np.float64) * 2.0 ** -k + float(origin)).astype(np.float32)


def heading_sincos(P):
    """sin, cos (float64) of the compass heading 180 + P 2^-23 deg, P exact heading counts (integer-valued, any magnitude)"""
    P = np.asarray(P)
    s, c = np.empty(P.shape), np.empty(P.shape)
    for idx in np.ndindex(P.shape):
        w = (int(P[idx]) + (180 << 23)) % TURN            # exact reduction of the heading to [0, 360) deg in counts
        th = math.radians(w * 2.0 ** -23)
        s[idx], c[idx] = math.sin(th), math.cos(th)
    return s, c


def active_bits(mask, N):
    """[B] uint64 masks -> [B, N] bool"""
    m = np.asarray(mask, np.uint64)
    return ((m[:, None] >> np.arange(N, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def traffic_reference(state, pos_origin, pos_k):
    """state: dict of x_fix, y_fix [B, N] int32, h [B, N] float64, P [B, N] exact heading counts (float64, integer-valued),
    v_fix [B, N] uint32, mask [B] uint64.  Returns a dict, everything for KMAX ranks (the first K ranks ARE the K-record answer):
      rec      [B, N, KMAX, 8] float64   the records, NOT normalised (absent: words 0..6 = 0, word 7 = -1)
      present  [B, N, KMAX] bool
      d, vsum  [B, N, KMAX]              the operands' magnitudes the bars scale with: distance, v_i + v_j
      d2       [B, N, KMAX + 1] float64  the sorted keys' d2, rank KMAX included (inf where there is no candidate)
      ncand    [B, N]                    candidates of each aircraft (0 for an aircraft not under control)"""
    xf, yf = np.asarray(state["x_fix"]), np.asarray(state["y_fix"])
    B, N = xf.shape
    x, y = positions_f32(xf, pos_origin[0], pos_k), positions_f32(yf, pos_origin[1], pos_k)
    h32 = np.asarray(state["h"], np.float64).astype(np.float32)
    v = np.asarray(state["v_fix"]).astype(np.uint32).astype(np.float64) * 2.0 ** -L.V_FIX_SHIFT
    sn, cs = heading_sincos(state["P"])
    vx, vy = v * sn, v * cs
    act = active_bits(state["mask"], N)
    rec = np.zeros((B, N, KMAX, L.TRAFFIC_DIM))
    rec[..., L.T_SLOT] = -1.0
    present = np.zeros((B, N, KMAX), bool)
    d_out, vsum = np.zeros((B, N, KMAX)), np.zeros((B, N, KMAX))
    d2_out = np.full((B, N, KMAX + 1), np.inf)
    ncand = np.zeros((B, N), np.int64)
    for e in range(B):
        on = np.nonzero(act[e])[0]
        if len(on) < 2:
            continue
        dx = x[e][None, :] - x[e][:, None]                 # [i, j] = xj - xi, fp32 (one rounding)
        dy = y[e][None, :] - y[e][:, None]
        pp = dy * dy                                       # the fp32 product
        d2 = {}
        for a, i in enumerate(on):                         # symmetric: (-dx)^2 = dx^2 exactly
            for j in on[a + 1:]:
                d2[(i, j)] = d2[(j, i)] = fma_sq_f32(dx[i, j], pp[i, j])
        for i in on:
            order = sorted((d2[(i, j)], int(j)) for j in on if j != i)
            ncand[e, i] = len(order)
            for r, (q, j) in enumerate(order[:KMAX + 1]):
                d2_out[e, i, r] = q
            for r, (q, j) in enumerate(order[:KMAX]):
                fx, fy = float(dx[i, j]), float(dy[i, j])
                dvx, dvy = vx[e, j] - vx[e, i], vy[e, j] - vy[e, i]
                s, c = sn[e, i], cs[e, i]
                rec[e, i, r] = (1.0, math.sqrt(q), fx * s + fy * c, fx * c - fy * s, float(h32[e, j] - h32[e, i]),
                                dvx * s + dvy * c, dvx * c - dvy * s, float(j))
                present[e, i, r] = True
                d_out[e, i, r] = math.sqrt(q)
                vsum[e, i, r] = v[e, i] + v[e, j]
    return dict(rec=rec, present=present, d=d_out, vsum=vsum, d2=d2_out, ncand=ncand)


def norm_scales(compiled):
    """(world diagonal, h_max, 2 v_max) of a compiled sector: what ATC_M_NORMALIZE divides words 1..3, 4, 5..6 by"""
    b = compiled.blob32
    return float(b[L.C_WORLD_DIAG]), float(b[L.C_H_MAX]), 2.0 * float(b[L.C_V_MAX])


def compare(got, ref, K, scales=None):
    """got [B, N, K, 8] float32 against the reference's first K ranks; the bars of the issue.  scales = norm_scales() for a
    normalised launch.  Returns a list of (what, worst excess) for every bar that is missed — empty when all hold."""
    got = np.asarray(got)
    rec, pres = ref["rec"][:, :, :K], ref["present"][:, :, :K]
    d, vs = np.maximum(1.0, ref["d"][:, :, :K]), np.maximum(1.0, ref["vsum"][:, :, :K])
    sp, sh, sv = scales if scales is not None else (1.0, 1.0, 1.0)
    bad = []

    def exact(name, a, b):
        if not np.array_equal(a, b):
            bad.append((name, int(np.sum(a != b))))

    def within(name, a, b, bar):
        ex = np.abs(a.astype(np.float64) - b) - bar
        if np.any(ex > 0) or np.any(np.isnan(a)):
            bad.append((name, float(np.nanmax(ex))))

    exact("word 0", got[..., L.T_PRESENT], rec[..., L.T_PRESENT].astype(np.float32))
    exact("word 7", got[..., L.T_SLOT], rec[..., L.T_SLOT].astype(np.float32))
    exact("absent pattern", got[~pres][:, :7], np.zeros((int((~pres).sum()), 7), np.float32))
    # word 4: (float)hj - (float)hi is exact; normalised it is the fp32 quotient by h_max — one more rounding, the same on both sides
    dh32 = rec[..., L.T_DH].astype(np.float32)
    exact("word 4", got[..., L.T_DH], dh32 if scales is None else dh32 / np.float32(sh))
    for w in (L.T_DIST, L.T_AHEAD, L.T_RIGHT):
        within("word %d" % w, got[..., w], rec[..., w] / sp, 1e-5 * d / sp * pres)
    for w in (L.T_DV_AHEAD, L.T_DV_RIGHT):
        within("word %d" % w, got[..., w], rec[..., w] / sv, 1e-5 * vs / sv * pres)
    return bad


# ---------------------------------------------------------------------------------------------------------------- state families
def _masks(rng, B, N):
    """random masks with 0 .. N bits set (env 0: all, env 1: none, env 2: one, where the batch has them)"""
    n = rng.integers(0, N + 1, B)
    n[:3] = (N, 0, 1)[:min(B, 3)]
    bits = np.argsort(rng.random((B, N)), axis=1) < n[:, None]          # bit k set iff its random rank is below the env's count
    return (bits.astype(np.uint64) << np.arange(N, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def _wide(rng, P, share):
    """marks a share of the headings WIDE: adds whole turns until the counts leave the 32-bit range (both directions)"""
    P = P.astype(np.float64)
    pick = rng.random(P.shape) < share
    turns = rng.integers(3, 2000, P.shape) * np.where(rng.random(P.shape) < 0.5, -1, 1)
    return np.where(pick, P + turns.astype(np.float64) * float(TURN), P)


def random_family(rng, B, N, pos_k):
    """aircraft spread over +-40 nm around the grid's origin, any altitude, heading (-70 .. 430 deg, some WIDE) and speed"""
    span = 40.0 * 2.0 ** pos_k
    P = rng.integers(int(-250 * 2 ** 23), int(250 * 2 ** 23), (B, N)).astype(np.float64)
    return dict(x_fix=rng.integers(-int(span), int(span), (B, N)).astype(np.int32), y_fix=rng.integers(-int(span), int(span), (B, N)).astype(np.int32),
                h=rng.uniform(0.0, 38000.0, (B, N)), P=_wide(rng, P, 0.08),
                v_fix=rng.integers(100 << 23, 300 << 23, (B, N)).astype(np.uint32), mask=_masks(rng, B, N))


def clustered_family(rng, B, N, pos_k):
    """positions on an 8 x 8 integer-nm lattice, altitudes on 500 ft steps, headings multiples of 45 deg (some WIDE), three speeds:
    exact ties and coincident aircraft are common"""
    P = ((rng.integers(0, 8, (B, N)) * 45 - 180) << 23).astype(np.float64)
    return dict(x_fix=(rng.integers(0, 8, (B, N)) << pos_k).astype(np.int32), y_fix=(rng.integers(0, 8, (B, N)) << pos_k).astype(np.int32),
                h=rng.integers(4, 40, (B, N)).astype(np.float64) * 500.0, P=_wide(rng, P, 0.08),
                v_fix=(rng.choice([200, 250, 300], (B, N)) << 23).astype(np.uint32), mask=_masks(rng, B, N))


FAMILIES = {"random": random_family, "clustered": clustered_family}


def phi_fields(P):
    """exact counts -> (phi_fix int32 [saturated where WIDE], is-wide mask)"""
    wide = (P <= L.I32_MIN) | (P >= L.I32_MAX)
    return np.clip(P, L.I32_MIN, L.I32_MAX).astype(np.int64).astype(np.int32), wide


def state_from_env(env):
    """the reference's input from an AtcVecEnv's state tensors (copied back from the device)"""
    B, N = env.B, env.N
    ac = env.ac.cpu().numpy().reshape(B, N, 4)
    return dict(x_fix=ac[..., L.AC_X], y_fix=ac[..., L.AC_Y], h=env.alt.cpu().numpy().reshape(B, N),
                P=env.phi_counts.cpu().numpy().reshape(B, N), v_fix=ac[..., L.AC_V].view(np.uint32),
                mask=env.active_mask.cpu().numpy().astype(np.uint64))


def state_from_oracle(orc):
    """the reference's input from an oracle.OracleEnv of the fp32 instantiation"""
    B, N = orc.B, orc.N
    return dict(x_fix=orc.px.reshape(B, N), y_fix=orc.py.reshape(B, N), h=orc.h.reshape(B, N),
                P=orc.phi_counts.astype(np.float64).reshape(B, N), v_fix=orc.v_fix.view(np.uint32).reshape(B, N), mask=orc.active_mask)


def check_traffic(got, state, comp, K, normalize, what):
    """got [B, N, K, 8] (a launch's records, copied back) against the reference on `state` under compare()'s bars; comp: the compiled
    sector, normalize: whether the launch normalised.  Prints the verdict, asserts it and returns the reference."""
    ref = traffic_reference(state, comp.pos_origin, comp.pos_k)
    bad = compare(got, ref, K, norm_scales(comp) if normalize else None)
    print("%s: %s" % (what, bad or "ok"))
    assert not bad, (what, bad)
    return ref
