"""Special fp32 action values per component, a placement helper that writes them into ordinary action blocks, and a plain restatement of
the action stage of include/atc_step.h.  TEST INFRASTRUCTURE ONLY; importing it needs no GPU and no oracle.

THE TABLE.  table(discrete) -> {component: [Edge(name, value, follow, wide)]}, component 0 / 1 / 2 = speed / altitude / heading.  `value` is
the fp32 action under test, `follow` the action the same aircraft is given after `value` was held (an ordinary one, or — the discriminator
pairs — the action whose target lies an exact distance from `value`'s), `wide` whether the HEADING target of `value` or `follow` lies
beyond the 32-bit heading field (the aircraft becomes WIDE; look-ahead calls do not evaluate such an env).  What is in it:
  non-finite / extreme   NaN (quiet, both signs, one with a payload), +-Inf, +-FLT_MAX, +-0.0, the smallest subnormal of either sign
  refusal boundaries     the action that decodes to exactly 100 kt, 300 kt, 0 ft, 38 000 ft and its fp32 neighbours on either side
  speed saturation       decoded speed targets just below 0 and at / above 2^32 counts (512 kt)
  heading bounds         decoded counts at +-2^31 (the 32-bit field) and +-2^52 (the clamp, ATC_F_PHI_LIMIT) with neighbours
  discriminator pairs    successive targets D-1, D, -(D-1), -D counts apart (speed, heading: the four ends of the unsigned compare
                         `within`), an altitude difference either side of 50 ft
Every number is derived here from the decode constants of the header (m, c per component and action space); nothing comes from the code
under test.

THE SPEC.  spec_step(state, action, discrete, dt) restates the action stage from the header's text with Python ints, Fractions and float64.
"""
import collections
import math
import struct
from fractions import Fraction

import numpy as np

import helpers as H

Q = 1 << 23                      # ATC_V_FIX_SHIFT / ATC_PHI_FIX_SHIFT
PHI_LIMIT = 1 << 52              # ATC_PHI_LIMIT
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
V_MIN_FIX, V_MAX_FIX = 100 * Q, 300 * Q
H_MIN, H_MAX = 0.0, 38000.0
DISCR_V, DISCR_H, DISCR_P = 5 * Q, 50.0, Q // 2      # atc_gym.py:84 in counts / feet
F_INVALID_V, F_INVALID_H, F_PHI_LIMIT = 1 << 4, 1 << 5, 1 << 9
FLT_MAX = float(np.finfo(np.float32).max)
SUBNORMAL = float(np.float32(1e-45))

Edge = collections.namedtuple("Edge", "name value follow wide")


def f32(x):
    return float(np.float32(x))


def from_bits(u):
    return struct.unpack("<f", struct.pack("<I", u))[0]


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def up(x, n=1):
    x = np.float32(x)
    for _ in range(n):
        x = np.nextafter(x, np.float32(np.inf))
    return float(x)


def down(x, n=1):
    x = np.float32(x)
    for _ in range(n):
        x = np.nextafter(x, np.float32(-np.inf))
    return float(x)


# ---------------------------------------------------------------------------------------------------------------- decode
def decode_consts(discrete):
    """(m, c) per component: target = a m + c.  Speed and heading in counts (integers), the altitude in feet.
    atc_gym.py:64-78,318-335: offset (v_min, 0, 0); factor (10, 100, 1) discrete, (200, 38000, 360) halved and centred continuous; the
    heading counts are relative to 180 deg (ATC_PHI_FIX_OFFSET)."""
    if discrete:
        return ((10 * Q, 100 * Q), (100, 0), (Q, -180 * Q))
    return ((100 * Q, 200 * Q), (19000, 19000), (180 * Q, 0))


def fma64(a, m, c):
    """ONE float64 fma of the fp32 action a with the integers m, c: the exact rational rounded once; NaN / Inf as IEEE gives them"""
    if math.isnan(a) or math.isinf(a):
        return a * float(m) + float(c)        # m > 0, c finite: NaN stays NaN, +-Inf stays +-Inf
    return float(Fraction(a) * m + c)         # (Fraction -> float is correctly rounded)


def speed_counts(a, discrete):
    """trunc toward zero, converted to uint32 SATURATING, NaN -> 0"""
    m, c = decode_consts(discrete)[0]
    x = fma64(a, m, c)
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return 0 if x < 0 else (1 << 32) - 1
    return min(max(math.trunc(x), 0), (1 << 32) - 1)


def altitude_target(a, discrete):
    m, c = decode_consts(discrete)[1]
    return fma64(a, m, c)


def heading_counts(a, discrete):
    """(trunc toward zero clamped to +-2^52, whether it was clamped); NaN -> 0, not clamped"""
    m, c = decode_consts(discrete)[2]
    x = fma64(a, m, c)
    if math.isnan(x):
        return 0, False
    if math.isinf(x):
        return (PHI_LIMIT if x > 0 else -PHI_LIMIT), True
    t = math.trunc(x)
    return min(max(t, -PHI_LIMIT), PHI_LIMIT), abs(t) > PHI_LIMIT


def is_wide_target(a, discrete):
    return not I32_MIN < heading_counts(a, discrete)[0] < I32_MAX


# ---------------------------------------------------------------------------------------------------------------- the spec
def wrap32(d):
    return (d + (1 << 31)) % (1 << 32) - (1 << 31)


def spec_step(st, action, discrete, dt=1.0):
    """One aircraft, one step of the action stage.  st: dict v (counts), h (float64), P (exact heading counts), la_v, la_h, la_P (the last
    accepted targets), acts (the env's counter) — updated in place.  Returns (flags, penalty): the ATC_F_INVALID_V / _H / PHI_LIMIT bits and
    the reward lost to refusals."""
    rate_v, rate_p = int(round(5.0 * dt * Q)), int(round(3.0 * dt * Q))
    flags, penalty = 0, 0.0
    # speed: refused outside [100, 300] kt (NaN decodes to 0 counts: refused); wrapping 32-bit differences
    tv = speed_counts(action[0], discrete)
    if tv < V_MIN_FIX or tv > V_MAX_FIX:
        flags |= F_INVALID_V
        penalty += 1.0
    else:
        st["v"] = (st["v"] + min(max(wrap32(tv - st["v"]), -rate_v), rate_v)) % (1 << 32)
        if not -DISCR_V < wrap32(tv - st["la_v"]) < DISCR_V:
            st["acts"] += 1
        st["la_v"] = tv
    # altitude: accepted iff h_min <= target <= h_max (a NaN target is refused); the reference's float64 operations
    th = altitude_target(action[1], discrete)
    if not (th >= H_MIN and th <= H_MAX):
        flags |= F_INVALID_H
        penalty += 1.0
    else:
        st["h"] = st["h"] + max(min(th - st["h"], 15.0 * dt), -41.0 * dt)
        if not abs(th - st["la_h"]) < DISCR_H:
            st["acts"] += 1
        st["la_h"] = th
    # heading: never refused; exact counts, the target clamped to +-2^52
    tp, lim = heading_counts(action[2], discrete)
    if lim:
        flags |= F_PHI_LIMIT
    st["P"] = st["P"] + min(max(tp - st["P"], -rate_p), rate_p)
    if not abs(tp - st["la_P"]) < DISCR_P:
        st["acts"] += 1
    st["la_P"] = tp
    return flags, penalty


# ---------------------------------------------------------------------------------------------------------------- the table
ORDINARY = {False: (0.25, -0.125, 0.5), True: (7.0, 120.0, 200.0)}      # 225 kt / 16 625 ft / 270 deg; 170 kt / 12 000 ft / 20 deg


def _solve(fn, target, m, c):
    """an fp32 action with fn(action) == target, or None (fn: trunc(a m + c), monotone): a short walk in ulps from the exact solution,
    started on either side of it (truncation is toward zero: downward for positive targets, upward for negative ones)"""
    for s in (0.5, 0.0, -0.5):
        a = f32((target + s - c) / m)
        for _ in range(16):
            got = fn(a)
            if got == target:
                return a
            a = up(a) if got < target else down(a)
    return None


def _pair(fn, m, c, diff, ok=lambda t: True):
    """(a1, a2) with fn(a2) - fn(a1) == diff > 0 exactly and both targets acceptable: a1 next to the action 0 — where fp32 actions are
    dense enough to reach every count —, a2 within a few ulps of the action whose target lies `diff` above fn(0)"""
    for k in (0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6):
        a2 = f32((fn(0.0) + diff + 0.5 - c) / m)
        a2 = up(a2, k) if k >= 0 else down(a2, -k)
        a1 = _solve(fn, fn(a2) - diff, m, c)
        if a1 is not None and ok(fn(a1)) and ok(fn(a2)):
            return a1, a2
    raise AssertionError(("no fp32 pair", diff))


_tables = {}


def table(discrete):
    discrete = bool(discrete)
    if discrete in _tables:
        return _tables[discrete]
    ordinary = ORDINARY[discrete]
    consts = decode_consts(discrete)
    common = [("nan", from_bits(0x7FC00000)), ("-nan", from_bits(0xFFC00000)), ("nan payload", from_bits(0x7FC12345)),
              ("+inf", math.inf), ("-inf", -math.inf), ("+flt_max", FLT_MAX), ("-flt_max", -FLT_MAX), ("+0", 0.0), ("-0", -0.0),
              ("+subnormal", SUBNORMAL), ("-subnormal", -SUBNORMAL)]
    out = {}
    for comp in range(3):
        m, c = consts[comp]
        inv = lambda t: f32((t - c) / m)   # noqa: E731
        rows = list(common)

        def around(name, a, n=1):
            rows.append((name, a))
            for j in range(1, n + 1):
                rows.append((name + " +%d ulp" % j, up(a, j)))
                rows.append((name + " -%d ulp" % j, down(a, j)))

        if comp == 0:
            around("100 kt", inv(100 * Q))
            around("300 kt", inv(300 * Q))
            around("0 counts", inv(0))                  # just below: saturates at 0
            top = inv(1 << 32)                          # the smallest action that decodes to 2^32 counts or more: at / above it the
            while fma64(top, m, c) < (1 << 32):         # conversion saturates at UINT32_MAX, a neighbour below it does not
                top = up(top)
            around("2^32 counts", top)
        elif comp == 1:
            around("0 ft", inv(0.0))
            around("38000 ft", inv(38000.0))
        else:
            around("+2^31 counts", inv(1 << 31), 2)
            around("-2^31 counts", inv(-(1 << 31)), 2)
            around("+2^52 counts", inv(PHI_LIMIT), 2)
            around("-2^52 counts", inv(-PHI_LIMIT), 2)
        edges = [Edge(n, v, ordinary[comp], comp == 2 and is_wide_target(v, discrete)) for n, v in rows]
        # discriminator pairs: value then follow
        if comp != 1:   # (a negative difference is the positive pair flown the other way round)
            fn = (lambda a: speed_counts(a, discrete)) if comp == 0 else (lambda a: heading_counts(a, discrete)[0])
            ok = (lambda t: V_MIN_FIX <= t <= V_MAX_FIX) if comp == 0 else (lambda t: True)
            D, what = (DISCR_V, "speed") if comp == 0 else (DISCR_P, "heading")
            for name, d in (("D-1", D - 1), ("D", D)):
                a1, a2 = _pair(fn, m, c, d, ok)
                edges.append(Edge("%s pair %s" % (what, name), a1, a2, False))
                edges.append(Edge("%s pair -%s" % (what, "(D-1)" if name == "D-1" else "D"), a2, a1, False))
        else:
            a1 = inv(10000.0)
            a2 = inv(10050.0)
            while not abs(altitude_target(a2, discrete) - altitude_target(a1, discrete)) < DISCR_H:
                a2 = down(a2)
            edges.append(Edge("altitude pair < 50 ft", a1, a2, False))
            while abs(altitude_target(a2, discrete) - altitude_target(a1, discrete)) < DISCR_H:
                a2 = up(a2)
            edges.append(Edge("altitude pair >= 50 ft", a1, a2, False))
            edges.append(Edge("altitude pair >= 50 ft down", a2, a1, False))
        out[comp] = edges
    _tables[discrete] = out
    return out


def n_values(discrete):
    return max(len(v) for v in table(discrete).values())


# ---------------------------------------------------------------------------------------------------------------- placement
def free_envs(B, N):
    """the envs of one whole wavefront (64 lanes = 64 / W envs) that placement leaves alone: the second wavefront of the batch"""
    per = max(1, 64 // H.lane_width(N))
    assert B >= 2 * per + 1, "the batch has no room for a free wavefront next to a first and a last env"
    return list(range(per, 2 * per))


def positions(N):
    return sorted({0, N // 2, N - 1})


Placement = collections.namedtuple("Placement", "value follow special wide_env full_env")


def place(seed, index, B, N, discrete, wide_envs=None):
    """Block `index` of the placement cycle of (seed, B, N, discrete).

    Returns Placement: value [B, N, 3] float32 — U(-1, 1) draws (integers inside the action space when discrete) with table values written
    in —, follow [B, N, 3] — the same block with every table value replaced by its `follow` —, special [B, N, 3] int32 (index into the
    component's table, -1 where ordinary), wide_env [B] bool (an aircraft of the env got a heading value that is WIDE), full_env.
    In every block:  the envs of free_envs(B, N) carry no table value;  env 0, env B-1 and full_env (the middle of the rest) carry one in
    EVERY aircraft and component;  every other env carries them in the aircraft of positions(N) = {0, N // 2, N - 1}.
    Table entry j of component c sits at rotation (j + index + the family's own offset) of each of these slot families.  ONE block need
    not hold every entry (at N = 16 .. 33 the batch has fewer scattered slots per position than the heading table has entries; env 0
    holds N of them), and a script of a few blocks shows every entry to SOME call, not to every one.  Over n_values(discrete) consecutive
    indices every (value, component) pair occurs in aircraft 0, in aircraft N // 2, in aircraft N - 1, in env 0, in env B - 1 and in
    full_env (coverage() counts exactly that).
    wide_envs (None: no such rule): the envs whose placed heading values all have `wide` set, while no other env gets one — the rotation
    skips to the next value of the wanted kind.  For look-ahead candidates, where a WIDE target means "not evaluated"."""
    tab = table(discrete)
    rng = np.random.default_rng([int(seed), int(index), B, N, int(bool(discrete))])
    if discrete:
        value = np.floor(rng.uniform(0, 1, (B, N, 3)) * np.array([20, 380, 360])).astype(np.float32)
    else:
        value = rng.uniform(-1.0, 1.0, (B, N, 3)).astype(np.float32)
    follow = value.copy()
    special = np.full((B, N, 3), -1, np.int32)
    free = set(free_envs(B, N))
    rest = [e for e in range(1, B - 1) if e not in free]
    full_env = rest[len(rest) // 2]
    wide_ok = np.ones(B, bool) if wide_envs is None else np.isin(np.arange(B), list(wide_envs))
    counters = {}
    # every slot family starts its rotation somewhere else, so that one block shows more of a table than its largest family holds
    offsets = {"first": 0, "last": 13, "full": 26}
    offsets.update({"slot %d" % k: 7 + 11 * r for r, k in enumerate(positions(N))})

    def put(e, k, family):
        for c in range(3):
            n = len(tab[c])
            j = (counters.get((family, c), 0) + index + offsets[family]) % n
            counters[(family, c)] = counters.get((family, c), 0) + 1
            if c == 2 and wide_envs is not None:
                while tab[c][j].wide != bool(wide_ok[e]):
                    j = (j + 1) % n
            special[e, k, c] = j
            value[e, k, c] = tab[c][j].value
            follow[e, k, c] = tab[c][j].follow

    for fam, e in (("first", 0), ("last", B - 1), ("full", full_env)):
        for k in range(N):
            put(e, k, fam)
    for e in rest:
        if e != full_env:
            for k in positions(N):
                put(e, k, "slot %d" % k)
    idx = special[..., 2]
    wide = (idx >= 0) & np.array([e.wide for e in tab[2]])[np.maximum(idx, 0)]
    return Placement(value, follow, special, wide.any(axis=1), full_env)


def coverage(seed, B, N, discrete, n_blocks, wide_envs=None):
    """occurrence counts over blocks 0 .. n_blocks-1: {family: [per component: counts per table entry]} for the families aircraft 0 /
    middle / last, env first / last / full, and the number of table values found in the free envs (must be 0)"""
    tab = table(discrete)
    fam = {k: [np.zeros(len(tab[c]), int) for c in range(3)] for k in ("ac 0", "ac mid", "ac last", "env first", "env last", "env full")}
    in_free = 0
    for b in range(n_blocks):
        p = place(seed, b, B, N, discrete, wide_envs)
        in_free += int((p.special[free_envs(B, N)] >= 0).sum())
        for name, sl in (("ac 0", p.special[:, 0]), ("ac mid", p.special[:, N // 2]), ("ac last", p.special[:, N - 1]),
                         ("env first", p.special[0]), ("env last", p.special[B - 1]), ("env full", p.special[p.full_env])):
            for c in range(3):
                idx = sl[..., c].ravel()
                np.add.at(fam[name][c], idx[idx >= 0], 1)
    return fam, in_free
