"""Sectors with random noise-abatement areas, and the probe points that go with them.  TEST INFRASTRUCTURE ONLY; importing it needs no GPU.

Noise-abatement areas are an extension with no reference implementation (oracle/atc_oracle_impl.h is their definition): an aircraft
inside an area's ring (the reference's crossing test, behind the area's inclusive bounds) and strictly below its ceiling pays the area's
penalty that step and is flagged F_NOISE.  The pieces of the product that implement it — the candidate masks in the lookup-grid cell
word, their decode, the per-area bits of the flag word, the penalty loop and the no-grid path — are held to the oracle on the sectors
drawn here (tests/test_noise_areas.py).

  random_sector / probe_points     the random MVA sectors of tests/test_random_sectors.py (moved here: test files are not imported from)
  noise_sector(seed, n_areas, base)   a scenario object (sector_io.from_dict) with n_areas in {1, 4, 16} areas on LOWW's or a random
                                      sector's MVAs; its document is kept as scn.doc
  noise_probe_points(comp, rng)    points over the grid's extent, along every edge, on every vertex, on the corners of every area's
                                   bounds and on the fp32 neighbours of each bound
  pip_reference                    plain float64 even-odd point-in-polygon + ceiling test (the independent reference)
  place / probe_batch              aircraft placed so that they sit on the probe points AFTER one step
  noise_case(seed)                 held_fuzz.case-shaped kw on a noise sector"""
import numpy as np

ENTRY_LEVELS = (30, 50, 70, 90)      # FL30 .. FL90, under the ceilings; 2000 ft apart, so that aircraft of one entry point that
#                                      climb and descend do not lose separation on their first step
CONT_CEILINGS = (4750.0, 5937.5, 7125.0, 8312.5, 9500.0)      # a 19000 + 19000 for a = -0.75, -0.6875, -0.625, -0.5625, -0.5 (exact in fp32)


# ------------------------------------------------------------------------------------------------ random MVA sectors
def random_sector(seed, n_poly):
    rng = np.random.default_rng(seed)
    mvas = []
    for p in range(n_poly):
        cx, cy = rng.uniform(10, 50, 2)
        n = int(rng.integers(3, 12))
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        rad = rng.uniform(3, 18, n)               # star-shaped (generally concave) ring
        pts = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
        if rng.random() < 0.4:                    # snap some vertices to a coarse lattice: shared / axis-aligned edges
            pts = _snap_to_lattice(pts)
            if len(pts) < 3:
                pts = np.array([[cx, cy], [cx + 6, cy], [cx + 6, cy + 6]])
        mvas.append((pts, float(rng.integers(20, 90)) * 100.0))
    # two exact rectangles sharing an edge (the classic tie-break case)
    mvas.append(([(20, 20), (30, 20), (30, 30), (20, 30)], 2500.0))
    mvas.append(([(30, 20), (40, 20), (40, 30), (30, 30)], 3500.0))
    return mvas, (30.0, 30.0, 500.0, float(rng.integers(0, 360))), [(12.0, 12.0, 45.0, [150])]


def _snap_to_lattice(pts):
    """the ring's vertices rounded to a 2 nm lattice, consecutive duplicates (the closing one included) dropped"""
    pts = np.round(pts / 2.0) * 2.0
    keep = [0]
    for k in range(1, len(pts)):
        if not np.array_equal(pts[k], pts[keep[-1]]):
            keep.append(k)
    pts = pts[keep]
    if len(pts) >= 2 and np.array_equal(pts[0], pts[-1]):
        pts = pts[:-1]
    return pts


def probe_points(comp, rng, n_random=2500):
    bb = comp.bbox
    pts = [np.stack([rng.uniform(bb[0] - 1, bb[2] + 1, n_random), rng.uniform(bb[1] - 1, bb[3] + 1, n_random)], 1)]
    for ring in comp.mva_rings:
        for k in range(len(ring) - 1):
            t = rng.uniform(0, 1, 6)[:, None]
            pts.append(ring[k][None, :] * (1 - t) + ring[k + 1][None, :] * t + rng.normal(0, 3e-4, (6, 2)))
            pts.append(ring[k][None, :] + rng.normal(0, 1e-5, (2, 2)))
            pts.append(ring[k][None, :])          # exact vertices
    return np.concatenate(pts)


# ------------------------------------------------------------------------------------------------ the independent reference
def pip_even_odd(x, y, ring):
    """Plain float64 even-odd rule for points x, y [n] and a closed ring [m, 2]: a ray to +x crosses the edge (a, b) when the edge
    straddles the point's y (half-open) and meets the ray right of the point.  Nothing of the product's or the oracle's code."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    inside = np.zeros(x.shape, bool)
    for (ax, ay), (bx, by) in zip(ring[:-1], ring[1:]):
        if ay == by:
            continue
        straddles = (ay > y) != (by > y)
        xc = ax + (y - ay) * (bx - ax) / (by - ay)
        inside ^= straddles & (x < xc)
    return inside


def edge_distance(x, y, ring):
    """distance [n] of the points to the nearest edge of the closed ring"""
    p = np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], 1)
    best = np.full(len(p), np.inf)
    for a, b in zip(ring[:-1], ring[1:]):
        ab = b - a
        L2 = float(ab @ ab)
        t = np.zeros(len(p)) if L2 == 0.0 else np.clip(((p - a) @ ab) / L2, 0.0, 1.0)
        best = np.minimum(best, np.hypot(*(p - (a + t[:, None] * ab)).T))
    return best


def areas_of(comp, scn):
    """[(closed ring float64 [m, 2], ceiling, penalty)] of a compiled noise sector"""
    return [(ring, float(a.ceiling), float(a.penalty)) for ring, a in zip(comp.noise_rings, scn.noise_areas)]


def pip_reference(x, y, h, areas):
    """(inside [n, Q] bool: in area q and below its ceiling, penalty [n]: the sum of those areas' penalties, clear [n] bool: farther than
    1e-3 nm from every noise edge and than 1 ft from every ceiling of an area whose ring the point is in or within 1e-3 nm of)"""
    x, y, h = (np.asarray(v, np.float64) for v in (x, y, h))
    inside = np.zeros((len(x), len(areas)), bool)
    clear = np.ones(len(x), bool)
    for q, (ring, ceiling, _) in enumerate(areas):
        pin = pip_even_odd(x, y, ring)
        near = edge_distance(x, y, ring) <= 1e-3
        inside[:, q] = pin & (h < ceiling)
        clear &= ~near & ~((pin | near) & (np.abs(h - ceiling) <= 1.0))
    pen = inside.astype(np.float64) @ np.array([p for _, _, p in areas], np.float64) if areas else np.zeros(len(x))
    return inside, pen, clear


# ------------------------------------------------------------------------------------------------ the noise sectors
def _star_ring(rng, cx, cy, r_lo, r_hi, snap):
    n = int(rng.integers(3, 12))
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(r_lo, r_hi, n)
    pts = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
    if snap:
        pts = _snap_to_lattice(pts)
        if len(pts) < 3:
            return None
    return pts


def _closed(pts):
    return np.concatenate([pts, pts[:1]])


def _ring_until(rng, cx, cy, r_lo, r_hi, snap, ok):
    """a star ring round (cx, cy) that satisfies ok(ring): redrawn until it does (a ring snapped to the lattice may lose its centre)"""
    for _ in range(200):
        pts = _star_ring(rng, cx, cy, r_lo, r_hi, snap)
        if pts is not None and abs(_signed_area(pts)) > 1e-6 * r_lo * r_lo and ok(pts):
            return pts
        snap = snap and rng.random() < 0.5
    raise AssertionError("no ring found")


def _signed_area(pts):
    x, y = pts[:, 0], pts[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def noise_sector(seed, n_areas, base):
    """Scenario object of a sector with n_areas noise-abatement areas.  base "LOWW": the shipped MVAs, runway and entry positions;
    "random": random_sector(seed, 9)'s MVAs and runway with drawn entry points.  Twelve entry points, 3.2 nm apart, each with the
    levels of FL30 / 50 / 70 / 90 that lie above its local floor (an aircraft spawned below its MVA would end the episode at once).  The areas:
    star-shaped rings of 3 - 11 vertices round centres on the entry points' tracks (so they overlap one another and traffic meets them),
    40 % snapped to a 2 nm lattice; area 0 contains entry point 0 and reaches beyond the MVAs' bounding box (and so beyond their union);
    with more than one area, area 1 reaches beyond the union of the MVA polygons, area 2 is smaller than a 0.5 nm cell and contains entry
    point 1, area 3 lies over area 0's centre.  Penalties: pairwise distinct multiples of 0.01.  Ceilings: altitude targets an fp32 action
    decodes to exactly — CONT_CEILINGS (continuous) or multiples of 100 ft (discrete; 9500 is both)."""
    from atc_hip import sector_io
    from envs.atc import scenarios
    assert n_areas in (1, 4, 16) and base in ("LOWW", "random")
    for attempt in range(40):     # (a random MVA set without twelve such entry points, or without room for area 0, is drawn again)
        try:
            doc = _noise_doc(np.random.default_rng([int(seed), n_areas, attempt, 0x4E4F4953]), 100 * int(seed) + attempt, n_areas, base)
            break
        except AssertionError:
            if attempt == 39:
                raise
    doc["name"] = "noise-%s-%d-%d" % (base, n_areas, seed)
    scn = sector_io.from_dict(doc)
    scn.doc = doc
    return scn


def _noise_doc(rng, mva_seed, n_areas, base):
    from envs.atc import scenarios
    if base == "LOWW":
        loww = scenarios.LOWW(random_entrypoints=True)
        mvas = [(np.asarray(m.area_as_list, np.float64), float(m.height)) for m in loww.mvas]
        rw = loww.runway
        runway = (rw.x, rw.y, rw.h, rw.phi_from_runway)
        cand = [(66.0, 39.0, 290.0)] + [(float(e.x), float(e.y), float(e.phi)) for e in loww.entrypoints if (e.x, e.y) != (66.0, 39.0)]
        cand += [(40.0, 45.0, 200.0), (30.0, 62.0, 150.0), (50.0, 25.0, 330.0), (45.0, 65.0, 200.0), (60.0, 50.0, 250.0), (20.0, 55.0, 90.0)]
    else:
        mvas, runway, _ = random_sector(mva_seed, 9)
        mvas = [(np.asarray(p, np.float64), h) for p, h in mvas]
        cand = [(float(rng.uniform(12, 48)), float(rng.uniform(12, 48)), float(rng.integers(0, 36)) * 10.0) for _ in range(400)]
    rings = [_closed(p) for p, _ in mvas]
    bx0, by0 = min(r[:, 0].min() for r in rings), min(r[:, 1].min() for r in rings)
    bx1, by1 = max(r[:, 0].max() for r in rings), max(r[:, 1].max() for r in rings)

    def floor_at(px, py):     # the first polygon's height (list order is the lookup's priority), None outside
        for r, (_, hgt) in zip(rings, mvas):
            if bool(pip_even_odd([px], [py], r)[0]):
                return hgt
        return None
    if base == "random":   # candidates on the right border of the MVAs' bounding box first, flying in: entry point 0
        cand = [(bx1 - d, float(rng.uniform(by0, by1)), 270.0) for d in (1.0, 2.0, 3.0) for _ in range(40)] + cand
    # entry points: inside the airspace, 3.2 nm apart (no conflict at the spawn), with the levels of FL30 .. FL90 above the local floor
    entries = []
    for x, y, phi in cand:
        f = floor_at(x, y)
        lv = [] if f is None else [v for v in ENTRY_LEVELS if 100.0 * v > f]
        if len(lv) >= 3 and all(np.hypot(x - a, y - b) >= 3.2 for a, b, _, _ in entries):
            entries.append((x, y, phi, lv))
        if len(entries) == 12:
            break
    assert len(entries) == 12, "no 12 entry points with three levels above their floor"
    # (36 distinct lattice slots: envs of up to 36 aircraft spawn free of conflicts; 64 aircraft share slots and end at once unless the
    # separation minimum is 0)
    assert len({(k % 12, (k // 12) % len(entries[k % 12][3])) for k in range(36)}) == 36

    def in_union(px, py):
        return any(bool(pip_even_odd([px], [py], r)[0]) for r in rings)

    def contains(pt):
        return lambda pts: bool(pip_even_odd([pt[0]], [pt[1]], _closed(pts))[0])

    areas = []
    e0, e1 = entries[0], entries[1]
    # area 0: contains entry point 0 and reaches beyond the bounding box of the MVAs
    areas.append(_ring_until(rng, e0[0], e0[1], 3.0, 18.0, rng.random() < 0.4,
                             lambda p: contains(e0)(p) and (p[:, 0].max() > bx1 + 0.6 or p[:, 0].min() < bx0 - 0.6 or
                                                            p[:, 1].max() > by1 + 0.6 or p[:, 1].min() < by0 - 0.6)))
    if n_areas > 1:
        # area 1: a vertex outside every MVA polygon (inside the bounding box or not)
        k = int(rng.integers(2, len(entries)))
        areas.append(_ring_until(rng, entries[k][0], entries[k][1], 3.0, 18.0, rng.random() < 0.4,
                                 lambda p: any(not in_union(a, b) for a, b in p)))
        # area 2: smaller than a 0.5 nm cell, round entry point 1
        areas.append(_ring_until(rng, e1[0], e1[1], 0.05, 0.2, False, contains(e1)))
        # area 3: over area 0 (two penalties at entry point 0)
        areas.append(_ring_until(rng, e0[0], e0[1], 3.0, 12.0, rng.random() < 0.4, contains(e0)))
    while len(areas) < n_areas:
        # the others: round a point up to 12 nm down the track of an entry point (compass heading: x += sin, y += cos)
        x, y, phi, _ = entries[int(rng.integers(len(entries)))]
        d = rng.uniform(0.0, 12.0)
        cx = x + d * np.sin(np.radians(phi)) + rng.normal(0, 1.5)
        cy = y + d * np.cos(np.radians(phi)) + rng.normal(0, 1.5)
        areas.append(_ring_until(rng, cx, cy, 3.0, 18.0, rng.random() < 0.4, lambda p: True))
    pen = rng.permutation(np.arange(1, 41))[:n_areas]
    pool = list(CONT_CEILINGS) + [float(c) for c in range(4000, 9600, 100)]
    ceilings = [float(CONT_CEILINGS[int(rng.integers(len(CONT_CEILINGS)))]) if rng.random() < 0.5 else
                float(pool[int(rng.integers(len(pool)))]) for _ in range(n_areas)]
    ceilings[0] = 9500.0       # area 0 (entry point 0) is above every entry level: its spawns are flagged, in both action spaces
    return {"format": "atc-sector/1", "name": "noise",
           "runway": {"x": runway[0], "y": runway[1], "h": runway[2], "phi_from_runway": runway[3]},
           "mvas": [{"height": h, "ring": [[float(a), float(b)] for a, b in p]} for p, h in mvas],
           "entrypoints": [{"x": x, "y": y, "phi": phi, "levels": lv} for x, y, phi, lv in entries],
           "noise_areas": [{"ceiling": c, "penalty": round(0.01 * int(p), 2), "ring": [[float(a), float(b)] for a, b in r]}
                           for r, c, p in zip(areas, ceilings, pen)]}


def without_noise(scn):
    """the same sector with no noise-abatement area"""
    from atc_hip import sector_io
    return sector_io.from_dict(dict(scn.doc, noise_areas=[]))


def noise_bounds(comp):
    return [(r[:, 0].min(), r[:, 1].min(), r[:, 0].max(), r[:, 1].max()) for r in comp.noise_rings]


def noise_probe_points(comp, rng, n_random=600):
    """[n, 2] float64: random points over the lookup grid's extent (the MVAs' bounding box and every area's bounds, a nautical mile
    beyond), six points per noise edge at N(0, 3e-4) nm from it, every vertex exactly and at N(0, 1e-5), the four corners of every
    area's bounds, and the fp32 neighbours either side of each bound (at the corners and at the middle of the other axis)."""
    bb, nb = comp.bbox, noise_bounds(comp)
    x0, y0 = min([bb[0]] + [b[0] for b in nb]), min([bb[1]] + [b[1] for b in nb])
    x1, y1 = max([bb[2]] + [b[2] for b in nb]), max([bb[3]] + [b[3] for b in nb])
    pts = [np.stack([rng.uniform(x0 - 1, x1 + 1, n_random), rng.uniform(y0 - 1, y1 + 1, n_random)], 1)]
    for ring, b in zip(comp.noise_rings, nb):
        for k in range(len(ring) - 1):
            t = rng.uniform(0, 1, 6)[:, None]
            pts.append(ring[k][None, :] * (1 - t) + ring[k + 1][None, :] * t + rng.normal(0, 3e-4, (6, 2)))
            pts.append(ring[k][None, :] + rng.normal(0, 1e-5, (2, 2)))
            pts.append(ring[k][None, :])
        pts.append(np.array([[b[0], b[1]], [b[0], b[3]], [b[2], b[1]], [b[2], b[3]]]))
        mid = ring[:-1].mean(0)                     # and a few points well inside a small ring, which the random points never meet
        pts.append(np.concatenate([mid[None, :], mid[None, :] + 0.5 * (ring[:-1] - mid[None, :]), mid[None, :] + 0.25 * (ring[:-1] - mid[None, :])]))
        mx, my = 0.5 * (b[0] + b[2]), 0.5 * (b[1] + b[3])
        for v in (b[0], b[2]):
            v32 = np.float32(v)
            for xv in (np.nextafter(v32, np.float32(-np.inf)), v32, np.nextafter(v32, np.float32(np.inf))):
                pts.append(np.array([[float(xv), b[1]], [float(xv), my], [float(xv), b[3]]]))
        for v in (b[1], b[3]):
            v32 = np.float32(v)
            for yv in (np.nextafter(v32, np.float32(-np.inf)), v32, np.nextafter(v32, np.float32(np.inf))):
                pts.append(np.array([[b[0], float(yv)], [mx, float(yv)], [b[2], float(yv)]]))
    return np.concatenate(pts)


# ------------------------------------------------------------------------------------------------ placement
PROBE_V, PROBE_PHI = 100.0, 0.0     # slow and due north: the step moves a placed aircraft by v dt / 3600 nm in +y


def start_of(points, dt):
    """where to place an aircraft (heading PROBE_PHI, speed PROBE_V, both held) so that ONE step of dt seconds takes it to the point"""
    p = np.array(points, np.float64)
    p[:, 1] -= PROBE_V / 3600.0 * dt
    return p


def hold_actions(h_target, discrete):
    """[n, 3] float32 actions: speed PROBE_V, heading PROBE_PHI, altitude target h_target [n] (NaN: a target beyond the ceiling of the
    action space, which is refused — the aircraft keeps its altitude to the last bit)"""
    h = np.asarray(h_target, np.float64)
    a = np.zeros((len(h), 3), np.float64)
    if discrete:
        a[:, 0], a[:, 2] = (PROBE_V - 100.0) / 10.0, PROBE_PHI
        a[:, 1] = np.where(np.isnan(h), 390.0, h / 100.0)
    else:
        a[:, 0], a[:, 2] = (PROBE_V - 200.0) / 100.0, PROBE_PHI / 180.0 - 1.0
        a[:, 1] = np.where(np.isnan(h), 1.5, h / 19000.0 - 1.0)
    return a.astype(np.float32)


def probe_batch(comp, scn, rng, B, N, dt, discrete, n_random=None, on_ceiling=2.0 / 3.0):
    """Probe aircraft for a batch of B x N: start positions [B N, 2], altitudes [B N] and hold actions [B, N, 3] such that after ONE step
    the aircraft sit on noise_probe_points (cycled or cut to B N).  Altitudes: the share 1 - on_ceiling of the aircraft somewhere in 2000 .. 11000 ft
    with their own altitude as target (rounded to what the action space decodes exactly), the others on a ceiling of an area — the
    nearest area's — at ceiling - 1 ulp, ceiling, ceiling + 1 ulp; half of those with the ceiling as target (the step takes all three
    onto the ceiling) and half with a refused target (they keep their altitude to the ulp)."""
    n = B * N
    pts = noise_probe_points(comp, rng, n_random=n_random if n_random is not None else max(16, n // 2))
    pts = pts[rng.permutation(len(pts))]
    pts = pts[np.arange(n) % len(pts)]
    areas = areas_of(comp, scn)
    ceil = np.array([c for _, c, _ in areas])
    d = np.stack([edge_distance(pts[:, 0], pts[:, 1], r) for r, _, _ in areas], 1)
    inside = np.stack([pip_even_odd(pts[:, 0], pts[:, 1], r) for r, _, _ in areas], 1)
    nearest = np.where(inside.any(1), np.where(inside, d, -np.inf).argmax(1), d.argmin(1))
    c = ceil[nearest]
    usable = np.array([(cc % 100.0 == 0.0) if discrete else (cc in CONT_CEILINGS) for cc in c])   # a ceiling this action space decodes
    kind = np.where(rng.random(n) < on_ceiling, rng.integers(3, 9, n), 0)
    kind = np.where(usable | (kind % 2 == 1), kind, 0)       # (a refused target needs no decodable ceiling)
    free = kind < 3
    if discrete:
        h_free = rng.integers(20, 111, n) * 100.0
    else:
        h_free = rng.integers(-57, -26, n) / 64.0 * 19000.0 + 19000.0     # a = k / 64: 2078 .. 11281 ft, exact
    under = np.floor((c - 500.0) / 100.0) * 100.0 if discrete else (np.floor((c - 500.0) / 19000.0 * 64.0) / 64.0) * 19000.0
    h_free = np.where(rng.random(n) < 0.5, under, h_free)      # half of them some 500 ft under the nearest area's ceiling
    off = (kind % 3) - 1                                       # -1, 0, +1 ulp
    h_ceil = np.where(off < 0, np.nextafter(c, -np.inf), np.where(off > 0, np.nextafter(c, np.inf), c))
    h = np.where(free, h_free, h_ceil)
    refused = ~free & (kind % 2 == 1)
    target = np.where(free, h_free, np.where(refused, np.nan, c))
    return start_of(pts, dt), h, hold_actions(target, discrete).reshape(B, N, 3), pts


def place(orc, env, start, h):
    """puts aircraft i at start[i], altitude h[i], heading PROBE_PHI, speed PROBE_V — on the oracle(s) and, if given, the env (in one
    copy per state array)"""
    from atc_hip import layout as L
    from atc_hip.scenario import to_fix
    for o in (orc if isinstance(orc, (list, tuple)) else [orc]):
        for i in range(len(h)):
            o.set_state(i // o.N, i % o.N, start[i, 0], start[i, 1], h[i], PROBE_PHI, PROBE_V)
    if env is not None:
        import torch
        ac = env.ac.cpu()
        ac[:, L.AC_X] = torch.as_tensor(to_fix(start[:, 0], env.pos_origin[0], env.pos_k))
        ac[:, L.AC_Y] = torch.as_tensor(to_fix(start[:, 1], env.pos_origin[1], env.pos_k))
        ac[:, L.AC_PHI] = env._phi_counts(PROBE_PHI)[0]
        ac[:, L.AC_V] = env._v_counts(PROBE_V)
        env.ac.copy_(ac)
        env.alt.copy_(torch.as_tensor(np.asarray(h, np.float64)))


# ------------------------------------------------------------------------------------------------ held-kernel cases
def noise_case(seed):
    """(scn, comp, kw) shaped like held_fuzz.case(seed)'s, on a noise sector: the env configuration and the calls are held_fuzz.case's own
    draw; the sector (4 or 16 areas, LOWW or random MVAs), a lookup grid of None / 0.125 / 0.5 / 2.0 nm and the spawn mode are drawn here."""
    import held_fuzz as F
    from envs.atc import scenarios
    _, _, kw = F.case(seed)
    rng = np.random.default_rng([int(seed), 0x4E43])
    scn = noise_sector(int(rng.integers(1, 5)), int(rng.choice([4, 16])), str(rng.choice(["LOWW", "random"])))
    kw = dict(kw, grid_cell=[None, 0.125, 0.5, 2.0][int(rng.integers(4))], spawn=str(rng.choice(["lattice", "random"])))
    return scn, scenarios.compile_scenario(scn, grid_cell=kw["grid_cell"]), kw


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
# (sector seed, n_areas, base) + fuzz_space.run_vs_oracle's keywords.  tests/test_noise_areas.py flies them on the GPU; its CPU twin
# flies the same cases on the oracle alone (fly_oracle) and holds them to the coverage conditions.
FLIGHT_CASES = (
    dict(sector=(1, 16, "LOWW"), B=256, N=1, steps=200, seed=701, dt=1.0, grid_cell=0.5, full=True, spawn="random"),
    dict(sector=(7, 4, "random"), B=64, N=16, steps=120, seed=702, dt=5.0, grid_cell=0.125, full=False, use_rollout=4),
    dict(sector=(3, 16, "random"), B=32, N=33, steps=120, seed=703, dt=0.37, grid_cell=None, full=True, use_rollout=4, rollout_hold=4, hold=8),
    dict(sector=(4, 16, "LOWW"), B=16, N=64, steps=100, seed=704, dt=1.0, grid_cell=2.0, full=False, discrete=True, sep_nm=0.0),
    dict(sector=(1, 4, "LOWW"), B=64, N=16, steps=120, seed=705, dt=0.37, grid_cell=0.5, full=True, discrete=True, timestep_limit=40,
         spawn="random"),
    dict(sector=(2, 16, "random"), B=32, N=16, steps=200, seed=706, dt=5.0, grid_cell=0.5, full=True, auto_reset=False),
    dict(sector=(3, 4, "LOWW"), B=256, N=1, steps=200, seed=707, dt=0.37, grid_cell=0.125, full=True, discrete=True, use_rollout=4,
         spawn="random"),
    dict(sector=(4, 16, "random"), B=16, N=64, steps=96, seed=708, dt=5.0, grid_cell=0.5, full=False, discrete=True, use_rollout=4,
         rollout_hold=4, hold=4, sep_nm=0.0),
)
# Flights that START on a ceiling.  No flown step lands an aircraft one ulp below a ceiling: the altitude moves by h + (target - h)
# with both in float64, the difference is exact whenever h / 2 <= target <= 2 h (Sterbenz) — always, at these altitudes and rates —
# so a levelling aircraft lands ON its target, and a climbing one adds rounded rate * dt increments that meet ceiling - 1 ulp only by
# a 2^-40 coincidence.  (The altitude and this update are float64 in BOTH oracle instantiations and in the kernels — include/atc_step.h,
# ABI 20 — so the argument is the same for the fp32 oracle the GPU tests compare with.)  These flights are therefore constructed: aircraft placed at ceiling - 1 ulp / ceiling / ceiling + 1 ulp inside
# the areas with a refused altitude target (they keep their altitude to the bit) or the ceiling as target, flown on without resets.
CEILING_FLIGHTS = (
    dict(sector=(1, 16, "LOWW"), B=32, N=16, steps=6, seed=721, dt=1.0, grid_cell=0.5, discrete=False, shaping=True),
    dict(sector=(3, 16, "random"), B=8, N=64, steps=6, seed=722, dt=5.0, grid_cell=None, discrete=True, shaping=False),
)
PROBE_N, PROBE_CELLS = (1, 5, 16, 64), (None, 0.125, 0.5, 2.0)
# twelve held_fuzz / branch_fuzz seeds, chosen on the oracle alone (tests/test_noise_areas.py::test_coverage_of_the_held_cases) so that the
# family flags every area index of its 16-area sectors (9022 and 9042 do between them) next to the conditions it meets per kernel
HELD_SEEDS = (9001, 9002, 9003, 9005, 9006, 9010, 9012, 9022, 9024, 9033, 9040, 9042)


def probe_cases():
    """the 16 (N, grid_cell) pairs of the point probe, each with an action space, shaping on or off, a timestep and a sector — every
    N and every grid cell meets both action spaces and both shaping modes"""
    out = []
    for i, N in enumerate(PROBE_N):
        for j, cell in enumerate(PROBE_CELLS):
            out.append(dict(N=N, grid_cell=cell, discrete=bool((i + j) % 2), shaping=bool((i + j // 2) % 2), dt=(1.0, 0.37, 5.0)[(i + j) % 3],
                            sector=(1 + (i + 2 * j) % 4, (16, 4, 1)[(i + j) % 3], ("LOWW", "random")[j % 2]), seed=800 + 4 * i + j,
                            B=min(256, 4096 // N)))
    return out


def case_sector(c, grid=True):
    from envs.atc import scenarios
    scn = noise_sector(*c["sector"])
    return scn, scenarios.compile_scenario(scn, grid_cell=c["grid_cell"] if grid else None)


def probe_params(c):
    """the env configuration of a probe case in fuzz_space.make_env / make_oracle's keywords"""
    return dict(B=c["B"], N=c["N"], seed=c["seed"], dt=c["dt"], discrete=c["discrete"], spawn="lattice", grid_cell=c["grid_cell"],
                timestep_limit=6000, full=True, shaping=c["shaping"], normalize=True, sep_nm=3.0, keep_active=False, auto_reset=True)


def fly_oracle(comp, cov, B, N, steps, seed, dt=1.0, discrete=False, spawn="lattice", hold=20, grid_cell=0.5, use_rollout=0,
               timestep_limit=6000, full=True, shaping=True, normalize=True, sep_nm=3.0, keep_active=False, rollout_hold=1, wild=0.0,
               auto_reset=True):
    """fuzz_space.run_vs_oracle's oracle side alone: the same env configuration, the same action stream.  cov.add(orc, auto_reset) after
    every step."""
    from fuzz_space import draw_actions, make_oracle
    kw = dict(B=B, N=N, seed=seed, dt=dt, discrete=discrete, spawn=spawn, grid_cell=grid_cell, timestep_limit=timestep_limit, full=full,
              shaping=shaping, normalize=normalize, sep_nm=sep_nm, keep_active=keep_active, auto_reset=auto_reset)
    orc = make_oracle(comp, kw)
    rng = np.random.default_rng(seed)
    act = None
    for t in range(steps):       # (run_vs_oracle draws one action block whenever t % hold == 0, chunked or not)
        if t % hold == 0 or act is None:
            act = draw_actions(rng, (B, N), discrete, wild, True)
        orc.step(act)
        cov.add(orc, auto_reset)
    return orc


def ceiling_flight_params(c):
    """a CEILING_FLIGHTS case in fuzz_space.make_env / make_oracle's keywords: no resets (every aircraft's state stays the step's) and
    no separation minimum (the placed aircraft do not end their envs by conflicts)"""
    return dict(probe_params(c), auto_reset=False, sep_nm=0.0)


def fly_ceiling(c, comp, scn, orc, env, each):
    """places the case's aircraft (probe_batch: on and either side of the ceilings) on the oracle and, if given, the env, and steps the
    oracle c["steps"] times with the hold actions; each(t, actions) after every oracle step"""
    start, h, act, _ = probe_batch(comp, scn, np.random.default_rng(c["seed"]), c["B"], c["N"], c["dt"], c["discrete"])
    place(orc, env, start, h)
    for t in range(c["steps"]):
        orc.step(act)
        each(t, act)


class Coverage:
    """What the oracle saw, step by step: the inputs' coverage conditions of tests/test_noise_areas.py.  Per-area membership is the
    float64 reference's (pip_reference) on aircraft farther than 1e-3 nm from every noise edge; positions and altitudes of envs that
    were reset in the step are gone, so the per-area and the ceiling conditions count envs that go on."""

    def __init__(self, areas):
        self.areas = areas
        self.ceil = np.array([c for _, c, _ in areas])
        self.controlled = self.noise = self.two = self.below = self.outside = self.conflict = self.on_finish = 0
        self.on_ceiling = self.ulp_below = self.wrong = self.lived_on = 0
        self.area_hits = np.zeros(len(areas), np.int64)

    def add(self, orc, auto_reset, state_kept=False):
        """state_kept: the oracle itself runs without auto-reset (every env's state is the step's), auto_reset says what the case does"""
        self.add_step(orc.flags, orc.done, orc.x, orc.y, orc.h, auto_reset, state_kept)

    def add_block(self, ref, executed, auto_reset):
        """held_fuzz._add_block's watch: the executed steps [K, B] of one skip_reference result"""
        B = executed.shape[1]
        for j in np.flatnonzero(executed.any(1)):
            e = executed[j]
            x, y, h = (v.reshape(B, -1)[e].ravel() for v in ref["step_pos"][j])
            self.add_step(ref["step_flags"][j][e], ref["step_done"][j][e], x, y, h, auto_reset)

    def add_step(self, fl, done, x, y, h, auto_reset, state_kept=False):
        """one step's flags [B, N], done [B] and positions / altitudes [B N] after it"""
        import helpers as H
        B, N = fl.shape
        noise = (fl & H.F_NOISE) != 0
        self.controlled += int(((fl & H.F_INACTIVE) == 0).sum())
        self.noise += int(noise.sum())
        self.below += int((noise & ((fl & H.F_BELOW_MVA) != 0)).sum())
        self.outside += int((noise & ((fl & H.F_OUTSIDE) != 0)).sum())
        self.conflict += int((noise & ((fl & H.F_CONFLICT) != 0)).sum())
        done = np.asarray(done).astype(bool)
        self.lived_on += int((~done).sum())
        if auto_reset:
            self.on_finish += int((noise.any(1) & done).sum())
        live = np.repeat(~done if auto_reset and not state_kept else np.ones(B, bool), N) & ((fl.ravel() & H.F_INACTIVE) == 0)
        x, y, h = x[live], y[live], h[live]
        if len(x) == 0:
            return
        nz = noise.ravel()[live]
        rings_in = np.stack([pip_even_odd(x, y, r) for r, _, _ in self.areas], 1)
        clear = np.stack([edge_distance(x, y, r) for r, _, _ in self.areas], 1).min(1) > 1e-3
        below = h[:, None] < self.ceil[None, :]
        member = rings_in & below
        self.wrong += int((clear & (member.any(1) != nz)).sum())
        self.two += int((clear & nz & (member.sum(1) >= 2)).sum())
        self.area_hits += (member & (clear & nz)[:, None]).sum(0)
        # on a ceiling / one ulp below it, in that area's ring and in no other area below its ceiling: the flag is that area's alone
        for q, c in enumerate(self.ceil):
            others = np.delete(member, q, axis=1).any(1)
            at = clear & rings_in[:, q] & ~others
            on, under = at & (h == c), at & (h == np.nextafter(c, -np.inf))
            self.on_ceiling += int((on & ~nz).sum())
            self.ulp_below += int((under & nz).sum())
            self.wrong += int((on & nz).sum()) + int((under & ~nz).sum())

    def summary(self):
        return dict(controlled=self.controlled, noise=self.noise, share=self.noise / max(1, self.controlled), two=self.two, below_mva=self.below,
                    outside=self.outside, conflict=self.conflict, on_finish=self.on_finish, on_ceiling=self.on_ceiling,
                    ulp_below=self.ulp_below, wrong=self.wrong, lived_on=self.lived_on, area_hits=self.area_hits.tolist())
