"""Noise-abatement areas on random geometry (tests/noise_sectors.py), on every kernel.

CPU tests (no marker) fix what the GPU tests rely on: the lookup grid's candidate masks are a superset of the areas whose bounds hold a
point, the cell words survive fp32, the oracle's definition agrees with a plain float64 point-in-polygon + ceiling test away from edges,
the limits (16 areas, 17 refused) and the JSON round trip, and — flown on the oracle alone — that the cases of the GPU tests reach what
they are for (the coverage conditions).  GPU tests: point probes through every launch form, flights, the held kernels.

Cases and seeds: noise_sectors.FLIGHT_CASES (flight seeds 701 .. 708 on sector seeds 1 .. 4 and 7) with noise_sectors.CEILING_FLIGHTS
(seeds 721, 722), noise_sectors.probe_cases() (seeds 800 .. 815), noise_sectors.HELD_SEEDS (twelve of 9001 .. 9042, listed there).

Coverage, measured on the oracle alone (test_coverage_*): the flight family flags 47 % of its aircraft-steps under control (366 528 of
783 824).  No flown step lands an aircraft one float64 ulp below a ceiling (0 of 777 680 in FLIGHT_CASES; noise_sectors.py, at
CEILING_FLIGHTS, says why), so the flight family meets that state in two constructed flights that start there (185 aircraft-steps).
The held family (skip 41 %, lookahead 53 %, plan 37 %, branch 53 % of the executed aircraft-steps flagged) meets every flag condition and
an aircraft on a ceiling per kernel, and every area index over its kernels together; for the same reason as the flights it does not
meet one ulp below a ceiling — the probe family, whose K = 3 held blocks are counted step by step, holds the held kernels to that."""
import ctypes as C
import json

import numpy as np
import pytest

import bars
import helpers as H
import noise_sectors as NS
import skip_ref as R
from atc_hip import layout as L

CELLS = (0.0625, 0.125, 0.5, 2.0, 4.0)


def _compile(scn, cell):
    from envs.atc import scenarios
    return scenarios.compile_scenario(scn, grid_cell=cell)


def _cells(comp, blob):
    g = int(blob[L.H_OFF_GRID])
    nx, ny = int(blob[g + L.G_NX]), int(blob[g + L.G_NY])
    return g, nx, ny, np.asarray(blob[g + L.G_HDR:g + L.G_HDR + 2 * nx * ny]).reshape(ny, nx, 2)


def _cell_index(blob32, g, nx, ny, x, y):
    """the kernel's index arithmetic (csrc/atc_device.h: mva_cell_load) restated: fp32 (x - x0) * inv, truncated to an integer that is
    clamped as an UNSIGNED one — a point left of or below the grid's origin selects the LAST column or row"""
    x0, y0, inv = (np.float32(blob32[g + k]) for k in (L.G_X0, L.G_Y0, L.G_INV))
    fx = ((x.astype(np.float32) - x0) * inv).astype(np.float32)
    fy = ((y.astype(np.float32) - y0) * inv).astype(np.float32)
    ix, iy = np.trunc(fx.astype(np.float64)).astype(np.int64), np.trunc(fy.astype(np.float64)).astype(np.int64)
    return np.where(ix < 0, nx - 1, np.minimum(ix, nx - 1)), np.where(iy < 0, ny - 1, np.minimum(iy, ny - 1))


# ================================================================================================= CPU
@pytest.mark.parametrize("n_areas,base,seed", [(1, "LOWW", 1), (4, "random", 2), (16, "LOWW", 3), (16, "random", 4)])
@pytest.mark.parametrize("cell", CELLS)
def test_candidate_mask_is_a_superset(n_areas, base, seed, cell):
    scn = NS.noise_sector(seed, n_areas, base)
    comp = _compile(scn, cell)
    b32 = comp.blob32
    g, nx, ny, cells = _cells(comp, b32)
    pts = NS.noise_probe_points(comp, np.random.default_rng(300 + seed), n_random=4000).astype(np.float32)
    ix, iy = _cell_index(b32, g, nx, ny, pts[:, 0], pts[:, 1])
    mask = (np.abs(cells[iy, ix, 0]).astype(np.int64) >> 6) & 0xffff
    op, n_mva = int(b32[L.H_OFF_POLY]), int(b32[L.H_N_MVA])
    n_in = 0
    for q in range(n_areas):
        b = b32[op + (n_mva + q) * L.P_WORDS + L.P_MINX:][:4]          # the fp32 bounds the kernel and the fp32 oracle compare with
        inb = (b[0] <= pts[:, 0]) & (pts[:, 0] <= b[2]) & (b[1] <= pts[:, 1]) & (pts[:, 1] <= b[3])
        assert np.all((mask[inb] >> q) & 1), (q, pts[inb][((mask[inb] >> q) & 1) == 0][:3])
        n_in += int(inb.sum())
    assert n_in > 100
    assert (mask >> n_areas).max() == 0, "a bit of an area that does not exist"
    ring = np.concatenate([cells[0, :, 0], cells[-1, :, 0], cells[:, 0, 0], cells[:, -1, 0]])
    assert not ring.any(), "the outermost ring has no bit set"


def _full_word_cells(c):
    a = np.abs(c).astype(np.int64)
    return ((a >> 6) & 0x8000 != 0) & (a & (1 << 22) != 0) & (a & (1 << 23) != 0)


def _sector_with_full_word(scn):
    """the sector with its 16th area laid over a split cell inside the bounds of the corridor's horizontal triangle"""
    comp = _compile(scn, 0.5)
    g, nx, ny, cells = _cells(comp, comp.blob64)
    a = np.abs(cells[:, :, 0]).astype(np.int64)
    jj, ii = np.nonzero((a & (1 << 22) != 0) & (a & (1 << 23) != 0))
    assert len(jj), "no split cell inside the corridor triangle's bounds"
    x0, y0, inv = comp.blob64[g + L.G_X0], comp.blob64[g + L.G_Y0], comp.blob64[g + L.G_INV]
    cx, cy = x0 + (ii[0] + 0.5) / inv, y0 + (jj[0] + 0.5) / inv
    doc = json.loads(json.dumps(scn.doc))
    doc["noise_areas"][15]["ring"] = [[cx - 1.0, cy - 1.0], [cx + 1.0, cy - 1.0], [cx + 1.0, cy + 1.0], [cx - 1.0, cy + 1.0]]
    from atc_hip import sector_io
    out = sector_io.from_dict(doc)
    out.doc = doc
    return out


@pytest.mark.parametrize("base,seed", [("random", 1), ("random", 2)])
def test_cell_words_are_exact_in_fp32(base, seed):
    """(LOWW's corridor triangle lies inside one MVA polygon: no border splits a cell there, so the full word needs the random sectors)"""
    scn = NS.noise_sector(seed, 16, base)
    comp = _compile(scn, 0.5)
    if not _full_word_cells(_cells(comp, comp.blob64)[3][:, :, 0]).any():
        scn = _sector_with_full_word(scn)
        comp = _compile(scn, 0.5)
    _, _, _, c64 = _cells(comp, comp.blob64)
    _, _, _, c32 = _cells(comp, comp.blob32)
    assert np.array_equal(c32[:, :, 0].astype(np.float64), c64[:, :, 0])
    assert np.abs(c64[:, :, 0]).max() < 2.0 ** 24
    full = _full_word_cells(c64[:, :, 0])
    assert full.any(), "no cell carries a mask bit >= 15, the corridor bit and GRID_CELL_LINE together"
    assert np.array_equal(_full_word_cells(c32[:, :, 0]), full)


@pytest.mark.parametrize("n_areas,base,seed", [(1, "random", 1), (4, "LOWW", 2), (16, "random", 3), (16, "LOWW", 4)])
@pytest.mark.parametrize("discrete", [False, True])
def test_definition_against_float64_point_in_polygon(n_areas, base, seed, discrete):
    """Both oracle instantiations against NS.pip_reference at the position the oracle reports after the step."""
    from oracle import oracle as O
    scn = NS.noise_sector(seed, n_areas, base)
    comp, comp0 = _compile(scn, None), _compile(NS.without_noise(scn), None)
    areas = NS.areas_of(comp, scn)
    B, N = 1500, 16
    rng = np.random.default_rng(400 + seed)
    start, h, act, pts = NS.probe_batch(comp, scn, rng, B, N, 1.0, discrete, n_random=22000, on_ceiling=0.02)
    # the cap is on the DRAWN points: those nearer than 1e-3 nm to a noise edge or 1 ft to a ceiling are at most 10 % of the set
    _, _, clear_drawn = NS.pip_reference(pts[:, 0], pts[:, 1], h, areas)
    assert (~clear_drawn).mean() <= 0.10, (~clear_drawn).mean()
    p = O.make_params(discrete=discrete, shaping=bool(seed % 2))
    for dtype, tol in ((np.float32, 1e-5), (np.float64, 1e-12)):   # bars.py's 1e-5 max(1, |r|); float64: rounding of a few additions
        orc, orc0 = O.OracleEnv(comp, B, N, p, dtype), O.OracleEnv(comp0, B, N, p, dtype)
        NS.place([orc, orc0], None, start, h)
        orc.step(act)
        orc0.step(act)
        inside, pen, clear = NS.pip_reference(orc.x, orc.y, orc.h, areas)
        assert clear.mean() >= 0.85
        flagged = (orc.flags.ravel() & H.F_NOISE) != 0
        assert np.array_equal(flagged[clear], inside.any(1)[clear]), np.argwhere(clear & (flagged != inside.any(1)))[:5]
        assert np.array_equal(orc.flags.ravel() & ~np.uint16(H.F_NOISE), orc0.flags.ravel())
        r0 = orc0.ac_reward.ravel().astype(np.float64)
        got = r0 - orc.ac_reward.ravel().astype(np.float64)
        assert np.all(np.abs(got - pen)[clear] <= tol * np.maximum(1.0, np.abs(r0[clear]))), np.abs(got - pen)[clear].max()
        assert inside.any(1)[clear].mean() > 0.02 and (n_areas == 1 or (inside.sum(1) >= 2)[clear].any())


def test_limits_and_round_trip(tmp_path):
    from atc_hip import sector_io
    scn = NS.noise_sector(2, 16, "LOWW")
    comp = _compile(scn, 0.5)
    assert comp.n_noise == 16
    path = sector_io.dump(scn, str(tmp_path / "n16.json"))
    again = _compile(sector_io.load(path), 0.5)
    assert again.blob32.tobytes() == comp.blob32.tobytes() and again.blob64.tobytes() == comp.blob64.tobytes()
    doc = json.loads(json.dumps(scn.doc))
    doc["noise_areas"].append(dict(doc["noise_areas"][0], penalty=0.77))
    with pytest.raises(AssertionError, match="at most 16"):
        _compile(sector_io.from_dict(doc), 0.5)


def _check_coverage(s, n_areas_hit=None, ceilings=True):
    assert s["wrong"] == 0, s
    assert s["share"] >= 0.01 and s["two"] > 0 and s["below_mva"] > 0 and s["outside"] > 0 and s["conflict"] > 0, s
    assert s["on_finish"] > 0, s
    if ceilings:
        assert s["on_ceiling"] > 0 and s["ulp_below"] > 0, s
    if n_areas_hit is not None:
        assert all(c > 0 for c in n_areas_hit), n_areas_hit


def _merge(total, s):
    for k, v in s.items():
        if k not in ("share", "area_hits"):
            total[k] = total.get(k, 0) + v
    total["share"] = total["noise"] / max(1, total["controlled"])
    return total


def test_coverage_of_the_flight_cases():
    """The oracle alone on FLIGHT_CASES and CEILING_FLIGHTS (the flight family).  Every case flags noise and has envs that fly on past a
    step; one ulp below a ceiling is met in the constructed CEILING_FLIGHTS only (noise_sectors.py says why no flown step lands there)."""
    from fuzz_space import make_oracle
    total, hits16 = {}, np.zeros(16, np.int64)
    for c in NS.FLIGHT_CASES:
        scn, comp = NS.case_sector(c, grid=False)
        cov = NS.Coverage(NS.areas_of(comp, scn))
        NS.fly_oracle(comp, cov, **{k: v for k, v in c.items() if k != "sector"})
        s = cov.summary()
        print(c["sector"], "N", c["N"], s)
        assert s["noise"] > 0 and s["wrong"] == 0, (c, s)        # what the GPU test asserts as seen & F_NOISE
        assert s["lived_on"] > 0, ("every env ends on every step: the case replays its spawn", c, s)
        _merge(total, s)
        if c["sector"][1] == 16:
            hits16 += cov.area_hits
    print("flown cases:", total, hits16.tolist())
    for c in NS.CEILING_FLIGHTS:
        scn, comp = NS.case_sector(c, grid=False)
        cov = NS.Coverage(NS.areas_of(comp, scn))
        orc = make_oracle(comp, NS.ceiling_flight_params(c))
        NS.fly_ceiling(c, comp, scn, orc, None, lambda t, act: cov.add(orc, False))
        s = cov.summary()
        print("ceiling flight", c["sector"], "N", c["N"], s)
        assert s["on_ceiling"] > 0 and s["ulp_below"] > 0 and s["wrong"] == 0, (c, s)
        _merge(total, s)
    print("flight family:", total, hits16.tolist())
    _check_coverage(total, hits16)


def _probe_oracle(c, comp, scn, **overrides):
    """one probe case on the oracle alone: (orc after placement, start, h, actions)"""
    from fuzz_space import make_oracle
    rng = np.random.default_rng(c["seed"])
    start, h, act, _ = NS.probe_batch(comp, scn, rng, c["B"], c["N"], c["dt"], c["discrete"])
    orc = make_oracle(comp, NS.probe_params(c), **overrides)
    NS.place(orc, None, start, h)
    return orc, start, h, act


def test_coverage_of_the_probe_cases():
    total, hits16 = {}, np.zeros(16, np.int64)
    for c in NS.probe_cases():
        scn, comp = NS.case_sector(c, grid=False)
        cov = NS.Coverage(NS.areas_of(comp, scn))
        orc, _, _, act = _probe_oracle(c, comp, scn)
        for _ in range(3):      # the three steps of the rollouts and of the held blocks (step_skip, lookahead, plan, branch with K = 3)
            orc.step(act)
            cov.add(orc, True)
        _merge(total, cov.summary())
        if c["sector"][1] == 16:
            hits16 += cov.area_hits
    print("probe cases:", total, hits16.tolist())
    _check_coverage(total, hits16)


def test_coverage_of_the_held_cases():
    """The oracle alone on noise_case(HELD_SEEDS), counted on the EXECUTED steps of every held block (held_fuzz._add_block's watch), per
    kernel: the share, two areas at once, the three coincidences, noise on a finishing step and an unflagged aircraft on a ceiling (a
    discrete target that is a ceiling); over the kernels together: every area index of the 16-area sectors.  One ulp below a ceiling is
    not met here: the runners draw their own actions and fly from spawns, and no flown step lands there but by coincidence
    (noise_sectors.py, CEILING_FLIGHTS); the held kernels meet that state in the probe family, whose K = 3 blocks
    test_coverage_of_the_probe_cases counts step by step."""
    import branch_fuzz
    import held_fuzz
    names = held_fuzz.KERNELS + ("branch",)
    ev = {k: 0 for k in names}
    total, hits16 = {k: {} for k in names}, {k: np.zeros(16, np.int64) for k in names}
    for seed in NS.HELD_SEEDS:
        case = NS.noise_case(seed)
        cov = {k: NS.Coverage(NS.areas_of(case[1], case[0])) for k in names}
        rec = held_fuzz.run(seed, device=False, case=case, watch={k: cov[k].add_block for k in held_fuzz.KERNELS})
        for k in held_fuzz.KERNELS:
            ev[k] += rec["events"][k]["noise"]
        ev["branch"] += branch_fuzz.run(seed, device=False, case=case, watch=cov["branch"].add_block)["events"]["noise"]
        for k in names:
            _merge(total[k], cov[k].summary())
            if len(case[0].noise_areas) == 16:
                hits16[k] += cov[k].area_hits
    print("held cases: envs of blocks with F_NOISE", ev)
    assert all(v > 0 for v in ev.values()), ev
    for k in names:
        print("held cases,", k, total[k], hits16[k].tolist())
        _check_coverage(total[k], None, ceilings=False)
        assert total[k]["on_ceiling"] > 0, (k, total[k])
    family = sum(hits16.values())
    print("held cases, area indices over the family:", family.tolist())
    assert all(n > 0 for n in family), family


# ================================================================================================= GPU
def _got(env, ret):
    obs, rew, done, info = ret
    cpu = lambda t: t.cpu().numpy()   # noqa: E731
    B, N = env.B, env.N
    return {"flags": cpu(info["flags"]), "done": cpu(done), "obs": cpu(obs).reshape(B, N, 10), "reward": cpu(rew),
            "raw_obs": cpu(info["original_state"]).reshape(B, N, 10), "ac_reward": cpu(info["aircraft_reward"]),
            "min_sep": cpu(info["min_separation"]), "term_obs": cpu(info["terminal_observation"]).reshape(B, N, 10)}


@pytest.mark.gpu
@pytest.mark.parametrize("c", NS.probe_cases(), ids=lambda c: "N%d-cell%s-%s-%s" % (c["N"], c["grid_cell"], "discrete" if c["discrete"] else "continuous",
                                                                                  "shaping" if c["shaping"] else "plain"))
def test_point_probe_through_every_launch_form(c):
    import torch
    import branch_ref as BR
    import held_fuzz
    from fuzz_space import make_env, make_oracle
    scn, comp = NS.case_sector(c)
    kw = NS.probe_params(c)
    B, N = c["B"], c["N"]
    half = bars.half_range(comp)
    rng = np.random.default_rng(c["seed"])
    start, h, act, _ = NS.probe_batch(comp, scn, rng, B, N, c["dt"], c["discrete"])
    orc = make_oracle(comp, kw)
    env, fast = make_env(scn, kw), make_env(scn, kw, full=False)
    seen = 0
    try:
        def again(e=env):
            NS.place(orc, e, start, h)

        def oracle_step(o=orc):
            nonlocal seen
            o.step(act)
            seen |= int(np.bitwise_or.reduce(o.flags.ravel()))

        # step, full and fast
        again()
        ret = env.step(act)
        term = ret[3]["terminal_observation"]      # (the env's bound tensor: the fast rollouts below do not write it, the oracle's steps do)
        got = _got(env, ret)
        oracle_step()
        bars.check_step(got, orc, True, half, "step full")
        bars.check_state(env, orc)
        orc_f = make_oracle(comp, kw)     # (the fast form is a second env, with an oracle of its own)
        NS.place(orc_f, fast, start, h)
        o, r, d, info = fast.step(act)
        oracle_step(orc_f)
        bars.check_step({"flags": info["flags"].cpu().numpy(), "done": d.cpu().numpy(), "obs": o.cpu().numpy().reshape(B, N, 10),
                         "reward": r.cpu().numpy()}, orc_f, True, half, "step fast")
        # rollout, T = 3 and hold = 3
        for tag, blocks, hold in (("rollout T=3", 3, 1), ("rollout hold=3", 1, 3)):
            again()
            out = env.rollout(torch.as_tensor(np.stack([act] * blocks)), hold=hold)
            for t in range(3):
                oracle_step()
                bars.check_step({"flags": out["flags"][t].cpu().numpy(), "done": out["done"][t].cpu().numpy(),
                                 "obs": out["obs"][t].cpu().numpy().reshape(B, N, 10), "reward": out["reward"][t].cpu().numpy()},
                                orc, True, half, (tag, t))
            bars.check_state(env, orc)
        # step_skip, K = 1 and K = 3
        for K in (1, 3):
            again()
            orc.term_obs[...] = term.cpu().numpy().reshape(B, N, 10)
            ref = R.skip_reference(orc, act, K)
            seen |= int(np.bitwise_or.reduce(ref["flags"].ravel()))
            bars.check_skip_outputs(held_fuzz._skip_outputs(env, env.step_skip(act, K), True), ref, half, True, "step_skip K=%d" % K)
            bars.check_state(env, orc)
        # lookahead M = 2, lookahead_plan H = 2: candidate 0 holds, candidate 1 climbs / descends through the ceilings
        again()
        other = act.copy()
        other[..., 1] = (rng.integers(20, 111, (B, N)) if c["discrete"] else rng.integers(-57, -26, (B, N)) / 64.0).astype(np.float32)
        ok = ~R.wide_envs(orc)
        snap = H.snapshot(env)
        outputs = ("flags", "min_sep", "ac_reward", "obs")
        cand = np.stack([act, other])
        refs = R.candidate_references(orc, cand, 3)
        res = {k: v.cpu().numpy() for k, v in env.lookahead(torch.as_tensor(cand, device=env.device), 3, outputs=outputs).items()}
        for m in range(2):
            bars.check_candidate_outputs({k: v[m] for k, v in res.items()}, refs[m], ok, half, tag=("lookahead", m))
        plans = np.stack([np.stack([act, other]), np.stack([other, act])])
        refs = R.plan_references(orc, plans, 2)
        res = {k: v.cpu().numpy() for k, v in env.lookahead_plan(torch.as_tensor(plans, device=env.device), 2,
                                                                  outputs=("seg_reward",) + outputs).items()}
        for m in range(2):
            g = {k: v[m] for k, v in res.items()}
            bars.check_candidate_outputs({k: v for k, v in g.items() if k != "seg_reward"}, refs[m], ok, half, tag=("plan", m))
            bars.check_plan_segments(g["seg_reward"], refs[m], ok, 2, tag=("plan", m))
        H.bytes_equal(env, snap)
        bars.check_state(env, orc)
        # branch into a child batch
        child = BR.child_of(env, 2, lambda b: make_env(scn, kw, B=b, grid_cell=env.grid_cell))
        try:
            env.branch(torch.as_tensor(cand, device=env.device), 3, into=child)
            names = ("obs", "reward", "done", "flags", "ac_reward", "min_sep")
            got = {k: getattr(child, k).cpu().numpy().reshape((2, B) + ((-1,) if getattr(child, k).dim() > 1 else ())) for k in names}
            got["n_steps"] = child.frame_steps.cpu().numpy().reshape(2, B)
            H.bytes_equal(env, snap)
            BR.oracle_branch(orc, cand, 3, ok, BR.child_check(child, orc, got, half, ok, "probe branch"))
        finally:
            child.close()
        assert seen & H.F_NOISE
    finally:
        env.close()
        fast.close()


@pytest.mark.gpu
@pytest.mark.parametrize("c", NS.FLIGHT_CASES, ids=lambda c: "%s%d-N%d-dt%g" % (c["sector"][2], c["sector"][1], c["N"], c["dt"]))
def test_flight_on_noise_sectors_vs_oracle(c):
    from fuzz_space import run_vs_oracle
    scn, comp = NS.case_sector(c)
    n_done, seen = run_vs_oracle(scn, comp, **{k: v for k, v in c.items() if k != "sector"})
    assert seen & H.F_NOISE


@pytest.mark.gpu
@pytest.mark.parametrize("c", NS.CEILING_FLIGHTS, ids=lambda c: "%s%d-N%d-dt%g" % (c["sector"][2], c["sector"][1], c["N"], c["dt"]))
def test_flight_from_the_ceilings_vs_oracle(c):
    """aircraft placed one ulp below, on and one ulp above the ceilings and flown on through the areas (noise_sectors.CEILING_FLIGHTS)"""
    from fuzz_space import make_env, make_oracle
    scn, comp = NS.case_sector(c)
    kw = NS.ceiling_flight_params(c)
    half = bars.half_range(comp)
    orc, env = make_oracle(comp, kw), make_env(scn, kw)
    seen = 0
    try:
        def each(t, act):
            nonlocal seen
            bars.check_step(_got(env, env.step(act)), orc, True, half, ("ceiling flight", t))
            seen |= int(np.bitwise_or.reduce(orc.flags.ravel()))

        NS.fly_ceiling(c, comp, scn, orc, env, each)
        bars.check_state(env, orc)
        assert seen & H.F_NOISE
    finally:
        env.close()


@pytest.mark.gpu
def test_held_kernels_on_noise_sectors():
    import branch_fuzz
    import held_fuzz
    ev = {k: 0 for k in held_fuzz.KERNELS}
    branch = 0
    for seed in NS.HELD_SEEDS:
        case = NS.noise_case(seed)
        rec = held_fuzz.run(seed, case=case)
        for k in ev:
            ev[k] += rec["events"][k]["noise"]
        branch += branch_fuzz.run(seed, case=case)["events"]["noise"]
    assert all(v > 0 for v in ev.values()) and branch > 0, (ev, branch)


@pytest.mark.gpu
def test_create_refuses_17_areas():
    from atc_hip import lib
    comp = _compile(NS.noise_sector(2, 16, "LOWW"), 0.5)
    blob = comp.blob32.copy()
    assert blob[L.H_N_NOISE] == 16.0
    blob[L.H_N_NOISE] = 17.0
    handle = C.c_void_p()
    rc = lib.load().atc_scenario_create(blob.ctypes.data_as(C.c_void_p), blob.size, 0, C.byref(handle))
    assert rc == -1 and not handle.value
    assert b"16 noise" in lib.load().atc_last_error()
