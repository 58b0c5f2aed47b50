"""The fuzz mode space in one place: the case draw, the action draw, the kw -> env / oracle mapping and the lock-step run against the
fp32 oracle.  TEST INFRASTRUCTURE ONLY; importing it needs no GPU.

  parity_case(seed)   one configuration of tests/test_fuzz_parity.py; tests/held_fuzz.py and tests/ref_diff.py draw theirs from it
  draw_actions        THE action draw: every harness that says "as run_vs_oracle draws them" calls this
  make_env / make_oracle   the one place that spells out the AtcVecEnv / SimParameters / oracle.make_params keyword lists
  run_vs_oracle       the run behind test_hip_parity, test_fuzz_parity, test_kernel_matrix and tests/fuzz_debug.py
tests/test_fuzz_draws.py pins the draws: the seed -> case records under profiles/ stay valid."""
import numpy as np

import bars
import helpers as H

NON_DYADIC = (0.05, 0.1, 0.15, 0.3, 0.7, 1.3, 3.7, 0.37, 2.1)     # parity_case's round-6 timesteps


class Mismatch(AssertionError):
    """a failed comparison of a fuzz harness (tests/held_fuzz.py, tests/ref_diff.py), with the context tests/fuzz_debug.py prints"""

    def __init__(self, ctx, what, where):
        super().__init__("%s: %s" % (where, what))
        self.ctx, self.what = ctx, what


def _n_cu():
    """CUs of the device the case will run on (256, MI355X's, where there is none: tools that only list the cases)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def parity_case(seed, n_cu=None):
    from envs.atc import scenarios
    rng = np.random.default_rng(seed)
    N = int(rng.choice([1, 1, 2, 3, 5, 8, 9, 15, 16, 16, 17, 24, 32, 33, 48, 63, 64]))
    kind = rng.choice(["LOWW", "LOWW_random", "Simple", "Dense"])
    if N > 54:
        kind = "Dense"      # the other sectors have fewer conflict-free spawn slots
    scn = scenarios.LOWWDense() if kind == "Dense" else H.make_scenario(str(kind))
    grid_cell = [None, 0.25, 0.5, 1.0][int(rng.integers(4))]
    comp = scenarios.compile_scenario(scn, grid_cell=grid_cell)
    rollout = int(rng.choice([0, 0, 0, 4]))
    kw = dict(B=int(rng.integers(1, 400)), N=N, steps=int(rng.choice([60, 120, 200])), seed=int(seed),
              dt=float(rng.choice([1.0, 1.0, 2.0, 5.0])), discrete=bool(rng.integers(2)),
              spawn=str(rng.choice(["lattice", "random"])) if comp.n_entry > 1 else "lattice",
              hold=int(rng.choice([1, 7, 20])), grid_cell=grid_cell, use_rollout=rollout,
              timestep_limit=int(rng.choice([6000, 6000, 40])), full=bool(rng.integers(2)),
              shaping=bool(rng.integers(4) > 0), normalize=bool(rng.integers(4) > 0),
              sep_nm=float(rng.choice([3.0, 3.0, 0.0, 5.0])), keep_active=bool(rng.integers(5) == 0))
    kw["held_hint"] = bool(rng.integers(2))   # drawn last: the cases of earlier sweeps keep their configurations
    # atc_rollout_hold with hold > 1 (drawn after everything else for the same reason): a quarter of the cases
    rh = int(rng.choice([1, 1, 1, 1, 1, 1, 4, 20]))
    if rh > 1:
        rollout = rh * int(rng.choice([1, 2, 5]))
        kw.update(use_rollout=rollout, rollout_hold=rh, hold=rh * int(rng.choice([1, 2])))
    if rollout:
        kw["steps"] = max(rollout, (kw["steps"] // rollout) * rollout)
    # round 4 (drawn after everything else: earlier sweeps keep their configurations): a third of the cases replace the
    # drawn cell size by the SHIPPED defaults — 0.125 nm explicitly, or "auto" (atc_hip.vec_env.auto_grid_cell: 0.125 nm for
    # every batch this sweep draws), whose compiled sector must be the one the env builds for itself
    pick = int(rng.integers(6))
    if pick < 2:
        kw["grid_cell"] = 0.125 if pick == 0 else "auto"
        comp = scenarios.compile_scenario(scn, grid_cell=0.125)
    elif pick == 2 and kind != "Dense":   # 0.0625 nm: what `auto` picks from 4 096 aircraft slots up (bigger than this sweep's batches)
        kw["grid_cell"] = 0.0625
        comp = scenarios.compile_scenario(scn, grid_cell=0.125)
    # round 4, drawn last again: a quarter of the cases whose aircraft count is a power of two get a batch that is a whole number of
    # workgroups — the launches then run the all-valid kernel instantiations (csrc/atc_step.hip: make_ids<W, ALLV>), the others
    # the general ones
    if int(rng.integers(4)) == 0 and (N & (N - 1)) == 0:
        per = max(1, 256 // N)
        kw["B"] = per * max(1, kw["B"] // per // (4 if N == 1 else 1))
    # round 5, drawn last: a tenth of the cases carry actions OUTSIDE the action space (U(-4, 4) and beyond) — the reference
    # enforces none (atc_gym.py:128-141) and never validates or wraps a heading (model.py:104-120)
    if int(rng.integers(10)) == 0:
        kw["wild"] = float(rng.choice([0.05, 0.3, 1.0]))
    # round 6, drawn last: a third of the cases step at a timestep that is NOT a small dyadic multiple (SimParameters.timestep is
    # any float, model.py:132-145): the class of inputs the sweeps of rounds 2-5 never drew (the fp32 altitude accumulator was
    # only exact at 1 / 2 / 5 s; tests/golden/g12 pins the reference at these)
    if int(rng.integers(3)) == 0:
        kw["dt"] = float(rng.choice(NON_DYADIC))
    # round 6 (ABI 21), drawn last: one-aircraft envs stepped by multi-step launches get, every second time, a batch of whole
    # 256-env workgroups — with a lookup grid and no noise-abatement areas that launch answers the MVA lookup from the sector's
    # LDS-resident table (k_step<1, ..., LDSG>; tests/test_lds_table.py)
    if N == 1 and kw["use_rollout"] and int(rng.integers(2)) == 0:
        kw["B"] = 256 * int(rng.integers(1, 3))
    # drawn last: one case in 50 never resets (the reference's FPS protocol, learning/atc-gym-compute-performance.py) — 500 to 5 000
    # steps with actions held for hundreds of steps, long enough to fly off the position grid (include/atc_step.h); B x N <= 2 048
    if int(rng.integers(50)) == 0:
        kw["auto_reset"] = False
        kw["hold"] = int(rng.choice([200, 400, 1000]))       # (multiples of every rollout_hold)
        kw["steps"] = int(rng.choice([500, 1000, 2000, 5000]))
        kw["B"] = min(kw["B"], max(1, 2048 // N))
        if kw["use_rollout"]:
            kw["steps"] = -(-kw["steps"] // kw["use_rollout"]) * kw["use_rollout"]
    # drawn last: one case in 25 whose aircraft count is a power of two flies a fast multi-step launch of whole workgroups just above
    # the latency-bound limit (2 wavefronts per SIMD of the device at hand), i.e. the all-valid THROUGHPUT instantiation
    # (k_step<W, false, false, true>) under whatever modes the case drew; two launches, so that the oracle's 131 072 aircraft stay cheap
    if int(rng.integers(25)) == 0 and (N & (N - 1)) == 0:
        n_cu = n_cu or _n_cu()
        T = kw["use_rollout"] or 4
        kw.update(B=(512 * n_cu + 256 * int(rng.integers(1, 4))) // N, full=False, use_rollout=T, steps=2 * T)
    return scn, comp, kw


def draw_actions(rng, shape, discrete, wild, heading_wild):
    """Actions [*shape, 3] (shape ends in B, N): discrete indices when discrete, U(-1.05, 1.05) otherwise, and with wild > 0 that share of
    the components from U(-4, 4) (a tenth of those a further factor 50 out) — drawn after the regular block, so a case without wild draws
    keeps its stream.  heading_wild says where the HEADING component takes part in the wild share: True — in every env (run_vs_oracle,
    tests/ref_diff.py); False — in none (candidates: a heading target outside the 32-bit heading field is WIDE, and a WIDE env is not
    evaluated by the look-ahead calls); [B] bool — in those envs."""
    full = tuple(shape) + (3,)
    if discrete:
        act = np.floor(rng.uniform(0, 1, full) * np.array([20, 380, 360])).astype(np.float32)
    else:
        act = rng.uniform(-1.05, 1.05, full).astype(np.float32)
    if wild > 0.0:
        out_of_space = rng.uniform(-4.0, 4.0, full) * np.where(rng.uniform(size=full) < 0.1, 50.0, 1.0)
        if discrete:
            out_of_space = np.floor(out_of_space * np.array([20, 380, 360]))
        pick = rng.uniform(size=full) < wild
        if heading_wild is not True:
            mask = np.asarray(heading_wild, bool)
            pick[..., 2] &= mask[:, None] if mask.ndim else mask
        act = np.where(pick, out_of_space, act).astype(np.float32)
    return act


def make_env(scn, kw, **overrides):
    """the AtcVecEnv of a case's kw (parity_case's keys; `traffic` and `auto_reset` where the case has them)"""
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import model
    kw = dict(kw, **overrides)
    sp = model.SimParameters(kw["dt"], discrete_action_space=kw["discrete"], reward_shaping=kw["shaping"], normalize_state=kw["normalize"])
    full = kw["full"]
    return AtcVecEnv(kw["B"], kw["N"], sim_parameters=sp, scenario=scn, auto_reset=kw.get("auto_reset", True), spawn=kw["spawn"],
                     seed=kw["seed"], grid_cell=kw["grid_cell"], want_raw_obs=full, want_ac_reward=full, want_min_sep=full,
                     want_term_obs=full, timestep_limit=kw["timestep_limit"], sep_nm=kw["sep_nm"], keep_active=kw["keep_active"],
                     traffic=kw.get("traffic", 0))


def make_oracle(comp, kw, dtype=np.float32, **overrides):
    """the oracle.OracleEnv of the same kw, in the fp32 (spec) or the float64 (reference) instantiation"""
    from oracle import oracle as O
    kw = dict(kw, **overrides)
    p = O.make_params(dt=kw["dt"], discrete=kw["discrete"], auto_reset=kw.get("auto_reset", True), random_entry=(kw["spawn"] == "random"),
                      seed=kw["seed"], timestep_limit=kw["timestep_limit"], shaping=kw["shaping"], normalize=kw["normalize"],
                      sep_nm=kw["sep_nm"], keep_active=kw["keep_active"])
    return O.OracleEnv(comp, kw["B"], kw["N"], p, dtype)


def run_vs_oracle(scen_obj, comp, B, N, steps, seed, dt=1.0, discrete=False, spawn="lattice", hold=20, grid_cell=0.5,
                  use_rollout=0, timestep_limit=6000, full=True, shaping=True, normalize=True, sep_nm=3.0,
                  keep_active=False, held_hint=False, rollout_hold=1, wild=0.0, auto_reset=True, check=bars.check_step):
    """full=False drives the fast kernel variant (obs / reward / done / flags only), full=True the one with every optional
    output; everything the variant produces is compared with the fp32 oracle.  held_hint: single steps that repeat the
    previous step's action array are launched with ATC_M_ACTIONS_HELD (must change nothing).
    rollout_hold > 1 (with use_rollout): the multi-step launches go through atc_rollout_hold — one action block per
    `rollout_hold` steps (frame skip, learning/atc-gym-demo.py:18-19), whose repeated steps skip the last-action bookkeeping
    inside the kernel; the oracle is stepped once per step with the block's actions.
    wild > 0: that fraction of the drawn action COMPONENTS lies outside the action space — U(-4, 4) (a tenth of those a further
    factor 50 out): the reference enforces no Box (atc_gym.py:128-141); speed / altitude targets beyond their limits are refused,
    heading targets are never validated and headings leave the state format's 32-bit range (include/atc_step.h, ABI 19).
    auto_reset=False: no env is ever reset — the reference's FPS protocol; held long enough, aircraft fly off the position grid.
    check(got, orc, normalize, half_range, step): the per-step comparison (tests/fuzz_debug.py passes a verbose one)."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    kw = dict(B=B, N=N, seed=seed, dt=dt, discrete=discrete, spawn=spawn, grid_cell=grid_cell, timestep_limit=timestep_limit, full=full,
              shaping=shaping, normalize=normalize, sep_nm=sep_nm, keep_active=keep_active, auto_reset=auto_reset)
    env, orc = make_env(scen_obj, kw), make_oracle(comp, kw)
    o0 = env.obs.cpu().numpy().reshape(B, N, 10)
    assert np.all(np.abs(o0 - orc.obs) <= 1e-5 * np.maximum(1.0, np.abs(orc.obs)))
    rng = np.random.default_rng(seed)
    half_range = bars.half_range(comp)
    n_done = 0
    seen = 0
    act = None
    if use_rollout:
        assert steps % use_rollout == 0
    if rollout_hold > 1:
        assert use_rollout and use_rollout % rollout_hold == 0 and hold % rollout_hold == 0
    t = 0
    while t < steps:
        chunk = use_rollout or 1
        acts = []
        repeated = act is not None and t % hold != 0
        for c in range(chunk):
            if (t + c) % hold == 0 or act is None:
                act = draw_actions(rng, (B, N), discrete, wild, True)
            acts.append(act)
        if use_rollout:
            step = 1
            if rollout_hold > 1:
                assert all(acts[c] is acts[c - c % rollout_hold] for c in range(chunk))   # blocks are constant by construction
                step = rollout_hold
            # full=True: the launch gets [T, ...] buffers for every optional output — without them AtcVecEnv.rollout asks for the
            # required four only and the library launches a fast form whatever the env was built with.  (Zeroed: term_obs is written
            # for envs that were auto-reset only, and the oracle's stays zero elsewhere — so must the launch's.)
            bufs = None if not full else {k: torch.zeros((chunk,) + shape, dtype=dt, device=env.device) for k, shape, dt in (
                ("obs", (B, N * 10), torch.float32), ("reward", (B,), torch.float32), ("done", (B,), torch.uint8),
                ("flags", (B, N), torch.int16), ("raw_obs", (B, N * 10), torch.float32), ("ac_reward", (B, N), torch.float32),
                ("min_sep", (B,), torch.float32), ("term_obs", (B, N * 10), torch.float32))}
            out = env.rollout(torch.as_tensor(np.stack(acts[::step])), out=bufs, hold=step)
            res = [(out["obs"][c], out["reward"][c], out["done"][c], out["flags"][c]) for c in range(chunk)]
        else:
            o, r, d, info = env.step(acts[0], held=held_hint and repeated)
            res = [(o, r, d, info["flags"])]
        for c in range(chunk):
            orc.step(acts[c])
            o, r, d, fl = res[c]
            got = {"flags": fl.cpu().numpy(), "done": d.cpu().numpy(), "obs": o.cpu().numpy().reshape(B, N, 10), "reward": r.cpu().numpy()}
            if full:
                # optional outputs (of the single step, or row c of the multi-step launch's buffers)
                if use_rollout:
                    raw, acr, msep, tob = (out[k][c].cpu().numpy() for k in ("raw_obs", "ac_reward", "min_sep", "term_obs"))
                else:
                    raw, acr, msep, tob = (info[k].cpu().numpy() for k in ("original_state", "aircraft_reward", "min_separation",
                                                                           "terminal_observation"))
                got.update(raw_obs=raw.reshape(B, N, 10), ac_reward=acr, min_sep=msep, term_obs=tob.reshape(B, N, 10))
            check(got, orc, normalize, half_range, t + c)   # flags / done exact, obs / rewards 1e-5, optional outputs: tests/bars.py
            n_done += int(orc.done.sum())
            seen |= int(np.bitwise_or.reduce(orc.flags.ravel()))
        t += chunk
    # persistent state after the run: integer state exact, float state within tolerance (tests/bars.py)
    bars.check_state(env, orc, total_reward=False)
    env.close()
    return n_done, seen
