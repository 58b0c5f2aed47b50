"""A call-sequence driver: one AtcVecEnv next to one fp32 oracle env, a scripted list of operations applied to both.
TEST INFRASTRUCTURE ONLY (in the style of tests/skip_ref.py).

The step kernels carry shortcuts that are only correct given what the PREVIOUS call left behind (include/atc_step.h: the last-action
record skipped under ATC_M_ACTIONS_HELD and inside held blocks, envs with timesteps == 0 handled in full, an env that ended early
inside atc_step_skip waiting in its spawn state, the WIDE side records).  The per-entry-point tests run each entry point in a loop of
its own; a Session interleaves them.  Every operation is applied to the oracle and — unless the session was made with device=False,
which is how the CPU tests look at what a script contains — to the device env, and then EVERYTHING is compared: the operation's
outputs by the bars of tests/bars.py, the whole persistent state bit for bit, sentinel rows of masked calls.

OPERATION TABLE — any new entry point or state-dependent shortcut of the library belongs here:
    ("step", "fresh" | "repeat" | "held")   env.step                    orc.step          repeat / held reuse the previous actions
    ("skip", K)                             env.step_skip               skip_ref.skip_reference
    ("rollout", T, hold, full)              env.rollout (out buffers iff full)            T x orc.step
    ("reset", mask kind)                    env.reset                   orc.reset         kinds: MASK_KINDS
    ("observe", mask kind)                  env.observe                 orc.observe       into sentinel-filled observation arrays
    ("traffic",)                            env.observe_traffic         traffic_ref.traffic_reference on the ORACLE's state
    ("set_state",)                          env.set_state               orc.set_state     six aircraft: two at a WIDE heading, two beyond
                                                                                          the position grid, two on a winning state
    ("set_last_action",)                    env.set_last_action         orc.set_last_action
Everything an operation needs beyond its tuple (actions, masks, aircraft) is drawn from a generator seeded by (case seed, index of the
operation), so a script means the same inputs on the oracle alone and next to the device.

held=True is a promise (ATC_M_ACTIONS_HELD): `held_is_legal` is the ONE statement of when a script may make it, and every scripted
held step is checked against it before anything runs."""
import collections

import numpy as np

import bars
import fuzz_space
import helpers as H
import skip_ref
import traffic_ref

SENTINEL = np.float32(-7.25e8)   # no observation word of any sector comes near it
MASK_KINDS = ("random", "zero", "one", "none", "placed")   # placed: the envs the last set_state touched
TRAFFIC_K = 3
SKIP_KS = (1, 2, 5, 20)
I32_EDGE = (-2 ** 31, 2 ** 31 - 1)

Case = collections.namedtuple("Case", "N B auto_reset normalize dt keep_active spawn timestep_limit sep_nm seed")


class IllegalScript(AssertionError):
    pass


def setup(N):
    """sector of a case: LOWW with its random entry points for one-aircraft envs, the dense sector (noise areas) otherwise"""
    from envs.atc import scenarios
    key = ("session", N == 1)
    if key not in H._compiled:
        scn = scenarios.LOWW(random_entrypoints=True) if N == 1 else scenarios.LOWWDense()
        H._compiled[key] = (scn, scenarios.compile_scenario(scn, grid_cell=0.5))
    return H._compiled[key]


def held_is_legal(prev_actions, la_touched, actions):
    """include/atc_step.h, ATC_M_ACTIONS_HELD: `actions` holds, for every aircraft, the same BITS as the previous step of these envs —
    the last step of whichever stepping call came before (atc_step, the last block of a rollout, the block of a frame skip) —, and
    nobody wrote a last-action record since.  Resets, observations and placed aircraft in between are allowed: envs reset since
    their last step are handled in full.  Returns (legal, why not)."""
    if prev_actions is None:
        return False, "no step before it"
    if la_touched:
        return False, "set_last_action since the previous step"
    if not np.array_equal(np.asarray(prev_actions, np.float32).view(np.int32), np.asarray(actions, np.float32).view(np.int32)):
        return False, "the actions differ from the previous step's"
    return True, ""


def draw_actions(rng, B, N):
    """a third of the components outside the action space (tests/held_tools.py::skip_actions)"""
    return fuzz_space.draw_actions(rng, (B, N), False, 0.33, True)


class Session:
    def __init__(self, case, device=True):
        from oracle import oracle as O
        self.case = case
        self.scn, self.comp = setup(case.N)
        c = case
        self.orc = O.OracleEnv(self.comp, c.B, c.N, O.make_params(
            dt=c.dt, normalize=c.normalize, auto_reset=c.auto_reset, random_entry=c.spawn == "random", seed=c.seed,
            timestep_limit=c.timestep_limit, sep_nm=c.sep_nm, keep_active=c.keep_active), np.float32)
        self.env = None
        if device:
            from atc_hip.vec_env import AtcVecEnv
            from envs.atc import model
            self.env = AtcVecEnv(c.B, c.N, sim_parameters=model.SimParameters(c.dt, normalize_state=c.normalize), scenario=self.scn,
                                 auto_reset=c.auto_reset, spawn=c.spawn, seed=c.seed, grid_cell=0.5, want_raw_obs=True, want_ac_reward=True,
                                 want_min_sep=True, want_term_obs=True, timestep_limit=c.timestep_limit, sep_nm=c.sep_nm,
                                 keep_active=c.keep_active, traffic=TRAFFIC_K if c.N > 1 else 0)
        self.half = bars.half_range(self.comp)
        self.done_ops = []            # the script so far
        self.prev_actions = None      # action bits of the last step of the last stepping operation
        self.la_touched = False       # set_last_action since then
        self.placed = []              # envs the last set_state touched
        self.win_pending = []         # (env, slot) placed on the winning state: the next fresh actions fly them into the corridor
        self.record = []              # what the ORACLE saw, one dict per operation (tests look for the interactions in it)
        if self.env is not None:
            self._guard("the constructor's reset", self._check_reset_obs, np.ones(c.B, bool))
            self._guard("the constructor's reset", bars.check_state, self.env, self.orc)

    # -------------------------------------------------------------------------------------------------------- plumbing
    def _guard(self, what, fn, *args):
        """the first mismatch reports the operation index, the operation and the script so far"""
        try:
            return fn(*args)
        except IllegalScript:
            raise
        except AssertionError as exc:
            raise AssertionError("call sequence %s: operation %d %r: %s\nscript so far: %r" % (
                self.case, len(self.done_ops), what, exc, self.done_ops)) from exc

    def _cpu(self, t):
        return t.cpu().numpy()

    def _rng(self):
        return np.random.default_rng([self.case.seed, len(self.done_ops)])

    def _mask(self, kind, rng):
        B = self.case.B
        if kind == "none":
            return None
        if kind == "zero":
            return np.zeros(B, np.uint8)
        if kind == "one":
            return np.ones(B, np.uint8)
        if kind == "placed":
            m = np.zeros(B, np.uint8)
            m[self.placed] = 7          # any non-zero byte selects
            return m
        assert kind == "random", kind
        return (rng.uniform(size=B) < 0.4).astype(np.uint8)

    def _wide_active(self):
        """aircraft at a WIDE heading and under control, on the oracle"""
        o = self.orc
        act = traffic_ref.active_bits(o.active_mask, o.N).reshape(-1)
        return int((np.isin(o.phi_fix, I32_EDGE) & act).sum())

    def _fresh_actions(self, rng, blocks=None):
        B, N = self.case.B, self.case.N
        a = draw_actions(rng, B, N) if blocks is None else np.stack([draw_actions(rng, B, N) for _ in range(blocks)])
        for e, k in self.win_pending:
            a[..., e, k, :] = H.WIN_ACTION
        self.win_pending = []
        return a

    def _step_outputs(self):
        env, B, N = self.env, self.case.B, self.case.N
        return {"flags": self._cpu(env.flags), "done": self._cpu(env.done), "obs": self._cpu(env.obs).reshape(B, N, 10),
                "reward": self._cpu(env.reward), "raw_obs": self._cpu(env.raw_obs).reshape(B, N, 10), "ac_reward": self._cpu(env.ac_reward),
                "min_sep": self._cpu(env.min_sep), "term_obs": self._cpu(env.term_obs).reshape(B, N, 10)}

    def _check_reset_obs(self, m, exact_words=()):
        """rows of selected envs against the oracle's (raw observations: the bar of an auto-reset row of a step); the others still
        hold the sentinel"""
        got = self._cpu(self.env.obs).reshape(self.case.B, self.case.N, 10)
        ref = self.orc.obs
        assert np.all(got[~m] == SENTINEL) and np.all(ref[~m] == SENTINEL), "an unselected env's observation row was written"
        assert np.all(np.abs(got[m] - ref[m]) <= 1e-5 * bars.obs_scale(ref[m], self.case.normalize, self.half)), "obs"
        for w in exact_words:
            assert np.array_equal(got[m][..., w], ref[m][..., w]), "raw word %d" % w

    def _check_traffic(self):
        o, c = self.orc, self.case
        st = dict(x_fix=o.px.reshape(c.B, c.N), y_fix=o.py.reshape(c.B, c.N), h=o.h.reshape(c.B, c.N),
                  P=o.phi_counts.astype(np.float64).reshape(c.B, c.N), v_fix=o.v_fix.view(np.uint32).reshape(c.B, c.N), mask=o.active_mask)
        ref = traffic_ref.traffic_reference(st, self.comp.pos_origin, self.comp.pos_k)
        if self.env is not None:
            bad = traffic_ref.compare(self._cpu(self.env.traffic), ref, TRAFFIC_K, traffic_ref.norm_scales(self.comp) if c.normalize else None)
            assert not bad, ("traffic", bad)
        return ref

    # -------------------------------------------------------------------------------------------------------- operations
    def apply(self, op):
        rec = self._guard(op, self._apply, op)
        rec["op"] = op
        self.record.append(rec)
        self.done_ops.append(op)
        if self.env is not None:
            self._guard(op, bars.check_state, self.env, self.orc)
        return rec

    def run(self, script):
        for op in script:
            self.apply(op)
        return self.record

    def _apply(self, op):
        kind = op[0]
        rng = self._rng()
        return getattr(self, "_op_" + kind)(rng, *op[1:])

    def _op_step(self, rng, mode):
        env, orc = self.env, self.orc
        if mode == "fresh":
            a = self._fresh_actions(rng)
        else:
            if self.prev_actions is None:
                raise IllegalScript("operation %d %r: no step to repeat" % (len(self.done_ops), ("step", mode)))
            a = self.prev_actions
        if mode == "held":
            ok, why = held_is_legal(self.prev_actions, self.la_touched, a)
            if not ok:
                raise IllegalScript("operation %d ('step', 'held') after %r: %s" % (len(self.done_ops), self.done_ops[-3:], why))
        rec = {"t0_envs": int((orc.timesteps == 0).sum()), "wide_active": self._wide_active()}
        orc.step(a)
        if env is not None:
            env.step(a, held=mode == "held")
            bars.check_step(self._step_outputs(), orc, self.case.normalize, self.half, mode)
        self.prev_actions, self.la_touched = a, False
        rec["done"] = int(orc.done.sum())
        return rec

    def _op_skip(self, rng, K):
        env, orc = self.env, self.orc
        a = self._fresh_actions(rng)
        rec = {"wide_active": self._wide_active()}
        ref = skip_ref.skip_reference(orc, a, K)
        if env is not None:
            obs, rew, done, info = env.step_skip(a, K)
            got = self._step_outputs()
            got["n_steps"] = self._cpu(info["frame_steps"])
            bars.check_skip_outputs(got, ref, self.half, True, ("skip", K))
        self.prev_actions, self.la_touched = a, False
        n = ref["n_steps"].astype(int)
        rec.update(early=int((n < K).sum()), ran_all=int((n == K).sum()), done=int(ref["done"].sum()))
        return rec

    def _op_rollout(self, rng, T, hold, full):
        env, orc, c = self.env, self.orc, self.case
        assert T % hold == 0
        a = self._fresh_actions(rng, blocks=T // hold)
        rec = {"wide_active": self._wide_active()}
        out = None
        if env is not None:
            torch = env.torch
            bufs = None if not full else {k: torch.zeros((T,) + shape, dtype=dt, device=env.device) for k, shape, dt in (
                ("obs", (c.B, c.N * 10), torch.float32), ("reward", (c.B,), torch.float32), ("done", (c.B,), torch.uint8),
                ("flags", (c.B, c.N), torch.int16), ("raw_obs", (c.B, c.N * 10), torch.float32), ("ac_reward", (c.B, c.N), torch.float32),
                ("min_sep", (c.B,), torch.float32), ("term_obs", (c.B, c.N * 10), torch.float32))}
            out = {k: self._cpu(v) for k, v in env.rollout(torch.as_tensor(a), out=bufs, hold=hold).items()}
        dones = 0
        term_before = orc.term_obs.copy()   # (a rollout's terminal observations go to its own [T, ...] buffers, not to the env's)
        for t in range(T):
            orc.step(a[t // hold])
            dones += int(orc.done.sum())
            if out is not None:
                got = {"flags": out["flags"][t], "done": out["done"][t], "obs": out["obs"][t].reshape(c.B, c.N, 10), "reward": out["reward"][t]}
                if full:
                    got.update(raw_obs=out["raw_obs"][t].reshape(c.B, c.N, 10), ac_reward=out["ac_reward"][t], min_sep=out["min_sep"][t],
                               term_obs=out["term_obs"][t].reshape(c.B, c.N, 10))
                bars.check_step(got, orc, c.normalize, self.half, ("rollout step", t))
        orc.term_obs[...] = term_before
        self.prev_actions, self.la_touched = a[-1], False
        rec["done"] = dones
        return rec

    def _masked(self, rng, kind, oracle_call, device_call, exact_words=()):
        m = self._mask(kind, rng)
        sel = np.ones(self.case.B, bool) if m is None else m.astype(bool)
        self.orc.obs[...] = SENTINEL
        oracle_call(m)
        if self.env is not None:
            self.env.obs.fill_(float(SENTINEL))
            device_call(m)
            self._check_reset_obs(sel, exact_words)
            if self.env.traffic_k:       # reset() and observe() launch the traffic observation of the state they leave
                self._check_traffic()
        return sel

    def _op_reset(self, rng, kind):
        o, N = self.orc, self.case.N
        full = np.uint64(2 ** N - 1)
        before_mask, before_ep = o.active_mask.copy(), o.episodes.copy()
        sel = self._masked(rng, kind, lambda m: o.reset(mask=m), lambda m: self.env.reset(mask=m))
        return {"selected": int(sel.sum()), "of": self.case.B, "handed_over_selected": int((before_mask[sel] != full).sum()),
                "hi_bit_clear_selected": int(((before_mask[sel] >> np.uint64(32)) != (full >> np.uint64(32))).sum()) if N > 32 else 0,
                "max_episode_selected": int(before_ep[sel].max()) if sel.any() else 0}

    def _op_observe(self, rng, kind):
        o, c = self.orc, self.case
        act = traffic_ref.active_bits(o.active_mask, c.N)
        lo, hi = -2 ** 31, 2 ** 31 - 1
        sel = self._masked(rng, kind, lambda m: o.observe(mask=m), lambda m: self.env.observe(mask=m), exact_words=(3, 9))
        per_env = lambda flat: flat.reshape(c.B, c.N)[sel]   # noqa: E731
        return {"selected": int(sel.sum()), "wide": int(per_env(np.isin(o.phi_fix, I32_EDGE)).sum()), "handed_over": int((~act[sel]).sum()),
                "off_grid": int(per_env(np.isin(o.px, (lo, hi)) | np.isin(o.py, (lo, hi))).sum())}

    def _op_traffic(self, rng):
        if self.case.N == 1:         # one-aircraft envs are made without the traffic observation (nothing to see)
            return {"short": 0}
        if self.env is not None:
            self.env.observe_traffic()
        ref = self._check_traffic()
        act = traffic_ref.active_bits(self.orc.active_mask, self.case.N)
        return {"short": int(((ref["ncand"] < TRAFFIC_K) & act).sum())}

    def _op_set_state(self, rng):
        """six aircraft in six envs: two at a heading of several hundred turns (WIDE), two beyond the position grid (pinned at its
        limit), two on the winning state (the next fresh actions fly them into the corridor: handed over).  Speeds inside the
        device format's 44 .. 356 kt."""
        c = self.case
        envs = [int(e) for e in rng.choice(c.B, 6, replace=False)]
        g_lo, g_hi = H.grid_range(self.comp)
        placed = []
        for j, e in enumerate(envs):
            k = c.N - 1 if j % 3 == 2 else int(rng.integers(0, c.N))
            if j % 3 == 0:
                turns = int(rng.integers(200, 900)) * (1 if j == 0 else -1)
                st = (float(rng.uniform(15, 60)), float(rng.uniform(20, 70)), float(rng.uniform(6000, 30000)),
                      360.0 * turns + float(rng.integers(0, 360 * 8)) / 8.0, float(rng.integers(150, 300)))
            elif j % 3 == 1:
                st = (float(g_hi[0] + 10.0) if j == 1 else float(rng.uniform(15, 60)), float(rng.uniform(20, 70)) if j == 1 else float(g_lo[1] - 10.0),
                      float(rng.uniform(6000, 30000)), float(rng.integers(0, 360)), float(rng.integers(150, 300)))
            else:
                st = H.WIN_STATE
                self.win_pending.append((e, k))
            self.orc.set_state(e, k, *st)
            if self.env is not None:
                self.env.set_state(e, k, *st)
            placed.append((e, k))
        self.placed = envs
        return {"placed": placed}

    def _op_set_last_action(self, rng):
        c = self.case
        for _ in range(4):
            e, k = int(rng.integers(0, c.B)), int(rng.integers(0, c.N))
            val = [float(rng.integers(100, 300)), float(rng.integers(0, 380)) * 100.0,
                   float(rng.integers(0, 360)) + (360.0 * 700 if rng.uniform() < 0.5 else 0.0)]     # some heading targets WIDE
            self.orc.set_last_action(e, k, val)
            if self.env is not None:
                self.env.set_last_action(e, k, val)
        self.la_touched = True
        return {}

    def close(self):
        if self.env is not None:
            self.env.close()


# ---------------------------------------------------------------------------------------------------------------- scripts
# The fixed opening of every script: whatever the seed draws afterwards, these interactions are in it.
PREAMBLE = (
    ("step", "fresh"), ("step", "held"), ("observe", "none"), ("step", "held"),          # observe between two held steps
    ("rollout", 8, 4, False), ("step", "held"),                                          # a held step after rollout(hold=4), the fast form
    ("reset", "random"), ("step", "held"), ("step", "held"),                             # ... after a masked reset of some envs
    # (envs reset three steps ago run all 20 under a time limit of 22 or more, the others meet it inside the block and wait)
    ("skip", 20), ("step", "held"), ("traffic",),                                        # ... right after step_skip
    ("skip", 5), ("step", "held"),
    ("reset", "none"), ("set_state",), ("observe", "random"), ("step", "fresh"),         # placed aircraft: WIDE, off the grid, a hand-over
    ("set_state",), ("observe", "none"), ("traffic",), ("reset", "placed"),              # observe all three kinds; reset handed-over envs
    ("set_state",), ("rollout", 8, 1, True), ("step", "held"),                           # a rollout after set_state to a WIDE heading
    ("set_state",), ("skip", 20), ("step", "held"), ("observe", "zero"),                 # ... and a skip; an all-zero observe mask
    ("reset", "zero"), ("reset", "one"), ("step", "held"),
    ("set_last_action",), ("step", "repeat"), ("step", "held"),                          # a record written from outside: repeat in full
    ("rollout", 4, 4, True), ("skip", 2), ("skip", 1), ("step", "held"), ("reset", "random"), ("traffic",),
)
LENGTH = 60


def make_script(case):
    """PREAMBLE + operations drawn from the case's seed, LENGTH in all; a drawn held step is only drawn where it is legal."""
    rng = np.random.default_rng([case.seed, 1 << 20])
    script = list(PREAMBLE)
    stepped, la_touched = True, False       # (the preamble ends with a stepping operation behind it and no record written since)
    while len(script) < LENGTH:
        r = rng.uniform()
        if r < 0.28:
            mode = ("fresh", "repeat", "held")[int(rng.integers(0, 3))]
            if mode == "held" and (la_touched or not stepped):
                mode = "repeat"
            op = ("step", mode)
        elif r < 0.42:
            op = ("skip", SKIP_KS[int(rng.integers(0, 4))])
        elif r < 0.56:
            hold = (1, 4)[int(rng.integers(0, 2))]
            op = ("rollout", hold * int(rng.integers(1, 4)), hold, bool(rng.integers(0, 2)))
        elif r < 0.68:
            op = ("reset", MASK_KINDS[int(rng.integers(0, 4))])
        elif r < 0.80:
            op = ("observe", MASK_KINDS[int(rng.integers(0, 4))])
        elif r < 0.87:
            op = ("traffic",)
        elif r < 0.95:
            op = ("set_state",)
        else:
            op = ("set_last_action",)
        if op[0] in ("step", "skip", "rollout"):
            la_touched = False
        if op[0] == "set_last_action":
            la_touched = True
        script.append(op)
    return script
