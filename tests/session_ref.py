"""A call-sequence driver: AtcVecEnvs next to fp32 oracle envs of the same size, a scripted list of operations applied to both.
TEST INFRASTRUCTURE ONLY (in the style of tests/skip_ref.py).

The step kernels carry shortcuts that are only correct given what the PREVIOUS call left behind (include/atc_step.h: the last-action
record skipped under ATC_M_ACTIONS_HELD and inside held blocks, envs with timesteps == 0 handled in full, an env that ended early
inside atc_step_skip waiting in its spawn state, the WIDE side records).  The per-entry-point tests run each entry point in a loop of
its own; a Session interleaves them.  Every operation is applied to the oracle and — unless the session was made with device=False,
which is how the CPU tests look at what a script contains — to the device env, and then EVERYTHING is compared: the operation's
outputs by the bars of tests/bars.py, the whole persistent state bit for bit, sentinel rows of masked calls.

BATCHES.  A plain session (tree=False) has one batch, `root`: B envs.  A tree session (tree=True) has three: `root` (B envs), `child`
(M B envs: what atc_branch writes) and `beam` (B envs), all byte-equal in sector and atc_params_t (tests/branch_ref.py::child_of).
Each batch owns an AtcVecEnv, an fp32 OracleEnv of the same size and parameters, and the bookkeeping of the held promise PER ENV
(prev_actions [B, N, 3], has_prev [B], la_touched [B]): branch and select move envs between batches and their previous step goes
with them.

OPERATION TABLE — any new entry point or state-dependent shortcut of the library belongs here.  The stepping, resetting and observing
operations take an optional batch name as their last element (default: root):
    ("step", "fresh" | "repeat" | "held")   env.step                    orc.step          repeat / held reuse the envs' previous actions
    ("step", "tame")                        env.step                    orc.step          fresh actions, every heading inside the action space
    ("step", "branch")                      env.step(held=True)         orc.step          the last branch's actions[m] for child m B + e
    ("skip", K)                             env.step_skip               skip_ref.skip_reference
    ("rollout", T, hold, full)              env.rollout (out buffers iff full)            T x orc.step
    ("reset", mask kind)                    env.reset                   orc.reset         kinds: MASK_KINDS
    ("observe", mask kind)                  env.observe                 orc.observe       into sentinel-filled observation arrays
    ("traffic",)                            env.observe_traffic         traffic_ref.traffic_reference on the ORACLE's state
    ("set_state",)                          env.set_state               orc.set_state     six aircraft: two at a WIDE heading, two beyond
                                                                                          the position grid, two on a winning state
    ("set_last_action",)                    env.set_last_action         orc.set_last_action
The scoring calls run on root or beam (optional batch name last) and must change NOTHING: the six state arrays and every bound output
tensor of the env are byte-equal to a snapshot taken before, the held bookkeeping is what it was:
    ("lookahead", K, "fast" | "all")        env.lookahead               skip_ref.candidate_references, on the oracle from a snapshot
    ("plan", K, H, "fast" | "all")          env.lookahead_plan          skip_ref.plan_references
    ("plan_sampled", K, H, mean_first)      env.lookahead_plan_sampled  plan_draw_ref.draw, then skip_ref.plan_references; bit for bit
                                                                        env.lookahead_plan on env.draw_plans(...)
    ("plan_iter", mode, M, H)               one iteration of a scored planner by the public calls: env.lookahead_plan_sampled -> score_plans
                                            -> refit_plans -> draw_plans(index=top[:1]); tests/planner_ref.py::check_iteration against the
                                            oracle's flight of the numpy-drawn plans.  mode: "elite" | "softmax"; K, the scoring arguments,
                                            the seed and the iteration follow from the operation's index.  The batch keeps the decision:
    ("step", "decision")                    the last plan_iter's decision of this batch flown for its K steps: one fresh step with the
                                            device's own decision tensor (the numpy row of the same candidate on the oracle, zeros where the
                                            env has no valid candidate), then K - 1 held steps
The state-moving calls:
    ("branch", src, K)                      src.branch(cand, K, into=child)   branch_ref.oracle_branch: every candidate flown on the SOURCE
                                            oracle from a snapshot (resets inside the call keyed by e), its rows copied into rows m B + e of
                                            the child oracle (later resets keyed by c = m B + e); not-evaluated (WIDE) env-candidates get the
                                            source's rows and zero outputs
    ("select", dst, src, kind)              dst.select(src, index, mask)      row gather between the two oracles; kinds: SELECT_KINDS
    ("replay", first, count)                operations first .. first + count - 1 of the script again, with the inputs they had: every
                                            output and the state after each is byte-equal to the first pass (after a stash / restore)
Candidates come from held_tools.look_draw: headings inside the action space, so no candidate makes a heading WIDE and the
env-candidates that are not evaluated are exactly those of envs the ORACLE shows WIDE when the call starts.
Everything an operation needs beyond its tuple (actions, masks, aircraft) is drawn from a generator seeded by (case seed, index of the
operation), so a script means the same inputs on the oracle alone and next to the device.

held=True is a promise (ATC_M_ACTIONS_HELD): `held_is_legal` is the ONE statement of when a script may make it, per env, and every
scripted held step is checked against it before anything runs.  The previous step of a child env is the branch's step with actions[m];
of a not-evaluated child, its source env's previous step; of a gathered env, that of the env it was gathered from."""
import collections
import hashlib

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
BATCHES = ("root", "child", "beam")
SELECT_KINDS = ("commit", "beam", "stash", "restore", "edge", "zero")
SCORE_M = 3                # candidates of ("lookahead", ...) and ("plan", ...)
TREE_WILD_ENVS = 0.2       # tree sessions: the share of ENVS whose heading components take part in the wild draws (see Session)
BOUND = ("obs", "raw_obs", "reward", "done", "flags", "ac_reward", "min_sep", "term_obs", "traffic", "frame_steps")
BATCH_OPS = ("step", "skip", "rollout", "reset", "observe", "traffic", "set_state", "set_last_action", "lookahead", "plan", "plan_sampled",
             "plan_iter")
ITER_KS = (2, 4, 5)        # K of ("plan_iter", ...), by the operation's index

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


def held_is_legal(prev_actions, la_touched, actions, has_prev=None):
    """include/atc_step.h, ATC_M_ACTIONS_HELD: `actions` holds, for every aircraft, the same BITS as the previous step of these envs —
    the last step of whichever stepping call came before (atc_step, the last block of a rollout, the block of a frame skip; for a child
    env the branch's step, for a not-evaluated child and for a gathered env the previous step of the env its rows came from) —, and
    nobody wrote a last-action record since.  Resets, observations and placed aircraft in between are allowed: envs reset since
    their last step are handled in full.  Per env: prev_actions [B, N, 3] (None: no env has a previous step), la_touched a bool or
    [B], has_prev [B] (None: every env has one).  Returns (legal, why not)."""
    if prev_actions is None:
        return False, "no step before it"
    act = np.asarray(actions, np.float32)
    B = act.shape[0]
    if has_prev is not None and not np.all(has_prev):
        return False, "no step before it (env %d)" % int(np.argmin(has_prev))
    la = np.broadcast_to(np.asarray(la_touched, bool), (B,))
    if la.any():
        return False, "set_last_action since the previous step (env %d)" % int(np.argmax(la))
    same = (np.asarray(prev_actions, np.float32).view(np.int32).reshape(B, -1) == act.view(np.int32).reshape(B, -1)).all(1)
    if not same.all():
        return False, "the actions differ from the previous step's (env %d)" % int(np.argmin(same))
    return True, ""


def draw_actions(rng, B, N):
    """a third of the components outside the action space (tests/held_tools.py::skip_actions)"""
    return fuzz_space.draw_actions(rng, (B, N), False, 0.33, True)


class Batch:
    """one named batch: the env, the oracle and what the session knows about the envs' previous step"""

    def __init__(self, name, B, N, env, orc):
        self.name, self.B, self.env, self.orc = name, B, env, orc
        self.prev_actions = np.zeros((B, N, 3), np.float32)   # action bits of each env's previous step (where has_prev)
        self.has_prev = np.zeros(B, bool)
        self.la_touched = np.zeros(B, bool)                   # set_last_action on the env since then
        self.placed = []              # envs the last set_state touched
        self.win_pending = []         # (env, slot) placed on the winning state: the next fresh actions fly them into the corridor
        self.branch_actions = None    # [B, N, 3]: the candidates of the last branch into this batch, child by child
        self.hi_from = B + 1          # child: root's B (envs c >= B: their reset key is not a source env's)
        self.decision = None          # (numpy [B, N, 3], the device's tensor or None, K) of the last plan_iter on this batch

    def stepped(self, a):
        self.prev_actions = np.ascontiguousarray(np.asarray(a, np.float32).reshape(self.prev_actions.shape)).copy()
        self.has_prev[...] = True
        self.la_touched[...] = False


class Session:
    def __init__(self, case, device=True, tree=False, M=3):
        """tree=True: the three batches, M children per env.  A tree session draws its fresh actions with the heading component wild
        in a TREE_WILD_ENVS share of the ENVS (drawn per operation) instead of in every env: a wild heading target is WIDE, a WIDE env is
        not evaluated by the scoring and branch calls, and with a third of all heading components wild no env of 8 or more aircraft would
        ever be evaluated (tests/test_tree_sequences.py states the shares the oracle shows).  A plain session draws as it always did."""
        from oracle import oracle as O
        self.case, self.tree, self.M = case, bool(tree), int(M)
        self.scn, self.comp = setup(case.N)
        c = case
        self.half = bars.half_range(self.comp)
        self.done_ops = []            # the script so far
        self.record = []              # what the ORACLE saw, one dict per operation (tests look for the interactions in it)
        self.digests = []             # per operation: (digest of the device's outputs and state, of the oracle's state)

        def make_orc(B):
            return O.OracleEnv(self.comp, B, c.N, O.make_params(
                dt=c.dt, normalize=c.normalize, auto_reset=c.auto_reset, random_entry=c.spawn == "random", seed=c.seed,
                timestep_limit=c.timestep_limit, sep_nm=c.sep_nm, keep_active=c.keep_active), np.float32)

        def make_env(B):
            from atc_hip.vec_env import AtcVecEnv
            from envs.atc import model
            return AtcVecEnv(B, c.N, sim_parameters=model.SimParameters(c.dt, normalize_state=c.normalize), scenario=self.scn,
                             auto_reset=c.auto_reset, spawn=c.spawn, seed=c.seed, grid_cell=0.5, want_raw_obs=True, want_ac_reward=True,
                             want_min_sep=True, want_term_obs=True, timestep_limit=c.timestep_limit, sep_nm=c.sep_nm,
                             keep_active=c.keep_active, traffic=TRAFFIC_K if c.N > 1 else 0)

        sizes = {"root": c.B, "child": self.M * c.B, "beam": c.B} if self.tree else {"root": c.B}
        self.b = {}
        for name, B in sizes.items():
            env = None
            if device:
                if name == "root":
                    env = make_env(B)
                else:
                    import branch_ref
                    env = branch_ref.child_of(self.b["root"].env, B // c.B, lambda n: make_env(n))
            self.b[name] = Batch(name, B, c.N, env, make_orc(B))
        if self.tree:
            self.b["child"].hi_from = c.B
        for bt in self.b.values():
            if bt.env is not None:
                self._guard("the constructor's reset", self._check_reset_obs, bt, np.ones(bt.B, bool))
                self._guard("the constructor's reset", bars.check_state, bt.env, bt.orc)

    # the root batch under the names a one-batch session always had
    env = property(lambda self: self.b["root"].env)
    orc = property(lambda self: self.b["root"].orc)

    @property
    def prev_actions(self):
        r = self.b["root"]
        return r.prev_actions if r.has_prev.all() else None

    @property
    def la_touched(self):
        return bool(self.b["root"].la_touched.any())

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

    def _dev(self, bt, a):
        return bt.env.torch.as_tensor(np.ascontiguousarray(a), device=bt.env.device)

    def _mask(self, bt, kind, rng):
        B = bt.B
        if kind == "none":
            return None
        if kind == "zero":
            return np.zeros(B, np.uint8)
        if kind == "one":
            return np.ones(B, np.uint8)
        if kind == "placed":
            m = np.zeros(B, np.uint8)
            m[bt.placed] = 7          # any non-zero byte selects
            return m
        assert kind == "random", kind
        return (rng.uniform(size=B) < 0.4).astype(np.uint8)

    def _wide_active(self, bt):
        """aircraft at a WIDE heading and under control, on the oracle"""
        o = bt.orc
        act = traffic_ref.active_bits(o.active_mask, o.N).reshape(-1)
        return int((np.isin(o.phi_fix, I32_EDGE) & act).sum())

    def _fresh_actions(self, rng, bt, blocks=None, tame=False):
        B, N = bt.B, self.case.N
        if self.tree:
            where = np.zeros(B, bool) if tame else rng.uniform(size=B) < TREE_WILD_ENVS
            one = lambda: fuzz_space.draw_actions(rng, (B, N), False, 0.33, where)   # noqa: E731
        else:
            one = lambda: draw_actions(rng, B, N)   # noqa: E731
        a = one() if blocks is None else np.stack([one() for _ in range(blocks)])
        for e, k in bt.win_pending:
            a[..., e, k, :] = H.WIN_ACTION
        bt.win_pending = []
        return a

    def _step_outputs(self, bt):
        env, B, N = bt.env, bt.B, self.case.N
        return {"flags": self._cpu(env.flags), "done": self._cpu(env.done), "obs": self._cpu(env.obs).reshape(B, N, 10),
                "reward": self._cpu(env.reward), "raw_obs": self._cpu(env.raw_obs).reshape(B, N, 10), "ac_reward": self._cpu(env.ac_reward),
                "min_sep": self._cpu(env.min_sep), "term_obs": self._cpu(env.term_obs).reshape(B, N, 10)}

    @staticmethod
    def _written(got):
        """the words of a stepping call's outputs that the call writes, for the replay digest: the terminal observation is written for
        envs that ended only"""
        out = dict(got)
        dn = out["done"].astype(bool)
        out["term_obs"] = np.where(dn.reshape(dn.shape + (1,) * (out["term_obs"].ndim - dn.ndim)), out["term_obs"], 0)
        return [np.ascontiguousarray(out[k]) for k in sorted(out)]

    def _check_reset_obs(self, bt, m, exact_words=()):
        """rows of selected envs against the oracle's (raw observations: the bar of an auto-reset row of a step); the others still
        hold the sentinel"""
        got = self._cpu(bt.env.obs).reshape(bt.B, self.case.N, 10)
        ref = bt.orc.obs
        assert np.all(got[~m] == SENTINEL) and np.all(ref[~m] == SENTINEL), "an unselected env's observation row was written"
        assert np.all(np.abs(got[m] - ref[m]) <= 1e-5 * bars.obs_scale(ref[m], self.case.normalize, self.half)), "obs"
        for w in exact_words:
            assert np.array_equal(got[m][..., w], ref[m][..., w]), "raw word %d" % w

    def _check_traffic(self, bt):
        o, c = bt.orc, self.case
        st = dict(x_fix=o.px.reshape(bt.B, c.N), y_fix=o.py.reshape(bt.B, c.N), h=o.h.reshape(bt.B, c.N),
                  P=o.phi_counts.astype(np.float64).reshape(bt.B, c.N), v_fix=o.v_fix.view(np.uint32).reshape(bt.B, c.N), mask=o.active_mask)
        ref = traffic_ref.traffic_reference(st, self.comp.pos_origin, self.comp.pos_k)
        if bt.env is not None:
            bad = traffic_ref.compare(self._cpu(bt.env.traffic), ref, TRAFFIC_K, traffic_ref.norm_scales(self.comp) if c.normalize else None)
            assert not bad, ("traffic", bt.name, bad)
        return ref

    def _untouched(self, bt):
        """Snapshots everything a read-only call must leave alone in batch bt — the six state arrays, every bound output tensor, the
        oracle's arrays, the held bookkeeping — and returns the function that asserts it is all still there, byte for byte."""
        env, orc = bt.env, bt.orc
        held = (bt.prev_actions.copy(), bt.has_prev.copy(), bt.la_touched.copy())
        osnap = skip_ref.snapshot(orc)
        if env is not None:
            torch = env.torch
            snap = H.snapshot(env)
            outs = {k: getattr(env, k).clone() for k in BOUND if getattr(env, k, None) is not None}

        def verify():
            for part in osnap:
                for k, v in part.items():
                    assert np.array_equal(getattr(orc, k), v), ("the reference changed the oracle", bt.name, k)
            assert np.array_equal(held[0].view(np.int32), bt.prev_actions.view(np.int32)) and np.array_equal(held[1], bt.has_prev) \
                and np.array_equal(held[2], bt.la_touched), "held bookkeeping"
            if env is not None:
                H.bytes_equal(env, snap)
                for k, v in outs.items():
                    assert torch.equal(getattr(env, k).contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), \
                        "bound output %s of %s changed" % (k, bt.name)
        return verify

    def _digest(self, names, out):
        """(device, oracle): sha256 over what the operation returned and over the state of the batches it touched"""
        ho = hashlib.sha256()
        for n in names:
            for k in skip_ref.STATE:
                ho.update(np.ascontiguousarray(getattr(self.b[n].orc, k)).tobytes())
        hd = None
        if self.b["root"].env is not None:
            hd = hashlib.sha256()
            for a in out:
                hd.update(np.ascontiguousarray(a).tobytes())
            for n in names:      # (a phi_wide word is specified only next to a saturated 32-bit field)
                st = {k: self._cpu(getattr(self.b[n].env, k)) for k in H.STATE}
                sat = np.stack([np.isin(st["ac"][:, 2], I32_EDGE), np.isin(st["last_act"][:, 1], I32_EDGE)], axis=1)
                st["phi_wide"] = np.where(sat, st["phi_wide"][:, :2], 0.0)
                for k in H.STATE:
                    hd.update(np.ascontiguousarray(st[k]).tobytes())
            hd = hd.hexdigest()
        return hd, ho.hexdigest()

    # -------------------------------------------------------------------------------------------------------- operations
    def apply(self, op):
        rec = self._guard(op, self._run_one, op, len(self.done_ops))
        rec["op"] = op
        self.record.append(rec)
        self.done_ops.append(op)
        return rec

    def run(self, script):
        for op in script:
            self.apply(op)
        return self.record

    def _split(self, op):
        """(kind, arguments, the batch an operation with an optional batch name runs on)"""
        kind, args = op[0], op[1:]
        if kind in BATCH_OPS and args and isinstance(args[-1], str) and args[-1] in BATCHES:
            return kind, args[:-1], args[-1]
        return kind, args, "root"

    def _batch(self, name):
        if name not in self.b:
            raise IllegalScript("operation %d: this session has no batch %r (tree=True makes them)" % (len(self.done_ops), name))
        return self.b[name]

    def _run_one(self, op, index):
        """one operation with the inputs of script position `index`; state check of every batch it may touch; its digests"""
        kind, args, name = self._split(op)
        rng = np.random.default_rng([self.case.seed, index])
        self._index = index
        if kind in BATCH_OPS:
            rec = getattr(self, "_op_" + kind)(rng, self._batch(name), *args)
            names = [name]
        else:
            rec, names = getattr(self, "_op_" + kind)(rng, *args)
        for n in names:
            if self.b[n].env is not None:
                bars.check_state(self.b[n].env, self.b[n].orc)
        d = self._digest(names, rec.pop("_out", []))
        if index == len(self.digests):
            self.digests.append(d)
        rec["_digest"] = d
        return rec

    def _ended(self, rec, bt, ep_before, ended):
        """for the "keyed by c" clause: the highest episode number at which an env c >= B of the child batch ended (and, with
        auto_reset, was reset inside the call)"""
        hi = ended.astype(bool) & (np.arange(bt.B) >= bt.hi_from)
        rec["hi_reset_episode"] = max(rec.get("hi_reset_episode", 0), int(ep_before[hi].max()) if hi.any() and self.case.auto_reset else 0)

    def _op_step(self, rng, bt, mode):
        env, orc = bt.env, bt.orc
        here = "operation %d %r" % (len(self.done_ops), ("step", mode, bt.name))
        if mode in ("fresh", "tame"):
            a = self._fresh_actions(rng, bt, tame=mode == "tame")
        elif mode == "branch":
            if bt.branch_actions is None:
                raise IllegalScript("%s: no branch into this batch" % here)
            a = bt.branch_actions
        elif mode == "decision":
            if bt.decision is None:
                raise IllegalScript("%s: no plan_iter on this batch" % here)
            return self._fly_decision(bt)
        else:
            if not bt.has_prev.all():
                raise IllegalScript("%s: no step to repeat" % here)
            a = bt.prev_actions
        held = mode in ("held", "branch")
        if held:
            ok, why = held_is_legal(bt.prev_actions if bt.has_prev.any() else None, bt.la_touched, a, bt.has_prev)
            if not ok:
                raise IllegalScript("%s after %r: %s" % (here, self.done_ops[-3:], why))
        rec = {"t0_envs": int((orc.timesteps == 0).sum()), "wide_active": self._wide_active(bt), "wide_envs": int(skip_ref.wide_envs(orc).sum()),
               "batch": bt.name}
        ep = orc.episodes.copy()
        orc.step(a)
        if env is not None:
            env.step(a, held=held)
            got = self._step_outputs(bt)
            bars.check_step(got, orc, self.case.normalize, self.half, mode)
            rec["_out"] = self._written(got) + ([self._cpu(env.traffic)] if env.traffic_k else [])
        bt.stepped(a)
        rec["done"] = int(orc.done.sum())
        self._ended(rec, bt, ep, orc.done)
        return rec

    def _fly_decision(self, bt):
        """("step", "decision"): K steps with the last plan_iter's decision, the first in full, the others held; every step compared"""
        env, orc = bt.env, bt.orc
        a, dev, K = bt.decision
        rec = {"t0_envs": int((orc.timesteps == 0).sum()), "wide_active": self._wide_active(bt), "wide_envs": int(skip_ref.wide_envs(orc).sum()),
               "batch": bt.name, "K": K, "held_steps": K - 1, "nonzero_rows": int(a.reshape(bt.B, -1).any(1).sum()), "done": 0, "_out": []}
        for j in range(K):
            if j > 0:       # the held promise, by the one rule every scripted held step goes through
                ok, why = held_is_legal(bt.prev_actions, bt.la_touched, a, bt.has_prev)
                if not ok:
                    raise IllegalScript("operation %d: held step %d of a decision: %s" % (len(self.done_ops), j, why))
            ep = orc.episodes.copy()
            orc.step(a)
            if env is not None:
                env.step(dev, held=j > 0)
                got = self._step_outputs(bt)
                bars.check_step(got, orc, self.case.normalize, self.half, ("decision", j))
                bars.check_state(env, orc)
                rec["_out"] += self._written(got) + ([self._cpu(env.traffic)] if env.traffic_k else [])
            bt.stepped(a)
            rec["done"] += int(orc.done.sum())
            self._ended(rec, bt, ep, orc.done)
        return rec

    def _op_skip(self, rng, bt, K):
        env, orc = bt.env, bt.orc
        a = self._fresh_actions(rng, bt)
        rec = {"wide_active": self._wide_active(bt), "wide_envs": int(skip_ref.wide_envs(orc).sum()), "batch": bt.name}
        ep = orc.episodes.copy()
        ref = skip_ref.skip_reference(orc, a, K)
        if env is not None:
            obs, rew, done, info = env.step_skip(a, K)
            got = self._step_outputs(bt)
            got["n_steps"] = self._cpu(info["frame_steps"])
            bars.check_skip_outputs(got, ref, self.half, True, ("skip", K))
            rec["_out"] = self._written(got) + ([self._cpu(env.traffic)] if env.traffic_k else [])
        bt.stepped(a)
        n = ref["n_steps"].astype(int)
        rec.update(early=int((n < K).sum()), ran_all=int((n == K).sum()), done=int(ref["done"].sum()))
        self._ended(rec, bt, ep, ref["done"])
        return rec

    def _op_rollout(self, rng, bt, T, hold, full):
        env, orc, c = bt.env, bt.orc, self.case
        B = bt.B
        assert T % hold == 0
        a = self._fresh_actions(rng, bt, blocks=T // hold)
        rec = {"wide_active": self._wide_active(bt), "wide_envs": int(skip_ref.wide_envs(orc).sum()), "batch": bt.name}
        out = None
        if env is not None:
            torch = env.torch
            bufs = None if not full else {k: torch.zeros((T,) + shape, dtype=dt, device=env.device) for k, shape, dt in (
                ("obs", (B, c.N * 10), torch.float32), ("reward", (B,), torch.float32), ("done", (B,), torch.uint8),
                ("flags", (B, c.N), torch.int16), ("raw_obs", (B, c.N * 10), torch.float32), ("ac_reward", (B, c.N), torch.float32),
                ("min_sep", (B,), torch.float32), ("term_obs", (B, c.N * 10), torch.float32))}
            out = {k: self._cpu(v) for k, v in env.rollout(torch.as_tensor(a), out=bufs, hold=hold).items()}
            rec["_out"] = [out[k] for k in sorted(out) if k != "term_obs"]
        dones = 0
        term_before = orc.term_obs.copy()   # (a rollout's terminal observations go to its own [T, ...] buffers, not to the env's)
        for t in range(T):
            ep = orc.episodes.copy()
            orc.step(a[t // hold])
            dones += int(orc.done.sum())
            self._ended(rec, bt, ep, orc.done)
            if out is not None:
                got = {"flags": out["flags"][t], "done": out["done"][t], "obs": out["obs"][t].reshape(B, c.N, 10), "reward": out["reward"][t]}
                if full:
                    got.update(raw_obs=out["raw_obs"][t].reshape(B, c.N, 10), ac_reward=out["ac_reward"][t], min_sep=out["min_sep"][t],
                               term_obs=out["term_obs"][t].reshape(B, c.N, 10))
                bars.check_step(got, orc, c.normalize, self.half, ("rollout step", t))
        orc.term_obs[...] = term_before
        bt.stepped(a[-1])
        rec["done"] = dones
        return rec

    def _masked(self, rng, bt, kind, oracle_call, device_call, rec, exact_words=()):
        m = self._mask(bt, kind, rng)
        sel = np.ones(bt.B, bool) if m is None else m.astype(bool)
        bt.orc.obs[...] = SENTINEL
        oracle_call(m)
        if bt.env is not None:
            bt.env.obs.fill_(float(SENTINEL))
            device_call(m)
            self._check_reset_obs(bt, sel, exact_words)
            rec["_out"] = [self._cpu(bt.env.obs)]
            if bt.env.traffic_k:       # reset() and observe() launch the traffic observation of the state they leave
                self._check_traffic(bt)
                rec["_out"].append(self._cpu(bt.env.traffic))
        return sel

    def _op_reset(self, rng, bt, kind):
        o, N = bt.orc, self.case.N
        full = np.uint64(2 ** N - 1)
        before_mask, before_ep = o.active_mask.copy(), o.episodes.copy()
        rec = {"batch": bt.name}
        sel = self._masked(rng, bt, kind, lambda m: o.reset(mask=m), lambda m: bt.env.reset(mask=m), rec)
        rec.update({"selected": int(sel.sum()), "of": bt.B, "handed_over_selected": int((before_mask[sel] != full).sum()),
                    "hi_bit_clear_selected": int(((before_mask[sel] >> np.uint64(32)) != (full >> np.uint64(32))).sum()) if N > 32 else 0,
                    "max_episode_selected": int(before_ep[sel].max()) if sel.any() else 0})
        return rec

    def _op_observe(self, rng, bt, kind):
        o, c = bt.orc, self.case
        act = traffic_ref.active_bits(o.active_mask, c.N)
        lo, hi = -2 ** 31, 2 ** 31 - 1
        rec = {"batch": bt.name, "wide_envs": int(skip_ref.wide_envs(o).sum())}
        sel = self._masked(rng, bt, kind, lambda m: o.observe(mask=m), lambda m: bt.env.observe(mask=m), rec, exact_words=(3, 9))
        per_env = lambda flat: flat.reshape(bt.B, c.N)[sel]   # noqa: E731
        rec.update({"selected": int(sel.sum()), "wide": int(per_env(np.isin(o.phi_fix, I32_EDGE)).sum()), "handed_over": int((~act[sel]).sum()),
                    "off_grid": int(per_env(np.isin(o.px, (lo, hi)) | np.isin(o.py, (lo, hi))).sum())})
        return rec

    def _op_traffic(self, rng, bt):
        if self.case.N == 1:         # one-aircraft envs are made without the traffic observation (nothing to see)
            return {"short": 0, "batch": bt.name, "wide_envs": 0}
        rec = {"batch": bt.name, "wide_envs": int(skip_ref.wide_envs(bt.orc).sum())}
        if bt.env is not None:
            bt.env.observe_traffic()
            rec["_out"] = [self._cpu(bt.env.traffic)]
        ref = self._check_traffic(bt)
        act = traffic_ref.active_bits(bt.orc.active_mask, self.case.N)
        rec["short"] = int(((ref["ncand"] < TRAFFIC_K) & act).sum())
        return rec

    def _op_set_state(self, rng, bt):
        """six aircraft in six envs: two at a heading of several hundred turns (WIDE), two beyond the position grid (pinned at its
        limit), two on the winning state (the next fresh actions fly them into the corridor: handed over).  Speeds inside the
        device format's 44 .. 356 kt."""
        c = self.case
        envs = [int(e) for e in rng.choice(bt.B, 6, replace=False)]
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
                bt.win_pending.append((e, k))
            bt.orc.set_state(e, k, *st)
            if bt.env is not None:
                bt.env.set_state(e, k, *st)
            placed.append((e, k))
        bt.placed = envs
        return {"placed": placed, "batch": bt.name}

    def _op_set_last_action(self, rng, bt):
        c = self.case
        for _ in range(4):
            e, k = int(rng.integers(0, bt.B)), int(rng.integers(0, c.N))
            val = [float(rng.integers(100, 300)), float(rng.integers(0, 380)) * 100.0,
                   float(rng.integers(0, 360)) + (360.0 * 700 if rng.uniform() < 0.5 else 0.0)]     # some heading targets WIDE
            bt.orc.set_last_action(e, k, val)
            if bt.env is not None:
                bt.env.set_last_action(e, k, val)
            bt.la_touched[e] = True
        return {"batch": bt.name}

    # -------------------------------------------------------------------------------------------------------- scoring calls
    def _score(self, bt, refs, ok, K, call, plan, tag):
        """what the three scoring operations share: the device call between two snapshots, its outputs at the bars of tests/bars.py —
        every env the oracle shows evaluated is compared, every other one must return zeros —, the oracle-side record"""
        verify = self._untouched_before
        rec = {"batch": bt.name, "pairs": len(refs) * bt.B, "evaluated": len(refs) * int(ok.sum()), "evaluated_per_candidate": [int(ok.sum())] * len(refs)}
        n = np.stack([r["n_steps"].astype(np.int64) for r in refs])[:, ok]
        done = np.stack([r["done"].astype(bool) for r in refs])[:, ok]
        rec.update(early=int((done & (n < K * plan)).sum()), ran_all=int((n == K * plan).sum()), done=int(done.sum()), t0_envs=int((bt.orc.timesteps == 0).sum()))
        if bt.env is not None:
            got = {k: self._cpu(v) for k, v in call().items()}
            for m, ref in enumerate(refs):
                bars.check_candidate_outputs({k: v[m] for k, v in got.items() if k != "seg_reward"}, ref, ok, self.half, tag=(tag, m))
                if "seg_reward" in got:
                    bars.check_plan_segments(got["seg_reward"][m], ref, ok, K, tag=(tag, m))
            rec["_out"] = [got[k] for k in sorted(got)]
        verify()
        return rec

    def _scoring_batch(self, bt, what):
        if bt.name == "child":
            raise IllegalScript("operation %d: %s runs on root or beam" % (len(self.done_ops), what))
        self._untouched_before = self._untouched(bt)

    def _op_lookahead(self, rng, bt, K, kind):
        import held_tools
        self._scoring_batch(bt, "lookahead")
        cand = held_tools.look_draw(rng, SCORE_M, bt.B, self.case.N)
        ok = ~skip_ref.wide_envs(bt.orc)
        refs = skip_ref.candidate_references(bt.orc, cand, K)
        outputs = () if kind == "fast" else ("flags", "min_sep", "ac_reward", "obs")
        rec = self._score(bt, refs, ok, K, lambda: bt.env.lookahead(self._dev(bt, cand), K, outputs=outputs), 1, ("lookahead", K, kind))
        rec["shape"] = ("lookahead", SCORE_M, 1, outputs)
        return rec

    def _op_plan(self, rng, bt, K, Hn, kind):
        import held_tools
        self._scoring_batch(bt, "plan")
        cand = held_tools.look_draw(rng, SCORE_M, Hn, bt.B, self.case.N)
        ok = ~skip_ref.wide_envs(bt.orc)
        refs = skip_ref.plan_references(bt.orc, cand, K)
        outputs = () if kind == "fast" else ("seg_reward", "flags", "min_sep", "ac_reward", "obs")
        rec = self._score(bt, refs, ok, K, lambda: bt.env.lookahead_plan(self._dev(bt, cand), K, outputs=outputs), Hn, ("plan", K, Hn, kind))
        rec["shape"] = ("plan", SCORE_M, Hn, outputs)
        return rec

    def _op_plan_sampled(self, rng, bt, K, Hn, mean_first):
        """mean and std tensors drawn, a seed and an iteration > 0 from the operation's index, M = 5 or 8; the fast form (no optional
        output) and all outputs alternate with the index"""
        import held_tools
        import plan_draw_ref
        self._scoring_batch(bt, "plan_sampled")
        N, idx = self.case.N, self._index
        M = 8 if idx % 2 else 5
        mean = (held_tools.look_draw(rng, Hn, bt.B, N) * np.float32(0.8)).astype(np.float32)
        std = rng.uniform(0.05, 0.5, (Hn, bt.B, N, 3)).astype(np.float32)
        key = dict(seed=self.case.seed * 1000 + idx, iteration=1 + idx, mean_first=bool(mean_first))
        plans = plan_draw_ref.draw(mean, std, M, **key)
        assert np.all(np.abs(plans[..., 2]) <= 1.0)          # (drawn headings are clamped into the action space: nothing is made WIDE)
        ok = ~skip_ref.wide_envs(bt.orc)
        refs = skip_ref.plan_references(bt.orc, plans, K)
        outputs = () if (idx // 2) % 2 else ("seg_reward", "flags", "min_sep", "ac_reward", "obs")

        def call():
            env, torch = bt.env, bt.env.torch
            mu, sd = self._dev(bt, mean), self._dev(bt, std)
            res = {k: v.clone() for k, v in env.lookahead_plan_sampled(mu, sd, K, M, outputs=outputs, **key).items()}
            drawn = env.draw_plans(mu, sd, M, **key)
            assert np.array_equal(self._cpu(drawn).view(np.int32), plans.view(np.int32)), "draw_plans against tests/plan_draw_ref.py"
            twin = env.lookahead_plan(drawn, K, outputs=outputs)
            assert set(twin) == set(res)
            for k, v in res.items():
                assert torch.equal(v.contiguous().view(torch.uint8), twin[k].contiguous().view(torch.uint8)), \
                    ("lookahead_plan_sampled is not lookahead_plan on draw_plans(...)", k)
            return res
        rec = self._score(bt, refs, ok, K, call, Hn, ("plan_sampled", K, Hn, M))
        rec["shape"] = ("plan_sampled", M, Hn, outputs)
        return rec

    def _op_plan_iter(self, rng, bt, mode, M, Hn):
        """mean and std tensors drawn (std 0.3 .. 1.5 per component), K = ITER_KS[index % 3]; elites, temperature, gamma and top rotate
        with the index.  Without a device the stand-in of tests/planner_ref.py takes the device's place, so that the oracle-only record
        holds a decision too."""
        import held_tools
        import plan_draw_ref
        import planner_ref
        self._scoring_batch(bt, "plan_iter")
        verify = self._untouched_before
        N, idx, B = self.case.N, self._index, bt.B
        K = ITER_KS[idx % 3]
        how = dict(gamma=(1.0, 0.9, 0.0)[(idx // 2) % 3], top=(1, 5)[idx % 2], mode=mode)
        if mode == "elite":
            how["elites"] = (1, min(3, M), M)[idx % 3]
        else:
            how["temperature"] = (0.5, 5.0)[(idx // 3) % 2]
        mean = (held_tools.look_draw(rng, Hn, B, N) * np.float32(0.8)).astype(np.float32)
        std = rng.uniform(0.3, 1.5, (Hn, B, N, 3)).astype(np.float32)
        key = dict(seed=self.case.seed * 1000 + idx, iteration=1 + idx, mean_first=True)
        plans = plan_draw_ref.draw(mean, std, M, **key)
        ok = ~skip_ref.wide_envs(bt.orc)
        refs = skip_ref.plan_references(bt.orc, plans, K)
        n = np.stack([r["n_steps"].astype(np.int64) for r in refs])[:, ok]
        done = np.stack([r["done"].astype(bool) for r in refs])[:, ok]
        rec = {"batch": bt.name, "pairs": M * B, "evaluated": M * int(ok.sum()), "evaluated_per_candidate": [int(ok.sum())] * M, "K": K,
               "early": int((done & (n < K * Hn)).sum()), "ran_all": int((n == K * Hn).sum()), "t0_envs": int((bt.orc.timesteps == 0).sum()),
               "shape": ("plan_iter", M, Hn, mode), "how": how}
        dev = None
        if bt.env is not None:
            env = bt.env
            mu, sd = self._dev(bt, mean), self._dev(bt, std)
            res = env.lookahead_plan_sampled(mu, sd, K, M, outputs=("seg_reward",), **key)
            sc = env.score_plans(res["seg_reward"], res["n_steps"], **how)
            new_mean, new_std = env.refit_plans(mu, sd, M, sc["weight"], **key)
            dev = env.draw_plans(mu, sd, M, index=sc["top"][:1], **key)[0, 0].clone()
            got = {k: self._cpu(v) for k, v in dict(res, **sc).items()}
            got.update(new_mean=self._cpu(new_mean), new_std=self._cpu(new_std), decision=self._cpu(dev))
            for m, r in enumerate(refs):
                bars.check_candidate_outputs({k: got[k][m] for k in ("reward", "done", "n_steps")}, r, ok, self.half, tag=("plan_iter", m))
                bars.check_plan_segments(got["seg_reward"][m], r, ok, K, tag=("plan_iter", m))
            ref = planner_ref.reference(refs, ok, seg32=got["seg_reward"], **how)
            rec["_out"] = [got[k] for k in sorted(got)]
        else:
            ref = planner_ref.reference(refs, ok, **how)
            got = planner_ref.stand_in(refs, ok, plans, mean, std, **how)
        rec["stats"] = planner_ref.check_iteration(got, ref, plans, mean, std, tag=("plan_iter", idx, mode, M, Hn))
        ev, ndw, asked, nde = planner_ref.shares(ref)
        rec.update(evaluated_envs=ev, none_valid=B - ev, non_decisive_winner=ndw, non_decisive_boundary=nde)
        t0 = np.asarray(got["top"])[0].astype(np.int64)
        row = np.where((t0 >= 0)[:, None, None], plans[np.maximum(t0, 0), 0, np.arange(B)], np.float32(0)).astype(np.float32)
        verify()
        bt.decision = (np.ascontiguousarray(row), dev, K)
        return rec

    # -------------------------------------------------------------------------------------------------------- state-moving calls
    def _op_branch(self, rng, src, K):
        import branch_ref
        import held_tools
        if src not in ("root", "beam"):
            raise IllegalScript("operation %d: branch runs on root or beam" % len(self.done_ops))
        sb, cb = self._batch(src), self._batch("child")
        M, B, N = self.M, sb.B, self.case.N
        cand = held_tools.look_draw(rng, M, B, N)
        ok = ~skip_ref.wide_envs(sb.orc)
        verify = self._untouched(sb)
        got = None
        if sb.env is not None:
            sb.env.branch(self._dev(sb, cand), K, into=cb.env)
            e = cb.env
            got = {k: self._cpu(t).reshape((M, B) + tuple(t.shape[1:])) for k, t in (
                ("obs", e.obs), ("reward", e.reward), ("done", e.done), ("n_steps", e.frame_steps), ("flags", e.flags),
                ("ac_reward", e.ac_reward), ("min_sep", e.min_sep))}

        def rows(m, per):
            return slice(m * B * per, (m + 1) * B * per)

        def check(m, ref):
            # (the oracle now holds what child rows [m B, (m + 1) B) must hold: oracle_branch put the source's rows back where not ok)
            assert not (skip_ref.wide_envs(sb.orc) & ok).any(), "a candidate made an env WIDE in flight: not one of look_draw's"
            for k in skip_ref.STATE:
                getattr(cb.orc, k)[rows(m, N if k in skip_ref.PER_AIRCRAFT else 1)] = getattr(sb.orc, k)
            for k in ("obs", "reward", "ac_reward", "done", "flags", "min_sep"):     # what the device's child outputs must hold
                dst = getattr(cb.orc, k)
                val = np.asarray(ref[k]).reshape((B,) + dst.shape[1:])
                dst[rows(m, 1)] = np.where(ok.reshape((B,) + (1,) * (val.ndim - 1)), val, 0).astype(dst.dtype)
            if got is not None:
                bars.check_candidate_outputs({k: v[m] for k, v in got.items()}, ref, ok, self.half, tag=("branch", src, K, m))
        refs = branch_ref.oracle_branch(sb.orc, cand, K, ok, check)
        verify()
        if N > 1:
            self._check_traffic(cb)
        # the children's previous step: the branch's, with actions[m]; of a not-evaluated child: its source's
        okc = np.tile(ok, M)
        flat = cand.reshape(M * B, N, 3)
        cb.prev_actions = np.where(okc[:, None, None], flat, np.tile(sb.prev_actions, (M, 1, 1))).astype(np.float32)
        cb.has_prev = np.where(okc, True, np.tile(sb.has_prev, M))
        cb.la_touched = np.where(okc, False, np.tile(sb.la_touched, M))
        cb.branch_actions = flat.copy()
        cb.placed = [m * B + e for m in range(M) for e in sb.placed]
        cb.win_pending = []
        n = np.stack([r["n_steps"].astype(np.int64) for r in refs])[:, ok]
        done = np.stack([r["done"].astype(bool) for r in refs])[:, ok]
        rec = {"src": src, "pairs": M * B, "evaluated": M * int(ok.sum()), "evaluated_per_candidate": [int(ok.sum())] * M,
               "not_evaluated": M * int((~ok).sum()), "early": int((n < K).sum()), "ran_all": int((n == K).sum()), "done": int(done.sum()),
               "src_held_ok": bool(sb.has_prev.all() and not sb.la_touched.any())}
        if got is not None:
            rec["_out"] = [got[k] for k in sorted(got)] + ([self._cpu(cb.env.traffic)] if cb.env.traffic_k else [])
        return rec, [src, "child"]

    def _op_select(self, rng, dst, src, kind):
        if dst not in ("root", "beam") or dst == src:
            raise IllegalScript("operation %d: select writes root or beam from another batch" % len(self.done_ops))
        db, sb = self._batch(dst), self._batch(src)
        B, N = db.B, self.case.N
        mask = None
        rec = {"dst": dst, "src": src, "kind": kind}
        if kind == "commit":        # the best child of every env, by the ORACLE's rewards: both sides pick the same
            if src != "child":
                raise IllegalScript("commit takes children")
            idx = np.argmax(sb.orc.reward.reshape(self.M, B), axis=0).astype(np.int64) * B + np.arange(B)
        elif kind == "beam":        # the top B of all children, the best quarter twice
            order = np.argsort(-sb.orc.reward.astype(np.float64), kind="stable")[:B].astype(np.int64)
            order[B - B // 4:] = order[:B // 4]
            idx = order
        elif kind in ("stash", "restore", "zero"):
            if sb.B != B and kind != "zero":
                raise IllegalScript("%s moves every env between batches of one size" % kind)
            idx = np.arange(B, dtype=np.int64)
            if kind == "zero":
                mask = np.zeros(B, np.uint8)
        else:
            assert kind == "edge", kind
            idx = rng.integers(0, sb.B, B).astype(np.int64)
            at = rng.choice(B, 6, replace=False)
            idx[at[0]], idx[at[1]], idx[at[2]] = -1, sb.B, 2 ** 32 + 1      # (the last one is env 1 to whoever keeps 32 bits of it)
            idx[at[3]] = idx[at[4]] = idx[at[5]]                           # a repeated index
            mask = (rng.uniform(size=B) < 0.6).astype(np.uint8) * 7
            mask[at[:5]] = 1
            mask[at[5]] = 0
            rec["out_of_range_under_mask"] = 3
        sel = (idx >= 0) & (idx < sb.B) & (np.ones(B, bool) if mask is None else mask != 0)
        take = idx[sel]
        rec.update(selected=int(sel.sum()), of=B, repeats=int(len(take) - len(set(take.tolist()))),
                   wide_selected=int(skip_ref.wide_envs(sb.orc)[take].sum()),
                   hi_bit_clear_selected=int(((sb.orc.active_mask[take] >> np.uint64(32)) != (np.uint64(2 ** N - 1) >> np.uint64(32))).sum()) if N > 32 else 0)
        verify = self._untouched(sb)
        if db.env is not None:
            torch = db.env.torch
            before = {k: self._cpu(getattr(db.env, k)) for k in H.STATE + ("obs", "raw_obs")}
            index = torch.as_tensor(idx if kind != "commit" else idx.astype(np.int32), device=db.env.device)   # int64, and int32 once
            db.env.select(sb.env, index, None if mask is None else mask)
            aircraft = np.repeat(sel, N)
            for k in H.STATE:
                now = self._cpu(getattr(db.env, k))
                keep = aircraft if now.shape[0] == B * N else sel
                assert np.array_equal(now[~keep].view(np.uint8), before[k][~keep].view(np.uint8)), ("an env that was not selected changed", k)
            for k in ("obs", "raw_obs"):
                now, theirs = self._cpu(getattr(db.env, k)), self._cpu(getattr(sb.env, k))
                assert np.array_equal(now[~sel].view(np.int32), before[k][~sel].view(np.int32)), (k, "of an env that was not selected changed")
                assert np.array_equal(now[sel].view(np.int32), theirs[take].view(np.int32)), (k, "is not the source's row")
            rec["_out"] = [self._cpu(db.env.obs), self._cpu(db.env.raw_obs)] + ([self._cpu(db.env.traffic)] if db.env.traffic_k else [])
        # the oracles: a row gather
        ac_sel, ac_take = np.repeat(sel, N), (take[:, None] * N + np.arange(N)[None, :]).reshape(-1)
        for k in skip_ref.STATE:
            a, s = getattr(db.orc, k), getattr(sb.orc, k)
            if k in skip_ref.PER_AIRCRAFT:
                a[ac_sel] = s[ac_take]
            else:
                a[sel] = s[take]
        for k in ("obs", "raw_obs"):
            getattr(db.orc, k)[sel] = getattr(sb.orc, k)[take]
        db.prev_actions[sel], db.has_prev[sel], db.la_touched[sel] = sb.prev_actions[take], sb.has_prev[take], sb.la_touched[take]
        src_of = {int(e): int(s) for e, s in zip(np.nonzero(sel)[0], take)}
        db.win_pending = [(e, k) for e, k in db.win_pending if e not in src_of] + \
            [(e, k) for e, s in src_of.items() for (se, k) in sb.win_pending if se == s]
        db.placed = [e for e in db.placed if e not in src_of]
        verify()
        if N > 1:
            self._check_traffic(db)        # select() refreshes the destination's traffic observation
        return rec, [dst, src]

    def _op_replay(self, rng, first, count):
        """operations first .. first + count - 1 again with the inputs of their own script positions; what they returned and the state
        they left must be byte-equal to the first pass — on the device (a check that needs no oracle) and on the oracle"""
        if not 0 <= first and first + count <= len(self.done_ops):
            raise IllegalScript("replay of operations that have not run")
        names, rec = [], {"replayed": []}
        for j in range(first, first + count):
            op = self.done_ops[j]
            if op[0] == "replay":
                raise IllegalScript("a replay of a replay")
            sub = self._run_one(op, j)
            assert sub["_digest"][1] == self.digests[j][1], ("replay: the ORACLE's state differs from the first pass", j, op)
            assert sub["_digest"][0] == self.digests[j][0], ("replay: outputs or state differ from the first pass", j, op)
            rec["replayed"].append(op)
            rec["done"] = rec.get("done", 0) + sub.get("done", 0)
            names += [n for n in ([self._split(op)[2]] if op[0] in BATCH_OPS else [x for x in op[1:] if x in BATCHES] + (["child"] if op[0] == "branch" else []))
                      if n not in names]
        return rec, names

    def close(self):
        for bt in self.b.values():
            if bt.env is not None:
                bt.env.close()


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


# ---------------------------------------------------------------------------------------------------------------- tree scripts
def _tree_preamble():
    """The fixed opening of every tree script (tests/test_tree_sequences.py names each interaction and finds it in the oracle's record)."""
    p = [
        # read-only calls between held steps: each of the three scoring calls sits between two held steps of the root
        ("step", "fresh"), ("step", "held"), ("lookahead", 20, "fast"), ("step", "held"),
        ("plan", 5, 3, "all"), ("step", "held"), ("plan_sampled", 4, 2, True), ("step", "held"),
        # ... one directly after a skip with early-ended and full envs (session_ref.PREAMBLE: envs reset three steps before run all 20)
        ("reset", "random"), ("step", "fresh"), ("step", "held"), ("skip", 20), ("lookahead", 5, "all"), ("step", "held"),
        # ... one after a masked reset of some envs; the plan shape (M, H, outputs) of above again, then another one
        ("reset", "random"), ("plan", 5, 3, "all"), ("step", "held"), ("plan", 4, 2, "fast"), ("plan_sampled", 4, 2, False), ("step", "held"),
        # branch then hold: a source without WIDE envs (tame headings), some envs reset two steps ago, the others near their time limit
        ("reset", "random"), ("step", "tame"), ("step", "held"), ("branch", "root", 20), ("step", "branch", "child"),
        # flying the child on: the "keyed by c" clause needs children c >= B that are reset again, episodes later
        ("skip", 5, "child"), ("step", "held", "child"), ("rollout", 4, 1, True, "child"), ("rollout", 8, 4, False, "child"),
        ("reset", "random", "child"), ("observe", "random", "child"), ("traffic", "child"), ("skip", 20, "child"), ("step", "held", "child"),
        ("rollout", 4, 4, True, "child"), ("rollout", 3, 1, False, "child"), ("skip", 20, "child"), ("skip", 20, "child"),
        # WIDE sources: placed aircraft at a WIDE heading (and wild heading targets) in the source; the not-evaluated children — byte
        # copies — hold their SOURCE's previous actions, are observed, given the traffic observation, and flown on
        ("set_state",), ("step", "fresh"), ("step", "held"), ("branch", "root", 5), ("step", "held", "child"), ("observe", "none", "child"),
        ("traffic", "child"), ("skip", 2, "child"), ("rollout", 4, 4, True, "child"),
        # stash (WIDE and handed-over rows go root -> beam), fly the root on, restore (beam -> root), the same operations again
        ("select", "beam", "root", "stash"),
    ]
    window = [("step", "fresh"), ("step", "held"), ("skip", 5), ("rollout", 4, 4, True), ("traffic",), ("observe", "random"),
              ("reset", "random"), ("step", "repeat")]
    first = len(p)
    p += window + [
        ("select", "root", "beam", "restore"), ("replay", first, len(window)),
        ("step", "held", "beam"), ("observe", "none", "beam"), ("traffic", "beam"),            # the stashed WIDE rows, flown in the beam
        # beam loop: root -> child -> select beam -> beam.branch -> child, two rounds, then commit; the root holds the gathered actions
        ("branch", "root", 10), ("select", "beam", "child", "beam"), ("lookahead", 5, "fast", "beam"),
        ("branch", "beam", 10), ("select", "beam", "child", "beam"), ("step", "held", "beam"),
        ("select", "root", "child", "commit"), ("step", "held"), ("step", "held"),
        # select edges: repeated, negative, too large and beyond-32-bit indices under a partial mask; an all-zero mask
        ("select", "beam", "child", "edge"), ("step", "held", "beam"), ("select", "root", "beam", "zero"), ("step", "held"), ("traffic", "beam"),
    ]
    return tuple(p)


TREE_PREAMBLE = _tree_preamble()
TREE_LENGTH = len(TREE_PREAMBLE) + 14
BRANCH_KS = (2, 5, 10, 20)


def make_tree_script(case):
    """TREE_PREAMBLE + operations drawn from the case's seed, TREE_LENGTH in all.  A held step is only drawn where it is legal whatever the
    oracle shows: every env of the batch has a previous step (its own, its branch's, its source's) and no last-action record was written
    in the batch or in a batch its envs may have come from."""
    rng = np.random.default_rng([case.seed, 1 << 21])
    script = list(TREE_PREAMBLE)
    stepped = {n: True for n in BATCHES}        # (the preamble leaves every env of every batch with a previous step)
    touched = {n: False for n in BATCHES}
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]   # noqa: E731
    while len(script) < TREE_LENGTH:
        r = rng.uniform()
        bt = pick(BATCHES)
        far = pick(("root", "beam"))
        if r < 0.22:
            mode = pick(("fresh", "repeat", "held", "held"))
            if touched[bt] and mode == "held":
                mode = "repeat"
            if not stepped[bt]:
                mode = "fresh"
            op = ("step", mode, bt)
        elif r < 0.30:
            op = ("skip", pick(SKIP_KS), bt)
        elif r < 0.38:
            hold = pick((1, 4))
            op = ("rollout", hold * int(rng.integers(1, 3)), hold, bool(rng.integers(0, 2)), bt)
        elif r < 0.46:
            op = (pick(("reset", "observe")), pick(MASK_KINDS[:4]), bt)
        elif r < 0.50:
            op = ("traffic", bt)
        elif r < 0.54:
            op = (pick(("set_state", "set_last_action")), far)
        elif r < 0.62:
            op = ("lookahead", pick(SKIP_KS), pick(("fast", "all")), far)
        elif r < 0.69:
            op = ("plan", pick((2, 5)), pick((2, 3)), pick(("fast", "all")), far)
        elif r < 0.76:
            op = ("plan_sampled", pick((2, 4)), pick((1, 2, 3)), bool(rng.integers(0, 2)), far)
        elif r < 0.88:
            op = ("branch", far, pick(BRANCH_KS))
        else:
            kind = pick(SELECT_KINDS)
            dst, src = {"commit": ("root", "child"), "beam": ("beam", "child"), "stash": ("beam", "root"), "restore": ("root", "beam"),
                        "edge": (far, "child"), "zero": (far, "child")}[kind]
            op = ("select", dst, src, kind)
        if op[0] in ("step", "skip", "rollout"):
            stepped[bt], touched[bt] = True, False
        elif op[0] == "set_last_action":
            touched[far] = True
        elif op[0] == "branch":
            stepped["child"], touched["child"] = stepped[op[1]], touched[op[1]]
        elif op[0] == "select" and op[3] != "zero":
            dst, src, whole = op[1], op[2], op[3] != "edge"
            stepped[dst] = stepped[src] and (whole or stepped[dst])
            touched[dst] = touched[src] or (touched[dst] and not whole)
        script.append(op)
    return script


# ---------------------------------------------------------------------------------------------------------------- planner scripts
def mixed_skip_k(case):
    """K of the planner scripts' step_skip that must leave early AND full envs behind: 20 — envs reset two steps before run all 20 under a
    time limit of 22 or more, the others meet it inside the block —, but 12 with 64 aircraft, where within 20 steps every env of the
    batch ends on something else than its time limit"""
    return 12 if case.N == 64 else 20


def make_planner_script(case):
    """A tree script around ("plan_iter", ...): the operation between two held steps; directly after a step_skip with early and full envs
    (mixed_skip_k); after a masked reset of some envs; directly before ("step", "decision"), which flies the decision, and a held step
    that holds it on; on the beam after a select, decision flown there.  The two modes, M in {3, 5, 8} and H in {1, 2, 3} rotate; one
    shape comes twice.  The case seeds the operations' inputs and sets that one K; the rest of the script is fixed."""
    return [
        ("step", "fresh"), ("step", "held"), ("plan_iter", "elite", 8, 3), ("step", "held"),
        ("skip", 5), ("reset", "random"), ("step", "fresh"), ("step", "held"), ("skip", mixed_skip_k(case)), ("plan_iter", "softmax", 5, 2),
        ("step", "held"),
        ("reset", "random"), ("plan_iter", "elite", 3, 1), ("step", "held"),
        ("plan_iter", "softmax", 8, 3), ("step", "decision"), ("step", "held"),
        ("plan_iter", "elite", 5, 2), ("step", "decision"), ("step", "held"), ("plan_iter", "elite", 8, 3), ("step", "held"),
        ("reset", "random"), ("step", "tame"), ("step", "held"), ("branch", "root", 5), ("select", "beam", "child", "beam"),
        ("plan_iter", "elite", 8, 2, "beam"), ("step", "decision", "beam"), ("step", "held", "beam"),
        ("select", "beam", "root", "stash"), ("plan_iter", "softmax", 3, 3, "beam"), ("step", "decision", "beam"),
        ("select", "root", "beam", "restore"), ("step", "held"),
    ]
