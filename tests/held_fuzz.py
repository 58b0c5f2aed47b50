"""Randomised differential harness for the held-block kernels — k_skip (atc_step_skip), k_lookahead (atc_lookahead), k_plan
(atc_lookahead_plan) — and k_traffic (atc_observe_traffic) against the fp32 oracle.  TEST INFRASTRUCTURE ONLY; importing it needs no GPU.

case(seed) draws the env configuration with tests/fuzz_space.py::parity_case (that function and its draws are untouched: the batch size,
the step count and the launch form it draws are simply not used here) and, from a random stream of its own, a small batch, a time limit
that ends episodes inside held blocks, and the calls.  run(seed) flies them on an AtcVecEnv and an oracle.OracleEnv built from the same
configuration by fuzz_space.make_env / make_oracle, the way fuzz_space.run_vs_oracle builds them:
  reset observation; 2-4 step_skip calls (tests/skip_ref.py, bars.check_skip_outputs, bars.check_state); observe_traffic (tests/traffic_ref.py
  on the oracle's state); lookahead (skip_ref.candidate_references) and lookahead_plan (skip_ref.plan_references) with the six state
  tensors compared byte for byte with a clone taken before and bars.check_state against the untouched oracle; one more step_skip.
Every comparison is one of tests/bars.py; nothing here has a tolerance of its own.  run(seed, device=False) runs the oracle side alone
and returns the case's event record, which tests/test_fuzz_held.py holds to what the sweep is for.
tests/fuzz_debug.py --held <seed> replays one case and prints the first deviation with its context."""
import numpy as np

import bars
import helpers as H
import skip_ref as R
import traffic_ref
from fuzz_space import NON_DYADIC, Mismatch, draw_actions, make_env, make_oracle, parity_case

FLOWN_K = (1, 2, 5, 20, 60)
LOOK_M, LOOK_K = (1, 3, 8), (1, 4, 20)
PLAN_M, PLAN_H, PLAN_K = (1, 3), (1, 2, 4), (1, 5, 20)
LOOK_OUTPUTS = ("flags", "min_sep", "ac_reward", "obs")
PLAN_OUTPUTS = ("seg_reward",) + LOOK_OUTPUTS
KERNELS = ("skip", "lookahead", "plan")
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
REFUSED = H.F_INVALID_V | H.F_INVALID_H
HEADING_WILD_ENVS = 0.25    # share of a flown call's envs whose HEADING components take part in the `wild` draw (env 0 never does)
_ENV_KEYS = ("N", "seed", "dt", "discrete", "spawn", "grid_cell", "full", "shaping", "normalize", "sep_nm", "keep_active")


# ---------------------------------------------------------------------------------------------------------------- the draw
def case(seed):
    """(scn, comp, kw) of one case.  kw: the env configuration (fuzz_space.parity_case's, with B in 1 .. 120 — fewer at N > 16, so that the
    oracle stays cheap — and timestep_limit in {6000, 40, 12}), auto_reset_off (a quarter of the cases: switched off after flying), and
    the calls: flown [K, ...], lookahead / plan dicts, traffic (K of observe_traffic; 0 at N == 1), last (K of the closing step_skip)."""
    scn, comp, drawn = parity_case(int(seed), n_cu=256)    # (n_cu given: no device is asked for its CU count)
    kw = {k: drawn[k] for k in _ENV_KEYS}
    kw["wild"] = float(drawn.get("wild", 0.0))
    rng = np.random.default_rng([int(seed), 0x48454C44])
    N = kw["N"]
    kw["B"] = min(int(rng.integers(1, 121)), max(4, 1920 // N))
    kw["timestep_limit"] = int(rng.choice([6000, 40, 12]))
    kw["auto_reset_off"] = bool(rng.integers(4) == 0)
    kw["flown"] = [int(k) for k in rng.choice(FLOWN_K, int(rng.integers(2, 5)))]

    def subset(names):   # a quarter: none (the fast form); otherwise each with probability 1 / 2
        return () if int(rng.integers(4)) == 0 else tuple(n for n in names if int(rng.integers(2)))

    M = int(rng.choice(LOOK_M))
    kw["lookahead"] = dict(M=M, K=int(rng.choice(LOOK_K)), outputs=subset(LOOK_OUTPUTS), mapping=int(rng.choice([0, 1, 2, M])))
    M = int(rng.choice(PLAN_M))
    kw["plan"] = dict(M=M, H=int(rng.choice(PLAN_H)), K=int(rng.choice(PLAN_K)), outputs=subset(PLAN_OUTPUTS),
                      mapping=int(rng.choice([0, 1, 2, M])))
    kw["traffic"] = int(rng.integers(1, 9)) if N > 1 else 0
    kw["last"] = int(rng.choice(FLOWN_K[:4]))
    return scn, comp, kw


_drawn_case = case     # (run() has an argument of that name)


def draw_flown(rng, B, N, discrete, wild):
    """The actions of a flown step_skip call: fuzz_space.draw_actions, with the HEADING components taking part in the `wild` share in
    HEADING_WILD_ENVS of the envs (env 0 never does)."""
    heading_wild = rng.uniform(size=B) < HEADING_WILD_ENVS
    heading_wild[0] = False
    return draw_actions(rng, (B, N), discrete, wild, heading_wild)


def draw_candidates(rng, shape, discrete, wild):
    """Candidate / plan actions: wild in the speed and altitude components only, headings inside the action space."""
    a = draw_actions(rng, shape, discrete, wild, False)
    if not discrete:
        a[..., 2] = np.clip(a[..., 2], -1.0, 1.0)
    return a


def properties(scn, kw):
    """the names of the mode-space properties a case has (what tests/test_fuzz_held.py counts per kernel)"""
    from atc_hip.vec_env import auto_grid_cell
    cell = auto_grid_cell(kw["B"], kw["N"]) if kw["grid_cell"] == "auto" else kw["grid_cell"]
    p = {"W=%d" % H.lane_width(kw["N"])}
    for name, has in (("discrete actions", kw["discrete"]), ("no lookup grid", cell is None), ("0.125 nm grid", cell == 0.125),
                      ("non-dyadic dt", kw["dt"] in NON_DYADIC), ("shaping off", not kw["shaping"]), ("sep_nm 0", kw["sep_nm"] == 0.0),
                      ("keep_active", kw["keep_active"]), ("auto-reset off", kw["auto_reset_off"]),
                      ("SimpleScenario", type(scn).__name__ == "SimpleScenario")):
        if has:
            p.add(name)
    return p


# ---------------------------------------------------------------------------------------------------------------- events
def _new_events():
    return dict(pairs=0, n_hist={}, early=0, differ=0, done=0, reset_in_block=0, conflict=0, below_mva=0, inactive=0, refused=0,
                refused_repeated=0, late_stop=0, late_reset=0, noise=0)


def _add_n(ev, n, done, limit):
    """n [..., B'] executed steps of evaluated (candidate, env) pairs; limit: the call's K (H K of a plan)"""
    ev["pairs"] += int(n.size)
    for v, c in zip(*np.unique(n, return_counts=True)):
        ev["n_hist"][int(v)] = ev["n_hist"].get(int(v), 0) + int(c)
    ev["early"] += int((n < limit).sum())
    ev["done"] += int(done.sum())


def _add_block(ev, ref, K, mask, auto_reset, watch=None):
    """one skip_reference result, the envs of mask [B]: what its executed steps' flag words show, and resets with steps of the block left.
    watch(ref, executed [K, B], auto_reset): a caller's own count on the same steps (tests/noise_sectors.py::Coverage.add_block)"""
    n = ref["n_steps"].astype(int)
    executed = (np.arange(K)[:, None] < n[None, :]) & mask[None, :]
    if watch is not None:
        watch(ref, executed, auto_reset)
    sf = np.where(executed[:, :, None], ref["step_flags"], 0)
    for name, bit in (("conflict", H.F_CONFLICT), ("below_mva", H.F_BELOW_MVA), ("inactive", H.F_INACTIVE), ("refused", REFUSED),
                      ("noise", H.F_NOISE)):
        ev[name] += int((sf & bit != 0).any(axis=(0, 2)).sum())
    ev["refused_repeated"] += int((sf[1:] & REFUSED != 0).any(axis=(0, 2)).sum())
    if auto_reset:
        ev["reset_in_block"] += int((ref["done"].astype(bool) & (n < K) & mask).sum())


# ---------------------------------------------------------------------------------------------------------------- the run
def _counters():
    from atc_hip import lib
    return dict(step=lib.launch_counts(), skip=lib.skip_launch_counts(), lookahead=lib.lookahead_launch_counts(),
                plan=lib.plan_launch_counts(), traffic=lib.traffic_launch_counts())


def _gained(before, after):
    """{record: {name: launches}} of what the launch records gained; records that gained nothing are left out"""
    out = {}
    for k, now in after.items():
        g = {n: c - before[k].get(n, 0) for n, c in now.items() if c != before[k].get(n, 0)}
        if g:
            out[k] = g
    return out


def _skip_outputs(env, ret, full):
    B, N = env.B, env.N
    obs, rew, done, info = ret
    cpu = lambda t: t.cpu().numpy()   # noqa: E731
    got = {"flags": cpu(info["flags"]), "done": cpu(done), "n_steps": cpu(info["frame_steps"]), "obs": cpu(obs).reshape(B, N, 10),
           "reward": cpu(rew)}
    if full:
        got.update(raw_obs=cpu(info["original_state"]).reshape(B, N, 10), ac_reward=cpu(info["aircraft_reward"]),
                   min_sep=cpu(info["min_separation"]), term_obs=cpu(info["terminal_observation"]).reshape(B, N, 10))
    return got


def run(seed, device=True, case=None, watch=None):
    """Flies case(seed) — or the given case=(scn, comp, kw) of the same shape (tests/noise_sectors.py::noise_case).  watch: {kernel: _add_block's
    watch}.  device=True: on the GPU against the oracle (raises Mismatch at the first comparison that fails); device=False:
    the oracle alone.  Returns the case's record: seed, kw, props (properties()), events {kernel: counts} on the oracle's results —
    pairs (evaluated (candidate, env) pairs), n_hist, early, differ (envs whose candidates stop at different n), done, reset_in_block
    (auto-reset with steps of the block left), conflict / below_mva / inactive / noise / refused / refused_repeated (a refused target on a step
    j >= 1 of a block), late_stop / late_reset (a plan that ends in a segment h >= 1; with auto-reset on) —, wide {kernel: (pairs excluded
    as WIDE at the start, pairs)}, traffic_short (aircraft under control with fewer than K others) and, on the device, launches (what each
    launch record gained)."""
    scn, comp, kw = case if case is not None else _drawn_case(seed)
    ctx = {"seed": int(seed), "call": "setup", "kw": kw}
    rec = dict(seed=int(seed), kw=kw, props=properties(scn, kw), events={k: _new_events() for k in KERNELS}, wide={}, traffic_short=0)
    env = None
    try:
        start = _counters() if device else None
        orc = make_oracle(comp, kw, auto_reset=True)
        env = make_env(scn, kw, auto_reset=True) if device else None
        _fly(env, orc, comp, kw, rec, ctx, watch or {})
        if device:
            rec["launches"] = _gained(start, _counters())
    except AssertionError as e:
        if isinstance(e, Mismatch):
            raise
        raise Mismatch(ctx, e, "held fuzz case %s, %s" % (ctx.get("seed"), ctx.get("call"))) from e
    finally:
        if env is not None:
            from atc_hip import lib
            lib.lookahead_set_mapping(0)
            env.close()
    return rec


def _fly(env, orc, comp, kw, rec, ctx, watch):
    B, N, full, discrete, wild = kw["B"], kw["N"], kw["full"], kw["discrete"], kw["wild"]
    half = bars.half_range(comp)
    rng = np.random.default_rng([kw["seed"], 0x464C59])
    ev = rec["events"]
    if env is not None:
        import torch
        from atc_hip import lib
        # 1. the reset observation
        ctx.update(call="reset")
        o0 = env.obs.cpu().numpy().reshape(B, N, 10)
        assert np.all(np.abs(o0 - orc.obs) <= 1e-5 * np.maximum(1.0, np.abs(orc.obs))), "reset observation"

    def skip_call(tag, K, auto_reset):
        a = draw_flown(rng, B, N, discrete, wild)
        ref = R.skip_reference(orc, a, K)
        _add_n(ev["skip"], ref["n_steps"].astype(int), ref["done"].astype(bool), K)
        _add_block(ev["skip"], ref, K, np.ones(B, bool), auto_reset, watch.get("skip"))
        if env is not None:
            got = _skip_outputs(env, env.step_skip(a, K), full)
            ctx.update(call=tag, K=K, got=got, ref=ref, records=None, cand=None)
            bars.check_skip_outputs(got, ref, half, full, tag)
            bars.check_state(env, orc)

    # 2. the flown calls
    for c, K in enumerate(kw["flown"]):
        skip_call("step_skip %d (K = %d)" % (c, K), K, True)
    auto_reset = not kw["auto_reset_off"]
    if not auto_reset:
        from oracle import oracle as O
        orc.params.mode &= ~O.M_AUTO_RESET
        if env is not None:
            H.set_auto_reset(env, False)

    # 3. the traffic observation of the state the calls left
    if kw["traffic"]:
        st = traffic_ref.state_from_oracle(orc)
        if env is not None:
            ctx.update(call="observe_traffic (K = %d)" % kw["traffic"], got=None, ref=None)
            t = env.observe_traffic()
            env.synchronize()
            tref = traffic_ref.check_traffic(t.cpu().numpy(), st, comp, kw["traffic"], kw["normalize"], "traffic K %d" % kw["traffic"])
        else:
            tref = traffic_ref.traffic_reference(st, comp.pos_origin, comp.pos_k)
        rec["traffic_short"] = int((traffic_ref.active_bits(orc.active_mask, N) & (tref["ncand"] < kw["traffic"])).sum())

    # 4. / 5. the look-ahead and the plan, from the same state; 6. which they leave as it is
    ok = ~R.wide_envs(orc)
    if env is not None:
        snap = H.snapshot(env)
    for kernel in ("lookahead", "plan"):
        c = kw[kernel]
        M, K, Hn = c["M"], c["K"], c.get("H")
        cand = draw_candidates(rng, (M, B, N) if Hn is None else (M, Hn, B, N), discrete, wild)
        records = [] if Hn is not None else None
        refs = R.candidate_references(orc, cand, K) if Hn is None else R.plan_references(orc, cand, K, records)
        rec["wide"][kernel] = (M * int((~ok).sum()), M * B)
        n = np.stack([r["n_steps"].astype(int) for r in refs])[:, ok]
        done = np.stack([r["done"].astype(bool) for r in refs])[:, ok]
        _add_n(ev[kernel], n, done, K * (Hn or 1))
        if n.size:
            ev[kernel]["differ"] += int((n.min(0) != n.max(0)).sum())
        for m in range(M):
            if Hn is None:
                _add_block(ev[kernel], refs[m], K, ok, auto_reset, watch.get(kernel))
            else:
                for alive, r in records[m]:
                    _add_block(ev[kernel], r, K, ok & alive, auto_reset, watch.get(kernel))
        if Hn is not None:
            late = done & (n > K)
            ev[kernel]["late_stop"] += int(late.sum())
            ev[kernel]["late_reset"] += int(late.sum()) if auto_reset else 0
        if env is None:
            continue
        before = _counters()
        lib.lookahead_set_mapping(c["mapping"])
        tag = "%s (M = %d, %sK = %d, outputs %s, mapping %d)" % (kernel, M, "" if Hn is None else "H = %d, " % Hn, K,
                                                               "+".join(c["outputs"]) or "none", c["mapping"])
        ctx.update(call=tag, K=K, got=None, ref=None)
        at = torch.as_tensor(cand, device=env.device)
        res = env.lookahead(at, K, outputs=c["outputs"]) if Hn is None else env.lookahead_plan(at, K, outputs=c["outputs"])
        lib.lookahead_set_mapping(0)
        assert set(res) == {"reward", "done", "n_steps"} | set(c["outputs"]), ("outputs that were not requested must not exist", sorted(res))
        got = {k: v.cpu().numpy() for k, v in res.items()}
        moved = _gained(before, _counters())
        assert moved == {kernel: {H.lane_width(N): 1}}, ("launch records moved by the call", moved)
        for m in range(M):
            g = {k: v[m] for k, v in got.items()}
            ctx.update(cand=m, got=g, ref=refs[m], records=records[m] if records else None, ok=ok)
            bars.check_candidate_outputs({k: v for k, v in g.items() if k != "seg_reward"}, refs[m], ok, half, tag=(kernel, m))
            if "seg_reward" in g:
                bars.check_plan_segments(g["seg_reward"], refs[m], ok, K, tag=(kernel, m))
        ctx.update(call=tag + ": state afterwards", got=None, ref=None, cand=None)
        H.bytes_equal(env, snap)
        bars.check_state(env, orc)

    # 7. one more frame-skip call: the queries left nothing behind
    skip_call("closing step_skip (K = %d)" % kw["last"], kw["last"], auto_reset)


# ---------------------------------------------------------------------------------------------------------------- replay
def first_deviation(got, ref, half, ok=None):
    """(output, env, aircraft or None, got, ref) of the first word of `got` outside its bar (tests/bars.py), or None"""
    B = ref["obs"].shape[0]
    ok = np.ones(B, bool) if ok is None else ok

    def first(key, bad):
        bad = bad & ok.reshape((B,) + (1,) * (bad.ndim - 1))
        if not bad.any():
            return None
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        g, r = np.asarray(got[key]).reshape(np.asarray(ref[key]).shape), np.asarray(ref[key])
        return key, idx[0], (idx[1] if len(idx) > 1 else None), g[idx], r[idx]

    def val(key):
        return np.asarray(got[key]).reshape(np.asarray(ref[key]).shape)

    for key in ("n_steps", "done", "flags", "min_sep"):
        if key in got:
            g = val(key).astype(np.uint16) if key == "flags" else val(key)
            hit = first(key, g.astype(np.float64) != np.asarray(ref[key]).astype(np.float64))
            if hit:
                return hit
    for key, scale in (("obs", None), ("raw_obs", half), ("term_obs", None), ("reward", "reward_scale"), ("ac_reward", "ac_reward_scale")):
        if key in got:
            r = np.asarray(ref[key]).astype(np.float64)
            bar = 1e-5 * (np.maximum(1.0, np.abs(r)) if scale is None else ref[scale] if isinstance(scale, str) else scale)
            hit = first(key, np.abs(val(key).astype(np.float64) - r) > bar)
            if hit:
                return hit
    return None


def describe(mismatch, comp):
    """prints a Mismatch: the call, the candidate, the segment, the env and aircraft of the first deviation and the oracle's per-step
    record (skip_reference's step_done / step_flags) of that env"""
    ctx = mismatch.ctx
    print("FIRST DEVIATION in", ctx.get("call"), "-", mismatch.what)
    got, ref = ctx.get("got"), ctx.get("ref")
    if got is None or ref is None:
        return
    K, records, ok = ctx.get("K"), ctx.get("records"), ctx.get("ok")
    if ctx.get("cand") is not None:
        print(" candidate", ctx["cand"])
    hit = first_deviation(got, ref, bars.half_range(comp), ok)
    seg = None
    if hit is None and "seg_reward" in got:
        err = np.abs(np.asarray(got["seg_reward"], np.float64) - ref["seg_reward"]) > 1e-5 * ref["seg_reward_scale"]
        if err.any():
            seg, e = (int(i) for i in np.argwhere(err)[0])
            hit = ("seg_reward", e, None, got["seg_reward"][seg, e], ref["seg_reward"][seg, e])
    if hit is None:
        print(" (no output word outside its bar: a not-evaluated env that did not return zeros, or the state)")
        return
    key, e, k, g, r = hit
    n = int(ref["n_steps"][e])
    if records is not None and seg is None:
        seg = max(0, -(-n // K) - 1)      # the segment the env took its last step in
    print(" output %s, env %d, aircraft %s%s: device %r, oracle %r" % (key, e, k, "" if seg is None else ", segment %d" % seg, g, r))
    print(" oracle: n_steps %d, done %d, flags %s" % (n, int(ref["done"][e]), ref["flags"][e].tolist()))
    for h, (alive, sref) in enumerate(records if records is not None else [(np.ones(len(ref["n_steps"]), bool), ref)]):
        if not alive[e]:
            break
        steps = int(sref["n_steps"][e])
        print(" oracle per step%s: done %s" % ("" if records is None else " (segment %d)" % h, sref["step_done"][:steps, e].astype(int).tolist()))
        fl = sref["step_flags"][:steps, e]
        print("   flags of aircraft %s per step: %s" % (k if k is not None else "(OR over the env)",
                                                      (fl[:, k] if k is not None else np.bitwise_or.reduce(fl, axis=1)).tolist()))
