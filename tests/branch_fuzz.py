"""Randomised differential harness for k_branch (atc_branch) against the fp32 oracle.  TEST INFRASTRUCTURE ONLY; importing it needs no GPU.

The cases are tests/held_fuzz.py's: case(seed) is held_fuzz.case(seed) — fuzz_space.parity_case's env configuration (sectors, lookup
grids, timesteps, discrete actions, shaping off, sep_nm, actions outside the action space), a small batch, a time limit that ends
episodes inside held blocks — flown the way held_fuzz.run flies them: the same random stream, the same frame-skip calls with
held_fuzz.draw_flown (heading components in the out-of-space draw in a quarter of the envs, never env 0), auto-reset switched off
afterwards in a quarter of the cases.  The case's look-ahead draw (M, K, candidate mapping; candidates by held_fuzz.draw_candidates) is
then flown as ONE atc_branch into a child env of M B envs and compared with tests/skip_ref.py on the oracle, candidate by candidate
(branch_ref.oracle_branch: skip_ref.candidate_references' loop — skip_reference per candidate from a snapshot — with the child-state
comparison made BEFORE the oracle is restored, which candidate_references leaves no room for):
outputs by bars.check_candidate_outputs, the child's state rows by bars.check_state, the parent's state byte for byte and against the
untouched oracle.  run(seed, device=False) flies the oracle side alone and returns the record tests/test_fuzz_branch.py's CPU twin reads."""
import numpy as np

import bars
import branch_ref as BR
import helpers as H
import held_fuzz as F
import skip_ref as R
from fuzz_space import Mismatch, make_env, make_oracle

SEEDS = range(5000, 5040)     # the first 40 cases of tests/test_fuzz_held.py's default sweep


def run(seed, device=True, case=None, watch=None):
    """case: (scn, comp, kw) shaped like held_fuzz.case(seed)'s, flown in its place (tests/noise_sectors.py::noise_case); watch:
    held_fuzz._add_block's, for the branch's blocks.  Returns dict(seed, kw, pairs, excluded (pairs not evaluated: WIDE at the start, on the oracle), events (held_fuzz's counters on the oracle's
    results)) and, on the device, launches (what the branch launch record gained) and not_evaluated (pairs the device returned n_steps == 0
    for; asserted equal to excluded)."""
    scn, comp, kw = case if case is not None else F.case(seed)
    ctx = {"seed": int(seed), "call": "setup", "kw": kw}
    B, N, discrete, wild = kw["B"], kw["N"], kw["discrete"], kw["wild"]
    c = kw["lookahead"]
    M, K = c["M"], c["K"]
    rec = dict(seed=int(seed), kw=kw, pairs=M * B, excluded=0, events=F._new_events())
    env = child = None
    try:
        orc = make_oracle(comp, kw, auto_reset=True)
        if device:
            import torch
            from atc_hip import lib
            env = make_env(scn, kw, auto_reset=True)
        rng = np.random.default_rng([kw["seed"], 0x464C59])
        for j, Kf in enumerate(kw["flown"]):
            a = F.draw_flown(rng, B, N, discrete, wild)
            R.skip_reference(orc, a, Kf)
            if device:
                ctx.update(call="step_skip %d (K = %d)" % (j, Kf))
                env.step_skip(a, Kf)
                bars.check_state(env, orc)
        auto_reset = not kw["auto_reset_off"]
        if not auto_reset:
            from oracle import oracle as O
            orc.params.mode &= ~O.M_AUTO_RESET
            if device:
                H.set_auto_reset(env, False)
        ok = ~R.wide_envs(orc)
        rec["excluded"] = M * int((~ok).sum())
        cand = F.draw_candidates(rng, (M, B, N), discrete, wild)
        check = None
        if device:
            ctx.update(call="branch (M = %d, K = %d, mapping %d)" % (M, K, c["mapping"]))
            # (the parent's RESOLVED grid cell: "auto" depends on the batch size, and the child must be built on the parent's sector blob)
            child = BR.child_of(env, M, lambda b: make_env(scn, kw, B=b, auto_reset=True, grid_cell=env.grid_cell))
            snap = H.snapshot(env)
            before = lib.branch_launch_counts()
            lib.lookahead_set_mapping(c["mapping"])
            env.branch(torch.as_tensor(cand, device=env.device), K, into=child)
            lib.lookahead_set_mapping(0)
            now = lib.branch_launch_counts()
            rec["launches"] = {w: n - before.get(w, 0) for w, n in now.items() if n != before.get(w, 0)}
            names = ("obs", "reward", "done", "flags") + (("ac_reward", "min_sep") if kw["full"] else ())
            got = {k: getattr(child, k).cpu().numpy().reshape((M, B) + ((-1,) if getattr(child, k).dim() > 1 else ())) for k in names}
            got["n_steps"] = child.frame_steps.cpu().numpy().reshape(M, B)
            H.bytes_equal(env, snap)
            # what the DEVICE left out: exactly the pairs the oracle calls WIDE at the start (the bound of the test counts these)
            rec["not_evaluated"] = int((got["n_steps"] == 0).sum())
            assert rec["not_evaluated"] == rec["excluded"], ("pairs with n_steps == 0", rec["not_evaluated"], rec["excluded"])
            check = BR.child_check(child, orc, got, bars.half_range(comp), ok, "branch fuzz %d" % seed)
        refs = BR.oracle_branch(orc, cand, K, ok, check)
        n = np.stack([r["n_steps"].astype(int) for r in refs])[:, ok]
        done = np.stack([r["done"].astype(bool) for r in refs])[:, ok]
        F._add_n(rec["events"], n, done, K)
        if n.size:
            rec["events"]["differ"] += int((n.min(0) != n.max(0)).sum())
        for r in refs:
            F._add_block(rec["events"], r, K, ok, auto_reset, watch)
        if device:
            ctx.update(call="the parent afterwards")
            bars.check_state(env, orc)
    except AssertionError as e:
        if isinstance(e, Mismatch):
            raise
        raise Mismatch(ctx, e, "branch fuzz case %s, %s" % (ctx.get("seed"), ctx.get("call"))) from e
    finally:
        if device:
            from atc_hip import lib
            lib.lookahead_set_mapping(0)
        for e in (env, child):
            if e is not None:
                e.close()
    return rec
