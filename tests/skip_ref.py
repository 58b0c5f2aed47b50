"""Reference of the frame-skip call (include/atc_step.h: atc_step_skip) on the CPU oracle.  TEST INFRASTRUCTURE ONLY.

skip_reference(orc, actions, K) is the definition — per env: step with the same actions until the step reports done or K steps are
taken; outputs and state are those of the n executed steps — evaluated for a whole batch: the oracle steps K times on ALL envs,
every step's state and outputs are kept, each env's n follows from the done column, and the env's rows of its step-n snapshot go
back into the oracle's arrays, so that consecutive calls chain.  Envs are independent and the oracle's reset sampler is keyed by
(seed, env, episode, slot), so what an env does after its own step n changes nothing for the others.

candidate_references / plan_references are the look-ahead and the plan call (atc_lookahead, atc_lookahead_plan) on the same footing: the
frame-skip reference per candidate — chained over a plan's segments, an env leaving at its first done — from a snapshot of the oracle
that is restored after each candidate."""
import numpy as np

# the 16 state arrays of oracle.OracleEnv (its _st table) and which of them have one row per aircraft (the others: one per env)
STATE = ("px", "py", "h", "_phi", "_v", "last_act", "timesteps", "actions_taken", "total_reward", "active_mask", "win_bits",
         "episodes", "ep_return", "ep_length", "ep_actions", "phi_wide")
PER_AIRCRAFT = ("px", "py", "h", "_phi", "_v", "last_act", "phi_wide")
OUTPUTS = ("obs", "raw_obs", "reward", "ac_reward", "done", "flags", "min_sep", "term_obs")


def snapshot_state(orc):
    return {k: getattr(orc, k).copy() for k in STATE}


def snapshot(orc):
    """state and output arrays of the oracle, for restore()"""
    return snapshot_state(orc), {k: getattr(orc, k).copy() for k in OUTPUTS}


def restore(orc, snap):
    for part in snap:
        for k, v in part.items():
            getattr(orc, k)[...] = v


def wide_envs(orc):
    """[B] bool: envs with an aircraft whose heading or last heading target is WIDE (saturated 32-bit field, include/atc_step.h ABI 19):
    the look-ahead calls do not evaluate them.  (orc: the fp32 instantiation — the float64 one has no such field)"""
    edge = (-2 ** 31, 2 ** 31 - 1)
    return np.isin(orc.last_act[:, 1], edge).reshape(orc.B, orc.N).any(1) | np.isin(orc.phi_fix, edge).reshape(orc.B, orc.N).any(1)


def f32_sequential_sum(terms, n, dtype=np.float32):
    """acc = t[0]; acc = acc + t[1]; ... over the first n[b] terms of every column, plain additions in `dtype` (float32: the kernels' and
    the fp32 oracle's; float64 for a reference built on the float64 oracle).  terms: [K, ...] with the env axis second; n: [B] (broadcast
    over trailing axes)."""
    terms = np.asarray(terms, dtype)
    acc = terms[0].copy()
    for j in range(1, terms.shape[0]):
        live = (j < n).reshape((-1,) + (1,) * (acc.ndim - 1))
        acc = np.where(live, (acc + terms[j]).astype(dtype), acc)
    return acc


def skip_reference(orc, actions, K):
    """Runs one frame-skip call of length K on the oracle env `orc` (left in the state after the call) and returns a dict:
    obs, raw_obs, reward, ac_reward, done, flags, min_sep, term_obs, n_steps as the call defines them, plus
    reward_scale [B] / ac_reward_scale [B, N] = sum over the executed steps of max(1, |r_j|) (the per-step 1e-5 bar, added up),
    step_done [K, B], step_flags [K, B, N], step_pos [K, 3, B N] (x, y [nm] and altitude [ft] after each step: the oracle's own
    per-step record, for event checks) and n_steps.
    The sums and the minimum are taken in the oracle's dtype: a float64 OracleEnv gives the float64-built reference."""
    B, N = orc.B, orc.N
    actions = np.ascontiguousarray(np.asarray(actions, np.float32).reshape(B, N, 3))
    term_before = orc.term_obs.copy()
    states, outs = [], []
    for _ in range(K):
        orc.step(actions)
        states.append(snapshot_state(orc))
        outs.append({k: getattr(orc, k).copy() for k in OUTPUTS})
    done = np.stack([o["done"] for o in outs]).astype(bool)                      # [K, B]
    n = np.where(done.any(axis=0), done.argmax(axis=0) + 1, K).astype(np.int64)     # [B]
    last = n - 1
    env_rows, ac_rows = np.arange(B), np.arange(B * N)
    last_ac = np.repeat(last, N)

    def at_last(name):
        return np.stack([o[name] for o in outs])[last, env_rows]

    rew = np.stack([o["reward"] for o in outs])                                   # [K, B]
    acr = np.stack([o["ac_reward"] for o in outs])                                # [K, B, N]
    executed = np.arange(K)[:, None] < n[None, :]                                 # [K, B]
    flags = np.stack([o["flags"] for o in outs])                                  # [K, B, N]
    res = {
        "n_steps": n.astype(np.uint8),
        "obs": at_last("obs"), "raw_obs": at_last("raw_obs"),
        "reward": f32_sequential_sum(rew, n, orc.dtype), "ac_reward": f32_sequential_sum(acr, n, orc.dtype),
        "reward_scale": np.where(executed, np.maximum(1.0, np.abs(rew.astype(np.float64))), 0.0).sum(axis=0),
        "ac_reward_scale": np.where(executed[:, :, None], np.maximum(1.0, np.abs(acr.astype(np.float64))), 0.0).sum(axis=0),
        "done": done[last, env_rows].astype(np.uint8),
        "flags": np.bitwise_or.reduce(np.where(executed[:, :, None], flags, 0).astype(np.uint16), axis=0),
        "min_sep": np.where(executed, np.stack([o["min_sep"] for o in outs]), np.inf).min(axis=0).astype(orc.dtype),
        "step_done": done, "step_flags": flags,
        "step_pos": np.stack([np.stack([orc._nm(s["px"], 0), orc._nm(s["py"], 1), s["h"]]) for s in states]),
    }
    # the terminal observation is written by the terminating step of envs that are auto-reset in this call; untouched otherwise
    ended = done[last, env_rows]
    res["term_obs"] = np.where(ended[:, None, None], at_last("term_obs"), term_before)
    # state: every env's rows of its step-n snapshot
    for k in STATE:
        stack = np.stack([s[k] for s in states])
        if k == "last_act" and not orc.fixed:      # the float64 instantiation keeps it [3, B N]: the aircraft on the second axis
            orc.last_act[...] = stack[last_ac, :, ac_rows].T
            continue
        getattr(orc, k)[...] = stack[last_ac, ac_rows] if k in PER_AIRCRAFT else stack[last, env_rows]
    for k in OUTPUTS:   # the oracle's output arrays show the call's result, like the product's
        getattr(orc, k)[...] = res[k].reshape(getattr(orc, k).shape)
    return res


def literal_skip(orc1, actions, K):
    """The definition itself on a ONE-env oracle: the loop, nothing batched.  Returns the same keys as skip_reference (outputs)."""
    assert orc1.B == 1
    term_before = orc1.term_obs.copy()
    n = 0
    rews, acrs, flags, seps = [], [], [], []
    while True:
        orc1.step(actions)
        n += 1
        rews.append(orc1.reward.copy()); acrs.append(orc1.ac_reward.copy()); flags.append(orc1.flags.copy()); seps.append(orc1.min_sep.copy())
        if orc1.done[0] or n == K:
            break
    acc, acc_ac = rews[0].astype(np.float32), acrs[0].astype(np.float32)
    for r, a in zip(rews[1:], acrs[1:]):
        acc = (acc + r).astype(np.float32)
        acc_ac = (acc_ac + a).astype(np.float32)
    return {"n_steps": np.array([n], np.uint8), "obs": orc1.obs.copy(), "raw_obs": orc1.raw_obs.copy(), "reward": acc, "ac_reward": acc_ac,
            "done": orc1.done.copy(), "flags": np.bitwise_or.reduce(np.stack(flags), axis=0),
            "min_sep": np.stack(seps).min(axis=0).astype(np.float32),
            "term_obs": orc1.term_obs.copy() if orc1.done[0] else term_before}


def candidate_references(orc, cand, K):
    """The look-ahead call (atc_lookahead) on the oracle: skip_reference per candidate of cand [M, B, N, 3] from a snapshot of the oracle,
    restored after each candidate — the oracle is left as it was.  Returns the M reference dicts."""
    snap = snapshot(orc)
    refs = []
    for m in range(cand.shape[0]):
        refs.append(skip_reference(orc, cand[m], K))
        restore(orc, snap)
    return refs


def plan_chain(orc, plan, K, record=None):
    """The plan call (atc_lookahead_plan) on the oracle for ONE candidate ([H, B, N, 3]): chained skip_reference calls, an env leaving at
    its first done.  The oracle is left wherever the chain ends: the caller restores it.  Returns what bars.check_skip_outputs reads, plus
    seg_reward [H, B] and seg_reward_scale [H, B] (each segment's own bar: that of one frame-skip call).  record: a list that gets one
    (alive [B] before the segment, the segment's skip_reference dict) per segment.  Sums in the oracle's dtype, like skip_reference."""
    B = orc.B
    alive = np.ones(B, bool)
    out = None
    seg = np.zeros((plan.shape[0], B), orc.dtype)
    seg_scale = np.zeros((plan.shape[0], B))
    for h in range(plan.shape[0]):
        r = skip_reference(orc, plan[h], K)
        if record is not None:
            record.append((alive.copy(), r))
        if out is None:
            out = {k: np.array(r[k]).copy() for k in ("obs", "raw_obs", "term_obs", "reward", "ac_reward", "done", "flags", "min_sep",
                                                      "reward_scale", "ac_reward_scale")}
            out["n_steps"] = r["n_steps"].astype(np.int64)
        else:
            a1, a2, a3 = alive, alive[:, None], alive[:, None, None]
            for k, m in (("obs", a3), ("raw_obs", a3), ("term_obs", a3), ("done", a1)):
                out[k] = np.where(m, r[k], out[k])
            out["reward"] = np.where(a1, (out["reward"] + r["reward"]).astype(orc.dtype), out["reward"])
            out["ac_reward"] = np.where(a2, (out["ac_reward"] + r["ac_reward"]).astype(orc.dtype), out["ac_reward"])
            out["reward_scale"] = out["reward_scale"] + np.where(a1, r["reward_scale"], 0.0)
            out["ac_reward_scale"] = out["ac_reward_scale"] + np.where(a2, r["ac_reward_scale"], 0.0)
            out["flags"] = np.where(a2, out["flags"] | r["flags"], out["flags"])
            out["min_sep"] = np.where(a1, np.minimum(out["min_sep"], r["min_sep"]), out["min_sep"])
            out["n_steps"] = out["n_steps"] + np.where(a1, r["n_steps"].astype(np.int64), 0)
        seg[h] = np.where(alive, r["reward"], 0.0)
        seg_scale[h] = np.where(alive, r["reward_scale"], 0.0)
        alive = alive & ~r["done"].astype(bool)
    out["seg_reward"], out["seg_reward_scale"] = seg, seg_scale
    return out


def plan_references(orc, cand, K, records=None):
    """plan_chain per candidate of cand [M, H, B, N, 3] from a snapshot of the oracle, restored after each candidate.  records: a list that
    gets each candidate's plan_chain record."""
    snap = snapshot(orc)
    refs = []
    for m in range(cand.shape[0]):
        rec = [] if records is not None else None
        refs.append(plan_chain(orc, cand[m], K, rec))
        if records is not None:
            records.append(rec)
        restore(orc, snap)
    return refs
