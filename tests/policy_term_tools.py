"""What tests/test_zz_policy_term.py shares between its cases: the CPU stand-in env of atc_hip.ppo.collect_bootstrap_traffic, and the GPU rig
of atc_rollout_policy_term — one per (W, K), computed once.

THE RIG.  Shapes and configuration are tests/test_z_policy_matrix.py's: N = 1, 2, 3, 5, 9, 17, 33 for W = 1 ... 64, B = one whole 256-lane
workgroup of envs plus a third, T = 12, hold = 3, normalize, shaping, auto-reset, timestep_limit = 4, lattice spawn; aircraft 1 of env 0,
aircraft 0 of the last env and (N > 32) aircraft 32 of env 1 are taken out of control before decision 0.  One thing is added: EVERY aircraft
of env 2 is taken out of control, so that env's episode is won at the run's first step — an end that is no time limit, on a block's first
step, with aircraft not under control at the end, at every width, N = 1 included — and its next episodes end by the time limit at steps 5
(a block's last step) and 10; every other env ends at steps 4 (a middle step) and 9 (a first step).
THE TERMINAL STATES come from envs the call under test never touches: `ref` (auto-reset, traffic=K) replays the stored decisions block by
block through rollout(clamp(action), hold) — the loop the launch replaces —, and before each block its state is copied into `twin`, an env
WITHOUT auto-reset, which flies the block's action one step at a time with observe_traffic() behind every step: where the block's ending step
for an env is step j, the twin's records behind step j are that env's terminal records (nothing has reset it)."""
import numpy as np

import helpers as H
import policy_ends_ref as E
import policy_ref as P
from atc_hip import layout as L

WIDTHS = (1, 2, 4, 8, 16, 32, 64)
KS = (1, 2, 4)
N_OF = {1: 1, 2: 2, 4: 3, 8: 5, 16: 9, 32: 17, 64: 33}
T, HOLD = 12, 3
D = T // HOLD
SEED, DECISION0 = 0x1234567890ABCDEF, 0xFFFFFFFE
CFG = dict(normalize=True, shaping=True, auto_reset=True, timestep_limit=4, spawn="lattice")
LOG_STD = (-0.5, -1.0, 0.25)
SENTINEL = -12345.5
OUT_KEYS = ("obs", "reward", "done", "flags", "action", "logp", "traffic", "term_obs", "term_flags", "control")
_rigs = {}


def batch(W):
    per = 256 // W
    return per + max(1, per // 3)


def make(B, N, traffic=0, auto_reset=True, timestep_limit=4):
    env = H.policy_env(dict(CFG, auto_reset=auto_reset, timestep_limit=timestep_limit), B, N, traffic)
    lo = env.env[:, L.ENV_MASK_LO].clone()
    if N > 1:
        lo[0] &= ~0b10
        lo[B - 1] &= ~0b01
    lo[2] = 0                                     # env 2: nobody under control — won at the first step
    env.env[:, L.ENV_MASK_LO] = lo
    if N > 32:
        env.stats[1, L.STAT_MASK_HI] = 0          # aircraft 32 of env 1: the high mask word
        env.stats[2, L.STAT_MASK_HI] = 0
    env.observe()
    env.synchronize()
    return env


def fresh(env, K, n_dec=D, steps=T, term_traffic=True):
    """out= buffers of one call, the per-decision outputs over sentinels"""
    import torch
    B, N, dev = env.B, env.N, env.device
    out = env._step_rows(steps)
    out.update(action=torch.empty((n_dec, B, N, 3), dtype=torch.float32, device=dev), logp=torch.empty((n_dec, B, N), dtype=torch.float32, device=dev),
               traffic=torch.empty((n_dec, B, N, K, 8), dtype=torch.float32, device=dev),
               term_obs=torch.full((n_dec, B, N, 10), SENTINEL, dtype=torch.float32, device=dev),
               term_flags=torch.full((n_dec, B), 0x5A5A, dtype=torch.int16, device=dev), control=torch.full((n_dec, B, N), 7, dtype=torch.uint8, device=dev))
    if term_traffic:
        out["term_traffic"] = torch.full((n_dec, B, N, K, 8), SENTINEL, dtype=torch.float32, device=dev)
    return out


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _state(env):
    return {k: getattr(env, k).cpu().numpy() for k in H.STATE}


def _terminal_records(ref, twin, action, done, K, chained):
    """want [D, B, N, K, 8] (sentinel where block d of env e has no ending step) from the twin without auto-reset; chained: the twin is put
    into ref's state before every block (ref auto-resets); otherwise the twin flies on its own (the run has no reset).  Also ref's obs [T, ...]."""
    import torch
    B, N = twin.B, twin.N
    t_end = E.ending_steps(done, HOLD)
    want = np.full((D, B, N, K, 8), SENTINEL, np.float32)
    obs = []
    for d in range(D):
        a = action[d:d + 1].clamp(-1.0, 1.0)
        if chained:
            H.restore(twin, H.snapshot(ref))
        for j in range(HOLD):
            twin.rollout(a, hold=1)
            rec = twin.observe_traffic()
            twin.synchronize()
            rec = rec.cpu().numpy().reshape(B, N, K, 8)
            here = t_end[d] == d * HOLD + j
            want[d, here] = rec[here]
        if chained:
            obs.append(ref.rollout(a, hold=HOLD)["obs"].clone())
    return want, (torch.cat(obs).cpu().numpy() if chained else None)


def rig(W, K):
    """numpy results of every run of one (W, K); see the module's text"""
    if (W, K) in _rigs:
        return _rigs[(W, K)]
    import torch
    from atc_hip import lib
    N, B = N_OF[W], batch(W)
    A, twin_ends, ref, twin = make(B, N), make(B, N), make(B, N, traffic=K), make(B, N, traffic=K, auto_reset=False)
    dev = A.device
    w = torch.as_tensor(P.random_weights(np.random.default_rng([17, K]), 1.0, LOG_STD, False, K), device=dev)
    snap, obs0 = H.snapshot(A), A.obs.clone()
    kw = dict(hold=HOLD, seed=SEED, decision0=DECISION0)
    r = dict(B=B, N=N, W=W, K=K)
    # the call, counted
    A.synchronize()
    before = lib.launch_records()
    out = fresh(A, K)
    got = A.rollout_policy_term(w, T, K, obs0=obs0.clone(), out=out, **kw)
    A.synchronize()
    after = lib.launch_records()
    r["same_dict"] = got is out
    r["gained"] = {g: {k: v - before[g].get(k, 0) for k, v in after[g].items() if v != before[g].get(k, 0)} for g in after}
    r["gained"] = {g: v for g, v in r["gained"].items() if v}
    r["full"], r["state"] = _np(got), _state(A)
    # the twin: rollout_policy_ends(traffic=K)
    ends = twin_ends.rollout_policy_ends(w, T, K, obs0=obs0.clone(), out=fresh(twin_ends, K, term_traffic=False), **kw)
    twin_ends.synchronize()
    r["ends"], r["state_ends"] = _np(ends), _state(twin_ends)
    # term_traffic NULL
    H.restore(A, snap)
    null = A.rollout_policy_term(w, T, K, obs0=obs0.clone(), out=fresh(A, K, term_traffic=False), **kw)
    A.synchronize()
    r["null"], r["state_null"] = _np(null), _state(A)
    # two launches of T / 2
    H.restore(A, snap)
    h, whole = T // 2, fresh(A, K)
    part = lambda a, b: {k: v[a:b] for k, v in whole.items()}      # noqa: E731
    first = A.rollout_policy_term(w, h, K, obs0=obs0.clone(), out=dict(part(0, h), **{k: whole[k][:h // HOLD] for k in OUT_KEYS[4:] + ("term_traffic",)}), **kw)
    A.rollout_policy_term(w, h, K, obs0=first["obs"][-1].clone(), out=dict(part(h, T), **{k: whole[k][h // HOLD:] for k in OUT_KEYS[4:] + ("term_traffic",)}),
                          **dict(kw, decision0=(DECISION0 + h // HOLD) & 0xffffffff))
    A.synchronize()
    r["halves"], r["state_halves"] = _np(whole), _state(A)
    # the terminal records, from envs the call never touched
    r["want"], ref_obs = _terminal_records(ref, twin, got["action"], r["full"]["done"], K, True)
    r["ref_obs"] = ref_obs
    # the call without auto-reset, against a twin flying on its own
    A2, twin2 = make(B, N, auto_reset=False), make(B, N, traffic=K, auto_reset=False)
    got2 = A2.rollout_policy_term(w, T, K, obs0=A2.obs.clone(), out=fresh(A2, K), **kw)
    A2.synchronize()
    r["noreset"] = _np(got2)
    r["want_noreset"], _ = _terminal_records(None, twin2, got2["action"], r["noreset"]["done"], K, False)
    for env in (A, twin_ends, ref, twin, A2, twin2):
        env.close()
    _rigs[(W, K)] = r
    return r


def events(r):
    """what the compared blocks of one rig contain, from the call's own per-step arrays (bit-equal to the twins', asserted by the cases)"""
    full, N = r["full"], r["N"]
    done, flags = full["done"], full["flags"].view(np.uint16)
    tf = full["term_flags"].view(np.uint16)
    t_end = E.ending_steps(done, HOLD)
    trunc = E.truncated(tf) != 0
    seen = set()
    for pos, name in ((0, "first"), (1, "middle"), (2, "last")):
        if ((t_end >= 0) & (t_end % HOLD == pos)).any():
            seen.add("an end on a block's %s step" % name)
    if trunc.any():
        seen.add("a pure time-limit end")
    if ((tf != 0) & ~trunc).any():
        seen.add("an end by another cause")
    for d, e in np.argwhere(t_end >= 0):
        out_of_control = (flags[t_end[d, e], e, :N] & (L.F_INACTIVE | L.F_WON)) != 0
        if out_of_control.any():
            seen.add("an aircraft not under control at its end")
        if N > 32 and out_of_control[32:].any() and not out_of_control.all():
            seen.add("the high mask word")
    return seen


# ---------------------------------------------------------------------------------------------------------------- the CPU stand-in
class StandIn:
    """What collect_bootstrap_traffic calls on an env, on the CPU: the rollout returns the arrays given, the value function and gae_boot
    record what they are called with."""
    device = "cpu"

    def __init__(self, B, N, K, stored):
        import torch
        self.torch, self.B, self.N, self.traffic_k, self.stored = torch, B, N, K, stored
        self.obs = stored["obs0"].reshape(B, N * 10)
        self.calls = []

    def rollout_policy_term(self, weights, T_, traffic, hold=1, seed=0, decision0=0, obs0=None):
        self.calls.append(("rollout_policy_term", int(T_), int(traffic), int(hold), int(seed), int(decision0)))
        self.obs0_seen = obs0
        return {k: v for k, v in self.stored.items() if k not in ("obs0", "traffic_final")}

    def observe_traffic(self):
        self.calls.append(("observe_traffic",))
        return self.stored["traffic_final"]

    def gae_boot(self, reward, done, values, boot, trunc, hold=1, gamma=0.99, lam=0.95, *, per_decision=False):
        import gae_boot_ref
        self.calls.append(("gae_boot", hold, gamma, lam, per_decision))
        self.gae_args = dict(reward=reward, done=done, values=values, boot=boot, trunc=trunc)
        res = gae_boot_ref.gae_boot(reward.numpy(), done.numpy(), values.numpy(), boot.numpy(), trunc.numpy(), hold=hold, gamma=gamma, lam=lam, per_decision=per_decision)
        return {k: self.torch.tensor(np.asarray(v)) for k, v in res.items()}


def synthetic(seed, B, N, T_, hold, K):
    """the stored arrays of a collection no env flew, as tensors: ends by several causes in turn, term rows zero where a block did not end"""
    import torch
    rng = np.random.default_rng([73, seed])
    n_dec = T_ // hold
    u = lambda *shape: rng.uniform(-1.0, 1.0, shape).astype(np.float32)      # noqa: E731
    s = {"obs0": u(B, N, 10), "obs": u(T_, B, N * 10), "reward": rng.normal(0.0, 0.5, (T_, B)).astype(np.float32), "done": (rng.random((T_, B)) < 0.25).astype(np.uint8),
         "action": u(n_dec, B, N, 3), "logp": u(n_dec, B, N), "traffic": u(n_dec, B, N, K, 8), "traffic_final": u(B, N, K, 8)}
    ended = s["done"].reshape(n_dec, hold, B).any(axis=1)
    causes = np.array([L.F_TIMEOUT, L.F_TIMEOUT | L.F_OUTSIDE, L.F_TIMEOUT | L.F_WON, L.F_BELOW_MVA, L.F_CONFLICT | L.F_TIMEOUT, L.F_OUTSIDE])
    cause = causes[(np.cumsum(ended.reshape(-1)) - 1).reshape(n_dec, B) % len(causes)]
    s["term_flags"] = np.where(ended, L.TERM_ENDED | cause, 0).astype(np.uint16).view(np.int16)
    s["term_obs"] = np.where(ended[:, :, None, None], u(n_dec, B, N, 10), np.float32(0))
    s["term_traffic"] = np.where(ended[:, :, None, None, None], u(n_dec, B, N, K, 8), np.float32(0))
    s["control"] = (rng.random((n_dec, B, N)) < 0.8).astype(np.uint8)
    return {k: torch.tensor(v) for k, v in s.items()}
