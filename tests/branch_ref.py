"""References and guarded calls shared by tests/test_branch.py and tests/test_state_select.py.  TEST INFRASTRUCTURE ONLY; importing it
needs no GPU.

  clone_reference   the DEFINITION of atc_branch on the product itself: env.step_skip once per candidate on the env's own state, which
                    is put back afterwards; returns the outputs [M, ...] and the state the call left behind, per candidate
  guarded_branch    atc_branch through ctypes into sentinel-filled state and output tensors with guard rows in front and behind
  sentinel_state    six state tensors of a batch, filled with a byte pattern
  child_of          an AtcVecEnv of M * B envs with the parent's sector and parameters
  fake_state        an atc_state_t of made-up addresses for the refusal tests
  oracle_branch     atc_branch on the CPU oracle (tests/skip_ref.py), candidate by candidate, against a child env at the bars of tests/bars.py"""
import ctypes as C

import helpers as H
from atc_hip import layout as L

GUARD = 2                 # guard envs / rows in front of and behind everything a call writes
SENTINEL = 0x5A           # every byte of an unwritten state row
ROW_STATE = ("ac", "alt", "last_act", "env", "stats")   # the arrays compared bit for bit (phi_wide: saturated aircraft only)


def fake_state(base, B, N, lib):
    """an atc_state_t of made-up, disjoint addresses for B envs of N aircraft, and the first address behind it (never dereferenced: the
    refusal tests' calls are refused before any launch)"""
    sizes = (B * N * 16, B * N * 8, B * N * 16, B * 16, B * 32, B * N * 32)
    ptrs, at = [], base
    for s in sizes:
        ptrs.append(at)
        at += (s + 255) & ~255
    return lib.AtcState(*ptrs), at


def clone_reference(env, actions, K):
    import torch
    M = actions.shape[0]
    snap = H.snapshot(env)
    keep = {k: getattr(env, k).clone() for k in ("obs", "reward", "done", "flags", "ac_reward", "min_sep")}
    fs = env.frame_steps.clone() if env.frame_steps is not None else None
    out = {k: [] for k in ("reward", "done", "n_steps", "flags", "ac_reward", "min_sep", "obs")}
    state = {k: [] for k in H.STATE}
    for m in range(M):
        obs, rew, done, info = env.step_skip(actions[m], K)
        row = {"reward": rew, "done": done, "n_steps": info["frame_steps"], "flags": info["flags"].view(env.B, env.N),
               "ac_reward": info["aircraft_reward"].view(env.B, env.N), "min_sep": info["min_separation"], "obs": obs.view(env.B, -1)}
        for k, v in row.items():
            out[k].append(v.clone())
        for k in H.STATE:
            state[k].append(getattr(env, k).clone())
        H.restore(env, snap)
    for k, v in keep.items():
        getattr(env, k).copy_(v)
    if fs is not None:
        env.frame_steps.copy_(fs)
    return {k: torch.stack(v).cpu() for k, v in out.items()}, {k: torch.cat(v).cpu() for k, v in state.items()}


def sentinel_state(envs, N, device):
    """six state tensors for `envs` envs of N aircraft, every byte SENTINEL"""
    import torch
    shapes = {"ac": ((envs * N, L.AC_WORDS), torch.int32), "alt": ((envs * N,), torch.float64), "last_act": ((envs * N, L.LA_WORDS), torch.int32),
              "env": ((envs, L.ENV_WORDS), torch.int32), "stats": ((envs, L.STAT_WORDS), torch.int32),
              "phi_wide": ((envs * N, L.PHI_WIDE_WORDS), torch.float64)}
    st = {}
    for k, (shape, dt) in shapes.items():
        t = torch.empty(shape, dtype=dt, device=device)
        t.view(torch.uint8).fill_(SENTINEL)
        st[k] = t
    return st


def guarded_branch(env, actions, K, outputs, n_steps=True):
    """Returns (outputs [M, ...] CPU, child state rows of the M * B envs CPU).  Guards checked: output rows and state envs in front of
    and behind what the call owns keep their pattern."""
    import torch
    from atc_hip import lib
    M, B, N = actions.shape[0], env.B, env.N
    shapes = {"reward": ((B,), torch.float32, 7.5), "done": ((B,), torch.uint8, 0xA5), "n_steps": ((B,), torch.uint8, 0xA5),
              "flags": ((B, N), torch.int16, 0x5A5A), "ac_reward": ((B, N), torch.float32, 7.5), "min_sep": ((B,), torch.float32, 7.5),
              "obs": ((B, N * 10), torch.float32, 7.5)}
    want = ("reward", "done") + (("n_steps",) if n_steps else ()) + tuple(outputs)
    buf = {k: torch.full((M + 2 * GUARD,) + shapes[k][0], shapes[k][2], dtype=shapes[k][1], device=env.device) for k in want}
    out = lib.AtcLookaheadOut(*[buf[k][GUARD:].data_ptr() if k in buf else None for k in lib.LOOKAHEAD_FIELDS])
    st = sentinel_state(M * B + 2 * GUARD, N, env.device)
    per = {k: (1 if k in ("env", "stats") else N) for k in H.STATE}
    dst = lib.AtcState(*[st[k][GUARD * per[k]:].data_ptr() for k in lib.STATE_FIELDS])
    a = actions.contiguous()
    lib.check(lib.load().atc_branch(env.sector.handle, B, N, K, M, C.byref(env._state), a.data_ptr(), C.byref(dst), C.byref(out), C.byref(env.params),
                                    torch.cuda.current_stream().cuda_stream))
    env.synchronize()
    res = {}
    for k, t in buf.items():
        g = torch.cat([t[:GUARD], t[GUARD + M:]])
        assert bool((g == torch.full_like(g, shapes[k][2])).all()), "guard rows of %s overwritten" % k
        res[k] = t[GUARD:GUARD + M].cpu()
    rows = {}
    for k, t in st.items():
        g, n = GUARD * per[k], M * B * per[k]
        guard = torch.cat([t[:g], t[g + n:]]).contiguous().view(torch.uint8)
        assert bool((guard == SENTINEL).all()), "guard envs of state array %s overwritten" % k
        rows[k] = t[g:g + n].cpu()
    return res, rows


def saturated(state):
    """[rows] bool: aircraft whose heading or accepted heading target is saturated (their phi_wide row is specified)"""
    phi, la = state["ac"][:, L.AC_PHI], state["last_act"][:, 1]
    return (phi == L.I32_MAX) | (phi == L.I32_MIN) | (la == L.I32_MAX) | (la == L.I32_MIN)


def assert_state_equal(got, ref, tag, env_mask=None, N=1):
    """bit for bit on ac, alt, last_act, env, stats (phi_wide is specified for saturated aircraft only: the callers compare those rows);
    env_mask [envs] bool: the envs compared"""
    import torch
    for k in ROW_STATE:
        g, r = got[k].contiguous().view(torch.uint8).view(got[k].shape[0], -1), ref[k].contiguous().view(torch.uint8).view(ref[k].shape[0], -1)
        if env_mask is not None:
            m = env_mask if k in ("env", "stats") else env_mask.repeat_interleave(N)
            g, r = g[m], r[m]
        assert torch.equal(g, r), (tag, k, int((g != r).any(1).sum()))


def child_of(parent, M, make):
    """make(B) -> an env built like `parent` with B envs; its parameters are made byte-equal to the parent's (mode word included)"""
    child = make(M * parent.B)
    C.memmove(C.byref(child.params), C.byref(parent.params), C.sizeof(parent.params))
    child.refresh_params()
    return child


def oracle_branch(orc, cand, K, ok, check=None):
    """atc_branch on the oracle: for each candidate of cand [M, B, N, 3] skip_ref.skip_reference from a snapshot of the oracle; envs outside
    ok [B] (WIDE at the start: not evaluated) get their SOURCE rows back, so that the oracle then holds what child rows [m B, (m + 1) B) must
    hold; check(m, ref) is called there, and the oracle is restored.  Returns the M reference dicts."""
    import numpy as np
    import skip_ref as R
    snap = R.snapshot(orc)
    refs = []
    for m in range(cand.shape[0]):
        ref = R.skip_reference(orc, cand[m], K)
        for k in R.STATE:
            a, src = getattr(orc, k), snap[0][k]
            rows = np.repeat(~ok, orc.N) if k in R.PER_AIRCRAFT else ~ok
            if k == "last_act" and not orc.fixed:
                a[:, rows] = src[:, rows]
            else:
                a[rows] = src[rows]
        if check:
            check(m, ref)
        refs.append(ref)
        R.restore(orc, snap)
    return refs


def child_check(child, orc, got, half, ok, tag):
    """check(m, ref) for oracle_branch: candidate m's outputs (got: [M, ...] numpy arrays) at the frame-skip bars of tests/bars.py, and child
    rows [m B, (m + 1) B) of the child env's state against the oracle's (bars.check_state: the integer state exact)"""
    import bars
    B, N = orc.B, orc.N

    def check(m, ref):
        bars.check_candidate_outputs({k: v[m] for k, v in got.items()}, ref, ok, half, tag=(tag, m))
        bars.check_state(child, orc, slice(m * B, (m + 1) * B), slice(m * B * N, (m + 1) * B * N))
    return check
