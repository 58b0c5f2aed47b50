"""atc_lookahead_policy on the GPU (include/atc_step.h; AtcVecEnv.lookahead_policy, atc_hip.shield.policy_shield, atc_hip.ppo.mc_returns):
candidates flown on copies of the state and continued by the packed policy inside the launch.

ORACLE: the composition of existing calls on a twin batch of M * B envs (child env m * B + e = candidate m of env e), folded by
tests/lookahead_policy_ref.py and cut at each candidate's first done:
  first=None   child.select(root, arange(M B) % B); child.rollout_policy(w, H K, hold=K, seed, decision0, obs0 = root's observation tiled M times)
  first given  root.branch(first, K, into=child); child.rollout_policy(w, (H - 1) K, hold=K, seed, decision0, obs0 = child.obs); segment 0 is the
               branch's own outputs
Bit for bit: seg_reward, reward, done, n_steps, flags (OR over the steps run), the last observation (of a candidate that is not done, or without an
auto-reset: the child env m B + e draws another spawn than env e), flown == clamp(the rollout's action), logp == the rollout's.  min_sep and
ac_reward, which no rollout stores, and the observation behind a look-ahead reset come from a SECOND oracle made of an existing call: the open-loop
root.lookahead_plan on the flown actions, every shared output bit for bit.  The root's state rows and bound tensors are byte-identical afterwards.
PRECONDITION, asserted on the oracle's arrays: every observation a decision saw is at most 4 in magnitude (then no wavefront of either side sums
layer 1 in float64) — in full for every case without an auto-reset.  WITH an auto-reset an episode that ends inside the plan (a lost separation
among 16 lattice spawns, the time limit) makes the child's rollout step on through the reset; the raw reset observation switches that child
wavefront at its next decision, and the header claims bit equality only where no wavefront of either side does.  There the comparison is over the
candidates whose child wavefront (64 consecutive lane slots) is clean at every decision they took — at least half of the candidates, asserted —
and the time-limit case asserts that candidates of all three kinds (ended in segment 0, ended before the last segment, ran all H) are among them.
The oracle (one call, both oracles, the comparison) is tests/lookahead_policy_compose.py.  Per-instantiation coverage — every (W, form) this call is compiled for, each against its oracle — lives in tests/test_z_policy_matrix.py."""
import numpy as np
import pytest

import helpers as H
import held_tools as T
import lookahead_policy_compose as LC
import lookahead_policy_ref as R
from atc_hip import layout as L
from lookahead_policy_compose import BASE, DECISION0, FULL_OUT, K, SEED      # noqa: F401  (the oracle's constants are this module's)

# the composition oracle lives in tests/lookahead_policy_compose.py, which tests/test_z_policy_matrix.py shares
_weights, _root, _np, _case, _compare = LC.weights, LC.root, LC.to_numpy, LC.case, LC.compare


# B x N x M: W = 1, 16, 64 — idle lanes at N = 40, five envs in a tile of 256 slots at N = 1
SHAPES = ((5, 1, 8), (3, 16, 5), (2, 40, 3))
GRID = [(B, N, M, Hh, wf) for B, N, M in SHAPES for Hh in (1, 2, 4) for wf in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,M,Hh,with_first", GRID, ids=["%dx%dx%d-H%d-%s" % (g[:4] + ("first" if g[4] else "policy",)) for g in GRID])
def test_equals_the_composition_on_a_child_batch(B, N, M, Hh, with_first):
    # both FULL forms, deterministic on and off, auto_reset on and off: spread over the grid so that every (shape, H, first) meets two of the eight
    for full, det, ar in (((B + Hh) % 2 == 0, with_first, True), ((B + Hh) % 2 == 1, not with_first, False)):
        r = _case(B, N, M, Hh, with_first, full, det, ar)
        _compare(r, M, B, N, Hh, with_first)
        if det:
            assert not r["got"]["logp"].any(), "deterministic: logp = 0"


@pytest.mark.gpu
@pytest.mark.parametrize("full", (False, True))
@pytest.mark.parametrize("with_first", (False, True))
def test_every_form_mode_and_draw_setting_at_one_shape(full, with_first):
    for det in (False, True):
        for ar in (False, True):
            _compare(_case(3, 16, 5, 4, with_first, full, det, ar), 5, 3, 16, 4, with_first)


@pytest.mark.gpu
@pytest.mark.parametrize("with_first", (False, True))
def test_past_one_chunk_of_candidate_tiles(with_first):
    B, N, M = T.look_tiles(16, 9, True), 16, 2      # 9 tiles of 256 slots: one whole chunk of 8, then a partial tile in a padded chunk
    r = _case(B, N, M, 2, with_first, True, False, True)
    _compare(r, M, B, N, 2, with_first)


ENDS = ((12, 16, 3), (3, 40, 3))      # W = 16: four envs to a child wavefront, one third of the envs each; W = 64: a wavefront per env


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,M", ENDS, ids=["%dx%dx%d" % s for s in ENDS])
@pytest.mark.parametrize("with_first", (False, True))
@pytest.mark.parametrize("auto_reset", (False, True))
def test_episodes_end_inside_the_plan(B, N, M, with_first, auto_reset):
    Hh = 4
    r = _case(B, N, M, Hh, with_first, True, False, auto_reset, True)
    ok = r["clean"] if auto_reset else np.ones((M, B), bool)
    counts = {k: int((v & ok).sum()) for k, v in r["kinds"].items()}
    print("candidates that ended in segment 0 / before the last segment / ran all %d segments: %s" % (Hh, counts))
    assert counts["seg0"] > 0 and counts["early"] > counts["seg0"] and counts["whole"] > 0, counts
    _compare(r, M, B, N, Hh, with_first)
    # zeros behind the cut
    seg, n = r["got"]["seg_reward"], r["n"]
    behind = np.arange(Hh)[None, :, None] * K >= n[:, None, :]
    assert behind.any() and not H.bits(seg)[behind].any()


# ---------------------------------------------------------------------------------------------------------------- the other properties
def _env(B=4, N=16, **kw):
    return _root(dict(BASE, auto_reset=True, **kw), B, N, False)


@pytest.mark.gpu
def test_out_allocates_nothing_and_equals_the_cached_call():
    import torch
    env = _env()
    dev, M, Hh, B, N = env.device, 4, 3, env.B, env.N
    w = torch.as_tensor(_weights(), device=dev)
    ref = {k: v.clone() for k, v in env.lookahead_policy(w, K, Hh, M=M, seed=SEED, decision0=7, outputs=FULL_OUT).items()}
    out = {k: torch.full_like(v, 77) for k, v in ref.items()}
    first = env.act(w, samples=M, seed=SEED, decision=3).contiguous()
    for kw in (dict(M=M), dict(first=first)):
        env.lookahead_policy(w, K, Hh, seed=SEED, decision0=7, out=out, **kw)      # (the first call of a kind: caches, module state)
        torch.cuda.synchronize(dev)
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        res = env.lookahead_policy(w, K, Hh, seed=SEED, decision0=7, out=out, **kw)
        torch.cuda.synchronize(dev)
        assert torch.cuda.max_memory_allocated(dev) == before and torch.cuda.memory_allocated(dev) == before, "out= allocated"
        assert all(res[k] is out[k] for k in out)
        if "M" in kw:
            assert H.same_bytes(ref, res)
    env.close()


@pytest.mark.gpu
def test_repeatable_and_seeded_by_decision0():
    import torch
    from atc_hip import lib
    env = _env()
    w = torch.as_tensor(_weights(), device=env.device)
    before = lib.launch_records()
    run = lambda d0: {k: v.clone() for k, v in env.lookahead_policy(w, K, 3, M=4, seed=SEED, decision0=d0, outputs=FULL_OUT).items()}      # noqa: E731
    a, b, c = run(5), run(5), run(6)
    env.synchronize()
    after = lib.launch_records()
    gained = {g: {k: v - before[g].get(k, 0) for k, v in after[g].items() if v != before[g].get(k, 0)} for g in after}
    assert {g: v for g, v in gained.items() if v} == {"atc_lookahead_policy_launch_counts": {16: 3}}
    assert H.same_bytes(a, b), "the same call twice"
    assert not torch.equal(a["flown"], c["flown"]) and not torch.equal(a["logp"], c["logp"]) and not torch.equal(a["seg_reward"], c["seg_reward"])
    # decision0 + 1 in segment h is decision0 in segment h + 1 only by number: the observations differ, the draws' z do not
    env.close()


@pytest.mark.gpu
def test_refusals_on_the_device():
    import ctypes as C
    import torch
    from atc_hip import lib, policy
    env = _env(B=2, N=3)
    dev = env.device
    w = torch.as_tensor(_weights(), device=dev)
    with pytest.raises(ValueError, match="traffic"):
        env.lookahead_policy(torch.zeros(L.policy_words(2), device=dev), K, 2, M=2)
    assert policy.traffic_of(L.policy_words(2)) == 2
    # ranges that only touch are accepted; one byte further is refused; the time increment is the last refusal of all
    M, Hh, B, N = 2, 2, env.B, env.N
    buf = torch.zeros(M * B * 2 + 8, dtype=torch.float32, device=dev)
    out = {"reward": buf[:M * B].view(M, B), "done": torch.zeros((M, B), dtype=torch.uint8, device=dev)}
    out["min_sep"] = buf[M * B:2 * M * B].view(M, B)      # directly behind reward
    env.lookahead_policy(w, K, Hh, M=M, out=out)
    h = lib.load()
    o = lib.AtcLookaheadPolicyOut(*[None] * 10)
    o.reward, o.done, o.min_sep = out["reward"].data_ptr(), out["done"].data_ptr(), out["reward"].data_ptr() + M * B * 4 - 1
    pol = lib.AtcPolicy(w.data_ptr(), 64, 0, 0, 0, 0)
    args = lambda p: (env.sector.handle, B, N, K, Hh, M, C.byref(env._state), env.obs.data_ptr(), None, C.byref(pol), C.byref(o), C.byref(p), None)      # noqa: E731
    assert h.atc_lookahead_policy(*args(env.params)) == -1 and b"out->min_sep overlaps out->reward" in h.atc_last_error()
    slow = lib.AtcParams.from_buffer_copy(bytes(env.params))
    slow.dt = 1e9
    assert h.atc_lookahead_policy(*args(slow)) == -1 and b"overlaps" in h.atc_last_error()      # (the overlap is named first)
    o.min_sep = None
    assert h.atc_lookahead_policy(*args(slow)) == -1 and b"dt too large" in h.atc_last_error()
    env.synchronize()
    env.close()


@pytest.mark.gpu
def test_policy_shield_takes_the_best_candidate_that_is_not_vetoed():
    import torch
    from atc_hip import shield
    # 4 x 16 with M = 4; the envs are taken apart in time under a time limit of 14, so that within the 9 steps of a plan the first two run into
    # the limit whatever they fly — with veto=F_TIMEOUT every candidate of theirs is vetoed — and the last two do not
    env = _root(dict(BASE, auto_reset=True, timestep_limit=14), 4, 16, True)
    w = torch.as_tensor(_weights(), device=env.device)
    snap = H.snapshot(env)
    M, Hh, gamma = 4, 3, 0.9
    seen = set()
    for veto in (L.F_CONFLICT | L.F_BELOW_MVA, L.F_TIMEOUT, L.F_TIMEOUT | L.F_CONFLICT | L.F_BELOW_MVA):
        chosen, index, look = shield.policy_shield(env, w, M, K, Hh, veto=veto, seed=SEED, decision=40, gamma=gamma)
        env.synchronize()
        H.bytes_equal(env, snap)      # (asserts: the shield did not step the env)
        seg = look["seg_reward"].cpu().numpy()
        score = seg[:, 0].copy()
        g = 1.0
        for h in range(1, Hh):
            g = g * gamma
            score = score + seg[:, h] * np.float32(g)      # (torch multiplies a float32 tensor by a python float in float32)
        flags = look["flags"].cpu().numpy().astype(np.int64) & 0xffff
        bad = ((flags & veto) != 0).any(axis=2) | (look["n_steps"].cpu().numpy() == 0)
        want = np.where(bad.all(axis=0), score.argmax(axis=0), np.where(bad, -np.inf, score).argmax(axis=0))
        assert np.array_equal(index.cpu().numpy(), want), (veto, index, want)
        cand = look["first"].cpu().numpy().reshape(M, env.B, env.N, 3)
        assert np.array_equal(chosen.cpu().numpy(), cand[want, np.arange(env.B)])
        assert tuple(chosen.shape) == (env.B, env.N, 3) and np.abs(chosen.cpu().numpy()).max() <= 1.0
        seen |= {"all vetoed" if c else "one stands" for c in bad.all(axis=0)} | ({"some vetoed"} if (bad.any(axis=0) & ~bad.all(axis=0)).any() else set())
    print("shield cases met:", sorted(seen))
    assert {"all vetoed", "one stands"} <= seen
    env.close()


@pytest.mark.gpu
def test_mc_returns_is_the_mean_of_the_discounted_fold():
    import torch
    from atc_hip import ppo
    B, N, M, Hh, gamma = 4, 16, 8, 3, 0.95
    cfg = dict(BASE, auto_reset=True)
    env, child = _root(cfg, B, N, False), H.policy_env(cfg, M * B, N)
    w = torch.as_tensor(_weights(), device=env.device)
    got = ppo.mc_returns(env, w, M, K, Hh, gamma, seed=SEED, decision0=11).cpu().numpy()
    child.select(env, torch.arange(M * B, device=env.device) % B)
    roll = _np(child.rollout_policy(w, Hh * K, hold=K, seed=SEED, decision0=11, obs0=env.obs.repeat(M, 1).contiguous()))
    seg = R.fold(roll["reward"], roll["done"], K, Hh)["seg_reward"].reshape(Hh, M, B)
    disc = R.discounted(seg.transpose(1, 0, 2), gamma)      # float64 [M, B]
    want = disc.mean(axis=0)
    # float32: each candidate's H-term discounted sum, then a mean of M terms — (H + M) roundings of at most eps / 2 relative to the running sums
    mag = (np.abs(seg.astype(np.float64)) * (gamma ** np.arange(Hh))[:, None, None]).sum(axis=0).mean(axis=0)
    bar = (Hh + M) * float(np.finfo(np.float32).eps) * mag
    print("mc_returns: max deviation %.3g, bar %.3g" % (float(np.abs(got - want).max()), float(bar.min())))
    assert got.shape == (B,) and np.all(np.abs(got - want) <= bar)
    env.close()
    child.close()
