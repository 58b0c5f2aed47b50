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
and the time-limit case asserts that candidates of all three kinds (ended in segment 0, ended before the last segment, ran all H) are among them."""
import functools

import numpy as np
import pytest

import helpers as H
import held_tools as T
import lookahead_policy_ref as R
import policy_ref as P
from atc_hip import layout as L

K = 3
SEED, DECISION0 = 0x1234567890ABCDEF, 0xFFFFFFFE     # (decision0 + h wraps inside every plan of more than two decisions)
BASE = dict(normalize=True, shaping=True, spawn="lattice", timestep_limit=6000)
FULL_OUT = ("seg_reward", "flags", "min_sep", "ac_reward", "obs", "flown", "logp")
FAST_OUT = ("seg_reward", "flown", "logp")
PLAN_KEYS = ("reward", "done", "n_steps", "seg_reward", "flags", "min_sep", "ac_reward", "obs")


def _weights(sampled=True):
    return P.random_weights(np.random.default_rng([17, 1]), 1.0, (-0.5, -1.0, 0.25) if sampled else (-0.5, -1.0, 0.0), False)


def _root(cfg, B, N, ends):
    """the root env, stepped at least once behind reset() so that its bound observation is a normalised one.  ends: the envs are taken apart in
    time — masked resets between the steps — so that under a time limit of 14 a third of them has 2 steps left, a third 8 and a third 13"""
    import torch
    env = H.policy_env(cfg, B, N)
    gen = torch.Generator(device="cpu").manual_seed(5)
    act = lambda: (torch.rand((B, N, 3), generator=gen) * 0.4 - 0.2).to(env.device)      # noqa: E731
    if ends:
        third = torch.arange(B) * 3 // B      # 0: untouched (t = 12), 1: reset behind step 6 (t = 6), 2: reset behind step 11 (t = 1)
        for t in range(12):
            if t == 6:
                env.reset(mask=(third >= 1).to(torch.uint8))
            if t == 11:
                env.reset(mask=(third == 2).to(torch.uint8))
            env.step(act())
    else:
        env.step(act())
    env.synchronize()
    return env


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _case(B, N, M, Hh, with_first, full, deterministic, auto_reset, ends=False):
    """one call and its two oracles, numpy: dict(got, want, plan, clean, n, kinds, max_x)"""
    import torch
    cfg = dict(BASE, auto_reset=auto_reset, timestep_limit=14 if ends else 6000)
    root, child = _root(cfg, B, N, ends), H.policy_env(cfg, M * B, N)
    dev = root.device
    w = torch.as_tensor(_weights(not deterministic), device=dev)
    first = None
    if with_first:
        first = (torch.rand((M, B, N, 3), generator=torch.Generator(device="cpu").manual_seed(9)) * 2.0 - 1.0).to(dev)
    snap = H.snapshot(root)
    bound = {k: getattr(root, k).clone() for k in ("obs", "reward", "done", "flags")}
    obs0 = root.obs.clone()
    got = root.lookahead_policy(w, K, Hh, first=first, M=None if with_first else M, seed=SEED, decision0=DECISION0, deterministic=deterministic,
                                outputs=FULL_OUT if full else FAST_OUT)
    root.synchronize()
    got = _np(got)
    H.bytes_equal(root, snap)      # (asserts: the call wrote no state array)
    for k, v in bound.items():
        assert torch.equal(getattr(root, k), v), "the call wrote the bound tensor %s" % k
    C = M * B
    # ---- oracle 1: the child batch
    if with_first:
        _, r0, d0, info = root.branch(first, K, into=child)
        child.synchronize()
        r0, d0, n0 = r0.cpu().numpy().reshape(C), d0.cpu().numpy().reshape(C).astype(bool), info["frame_steps"].cpu().numpy().reshape(C).astype(np.int64)
        fl0, ob0 = child.flags.cpu().numpy().reshape(C, N).astype(np.uint16), child.obs.cpu().numpy().reshape(C, N * 10)
        x0, D = child.obs.clone(), Hh - 1
    else:
        child.select(root, torch.arange(C, device=dev) % B)
        x0, D = obs0.repeat(M, 1), Hh
    seg = np.zeros((Hh, C), np.float32)
    if D:
        roll = _np(child.rollout_policy(w, D * K, hold=K, seed=SEED, decision0=DECISION0, deterministic=deterministic, obs0=x0.contiguous()))
        child.synchronize()
        f = R.fold(roll["reward"], roll["done"], K, D)
        xs = np.stack([x0.cpu().numpy().reshape(C, N, 10)] + [roll["obs"][b * K - 1].reshape(C, N, 10) for b in range(1, D)])     # what decision b saw
    if with_first:
        cont = ~d0      # candidates the rollout continues
        seg[0] = r0
        n, done, total, flags, obs = n0.copy(), d0.copy(), r0.copy(), fl0.copy(), ob0.copy()
        if D:
            seg[1:] = np.where(cont, f["seg_reward"], np.float32(0.0))
            n += np.where(cont, f["n_steps"], 0)
            done = np.where(cont, f["done"].astype(bool), d0)
            for h in range(1, Hh):
                total = np.where(cont & ((h - 1) * K < f["n_steps"]), (total + seg[h]).astype(np.float32), total)
            flags = np.where(cont[:, None], fl0 | R.or_flags(roll["flags"], f["n_steps"]), fl0)
            obs = np.where(cont[:, None], R.last_rows(roll["obs"], f["n_steps"]), ob0)
        decided = np.maximum(-(-n // K) - 1, 0)      # decisions each candidate took
    else:
        seg, n, done, total = f["seg_reward"], f["n_steps"], f["done"].astype(bool), f["reward"]
        flags, obs = R.or_flags(roll["flags"], n), R.last_rows(roll["obs"], n)
        decided = -(-n // K)
    want = dict(seg_reward=seg.reshape(Hh, M, B).transpose(1, 0, 2), reward=total.reshape(M, B), done=done.reshape(M, B).astype(np.uint8),
                n_steps=n.reshape(M, B), flags=flags.reshape(M, B, N), obs=obs.reshape(M, B, N * 10))
    h0 = 1 if with_first else 0
    flown = np.zeros((M, Hh, B, N, 3), np.float32)
    logp = np.zeros((M, Hh, B, N), np.float32)
    if with_first:
        flown[:, 0] = first.cpu().numpy()
    if D:
        flown[:, h0:] = np.clip(roll["action"], -1.0, 1.0).reshape(D, M, B, N, 3).transpose(1, 0, 2, 3, 4)
        logp[:, h0:] = roll["logp"].reshape(D, M, B, N).transpose(1, 0, 2, 3)
    want.update(flown=flown, logp=logp)
    # ---- which candidates the bit-equality claim covers: the child wavefront of each decision they took saw nothing above 4
    W = H.lane_width(N)
    per = 64 // W
    clean = np.ones(C, bool)
    max_x = 0.0
    if D:
        big = ~(np.abs(xs) <= 4.0)
        dirty_env = big.reshape(D, C, -1).any(axis=2)
        pad = (-C) % per
        dirty_wave = np.pad(dirty_env, ((0, 0), (0, pad))).reshape(D, -1, per).any(axis=2).repeat(per, axis=1)[:, :C]
        took = np.arange(D)[:, None] < decided[None, :]
        clean = ~(dirty_wave & took).any(axis=0)
        max_x = float(np.abs(np.where(took[:, :, None, None], xs, 0.0)).max())
    # ---- oracle 2: the open-loop plan on the flown actions (M <= 64)
    plan = None
    if M <= L.LOOKAHEAD_MAX_M and full:
        plan = _np(root.lookahead_plan(torch.as_tensor(want["flown"], device=dev), K, outputs=("seg_reward", "flags", "min_sep", "ac_reward", "obs")))
        root.synchronize()
    kinds = dict(seg0=(n <= K) & done & (Hh > 1), early=(n <= (Hh - 1) * K) & done, whole=n > (Hh - 1) * K)
    root.close()
    child.close()
    return dict(got=got, want=want, plan=plan, clean=clean.reshape(M, B), n=n.reshape(M, B), kinds={k: v.reshape(M, B) for k, v in kinds.items()}, max_x=max_x,
                auto_reset=auto_reset)


def _compare(r, M, B, N, Hh, with_first):
    got, want, n = r["got"], r["want"], r["n"]
    restrict = r["auto_reset"]      # (the child's rollout steps on through an auto-reset: see PRECONDITION above)
    ok = r["clean"] if restrict else np.ones((M, B), bool)
    assert 2 * ok.sum() >= M * B, "fewer than half of the candidates are covered by the bit-equality claim"
    if not restrict:
        assert r["clean"].all() and r["max_x"] <= 4.0, "precondition: a decision of the oracle saw an observation above 4 (%g)" % r["max_x"]
    print("max |x| a decision saw: %.3g; candidates compared: %d of %d; steps run: %d .. %d" % (r["max_x"], int(ok.sum()), M * B, n.min(), n.max()))
    assert n.min() >= 1
    for k in ("reward", "done", "n_steps"):
        assert np.array_equal(H.bits(got[k].astype(want[k].dtype))[ok], H.bits(want[k])[ok]), k
    assert np.array_equal(H.bits(got["seg_reward"]).transpose(0, 2, 1)[ok], H.bits(want["seg_reward"]).transpose(0, 2, 1)[ok]), "seg_reward"
    ran = (np.arange(Hh)[None, :, None] * K < n[:, None, :]) & ok[:, None, :]           # [M, H, B]: segments run
    pol = ran & (np.arange(Hh)[None, :, None] >= (1 if with_first else 0))
    assert np.array_equal(H.bits(got["flown"])[ran], H.bits(want["flown"])[ran]), "flown"
    assert np.array_equal(H.bits(got["logp"])[pol], H.bits(want["logp"])[pol]), "logp"
    if "flags" in got:
        assert np.array_equal(got["flags"].astype(np.uint16)[ok], want["flags"][ok]), "flags"
        live = ok & ((got["done"] == 0) | (not r["auto_reset"]))       # (behind a look-ahead reset the child env draws another spawn: oracle 2)
        assert np.array_equal(H.bits(got["obs"])[live], H.bits(want["obs"])[live]), "obs"
    if r["plan"] is not None:
        for k in PLAN_KEYS:
            a, b = H.bits(got[k]), H.bits(r["plan"][k])
            if k == "seg_reward":
                a, b = a.transpose(0, 2, 1), b.transpose(0, 2, 1)
            assert np.array_equal(a[ok], b[ok]), "lookahead_plan on the flown actions: %s" % k


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
