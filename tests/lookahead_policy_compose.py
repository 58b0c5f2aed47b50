"""atc_lookahead_policy's composition oracle (include/atc_step.h; AtcVecEnv.lookahead_policy): one call on a root env and its two oracles made of
existing calls, shared by tests/test_z_lookahead_policy.py and tests/test_z_policy_matrix.py (test files here do not import from each other).

ORACLE 1: the composition on a twin batch of M * B envs (child env m * B + e = candidate m of env e), folded by tests/lookahead_policy_ref.py and
cut at each candidate's first done:
  first=None   child.select(root, arange(M B) % B); child.rollout_policy(w, H K, hold=K, seed, decision0, obs0 = root's observation tiled M times)
  first given  root.branch(first, K, into=child); child.rollout_policy(w, (H - 1) K, hold=K, seed, decision0, obs0 = child.obs); segment 0 is the
               branch's own outputs
ORACLE 2: the open-loop root.lookahead_plan on the flown actions, for min_sep, ac_reward and the observation behind a look-ahead reset.

  root(cfg, B, N, ends)                      the root env, stepped behind its reset
  case(B, N, M, H, with_first, full, ...)    one call and both oracles, numpy (cached)
  compare(r, M, B, N, H, with_first)         the assertions on one case

LAYER 1.  The header claims bit equality where no wavefront of either side sums layer 1 in float64: case() records which child wavefronts (64
consecutive lane slots) saw an input above 4 at a decision, compare() asserts the precondition (layer1="fp32", the default).  normalize=False
with layer1="float64" is the opposite run: every row a decision saw is a raw one, so every wavefront that holds a live lane — on the child batch
and in the candidate tiles, however either is composed — takes the float64 form, where a lane's sum depends on its own row only.
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import helpers as H
import lookahead_policy_ref as R
import policy_ref as P
from atc_hip import layout as L

K = 3
SEED, DECISION0 = 0x1234567890ABCDEF, 0xFFFFFFFE     # (decision0 + h wraps inside every plan of more than two decisions)
BASE = dict(normalize=True, shaping=True, spawn="lattice", timestep_limit=6000)
FULL_OUT = ("seg_reward", "flags", "min_sep", "ac_reward", "obs", "flown", "logp")
FAST_OUT = ("seg_reward", "flown", "logp")
PLAN_KEYS = ("reward", "done", "n_steps", "seg_reward", "flags", "min_sep", "ac_reward", "obs")


def weights(sampled=True):
    return P.random_weights(np.random.default_rng([17, 1]), 1.0, (-0.5, -1.0, 0.25) if sampled else (-0.5, -1.0, 0.0), False)


def root(cfg, B, N, ends):
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


def to_numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def case(B, N, M, Hh, with_first, full, deterministic, auto_reset, ends=False, normalize=True):
    """one call and its two oracles, numpy: dict(got, want, plan, clean, n, kinds, max_x, ...); gained: what the call under test — and nothing
    else — added to the library's launch records; raw_rows: every row a decision of the oracle saw held a word above 4"""
    import torch
    from atc_hip import lib
    cfg = dict(BASE, auto_reset=auto_reset, timestep_limit=14 if ends else 6000, normalize=normalize)
    root_env, child = root(cfg, B, N, ends), H.policy_env(cfg, M * B, N)
    dev = root_env.device
    w = torch.as_tensor(weights(not deterministic), device=dev)
    first = None
    if with_first:
        first = (torch.rand((M, B, N, 3), generator=torch.Generator(device="cpu").manual_seed(9)) * 2.0 - 1.0).to(dev)
    snap = H.snapshot(root_env)
    bound = {k: getattr(root_env, k).clone() for k in ("obs", "reward", "done", "flags")}
    obs0 = root_env.obs.clone()
    root_env.synchronize()
    before = lib.launch_records()
    got = root_env.lookahead_policy(w, K, Hh, first=first, M=None if with_first else M, seed=SEED, decision0=DECISION0, deterministic=deterministic,
                                    outputs=FULL_OUT if full else FAST_OUT)
    root_env.synchronize()
    after = lib.launch_records()
    gained = {g: {k: v - before[g].get(k, 0) for k, v in after[g].items() if v != before[g].get(k, 0)} for g in after}
    got = to_numpy(got)
    H.bytes_equal(root_env, snap)      # (asserts: the call wrote no state array)
    for k, v in bound.items():
        assert torch.equal(getattr(root_env, k), v), "the call wrote the bound tensor %s" % k
    C = M * B
    # ---- oracle 1: the child batch
    if with_first:
        _, r0, d0, info = root_env.branch(first, K, into=child)
        child.synchronize()
        r0, d0, n0 = r0.cpu().numpy().reshape(C), d0.cpu().numpy().reshape(C).astype(bool), info["frame_steps"].cpu().numpy().reshape(C).astype(np.int64)
        fl0, ob0 = child.flags.cpu().numpy().reshape(C, N).astype(np.uint16), child.obs.cpu().numpy().reshape(C, N * 10)
        x0, D = child.obs.clone(), Hh - 1
    else:
        child.select(root_env, torch.arange(C, device=dev) % B)
        x0, D = obs0.repeat(M, 1), Hh
    seg = np.zeros((Hh, C), np.float32)
    if D:
        roll = to_numpy(child.rollout_policy(w, D * K, hold=K, seed=SEED, decision0=DECISION0, deterministic=deterministic, obs0=x0.contiguous()))
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
    raw_rows, n_decided = False, 0
    if D:
        big = ~(np.abs(xs) <= 4.0)
        dirty_env = big.reshape(D, C, -1).any(axis=2)
        pad = (-C) % per
        dirty_wave = np.pad(dirty_env, ((0, 0), (0, pad))).reshape(D, -1, per).any(axis=2).repeat(per, axis=1)[:, :C]
        took = np.arange(D)[:, None] < decided[None, :]
        clean = ~(dirty_wave & took).any(axis=0)
        max_x = float(np.abs(np.where(took[:, :, None, None], xs, 0.0)).max())
        n_decided = int(took.sum())
        raw_rows = bool(big.any(axis=3)[np.broadcast_to(took[:, :, None], big.shape[:3])].all())     # every aircraft row of a decision taken
    # ---- oracle 2: the open-loop plan on the flown actions (M <= 64)
    plan = None
    if M <= L.LOOKAHEAD_MAX_M and full:
        plan = to_numpy(root_env.lookahead_plan(torch.as_tensor(want["flown"], device=dev), K, outputs=("seg_reward", "flags", "min_sep", "ac_reward", "obs")))
        root_env.synchronize()
    kinds = dict(seg0=(n <= K) & done & (Hh > 1), early=(n <= (Hh - 1) * K) & done, whole=n > (Hh - 1) * K)
    root_env.close()
    child.close()
    return dict(got=got, want=want, plan=plan, clean=clean.reshape(M, B), n=n.reshape(M, B), kinds={k: v.reshape(M, B) for k, v in kinds.items()}, max_x=max_x,
                auto_reset=auto_reset, gained={g: v for g, v in gained.items() if v}, raw_rows=raw_rows, n_decided=n_decided)


def compare(r, M, B, N, Hh, with_first, layer1="fp32"):
    got, want, n = r["got"], r["want"], r["n"]
    restrict = r["auto_reset"]      # (the child's rollout steps on through an auto-reset: see PRECONDITION in tests/test_z_lookahead_policy.py)
    ok = r["clean"] if restrict else np.ones((M, B), bool)
    if layer1 == "float64":      # every decision of every candidate on a raw row: no wavefront of either side sums layer 1 in fp32
        assert not restrict and r["n_decided"] > 0 and r["raw_rows"] and r["max_x"] > 4.0, "a decision of the oracle saw a row with no word above 4"
    else:
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
