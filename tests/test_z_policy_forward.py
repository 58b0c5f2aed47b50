"""The stand-alone policy forward on the GPU (include/atc_step.h: atc_policy_forward; AtcVecEnv.policy_forward / act; atc_hip.agent.Agent).

Against the float64 restatement (tests/policy_forward_ref.py on tests/policy_ref.py, whose bars are used unchanged): mean within mu_bar,
(action - mean) / sigma within Z_BAR (plus the mean's bar over sigma) of z64 at the restated keys, logp within LOGP_BAR, flown the clamp of
action bit for bit — for R in {1, 63, 64, 65, 257}, K in {0, 1, 2, 4}, S in {1, 3}, P in {R, 7}, on inputs in [-1, 1] and with one
altitude-sized word in a single row (one tile of 64 rows takes the float64 layer).  Rows of a tile without a large input give the same bits
whether or not another tile holds one.
BIT EQUALITY WITH THE ROLLOUT where a rollout wavefront and a forward tile hold the same 64 rows (one aircraft per env: lane = env; 16
aircraft in 16 lanes: lane = env * 16 + aircraft — make_ids in csrc/atc_step.hip): 128 x 1 envs right after reset() for 4 steps (decision 0
sees raw reset observations, the later ones normalised ones), the same without normalisation for 40 steps, and rollout_policy_traffic at
16 x 16 with K = 2.  Everywhere else the claim is the bars above.
act() + step_skip() against rollout_policy(hold = 4) on a twin env; samples; deterministic; out= without an allocation; the launch record;
the refusals; Agent.predict on AtcGym and AtcSBVecEnv; rows beyond R and a NaN row."""
import functools

import numpy as np
import pytest

import helpers as H
import policy_forward_ref as PF
import policy_ref as P
from atc_hip import layout as L

KS = (0, 1, 2, 4)
RS = (1, 63, 64, 65, 257)
SEED, D0 = 0x1234567890ABCDEF, 0xFFFFFFFE      # (the decision counter wraps inside every call of more than two decisions)
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _env():
    from atc_hip.vec_env import AtcVecEnv
    return AtcVecEnv(1, 1)


def _weights(K, seed=7):
    rng = np.random.default_rng([seed, K])
    return P.random_weights(rng, 1.0, tuple(rng.uniform(-1.0, 0.5, 3)), K=K)


def _inputs(R, K, seed, large=None):
    """(obs_rows [R, 10], traffic [R, K, 8] or None) in [-1, 1]; large = (row, word): that word of the own row is 1.5e4"""
    rng = np.random.default_rng([seed, R, K])
    obs = rng.uniform(-1, 1, (R, 10)).astype(np.float32)
    tr = rng.uniform(-1, 1, (R, K, 8)).astype(np.float32) if K else None
    if K:
        tr[:, :, 7] = rng.integers(0, 64, (R, K))      # word 7, the slot: stored, never an input
    if large is not None:
        obs[large[0], large[1]] = 1.5e4
    return obs, tr


def _run(w, obs, tr, **kw):
    import torch
    env = _env()
    dev = env.device
    res = env.policy_forward(torch.as_tensor(w, device=dev), torch.as_tensor(obs, device=dev), traffic=None if tr is None else torch.as_tensor(tr, device=dev), **kw)
    env.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


ALL = ("mean", "action", "flown", "logp")


@pytest.mark.parametrize("K", KS)
def test_against_the_float64_restatement(K):
    w = _weights(K)
    log_std = P.split(w, K)["log_std"].astype(np.float64)
    sigma = np.exp(log_std)
    worst = dict(mean=0.0, z=0.0, logp=0.0)
    for R in RS:
        for large in (None, (R // 2, 2)):
            obs, tr = _inputs(R, K, 3, large)
            x = PF.rows(obs, tr)
            bar, dev32 = P.mu_bar(w, x, K)
            for S in (1, 3):
                for Pr in sorted({R, min(7, R)}):
                    got = _run(w, obs, tr, samples=S, rows_per_decision=Pr, seed=SEED, decision0=D0, outputs=ALL)
                    ref = PF.forward64(w, x, K, SEED, D0, Pr, S)
                    assert got["mean"].shape == (R, 3) and got["action"].shape == got["flown"].shape == (S, R, 3) and got["logp"].shape == (S, R)
                    e_mean = float(np.abs(got["mean"] - ref["mean"]).max())
                    z = (got["action"].astype(np.float64) - got["mean"].astype(np.float64)[None]) / sigma
                    e_z = np.abs(z - ref["z"])
                    e_lp = float(np.abs(got["logp"] - ref["logp"]).max())
                    worst["mean"] = max(worst["mean"], e_mean / bar)
                    worst["z"] = max(worst["z"], float((e_z / (P.Z_BAR + bar / sigma)).max()))
                    worst["logp"] = max(worst["logp"], e_lp / P.LOGP_BAR)
                    tag = (K, R, large, S, Pr)
                    assert e_mean <= bar, (tag, e_mean, bar, dev32)
                    assert np.all(e_z <= P.Z_BAR + bar / sigma), (tag, float(e_z.max()))
                    assert e_lp <= P.LOGP_BAR, (tag, e_lp)
                    assert np.array_equal(H.bits(got["flown"]), H.bits(P.clamp(got["action"]))), tag
                    if S == 3:      # sample 0 is the S = 1 call; the three samples differ
                        assert not np.array_equal(got["action"][0], got["action"][1]) and not np.array_equal(got["action"][1], got["action"][2])
    print("K=%d: largest deviation / bar: mean %.3f, z %.3f, logp %.3f" % (K, worst["mean"], worst["z"], worst["logp"]))


@pytest.mark.parametrize("K", (0, 4))
def test_a_large_input_changes_only_its_own_tile(K):
    w, R = _weights(K), 257
    plain = _run(w, *_inputs(R, K, 4), samples=2, seed=1, outputs=ALL)
    obs, tr = _inputs(R, K, 4, (70, 2))      # tile 1 (rows 64 .. 127) takes the float64 layer
    big = _run(w, obs, tr, samples=2, seed=1, outputs=ALL)
    others = np.r_[0:64, 128:R]
    for k in ALL:
        a, b = (plain[k], big[k]) if k == "mean" else (np.moveaxis(plain[k], 1, 0), np.moveaxis(big[k], 1, 0))
        assert np.array_equal(H.bits(a[others]), H.bits(b[others])), k
    # ... and inside the tile another rounding of the same sums: within the bar, and not the same bits everywhere
    tile = np.r_[64:70, 71:128]
    x = PF.rows(*_inputs(R, K, 4))
    assert np.abs(plain["mean"][tile] - big["mean"][tile]).max() <= 2 * P.mu_bar(w, x, K)[0]
    assert not np.array_equal(plain["mean"][tile], big["mean"][tile])


def _sim(normalize):
    from envs.atc import model
    return model.SimParameters(1, normalize_state=normalize)


@pytest.mark.parametrize("normalize,T", [(True, 4), (False, 40)], ids=["normalised-T4", "raw-T40"])
def test_bit_equal_to_the_rollout_one_aircraft_per_env(normalize, T):
    import torch
    from atc_hip.vec_env import AtcVecEnv
    env = AtcVecEnv(128, 1, sim_parameters=_sim(normalize))
    x0 = env.reset().clone()
    w = torch.as_tensor(_weights(0), device=env.device)
    out = env.rollout_policy(w, T, hold=1, seed=5, decision0=9, obs0=x0)
    env.synchronize()
    if normalize:
        assert not bool(out["done"].any()), "precondition: no episode ends in these steps (every later row is a normalised observation)"
        assert float(x0.abs().max()) > 4.0 and float(out["obs"][:-1].abs().max()) <= 4.0      # decision 0: float64 in both; later: float32 in both
    else:
        assert float(torch.cat([x0[None], out["obs"][:-1]]).view(T, 128, 10).abs().amax(dim=2).min()) > 4.0      # every row: float64 in both
    rows = torch.cat([x0[None], out["obs"][:-1]]).view(T, 128, 1, 10).contiguous()
    got = env.policy_forward(w, rows, rows_per_decision=128, seed=5, decision0=9, outputs=("action", "logp", "flown"))
    env.synchronize()
    assert torch.equal(got["action"][0].view(torch.int32), out["action"].view(torch.int32))
    assert torch.equal(got["logp"][0].view(torch.int32), out["logp"].view(torch.int32))
    assert torch.equal(got["flown"][0], out["action"].clamp(-1.0, 1.0))
    env.close()


def test_bit_equal_to_the_traffic_rollout_at_16_lanes_per_env():
    import torch
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    K, T = 2, 6
    env = AtcVecEnv(16, 16, sim_parameters=_sim(False), scenario=scenarios.LOWWDense())
    x0 = env.reset().clone()
    w = torch.as_tensor(_weights(K), device=env.device)
    out = env.rollout_policy_traffic(w, T, K, hold=1, seed=5, decision0=9, obs0=x0)
    env.synchronize()
    rows = torch.cat([x0[None], out["obs"][:-1]]).view(T, 16, 16, 10).contiguous()
    got = env.policy_forward(w, rows, traffic=out["traffic"], rows_per_decision=256, seed=5, decision0=9, outputs=("action", "logp"))
    env.synchronize()
    assert torch.equal(got["action"][0].view(torch.int32), out["action"].view(torch.int32))
    assert torch.equal(got["logp"][0].view(torch.int32), out["logp"].view(torch.int32))
    env.close()


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "raw"])
def test_act_then_step_skip_is_the_rollouts_block(normalize):
    import torch
    from atc_hip import lib
    from atc_hip.vec_env import AtcVecEnv
    A, Bv = (AtcVecEnv(128, 1, sim_parameters=_sim(normalize)) for _ in range(2))
    for k in H.STATE + ("obs",):
        assert torch.equal(getattr(A, k), getattr(Bv, k)), k
    w = torch.as_tensor(_weights(0), device=A.device)
    before = lib.launch_records()
    flown = A.act(w, seed=3, decision=7)
    A.synchronize()
    after = lib.launch_records()
    gained = {g: {k: v - before[g].get(k, 0) for k, v in after[g].items() if v != before[g].get(k, 0)} for g in after}
    assert {g: v for g, v in gained.items() if v} == {"atc_policy_forward_launch_counts": {0: 1}}      # only the new record moves
    assert tuple(flown.shape) == (128, 1, 3) and float(flown.abs().max()) <= 1.0
    obs, reward, done, _ = A.step_skip(flown, 4)
    ref = Bv.rollout_policy(w, 4, hold=4, seed=3, decision0=7)
    A.synchronize()
    Bv.synchronize()
    assert not bool(ref["done"].any()), "precondition: no episode ends inside the block"
    assert torch.equal(flown.view(torch.int32), ref["action"][0].clamp(-1.0, 1.0).view(torch.int32))
    for k in H.STATE:
        assert torch.equal(getattr(A, k), getattr(Bv, k)), k
    assert torch.equal(obs.view(torch.int32), ref["obs"][-1].view(torch.int32))
    total = ref["reward"][0].clone()
    for t in range(1, 4):
        total = total + ref["reward"][t]
    assert torch.equal(reward.view(torch.int32), total.view(torch.int32)) and not bool(done.any())
    # samples: [0] is the S = 1 call, and all five differ; deterministic: the clamp of the mean, logp = 0
    five = A.act(w, samples=5, seed=3, decision=11)
    one = A.act(w, seed=3, decision=11)
    assert tuple(five.shape) == (5, 128, 1, 3) and torch.equal(five[0], one)
    assert len({five[m].cpu().numpy().tobytes() for m in range(5)}) == 5
    det = A.policy_forward(w, A.obs.view(128, 1, 10), deterministic=True, outputs=("mean", "action", "flown", "logp"))
    assert torch.equal(det["flown"][0], det["mean"].clamp(-1.0, 1.0)) and torch.equal(det["action"][0], det["mean"]) and not bool(det["logp"].any())
    assert torch.equal(A.act(w, deterministic=True), det["flown"][0]) and torch.equal(A.act(w, deterministic=True, seed=99), det["flown"][0])
    # out=: nothing is allocated
    buf, buf5 = torch.empty(128, 1, 3, device=A.device), torch.empty(5, 128, 1, 3, device=A.device)
    outs = {"mean": torch.empty(128, 1, 3, device=A.device), "logp": torch.empty(5, 128, 1, device=A.device), "flown": buf5}
    A.act(w, out=buf)      # (the env keeps the tensors of its LAST call alive: from here on those are the caller's own)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(A.device)
    assert A.act(w, seed=3, decision=11, out=buf) is buf and A.act(w, samples=5, seed=3, decision=11, out=buf5) is buf5
    res = A.policy_forward(w, A.obs.view(128, 1, 10), samples=5, rows_per_decision=128, seed=3, decision0=11, out=outs)
    assert torch.cuda.memory_allocated(A.device) == held
    assert torch.equal(buf, one) and torch.equal(buf5, five) and res["flown"] is buf5 and set(res) == set(outs)
    # the refusals
    with pytest.raises(ValueError, match="traffic"):
        A.act(torch.as_tensor(_weights(2), device=A.device))
    with pytest.raises(RuntimeError, match="overlaps"):
        A.policy_forward(w, A.obs.view(128, 10), out={"mean": A.obs.view(-1)[:384].view(128, 3)})
    A.close()
    Bv.close()


def test_act_refuses_a_discrete_env_and_reads_the_envs_traffic():
    import torch
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import model, scenarios
    env = AtcVecEnv(4, 1, sim_parameters=model.SimParameters(1, discrete_action_space=True))
    with pytest.raises(ValueError, match="discrete"):
        env.act(torch.as_tensor(_weights(0), device=env.device))
    env.close()
    env = AtcVecEnv(8, 4, scenario=scenarios.LOWWDense(), traffic=2)
    w = torch.as_tensor(_weights(2), device=env.device)
    with pytest.raises(ValueError, match="traffic"):
        env.act(torch.as_tensor(_weights(0), device=env.device))
    flown = env.act(w, seed=2, decision=5)
    want = env.policy_forward(w, env.obs.view(8, 4, 10), traffic=env.traffic, rows_per_decision=32, seed=2, decision0=5, outputs=("flown",))["flown"][0]
    assert tuple(flown.shape) == (8, 4, 3) and torch.equal(flown, want)
    env.close()


def test_agent_predict_on_the_gym_and_the_sb_adapter():
    import torch
    from atc_hip.agent import Agent
    from atc_hip.sb_adapter import AtcSBVecEnv
    from envs.atc import atc_gym, scenarios
    host = _env()
    w = _weights(0)
    agent, twin = Agent(w, seed=4), Agent(torch.as_tensor(w), seed=4)
    env = atc_gym.AtcGym()
    obs = env.reset()
    for t in range(20):
        action, state = agent.predict(obs)
        assert state is None and isinstance(action, np.ndarray) and action.shape == (3,) and action.dtype == np.float32
        want = host.policy_forward(agent.weights, torch.as_tensor(np.asarray(obs, np.float32).reshape(1, 10), device=host.device), rows_per_decision=1,
                                   seed=4, decision0=t, outputs=("flown",))["flown"][0, 0].cpu().numpy()
        assert np.array_equal(H.bits(action), H.bits(want)), t
        if t == 0:      # the same observation again: fresh noise; deterministic: repeatable, and the counter stays
            again, _ = twin.predict(obs)
            assert np.array_equal(again, action) and not np.array_equal(twin.predict(obs)[0], action)
            d1, d2 = twin.predict(obs, deterministic=True)[0], twin.predict(obs, deterministic=True)[0]
            assert np.array_equal(d1, d2) and twin.decision == 2
        obs, _, done, _ = env.step(action)
        if done:
            obs = env.reset()
    env.close()
    K, n, N = 2, 8, 4
    wk = _weights(K)
    agent = Agent(wk, seed=6)
    venv = AtcSBVecEnv(n, N, scenario=scenarios.LOWWDense(), traffic=K)
    obs = venv.reset()
    assert obs.shape == (n, N * 10 + N * K * 7)
    for t in range(3):
        actions, _ = agent.predict(obs)
        assert actions.shape == (n, N * 3) and actions.dtype == np.float32
        rec = np.zeros((n, N, K, 8), np.float32)
        rec[..., :7] = obs[:, N * 10:].reshape(n, N, K, 7)
        want = host.policy_forward(agent.weights, torch.as_tensor(obs[:, :N * 10].reshape(n, N, 10).copy(), device=host.device),
                                   traffic=torch.as_tensor(rec, device=host.device), rows_per_decision=n * N, seed=6, decision0=t, outputs=("flown",))["flown"][0]
        assert np.array_equal(H.bits(actions), H.bits(want.reshape(n, N * 3).cpu().numpy())), t
        obs, _, _, _ = venv.step(actions)
    with pytest.raises(ValueError, match="obs"):
        agent.predict(np.zeros((n, N * 10), np.float32))
    venv.close()


@pytest.mark.parametrize("K", (0, 2))
def test_rows_beyond_r_and_a_nan_row(K):
    import torch
    env = _env()
    dev, R, pad = env.device, 65, 192
    w = torch.as_tensor(_weights(K), device=dev)
    obs, tr = _inputs(pad, K, 9)
    kw = dict(samples=2, seed=8, decision0=3, outputs=ALL)

    def run(obs, tr, rows=R):
        o = torch.as_tensor(obs, device=dev)
        t = None if tr is None else torch.as_tensor(tr, device=dev)
        res = env.policy_forward(w, o[:rows], traffic=None if t is None else t[:rows], **kw)
        env.synchronize()
        return {k: v.cpu().numpy() for k, v in res.items()}
    clean = run(obs, tr)
    for poison in (np.nan, np.inf, -np.inf):      # behind row R - 1, in the same buffer: the rest of tile 1 and tile 2
        o2, t2 = obs.copy(), None if tr is None else tr.copy()
        o2[R:] = poison
        if K:
            t2[R:] = poison
        got = run(o2, t2)
        for k in ALL:
            assert np.array_equal(H.bits(got[k]), H.bits(clean[k])), (k, poison)
    # a NaN input row: flown = -1 as the rollout's clamp gives; the other rows of its tile take the float64 layer (within the bar), every
    # other tile keeps its bits
    o2 = obs.copy()
    o2[5, 4] = np.nan
    got = run(o2, tr)
    assert np.all(got["flown"][:, 5] == -1.0) and np.all(np.isnan(got["action"][:, 5])) and np.all(np.isnan(got["mean"][5]))
    assert np.array_equal(H.bits(got["flown"][:, 64:]), H.bits(clean["flown"][:, 64:])) and np.array_equal(H.bits(got["logp"][:, 64:]), H.bits(clean["logp"][:, 64:]))
    rest = np.r_[0:5, 6:64]
    assert np.all(np.isfinite(got["flown"][:, rest])) and np.array_equal(H.bits(got["logp"][:, rest]), H.bits(clean["logp"][:, rest]))      # (logp is the draw's alone)
    bar = P.mu_bar(_weights(K), PF.rows(obs[:R], None if tr is None else tr[:R]), K)[0]
    assert np.abs(got["mean"][rest] - clean["mean"][rest]).max() <= 2 * bar
