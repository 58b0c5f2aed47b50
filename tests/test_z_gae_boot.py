"""atc_gae_boot on the GPU (include/atc_step.h; AtcVecEnv.gae_boot): atc_gae with the ends the caller marks as truncated bootstrapped from
the value of the terminal state.  Every word against tests/gae_boot_ref.py (the numpy restatement, held to its float64 twin and to
tests/gae_ref.py in tests/test_z_policy_ends.py), over D in {1, 5, 17} x hold in {1, 3, 20} x NV in {1, 3, 64} x B in {1, 70}, both flag
modes and the per-column reward rotating through the cases, random dones and trunc, and a NaN in every boot word that must not be read.
(The module's name sorts it behind the existing test modules on purpose: tests/test_rollout_policy_traffic.py's overlap refusals depend
on where the allocator places that test's buffers next to the env's state arrays, which every GPU test run before it shifts.)"""
import functools
import itertools

import numpy as np
import pytest

import gae_boot_ref as GB
import gae_ref as G

CASES = list(itertools.product((1, 5, 17), (1, 3, 20), (1, 3, 64), (1, 70)))      # (D, hold, NV, B)
KEYS = ("adv", "ret", "block_reward", "block_done", "block_steps")


@functools.lru_cache(maxsize=None)
def _env(B):
    """an env of B: atc_gae_boot reads nothing of it but the device"""
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import model, scenarios
    env = AtcVecEnv(B, 1, sim_parameters=model.SimParameters(1), scenario=scenarios.LOWWDense(), seed=11, grid_cell=0.5)
    env.synchronize()
    return env


@functools.lru_cache(maxsize=None)
def _case(k):
    D, hold, NV, B = CASES[k]
    rng = np.random.default_rng([2025, k])
    T = D * hold
    per_decision, per_column, flat = bool(k & 1), bool(k & 2) and NV > 1, NV == 1 and bool(k & 4)
    cols = (B,) if flat else (B, NV)
    reward = rng.normal(0.0, 50.0, (T, B, NV) if per_column else (T, B)).astype(np.float32)
    done = (rng.random((T, B)) < (0.5 / hold, 0.15, 0.6)[k % 3]).astype(np.uint8)
    values = rng.normal(0.0, 100.0, (D + 1,) + cols).astype(np.float32)
    trunc = (rng.random((D, B)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (D, B)).astype(np.uint8)      # any non-zero byte counts
    boot = rng.normal(0.0, 100.0, (D,) + cols).astype(np.float32)
    term = done.reshape(D, hold, B).any(axis=1)
    read = (term & (trunc != 0)).reshape((D, B) + (1,) * (len(cols) - 1))
    boot = np.where(np.broadcast_to(read, boot.shape), boot, np.float32(np.nan))      # a NaN wherever the word must not be read
    adv_next = rng.normal(0.0, 10.0, cols).astype(np.float32) if k % 3 == 1 else None
    gamma, lam = ((0.99, 0.95), (0.9, 1.0), (1.0, 0.5))[k % 3]
    kw = dict(hold=hold, gamma=gamma, lam=lam, per_decision=per_decision)
    return dict(reward=reward, done=done, values=values, boot=boot, trunc=trunc, adv_next=adv_next, kw=kw, B=B, D=D, hold=hold, read=int(read.sum()),
                ended=int(term.sum()))


def _run(env, c, reward, done, values, boot, trunc, adv_next):
    import torch
    t = lambda a: None if a is None else torch.as_tensor(a, device=env.device)      # noqa: E731
    res = env.gae_boot(t(reward), t(done), t(values), t(boot), t(trunc), adv_next=t(adv_next), **c["kw"])
    env.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)))
def test_every_word_equals_the_restatement(k):
    from atc_hip import lib
    c = _case(k)
    env = _env(c["B"])
    before = lib.launch_records()
    got = _run(env, c, c["reward"], c["done"], c["values"], c["boot"], c["trunc"], c["adv_next"])
    after = lib.launch_records()
    want = GB.gae_boot(c["reward"], c["done"], c["values"], c["boot"], c["trunc"], adv_next=c["adv_next"], **c["kw"])
    for name in KEYS:
        assert got[name].shape == want[name].shape and np.array_equal(G.words(got[name]), G.words(want[name])), (k, name, c["kw"])
    assert np.all(np.isfinite(got["adv"])) and np.all(np.isfinite(got["ret"])), "a boot word that must not be read reached an output"
    moved = {g for g in after if after[g] != before[g]}
    assert moved == {"atc_gae_boot_launch_counts"} and after["atc_gae_boot_launch_counts"]["gae_boot"] == before["atc_gae_boot_launch_counts"].get("gae_boot", 0) + 1


@pytest.mark.gpu
def test_the_cases_contain_what_they_are_meant_to_test():
    cs = [_case(k) for k in range(len(CASES))]
    assert sum(c["read"] > 0 for c in cs) >= 40 and sum(c["ended"] > c["read"] for c in cs) >= 40      # bootstrapped ends, and ends that are not
    assert any(c["kw"]["per_decision"] for c in cs) and any(c["reward"].ndim == 3 for c in cs) and any(c["values"].ndim == 2 for c in cs)
    assert any(c["adv_next"] is not None for c in cs)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 9, 20, 31, 44, 53))
def test_null_null_equals_gae(k):
    import torch
    c = _case(k)
    env = _env(c["B"])
    t = lambda a: None if a is None else torch.as_tensor(a, device=env.device)      # noqa: E731
    a = env.gae_boot(t(c["reward"]), t(c["done"]), t(c["values"]), None, None, adv_next=t(c["adv_next"]), **c["kw"])
    b = env.gae(t(c["reward"]), t(c["done"]), t(c["values"]), adv_next=t(c["adv_next"]), **c["kw"])
    env.synchronize()
    for name in KEYS:
        assert np.array_equal(G.words(a[name].cpu().numpy()), G.words(b[name].cpu().numpy())), (k, name)
    zero = _run(env, c, c["reward"], c["done"], c["values"], c["boot"], np.zeros_like(c["trunc"]), c["adv_next"])      # ... and so does trunc == 0
    for name in KEYS:
        assert np.array_equal(G.words(zero[name]), G.words(b[name].cpu().numpy())), (k, name)
    with pytest.raises(ValueError, match="both or neither"):
        env.gae_boot(t(c["reward"]), t(c["done"]), t(c["values"]), t(c["boot"]), None, **c["kw"])
    with pytest.raises(ValueError, match="both or neither"):
        env.gae_boot(t(c["reward"]), t(c["done"]), t(c["values"]), None, t(c["trunc"]), **c["kw"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", (18, 22, 25, 37, 40, 53))      # D = 5 and 17
def test_the_split_at_half_equals_one_call(k):
    c = _case(k)
    env = _env(c["B"])
    D, hold, h = c["D"], c["hold"], c["D"] // 2
    one = _run(env, c, c["reward"], c["done"], c["values"], c["boot"], c["trunc"], c["adv_next"])
    late = _run(env, c, c["reward"][h * hold:], c["done"][h * hold:], c["values"][h:], c["boot"][h:], c["trunc"][h:], c["adv_next"])
    early = _run(env, c, c["reward"][:h * hold], c["done"][:h * hold], c["values"][:h + 1], c["boot"][:h], c["trunc"][:h], late["adv"][0])
    for name in KEYS:
        assert np.array_equal(G.words(np.concatenate([early[name], late[name]])), G.words(one[name])), (k, name)
