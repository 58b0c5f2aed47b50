"""atc_hip.ppo.collect_bootstrap on the GPU, 5 x 3: the collection that bootstraps time-limit ends equals its calls written out by hand —
rollout_policy_ends, the rows, ONE value forward over 2 D + 1 rows, truncated(), gae_boot — and collect() itself is as before.
(The module's name sorts it behind the existing test modules on purpose: tests/test_rollout_policy_traffic.py's overlap refusals depend
on where the allocator places that test's buffers next to the env's state arrays, which every GPU test run before it shifts.)"""
import numpy as np
import pytest

import helpers as H
import policy_ref as P

B, N, T, HOLD = 5, 3, 30, 3
CFG = dict(normalize=True, shaping=True, auto_reset=True, timestep_limit=7, spawn="lattice")


def _value_fn(calls):
    def value_fn(x):
        calls.append(tuple(x.shape))
        return (x * x.new_tensor(np.linspace(-1.0, 1.0, 10))).sum(dim=-1) * 30.0 + 5.0      # [rows, B, N]: a per-aircraft critic
    return value_fn


@pytest.mark.gpu
def test_collect_bootstrap_equals_the_five_calls_by_hand():
    import torch
    from atc_hip import lib, ppo
    A, Bv = H.policy_env(CFG, B, N), H.policy_env(CFG, B, N)
    w = torch.as_tensor(P.random_weights(np.random.default_rng(3)), device=A.device)
    D = T // HOLD
    calls = []
    before = lib.launch_records()
    res = ppo.collect_bootstrap(A, w, _value_fn(calls), T, hold=HOLD, gamma=0.98, lam=0.9, seed=77, decision0=5)
    A.synchronize()
    after = lib.launch_records()
    assert calls == [(2 * D + 1, B, N, 10)], calls          # exactly one forward, with 2 D + 1 rows
    moved = {g for g in after if after[g] != before[g]}
    assert moved == {"atc_rollout_policy_ends_launch_counts", "atc_gae_boot_launch_counts"}, moved
    # by hand
    x0 = Bv.obs.clone()
    out = Bv.rollout_policy_ends(w, T, 0, hold=HOLD, seed=77, decision0=5, obs0=x0)                                 # 1
    rows = torch.cat([ppo.value_rows(Bv, out, x0, hold=HOLD), out["term_obs"].reshape(D, B, N, 10)], dim=0)       # 2
    v = _value_fn([])(rows).to(torch.float32).contiguous()                                                         # 3
    values, boot = v[:D + 1].contiguous(), v[D + 1:].contiguous()
    trunc = ppo.truncated(out["term_flags"])                                                                       # 4
    hand = Bv.gae_boot(out["reward"], out["done"], values, boot, trunc, hold=HOLD, gamma=0.98, lam=0.9)            # 5
    Bv.synchronize()
    hand = dict(out, values=values, boot=boot, trunc=trunc, **hand)
    assert set(res) == set(hand) >= {"term_obs", "term_flags", "control", "boot", "trunc", "adv", "ret", "values"}
    for k in hand:
        assert torch.equal(res[k].contiguous().view(torch.uint8), hand[k].contiguous().view(torch.uint8)), k
    tf = out["term_flags"].cpu().numpy().view(np.uint16)
    assert np.array_equal(trunc.cpu().numpy(), (((tf & 8) != 0) & ((tf & (1 | 2 | 64)) == 0)).astype(np.uint8)) and trunc.dtype == torch.uint8
    assert trunc.any(), "no time-limit end in the collection: nothing was bootstrapped"
    # a bootstrapped end differs from the terminal treatment, exactly where trunc is set and the value of the terminal state is not zero
    plain = Bv.gae(out["reward"], out["done"], values, hold=HOLD, gamma=0.98, lam=0.9)
    differs = (plain["adv"] != hand["adv"]).any(dim=-1)
    assert differs.any() and not (differs & (trunc == 0) & (hand["block_done"] != 0)).any()
    A.close()
    Bv.close()


@pytest.mark.gpu
def test_collect_is_as_before_and_traffic_is_refused():
    import torch
    from atc_hip import lib, ppo
    A, Bv = H.policy_env(CFG, B, N), H.policy_env(CFG, B, N)
    w = torch.as_tensor(P.random_weights(np.random.default_rng(3)), device=A.device)
    D = T // HOLD
    calls = []
    before = lib.launch_records()
    res = ppo.collect(A, w, _value_fn(calls), T, hold=HOLD, seed=77)
    A.synchronize()
    after = lib.launch_records()
    assert calls == [(D + 1, B, N, 10)]
    assert {g for g in after if after[g] != before[g]} == {"atc_rollout_policy_launch_counts", "atc_gae_launch_counts"}
    assert not {"term_obs", "term_flags", "control", "boot", "trunc"} & set(res)
    x0 = Bv.obs.clone()
    out = Bv.rollout_policy(w, T, hold=HOLD, seed=77, obs0=x0)
    values = _value_fn([])(ppo.value_rows(Bv, out, x0, hold=HOLD)).to(torch.float32).contiguous()
    hand = dict(out, values=values, **Bv.gae(out["reward"], out["done"], values, hold=HOLD))
    Bv.synchronize()
    assert set(res) == set(hand)
    for k in hand:
        assert torch.equal(res[k].contiguous().view(torch.uint8), hand[k].contiguous().view(torch.uint8)), k
    with pytest.raises(ValueError, match="traffic"):
        ppo.collect_bootstrap(A, w, _value_fn(calls), T, hold=HOLD, traffic=2)
    assert len(calls) == 1
    A.close()
    Bv.close()
