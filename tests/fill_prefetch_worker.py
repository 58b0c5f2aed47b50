"""Runs the cases of tests/test_fill_prefetch.py in a process of its own and writes their digests as JSON: the test starts it with
ATC_NO_FILL_PREFETCH=1 (the library reads the knob once per process), and calls run_case itself for the prefetching side.
    python fill_prefetch_worker.py OUT.json N:WORKGROUPS:SEED ..."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, "atc-reinforcement-learning_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STEPS = 25
TIME_LIMIT = 10     # steps: every env is auto-reset twice inside a case, and the held launches after a reset read last_action again
GRID_CELL = 0.5
EDGE = 256          # envs at either end of the batch that also go to the oracle


def _digest(t):
    return hashlib.blake2b(t.contiguous().cpu().numpy().tobytes(), digest_size=16).hexdigest()


def actions_for(N, B, seed):
    """The case's ONE action block [B, N, 3]: a twentieth of the speed / altitude components outside the action space."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (B, N, 3)).astype(np.float32)
    wild = rng.uniform(size=(B, N, 3)) < 0.05
    return np.where(wild, a * 4.0, a).astype(np.float32)


def run_case(N, workgroups, seed, keep_edges=False):
    """25 single steps of workgroups * 256 / N envs (N a power of two: every lane an aircraft), the first with a fresh action block,
    the others held.  Returns {"stride", "steps": per-step digests of obs / reward / done / flags, "state": digests of the final
    ac / alt / last_act / env / stats records} and, with keep_edges, the per-step outputs of the first and last EDGE envs."""
    import torch
    from atc_hip import lib
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    assert 256 % N == 0
    B = workgroups * 256 // N
    env = AtcVecEnv(B, N, scenario=scenarios.LOWW(random_entrypoints=True), auto_reset=True, seed=seed, grid_cell=GRID_CELL,
                    timestep_limit=TIME_LIMIT)
    resident, stride = lib.fill_prefetch_info(env.sector, B, N)
    before = lib.launch_counts().get("%d/allv-one" % N, 0)
    a = torch.as_tensor(actions_for(N, B, seed), device=env.device)
    res = {"resident": resident, "stride": stride, "steps": [], "edges": []}
    sel = torch.cat([torch.arange(EDGE), torch.arange(B - EDGE, B)]).to(env.device)
    for t in range(STEPS):
        obs, rew, done, info = env.step(a, held=t > 0)
        res["steps"].append([_digest(obs), _digest(rew), _digest(done), _digest(info["flags"])])
        if keep_edges:
            res["edges"].append(tuple(x[sel].cpu().numpy() for x in (obs, rew, done, info["flags"])))
    res["state"] = [_digest(x) for x in (env.ac, env.alt, env.last_act, env.env, env.stats)]
    res["launches"] = lib.launch_counts().get("%d/allv-one" % N, 0) - before
    if keep_edges:
        res["edge_actions_taken"] = env.actions_taken[sel].cpu().numpy()
    env.close()
    return res


if __name__ == "__main__":
    out = {}
    for spec in sys.argv[2:]:
        N, wg, seed = (int(v) for v in spec.split(":"))
        out[spec] = run_case(N, wg, seed)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f)
