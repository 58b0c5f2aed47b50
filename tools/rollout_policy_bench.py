"""Developer measurement: what the on-policy collection loop costs as one launch (AtcVecEnv.rollout_policy) against the loop it replaces
and against the floor with the policy free.

    python tools/rollout_policy_bench.py [--out profiles/rollout_policy_bench.json] [--samples 7] [--quick] [--lib VARIANT.so]

For 8 192 x 16 and 65 536 x 16, T = 64 steps, hold in {1, 20} (hold 20: T = 80, four decisions), from a reset, normalised observations:
  policy    (a) env.rollout_policy(weights, T, hold) into preallocated buffers: one launch
  torch     (b) the loop it replaces: per decision a torch MLP forward (two addmm + tanh, one addmm), a Gaussian sample and the clamp,
                then `hold` env.step calls (the repeats with held=True) — T step launches plus about eight torch launches per decision;
                observations, rewards, dones and flags are copied into [T, ...] buffers like a collector does
  rollout   (c) env.rollout(actions, hold) on pre-drawn actions: the floor, the policy free
No time is fixed in advance: `rows_slower` lists every row where (a)'s median is above (b)'s.
A sample is the device time (HIP events) of one whole T-step collection; the variants take turns sample by sample after two warm-up
rounds; reported are median, quartiles, min and max in us per env STEP (the collection's time / T) and the env-steps per second of the
median.  Every configuration runs in a child process of its own under a time limit, and nothing is started after one that failed.
One JSON file; needs the GPU."""
import json
import subprocess
import sys

import numpy as np

import benchlib

CONFIGS = ((8192, 16), (65536, 16))
RUNS = ((64, 1), (80, 20))      # (T, hold): T = 64 with a decision per step; hold 20 needs a multiple of 20
CHILD_LIMIT = 240               # seconds per configuration


def measure(B, N, T, hold, samples, seed=11):
    import torch
    from atc_hip import policy
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=seed, timestep_limit=6000, sep_nm=0.0)
    dev = env.device
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 3)).to(dev)
    log_std = torch.full((3,), -0.5, device=dev)
    w = policy.from_torch(net, log_std)
    n_dec = T // hold
    out = {"obs": torch.empty((T, B, N * 10), device=dev), "reward": torch.empty((T, B), device=dev),
           "done": torch.empty((T, B), dtype=torch.uint8, device=dev), "flags": torch.empty((T, B, N), dtype=torch.int16, device=dev),
           "action": torch.empty((n_dec, B, N, 3), device=dev), "logp": torch.empty((n_dec, B, N), device=dev)}
    rbuf = {k: out[k] for k in ("obs", "reward", "done", "flags")}
    actions = torch.as_tensor(benchlib.same_work_actions(np.random.default_rng(seed), (n_dec, B, N)), device=dev)
    sigma = log_std.exp()
    state = {"dec": 0}

    def run_policy():
        env.rollout_policy(w, T, hold=hold, seed=seed, decision0=state["dec"], out=out)
        state["dec"] += n_dec

    def run_torch():
        with torch.no_grad():
            obs = env.obs
            for b in range(n_dec):
                mu = net(obs.view(B * N, 10))
                u = mu + sigma * torch.randn_like(mu)
                out["action"][b].copy_(u.view(B, N, 3))
                out["logp"][b].copy_((-0.5 * ((u - mu) / sigma) ** 2 - log_std).sum(-1).view(B, N) - 2.7568156)
                a = u.clamp(-1.0, 1.0).view(B, N, 3)
                for k in range(hold):
                    obs, rew, done, info = env.step(a, held=k > 0)
                    t = b * hold + k
                    out["obs"][t].copy_(obs)
                    out["reward"][t].copy_(rew)
                    out["done"][t].copy_(done)
                    out["flags"][t].copy_(info["flags"])

    def run_rollout():
        env.rollout(actions, out=rbuf, hold=hold)
    calls = {"policy": run_policy, "torch": run_torch, "rollout": run_rollout}
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock, prepare=lambda v: env.reset())
    res = {"B": B, "N": N, "T": T, "hold": hold, "samples": samples}
    for v in calls:
        q = benchlib.quartiles([t / T for t in times[v]])
        res[v] = {"us_per_step": q, "env_steps_per_s": B / (q["median"] * 1e-6)}
    med = lambda v: res[v]["us_per_step"]["median"]   # noqa: E731
    res["ratio_policy_vs_torch"] = med("policy") / med("torch")
    res["ratio_policy_vs_rollout"] = med("policy") / med("rollout")
    res["slower"] = med("policy") > med("torch")
    res["box"] = benchlib.box(torch)
    env.close()
    return res


def main():
    ap = benchlib.parser("rollout_policy_bench.json", quick="8 192 x 16 only")
    ap.add_argument("--one", nargs=4, type=int, metavar=("B", "N", "T", "HOLD"), help="measure one configuration and print its record (what the tool runs per child)")
    a = ap.parse_args()
    if a.one:
        benchlib.start(a, "rollout_policy_bench")
        print("RECORD " + json.dumps(measure(*a.one, a.samples)), flush=True)
        return
    rows, failed, box = [], None, None
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        for T, hold in RUNS:
            cmd = [sys.executable, __file__, "--one", str(B), str(N), str(T), str(hold), "--samples", str(a.samples)] + (["--lib", a.lib] if a.lib else [])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT)
                rec = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
                if r.returncode != 0 or not rec:
                    failed = {"B": B, "N": N, "T": T, "hold": hold, "returncode": r.returncode, "stderr": r.stderr[-2000:]}
            except subprocess.TimeoutExpired:
                failed = {"B": B, "N": N, "T": T, "hold": hold, "returncode": None, "stderr": "time limit of %d s" % CHILD_LIMIT}
            if failed:       # nothing is started after a failure
                print("FAILED: %s" % failed, flush=True)
                break
            row = json.loads(rec[0][len("RECORD "):])
            box = row.pop("box")
            rows.append(row)
            cell = lambda v: "%8.2f us/step %6.2f G env-steps/s" % (row[v]["us_per_step"]["median"], row[v]["env_steps_per_s"] / 1e9)   # noqa: E731
            print("%6d x %-2d T=%d hold=%-2d  (a) policy %s | (b) torch loop %s | (c) rollout %s  %s" % (
                B, N, T, hold, cell("policy"), cell("torch"), cell("rollout"), "SLOWER than the torch loop" if row["slower"] else ""), flush=True)
        if failed:
            break
    ident = lambda r: {k: r[k] for k in ("B", "N", "T", "hold")}   # noqa: E731
    doc = {"what": "us per env step (a T-step collection's device time / T): rollout_policy | the torch loop it replaces (MLP forward, sample, clamp, env.step per step, "
                   "results copied to [T, ...] buffers) | rollout on pre-drawn actions",
           "method": "HIP events around one whole collection from a reset, variants alternating per sample, 2 warm-up rounds; one child process per configuration",
           "expectation": "no time is fixed: rows_slower lists the rows where rollout_policy's median is above the torch loop's",
           "box": box, "library": a.lib or "in-tree build", "rows": rows, "rows_slower": [ident(r) for r in rows if r["slower"]], "failed": failed}
    benchlib.write_json(a.out, doc)
    if failed:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
