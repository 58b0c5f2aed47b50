"""Developer measurement: what the on-policy collection loop of a TRAFFIC-AWARE policy costs as one launch (AtcVecEnv.rollout_policy_traffic)
against the loop it replaces and against the same launch without the traffic input.

    python tools/rollout_policy_traffic_bench.py [--out profiles/rollout_policy_traffic_bench.json] [--samples 7] [--quick] [--lib VARIANT.so]

For 8 192 x 16 and 65 536 x 16, T = 64 steps, hold in {1, 20} (hold 20: T = 80, four decisions), K = 4 records, from a reset, normalised
observations (the shapes and rows of tools/rollout_policy_bench.py):
  traffic   (a) env.rollout_policy_traffic(weights, T, 4, hold) into preallocated buffers: one launch
  torch     (b) the loop it replaces: per decision observe_traffic(), torch.cat of the own row and words 0..6 of the records, a torch MLP
                forward (38 -> 64 -> 64 -> 3), a Gaussian sample and the clamp, then `hold` env.step calls (the repeats with held=True);
                observations, rewards, dones, flags and the records are copied into [T, ...] buffers like a collector does
  policy    (c) env.rollout_policy(weights10, T, hold): the launch without the traffic input, i.e. what the traffic input costs
The acceptance condition is (a) < (b) in every row with the quartile ranges disjoint: `rows_slower` lists every row where it does not
hold.  There is no bar on (a) / (c): the ratio is written down.
A sample is the device time (HIP events) of one whole T-step collection; the variants take turns sample by sample after two warm-up
rounds; reported are median, quartiles, min and max in us per env STEP (the collection's time / T) and the env-steps per second of the
median.  Every configuration runs in a child process of its own under a time limit, and nothing is started after one that failed.
One JSON file; needs the GPU."""
import json
import subprocess
import sys

import benchlib

CONFIGS = ((8192, 16), (65536, 16))
RUNS = ((64, 1), (80, 20))      # (T, hold): T = 64 with a decision per step; hold 20 needs a multiple of 20
K = 4
CHILD_LIMIT = 240               # seconds per configuration


def measure(B, N, T, hold, samples, seed=11):
    import torch
    from atc_hip import layout as L
    from atc_hip import policy
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    # (b) needs the env's own traffic observation; (a) and (c) neither read nor write it
    env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=seed, timestep_limit=6000, sep_nm=0.0, traffic=K)
    dev = env.device
    torch.manual_seed(seed)
    mlp = lambda n_in: torch.nn.Sequential(torch.nn.Linear(n_in, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 3)).to(dev)   # noqa: E731
    net, net10 = mlp(L.policy_in(K)), mlp(L.POLICY_IN)
    log_std = torch.full((3,), -0.5, device=dev)
    w, w10 = policy.from_torch(net, log_std, traffic=K), policy.from_torch(net10, log_std)
    n_dec = T // hold
    out = {"obs": torch.empty((T, B, N * 10), device=dev), "reward": torch.empty((T, B), device=dev),
           "done": torch.empty((T, B), dtype=torch.uint8, device=dev), "flags": torch.empty((T, B, N), dtype=torch.int16, device=dev),
           "action": torch.empty((n_dec, B, N, 3), device=dev), "logp": torch.empty((n_dec, B, N), device=dev),
           "traffic": torch.empty((n_dec, B, N, K, 8), device=dev)}
    out10 = {k: v for k, v in out.items() if k != "traffic"}
    sigma = log_std.exp()
    state = {"dec": 0}

    def run_traffic():
        env.rollout_policy_traffic(w, T, K, hold=hold, seed=seed, decision0=state["dec"], out=out)
        state["dec"] += n_dec

    def run_torch():
        with torch.no_grad():
            obs = env.obs
            for b in range(n_dec):
                tr = env.observe_traffic() if b else env.traffic      # (reset and step leave the records of the state they leave)
                out["traffic"][b].copy_(tr)
                x = torch.cat([obs.view(B * N, 10), tr[..., :7].reshape(B * N, 7 * K)], dim=1)
                mu = net(x)
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

    def run_policy():
        env.rollout_policy(w10, T, hold=hold, seed=seed, decision0=state["dec"], out=out10)
    calls = {"traffic": run_traffic, "torch": run_torch, "policy": run_policy}
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock, prepare=lambda v: env.reset())
    res = {"B": B, "N": N, "T": T, "hold": hold, "K": K, "samples": samples}
    for v in calls:
        q = benchlib.quartiles([t / T for t in times[v]])
        res[v] = {"us_per_step": q, "env_steps_per_s": B / (q["median"] * 1e-6)}
    us = lambda v: res[v]["us_per_step"]   # noqa: E731
    res["ratio_traffic_vs_torch"] = us("traffic")["median"] / us("torch")["median"]
    res["ratio_traffic_vs_policy"] = us("traffic")["median"] / us("policy")["median"]
    # the acceptance condition: (a) below (b), the quartile ranges disjoint
    res["slower"] = not (us("traffic")["median"] < us("torch")["median"] and us("traffic")["q3"] < us("torch")["q1"])
    res["box"] = benchlib.box(torch)
    env.close()
    return res


def main():
    ap = benchlib.parser("rollout_policy_traffic_bench.json", quick="8 192 x 16 only")
    ap.add_argument("--one", nargs=4, type=int, metavar=("B", "N", "T", "HOLD"), help="measure one configuration and print its record (what the tool runs per child)")
    a = ap.parse_args()
    if a.one:
        benchlib.start(a, "rollout_policy_traffic_bench")
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
            print("%6d x %-2d T=%d hold=%-2d K=%d  (a) traffic %s | (b) torch loop %s | (c) no traffic %s  (a)/(c) %.2f  %s" % (
                B, N, T, hold, K, cell("traffic"), cell("torch"), cell("policy"), row["ratio_traffic_vs_policy"],
                "NOT below the torch loop with disjoint quartiles" if row["slower"] else ""), flush=True)
        if failed:
            break
    ident = lambda r: {k: r[k] for k in ("B", "N", "T", "hold")}   # noqa: E731
    doc = {"what": "us per env step (a T-step collection's device time / T), K = 4: rollout_policy_traffic | the torch loop it replaces (observe_traffic, cat, MLP forward, "
                   "sample, clamp, env.step per step, results copied to [T, ...] buffers) | rollout_policy without the traffic input",
           "method": "HIP events around one whole collection from a reset, variants alternating per sample, 2 warm-up rounds; one child process per configuration",
           "expectation": "rollout_policy_traffic below the torch loop in every row, quartile ranges disjoint: rows_slower lists the rows where that does not hold; "
                          "no bar on the ratio to rollout_policy (the fmaf ratio alone is 1.36 for K = 4)",
           "box": box, "library": a.lib or "in-tree build", "rows": rows, "rows_slower": [ident(r) for r in rows if r["slower"]], "failed": failed}
    benchlib.write_json(a.out, doc)
    if failed:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
