"""Developer measurement: what the three per-decision outputs of the collection launch and the two inputs of the bootstrapped advantages
cost.

    python tools/collect_ends_bench.py [--out profiles/collect_ends_bench.json] [--samples 7] [--quick] [--lib VARIANT.so]

On the shapes of tools/rollout_policy_bench.py (8 192 x 16 and 65 536 x 16; T = 64, hold 1 and T = 80, hold 20) and of tools/gae_bench.py
((D, hold) in {(1024, 1), (64, 20)}, NV = 16), in one process, the variants taking turns sample by sample after two warm-up rounds:
  rollout   env.rollout_policy_ends(weights, T, 0, hold) with term_obs, term_flags and control | env.rollout_policy(weights, T, hold)
  gae       env.gae_boot(reward, done, values, boot, trunc) | env.gae(reward, done, values)
Each old call is measured under two names (`policy` / `policy_again`, `gae` / `gae_again`): the ratio of those two medians is the
run-to-run spread the new call's ratio is read against.  `bytes_share` is what the new outputs (inputs) add to the launch's traffic:
D B (N + 2) against T B (42 N + 5) for the rollout (the rare terminal rows left out), 4 D C + D B against 4 (D + 1) C + 8 D C + 5 T B
for the advantages.  No time is fixed in advance: `beyond` marks a row whose ratio exceeds 1 + bytes_share + spread.
A sample is the device time (HIP events) of one call; median, quartiles, min and max.  One JSON file; needs the GPU."""
import benchlib

CONFIGS = ((8192, 16), (65536, 16))
ROLLOUT_RUNS = ((64, 1), (80, 20))      # (T, hold)
GAE_RUNS = ((1024, 1), (64, 20))        # (D, hold)
GAMMA, LAM, DONE_RATE = 0.99, 0.95, 0.02


def _row(res, times, old, new, share, per=1.0, unit="us_per_call"):
    for v in times:
        res[v] = {unit: benchlib.quartiles([t / per for t in times[v]])}
    med = lambda v: res[v][unit]["median"]   # noqa: E731
    res["ratio"] = med(new) / med(old)
    res["spread"] = abs(med(old + "_again") / med(old) - 1.0)
    res["bytes_share"] = share
    res["beyond"] = res["ratio"] > 1.0 + share + res["spread"]
    return res


def measure_rollout(env, T, hold, samples, seed=11):
    import torch
    from atc_hip import policy
    B, N, dev = env.B, env.N, env.device
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 3)).to(dev)
    w = policy.from_torch(net, torch.full((3,), -0.5, device=dev))
    D = T // hold
    out = {"obs": torch.empty((T, B, N * 10), device=dev), "reward": torch.empty((T, B), device=dev),
           "done": torch.empty((T, B), dtype=torch.uint8, device=dev), "flags": torch.empty((T, B, N), dtype=torch.int16, device=dev),
           "action": torch.empty((D, B, N, 3), device=dev), "logp": torch.empty((D, B, N), device=dev)}
    more = dict(out, term_obs=torch.zeros((D, B, N, 10), device=dev), term_flags=torch.empty((D, B), dtype=torch.int16, device=dev),
                control=torch.empty((D, B, N), dtype=torch.uint8, device=dev))
    state = {"dec": 0}

    def run_policy():
        env.rollout_policy(w, T, hold=hold, seed=seed, decision0=state["dec"], out=out)
        state["dec"] += D

    def run_ends():
        env.rollout_policy_ends(w, T, 0, hold=hold, seed=seed, decision0=state["dec"], out=more)
        state["dec"] += D
    calls = {"policy": run_policy, "ends": run_ends, "policy_again": run_policy}
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock, prepare=lambda v: env.reset())
    share = D * B * (N + 2) / (T * B * (42 * N + 5))
    return _row({"B": B, "N": N, "T": T, "hold": hold, "samples": samples}, times, "policy", "ends", share, per=T, unit="us_per_step")


def measure_gae(env, NV, D, hold, samples, seed=11):
    import torch
    B, dev = env.B, env.device
    T = D * hold
    gen = torch.Generator(device=dev).manual_seed(seed + D)
    reward = torch.rand((T, B), device=dev, generator=gen) * 6.0 - 3.0
    done = (torch.rand((T, B), device=dev, generator=gen) < DONE_RATE).to(torch.uint8)
    values = torch.rand((D + 1, B, NV), device=dev, generator=gen) * 6.0 - 3.0
    boot = torch.rand((D, B, NV), device=dev, generator=gen) * 6.0 - 3.0
    trunc = (torch.rand((D, B), device=dev, generator=gen) < 0.5).to(torch.uint8)
    out = {"adv": torch.empty((D, B, NV), device=dev), "ret": torch.empty((D, B, NV), device=dev), "block_reward": torch.empty((D, B), device=dev),
           "block_done": torch.empty((D, B), dtype=torch.uint8, device=dev), "block_steps": torch.empty((D, B), dtype=torch.uint8, device=dev)}
    run_gae = lambda: env.gae(reward, done, values, hold=hold, gamma=GAMMA, lam=LAM, out=out)                       # noqa: E731
    run_boot = lambda: env.gae_boot(reward, done, values, boot, trunc, hold=hold, gamma=GAMMA, lam=LAM, out=out)    # noqa: E731
    calls = {"gae": run_gae, "boot": run_boot, "gae_again": run_gae}
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock)
    C = B * NV
    share = (4 * D * C + D * B) / (4 * (D + 1) * C + 8 * D * C + 5 * T * B)
    return _row({"B": B, "NV": NV, "D": D, "hold": hold, "samples": samples}, times, "gae", "boot", share)


def main():
    ap = benchlib.parser("collect_ends_bench.json", quick="8 192 x 16 only")
    ap.set_defaults(samples=7)
    a = ap.parse_args()
    torch = benchlib.start(a, "collect_ends_bench")
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    rollout_rows, gae_rows = [], []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=11, timestep_limit=6000, sep_nm=0.0)
        for T, hold in ROLLOUT_RUNS:
            r = measure_rollout(env, T, hold, a.samples)
            rollout_rows.append(r)
            print("rollout %6d x %-2d T=%d hold=%-2d  policy %8.3f us/step  ends %8.3f us/step  ratio %.4f  spread %.4f  bytes share %.4f %s" % (
                B, N, T, hold, r["policy"]["us_per_step"]["median"], r["ends"]["us_per_step"]["median"], r["ratio"], r["spread"], r["bytes_share"],
                "BEYOND" if r["beyond"] else ""), flush=True)
            torch.cuda.empty_cache()
        for D, hold in GAE_RUNS:
            r = measure_gae(env, N, D, hold, a.samples)
            gae_rows.append(r)
            print("gae     %6d x %-2d D=%-4d hold=%-2d  gae %9.1f us  boot %9.1f us  ratio %.4f  spread %.4f  bytes share %.4f %s" % (
                B, N, D, hold, r["gae"]["us_per_call"]["median"], r["boot"]["us_per_call"]["median"], r["ratio"], r["spread"], r["bytes_share"],
                "BEYOND" if r["beyond"] else ""), flush=True)
            torch.cuda.empty_cache()
        env.close()
    doc = {"what": "rollout: us per env step of rollout_policy_ends(K = 0, all three outputs) against rollout_policy; gae: us per call of gae_boot against gae",
           "method": "HIP events around one call, variants alternating per sample in one process, 2 warm-up rounds; the old call measured under two names: "
                     "spread = |median ratio of the two - 1|; bytes_share = added bytes / the old call's bytes",
           "expectation": "no time is fixed: beyond marks ratio > 1 + bytes_share + spread",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rollout_rows": rollout_rows, "gae_rows": gae_rows}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
