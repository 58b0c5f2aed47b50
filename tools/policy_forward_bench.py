"""Developer measurement: the stand-alone policy forward (AtcVecEnv.policy_forward: the packed policy's decisions on R rows in one launch, the
MLP once per row and S draws behind it, no activation in memory) against the float32 torch recipe it replaces and against its sibling with the
same trunk, the critic's value_forward.

    python tools/policy_forward_bench.py [--out profiles/policy_forward_bench.json] [--samples 7] [--quick] [--lib VARIANT.so]

For R = 4 096 x 16 and 65 536 x 16 rows, K in {0, 4} records per aircraft (input rows of 10 and 38 words), S in {1, 32} samples per row, weights
N(0, 1 / fan_in), inputs uniform in [-1, 1]:
  policy_forward  (a) the call with out= (flown and logp preallocated)
  torch_recipe    (b) under no_grad: input_rows -> atc_hip.policy.to_torch's module -> mean; randn [S, R, 3]; mean + exp(log_std) z; clamp;
                      logp = sum(-0.5 z^2 - log_std) - 1.5 log(2 pi)
  value_forward   (c) the critic on the same (widened) rows with out=: the same trunk, one head row, no draw
A sample is the device time (HIP events) of one call; the variants take turns sample by sample after two warm-up rounds; reported are median,
quartiles, min and max in ms per call, and for each variant torch.cuda.max_memory_allocated over one call above what was allocated before it.
No ratio is fixed in advance: EVERY row is recorded and `rows_slower` lists the rows where the call's range (min .. max) is not below the
torch recipe's.  One JSON file; needs the GPU."""
import math

import benchlib

ROWS = (4096 * 16, 65536 * 16)
KS = (0, 4)
SAMPLES = (1, 32)


def measure(env, R, K, S, samples, seed=11):
    import torch
    from atc_hip import layout as L
    from atc_hip import policy
    dev = env.device
    gen = torch.Generator(device=dev).manual_seed(seed + K)
    n_in = L.policy_in(K)
    scale = lambda o, i: torch.randn((o, i), device=dev, generator=gen) / math.sqrt(i)      # noqa: E731
    w = policy.pack_mlp(scale(64, n_in), torch.zeros(64), scale(64, 64), torch.zeros(64), scale(3, 64), torch.zeros(3), torch.tensor([-0.5, -1.0, 0.0]),
                        device=dev, traffic=K)
    vw = w[:L.value_words(K)].clone()      # a critic with the policy's trunk: its first head row, and one more word as b3
    net, log_std = policy.to_torch(w)
    obs_rows = torch.rand((R, 10), device=dev, generator=gen) * 2.0 - 1.0
    traffic = torch.rand((R, K, 8), device=dev, generator=gen) * 2.0 - 1.0 if K else None
    widen = lambda: policy.input_rows(obs_rows.view(R, 1, 10), traffic.view(R, 1, K, 8)).view(R, n_in) if K else obs_rows      # noqa: E731
    x = widen().contiguous()
    out = {"flown": torch.empty((S, R, 3), device=dev), "logp": torch.empty((S, R), device=dev)}
    values = torch.empty(R, device=dev)
    kept = {}

    def forward():
        env.policy_forward(w, obs_rows, traffic=traffic, samples=S, rows_per_decision=R, seed=seed, out=out)

    def recipe():
        with torch.no_grad():
            mean = net(widen())
            z = torch.randn((S, R, 3), device=dev)
            kept["flown"] = (mean + log_std.exp() * z).clamp(-1.0, 1.0)
            kept["logp"] = (-0.5 * z * z - log_std).sum(-1) - 1.5 * math.log(2.0 * math.pi)

    def critic():
        env.value_forward(vw, x, out=values)
    calls = {"policy_forward": forward, "torch_recipe": recipe, "value_forward": critic}
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock)
    kept.clear()
    res = {"R": R, "K": K, "S": S, "input_words": n_in, "samples": samples}
    for name, fn in calls.items():
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize(dev)
        kept.clear()
        t = [s / 1000.0 for s in times[name]]
        res[name] = {"ms_per_call": benchlib.quartiles(t), "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated(dev) - base)}
    med = lambda n: res[n]["ms_per_call"]["median"]      # noqa: E731
    res["ratio_vs_torch"] = med("policy_forward") / med("torch_recipe")
    res["ratio_vs_value_forward"] = med("policy_forward") / med("value_forward")
    res["ns_per_row"] = med("policy_forward") * 1e6 / R
    res["slower"] = not res["policy_forward"]["ms_per_call"]["max"] < res["torch_recipe"]["ms_per_call"]["min"]
    return res


def main():
    ap = benchlib.parser("policy_forward_bench.json", quick="4 096 x 16 rows only")
    ap.set_defaults(samples=7)
    a = ap.parse_args()
    torch = benchlib.start(a, "policy_forward_bench")
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    env = AtcVecEnv(4, 1, scenario=scenarios.LOWWDense(), auto_reset=True, seed=11)      # (the calls need an env for its device and stream only)
    rows = []
    for R in (ROWS[:1] if a.quick else ROWS):
        for K in KS:
            for S in SAMPLES:
                r = measure(env, R, K, S, a.samples)
                rows.append(r)
                print("R = %8d  K = %d  S = %2d  policy_forward %9.3f ms, %7.1f MB   torch %9.3f ms, %8.1f MB   ratio %.3f   value_forward %9.3f ms  %6.1f ns per row %s" % (
                    R, K, S, r["policy_forward"]["ms_per_call"]["median"], r["policy_forward"]["peak_bytes_above_inputs"] / 1e6,
                    r["torch_recipe"]["ms_per_call"]["median"], r["torch_recipe"]["peak_bytes_above_inputs"] / 1e6, r["ratio_vs_torch"],
                    r["value_forward"]["ms_per_call"]["median"], r["ns_per_row"], "SLOWER" if r["slower"] else ""), flush=True)
                torch.cuda.empty_cache()
    env.close()
    doc = {"what": "ms per call and peak bytes allocated during a call: AtcVecEnv.policy_forward with out= (flown, logp) | the float32 torch recipe under "
                   "no_grad (module forward, randn, mean + std z, clamp, logp) | AtcVecEnv.value_forward on the same rows",
           "method": "HIP events around one call, variants alternating per sample, 2 warm-up rounds; median of `samples` with quartiles, min and max; "
                     "peak = torch.cuda.max_memory_allocated over one further call minus memory_allocated before it",
           "expectation": "no ratio is fixed: every row is recorded, rows_slower lists the rows where the call's range (min .. max) is not below the torch recipe's",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows,
           "rows_slower": [{"R": r["R"], "K": r["K"], "S": r["S"]} for r in rows if r["slower"]]}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
