"""Developer measurement: candidates continued by the policy inside the launch (AtcVecEnv.lookahead_policy, include/atc_step.h:
atc_lookahead_policy) against the composition of calls it replaces and against the same loop without the MLP.

    python tools/lookahead_policy_bench.py [--out profiles/lookahead_policy_bench.json] [--samples 7] [--quick] [--lib VARIANT.so]

For 4 096 x 16 and 65 536 x 16, M in {8, 32} candidates per env, H = 4 segments of K = 20 steps, first=None (the policy decides every segment),
weights N(0, 1 / fan_in), log_std (-0.5, -1, 0):
  lookahead_policy  (a) the call with out= (seg_reward, flown, logp and the three required outputs preallocated): allocates nothing
  composition       (b) child.select(root, arange(M B) % B) -> child.rollout_policy(w, H K, hold=K, obs0 = root.obs tiled M times) -> the torch
                        fold of its reward / done [T, M B] into seg_reward [H, M B] (cut at the first done).  The child env itself (M B states)
                        exists beforehand and is not counted; what the call allocates — the rollout's [T, ...] streams — is.
                        Skipped, with the size it would need, where those streams pass SKIP_BYTES.
  plan_sampled      (c) lookahead_plan_sampled at the same M, H, K (mean 0, std 0.3): the same loop with a draw where (a) has the MLP
A sample is the device time (HIP events) of one call from a reset of all envs plus one step; the variants take turns sample by sample after two
warm-up rounds; reported are median, quartiles, min and max in ms per call and, for (a) and (b), torch.cuda.max_memory_allocated over one call
above what was allocated before it.  No ratio is fixed in advance: every row is recorded as measured.  One JSON file; needs the GPU."""
import math

import benchlib

CONFIGS = ((4096, 16), (65536, 16))
MS = (8, 32)
H, K = 4, 20
SKIP_BYTES = 48 * 2 ** 30


def measure(B, N, M, samples, seed=11):
    import torch
    from atc_hip import policy
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    make = lambda b: AtcVecEnv(b, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=seed, timestep_limit=6000, sep_nm=0.0, grid_cell=0.5)      # noqa: E731  (one grid for both: select needs byte-equal sectors)
    root = make(B)
    dev = root.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    scale = lambda o, i: torch.randn((o, i), device=dev, generator=gen) / math.sqrt(i)      # noqa: E731
    w = policy.pack_mlp(scale(64, 10), torch.zeros(64), scale(64, 64), torch.zeros(64), scale(3, 64), torch.zeros(3), torch.tensor([-0.5, -1.0, 0.0]), device=dev)
    T, C = H * K, M * B
    stream_bytes = T * C * (N * 40 + N * 2 + 4 + 1) + H * C * N * 16      # obs, flags, reward, done per step; action, logp per decision
    out = {"reward": torch.empty((M, B), device=dev), "done": torch.empty((M, B), dtype=torch.uint8, device=dev),
           "n_steps": torch.empty((M, B), dtype=torch.int16, device=dev), "seg_reward": torch.empty((M, H, B), device=dev),
           "flown": torch.empty((M, H, B, N, 3), device=dev), "logp": torch.empty((M, H, B, N), device=dev)}
    mean = torch.zeros((H, B, N, 3), device=dev)
    first_action = torch.zeros((B, N, 3), device=dev)
    kept = {}
    calls = {"lookahead_policy": lambda: root.lookahead_policy(w, K, H, M=M, seed=seed, decision0=3, out=out),
             "plan_sampled": lambda: root.lookahead_plan_sampled(mean, 0.3, K, M, seed=seed, outputs=("seg_reward",))}
    child = None
    if stream_bytes <= SKIP_BYTES:
        child = make(C)
        index = torch.arange(C, device=dev) % B

        def composition():
            child.select(root, index)
            roll = child.rollout_policy(w, T, hold=K, seed=seed, decision0=3, obs0=root.obs.repeat(M, 1))
            done = roll["done"].bool()
            alive = (done.cumsum(0) - done.int()) == 0      # steps up to and including the first done
            kept["seg_reward"] = (roll["reward"] * alive).view(H, K, C).sum(1)
            kept["n_steps"] = alive.sum(0)
        calls["composition"] = composition

    def prepare(v):
        root.reset()
        root.step(first_action)
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock, prepare)
    kept.clear()
    res = {"B": B, "N": N, "M": M, "H": H, "K": K, "samples": samples, "child_stream_bytes": int(stream_bytes),
           "mean_n_steps": float(out["n_steps"].float().mean())}
    for name in ("lookahead_policy", "composition", "plan_sampled"):
        if name not in calls:
            res[name] = "n/a: the child's per-step streams would take %d bytes" % stream_bytes
            continue
        prepare(name)
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        calls[name]()
        torch.cuda.synchronize(dev)
        kept.clear()
        res[name] = {"ms_per_call": benchlib.quartiles([t / 1000.0 for t in times[name]]), "peak_bytes_above_start": int(torch.cuda.max_memory_allocated(dev) - base)}
    med = lambda n: res[n]["ms_per_call"]["median"]      # noqa: E731
    res["ratio_vs_plan_sampled"] = med("lookahead_policy") / med("plan_sampled")
    res["ratio_vs_composition"] = med("lookahead_policy") / med("composition") if child is not None else "n/a"
    res["us_per_candidate_step"] = med("lookahead_policy") * 1e3 / (M * res["mean_n_steps"]) if res["mean_n_steps"] else "n/a"
    root.close()
    if child is not None:
        child.close()
    return res


def main():
    ap = benchlib.parser("lookahead_policy_bench.json", quick="4 096 x 16 only")
    ap.set_defaults(samples=7)
    a = ap.parse_args()
    torch = benchlib.start(a, "lookahead_policy_bench")
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        for M in MS:
            r = measure(B, N, M, a.samples)
            rows.append(r)
            ms = lambda v: "%9.3f" % r[v]["ms_per_call"]["median"] if isinstance(r[v], dict) else "      n/a"      # noqa: E731
            mem = lambda v: "%d" % r[v]["peak_bytes_above_start"] if isinstance(r[v], dict) else "n/a"      # noqa: E731
            print("%6d x %-2d M=%-2d  lookahead_policy %s ms (+%s B) | composition %s ms (+%s B) | plan_sampled %s ms   mean n_steps %.1f"
                  % (B, N, M, ms("lookahead_policy"), mem("lookahead_policy"), ms("composition"), mem("composition"), ms("plan_sampled"), r["mean_n_steps"]), flush=True)
            torch.cuda.empty_cache()
    doc = {"what": "ms per call: lookahead_policy(out=) | select + rollout_policy on a child of M B envs + torch fold | lookahead_plan_sampled; H = 4, K = 20, first=None",
           "method": "HIP events around one call, variants alternating per sample, 2 warm-up rounds, every sample from a reset of all envs plus one step; "
                     "peak bytes: torch.cuda.max_memory_allocated over one call above the bytes allocated before it",
           "claim": "lookahead_policy with out= allocates nothing where the composition allocates the child's per-step streams; no ratio is fixed in advance",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
