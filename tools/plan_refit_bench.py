"""Developer measurement: what refitting a sampling planner's distribution inside a launch costs and saves.

    python tools/plan_refit_bench.py [--out profiles/plan_refit_bench.json] [--samples 15] [--quick] [--lib VARIANT.so]

For 65 536 x 16 and 4 096 x 64, H in {2, 4}, M in {64, 256, 1024}, mean = the "same work" action family of tools/frame_skip_bench.py,
std = 0.1:
  refit_elites    (a) AtcVecEnv.refit_plans with 0/1 weights, 16 elites per env
  draw_mean_std   (b) the recipe without it: draw_plans(index=elites) [16, H, B, N, 3], then .mean(0) and .std(0)
  refit_dense     (c) AtcVecEnv.refit_plans with dense softmax weights (MPPI)
  draw_weighted   (d) draw_plans(index=None) [M, H, B, N, 3] plus the weighted mean and std in torch — only where that tensor is at most
                      DENSE_LIMIT bytes ("n/a" beyond)
and, for scale, `score`: the atc_lookahead_plan_sampled launch of the same iteration (K = 5, fast form), a few samples.
For every variant: time, and torch.cuda.max_memory_allocated above the start of a call of its own, next to `outputs_bytes` (the two
[H, B, N, 3] results).  `missed` names a row where (a)'s median is above (b)'s slowest sample, or where (a) / (c) allocate more than
their outputs; `rows_slower` lists every row where (a)'s median is above (b)'s median.
A sample is the device time (HIP events) of one call; the variants take turns sample by sample after two warm-up rounds; reported are
median, quartiles, min and max in us per call.  One JSON file; needs the GPU."""
import numpy as np

import benchlib

CONFIGS = ((65536, 16), (4096, 64))
HS = (2, 4)
MS = (64, 256, 1024)
ELITES = 16
STD = 0.1
SCORE_K, SCORE_SAMPLES = 5, 3
DENSE_LIMIT = 16 << 30


def measure(B, N, Hn, M, samples, seed=11):
    import torch
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=seed, timestep_limit=6000, sep_nm=0.0)
    dev = env.device
    rng = np.random.default_rng(seed)
    mean = torch.as_tensor(benchlib.same_work_actions(rng, (Hn, B, N)), device=dev)
    std = torch.full_like(mean, STD)
    gen = torch.Generator(device=dev).manual_seed(seed)
    score = torch.randn((M, B), device=dev, generator=gen)
    elite_idx = score.topk(ELITES, dim=0).indices
    w_elite = torch.zeros_like(score).scatter_(0, elite_idx, 1.0)
    w_dense = torch.exp(score - score.max(0).values)
    key = dict(seed=seed, iteration=0, mean_first=True)
    keep = {}

    def draw_mean_std():
        plans = env.draw_plans(mean, std, M, index=elite_idx, **key)
        keep["r"] = (plans.mean(0), plans.std(0, unbiased=False))

    def draw_weighted():
        plans = env.draw_plans(mean, std, M, **key)
        wn = (w_dense / w_dense.sum(0))[:, None, :, None, None]
        mu = (plans * wn).sum(0)
        keep["r"] = (mu, ((plans - mu) ** 2 * wn).sum(0).sqrt())

    def refit(w):
        def run():
            keep["r"] = env.refit_plans(mean, std, M, w, **key)
        return run
    calls = {"refit_elites": refit(w_elite), "draw_mean_std": draw_mean_std, "refit_dense": refit(w_dense)}
    dense_bytes = M * Hn * B * N * 12
    if dense_bytes <= DENSE_LIMIT:
        calls["draw_weighted"] = draw_weighted
    stream = torch.cuda.current_stream(dev)
    clock = benchlib.hip_clock(torch, stream)
    times = benchlib.sample(calls, samples, 1, clock)
    peak = {}
    for v, fn in calls.items():       # peak memory of one call of each variant, on top of what the env and the inputs hold
        keep.clear()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize(dev)
        peak[v] = int(torch.cuda.max_memory_allocated(dev) - base)
    keep.clear()
    env.reset()
    scoring = benchlib.sample({"score": lambda: env.lookahead_plan_sampled(mean, std, SCORE_K, M, **key)}, SCORE_SAMPLES, 1, clock)
    outputs_bytes = 2 * Hn * B * N * 12
    res = {"B": B, "N": N, "H": Hn, "M": M, "elites": ELITES, "samples": samples, "outputs_bytes": outputs_bytes, "elite_tensor_bytes": ELITES * Hn * B * N * 12,
           "dense_tensor_bytes": dense_bytes, "score_K": SCORE_K, "score": {"us_per_call": benchlib.quartiles(scoring["score"])}}
    for v in ("refit_elites", "draw_mean_std", "refit_dense", "draw_weighted"):
        res[v] = {"us_per_call": benchlib.quartiles(times[v]), "peak_bytes_above_start": peak[v]} if v in times else "n/a"
    a, b = res["refit_elites"]["us_per_call"], res["draw_mean_std"]["us_per_call"]
    res["ratio_refit_elites_vs_draw_mean_std"] = a["median"] / b["median"]
    res["refit_dense_share_of_score"] = res["refit_dense"]["us_per_call"]["median"] / res["score"]["us_per_call"]["median"]
    res["slower"] = a["median"] > b["median"]
    res["missed"] = (["refit_elites above draw_mean_std's slowest sample"] if a["median"] > b["max"] else []) + \
        ["%s allocates more than its outputs" % v for v in ("refit_elites", "refit_dense") if peak[v] > outputs_bytes]
    env.close()
    return res


def main():
    a = benchlib.parser("plan_refit_bench.json", quick="65 536 x 16, H = 2 only").parse_args()
    torch = benchlib.start(a, "plan_refit_bench")
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        for Hn in (HS[:1] if a.quick else HS):
            for M in MS:
                r = measure(B, N, Hn, M, a.samples)
                rows.append(r)
                us = lambda v: "%9.1f" % r[v]["us_per_call"]["median"] if r[v] != "n/a" else "      n/a"   # noqa: E731
                mb = lambda v: "%7.1f" % (r[v]["peak_bytes_above_start"] / 2 ** 20) if r[v] != "n/a" else "    n/a"   # noqa: E731
                b = r["draw_mean_std"]["us_per_call"]
                print("%6d x %-2d H=%d M=%-4d  (a) %s us %s MiB | (b) %s us [%.1f .. %.1f] %s MiB | (c) %s us %s MiB | (d) %s us %s MiB | score %s us  %s"
                      % (B, N, Hn, M, us("refit_elites"), mb("refit_elites"), us("draw_mean_std"), b["min"], b["max"], mb("draw_mean_std"),
                         us("refit_dense"), mb("refit_dense"), us("draw_weighted"), mb("draw_weighted"), us("score"),
                         "MISSED: " + ", ".join(r["missed"]) if r["missed"] else ""), flush=True)
                torch.cuda.empty_cache()
    ident = lambda r: {k: r[k] for k in ("B", "N", "H", "M")}   # noqa: E731
    doc = {"what": "us per call and peak bytes allocated: refit_plans with 16 elites | draw_plans(index=elites) + mean + std | refit_plans with "
                   "dense softmax weights | draw_plans(index=None) + weighted mean and std in torch | the scoring launch, for scale",
           "method": "HIP events around one call, variants alternating per sample, 2 warm-up rounds; peak = torch.cuda.max_memory_allocated above the start of one call",
           "expectation": "refit_elites and refit_dense allocate their two outputs and nothing else; no time is fixed: rows_slower lists the rows "
                          "where refit_elites' median is above draw_mean_std's, rows_missed those above its slowest sample or with more memory",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows,
           "rows_slower": [ident(r) for r in rows if r["slower"]],
           "rows_missed": [dict(ident(r), missed=r["missed"]) for r in rows if r["missed"]]}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
