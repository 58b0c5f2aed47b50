"""Developer measurement: what drawing a plan query's candidates inside the launch costs and saves.

    python tools/plan_sampled_bench.py [--out profiles/plan_sampled_bench.json] [--samples 15] [--quick] [--lib VARIANT.so]

For 65 536 x 16 and 4 096 x 64, K in {5, 20}, H in {2, 4}, M in {8, 64} (at 4 096 x 64 also M = 512, where the tensor route cannot go:
"n/a"), mean = the "same work" action family of tools/frame_skip_bench.py, std = 0.1 (climbing, slowing targets, the default time limit,
a separation minimum of 0: almost no episode ends, every variant executes M x H x K steps per env), fast form (seg_reward only), every
sample started from a reset of all envs plus one step:
  sampled         (a) atc_lookahead_plan_sampled
  randn_plan      (b) the recipe without it: (mean + std * torch.randn(M, H, B, N, 3)).clamp(-1, 1), then atc_lookahead_plan
  plan            (c) atc_lookahead_plan alone on a tensor made beforehand (the same kernel work as (a), minus the draw, plus the load)
The expectation is sampled <= randn_plan in every row, no margin, and sampled within plan's own sample spread (<= the max of its samples);
`ratio_*` holds median / median and `rows_missed` lists every (row, comparison) that misses.  torch.cuda.max_memory_allocated is
recorded for (a) and (b), each over a call of its own.
A sample is the device time (HIP events) of one call; the variants take turns sample by sample after two warm-up rounds; reported are
median, quartiles, min and max in us per call.  One JSON file; needs the GPU."""
import ctypes as C

import numpy as np

import benchlib

CONFIGS = ((65536, 16), (4096, 64))
KS = (5, 20)
HS = (2, 4)
MS = (8, 64)
M_BEYOND = 512      # 4 096 x 64 only: more candidates than atc_lookahead_plan takes
STD = 0.1


def verdict(row):
    """{"ratio_<a>_vs_<b>": median / median} of a measured row, and the names of the comparisons it misses"""
    out, missed = {}, []
    a = row["sampled"]["us_per_call"]
    for other in ("randn_plan", "plan"):
        if row[other] == "n/a":
            out["ratio_sampled_vs_%s" % other] = "n/a"
            continue
        out["ratio_sampled_vs_%s" % other] = a["median"] / row[other]["us_per_call"]["median"]
    if row["randn_plan"] != "n/a" and a["median"] > row["randn_plan"]["us_per_call"]["median"]:
        missed.append("sampled > randn_plan")
    if row["plan"] != "n/a" and a["median"] > row["plan"]["us_per_call"]["max"]:
        missed.append("sampled above plan's sample spread")
    return out, missed


def measure(B, N, K, Hn, M, samples, seed=11):
    import torch
    from atc_hip import layout as L
    from atc_hip import lib as _lib
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=seed, timestep_limit=6000, sep_nm=0.0)
    dev = env.device
    rng = np.random.default_rng(seed)
    mean = torch.as_tensor(benchlib.same_work_actions(rng, (Hn, B, N)), device=dev)
    std = torch.full_like(mean, STD)
    first = mean[0].contiguous()
    tensor_route = M <= L.LOOKAHEAD_MAX_M
    h = _lib.load()
    stream = torch.cuda.current_stream(dev)
    q = C.c_void_p(stream.cuda_stream)
    res_s = env.lookahead_plan_sampled(mean, std, K, M, seed=seed)       # (first use: the result tensors of both routes exist)
    _, out_s = env._plan_sampled_cache[(M, Hn, ("seg_reward",))]
    dr = _lib.AtcPlanDraw(seed, 0, L.DRAW_MEAN_FIRST)
    args_s = (env.sector.handle, B, N, K, Hn, M, C.byref(env._state), C.c_void_p(mean.data_ptr()), C.c_void_p(std.data_ptr()), C.byref(dr),
              C.byref(out_s), C.byref(env.params), q)
    calls = {"sampled": lambda: _lib.check(h.atc_lookahead_plan_sampled(*args_s))}
    n_of = {"sampled": res_s["n_steps"]}
    if tensor_route:
        made = env.draw_plans(mean, std, M, seed=seed)
        res_p = env.lookahead_plan(made, K, outputs=("seg_reward",))
        _, out_p = env._plan_cache[(M, Hn, ("seg_reward",))]
        plan_args = lambda t: (env.sector.handle, B, N, K, Hn, M, C.byref(env._state), C.c_void_p(t.data_ptr()), C.byref(out_p),   # noqa: E731
                               C.byref(env.params), q)
        args_c = plan_args(made)
        keep = {}

        def randn_plan():
            keep["a"] = (mean + std * torch.randn((M, Hn, B, N, 3), device=dev)).clamp(-1, 1)
            _lib.check(h.atc_lookahead_plan(*plan_args(keep["a"])))
        calls["randn_plan"] = randn_plan
        calls["plan"] = lambda: _lib.check(h.atc_lookahead_plan(*args_c))
        n_of["randn_plan"] = n_of["plan"] = res_p["n_steps"]
    n_mean = {v: [] for v in calls}

    def prepare(v):
        env.reset()
        env.step(first)

    def after(v):
        n_mean[v].append(float(n_of[v].float().mean()))
    times = benchlib.sample(calls, samples, 1, benchlib.hip_clock(torch, stream), prepare, after)
    peak = {}
    for v in ("sampled", "randn_plan"):       # peak memory of one call of each route, on top of what the env and its results hold
        if v in calls:
            if v == "randn_plan":
                keep.clear()
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            calls[v]()
            torch.cuda.synchronize(dev)
            peak[v] = {"max_memory_allocated": int(torch.cuda.max_memory_allocated(dev)), "above_start": int(torch.cuda.max_memory_allocated(dev) - base)}
    res = {"B": B, "N": N, "K": K, "H": Hn, "M": M, "samples": samples, "calls_per_sample": 1, "candidate_tensor_bytes": M * Hn * B * N * 12,
           "mean_n_steps": {v: float(np.mean(t)) for v, t in n_mean.items()}, "memory": peak}
    for v in ("sampled", "randn_plan", "plan"):
        res[v] = {"us_per_call": benchlib.quartiles(times[v])} if v in times else "n/a"
    r, missed = verdict(res)
    res.update(r)
    res["missed"] = missed
    env.close()
    return res


def main():
    a = benchlib.parser("plan_sampled_bench.json", quick="65 536 x 16, K = 5 only").parse_args()
    torch = benchlib.start(a, "plan_sampled_bench")
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        for K in (KS[:1] if a.quick else KS):
            for Hn in HS:
                for M in MS + ((M_BEYOND,) if (B, N) == CONFIGS[1] else ()):
                    r = measure(B, N, K, Hn, M, a.samples)
                    rows.append(r)
                    us = lambda v: "%10.1f" % r[v]["us_per_call"]["median"] if r[v] != "n/a" else "       n/a"   # noqa: E731
                    fmt = lambda x: "%.3f" % x if x != "n/a" else "n/a"   # noqa: E731
                    print("%6d x %-2d K=%-2d H=%d M=%-3d  sampled %s | randn + plan %s (ratio %s) | plan alone %s (ratio %s) us/call  %s"
                          % (B, N, K, Hn, M, us("sampled"), us("randn_plan"), fmt(r["ratio_sampled_vs_randn_plan"]), us("plan"),
                             fmt(r["ratio_sampled_vs_plan"]), "MISSED: " + ", ".join(r["missed"]) if r["missed"] else ""), flush=True)
                    torch.cuda.empty_cache()
    doc = {"what": "us per call, fast form: atc_lookahead_plan_sampled | (mean + std * randn).clamp + atc_lookahead_plan | atc_lookahead_plan on a tensor made beforehand",
           "method": "HIP events around one call, variants alternating per sample, 2 warm-up rounds, every sample from a reset of all envs plus one step",
           "expectation": "sampled <= randn_plan in every row, no margin; sampled <= the max of plan's samples; rows_missed lists the rows that miss",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows,
           "rows_missed": [{"B": r["B"], "N": r["N"], "K": r["K"], "H": r["H"], "M": r["M"], "missed": r["missed"]} for r in rows if r["missed"]]}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
