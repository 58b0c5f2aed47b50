"""Developer measurement: what the glue between a sampling planner's scoring launch and its refit launch costs as stock torch ops, and
what it costs as one launch.

    python tools/plan_score_bench.py [--out profiles/plan_score_bench.json] [--samples 15] [--quick] [--lib VARIANT.so]

For 65 536 x 16 and 4 096 x 64, H in {2, 4}, M in {64, 256, 1024}, on a seg_reward [M, H, B] of negative random rewards and an n_steps
[M, B] with a tenth of the candidates not evaluated, gamma = 0.9:
  score_elite     (a) AtcVecEnv.score_plans, mode "elite", 16 elites, top = 1, into preallocated buffers
  glue_cem        (b) the torch glue of cem.py::_cem on the same seg_reward: the discount multiply-and-sum, topk, scatter_ (and the
                      winner's row, elite_idx[:1])
  score_softmax   (c) AtcVecEnv.score_plans, mode "softmax", top = 1, into preallocated buffers
  glue_mppi       (d) the torch glue of mppi_plan: the discount, max, exp, where on n_steps, argmax
For every variant: time, and torch.cuda.max_memory_allocated above the start of a call of its own — the inputs and, for (a) and (c),
the preallocated result buffers are held before that start, so (a) and (c) are expected to show 0.  `lookahead_us` is the median of the
atc_lookahead_plan_sampled launch of the same shape taken from profiles/plan_refit_bench.json where that file has the row (K = 5), for
scale; it is not measured again here.  No time is fixed in advance: `rows_slower` lists every row where (a)'s median is above (b)'s or
(c)'s above (d)'s.
A sample is the device time (HIP events) of one call; the variants take turns sample by sample after two warm-up rounds; reported are
median, quartiles, min and max in us per call.  One JSON file; needs the GPU."""
import json
import os

import numpy as np

import benchlib

CONFIGS = ((65536, 16), (4096, 64))
HS = (2, 4)
MS = (64, 256, 1024)
ELITES = 16
GAMMA, TEMPERATURE = 0.9, 5.0
REFIT_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "plan_refit_bench.json")


def lookahead_medians():
    """{(B, N, H, M): median us of the scoring launch} from the refit measurement's file, {} where it is missing"""
    try:
        rows = json.load(open(REFIT_JSON))["rows"]
    except (OSError, ValueError, KeyError):
        return {}
    return {(r["B"], r["N"], r["H"], r["M"]): r["score"]["us_per_call"]["median"] for r in rows}


def measure(env, Hn, M, samples, seed=11):
    import torch
    B, dev = env.B, env.device
    gen = torch.Generator(device=dev).manual_seed(seed + M + Hn)
    seg = -torch.rand((M, Hn, B), device=dev, generator=gen) * 10.0
    n_steps = torch.where(torch.rand((M, B), device=dev, generator=gen) < 0.1, 0, 5 * Hn).to(torch.int16)
    discount = torch.tensor([GAMMA ** h for h in range(Hn)], dtype=torch.float32, device=dev)
    out = {"score": torch.empty((M, B), dtype=torch.float32, device=dev), "weight": torch.empty((M, B), dtype=torch.float32, device=dev),
           "top": torch.empty((1, B), dtype=torch.int32, device=dev)}
    keep = {}

    def glue_cem():
        score = (seg * discount[None, :, None]).sum(1)
        elite_idx = score.topk(ELITES, dim=0).indices
        keep["r"] = (torch.zeros_like(score).scatter_(0, elite_idx, 1.0), elite_idx[:1])

    def glue_mppi():
        score = (seg * discount[None, :, None]).sum(1)
        weight = torch.exp((score - score.max(0).values) / TEMPERATURE)
        keep["r"] = (torch.where(n_steps == 0, torch.zeros_like(weight), weight), score.argmax(0)[None])

    def score_elite():
        env.score_plans(seg, n_steps, mode="elite", elites=ELITES, gamma=GAMMA, top=1, out=out)

    def score_softmax():
        env.score_plans(seg, n_steps, mode="softmax", temperature=TEMPERATURE, gamma=GAMMA, top=1, out=out)
    calls = {"score_elite": score_elite, "glue_cem": glue_cem, "score_softmax": score_softmax, "glue_mppi": glue_mppi}
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock)
    peak = {}
    for v, fn in calls.items():       # peak memory of one call of each variant, on top of what the inputs and the result buffers hold
        keep.clear()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize(dev)
        peak[v] = int(torch.cuda.max_memory_allocated(dev) - base)
    keep.clear()
    res = {"B": B, "N": env.N, "H": Hn, "M": M, "elites": ELITES, "samples": samples, "seg_reward_bytes": M * Hn * B * 4,
           "result_bytes": 2 * M * B * 4 + B * 4}
    for v in calls:
        res[v] = {"us_per_call": benchlib.quartiles(times[v]), "peak_bytes_above_start": peak[v]}
    med = lambda v: res[v]["us_per_call"]["median"]   # noqa: E731
    res["ratio_score_elite_vs_glue_cem"] = med("score_elite") / med("glue_cem")
    res["ratio_score_softmax_vs_glue_mppi"] = med("score_softmax") / med("glue_mppi")
    res["slower"] = [a for a, b in (("score_elite", "glue_cem"), ("score_softmax", "glue_mppi")) if med(a) > med(b)]
    res["missed"] = ["%s allocates device memory" % v for v in ("score_elite", "score_softmax") if peak[v] > 0]
    return res


def main():
    a = benchlib.parser("plan_score_bench.json", quick="65 536 x 16, H = 2 only").parse_args()
    torch = benchlib.start(a, "plan_score_bench")
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    look = lookahead_medians()
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=11, timestep_limit=6000, sep_nm=0.0)
        for Hn in (HS[:1] if a.quick else HS):
            for M in MS:
                r = measure(env, Hn, M, a.samples)
                r["lookahead_us"] = look.get((B, N, Hn, M))
                rows.append(r)
                cell = lambda v: "%9.1f us %7.1f MiB" % (r[v]["us_per_call"]["median"], r[v]["peak_bytes_above_start"] / 2 ** 20)   # noqa: E731
                print("%6d x %-2d H=%d M=%-4d  (a) %s | (b) %s | (c) %s | (d) %s | lookahead %s us  %s" % (
                    B, N, Hn, M, cell("score_elite"), cell("glue_cem"), cell("score_softmax"), cell("glue_mppi"),
                    "%.0f" % r["lookahead_us"] if r["lookahead_us"] else "n/a", ("SLOWER: " + ", ".join(r["slower"])) if r["slower"] else ""), flush=True)
                torch.cuda.empty_cache()
        env.close()
    ident = lambda r: {k: r[k] for k in ("B", "N", "H", "M")}   # noqa: E731
    doc = {"what": "us per call and peak bytes allocated: score_plans (elite, 16 elites, top 1) | the torch glue of cem.py::_cem (discount, topk, scatter_) | "
                   "score_plans (softmax) | the torch glue of mppi_plan (discount, max, exp, where, argmax); lookahead_us: the scoring launch, from plan_refit_bench.json",
           "method": "HIP events around one call, variants alternating per sample, 2 warm-up rounds; peak = torch.cuda.max_memory_allocated above the start of one call "
                     "(inputs and score_plans' preallocated results held before it)",
           "expectation": "score_elite and score_softmax allocate nothing; no time is fixed: rows_slower lists the rows where score_plans' median is above the glue's",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows,
           "rows_slower": [dict(ident(r), slower=r["slower"]) for r in rows if r["slower"]],
           "rows_missed": [dict(ident(r), missed=r["missed"]) for r in rows if r["missed"]]}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
