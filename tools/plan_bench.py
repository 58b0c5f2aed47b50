"""Developer measurement: what scoring M plans of H held decisions per env costs.

    python tools/plan_bench.py [--out profiles/plan_bench.json] [--samples 15] [--quick] [--lib VARIANT.so]

For 65 536 x 16 and 4 096 x 64, K in {5, 20}, H in {2, 4}, M in {4, 8}, the "same work" state family of tools/lookahead_bench.py
(climbing, slowing targets inside the action space, the default time limit, a separation minimum of 0: almost no episode ends, every
variant executes M x H x K steps per env), every sample started from a reset of all envs plus one step:
  plan_fast     atc_lookahead_plan, reward / done / n_steps / seg_reward only (the fast form)
  plan_default  atc_lookahead_plan with seg_reward + flags + min_sep (the default of AtcVecEnv.lookahead_plan: the full form)
  skip_x_MH     (a) M x H back-to-back atc_step_skip(K) launches — how the parent commit runs the same arithmetic; its state flies on,
                which a planner would have to undo:
  host_recipe   (b) the host recipe: copy the six state tensors aside, then per candidate H x atc_step_skip + copy them back
A sample is the device time (HIP events) of `decisions_per_sample` decisions launched back to back; the variants take turns sample by
sample after two warm-up rounds; reported are median and quartiles in us per decision, and the ratio of the medians plan_fast /
skip_x_MH (the expectation of section 3d: at most 1 in every row).  One JSON file; needs the GPU."""
import ctypes as C

import numpy as np

import benchlib

CONFIGS = ((65536, 16), (4096, 64))
KS = (5, 20)
HS = (2, 4)
MS = (4, 8)
STATE = ("ac", "alt", "last_act", "env", "stats", "phi_wide")
VARIANTS = ("plan_fast", "plan_default", "skip_x_MH", "host_recipe")


def measure(B, N, K, H, M, samples, seed=11):
    import torch
    from atc_hip import lib as _lib
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=seed, timestep_limit=6000, sep_nm=0.0)
    dev = env.device
    cand = torch.as_tensor(benchlib.same_work_actions(np.random.default_rng(seed), (M, H, B, N)), device=dev)
    h = _lib.load()
    stream = torch.cuda.current_stream(dev)
    q = C.c_void_p(stream.cuda_stream)
    env.step_skip(cand[0, 0], 1)   # (allocates frame_steps)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
    o = {"reward": z((M, B), torch.float32), "done": z((M, B), torch.uint8), "n_steps": z((M, B), torch.int16),
         "seg_reward": z((M, H, B), torch.float32), "flags": z((M, B, N), torch.int16), "min_sep": z((M, B), torch.float32)}
    ptr = lambda *names: _lib.AtcPlanOut(*[o[n].data_ptr() if n in names else None for n in _lib.PLAN_FIELDS])   # noqa: E731
    out_fast = ptr("reward", "done", "n_steps", "seg_reward")
    out_def = ptr("reward", "done", "n_steps", "seg_reward", "flags", "min_sep")
    plan_args = lambda out: (env.sector.handle, B, N, K, H, M, C.byref(env._state), C.c_void_p(cand.data_ptr()), C.byref(out),   # noqa: E731
                             C.byref(env.params), q)
    a_fast, a_def = plan_args(out_fast), plan_args(out_def)
    skip_args = [[(env.sector.handle, B, N, K, C.byref(env._state), C.c_void_p(cand[m, j].data_ptr()), C.byref(env._out),
                   C.c_void_p(env._frame_steps_ptr), C.byref(env.params), q) for j in range(H)] for m in range(M)]
    _lib.lookahead_set_mapping(0)
    _lib.check(h.atc_lookahead_plan(*a_fast))

    def plan(args):
        return lambda: _lib.check(h.atc_lookahead_plan(*args))

    def skip_x_mh():
        for m in range(M):
            for j in range(H):
                _lib.check(h.atc_step_skip(*skip_args[m][j]))
    aside = {k: torch.empty_like(getattr(env, k)) for k in STATE}

    def host_recipe():
        for k, t in aside.items():
            t.copy_(getattr(env, k))
        for m in range(M):
            for j in range(H):
                _lib.check(h.atc_step_skip(*skip_args[m][j]))
            for k, t in aside.items():
                getattr(env, k).copy_(t)
    calls = dict(zip(VARIANTS, (plan(a_fast), plan(a_def), skip_x_mh, host_recipe)))
    inner = max(1, 60 // (M * H * K))
    n_mean = []

    def prepare(v):
        env.reset()
        env.step(cand[0, 0])
    times = benchlib.sample(calls, samples, inner, benchlib.hip_clock(torch, stream), prepare,
                            after=lambda v: v == "plan_fast" and n_mean.append(float(o["n_steps"].float().mean())))
    res = {"B": B, "N": N, "K": K, "H": H, "M": M, "samples": samples, "decisions_per_sample": inner, "mean_n_steps": float(np.mean(n_mean))}
    for v, t in times.items():
        res[v] = {"us_per_decision": benchlib.quartiles(t)}
        res[v]["us_per_candidate_step_median"] = res[v]["us_per_decision"]["median"] / (M * H * K)
    med = lambda v: res[v]["us_per_decision"]["median"]   # noqa: E731
    res["ratio_to_skip_x_MH"] = {v: med(v) / med("skip_x_MH") for v in ("plan_fast", "plan_default", "host_recipe")}
    res["fast_within_expectation"] = med("plan_fast") <= med("skip_x_MH")
    env.close()
    return res


def main():
    a = benchlib.parser("plan_bench.json", quick="65 536 x 16 only").parse_args()
    torch = benchlib.start(a, "plan_bench")
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        for K in KS:
            for H in HS:
                for M in MS:
                    r = measure(B, N, K, H, M, a.samples)
                    rows.append(r)
                    print("%6d x %-2d K=%-2d H=%d M=%d  plan fast %9.1f  default %9.1f | M x H x skip %9.1f  host recipe %9.1f us/decision | fast / (a) %.3f %s"
                          % tuple([B, N, K, H, M] + [r[v]["us_per_decision"]["median"] for v in VARIANTS] +
                                  [r["ratio_to_skip_x_MH"]["plan_fast"], "" if r["fast_within_expectation"] else "MISSED"]), flush=True)
    doc = {"what": "us per decision (M plans x H segments x K held steps per env): atc_lookahead_plan fast / default form | M x H x atc_step_skip | the host recipe",
           "method": "HIP events around `decisions_per_sample` back-to-back decisions, variants alternating per sample, 2 warm-up rounds, "
                     "every sample from a reset of all envs plus one step",
           "expectation": "plan_fast median <= skip_x_MH median in every row (no margin)",
           "rows_missed": [[r["B"], r["N"], r["K"], r["H"], r["M"]] for r in rows if not r["fast_within_expectation"]],
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
