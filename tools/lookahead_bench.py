"""Developer measurement: what scoring M candidate decisions per env costs.

    python tools/lookahead_bench.py [--out profiles/lookahead_bench.json] [--samples 15] [--quick] [--lib VARIANT.so]

For 65 536 x 16 and 4 096 x 64, K in {4, 20}, M in {4, 8}, the "same work" state family of tools/frame_skip_bench.py (climbing, slowing
targets inside the action space, the default time limit, a separation minimum of 0: almost no episode ends, every variant executes
M x K steps per env), every sample started from a reset of all envs plus one step:
  look_fast       atc_lookahead, reward / done / n_steps only (the fast form), one workgroup per (tile, candidate)
  look_fm         atc_lookahead with flags + min_sep (the default of AtcVecEnv.lookahead), the same mapping
  look_fast_loop  / look_fm_loop: the same with the other mapping (atc_lookahead_set_mapping(M): one workgroup per tile that loops
                  over all M candidates)
  skip_x_M        (a) M back-to-back atc_step_skip(K) launches — what the parent commit offers for the same arithmetic; its state
                  flies on (M x K steps per decision), which a look-ahead caller would have to undo:
  host_recipe     (b) the honest host recipe: copy the six state tensors aside, then per candidate atc_step_skip + copy them back
A sample is the device time (HIP events) of `decisions_per_sample` decisions launched back to back; the variants take turns sample by
sample after two warm-up rounds; reported are median and quartiles in us per decision.  One JSON file; needs the GPU."""
import ctypes as C

import numpy as np

import benchlib

CONFIGS = ((65536, 16), (4096, 64))
KS = (4, 20)
MS = (4, 8)
STATE = ("ac", "alt", "last_act", "env", "stats", "phi_wide")


def measure(B, N, K, M, samples, seed=11):
    import torch
    from atc_hip import lib as _lib
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    scn = scenarios.LOWWDense()
    env = AtcVecEnv(B, N, scenario=scn, auto_reset=True, seed=seed, timestep_limit=6000, sep_nm=0.0)
    dev = env.device
    cand = torch.as_tensor(benchlib.same_work_actions(np.random.default_rng(seed), (M, B, N)), device=dev)
    h = _lib.load()
    stream = torch.cuda.current_stream(dev)
    q = C.c_void_p(stream.cuda_stream)
    env.step_skip(cand[0], 1)   # (allocates frame_steps)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
    o = {"reward": z((M, B), torch.float32), "done": z((M, B), torch.uint8), "n_steps": z((M, B), torch.uint8),
         "flags": z((M, B, N), torch.int16), "min_sep": z((M, B), torch.float32)}
    out_fast = _lib.AtcLookaheadOut(o["reward"].data_ptr(), o["done"].data_ptr(), o["n_steps"].data_ptr(), None, None, None, None)
    out_fm = _lib.AtcLookaheadOut(o["reward"].data_ptr(), o["done"].data_ptr(), o["n_steps"].data_ptr(), o["flags"].data_ptr(), None,
                                  o["min_sep"].data_ptr(), None)
    look_args = lambda out: (env.sector.handle, B, N, K, M, C.byref(env._state), C.c_void_p(cand.data_ptr()), C.byref(out),   # noqa: E731
                             C.byref(env.params), q)
    a_fast, a_fm = look_args(out_fast), look_args(out_fm)
    skip_args = [(env.sector.handle, B, N, K, C.byref(env._state), C.c_void_p(cand[m].data_ptr()), C.byref(env._out),
                  C.c_void_p(env._frame_steps_ptr), C.byref(env.params), q) for m in range(M)]
    _lib.lookahead_set_mapping(0)
    _lib.check(h.atc_lookahead(*a_fast))
    other = M   # candidates per workgroup of the loop mapping

    def look(args, cpg):
        def run():
            h.atc_lookahead_set_mapping(cpg)
            _lib.check(h.atc_lookahead(*args))
        return run

    def skip_x_m():
        for m in range(M):
            _lib.check(h.atc_step_skip(*skip_args[m]))
    aside = {k: torch.empty_like(getattr(env, k)) for k in STATE}

    def host_recipe():
        for k, t in aside.items():
            t.copy_(getattr(env, k))
        for m in range(M):
            _lib.check(h.atc_step_skip(*skip_args[m]))
            for k, t in aside.items():
                getattr(env, k).copy_(t)
    calls = {"look_fast": look(a_fast, 1), "look_fm": look(a_fm, 1), "look_fast_loop": look(a_fast, other), "look_fm_loop": look(a_fm, other),
             "skip_x_M": skip_x_m, "host_recipe": host_recipe}
    inner = max(1, 60 // (M * K))
    n_mean = {"look": [], "skip": []}

    def prepare(v):
        env.reset()
        env.step(cand[0])

    def after(v):
        if v == "look_fast":
            n_mean["look"].append(float(o["n_steps"].float().mean()))
        if v == "skip_x_M":
            n_mean["skip"].append(float(env.frame_steps.float().mean()))
    times = benchlib.sample(calls, samples, inner, benchlib.hip_clock(torch, stream), prepare, after)
    h.atc_lookahead_set_mapping(0)
    res = {"B": B, "N": N, "K": K, "M": M, "samples": samples, "decisions_per_sample": inner,
           "mean_n_steps": {"lookahead": float(np.mean(n_mean["look"])), "last_skip_launch": float(np.mean(n_mean["skip"]))}}
    for v, t in times.items():
        res[v] = {"us_per_decision": benchlib.quartiles(t)}
        res[v]["us_per_candidate_step_median"] = res[v]["us_per_decision"]["median"] / (M * K)
    env.close()
    return res


def main():
    a = benchlib.parser("lookahead_bench.json", quick="65 536 x 16 only").parse_args()
    torch = benchlib.start(a, "lookahead_bench")
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        for K in KS:
            for M in MS:
                r = measure(B, N, K, M, a.samples)
                rows.append(r)
                print("%6d x %-2d K=%-2d M=%d  look fast %8.1f  +flags,min_sep %8.1f | other mapping %8.1f %8.1f | M x skip %8.1f  host recipe %8.1f us/decision"
                      % tuple([B, N, K, M] + [r[v]["us_per_decision"]["median"] for v in
                                              ("look_fast", "look_fm", "look_fast_loop", "look_fm_loop", "skip_x_M", "host_recipe")]), flush=True)
    doc = {"what": "us per decision (M candidates x K held steps per env): atc_lookahead, both candidate mappings | M x atc_step_skip | the host recipe",
           "method": "HIP events around `decisions_per_sample` back-to-back decisions, variants alternating per sample, 2 warm-up rounds, "
                     "every sample from a reset of all envs plus one step",
           "mappings": "look_* : one workgroup per (tile, candidate) (atc_lookahead_set_mapping(1)); look_*_loop: one workgroup per tile, all M candidates in a loop",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
