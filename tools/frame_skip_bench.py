"""Developer measurement: what one DECISION of a frame-skipping caller costs, three ways (frame skip).

    python tools/frame_skip_bench.py [--out profiles/frame_skip_bench.json] [--samples 15] [--inner 10] [--quick] [--lib VARIANT.so]

For 65 536 x 16 (the headline batch), 65 536 x 1, 8 192 x 16, 4 096 x 64 and K in {4, 20}, same sector, seed and action stream:
  1. steps    K x atc_step, ATC_M_ACTIONS_HELD on launches 2 .. K       (what a caller does today for per-launch outputs)
  2. rollout  atc_rollout_hold(T = K, hold = K), [T] outputs              (today's one-launch form; steps THROUGH resets)
  3. skip     atc_step_skip(K)                                            (one launch, one set of outputs, stops at done)
Two series each: "same_work" — climbing, slowing targets inside the action space, the default time limit and a separation minimum
of 0 (nobody is ever in conflict), every sample started from a reset of all envs and kept to 60 steps of flight (an aircraft needs
longer than that to leave the airspace), so that almost no episode ends and the three execute the same steps — and "ordinary" —
uniform actions, a third outside the action space, a time limit of 60 steps, the default 3 nm minimum, no resets between samples.  A sample is the device time (HIP events) of `inner` decisions launched back to back with pre-bound foreign
calls; the three variants take turns sample by sample, after a warm-up of every variant; reported are median and quartiles in us
per decision and per executed env-step (variant 3: per mean n_steps of the sampled decisions).  One JSON file; needs the GPU."""
import ctypes as C
import itertools

import numpy as np

import benchlib

CONFIGS = ((65536, 16), (65536, 1), (8192, 16), (4096, 64))
KS = (4, 20)
POOL = 4   # action blocks that take turns


def action_pool(series, B, N, seed):
    rng = np.random.default_rng(seed)
    pool = []
    for _ in range(POOL):
        if series == "same_work":
            a = benchlib.same_work_actions(rng, (B, N))
        else:
            a = rng.uniform(-1.05, 1.05, (B, N, 3))
            far = rng.uniform(-4.0, 4.0, (B, N, 3))
            a = np.where(rng.uniform(size=(B, N, 3)) < 0.33, far, a)
        pool.append(a.astype(np.float32))
    return pool


def measure(B, N, K, series, samples, inner, seed=11):
    import torch
    from atc_hip import lib as _lib
    from atc_hip import layout as L
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    scn = scenarios.LOWW(random_entrypoints=True) if N == 1 else scenarios.LOWWDense()
    limit, sep_nm = (6000, 0.0) if series == "same_work" else (60, 3.0)
    envs = {v: AtcVecEnv(B, N, scenario=scn, auto_reset=True, seed=seed, timestep_limit=limit, sep_nm=sep_nm) for v in ("steps", "rollout", "skip")}
    dev = envs["skip"].device
    pool = [torch.as_tensor(a, device=dev) for a in action_pool(series, B, N, seed)]
    h = _lib.load()
    stream = torch.cuda.current_stream(dev)
    q = C.c_void_p(stream.cuda_stream)
    calls = {}
    # 1. K launches per decision through the env's pre-bound launchers
    e = envs["steps"]
    first = [e.make_launcher(a) for a in pool]
    held = [e.make_launcher(a, held=True) for a in pool]

    def steps(i):
        first[i]()
        for _ in range(K - 1):
            held[i]()
    calls["steps"] = steps
    # 2. one multi-step launch with [T] outputs
    e = envs["rollout"]
    bufs = {"obs": torch.empty((K, B, N * L.OBS_DIM), dtype=torch.float32, device=dev), "reward": torch.empty((K, B), dtype=torch.float32, device=dev),
            "done": torch.empty((K, B), dtype=torch.uint8, device=dev), "flags": torch.empty((K, B, N), dtype=torch.int16, device=dev)}
    out_r = e._make_out(bufs["obs"], None, bufs["reward"], None, bufs["done"], bufs["flags"], None, None, None)
    args_r = [(e.sector.handle, B, N, K, K, C.byref(e._state), C.c_void_p(a.data_ptr()), C.byref(out_r), C.byref(e.params), q) for a in pool]
    calls["rollout"] = lambda i: _lib.check(h.atc_rollout_hold(*args_r[i]))
    # 3. the frame-skip launch
    e = envs["skip"]
    e.step_skip(pool[0], 1)   # (allocates frame_steps; every variant gets the same extra first step below)
    args_s = [(e.sector.handle, B, N, K, C.byref(e._state), C.c_void_p(a.data_ptr()), C.byref(e._out), C.c_void_p(e._frame_steps_ptr),
               C.byref(e.params), q) for a in pool]
    calls["skip"] = lambda i: _lib.check(h.atc_step_skip(*args_s[i]))
    envs["steps"].step(pool[0])
    envs["rollout"].step(pool[0])

    if series == "same_work":
        inner = max(2, min(inner, 60 // K))
    n_mean = []

    def rotating(fn):   # the action blocks take turns call by call, every variant through the same sequence
        n = itertools.count()
        return lambda: fn(next(n) % POOL)
    times = benchlib.sample({v: rotating(fn) for v, fn in calls.items()}, samples, inner, benchlib.hip_clock(torch, stream),
                            prepare=(lambda v: envs[v].reset()) if series == "same_work" else None,
                            after=lambda v: v == "skip" and n_mean.append(float(envs["skip"].frame_steps.float().mean())))
    res = {"B": B, "N": N, "K": K, "series": series, "timestep_limit": limit, "sep_nm": sep_nm, "samples": samples, "decisions_per_sample": inner,
           "mean_n_steps_skip": float(np.mean(n_mean)), "episodes_ended": {v: int(envs[v].episodes.sum()) for v in envs}}
    for v, t in times.items():
        per = res["mean_n_steps_skip"] if v == "skip" else float(K)
        res[v] = {"us_per_decision": benchlib.quartiles(t), "executed_steps_per_decision": per}
        res[v]["us_per_env_step_median"] = res[v]["us_per_decision"]["median"] / per
    for v in envs:
        envs[v].close()
    return res


def main():
    a = benchlib.parser("frame_skip_bench.json", inner=10, quick="the headline batch only").parse_args()
    torch = benchlib.start(a, "frame_skip_bench")
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        for K in KS:
            for series in ("same_work", "ordinary"):
                r = measure(B, N, K, series, a.samples, a.inner)
                rows.append(r)
                print("%6d x %-2d K=%-2d %-9s  steps %8.1f  rollout %8.1f  skip %8.1f us/decision (medians; skip mean n = %.2f)"
                      % (B, N, K, series, r["steps"]["us_per_decision"]["median"], r["rollout"]["us_per_decision"]["median"],
                         r["skip"]["us_per_decision"]["median"], r["mean_n_steps_skip"]), flush=True)
    doc = {"what": "us per decision of a frame-skipping caller: K x atc_step (held hint) | atc_rollout_hold(T = K, hold = K) | atc_step_skip(K)",
           "method": "HIP events around `decisions_per_sample` back-to-back decisions, variants alternating per sample, 2 warm-up rounds",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
