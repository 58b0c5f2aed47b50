"""Developer measurement: what keeping M look-ahead outcomes per env as states costs, and what gathering states by index costs
(DESIGN.md, section 3f).

    python tools/branch_bench.py [--out profiles/branch_bench.json] [--samples 15] [--quick] [--lib VARIANT.so]

For 65 536 x 16 and 4 096 x 64, K in {4, 20}, M in {4, 8}, the "same work" state family of tools/frame_skip_bench.py (climbing, slowing
targets inside the action space, the default time limit, a separation minimum of 0: almost no episode ends, every variant executes
M x K steps per env), every sample started from a reset of all envs plus one step:
  branch          atc_branch into a child env's bound outputs (obs, reward, done, flags, frame_steps: the full form)
  copies_skip     (a) the same child batch without atc_branch: six expanded copy_ of the parent's state tensors into the child's, then
                  ONE atc_step_skip(K) over the child's M x B envs
  select          atc_state_select: the parent takes env best[e] * B + e of the child
  index_copy      (b) the same gather in torch: six index_select + six copy_
The expectation is branch <= copies_skip and select <= index_copy in every row, with no margin; `ratio_*` holds median / median and
`rows_missed` lists every (row, comparison) whose ratio is above 1.
A sample is the device time (HIP events) of `calls_per_sample` calls launched back to back; the variants take turns sample by sample
after two warm-up rounds; reported are median and quartiles in us per call.  One JSON file; needs the GPU."""
import ctypes as C

import numpy as np

import benchlib

CONFIGS = ((65536, 16), (4096, 64))
KS = (4, 20)
MS = (4, 8)
STATE = ("ac", "alt", "last_act", "env", "stats", "phi_wide")
PAIRS = (("branch", "copies_skip"), ("select", "index_copy"))


def ratios(row):
    """{"ratio_<new>_vs_<old>": median / median} of a measured row, and the names of the comparisons it misses (ratio > 1)"""
    out, missed = {}, []
    for new, old in PAIRS:
        r = row[new]["us_per_call"]["median"] / row[old]["us_per_call"]["median"]
        out["ratio_%s_vs_%s" % (new, old)] = r
        if r > 1.0:
            missed.append("%s > %s" % (new, old))
    return out, missed


def measure(B, N, K, M, samples, seed=11):
    import torch
    from atc_hip import lib as _lib
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    scn = scenarios.LOWWDense()
    make = lambda b, cell="auto": AtcVecEnv(b, N, scenario=scn, auto_reset=True, seed=seed, timestep_limit=6000, sep_nm=0.0, grid_cell=cell)   # noqa: E731
    env = make(B)
    child = make(M * B, env.grid_cell)   # (the parent's resolved lookup-grid cell: "auto" depends on the batch size, and both must share one sector blob)
    dev = env.device
    cand = torch.as_tensor(benchlib.same_work_actions(np.random.default_rng(seed), (M, B, N)), device=dev)
    h = _lib.load()
    stream = torch.cuda.current_stream(dev)
    q = C.c_void_p(stream.cuda_stream)
    child.step_skip(cand.view(M * B, N, 3), 1)   # (allocates the child's frame_steps)
    env.branch(cand, K, into=child)              # (first use: every tensor touched once)
    out = _lib.AtcLookaheadOut(reward=child.reward.data_ptr(), done=child.done.data_ptr(), n_steps=child.frame_steps.data_ptr(),
                               flags=child.flags.data_ptr(), obs=child.obs.data_ptr())
    branch_args = (env.sector.handle, B, N, K, M, C.byref(env._state), C.c_void_p(cand.data_ptr()), C.byref(child._state), C.byref(out),
                   C.byref(env.params), q)
    skip_args = (child.sector.handle, M * B, N, K, C.byref(child._state), C.c_void_p(cand.data_ptr()), C.byref(child._out),
                 C.c_void_p(child._frame_steps_ptr), C.byref(child.params), q)
    rows = {k: getattr(env, k).shape[0] for k in STATE}
    wide = {k: (getattr(child, k).view(M, rows[k], -1), getattr(env, k).view(rows[k], -1)) for k in STATE}
    best = torch.as_tensor(np.random.default_rng(seed + 1).integers(0, M, B), device=dev)
    idx64 = best * B + torch.arange(B, device=dev)
    idx32 = idx64.to(torch.int32)
    sel_args = (env.sector.handle, N, B, C.byref(env._state), M * B, C.byref(child._state), C.c_void_p(idx32.data_ptr()), None, q)
    per_env = {k: (getattr(env, k).view(B, -1), getattr(child, k).view(M * B, -1)) for k in STATE}

    def branch():
        _lib.check(h.atc_branch(*branch_args))

    def copies_skip():
        for k in STATE:
            wide[k][0].copy_(wide[k][1])     # [M, rows, words] <- [rows, words]: the expanded copy
        _lib.check(h.atc_step_skip(*skip_args))

    def select():
        _lib.check(h.atc_state_select(*sel_args))

    def index_copy():
        for k in STATE:
            per_env[k][0].copy_(per_env[k][1].index_select(0, idx64))
    calls = {"branch": branch, "copies_skip": copies_skip, "select": select, "index_copy": index_copy}
    inner = max(1, 60 // (M * K))
    n_mean = {"branch": [], "copies_skip": []}

    def prepare(v):
        env.reset()
        env.step(cand[0])

    def after(v):
        if v in n_mean:
            n_mean[v].append(float(child.frame_steps.float().mean()))
    times = benchlib.sample(calls, samples, inner, benchlib.hip_clock(torch, stream), prepare, after)
    res = {"B": B, "N": N, "K": K, "M": M, "samples": samples, "calls_per_sample": inner,
           "mean_n_steps": {v: float(np.mean(t)) for v, t in n_mean.items()}}
    for v, t in times.items():
        res[v] = {"us_per_call": benchlib.quartiles(t)}
    r, missed = ratios(res)
    res.update(r)
    res["missed"] = missed
    env.close()
    child.close()
    return res


def main():
    a = benchlib.parser("branch_bench.json", quick="65 536 x 16 only").parse_args()
    torch = benchlib.start(a, "branch_bench")
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        for K in KS:
            for M in MS:
                r = measure(B, N, K, M, a.samples)
                rows.append(r)
                print("%6d x %-2d K=%-2d M=%d  branch %9.1f | copies + skip %9.1f (ratio %.3f)   select %7.1f | index_select + copy_ %7.1f (ratio %.3f) us/call  %s"
                      % (B, N, K, M, r["branch"]["us_per_call"]["median"], r["copies_skip"]["us_per_call"]["median"], r["ratio_branch_vs_copies_skip"],
                         r["select"]["us_per_call"]["median"], r["index_copy"]["us_per_call"]["median"], r["ratio_select_vs_index_copy"],
                         "MISSED: " + ", ".join(r["missed"]) if r["missed"] else ""), flush=True)
    doc = {"what": "us per call: atc_branch | six expanded copy_ + one atc_step_skip over M x B envs;  atc_state_select | six index_select + six copy_",
           "method": "HIP events around `calls_per_sample` back-to-back calls, variants alternating per sample, 2 warm-up rounds, "
                     "every sample from a reset of all envs plus one step",
           "expectation": "branch <= copies_skip and select <= index_copy in every row, no margin; rows_missed lists the rows that miss",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows,
           "rows_missed": [{"B": r["B"], "N": r["N"], "K": r["K"], "M": r["M"], "missed": r["missed"]} for r in rows if r["missed"]]}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
