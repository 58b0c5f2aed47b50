"""Developer measurement: what the terminal traffic records cost the collection launch.

    python tools/collect_term_bench.py --parent PARENT.so [--out profiles/collect_term_bench.json] [--samples 7] [--quick]

At 4 096 x 16 and 65 536 x 16, hold = 20, D = 52 decisions (T = 1 040), K = 2 and 4, timestep_limit = 200 (so episodes end inside the run),
in one process, the variants taking turns sample by sample after two warm-up rounds:
  term      env.rollout_policy_term(weights, T, K, hold) into preallocated buffers, term_traffic included
  ends      env.rollout_policy_ends(weights, T, K, hold) through PARENT.so — libatcstep.so built from the PARENT commit
            (git stash / git worktree, python atc-reinforcement-learning_amd/build.py, copy the library aside), loaded next to the in-tree
            library and called on the same env: the comparison is against the parent, never against the code under test.  Measured under
            two names (`ends` / `ends_again`): the ratio of those two medians is the within-session range the new call's ratio is read against.
  collect   env.rollout_policy_traffic(weights, T, K, hold) of the in-tree library: the launch behind ppo.collect(traffic=K), the only
            collection a trainer of a traffic policy had — without bootstrap —, for context.
Without --parent the `ends` rows come from the in-tree library and the file says so.  A sample is the device time (HIP events) of one call;
median, quartiles, min and max.  One JSON file; needs the GPU."""
import ctypes as C

import benchlib

CONFIGS = ((4096, 16), (65536, 16))
KS = (2, 4)
HOLD, D = 20, 52
LIMIT = 200


def measure(env, K, samples, parent, seed=11):
    import torch
    from atc_hip import policy
    B, N, dev = env.B, env.N, env.device
    T = HOLD * D
    torch.manual_seed(seed)
    IN = 10 + 7 * K
    net = torch.nn.Sequential(torch.nn.Linear(IN, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 3)).to(dev)
    w = policy.from_torch(net, torch.full((3,), -0.5, device=dev), traffic=K)
    out = {"obs": torch.empty((T, B, N * 10), device=dev), "reward": torch.empty((T, B), device=dev),
           "done": torch.empty((T, B), dtype=torch.uint8, device=dev), "flags": torch.empty((T, B, N), dtype=torch.int16, device=dev),
           "action": torch.empty((D, B, N, 3), device=dev), "logp": torch.empty((D, B, N), device=dev), "traffic": torch.empty((D, B, N, K, 8), device=dev)}
    ends = dict(out, term_obs=torch.zeros((D, B, N, 10), device=dev), term_flags=torch.empty((D, B), dtype=torch.int16, device=dev),
                control=torch.empty((D, B, N), dtype=torch.uint8, device=dev))
    term = dict(ends, term_traffic=torch.zeros((D, B, N, K, 8), device=dev))
    state = {"dec": 0}
    own = env._lib

    def run_term():
        env.rollout_policy_term(w, T, K, hold=HOLD, seed=seed, decision0=state["dec"], out=term)
        state["dec"] += D

    def run_ends():
        env._lib = parent or own
        try:
            env.rollout_policy_ends(w, T, K, hold=HOLD, seed=seed, decision0=state["dec"], out=ends)
        finally:
            env._lib = own
        state["dec"] += D

    def run_collect():
        env.rollout_policy_traffic(w, T, K, hold=HOLD, seed=seed, decision0=state["dec"], out=out)
        state["dec"] += D
    calls = {"ends": run_ends, "term": run_term, "collect": run_collect, "ends_again": run_ends}
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock, prepare=lambda v: env.reset())
    res = {"B": B, "N": N, "K": K, "T": T, "hold": HOLD, "samples": samples, "ended_blocks_share": float((term["term_flags"] != 0).float().mean())}
    for v in times:
        res[v] = {"us_per_step": benchlib.quartiles([t / T for t in times[v]])}
    med = lambda v: res[v]["us_per_step"]["median"]      # noqa: E731
    res["ratio_term_to_parent_ends"] = med("term") / med("ends")
    res["ratio_ends_again_to_ends"] = med("ends_again") / med("ends")
    res["ratio_collect_to_parent_ends"] = med("collect") / med("ends")
    both = times["ends"] + times["ends_again"]
    res["parent_ends_range"] = [min(both) / T / med("ends"), max(both) / T / med("ends")]
    res["inside_parent_range"] = res["parent_ends_range"][0] <= res["ratio_term_to_parent_ends"] <= res["parent_ends_range"][1]
    return res


def load_parent(path):
    """the parent commit's library next to the in-tree one: only atc_rollout_policy_ends is called through it"""
    from atc_hip import lib
    own = lib.load()
    parent = C.CDLL(path)
    assert not hasattr(parent, "atc_rollout_policy_term"), "%s has atc_rollout_policy_term: not a build of the parent commit" % path
    parent.atc_rollout_policy_ends.argtypes = own.atc_rollout_policy_ends.argtypes
    parent.atc_rollout_policy_ends.restype = C.c_int
    return parent


def main():
    ap = benchlib.parser("collect_term_bench.json", quick="4 096 x 16 only")
    ap.add_argument("--parent", default=None, help="libatcstep.so built from the parent commit")
    ap.set_defaults(samples=7)
    a = ap.parse_args()
    torch = benchlib.start(a, "collect_term_bench")
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    parent = load_parent(a.parent) if a.parent else None
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=11, timestep_limit=LIMIT, sep_nm=0.0)
        for K in KS:
            r = measure(env, K, a.samples, parent)
            rows.append(r)
            print("%6d x %-2d K=%d  parent ends %8.3f us/step  term %8.3f  collect %8.3f  term/ends %.4f  ends_again/ends %.4f  parent range [%.4f, %.4f] %s" % (
                B, N, K, r["ends"]["us_per_step"]["median"], r["term"]["us_per_step"]["median"], r["collect"]["us_per_step"]["median"],
                r["ratio_term_to_parent_ends"], r["ratio_ends_again_to_ends"], r["parent_ends_range"][0], r["parent_ends_range"][1],
                "" if r["inside_parent_range"] else "OUTSIDE"), flush=True)
            torch.cuda.empty_cache()
        env.close()
    doc = {"what": "us per env step of rollout_policy_term (in-tree) against rollout_policy_ends(traffic=K) of the parent commit's library and against "
                   "rollout_policy_traffic (the launch behind collect(traffic=K))",
           "method": "HIP events around one call, variants alternating per sample in one process, 2 warm-up rounds; the parent's call measured under two "
                     "names; parent_ends_range = min and max of all its samples over its median",
           "expectation": "the query runs at ending steps only: term / ends inside the parent's own range; inside_parent_range says whether it is",
           "box": benchlib.box(torch), "parent_library": a.parent or "NOT GIVEN: the ends rows are the in-tree library's", "rows": rows}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
