"""Developer measurement: the evaluation launch against a collection launch folded in torch.

    python tools/policy_eval_bench.py [--out profiles/policy_eval_bench.json] [--samples 7] [--quick]  [--lib VARIANT.so]

On 4 096 x 16 and 65 536 x 16, T = 100, K = 0 and 4, hold 1 and 20, in one process, the two variants taking turns sample by sample after two
warm-up rounds, each sample from a fresh reset (outside the clock), same T, hold, K, weights and seed for both:
  eval      env.evaluate_policy(weights, T, K, hold): the per-env record, nothing stored per step
  collect   env.rollout_policy_ends(weights, T, K, hold) into preallocated out= buffers (the four step outputs and action; logp, traffic and
            the three per-decision outputs left out), then the torch fold of reward / done / flags into the record's EPISODES, WINS and
            RETURN_SUM words
A sample is the device time (HIP events) of the variant's calls; median with min and max.  ratio = eval / collect; `slower` marks a row
where the evaluation launch is the slower one.  `fold_matches`: once per row, outside the clock, the fold's EPISODES and WINS equal the
record's exactly and its RETURN_SUM within 1e-4 relative (the fold adds a block's rewards in another order).  timestep_limit 25, so that
episodes end inside the T steps.  No time is fixed in advance.  One JSON file; needs the GPU."""
import benchlib

CONFIGS = ((4096, 16), (65536, 16))
T = 100
RUNS = ((0, 1), (0, 20), (4, 1), (4, 20))      # (K, hold)
SEED = 11
F_WON, F_INACTIVE = 4, 256


def fold(torch, out):
    """EPISODES, WINS, RETURN_SUM [B] of a launch that began at a reset, from its reward / done [T, B] and flags [T, B, N]"""
    done = out["done"] != 0
    episodes = done.sum(dim=0, dtype=torch.int32)
    fl = out["flags"]
    won, gone = (fl & F_WON) != 0, (fl & (F_WON | F_INACTIVE)) != 0
    wins = (done & won.any(dim=2) & gone.all(dim=2)).sum(dim=0, dtype=torch.int32)     # every aircraft handed over, the last of them now
    counted = out["done"].flip(0).cummax(dim=0).values.flip(0)                        # 1 on the steps of episodes that end inside the launch
    return episodes, wins, (out["reward"] * counted).sum(dim=0)


def measure(env, K, hold, samples):
    import torch
    from atc_hip import layout as L
    B, N, dev = env.B, env.N, env.device
    gen = torch.Generator(device=dev).manual_seed(SEED + K)
    w = torch.randn(L.policy_words(K) if K else L.POLICY_WORDS, device=dev, generator=gen) * 0.1
    D = T // hold
    out = {"obs": torch.empty((T, B, N * 10), device=dev), "reward": torch.empty((T, B), device=dev), "done": torch.empty((T, B), dtype=torch.uint8, device=dev),
           "flags": torch.empty((T, B, N), dtype=torch.int16, device=dev), "action": torch.empty((D, B, N, 3), device=dev)}
    record = torch.empty((B, L.EVAL_WORDS), dtype=torch.int32, device=dev)

    def run_eval(obs0=None):
        return env.evaluate_policy(w, T, traffic=K, hold=hold, seed=SEED, deterministic=False, obs0=obs0, record=record)["record"]

    def run_collect(obs0=None):
        env.rollout_policy_ends(w, T, K, hold=hold, seed=SEED, obs0=obs0, out=out)
        return fold(torch, out)
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample({"eval": run_eval, "collect": run_collect}, samples, 1, clock, prepare=lambda v: env.reset())
    # outside the clock: both variants once from the same state
    env.reset()
    state = ("ac", "alt", "last_act", "env", "stats", "phi_wide")
    snap, x0 = {k: getattr(env, k).clone() for k in state}, env.obs.clone()
    rec = run_eval(x0).clone()
    for k, v in snap.items():
        getattr(env, k).copy_(v)
    episodes, wins, ret = run_collect(x0)
    rsum = rec[:, L.EVAL_RETURN_SUM].contiguous().view(torch.float32)
    matches = bool(torch.equal(rec[:, L.EVAL_EPISODES], episodes) and torch.equal(rec[:, L.EVAL_WINS], wins) and
                   torch.all((rsum - ret).abs() <= 1e-4 * rsum.abs().clamp(min=1.0)))
    res = {"B": B, "N": N, "T": T, "K": K, "hold": hold, "samples": samples, "episodes": int(episodes.sum()), "wins": int(wins.sum()), "fold_matches": matches}
    for v in times:
        res[v] = {"us_per_step": benchlib.quartiles([t / T for t in times[v]])}
    res["ratio"] = res["eval"]["us_per_step"]["median"] / res["collect"]["us_per_step"]["median"]
    res["slower"] = res["ratio"] > 1.0
    return res


def main():
    ap = benchlib.parser("policy_eval_bench.json", quick="4 096 x 16 only")
    ap.set_defaults(samples=7)
    a = ap.parse_args()
    torch = benchlib.start(a, "policy_eval_bench")
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=SEED, timestep_limit=25, sep_nm=0.0)
        for K, hold in RUNS:
            r = measure(env, K, hold, a.samples)
            rows.append(r)
            e, c = r["eval"]["us_per_step"], r["collect"]["us_per_step"]
            print("%6d x %-2d T=%d K=%d hold=%-2d  eval %8.3f (%.3f - %.3f)  collect+fold %8.3f (%.3f - %.3f) us/step  ratio %.4f %s  episodes %d  fold %s" % (
                B, N, T, K, hold, e["median"], e["min"], e["max"], c["median"], c["min"], c["max"], r["ratio"], "SLOWER" if r["slower"] else "", r["episodes"],
                "matches" if r["fold_matches"] else "DIFFERS"), flush=True)
            torch.cuda.empty_cache()
        env.close()
    doc = {"what": "us per env step of evaluate_policy against rollout_policy_ends into preallocated buffers plus the torch fold of EPISODES, WINS and RETURN_SUM",
           "method": "HIP events around one variant's calls, variants alternating per sample in one process, 2 warm-up rounds, every sample from a fresh reset",
           "expectation": "no time is fixed: ratio = eval / collect, slower marks ratio > 1",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
