"""Developer measurement: what turning a collection's rewards, dones and values into advantages and returns costs as the torch recipe
— a Python loop backwards over the decisions — and what it costs as one launch.

    python tools/gae_bench.py [--out profiles/gae_bench.json] [--samples 7] [--quick] [--lib VARIANT.so]

For 8 192 x 16 and 65 536 x 16 (NV = N = 16: a per-aircraft critic), (D, hold) in {(1024, 1), (64, 20)}, rewards and values uniform in
[-3, 3], dones Bernoulli at 0.02 per step, gamma = 0.99, lam = 0.95:
  gae        (a) AtcVecEnv.gae into preallocated buffers (adv, ret and the three block outputs)
  torch_loop (b) the recipe a trainer writes in torch: for d = D - 1 .. 0 the block's fold over its `hold` steps (the discounted sum up to
                 the first done, the steps behind it masked out), then delta and the advantage, on [B] and [B, NV] tensors, into
                 preallocated adv / ret; it uses nothing of this library, so it runs unchanged on any commit
  bytes      (c) what (a) has to move — 4 (D + 1) C read, 8 D C written, 5 T B read — and that count over (a)'s median, in GB/s
A sample is the device time (HIP events) of one call; the variants take turns sample by sample after two warm-up rounds; reported are
median, quartiles, min and max in us per call.  No time is fixed in advance: `rows_slower` lists every row where (a)'s range (min ..
max) is not below (b)'s.  One JSON file; needs the GPU."""
import benchlib

CONFIGS = ((8192, 16), (65536, 16))
RUNS = ((1024, 1), (64, 20))
GAMMA, LAM, DONE_RATE = 0.99, 0.95, 0.02


def torch_recipe(torch, reward, done, values, hold, gamma, lam, adv, ret):
    """the reverse loop over D with the per-block fold, in stock torch ops"""
    D = values.shape[0] - 1
    G = gamma ** hold
    a_next = torch.zeros_like(values[0])
    for d in range(D - 1, -1, -1):
        t0 = d * hold
        R = reward[t0].clone()
        term = done[t0] != 0
        g = 1.0
        for j in range(1, hold):
            g *= gamma
            R = torch.where(term, R, R + reward[t0 + j] * g)
            term = term | (done[t0 + j] != 0)
        live = (~term).to(values.dtype)[:, None]
        delta = R[:, None] + G * values[d + 1] * live - values[d]
        a_next = delta + (G * lam) * live * a_next
        adv[d] = a_next
        ret[d] = a_next + values[d]


def measure(env, NV, D, hold, samples, seed=11):
    import torch
    B, dev = env.B, env.device
    T = D * hold
    gen = torch.Generator(device=dev).manual_seed(seed + D)
    reward = torch.rand((T, B), device=dev, generator=gen) * 6.0 - 3.0
    done = (torch.rand((T, B), device=dev, generator=gen) < DONE_RATE).to(torch.uint8)
    values = torch.rand((D + 1, B, NV), device=dev, generator=gen) * 6.0 - 3.0
    out = {"adv": torch.empty((D, B, NV), device=dev), "ret": torch.empty((D, B, NV), device=dev), "block_reward": torch.empty((D, B), device=dev),
           "block_done": torch.empty((D, B), dtype=torch.uint8, device=dev), "block_steps": torch.empty((D, B), dtype=torch.uint8, device=dev)}
    adv_t, ret_t = torch.empty_like(out["adv"]), torch.empty_like(out["ret"])
    calls = {"gae": lambda: env.gae(reward, done, values, hold=hold, gamma=GAMMA, lam=LAM, out=out),
             "torch_loop": lambda: torch_recipe(torch, reward, done, values, hold, GAMMA, LAM, adv_t, ret_t)}
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock)
    # the two compute the same thing (the recipe's operation order differs: values, not words)
    err = float((out["adv"] - adv_t).abs().max())
    C = B * NV
    moved = 4 * (D + 1) * C + 8 * D * C + 5 * T * B
    res = {"B": B, "NV": NV, "D": D, "hold": hold, "samples": samples, "bytes": moved, "max_abs_adv_difference": err}
    for v in calls:
        res[v] = {"us_per_call": benchlib.quartiles(times[v])}
    res["gae_gb_per_s"] = moved / res["gae"]["us_per_call"]["median"] / 1e3
    res["ratio_gae_vs_torch_loop"] = res["gae"]["us_per_call"]["median"] / res["torch_loop"]["us_per_call"]["median"]
    res["slower"] = not res["gae"]["us_per_call"]["max"] < res["torch_loop"]["us_per_call"]["min"]
    return res


def main():
    ap = benchlib.parser("gae_bench.json", quick="8 192 x 16 only")
    ap.set_defaults(samples=7)
    a = ap.parse_args()
    torch = benchlib.start(a, "gae_bench")
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    rows = []
    for B, N in (CONFIGS[:1] if a.quick else CONFIGS):
        env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=11, timestep_limit=6000, sep_nm=0.0)
        for D, hold in RUNS:
            r = measure(env, N, D, hold, a.samples)
            rows.append(r)
            print("%6d x %-2d D=%-4d hold=%-2d  (a) %9.1f us  (b) %11.1f us  (c) %6.2f MB -> %7.1f GB/s  ratio %.4f  max |adv - adv_torch| %.2e %s" % (
                B, N, D, hold, r["gae"]["us_per_call"]["median"], r["torch_loop"]["us_per_call"]["median"], r["bytes"] / 1e6, r["gae_gb_per_s"],
                r["ratio_gae_vs_torch_loop"], r["max_abs_adv_difference"], "SLOWER" if r["slower"] else ""), flush=True)
            torch.cuda.empty_cache()
        env.close()
    ident = lambda r: {k: r[k] for k in ("B", "NV", "D", "hold")}   # noqa: E731
    doc = {"what": "us per call: AtcVecEnv.gae into preallocated buffers | the torch recipe (reverse Python loop over D, the block fold in torch ops); "
                   "bytes: 4 (D+1) C read + 8 D C written + 5 T B read, and that count over gae's median (gae_gb_per_s)",
           "method": "HIP events around one call, variants alternating per sample, 2 warm-up rounds; median of `samples` with quartiles, min and max",
           "expectation": "no time is fixed: rows_slower lists the rows where gae's range (min .. max) is not below the torch recipe's",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows, "rows_slower": [ident(r) for r in rows if r["slower"]]}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
