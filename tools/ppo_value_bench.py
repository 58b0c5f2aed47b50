"""Developer measurement: the critic in the library (AtcVecEnv.value_forward: V of R rows in one launch; AtcVecEnv.ppo_value_grad: the clipped
value loss and its gradient in one call, no activation in memory) against the same network through torch in float32 on the device (DESIGN.md,
section 3p).

    python tools/ppo_value_bench.py [--out profiles/ppo_value_bench.json] [--samples 7] [--quick] [--lib VARIANT.so]

For R = 2^20 and 2^23 rows and K in {0, 4} records per aircraft (input rows of 10 and 38 words), weights N(0, 1 / fan_in), inputs uniform in
[-1, 1], v_old = V + N(0, 0.3), ret = V + N(0, 0.5), clip 0.2, no mask, no index:
  value_forward   (a) the call with out=
  torch_forward   (b) the same net as nn.Sequential under no_grad on the widened rows
  ppo_value_grad  (c) the call with out= (grad, stats, value and scratch preallocated), the library's own number of workgroups
  torch_autograd  (d) what a trainer writes: input_rows -> the nn.Sequential -> 0.5 maximum((v - ret)^2, (v_old + clamp(v - v_old) - ret)^2).mean()
                      -> backward()
A sample is the device time (HIP events) of one call; the variants take turns sample by sample after two warm-up rounds; reported are median,
quartiles, min and max in ms per call, and for each variant torch.cuda.max_memory_allocated over one call above what was allocated before it.
No time is fixed in advance: EVERY row is recorded and `rows_slower` lists the rows where a call's range (min .. max) is not below torch's.
One JSON file; needs the GPU."""
import benchlib

ROWS = (2 ** 20, 2 ** 23)
KS = (0, 4)
CLIP = 0.2


def measure(env, R, K, samples, seed=11):
    import torch
    from torch import nn
    from atc_hip import layout as L
    from atc_hip import policy, value
    dev = env.device
    torch.manual_seed(seed + K)
    gen = torch.Generator(device=dev).manual_seed(seed + K)
    n_in, words = L.policy_in(K), L.value_words(K)
    net = nn.Sequential(nn.Linear(n_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
    w = value.from_torch(net, device=dev, traffic=K)
    obs_rows = torch.rand((R, 10), device=dev, generator=gen) * 2.0 - 1.0
    traffic = torch.rand((R, K, 8), device=dev, generator=gen) * 2.0 - 1.0 if K else None
    widen = lambda: policy.input_rows(obs_rows.view(R, 1, 10), traffic.view(R, 1, K, 8)).view(R, n_in) if K else obs_rows      # noqa: E731
    x = widen().contiguous()
    with torch.no_grad():
        v = net(x)[:, 0]
        v_old = (v + 0.3 * torch.randn(R, device=dev, generator=gen)).contiguous()
        ret = (v + 0.5 * torch.randn(R, device=dev, generator=gen)).contiguous()
        del v
    G = L.ppo_grad_workgroups(R)
    values = torch.empty(R, device=dev)
    out = {"grad": torch.empty(words, device=dev), "stats": torch.empty(L.PPO_VALUE_STATS, device=dev), "value": torch.empty(R, device=dev),
           "scratch": torch.empty((G, words + L.PPO_VALUE_STATS), device=dev)}
    kept = {}

    def forward():
        env.value_forward(w, x, out=values)

    def torch_forward():
        with torch.no_grad():
            kept["v"] = net(x)[:, 0]

    def call():
        env.ppo_value_grad(w, obs_rows, v_old, ret, traffic=traffic, clip=CLIP, out=out)

    def autograd():
        for p in net.parameters():
            p.grad = None
        vv = net(widen())[:, 0]
        vc = v_old + torch.clamp(vv - v_old, -CLIP, CLIP)
        (0.5 * torch.maximum((vv - ret) ** 2, (vc - ret) ** 2)).mean().backward()
    calls = {"value_forward": forward, "torch_forward": torch_forward, "ppo_value_grad": call, "torch_autograd": autograd}
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock)
    lin = list(net)[0::2]
    g_t = torch.cat([p.grad.reshape(-1) for m in lin for p in (m.weight, m.bias)])
    res = {"R": R, "K": K, "input_words": n_in, "workgroups": G, "samples": samples,
           "max_grad_difference_over_largest_word": float((out["grad"] - g_t).abs().max() / g_t.abs().max()),
           "max_value_difference": float((values - kept["v"]).abs().max()), "stats": [float(s) for s in out["stats"].cpu()]}
    kept.clear()
    for name, fn in calls.items():
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize(dev)
        kept.clear()
        t = [s / 1000.0 for s in times[name]]
        res[name] = {"ms_per_call": benchlib.quartiles(t), "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated(dev) - base)}
    for mine, theirs, key in (("value_forward", "torch_forward", "forward"), ("ppo_value_grad", "torch_autograd", "grad")):
        res["ratio_%s_vs_torch" % key] = res[mine]["ms_per_call"]["median"] / res[theirs]["ms_per_call"]["median"]
        res["%s_ns_per_row" % key] = res[mine]["ms_per_call"]["median"] * 1e6 / R
        res["%s_slower" % key] = not res[mine]["ms_per_call"]["max"] < res[theirs]["ms_per_call"]["min"]
    return res


def main():
    ap = benchlib.parser("ppo_value_bench.json", quick="2^20 rows only")
    ap.set_defaults(samples=7)
    a = ap.parse_args()
    torch = benchlib.start(a, "ppo_value_bench")
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    env = AtcVecEnv(4, 1, scenario=scenarios.LOWWDense(), auto_reset=True, seed=11)      # (the calls need an env for its device and stream only)
    rows = []
    for R in (ROWS[:1] if a.quick else ROWS):
        for K in KS:
            r = measure(env, R, K, a.samples)
            rows.append(r)
            for mine, theirs, key in (("value_forward", "torch_forward", "forward"), ("ppo_value_grad", "torch_autograd", "grad")):
                print("R = %8d  K = %d  %-14s %9.3f ms, %6.1f MB   torch %9.3f ms, %8.1f MB   ratio %.3f  %5.1f ns per row %s" % (
                    R, K, mine, r[mine]["ms_per_call"]["median"], r[mine]["peak_bytes_above_inputs"] / 1e6, r[theirs]["ms_per_call"]["median"],
                    r[theirs]["peak_bytes_above_inputs"] / 1e6, r["ratio_%s_vs_torch" % key], r["%s_ns_per_row" % key], "SLOWER" if r["%s_slower" % key] else ""), flush=True)
            print("          grad difference over the largest word %.2e, largest value difference %.2e" % (r["max_grad_difference_over_largest_word"], r["max_value_difference"]),
                  flush=True)
            torch.cuda.empty_cache()
    env.close()
    doc = {"what": "ms per call and peak bytes allocated during a call: AtcVecEnv.value_forward | the same nn.Sequential under no_grad; "
                   "AtcVecEnv.ppo_value_grad with out= | the same loss through torch autograd; all float32",
           "method": "HIP events around one call, variants alternating per sample, 2 warm-up rounds; median of `samples` with quartiles, min and max; "
                     "peak = torch.cuda.max_memory_allocated over one further call minus memory_allocated before it",
           "expectation": "no time is fixed: every row is recorded, rows_slower lists the rows where a call's range (min .. max) is not below torch's",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows,
           "rows_slower": [{"R": r["R"], "K": r["K"], "call": key} for r in rows for key in ("forward", "grad") if r["%s_slower" % key]]}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
