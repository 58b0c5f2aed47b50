"""Developer measurement: the PPO policy loss and its gradient as ONE call (AtcVecEnv.ppo_policy_grad: forward, loss and backward per row
inside a workgroup, no activation in memory) against the same loss through torch autograd in float32 on the device.

    python tools/ppo_grad_bench.py [--out profiles/ppo_grad_bench.json] [--samples 7] [--quick] [--lib VARIANT.so]

For R = 2^20 and 2^23 rows and K in {0, 4} records per aircraft (input rows of 10 and 38 words), weights N(0, 1 / fan_in), inputs uniform
in [-1, 1], actions mu + sigma z, ratios spread over [0.5, 2], advantages N(0, 1), clip 0.2, no mask, no index:
  ppo_policy_grad (a) the call with out= (grad, stats, logp and scratch preallocated), the library's own number of workgroups
  torch_autograd  (b) what a trainer writes: input_rows -> Linear / tanh / Linear / tanh / Linear on the unpacked weights -> logp -> ratio ->
                      -min(ratio A, clamp(ratio) A).mean() -> backward(); it uses nothing of this library but the packed layout
A sample is the device time (HIP events) of one call; the variants take turns sample by sample after two warm-up rounds; reported are
median, quartiles, min and max in ms per call, and for each variant torch.cuda.max_memory_allocated over one call above what was allocated
before it.  At 2^20 rows both gradients are also compared with the loss through autograd in float64 (largest difference over the largest
gradient word).  No time is fixed in advance: EVERY row is recorded and `rows_slower` lists the rows where (a)'s range (min .. max) is not below
(b)'s.  One JSON file; needs the GPU."""
import benchlib

ROWS = (2 ** 20, 2 ** 23)
KS = (0, 4)
CLIP = 0.2
CHECK_ROWS = 2 ** 20      # up to here both gradients are also compared with float64 autograd


def torch_loss(torch, parts, x, action, logp_old, adv, clip):
    h = torch.tanh(torch.nn.functional.linear(x, parts["W1"], parts["b1"]))
    h = torch.tanh(torch.nn.functional.linear(h, parts["W2"], parts["b2"]))
    mu = torch.nn.functional.linear(h, parts["W3"], parts["b3"])
    d = (action - mu) / torch.exp(parts["log_std"])
    logp = (-0.5 * d * d - parts["log_std"]).sum(-1) - 2.7568155996140185
    ratio = torch.exp(logp - logp_old)
    return -torch.minimum(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv).mean()


def measure(env, R, K, samples, seed=11):
    import torch
    from atc_hip import layout as L
    from atc_hip import policy
    dev = env.device
    gen = torch.Generator(device=dev).manual_seed(seed + K)
    n_in, words = L.policy_in(K), L.policy_words(K)
    shapes = policy.shapes(K)
    init = [torch.randn(s, device=dev, generator=gen) / (s[1] ** 0.5 if len(s) == 2 else 10.0) for _, s in shapes[:-1]] + [torch.full((3,), -0.5, device=dev)]
    w = policy.pack_mlp(*init, device=dev, traffic=K)
    obs_rows = torch.rand((R, 10), device=dev, generator=gen) * 2.0 - 1.0
    traffic = torch.rand((R, K, 8), device=dev, generator=gen) * 2.0 - 1.0 if K else None
    offs = policy.offsets(K)
    parts = {name: w[at:at + int(torch.tensor(shape).prod())].view(shape).clone().requires_grad_(True) for name, (at, shape) in offs.items()}
    with torch.no_grad():
        x = policy.input_rows(obs_rows.view(R, 1, 10), traffic.view(R, 1, K, 8)).view(R, n_in) if K else obs_rows
        h = torch.tanh(torch.tanh(x @ parts["W1"].T + parts["b1"]) @ parts["W2"].T + parts["b2"])
        mu = h @ parts["W3"].T + parts["b3"]
        z = torch.randn((R, 3), device=dev, generator=gen)
        action = (mu + torch.exp(parts["log_std"]) * z).contiguous()
        logp = (-0.5 * z * z - parts["log_std"]).sum(-1) - 2.7568155996140185
        logp_old = (logp - (torch.rand(R, device=dev, generator=gen) * 2.0 - 1.0) * 0.6931).contiguous()
        adv = torch.randn(R, device=dev, generator=gen)
        del x, h, mu, z, logp
    G = L.ppo_grad_workgroups(R)
    out = {"grad": torch.empty(words, device=dev), "stats": torch.empty(L.PPO_GRAD_STATS, device=dev), "logp": torch.empty(R, device=dev),
           "scratch": torch.empty((G, words + L.PPO_GRAD_STATS), device=dev)}

    def call():
        env.ppo_policy_grad(w, obs_rows, action, logp_old, adv, traffic=traffic, clip=CLIP, out=out)

    def autograd():
        for p in parts.values():
            p.grad = None
        xin = policy.input_rows(obs_rows.view(R, 1, 10), traffic.view(R, 1, K, 8)).view(R, n_in) if K else obs_rows
        torch_loss(torch, parts, xin, action, logp_old, adv, CLIP).backward()
    calls = {"ppo_policy_grad": call, "torch_autograd": autograd}
    clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
    times = benchlib.sample(calls, samples, 1, clock)
    # the two compute the same thing: largest difference of the gradients over the largest gradient word
    g_t = torch.cat([parts[name].grad.reshape(-1) for name, _ in shapes])
    rel = float((out["grad"] - g_t).abs().max() / g_t.abs().max())
    res = {"R": R, "K": K, "input_words": n_in, "workgroups": G, "samples": samples, "max_grad_difference_over_largest_word": rel,
           "stats": [float(v) for v in out["stats"].cpu()]}
    if R <= CHECK_ROWS:      # which of the two is closer to the same loss through autograd in float64
        p64 = {k: v.detach().double().requires_grad_(True) for k, v in parts.items()}
        xin = (policy.input_rows(obs_rows.view(R, 1, 10), traffic.view(R, 1, K, 8)).view(R, n_in) if K else obs_rows).double()
        torch_loss(torch, p64, xin, action.double(), logp_old.double(), adv.double(), float(torch.tensor(CLIP, dtype=torch.float32))).backward()
        g64 = torch.cat([p64[name].grad.reshape(-1) for name, _ in shapes])
        top = g64.abs().max()
        res["against_float64_autograd"] = {"ppo_policy_grad": float((out["grad"].double() - g64).abs().max() / top),
                                           "torch_autograd_float32": float((g_t.double() - g64).abs().max() / top)}
        del p64, xin, g64
    for v, fn in calls.items():
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize(dev)
        t = [x / 1000.0 for x in times[v]]
        res[v] = {"ms_per_call": benchlib.quartiles(t), "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated(dev) - base)}
    res["ratio_call_vs_autograd"] = res["ppo_policy_grad"]["ms_per_call"]["median"] / res["torch_autograd"]["ms_per_call"]["median"]
    res["ns_per_row"] = res["ppo_policy_grad"]["ms_per_call"]["median"] * 1e6 / R
    res["slower"] = not res["ppo_policy_grad"]["ms_per_call"]["max"] < res["torch_autograd"]["ms_per_call"]["min"]
    return res


def main():
    ap = benchlib.parser("ppo_grad_bench.json", quick="2^20 rows only")
    ap.set_defaults(samples=7)
    a = ap.parse_args()
    torch = benchlib.start(a, "ppo_grad_bench")
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    env = AtcVecEnv(4, 1, scenario=scenarios.LOWWDense(), auto_reset=True, seed=11)      # (the call needs an env for its device and stream only)
    rows = []
    for R in (ROWS[:1] if a.quick else ROWS):
        for K in KS:
            r = measure(env, R, K, a.samples)
            rows.append(r)
            if "against_float64_autograd" in r:
                print("          against float64 autograd, over its largest word: the call %.2e, float32 autograd %.2e" % (
                    r["against_float64_autograd"]["ppo_policy_grad"], r["against_float64_autograd"]["torch_autograd_float32"]))
            print("R = %8d  K = %d  (a) %9.3f ms, %6.1f MB   (b) %9.3f ms, %8.1f MB   ratio %.3f  %5.1f ns per row  grad difference %.2e %s" % (
                R, K, r["ppo_policy_grad"]["ms_per_call"]["median"], r["ppo_policy_grad"]["peak_bytes_above_inputs"] / 1e6,
                r["torch_autograd"]["ms_per_call"]["median"], r["torch_autograd"]["peak_bytes_above_inputs"] / 1e6, r["ratio_call_vs_autograd"], r["ns_per_row"],
                r["max_grad_difference_over_largest_word"], "SLOWER" if r["slower"] else ""), flush=True)
            torch.cuda.empty_cache()
    env.close()
    doc = {"what": "ms per call and peak bytes allocated during a call: AtcVecEnv.ppo_policy_grad with out= | the same loss through torch autograd in float32",
           "method": "HIP events around one call, variants alternating per sample, 2 warm-up rounds; median of `samples` with quartiles, min and max; "
                     "peak = torch.cuda.max_memory_allocated over one further call minus memory_allocated before it",
           "expectation": "no time is fixed: every row is recorded, rows_slower lists the rows where the call's range (min .. max) is not below autograd's",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows,
           "rows_slower": [{"R": r["R"], "K": r["K"]} for r in rows if r["slower"]]}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
