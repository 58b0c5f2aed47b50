"""Developer measurement: one PPO update on a collection through atc_hip.ppo.update (advantages normalised by atc_adv_normalise, per minibatch
the two gradient calls and one atc_adam_step on both packed tensors) against the loop a trainer wrote before it: ppo.policy_grad(normalise=True)
— three torch reductions and two host reads per minibatch —, ppo.value_grad, the entropy term and clip_grad_norm_ over both tensors in torch,
and two torch.optim.Adam steps.

    python tools/ppo_update_bench.py [--out profiles/ppo_update_bench.json] [--samples 7] [--quick] [--lib VARIANT.so]

For B x N = 4 096 x 16 and 65 536 x 16 envs, D = 8 decisions (collect_bootstrap, T = 8, hold 1), 4 epochs of 4 and of 32 minibatches, both sides
on the same collection with the same permutations, clip 0.2, lr 3e-4, ent_coef 0.01, vf_coef 0.5, max_grad_norm 0.5:
  update        (a) ppo.update with the state of ppo.adam_state (every buffer kept from call to call)
  torch_loop    (b) the loop above
  adv_normalise (c) env.adv_normalise with out= on the collection's advantages and control mask
  torch_moments (d) adv[control.bool()] -> mean, std, (adv - mean) / (std + 1e-8), the two scalars read on the host as policy_grad does
A sample is the device time (HIP events) of one call, which contains the host's share wherever the device waits for it; the variants take turns
sample by sample after two warm-up rounds; reported are median, quartiles, min and max in ms per call, the library calls of one call (launch
records) and torch.cuda.max_memory_allocated over one call above what was allocated before it.  No time is fixed in advance: EVERY row is
recorded and `rows_slower` lists the rows where a call's range (min .. max) is not below the torch side's.  One JSON file; needs the GPU."""
import benchlib

SHAPES = ((4096, 16), (65536, 16))
D = 8
EPOCHS = 4
MINIBATCHES = (4, 32)
HP = dict(clip=0.2, vclip=0.2, lr=3e-4, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, eps=1e-5)


def _moved(before, after):
    return {g: {str(k): v - before[g].get(k, 0) for k, v in after[g].items() if v != before[g].get(k, 0)} for g in after
            if any(v != before[g].get(k, 0) for k, v in after[g].items())}


def measure(torch, B, N, samples, quick, seed=11):
    from torch import nn
    from atc_hip import layout as L
    from atc_hip import lib, policy, ppo, value
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=seed)
    dev = env.device
    torch.manual_seed(seed)
    mlp = lambda out: nn.Sequential(nn.Linear(10, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, out))      # noqa: E731
    w0 = policy.from_torch(mlp(3), torch.full((3,), -0.5), device=dev)
    vw0 = value.from_torch(mlp(1), device=dev)
    res = ppo.collect_bootstrap(env, w0, ppo.critic(env, vw0), T=D, hold=1, seed=seed)
    res = dict(res, obs0=env._collected_obs0[1])
    R = D * B * N
    log_std = policy.offsets(0)["log_std"][0]
    rows = []
    control = res["control"]
    adv = res["adv"]
    abuf = {"adv": torch.empty_like(adv), "stats": torch.empty(L.ADV_STATS, device=dev), "scratch": torch.empty((L.adv_workgroups(R), 3), dtype=torch.float64, device=dev)}
    kept = {}

    def adv_normalise():
        env.adv_normalise(adv, control, out=abuf)

    def torch_moments():
        a = adv[control.bool()]
        shift, scale = float(a.mean()), float(1.0 / (a.std() + 1e-8))
        kept["adv"] = (adv - shift) * scale

    for M in (MINIBATCHES[:1] if quick else MINIBATCHES):
        gen = torch.Generator(device=dev).manual_seed(seed + M)
        perm = torch.stack([torch.randperm(R, generator=gen, device=dev) for _ in range(EPOCHS)]).to(torch.int32)
        w1, vw1 = w0.clone(), vw0.clone()
        state = ppo.adam_state(env, w1, vw1)
        w2, vw2 = w0.clone().requires_grad_(True), vw0.clone().requires_grad_(True)
        opt, vopt = torch.optim.Adam([w2], lr=HP["lr"], eps=HP["eps"]), torch.optim.Adam([vw2], lr=HP["lr"], eps=HP["eps"])

        def update():
            ppo.update(env, res, w1, vw1, state, epochs=EPOCHS, minibatches=M, perm=perm, **HP)

        def torch_loop():
            for e in range(EPOCHS):
                for k in range(M):
                    mb = perm[e][k * R // M:(k + 1) * R // M]
                    g = ppo.policy_grad(env, res, w2.detach(), index=mb, clip=HP["clip"])
                    v = ppo.value_grad(env, res, vw2.detach(), index=mb, clip=HP["vclip"])
                    w2.grad = g["grad"]
                    w2.grad[log_std:] -= HP["ent_coef"]
                    vw2.grad = v["grad"] * HP["vf_coef"]
                    nn.utils.clip_grad_norm_([w2, vw2], HP["max_grad_norm"])
                    opt.step()
                    vopt.step()
        calls = {"update": update, "torch_loop": torch_loop}
        if M == MINIBATCHES[0]:
            calls.update(adv_normalise=adv_normalise, torch_moments=torch_moments)
        clock = benchlib.hip_clock(torch, torch.cuda.current_stream(dev))
        times = benchlib.sample(calls, samples, 1, clock)
        row = {"B": B, "N": N, "D": D, "rows": R, "controlled_rows": int(control.sum()), "epochs": EPOCHS, "minibatches": M, "samples": samples,
               "max_weight_difference": float((w1 - w2.detach()).abs().max()), "max_critic_difference": float((vw1 - vw2.detach()).abs().max())}
        for name, fn in calls.items():
            torch.cuda.synchronize(dev)
            kept.clear()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            before = lib.launch_records()
            fn()
            torch.cuda.synchronize(dev)
            t = [s / 1000.0 for s in times[name]]
            row[name] = {"ms_per_call": benchlib.quartiles(t), "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated(dev) - base),
                         "library_calls": _moved(before, lib.launch_records())}
        pairs = [("update", "torch_loop")] + ([("adv_normalise", "torch_moments")] if "adv_normalise" in calls else [])
        for mine, theirs in pairs:
            row["ratio_%s_vs_torch" % mine] = row[mine]["ms_per_call"]["median"] / row[theirs]["ms_per_call"]["median"]
            row["%s_slower" % mine] = not row[mine]["ms_per_call"]["max"] < row[theirs]["ms_per_call"]["min"]
            print("%6d x %2d  M = %2d  %-13s %9.3f ms, %7.1f MB   %-13s %9.3f ms, %7.1f MB   ratio %.3f %s" % (
                B, N, M, mine, row[mine]["ms_per_call"]["median"], row[mine]["peak_bytes_above_inputs"] / 1e6, theirs, row[theirs]["ms_per_call"]["median"],
                row[theirs]["peak_bytes_above_inputs"] / 1e6, row["ratio_%s_vs_torch" % mine], "SLOWER" if row["%s_slower" % mine] else ""), flush=True)
        rows.append(row)
        kept.clear()
    env.close()
    return rows


def main():
    ap = benchlib.parser("ppo_update_bench.json", quick="4 096 x 16 and 4 minibatches only")
    ap.set_defaults(samples=7)
    a = ap.parse_args()
    torch = benchlib.start(a, "ppo_update_bench")
    rows = []
    for B, N in (SHAPES[:1] if a.quick else SHAPES):
        rows += measure(torch, B, N, a.samples, a.quick)
        torch.cuda.empty_cache()
    doc = {"what": "ms per call, library calls and peak bytes allocated during a call: atc_hip.ppo.update | the torch loop it replaces (policy_grad(normalise=True), "
                   "value_grad, entropy term, clip_grad_norm_, two torch.optim.Adam steps); AtcVecEnv.adv_normalise | the three torch reductions",
           "method": "HIP events around one call, variants alternating per sample, 2 warm-up rounds; median of `samples` with quartiles, min and max; "
                     "peak = torch.cuda.max_memory_allocated over one further call minus memory_allocated before it; the weights keep moving from sample to sample on both sides",
           "expectation": "no time is fixed: every row is recorded, rows_slower lists the rows where a call's range (min .. max) is not below the torch side's",
           "box": benchlib.box(torch), "library": a.lib or "in-tree build", "rows": rows,
           "rows_slower": [{"B": r["B"], "minibatches": r["minibatches"], "call": k} for r in rows for k in ("update", "adv_normalise") if r.get("%s_slower" % k)]}
    benchlib.write_json(a.out, doc)


if __name__ == "__main__":
    main()
