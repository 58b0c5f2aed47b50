"""Cross-entropy-method planning on AtcVecEnv's drawn-plan calls: the candidates of every iteration are drawn and scored inside one
launch (lookahead_plan_sampled), and only the elites are ever materialised (draw_plans(index=...))."""
import torch


def cem_plan(env, mean, std, K, M, iters, elites, gamma=1.0, seed=0):
    """`iters` CEM iterations of H-segment plans from the state `env` is in now (which is left as it is).

    env: AtcVecEnv with continuous actions.  mean, std: [H, B, N, 3] float tensors, the sampling distribution's start (std may be a
    python float).  K: steps a decision is held; M: plans drawn per env and iteration (1 .. 1024); elites: plans per env the refit
    keeps (1 .. M); iters >= 1 (ValueError otherwise).  gamma: discount per SEGMENT applied to seg_reward.  Iteration t draws with
    (seed, iteration=t), candidate 0 being the current mean, so an iteration never scores worse than the mean it started from.
    Returns (mean, std, best_first_decision): the refit distribution [H, B, N, 3] twice, and [B, N, 3], the first decision of the
    best plan of the last iteration — what to pass to env.step_skip(..., K)."""
    H, B, N = int(mean.shape[0]), env.B, env.N
    mean = torch.as_tensor(mean, dtype=torch.float32, device=env.device).reshape(H, B, N, 3).clone()
    std = (torch.full_like(mean, float(std)) if isinstance(std, (int, float))
           else torch.as_tensor(std, dtype=torch.float32, device=env.device).reshape(H, B, N, 3).clone())
    if int(iters) < 1:
        raise ValueError("iters >= 1 (there is no best plan before the first iteration)")
    if not 1 <= int(elites) <= int(M):
        raise ValueError("1 <= elites <= M")
    discount = torch.tensor([float(gamma) ** h for h in range(H)], dtype=torch.float32, device=env.device)
    best = None
    for t in range(int(iters)):
        seg = env.lookahead_plan_sampled(mean, std, K, M, seed=seed, iteration=t, mean_first=True, outputs=("seg_reward",))["seg_reward"]
        score = (seg * discount[None, :, None]).sum(1)                      # [M, B]
        elite_idx = score.topk(int(elites), dim=0).indices                  # [E, B], best first
        plans = env.draw_plans(mean, std, M, seed=seed, iteration=t, mean_first=True, index=elite_idx)   # [E, H, B, N, 3]
        best = plans[0, 0].clone()
        mean = plans.mean(0)
        std = plans.std(0, unbiased=False)
    return mean, std, best
