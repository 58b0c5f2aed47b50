"""Sampling planners on AtcVecEnv's drawn-plan calls: the candidates of every iteration are drawn and scored inside one launch
(lookahead_plan_sampled) and the distribution is refit from per-candidate weights in another (refit_plans), so that nothing scales with
M * H * B * N.  cem_plan: the cross-entropy method with the elites materialised (draw_plans(index=...)); cem_plan_launch: the same
with the refit in a launch; mppi_plan: model-predictive path integral control, a softmax-weighted refit over all M candidates.
cem_plan_scored / mppi_plan_scored: the same two planners with the glue between the scoring and the refit — discount, ranking, weights,
winner — in a launch of its own (score_plans), so that an iteration is three launches, lookahead_plan_sampled -> score_plans ->
refit_plans, on buffers allocated once; their ranking is defined (ties to the lower candidate number) and leaves out candidates that
were not evaluated."""
import torch


def _start(env, mean, std):
    """mean and std of a planner's start as fresh [H, B, N, 3] float32 tensors on the env's device (std may be a python float)"""
    H, B, N = int(mean.shape[0]), env.B, env.N
    mean = torch.as_tensor(mean, dtype=torch.float32, device=env.device).reshape(H, B, N, 3).clone()
    std = (torch.full_like(mean, float(std)) if isinstance(std, (int, float))
           else torch.as_tensor(std, dtype=torch.float32, device=env.device).reshape(H, B, N, 3).clone())
    return H, mean, std


def cem_plan(env, mean, std, K, M, iters, elites, gamma=1.0, seed=0):
    """`iters` CEM iterations of H-segment plans from the state `env` is in now (which is left as it is).

    env: AtcVecEnv with continuous actions.  mean, std: [H, B, N, 3] float tensors, the sampling distribution's start (std may be a
    python float).  K: steps a decision is held; M: plans drawn per env and iteration (1 .. 1024); elites: plans per env the refit
    keeps (1 .. M); iters >= 1 (ValueError otherwise).  gamma: discount per SEGMENT applied to seg_reward.  Iteration t draws with
    (seed, iteration=t), candidate 0 being the current mean, so an iteration never scores worse than the mean it started from.
    The elites are materialised ([E, H, B, N, 3]) and their mean and std taken in torch; cem_plan_launch() is the same loop without
    that tensor.
    Returns (mean, std, best_first_decision): the refit distribution [H, B, N, 3] twice, and [B, N, 3], the first decision of the
    best plan of the last iteration — what to pass to env.step_skip(..., K)."""
    return _cem(env, mean, std, K, M, iters, elites, gamma, seed, "torch")


def cem_plan_launch(env, mean, std, K, M, iters, elites, gamma=1.0, seed=0):
    """cem_plan() with the refit done by env.refit_plans(): the elites get weight 1 and every other candidate 0, and no tensor of plans
    exists beyond the best one's [1, H, B, N, 3].  Arguments and results as cem_plan()'s; the two agree to rounding, not bit for bit
    (refit_plans sums about the clamped mean, in candidate order)."""
    return _cem(env, mean, std, K, M, iters, elites, gamma, seed, "launch")


def _cem(env, mean, std, K, M, iters, elites, gamma, seed, refit):
    H, mean, std = _start(env, mean, std)
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
        if refit == "launch":
            weight = torch.zeros_like(score).scatter_(0, elite_idx, 1.0)    # [M, B]: 1 for an env's elites
            best = env.draw_plans(mean, std, M, seed=seed, iteration=t, mean_first=True, index=elite_idx[:1])[0, 0].clone()
            mean, std = env.refit_plans(mean, std, M, weight, seed=seed, iteration=t, mean_first=True)
            continue
        plans = env.draw_plans(mean, std, M, seed=seed, iteration=t, mean_first=True, index=elite_idx)   # [E, H, B, N, 3]
        best = plans[0, 0].clone()
        mean = plans.mean(0)
        std = plans.std(0, unbiased=False)
    return mean, std, best


def mppi_plan(env, mean, std, K, M, iters, temperature, gamma=1.0, seed=0, std_min=0.0):
    """`iters` MPPI iterations of H-segment plans from the state `env` is in now (which is left as it is): every iteration draws and
    scores M plans per env in one launch, weighs candidate m of env e with exp((score - max over m) / temperature) — 0 where the
    candidate was not evaluated (n_steps == 0) — and refits mean and std from ALL M candidates with env.refit_plans(); no plan is
    materialised but the best one of the last iteration.

    env, mean, std, K, M, gamma, seed: as in cem_plan().  temperature > 0 and iters >= 1 (ValueError otherwise).  std_min: lower
    bound put on the refit std, so that a sharp softmax does not collapse the search.
    Returns (mean, std, best_first_decision): [H, B, N, 3] twice, and [B, N, 3], the first decision of the best-scoring plan of the
    last iteration."""
    H, mean, std = _start(env, mean, std)
    if int(iters) < 1:
        raise ValueError("iters >= 1 (there is no best plan before the first iteration)")
    if not float(temperature) > 0.0:
        raise ValueError("temperature > 0")
    discount = torch.tensor([float(gamma) ** h for h in range(H)], dtype=torch.float32, device=env.device)
    best = None
    for t in range(int(iters)):
        res = env.lookahead_plan_sampled(mean, std, K, M, seed=seed, iteration=t, mean_first=True, outputs=("seg_reward",))   # (n_steps: always)
        score = (res["seg_reward"] * discount[None, :, None]).sum(1)        # [M, B]
        weight = torch.exp((score - score.max(0).values) / float(temperature))
        weight = torch.where(res["n_steps"] == 0, torch.zeros_like(weight), weight)
        if t == int(iters) - 1:
            best = env.draw_plans(mean, std, M, seed=seed, iteration=t, mean_first=True, index=score.argmax(0)[None])[0, 0].clone()
        mean, std = env.refit_plans(mean, std, M, weight, seed=seed, iteration=t, mean_first=True, std_min=std_min)
    return mean, std, best


def _score_buffers(env, M, B):
    """score, weight and top of score_plans(top=1), allocated once for a whole planner call"""
    return {"score": torch.empty((M, B), dtype=torch.float32, device=env.device),
            "weight": torch.empty((M, B), dtype=torch.float32, device=env.device),
            "top": torch.empty((1, B), dtype=torch.int32, device=env.device)}


def _scored(env, mean, std, K, M, iters, gamma, seed, std_min, **how):
    H, mean, std = _start(env, mean, std)
    if int(iters) < 1:
        raise ValueError("iters >= 1 (there is no best plan before the first iteration)")
    buf = _score_buffers(env, int(M), env.B)
    best = None
    for t in range(int(iters)):
        res = env.lookahead_plan_sampled(mean, std, K, M, seed=seed, iteration=t, mean_first=True, outputs=("seg_reward",))   # (n_steps: always)
        env.score_plans(res["seg_reward"], n_steps=res["n_steps"], gamma=gamma, top=1, out=buf, **how)
        if t == int(iters) - 1:
            best = env.draw_plans(mean, std, M, seed=seed, iteration=t, mean_first=True, index=buf["top"][:1])[0, 0].clone()
        mean, std = env.refit_plans(mean, std, M, buf["weight"], seed=seed, iteration=t, mean_first=True, std_min=std_min)
    return mean, std, best


def cem_plan_scored(env, mean, std, K, M, iters, elites, gamma=1.0, seed=0):
    """cem_plan_launch() with everything between the scoring launch and the refit launch done by env.score_plans(): an iteration is
    lookahead_plan_sampled -> score_plans -> refit_plans, three launches on the env's stream, and the score / weight / top buffers are
    allocated once before the loop.  Arguments and results as cem_plan()'s.  It differs from the older loops in three ways:
    candidates that were NOT EVALUATED (n_steps == 0, a WIDE heading) and candidates whose score is not finite are left out of the
    elites (the older loops let their score of 0 compete); equal scores go to the LOWER candidate number (torch.topk does not say);
    the discount of segment h is the fp32 running product gamma * gamma * ... (the older loops round float(gamma) ** h once).  So the
    results agree with cem_plan_launch() only where none of that bites.  An env with no valid candidate keeps its mean and std, and its
    best_first_decision row is zero."""
    if not 1 <= int(elites) <= int(M):
        raise ValueError("1 <= elites <= M")
    return _scored(env, mean, std, K, M, iters, gamma, seed, 0.0, mode="elite", elites=int(elites))


def mppi_plan_scored(env, mean, std, K, M, iters, temperature, gamma=1.0, seed=0, std_min=0.0):
    """mppi_plan() with the softmax weights and the winner computed by env.score_plans(): an iteration is lookahead_plan_sampled ->
    score_plans -> refit_plans, three launches on the env's stream, and the score / weight / top buffers are allocated once before the
    loop.  Arguments and results as mppi_plan()'s.  It differs from mppi_plan() in three ways: candidates that were NOT EVALUATED or
    whose score is not finite are left out of the maximum and of the winner as well (mppi_plan() only zeroes the weight of the
    former); equal scores go to the LOWER candidate number; the discount of segment h is the fp32 running product (mppi_plan() rounds
    float(gamma) ** h once).  So the results agree with mppi_plan() only where none of that bites."""
    if not float(temperature) > 0.0:
        raise ValueError("temperature > 0")
    return _scored(env, mean, std, K, M, iters, gamma, seed, std_min, mode="softmax", temperature=float(temperature))
