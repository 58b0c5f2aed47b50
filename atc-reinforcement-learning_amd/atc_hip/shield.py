"""An action shield on the policy's own continuation: the policy proposes M decisions per env (AtcVecEnv.act), each is flown on a copy of
the state for K steps and then CONTINUED BY THE POLICY for H - 1 further decisions inside one launch (AtcVecEnv.lookahead_policy,
include/atc_step.h: atc_lookahead_policy), and the best candidate that does not end badly is chosen.  Holding a candidate for the whole
horizon — lookahead(cand, H * K) — asks another question: an approach heading held a minute past the final approach fix is not what the
agent would fly, so that veto is pessimistic.  Nothing here steps the env: fly the choice with env.step_skip(chosen, K)."""
from . import layout as L


def discounted(seg_reward, gamma=1.0):
    """seg_reward [M, H, B] -> [M, B]: seg[:, 0] + gamma seg[:, 1] + gamma^2 seg[:, 2] + ... in float32, left to right, the discount a
    running product (atc_plan_score's order)"""
    score = seg_reward[:, 0].clone()
    g = 1.0
    for h in range(1, int(seg_reward.shape[1])):
        g = g * float(gamma)
        score = score + seg_reward[:, h] * g
    return score


def policy_shield(env, w, M, K, H, *, veto=L.F_CONFLICT | L.F_BELOW_MVA, seed=0, decision=0, gamma=1.0):
    """Per env: the best of M decisions drawn from the packed policy `w` that is not vetoed, each judged by what happens when it is held
    for K steps and the policy then takes the next H - 1 decisions (K steps each) from the observations the candidate is then in.
    A candidate is vetoed when a flag of `veto` was raised in any step it flew (default: lost separation or below the minimum vectoring
    altitude) or when it was not evaluated (n_steps == 0, a WIDE heading); its score is the discounted sum of its segment rewards.  Where
    every candidate of an env is vetoed the best-scoring one is taken.  The candidates are drawn with the rollout's key of `decision`, the
    continuation with decision + 1, decision + 2, ...: call t passes decision = t * H for draws no other call shares.
    Returns (chosen [B, N, 3] — what env.step_skip takes —, index [B] int64, the look-ahead's dict with "flags" and the candidates under
    "first").  The env is not stepped."""
    torch = env.torch
    cand = env.act(w, samples=int(M), seed=seed, decision=decision)
    look = env.lookahead_policy(w, K, H, first=cand, seed=seed, decision0=(int(decision) + 1) & 0xffffffff, outputs=("flags", "min_sep"))
    score = discounted(look["seg_reward"], gamma)
    bad = (look["flags"].int() & int(veto)).ne(0).any(dim=2) | look["n_steps"].eq(0)
    allowed = torch.where(bad, torch.full_like(score, float("-inf")), score)
    index = torch.where(bad.all(dim=0), score.argmax(dim=0), allowed.argmax(dim=0))
    chosen = cand.view(int(M), env.B, env.N, L.ACT_DIM)[index, torch.arange(env.B, device=index.device)]
    return chosen, index, dict(look, first=cand)
