"""How good is this policy?  Whole-episode statistics from AtcVecEnv.evaluate_policy (include/atc_step.h: atc_policy_eval), which flies a
packed policy inside the launch and stores nothing per step: what the reference's trainer logs after every update — winning_ratio, the
mean episode length, Monitor's r / l (learning/atc-gym-stable-baselines.py) — at training batch size.

    summary(record)                       the per-env records [B, L.EVAL_WORDS] folded into a dict of Python numbers
    evaluate(env, weights, ...)           evaluate_policy in chunks until every env has finished its episodes; returns (summary, record)

The fold is a few torch reductions over B x 64 bytes in int64 / float64: it needs no kernel."""
import math

from . import layout as L

END_CAUSES = (("below_mva", L.EVAL_END_BELOW_MVA), ("outside", L.EVAL_END_OUTSIDE), ("conflict", L.EVAL_END_CONFLICT), ("timeout", L.EVAL_END_TIMEOUT))


def summary(record):
    """record: int32 [B, L.EVAL_WORDS] as evaluate_policy returns it.  Over all envs together: episodes; win_ratio = wins / episodes;
    mean_return, std_return (population, from the sum and the sum of squares), min_return, max_return; mean_length; end_below_mva,
    end_outside, end_conflict, end_timeout as fractions of the episodes (an end can count in several); flags_or; steps = B times the
    steps flown.  With no finished episode the ratios and means are nan and min / max are +inf / -inf."""
    import torch
    rec = record.reshape(-1, L.EVAL_WORDS)
    ints = rec.to(torch.int64).sum(dim=0)
    f64 = rec.view(torch.float32).to(torch.float64)
    n = int(ints[L.EVAL_EPISODES])
    per = (lambda v: float(v) / n) if n else (lambda v: math.nan)
    s, sq = float(f64[:, L.EVAL_RETURN_SUM].sum()), float(f64[:, L.EVAL_RETURN_SQ].sum())
    mean = per(s)
    flags_or = 0
    for v in torch.unique(rec[:, L.EVAL_FLAGS_OR]).tolist():
        flags_or |= int(v) & 0xffffffff
    out = {"episodes": n, "win_ratio": per(int(ints[L.EVAL_WINS])), "mean_return": mean,
           "std_return": math.sqrt(max(per(sq) - mean * mean, 0.0)) if n else math.nan,
           "min_return": float(f64[:, L.EVAL_RETURN_MIN].min()), "max_return": float(f64[:, L.EVAL_RETURN_MAX].max()),
           "mean_length": per(int(ints[L.EVAL_STEPS]))}
    for name, word in END_CAUSES:
        out["end_" + name] = per(int(ints[word]))
    out["flags_or"] = flags_or
    out["steps"] = int(ints[L.EVAL_LAUNCH_STEPS])
    return out


def evaluate(env, weights, episodes_per_env=1, chunk=256, max_steps=None, traffic=0, hold=1, seed=0, decision0=0, deterministic=True):
    """evaluate_policy in chunks of `chunk` steps (rounded down to a multiple of hold, at least one decision) on one record, cleared by
    the first chunk only, decision0 advancing and each chunk's obs_last the next one's obs0 — so the chunks together are one launch of
    their total length, bit for bit.  Stops once every env has finished at least episodes_per_env episodes — one readback of
    record[:, L.EVAL_EPISODES].min() per chunk — or, with max_steps, before a chunk that would pass it.  Returns (summary(record), record)."""
    hold = int(hold)
    chunk = max(hold, int(chunk) // hold * hold)
    record, obs0, flown = None, None, 0
    while max_steps is None or flown + chunk <= int(max_steps):
        r = env.evaluate_policy(weights, chunk, traffic=traffic, hold=hold, seed=seed, decision0=int(decision0) + flown // hold, deterministic=deterministic,
                                obs0=obs0, record=record, clear=record is None)
        record, obs0 = r["record"], r["obs_last"]
        flown += chunk
        if int(record[:, L.EVAL_EPISODES].min()) >= int(episodes_per_env):
            break
    if record is None:
        raise ValueError("max_steps is less than one chunk of %d steps" % chunk)
    return summary(record), record
