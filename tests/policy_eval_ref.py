"""The per-env record of atc_policy_eval (include/atc_step.h) folded from the arrays of a rollout_policy_ends run, in numpy.

  initial(B)                                              the record under ATC_EVAL_CLEAR: zeros, RETURN_MIN / _MAX = +inf / -inf
  fold(reward, done, flags, t0, r0, record=None, ...)     [B, 16] int32: the launch's record, float words by bit pattern
      reward [T, B] float32, done [T, B], flags [T, B, N] uint16 as the rollout stores them; t0 / r0 [B]: each env's ATC_ENV_TIMESTEPS
      and ATC_ENV_TOTAL_REWARD before the run (the episode it is in counts in full); record: the carried-in record, None = cleared.
      float32 arithmetic in the header's order: total = total + reward per step, sum = sum + r, sq = sq + float32(r * r).
      dtype=np.float64: the same fold with every float in float64 (returns {"ints", "floats"}).
      returns=[]: appended to, one (env, length, r) per ending step in the order they are folded — r as the fold holds it.
  words(rec)                                              dict of the named words (floats as floats) of one record row or of [B, 16]

WINS from the flag arrays: under keep_active an end is a win iff an aircraft's word has F_WON at the ending step; otherwise iff no aircraft
is left under control — every aircraft of the episode has been handed over (F_WON at some step of it) or was not under control when the
launch began (mask0).  TEST INFRASTRUCTURE ONLY; needs no GPU."""
import numpy as np

WORDS = 16
(EPISODES, WINS, END_BELOW_MVA, END_OUTSIDE, END_CONFLICT, END_TIMEOUT, STEPS, RETURN_SUM, RETURN_SQ, RETURN_MIN, RETURN_MAX, FLAGS_OR,
 LAUNCH_STEPS) = range(13)
F_BELOW_MVA, F_OUTSIDE, F_WON, F_TIMEOUT, F_CONFLICT = 1, 2, 4, 8, 64
FLOAT_WORDS = (RETURN_SUM, RETURN_SQ, RETURN_MIN, RETURN_MAX)
NAMES = ("episodes", "wins", "end_below_mva", "end_outside", "end_conflict", "end_timeout", "steps", "return_sum", "return_sq", "return_min",
         "return_max", "flags_or", "launch_steps")


def initial(B):
    rec = np.zeros((B, WORDS), np.int32)
    f = rec.view(np.float32)
    f[:, RETURN_MIN] = np.inf
    f[:, RETURN_MAX] = -np.inf
    return rec


def fold(reward, done, flags, t0, r0, record=None, mask0=None, keep_active=False, dtype=np.float32, returns=None):
    reward, done = np.asarray(reward, np.float32), np.asarray(done) != 0
    flags = np.asarray(flags).view(np.uint16) if np.asarray(flags).dtype == np.int16 else np.asarray(flags).astype(np.uint16)
    T, B = done.shape
    N = flags.shape[2]
    full = (1 << N) - 1
    rec = initial(B) if record is None else np.array(record, dtype=np.int32).reshape(B, WORDS)
    ints = rec.astype(np.int64)
    fl = {w: rec.view(np.float32)[:, w].astype(dtype) for w in FLOAT_WORDS}
    for e in range(B):
        length, total = int(t0[e]), dtype(np.float32(r0[e]))
        mask = full if mask0 is None else int(mask0[e]) & full
        for t in range(T):
            length += 1
            total = dtype(total + dtype(reward[t, e]))
            seen = int(np.bitwise_or.reduce(flags[t, e]))
            ints[e, FLAGS_OR] |= seen
            won = 0
            for k in range(N):
                if flags[t, e, k] & F_WON:
                    won |= 1 << k
            if not keep_active:
                mask &= ~won
            if done[t, e]:
                r = total
                if returns is not None:
                    returns.append((e, length, r))
                ints[e, EPISODES] += 1
                ints[e, WINS] += int(won != 0 if keep_active else mask == 0)
                for word, bit in ((END_BELOW_MVA, F_BELOW_MVA), (END_OUTSIDE, F_OUTSIDE), (END_CONFLICT, F_CONFLICT), (END_TIMEOUT, F_TIMEOUT)):
                    ints[e, word] += int((seen & bit) != 0)
                ints[e, STEPS] += length
                fl[RETURN_SUM][e] = dtype(fl[RETURN_SUM][e] + r)
                fl[RETURN_SQ][e] = dtype(fl[RETURN_SQ][e] + dtype(r * r))
                fl[RETURN_MIN][e] = min(fl[RETURN_MIN][e], r)
                fl[RETURN_MAX][e] = max(fl[RETURN_MAX][e], r)
                length, total, mask = 0, dtype(0.0), full
        ints[e, LAUNCH_STEPS] += T
    if dtype is not np.float32:
        return {"ints": ints, "floats": fl}
    out = (ints & 0xffffffff).astype(np.uint32).view(np.int32)
    for w in FLOAT_WORDS:
        out.view(np.float32)[:, w] = fl[w]
    return out


def words(rec):
    rec = np.asarray(rec, np.int32)
    f = np.ascontiguousarray(rec).view(np.float32)
    return {n: (f[..., i] if i in FLOAT_WORDS else rec[..., i]) for i, n in enumerate(NAMES)}
