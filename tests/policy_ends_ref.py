"""The three per-decision outputs of atc_rollout_policy_ends (include/atc_step.h) derived from a per-step rollout's arrays, in numpy.

  ending_steps(done, hold)                      t* [D, B]: the first step of block d with done set, -1 where the block has none
  term_flags(flags, done, hold)                 [D, B] uint16: 0, or TERM_ENDED | the OR of the env's N flag words at step t*
  control(mask0, flags, done, hold, N, ...)     [D, B, N] uint8: the aircraft's bit of the env's active mask in the state decision d is
                                                taken in — mask0 at launch; a step clears the bits of the aircraft it hands over (F_WON,
                                                unless keep_active); an auto-reset sets all N

TEST INFRASTRUCTURE ONLY; needs no GPU."""
import numpy as np

TERM_ENDED = 0x8000
F_WON, F_TIMEOUT = 4, 8
F_HARD = 1 | 2 | 64          # ATC_F_BELOW_MVA | ATC_F_OUTSIDE | ATC_F_CONFLICT


def ending_steps(done, hold):
    done = np.asarray(done) != 0
    T, B = done.shape
    D = T // hold
    blocks = done.reshape(D, hold, B)
    first = blocks.argmax(axis=1)
    return np.where(blocks.any(axis=1), np.arange(D)[:, None] * hold + first, -1)


def term_flags(flags, done, hold):
    flags = np.asarray(flags).astype(np.uint16)
    t_end = ending_steps(done, hold)
    D, B = t_end.shape
    out = np.zeros((D, B), np.uint16)
    for d in range(D):
        for e in range(B):
            if t_end[d, e] >= 0:
                out[d, e] = TERM_ENDED | np.bitwise_or.reduce(flags[t_end[d, e], e])
    return out


def truncated(tf):
    """a time-limit end: ATC_F_TIMEOUT set with the three hard ends clear"""
    tf = np.asarray(tf).astype(np.uint16)
    return (((tf & F_TIMEOUT) != 0) & ((tf & F_HARD) == 0)).astype(np.uint8)


def control(mask0, flags, done, hold, N, auto_reset=True, keep_active=False):
    """mask0: [B] python ints / uint64, the active masks at launch"""
    flags = np.asarray(flags).astype(np.uint16)
    done = np.asarray(done) != 0
    T, B = done.shape
    D = T // hold
    full = (1 << N) - 1
    mask = [int(m) & full for m in mask0]
    out = np.zeros((D, B, N), np.uint8)
    for t in range(T):
        if t % hold == 0:
            for e in range(B):
                out[t // hold, e] = [(mask[e] >> k) & 1 for k in range(N)]
        for e in range(B):
            if not keep_active:
                for k in range(N):
                    if flags[t, e, k] & F_WON:
                        mask[e] &= ~(1 << k)
            if done[t, e] and auto_reset:
                mask[e] = full
    return out
