"""The fold that turns a policy rollout's per-step arrays on a child batch into atc_lookahead_policy's per-candidate outputs (include/atc_step.h):
column c of reward / done [T, C] is one candidate flown for T = H * K steps; the plan is CUT at the column's first done, the segments it did not
run are zero, and the sums are sequential float32 additions at two levels — a segment's steps, then the segments (acc = r_0; acc = acc + r_1;
...: a first term is assigned, so a -0 stays a -0).  numpy only."""
import numpy as np


def first_done(done):
    """n [C]: steps each column runs — up to and including its first done, T without one"""
    done = np.asarray(done).astype(bool)
    T = done.shape[0]
    return np.where(done.any(axis=0), done.argmax(axis=0) + 1, T).astype(np.int64)


def fold(reward, done, K, H):
    """reward float32 [T, C], done [T, C], T == H * K -> dict(seg_reward float32 [H, C], reward float32 [C], done uint8 [C], n_steps int64 [C])"""
    reward = np.asarray(reward, np.float32)
    done = np.asarray(done).astype(bool)
    T, C = reward.shape
    assert T == H * K and done.shape == (T, C)
    n = first_done(done)
    seg = np.zeros((H, C), np.float32)
    total = np.zeros(C, np.float32)
    for h in range(H):
        acc = np.zeros(C, np.float32)
        for j in range(K):
            t = h * K + j
            run = t < n
            acc = np.where(run, reward[t] if j == 0 else (acc + reward[t]).astype(np.float32), acc).astype(np.float32)
        ran = h * K < n      # the segment has at least one step
        seg[h] = np.where(ran, acc, np.float32(0.0))
        total = np.where(ran, seg[h] if h == 0 else (total + seg[h]).astype(np.float32), total).astype(np.float32)
    return dict(seg_reward=seg, reward=total, done=done[n - 1, np.arange(C)].astype(np.uint8), n_steps=n)


def fold64(reward, done, K, H):
    """the same cut and padding with float64 sums: what the float32 fold is held to"""
    reward = np.asarray(reward, np.float64)
    n = first_done(done)
    T, C = reward.shape
    run = np.arange(T)[:, None] < n[None, :]
    seg = np.where(run, reward, 0.0).reshape(H, K, C).sum(axis=1)
    return dict(seg_reward=seg, reward=seg.sum(axis=0), n_steps=n)


def or_flags(flags, n):
    """flags [T, C, N] (any integer dtype) -> uint16 [C, N]: the OR over each column's first n[c] steps"""
    f = np.asarray(flags).astype(np.int64) & 0xffff
    run = np.arange(f.shape[0])[:, None, None] < np.asarray(n)[None, :, None]
    return np.bitwise_or.reduce(np.where(run, f, 0), axis=0).astype(np.uint16)


def last_rows(rows, n):
    """rows [T, C, ...] -> [C, ...]: row n[c] - 1 of column c"""
    rows = np.asarray(rows)
    return rows[np.asarray(n) - 1, np.arange(rows.shape[1])]


def discounted(seg_reward, gamma):
    """seg_reward [..., H, C] -> float64 [..., C]: sum_h gamma^h seg[h]"""
    seg = np.asarray(seg_reward, np.float64)
    H = seg.shape[-2]
    return (seg * (float(gamma) ** np.arange(H))[:, None]).sum(axis=-2)
