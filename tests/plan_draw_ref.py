"""The draw of the drawn-plan calls (include/atc_step.h: atc_plan_draw, atc_lookahead_plan_sampled) restated in numpy: uint64 wraparound
for the keys, an exact integer sum, ONE float32 multiply, then mean + std * z with two float32 roundings and np.fmax / np.fmin (which
return the other operand for a NaN, like fmaxf / fminf).  TEST INFRASTRUCTURE ONLY; needs no GPU.

  mix64(z)                                  the 64-bit mixer of csrc/atc_device.h
  draw_sum(seed, iteration, m, h, i, c)     S, the Irwin-Hall integer 0 .. 262140 (arguments broadcast)
  draw_z(...)                               (float32)(S - 131070) * DRAW_SCALE
  draw(mean, std, M, ...)                   the plans [M, H, B, N, 3] (with index [E, B]: [E, H, B, N, 3])"""
import numpy as np

U64 = np.uint64
DRAW_SCALE_BITS = 0x37DDB3D7
DRAW_SCALE = np.array([DRAW_SCALE_BITS], np.uint32).view(np.float32)[0]     # 0x1.bb67aep-16
S_MID, S_MAX = 131070, 262140


def _u64(x):
    return np.asarray(x).astype(U64)


def mix64(z):
    with np.errstate(over="ignore"):
        z = _u64(z) + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def draw_sum(seed, iteration, m, h, i, c):
    cand = mix64(U64(int(seed) & (2 ** 64 - 1)) ^ ((_u64(iteration) << U64(32)) | _u64(m)))
    key = mix64(cand ^ ((_u64(h) << U64(32)) | _u64(i)))
    w = mix64(key ^ (_u64(c) + U64(1)))
    f = U64(0xffff)
    return ((w & f) + ((w >> U64(16)) & f) + ((w >> U64(32)) & f) + (w >> U64(48))).astype(np.int64)


def draw_z(seed, iteration, m, h, i, c):
    return (draw_sum(seed, iteration, m, h, i, c) - S_MID).astype(np.float32) * DRAW_SCALE


def clamp(a):
    return np.fmin(np.fmax(np.asarray(a, np.float32), np.float32(-1.0)), np.float32(1.0))


def draw(mean, std, M, seed=0, iteration=0, mean_first=True, index=None, into=None):
    """mean, std: [H, B, N, 3] float32 (std also a scalar).  index None: candidates 0 .. M-1.  index [E, B]: row r of env e is candidate
    index[r, e]; an env whose index is outside 0 .. M-1 keeps what `into` holds (zeros without `into`)."""
    mean = np.asarray(mean, np.float32)
    H, B, N, _ = mean.shape
    std = np.broadcast_to(np.asarray(std, np.float32), mean.shape)
    cand = np.arange(M)[:, None] if index is None else np.asarray(index).reshape(-1, B).astype(np.int64)       # [R, 1 or B]
    R = cand.shape[0]
    m = np.broadcast_to(cand[:, None, :, None, None], (R, H, B, N, 3))
    valid = (m >= 0) & (m < M)
    hh = np.arange(H)[None, :, None, None, None]
    i = (np.arange(B)[:, None] * N + np.arange(N)[None, :])[None, None, :, :, None]
    c = np.arange(3)[None, None, None, None, :]
    z = draw_z(seed, iteration, np.where(valid, m, 0), hh, i, c)
    a = clamp(mean[None] + std[None] * z)            # float32 product, float32 sum: two roundings
    if mean_first:
        a = np.where(m == 0, clamp(mean)[None], a)
    base = np.zeros((R, H, B, N, 3), np.float32) if into is None else np.asarray(into, np.float32).reshape(R, H, B, N, 3)
    return np.where(valid, a, base).astype(np.float32)
