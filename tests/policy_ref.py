"""The decision of the policy rollout (include/atc_step.h: atc_rollout_policy) restated in numpy: the key and u1 / u2 in exact integers,
z, the MLP and logp in float64, and a second MLP evaluation in plain float32 numpy (what two correct fp32 evaluations may differ by).
TEST INFRASTRUCTURE ONLY; needs no GPU.

  split(w, K)                    the seven parts of the packed array, as float arrays [out, in]
  key(seed, decision, i)         the 64-bit key of (decision, aircraft slot); arguments broadcast
  uniforms(seed, decision, i, c) (n1, n2): u1 = n1 2^-24 with n1 in 1 .. 2^24, u2 = n2 2^-24 with n2 in 0 .. 2^24 - 1, exact integers
  z64(...)                       sqrt(-2 log u1) cos(2 pi u2) in float64
  mlp(w, x, K, dtype)            mu [.., 3] of rows x [.., 10 + 7 K] evaluated in `dtype`
  logp64(z, log_std)             sum_c (-0.5 z_c^2 - log_std_c) - 1.5 log(2 pi)
  clamp(u)                       fminf(fmaxf(u, -1), 1): a NaN gives -1

K (default 0) is the number of traffic records in the input row (atc_rollout_policy_traffic: 10 + 7 K words, tests/policy_traffic_ref.py
builds the rows); only the first layer's width depends on it.

THE BARS (derived in the issue that introduced the call; the measured figures are in DESIGN.md section 3k):
  Z_BAR     |z_kernel - z64| <= 2e-5: logf and cosf good to <= 2 ulp, the fp32 rounding of the argument 2 pi u2 <= 4e-7, amplitude <= 5.77:
            together under 1e-5, with a factor 2 of margin.
  mu_bar    4 x the largest deviation of the float32-numpy MLP from the float64 one on the same inputs, with a floor of 1e-6: summation
            order and tanh differ between two correct fp32 evaluations by a small multiple of one of them.
  LOGP_BAR  |logp_kernel - logp64| <= 4e-5: at most eight fp32 roundings of magnitudes <= 64."""
import numpy as np

from plan_draw_ref import U64, _u64, mix64

IN, HIDDEN, ACT, WORDS = 10, 64, 3, 5062
SHAPES = (("W1", (HIDDEN, IN)), ("b1", (HIDDEN,)), ("W2", (HIDDEN, HIDDEN)), ("b2", (HIDDEN,)), ("W3", (ACT, HIDDEN)), ("b3", (ACT,)),
          ("log_std", (ACT,)))
RECORD_INPUTS = 7          # words 0..6 of a traffic record are inputs; word 7 (the slot) is stored only
Z_BAR = 2e-5
LOGP_BAR = 4e-5
MU_FLOOR = 1e-6
Z_MAX = 5.77          # sqrt(-2 log 2^-24) = 5.768
LOGP_C = 1.5 * np.log(2.0 * np.pi)


def n_in(K=0):
    return IN + RECORD_INPUTS * K


def words(K=0):
    return WORDS + HIDDEN * RECORD_INPUTS * K


def shapes(K=0):
    return (("W1", (HIDDEN, n_in(K))),) + SHAPES[1:]


def split(w, K=0):
    w = np.asarray(w).reshape(-1)
    assert w.size == words(K)
    parts, at = {}, 0
    for name, shape in shapes(K):
        n = int(np.prod(shape))
        parts[name] = w[at:at + n].reshape(shape)
        at += n
    return parts


def pack(W1, b1, W2, b2, W3, b3, log_std, K=0):
    parts = [np.asarray(v, np.float32) for v in (W1, b1, W2, b2, W3, b3, log_std)]
    for (name, shape), v in zip(shapes(K), parts):
        assert v.shape == shape, name
    return np.concatenate([v.reshape(-1) for v in parts])


def key(seed, decision, i):
    d = _u64(np.asarray(decision).astype(np.int64) & 0xffffffff)        # decision0 + b wraps modulo 2^32
    return mix64(mix64(U64(int(seed) & (2 ** 64 - 1)) ^ d) ^ _u64(i))


def uniforms(seed, decision, i, c):
    w = mix64(key(seed, decision, i) ^ (_u64(c) + U64(1)))
    n1 = (w >> U64(40)).astype(np.int64) + 1
    n2 = ((w >> U64(16)) & U64(0xffffff)).astype(np.int64)
    return n1, n2


def z64(seed, decision, i, c):
    n1, n2 = uniforms(seed, decision, i, c)
    u1, u2 = n1.astype(np.float64) * 2.0 ** -24, n2.astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def mlp(w, x, K=0, dtype=np.float64):
    p = {k: v.astype(dtype) for k, v in split(w, K).items()}
    x = np.asarray(x).astype(dtype)
    assert x.shape[-1] == n_in(K)
    with np.errstate(all="ignore"):
        h1 = np.tanh(x @ p["W1"].T + p["b1"])
        h2 = np.tanh(h1 @ p["W2"].T + p["b2"])
        mu = h2 @ p["W3"].T + p["b3"]
    assert mu.dtype == dtype
    return mu


def logp64(z, log_std):
    z = np.asarray(z, np.float64)
    return (-0.5 * z * z - np.asarray(log_std, np.float64)).sum(-1) - LOGP_C


def clamp(u):
    return np.fmin(np.fmax(np.asarray(u, np.float32), np.float32(-1.0)), np.float32(1.0))


def mu_bar(w, x, K=0):
    """(bar, deviation): 4 x the largest |float32-numpy MLP - float64 MLP| over the rows x, floored at MU_FLOOR"""
    dev = float(np.max(np.abs(mlp(w, x, K, np.float32).astype(np.float64) - mlp(w, x, K, np.float64)))) if np.asarray(x).size else 0.0
    return max(4.0 * dev, MU_FLOOR), dev


def random_weights(rng, gain=1.0, log_std=(-0.5, -1.0, 0.0), zero_head=False, K=0):
    """N(0, 1 / fan_in) times `gain` (a gain of 8 saturates tanh); zero_head: W3 = 0 and b3 = 0, so that mu is exactly 0"""
    g = lambda o, i: (rng.normal(0.0, 1.0, (o, i)) * gain / np.sqrt(i)).astype(np.float32)      # noqa: E731
    W3, b3 = g(ACT, HIDDEN), (rng.normal(0.0, 0.1, ACT) * gain).astype(np.float32)
    if zero_head:
        W3, b3 = np.zeros_like(W3), np.zeros_like(b3)
    return pack(g(HIDDEN, n_in(K)), (rng.normal(0.0, 0.1, HIDDEN) * gain).astype(np.float32), g(HIDDEN, HIDDEN),
                (rng.normal(0.0, 0.1, HIDDEN) * gain).astype(np.float32), W3, b3, np.asarray(log_std, np.float32), K)
