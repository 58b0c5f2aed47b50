"""The decision of the policy rollout with traffic (include/atc_step.h: atc_rollout_policy_traffic) restated in numpy: tests/policy_ref.py's
split / pack / mlp / mu_bar / random_weights generalised to an input row of IN = 10 + 7 K words, and the row itself built from stored
observation rows and stored traffic records.  The key, the draw, logp and the clamp are policy_ref's, unchanged; the records are
traffic_ref's (the launch's traffic half is held to atc_observe_traffic bit for bit, and that call to traffic_ref by
tests/test_traffic_obs.py).  TEST INFRASTRUCTURE ONLY; needs no GPU.

THE BARS are policy_ref's, not new numbers: Z_BAR and LOGP_BAR as they stand; mu_bar(w, x, K) = 4 x the largest
deviation of the float32-numpy MLP from the float64 one on the same widened rows, floored at MU_FLOOR."""
import numpy as np

import policy_ref as P
import traffic_ref as R  # noqa: F401  (the reference of the records: re-exported for the tests of this call)

KS = (1, 2, 4)
RECORD_INPUTS = 7          # words 0..6 of a record are inputs; word 7 (the slot) is stored only
Z_BAR, LOGP_BAR, MU_FLOOR, Z_MAX = P.Z_BAR, P.LOGP_BAR, P.MU_FLOOR, P.Z_MAX
key, uniforms, z64, logp64, clamp = P.key, P.uniforms, P.z64, P.logp64, P.clamp


def n_in(K=0):
    return P.IN + RECORD_INPUTS * K


def words(K=0):
    return P.WORDS + P.HIDDEN * RECORD_INPUTS * K


def shapes(K=0):
    return (("W1", (P.HIDDEN, n_in(K))),) + P.SHAPES[1:]


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


def mu_bar(w, x, K=0):
    """(bar, deviation): 4 x the largest |float32-numpy MLP - float64 MLP| over the rows x, floored at MU_FLOOR"""
    dev = float(np.max(np.abs(mlp(w, x, K, np.float32).astype(np.float64) - mlp(w, x, K, np.float64)))) if np.asarray(x).size else 0.0
    return max(4.0 * dev, MU_FLOOR), dev


def random_weights(rng, K=0, gain=1.0, log_std=(-0.5, -1.0, 0.0), zero_head=False):
    """policy_ref.random_weights with a first layer of 10 + 7 K inputs: N(0, 1 / fan_in) times `gain`"""
    g = lambda o, i: (rng.normal(0.0, 1.0, (o, i)) * gain / np.sqrt(i)).astype(np.float32)      # noqa: E731
    W3, b3 = g(P.ACT, P.HIDDEN), (rng.normal(0.0, 0.1, P.ACT) * gain).astype(np.float32)
    if zero_head:
        W3, b3 = np.zeros_like(W3), np.zeros_like(b3)
    return pack(g(P.HIDDEN, n_in(K)), (rng.normal(0.0, 0.1, P.HIDDEN) * gain).astype(np.float32), g(P.HIDDEN, P.HIDDEN),
                (rng.normal(0.0, 0.1, P.HIDDEN) * gain).astype(np.float32), W3, b3, np.asarray(log_std, np.float32), K)


def input_rows(obs_rows, records):
    """[..., N, 10 + 7 K] from observation rows [..., N, 10] and records [..., N, K, 8]: own words, then words 0..6 of each record"""
    records = np.asarray(records)
    N, K = records.shape[-3], records.shape[-2]
    lead = records.shape[:-3]
    own = np.asarray(obs_rows).reshape(lead + (N, P.IN))
    return np.concatenate([own, records[..., :RECORD_INPUTS].reshape(lead + (N, K * RECORD_INPUTS))], axis=-1)


def widen(w10, K, traffic_columns=None):
    """the K-record policy whose own ten columns of W1 and every other part are those of the 10-input policy w10; the 7 K traffic columns
    are zero, or `traffic_columns` [64, 7 K]"""
    p = P.split(w10)
    cols = np.zeros((P.HIDDEN, RECORD_INPUTS * K), np.float32) if traffic_columns is None else np.asarray(traffic_columns, np.float32)
    W1 = np.concatenate([p["W1"], cols], axis=1)
    return pack(W1, p["b1"], p["W2"], p["b2"], p["W3"], p["b3"], p["log_std"], K)
