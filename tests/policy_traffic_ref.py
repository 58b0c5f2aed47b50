"""The decision of the policy rollout with traffic (include/atc_step.h: atc_rollout_policy_traffic) restated in numpy.  Everything of the
decision is tests/policy_ref.py's, taken at K records — split / pack / mlp / mu_bar / random_weights, the key, the draw, logp, the clamp and
the bars, all re-exported here under their names; this module adds what is about traffic only: the input row of
10 + 7 K words built from stored observation rows and stored traffic records, and the widening of a 10-input policy.  The records are
traffic_ref's (the launch's traffic half is held to atc_observe_traffic bit for bit, and that call to traffic_ref by
tests/test_traffic_obs.py).  TEST INFRASTRUCTURE ONLY; needs no GPU."""
import numpy as np

import policy_ref as P
import traffic_ref as R  # noqa: F401  (the reference of the records: re-exported for the tests of this call)
from policy_ref import (LOGP_BAR, MU_FLOOR, RECORD_INPUTS, Z_BAR, Z_MAX, clamp, key, logp64, mlp, mu_bar, n_in, pack,  # noqa: F401
                        shapes, split, uniforms, words, z64)

KS = (1, 2, 4)


def random_weights(rng, K=0, gain=1.0, log_std=(-0.5, -1.0, 0.0), zero_head=False):
    """policy_ref.random_weights with K in second place, as the tests of this call pass it"""
    return P.random_weights(rng, gain, log_std, zero_head, K)


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
