"""The stand-alone policy forward (include/atc_step.h: atc_policy_forward) restated in numpy, on tests/policy_ref.py: which key a sample of a
row gets, the input row, and mean / z / action / logp in float64.  TEST INFRASTRUCTURE ONLY; needs no GPU.

  keys(R, P, S, decision0)        (decision [S, R], i [S, R]): sample s of row r uses policy_ref.key(seed, decision0 + s ceil(R / P) + r // P, r % P)
  rows(obs_rows, traffic)         x [R, 10 + 7 K]: the own words, then words 0..6 of each record
  forward64(w, x, K, seed, ...)   dict(mean [R, 3], z [S, R, 3], action [S, R, 3], logp [S, R]) in float64

The bars are policy_ref's, unchanged: Z_BAR, LOGP_BAR and mu_bar."""
import numpy as np

import policy_ref as P


def keys(R, P_rows, S, decision0):
    """(decision, i), int64 [S, R] each; decision modulo 2^32"""
    R, P_rows, S = int(R), int(P_rows), int(S)
    assert R >= 1 and 1 <= P_rows <= R and S >= 1
    stride = (R + P_rows - 1) // P_rows
    r = np.arange(R, dtype=np.int64)[None, :]
    s = np.arange(S, dtype=np.int64)[:, None]
    decision = (int(decision0) + s * stride + r // P_rows) & 0xffffffff
    return decision, np.broadcast_to(r % P_rows, (S, R)).copy()


def rows(obs_rows, traffic=None):
    own = np.asarray(obs_rows, np.float32).reshape(-1, P.IN)
    if traffic is None:
        return own
    tr = np.asarray(traffic, np.float32)
    K = tr.shape[-2]
    return np.concatenate([own, tr.reshape(-1, K, 8)[:, :, :P.RECORD_INPUTS].reshape(-1, K * P.RECORD_INPUTS)], axis=1)


def forward64(w, x, K, seed, decision0=0, P_rows=None, S=1, deterministic=False):
    x = np.asarray(x)
    R = x.shape[0]
    mean = P.mlp(w, x, K, np.float64)
    if deterministic:
        assert S == 1
        return dict(mean=mean, z=np.zeros((1, R, 3)), action=mean[None].copy(), logp=np.zeros((1, R)))
    decision, i = keys(R, R if P_rows is None else P_rows, S, decision0)
    z = P.z64(seed, decision[:, :, None], i[:, :, None], np.arange(3)[None, None, :])
    log_std = P.split(w, K)["log_std"].astype(np.float64)
    return dict(mean=mean, z=z, action=mean[None] + np.exp(log_std) * z, logp=P.logp64(z, log_std))
