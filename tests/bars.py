"""The bars a HIP result is held to against the fp32 oracle, in one place.  TEST INFRASTRUCTURE ONLY.

Factored out of tests/test_hip_parity.py (_run_vs_oracle: one step's outputs, the whole state) and tests/test_frame_skip.py (one
frame-skip call's outputs) so that tests/session_ref.py applies the very same comparisons after every operation of a call sequence:
  exact      flags, done, n_steps, min_sep (positions are bit-identical and d^2 is the same fma on both sides), raw words 3 and 9
             (heading arithmetic is exact in both implementations)
  1e-5       observations relative to max(1, |ref|) — and to the component's half range where nothing is normalised —, raw values
             against the half range, per-aircraft rewards relative to max(1, |ref|); the env reward additionally 6e-8 N sum |r_k|
             (the fp32 sum of N terms); a frame-skip call's summed rewards: the per-step bar added up over the executed steps
  state      every integer word and the float64 altitudes bit for bit, the exact counts of WIDE headings and heading targets included;
             the fp32 accumulators total_reward / ep_return within rtol 1e-5, atol 1e-3
Inputs are numpy arrays (the caller copies device tensors back); `orc` is an oracle.OracleEnv of the fp32 instantiation."""
import numpy as np


def half_range(comp):
    return 0.5 * comp.norm_max.astype(np.float64)


def obs_scale(ref, normalize, half):
    """what 1e-5 is relative to: envs that were auto-reset return RAW obs (large values): compare relative to magnitude; without
    normalisation every obs is raw and 1e-5 in obs units is 1e-5 of the component's normalisation half-range"""
    scale = np.maximum(1.0, np.abs(ref))
    if not normalize:
        scale = np.maximum(scale, half.astype(np.float32))
    return scale


def check_step(got, orc, normalize, half, tag):
    """One step's outputs against the oracle's arrays after the same step.  got: flags [B, N], done [B], obs [B, N, 10], reward [B]
    and, all four or none, raw_obs / ac_reward / min_sep / term_obs."""
    N = orc.N
    fl = got["flags"].astype(np.uint32)
    assert np.array_equal(fl, orc.flags), ("flags", tag, np.argwhere(fl != orc.flags)[:5])
    assert np.array_equal(got["done"], orc.done), ("done", tag)
    assert np.all(np.abs(got["obs"] - orc.obs) <= 1e-5 * obs_scale(orc.obs, normalize, half)), ("obs", tag)
    # env reward = sum over the env's aircraft of per-aircraft rewards that each meet 1e-5 (checked below when the
    # variant outputs them); the fp32 sum of N terms adds at most N/2 ulps of the running sum
    rtol = 1e-5 * np.maximum(1.0, np.abs(orc.reward)) + 6e-8 * N * np.abs(orc.ac_reward).sum(1)
    assert np.all(np.abs(got["reward"] - orc.reward) <= rtol), ("rew", tag, np.abs(got["reward"] - orc.reward).max())
    if got.get("raw_obs") is None:
        return
    raw, acr, msep, tob = got["raw_obs"], got["ac_reward"], got["min_sep"], got["term_obs"]
    # heading arithmetic is exact in both implementations -> relative_angle (raw[9]) must be bit-identical
    # (checks the division-free Python-modulo of csrc/atc_device.h against the fmodf-based oracle)
    assert np.array_equal(raw[..., 9], orc.raw_obs[..., 9]), tag
    assert np.array_equal(raw[..., 3], orc.raw_obs[..., 3]), tag
    # raw (un-normalised) values: 1e-5 of each component's normalisation half-range (= 1e-5 in obs units)
    assert np.all(np.abs(raw - orc.raw_obs) <= 1e-5 * half), tag
    assert np.all(np.abs(acr - orc.ac_reward) <= 1e-5 * np.maximum(1.0, np.abs(orc.ac_reward))), tag
    # positions are bit-identical and d^2 is the same fma on both sides: the minimum separation is too
    assert np.array_equal(msep, orc.min_sep), tag
    dn = orc.done.astype(bool)
    if dn.any():
        assert np.all(np.abs(tob[dn] - orc.term_obs[dn]) <= 1e-5 * obs_scale(orc.term_obs[dn], normalize, half)), tag


def check_skip_outputs(got, ref, half, full, tag=None):
    """One frame-skip call against tests/skip_ref.py's reference dict.  got: flags, done, n_steps, obs [B, N, 10], reward and (full)
    raw_obs, ac_reward, min_sep, term_obs."""
    assert np.array_equal(got["flags"].astype(np.uint16), ref["flags"]), ("flags", tag)
    assert np.array_equal(got["done"], ref["done"]), ("done", tag)
    assert np.array_equal(got["n_steps"], ref["n_steps"]), ("n_steps", tag)
    err = np.abs(got["obs"] - ref["obs"]) / np.maximum(1.0, np.abs(ref["obs"]))
    print("frame skip", tag, "max obs err %.3g" % err.max(), end=" ")
    assert np.all(err <= 1e-5), ("obs", tag, err.max())
    tol = 1e-5 * ref["reward_scale"]   # the per-step bar, added up over the executed steps
    rerr = np.abs(got["reward"].astype(np.float64) - ref["reward"])
    print("max reward err / bar %.3g" % (rerr / tol).max())
    assert np.all(rerr <= tol), ("reward", tag, (rerr / tol).max())
    if full:
        assert np.all(np.abs(got["raw_obs"] - ref["raw_obs"]) <= 1e-5 * half), ("raw_obs", tag)
        assert np.all(np.abs(got["ac_reward"].astype(np.float64) - ref["ac_reward"]) <= 1e-5 * ref["ac_reward_scale"]), ("ac_reward", tag)
        assert np.array_equal(got["min_sep"], ref["min_sep"]), ("min_sep", tag)
        assert np.all(np.abs(got["term_obs"] - ref["term_obs"]) <= 1e-5 * np.maximum(1.0, np.abs(ref["term_obs"]))), ("term_obs", tag)


_SKIP_KEYS = ("flags", "done", "n_steps", "obs", "reward", "reward_scale", "raw_obs", "ac_reward", "ac_reward_scale", "min_sep", "term_obs")


def check_candidate_outputs(got, ref, ok, half, tag=None):
    """One candidate of a look-ahead or plan call against its reference dict (tests/skip_ref.py: skip_reference / plan_chain), under
    check_skip_outputs' bars.  got: the candidate's rows of the outputs the call returned — reward, done, n_steps always, flags,
    ac_reward, min_sep, obs where requested — as numpy arrays with the env axis first; ok [B] bool: the envs that are evaluated.  An output
    the call does not have (raw_obs, term_obs) or was not asked for takes the reference's own value.  Envs outside `ok` (WIDE at the
    start): n_steps == 0 and every returned word zero."""
    B, N = ref["obs"].shape[:2]
    r = {k: np.asarray(ref[k])[ok] for k in _SKIP_KEYS}
    g = {k: (np.asarray(got[k]).reshape(np.asarray(ref[k]).shape)[ok] if k in got else r[k]) for k in _SKIP_KEYS if not k.endswith("_scale")}
    g["n_steps"] = g["n_steps"].astype(np.int64)
    r["n_steps"] = r["n_steps"].astype(np.int64)
    if ok.any():
        check_skip_outputs(g, r, half, True, tag)
    for k, v in got.items():
        v = np.ascontiguousarray(np.asarray(v).reshape(B, -1)[~ok])
        assert not v.view(np.uint8).any(), ("an env that is not evaluated must return zeros", k, tag)


def check_plan_segments(seg_reward, ref, ok, K, tag=None):
    """seg_reward [H, B] of one plan against tests/skip_ref.py::plan_chain: each segment's reward is one frame-skip call's reward and gets
    that call's bar; zero words behind the env's stop, and everywhere for an env that is not evaluated."""
    seg_reward = np.ascontiguousarray(seg_reward)
    err = np.abs(seg_reward.astype(np.float64) - ref["seg_reward"])
    assert np.all((err <= 1e-5 * ref["seg_reward_scale"])[:, ok]), ("seg_reward", tag, float((err[:, ok] / np.maximum(1e-5 * ref["seg_reward_scale"][:, ok], 1e-300)).max()))
    segs = -(-ref["n_steps"].astype(np.int64) // K)
    behind = np.arange(seg_reward.shape[0])[:, None] >= np.where(ok, segs, 0)[None, :]
    assert not seg_reward.view(np.uint32)[behind].any(), ("seg_reward behind the stop", tag)


def check_state(env, orc, rows_env=slice(None), rows_ac=slice(None), total_reward=True):
    """The persistent state of an AtcVecEnv against the oracle's: the fp32 spec (include/atc_step.h: fixed-point position grid, shared
    heading kinematics, exact rate-limit arithmetic) makes the whole aircraft state BIT-IDENTICAL to the fp32 oracle's — the exact
    counts of WIDE headings / last heading targets (beyond the 32-bit fields, ABI 19) included."""
    e = lambda t: t.cpu().numpy()[rows_env]   # noqa: E731
    a = lambda t: t.cpu().numpy()[rows_ac]    # noqa: E731
    for name in ("timesteps", "actions_taken", "episodes", "ep_length", "ep_actions"):
        assert np.array_equal(e(getattr(env, name)), getattr(orc, name)), name
    assert np.array_equal(e(env.win_bits).astype(np.uint32), orc.win_bits), "win_bits"
    assert np.array_equal(e(env.active_mask).astype(np.uint64), orc.active_mask), "active_mask"
    assert np.array_equal(a(env.ac[:, 0]), orc.px) and np.array_equal(a(env.ac[:, 1]), orc.py), "position counts"
    assert np.array_equal(a(env.h), orc.h), "altitude (float64)"
    assert np.array_equal(a(env.phi_fix), orc.phi_fix) and np.array_equal(a(env.v_fix), orc.v_fix), "heading / speed counts"
    assert np.array_equal(a(env.phi_counts), orc.phi_counts.astype(np.float64)), "exact heading counts (WIDE)"
    assert np.array_equal(a(env.last_act), orc.last_act), "last_act"
    la_wide = np.isin(orc.last_act[:, 1], (-2 ** 31, 2 ** 31 - 1))
    assert np.array_equal(a(env.phi_wide[:, 1])[la_wide], orc.phi_wide[la_wide, 1]), "exact last heading target (WIDE)"
    if total_reward:
        assert np.allclose(e(env.total_reward), orc.total_reward, rtol=1e-5, atol=1e-3), "total_reward"
    assert np.allclose(e(env.ep_return), orc.ep_return, rtol=1e-5, atol=1e-3), "ep_return"
