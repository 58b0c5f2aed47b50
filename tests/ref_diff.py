"""Differential harness of the SECOND link of the parity chain.  TEST INFRASTRUCTURE ONLY; importing it needs no GPU.

  kernels == fp32 oracle      bit-tight: tests/bars.py, swept by test_fuzz_parity / test_fuzz_held / test_call_sequences / ...
  fp32 oracle == reference    the fp32 instantiation is a SPEC co-designed with the kernels (include/atc_step.h); the float64
                              instantiation is the reference as it is (oracle/atc_oracle_impl.h).  This module flies both side by side.

fly(seed) draws a configuration with tests/fuzz_space.py::parity_case (its draws are untouched; the batch is capped at MAX_B envs, the
step count kept), builds the two oracle.OracleEnv instantiations from identical parameters (fuzz_space.make_oracle), draws the actions with
fuzz_space.draw_actions as run_vs_oracle does and compares after every step through a Comparator, the float64 instantiation as the reference.
The same Comparator holds a KERNEL result to the float64 oracle directly (tests/test_ref_diff.py, -m gpu) with extra=True.

THE BARS (Comparator): none is invented here.
  exact   flags, done, timesteps, actions_taken, episodes, ep_length, ep_actions, win_bits, active_mask, mva
  taken from tests/test_oracle_golden.py (what the fp32 instantiation is held to against the reference's golden vectors):
    obs           1e-5 in normalised units — 1e-5 of the component's half range where the words are raw (no normalisation; the reset
                  observation of an auto-reset env)                                                        (_check_factory: obs_tol)
    raw_obs       1e-5 of the component's half range                                                      (_check_factory: raw_scale)
    ac_reward     1e-5 max(1, |ref|)                                                                      (_check_factory: rew_tol)
    reward        1e-5 sum over the env's aircraft of max(1, |ref_k|)                                     (helpers.replay_wide_interleaved)
    x, y, h, heading, speed   1e-5 max(1, |ref|) in nm / ft / deg / kt                                    (_check_factory: st_tol)
                  The heading and the speed get, on top, the spec's own rate-limit quantisation: a rate-limited step moves the fixed-point
                  word by rint(rate dt 2^23) counts where the reference adds rate dt (include/atc_step.h, "rate limits"), so the two part
                  by q = |rint(rate dt 2^23) - rate dt 2^23| 2^-23 per rate-limited step: (the aircraft's rate-limited steps since its spawn) x q is added.  q is 0 at
                  1 / 2 / 5 s, where the golden vectors that set st_tol live; at 0.15 s it is 4.8e-8 deg per step, and the no-reset case
                  of seed 1118 turns an aircraft for 263 steps to 1.1999874 deg against 1.2: 1.26e-5 deg, past st_tol alone.
  measured: no project bar existed.  The bar is twice the largest deviation of the 2 000-case sweep recorded in
  profiles/ref_diff_sweep.txt (seeds 1000 ... 2999, 8 352 830 env-steps), rounded up to one significant digit — the factor two for seeds the
  sweep did not draw:
    total_reward  largest 1.672e-5 (seed 2351) -> bar 4e-5  relative to S = the reward's unit (sum over the env's aircraft of max(1, |ref_k|)) added
                  up over the episode's steps.  (_check_factory's tot_tol is relative to |ref| and holds for its ONE aircraft; a sum over 33
                  aircraft of rewards of either sign cancels — seed 1064, env 12, step 33: -0.209049 against -0.209060 after 561 addends
                  of magnitude 0.1 ... 1 — so no project bar transfers, and the bar is measured like the others, without growth in t.)
    min_sep       largest 1.148e-5 (seed 1118) -> bar 3e-5  (nm, relative to max(1, |ref|); the 1e30 of an env with fewer than two aircraft is exact)
    ep_return     largest 1.329e-6 (seed 1079) -> bar 3e-6  (relative to S of the finished episode, S as for total_reward)
    term_obs      largest 3.576e-7 (seed 1304) -> bar 8e-7  (the units of obs)
  extra=True (a kernel against the float64 oracle) adds the kernel-vs-fp32-oracle bar of tests/bars.py to each of these — the triangle
  inequality; exact words stay exact, and what tests/bars.py holds bit for bit (min_sep, the aircraft state) adds nothing.

TIES.  The two instantiations may decide a knife edge differently.  An integer mismatch counts as a tie only when attribute() names the
predicate that flipped and the FLOAT64 side's margin on that predicate is below the threshold written next to the rule (TIE_*); such an
env leaves the comparison from that step on and is counted (its remaining steps as excluded env-steps).  Anything else fails.

WORD 9 AT THE WRAP.  relative_angle (model.py:340-342) jumps from +180 to -180 deg where the heading is exactly opposite the runway's;
include/atc_step.h ("Observation word 9 at the wrap") states which side each instantiation takes.  Where the float64 side's |word 9| is
within WRAP_WINDOW_DEG of 180 deg, words 9 of obs / raw_obs / term_obs are compared modulo a turn; rows that do sit on opposite sides
are counted (wrap9)."""
import numpy as np

import bars
import helpers as H
from fuzz_space import Mismatch, draw_actions, make_env, make_oracle, parity_case

MAX_B = 32
WRAP_WINDOW_DEG = 1e-3
REFUSED = H.F_INVALID_V | H.F_INVALID_H
FLAG_NAMES = ((H.F_BELOW_MVA, "below_mva"), (H.F_OUTSIDE, "outside"), (H.F_WON, "won"), (H.F_TIMEOUT, "timeout"), (H.F_INVALID_V, "invalid_v"),
              (H.F_INVALID_H, "invalid_h"), (H.F_CONFLICT, "conflict"), (H.F_NOISE, "noise"), (H.F_INACTIVE, "inactive"))
EXACT_OUT = ("flags", "done", "mva")
EXACT_STATE = ("timesteps", "actions_taken", "episodes", "ep_length", "ep_actions", "win_bits", "active_mask")
FLOAT_OUT = ("obs", "raw_obs", "term_obs", "reward", "ac_reward", "min_sep")
FLOAT_STATE = ("total_reward", "ep_return", "x", "y", "h", "phi", "v")
MEASURED = {"total_reward": 4e-5, "min_sep": 3e-5, "ep_return": 3e-6, "term_obs": 8e-7}     # 2 x the largest of profiles/ref_diff_sweep.txt, one digit, up

# --- tie thresholds: the float64 side's margin below which a flipped predicate is a tie.  Each from the spec's resolution.
# A polygon test of the fp32 spec sees the position and the ring's vertices rounded to fp32: half an ulp each, 2^-18 nm in [64, 128) nm
# (every shipped sector lies inside), plus the agreement of the fixed-point position itself with the float64 one — the dithered rounding
# keeps it within a few position counts (2^-25 nm) per leg, 2^-20 nm over an episode (helpers.replay_wide).
TIE_POS_NM = 2 * 2.0 ** -18 + 2.0 ** -20
# the altitude is float64 on BOTH sides, the reference's operations one for one (ABI 20): only the order of two roundings may differ —
# 128 ulps of a float64 38 000 ft
TIE_ALT_FT = 2.0 ** -30
# the glide-slope ceiling of the corridor is four fp32 operations on a value below 8 192 ft (ulp 2^-10) and moves 318 ft / nm with the
# position (TIE_POS_NM x 318 = 2.6e-3 ft); the altitude it is compared with is rounded to fp32 once
TIE_GS_FT = 2.0 ** -7
# the fixed-point heading turns by rint(3 dt 2^23) counts per step where the reference adds 3 dt deg: half a count, 2^-24 deg, per step
TIE_PHI_DEG_PER_STEP = 2.0 ** -24
# separation: four fp32-rounded coordinates (2^-18 nm each) and the position agreement of two aircraft; two altitudes rounded to fp32
# (half an ulp of 2^-8 ft below 65 536 ft each)
TIE_SEP_NM = 4 * 2.0 ** -18 + 2 * 2.0 ** -20
TIE_SEP_FT = 2.0 ** -8


def case(seed):
    """(scn, comp, kw): fuzz_space.parity_case's draw with the batch capped at MAX_B"""
    scn, comp, kw = parity_case(int(seed), n_cu=256)   # (n_cu given: no device is asked for its CU count)
    kw = dict(kw, B=min(kw["B"], MAX_B))
    return scn, comp, kw


def properties(scn, kw):
    """the mode-space properties of a case (what the coverage test counts)"""
    name = type(scn).__name__
    p = {name + ("_random" if name == "LOWW" and len(scn.entrypoints) > 1 else ""), "sep_nm %g" % kw["sep_nm"],
         "grid " + str(kw["grid_cell"]), "N=1" if kw["N"] == 1 else "N>16" if kw["N"] > 16 else "N 2..16"}
    for label, has in (("discrete", kw["discrete"]), ("continuous", not kw["discrete"]), ("shaping off", not kw["shaping"]),
                       ("normalisation off", not kw["normalize"]), ("keep_active", kw["keep_active"]), ("random entry", kw["spawn"] == "random"),
                       ("non-dyadic dt", kw["dt"] not in (1.0, 2.0, 5.0)), ("out-of-space actions", kw.get("wild", 0.0) > 0.0),
                       ("40-step limit", kw["timestep_limit"] == 40), ("no reset", not kw.get("auto_reset", True)), ("held actions", kw["hold"] > 1)):
        if has:
            p.add(label)
    return p


def new_record():
    return dict(cases=0, env_steps=0, ac_steps=0, done=0, resets=0, refused=0, handovers=0, wrap9=0, off_grid=0, excluded={}, excluded_steps=0,
                flags={n: 0 for _, n in FLAG_NAMES}, props=set(), maxdev={}, where={}, ties=[])


def merge(total, rec):
    for k in ("cases", "env_steps", "ac_steps", "done", "resets", "refused", "handovers", "wrap9", "off_grid", "excluded_steps"):
        total[k] += rec[k]
    for k, v in rec["flags"].items():
        total["flags"][k] += v
    for k, v in rec["excluded"].items():
        total["excluded"][k] = total["excluded"].get(k, 0) + v
    total["props"] |= rec["props"]
    total["ties"] += rec["ties"]
    for k, v in rec["maxdev"].items():
        if v > total["maxdev"].get(k, -1.0):
            total["maxdev"][k], total["where"][k] = v, rec["where"][k]
    return total


# ---------------------------------------------------------------------------------------------------------------- geometry for the ties
def _ring_distance(x, y, rings):
    """distance [nm] from (x, y) to the nearest edge of any of the closed rings"""
    best = np.inf
    for ring in rings:
        r = np.asarray(ring, dtype=np.float64)
        p, q = r[:-1], r[1:]
        d = q - p
        L2 = np.maximum((d * d).sum(1), 1e-300)
        s = np.clip(((x - p[:, 0]) * d[:, 0] + (y - p[:, 1]) * d[:, 1]) / L2, 0.0, 1.0)
        best = min(best, float(np.hypot(p[:, 0] + s * d[:, 0] - x, p[:, 1] + s * d[:, 1] - y).min()))
    return best


def _rel(a1, a2):
    return (a2 - a1 + 180.0) % 360.0 - 180.0


def attribute(ref, comp, e, got_flags, got_mva=None, alt=None):
    """Names the knife edge behind an integer mismatch of env e, or returns None.  ref: the float64 OracleEnv AFTER the step (no reset
    of env e has happened on it if the mismatch is in its flags: an env whose float64 side was auto-reset in this step shows its spawn
    state, and nothing is attributed).  Returns (predicate, aircraft, margin, threshold) of the first aircraft whose flag word (or MVA
    word) differs — after EVERY differing aircraft of the env has been attributed, None otherwise —: the predicate that explains EVERY differing bit of it, the float64 side's margin and the threshold it is below."""
    N = ref.N
    p = ref.params
    src, slack = ref, 0.0
    if ref.done[e] and (p.mode & 8):
        # the float64 side was auto-reset in this step and shows its spawn state.  alt: the fp32 OracleEnv after the same step — where IT
        # was not reset, its position is the float64 one to within 2^-20 nm (the position agreement TIE_POS_NM already counts), so the
        # float64 margin is at most the fp32 side's plus 2^-20 nm; altitudes are the same float64 on both sides
        if alt is None or alt.done[e]:
            return None
        src, slack = alt, 2.0 ** -20
    fa = ref.flags[e].astype(np.int64)
    fb = np.asarray(got_flags[e]).astype(np.int64) & 0x1ff
    ma = ref.mva[e]
    mb = ma if got_mva is None else np.asarray(got_mva[e])
    x, y, h, phi = (np.asarray(getattr(src, n), np.float64).reshape(ref.B, N)[e] for n in ("x", "y", "h", "phi"))
    cg = comp.corridor
    t = int(ref.timesteps[e])
    verdicts = []
    for k in np.flatnonzero((fa != fb) | (ma != mb)):     # EVERY differing aircraft must be explained
        bits = int(fa[k] ^ fb[k])
        found = None
        if (bits & H.F_OUTSIDE) or ma[k] != mb[k] or (bits & H.F_NOISE):
            rings = list(comp.mva_rings) + list(comp.noise_rings)
            found = ("mva_border", _ring_distance(x[k], y[k], rings) + slack, TIE_POS_NM)
            bits &= ~(H.F_OUTSIDE | H.F_BELOW_MVA | H.F_NOISE)      # the floor under the aircraft changes with the polygon
        if bits & H.F_BELOW_MVA:
            found = ("altitude_tie", abs(h[k] - float(ma[k])), TIE_ALT_FT)
            bits &= ~H.F_BELOW_MVA
        if bits & H.F_WON:
            margins = [(_ring_distance(x[k], y[k], [cg["tri_h"], cg["tri_1"], cg["tri_2"]]) + slack, TIE_POS_NM)]
            faf, nrm = np.asarray(cg["faf"]), np.asarray(cg["normal"])
            s = (x[k] - faf[0]) * nrm[0] + (y[k] - faf[1]) * nrm[1]
            foot = faf + s * nrm
            h_max = np.hypot(foot[0] - cg["x"], foot[1] - cg["y"]) * np.tan(np.radians(3.0)) * 6076.0 + cg["h"]
            margins.append((abs(h[k] - h_max), TIE_GS_FT))
            rel = abs(_rel(cg["phi_to_runway"], phi[k]))
            margins.append((min(rel, abs(rel - cg["faf_angle"])), TIE_PHI_DEG_PER_STEP * max(1, t)))
            m = min(margins, key=lambda mt: mt[0] / mt[1])
            found = ("corridor_border", m[0], m[1])
            bits &= ~H.F_WON
        if bits & H.F_CONFLICT:
            act = (fa & H.F_INACTIVE) == 0
            best = (np.inf, 1.0)
            for j in np.flatnonzero(act):
                if j == k:
                    continue
                d, dh = float(np.hypot(x[k] - x[j], y[k] - y[j])), abs(float(h[k]) - float(h[j]))
                # the pair's verdict hangs on the horizontal threshold when it is vertically inside, and the other way round
                for m, thr, inside in ((abs(d - p.sep_nm) + 2 * slack, TIE_SEP_NM, dh < p.sep_ft + TIE_SEP_FT), (abs(dh - p.sep_ft), TIE_SEP_FT, d < p.sep_nm + TIE_SEP_NM)):
                    if inside and m / thr < best[0] / best[1]:
                        best = (m, thr)
            found = ("separation_threshold", best[0], best[1])
            bits &= ~H.F_CONFLICT
        if bits or found is None or not found[1] < found[2]:
            return None
        verdicts.append((found[0], int(k), float(found[1]), float(found[2])))
    return verdicts[0] if verdicts else None


# ---------------------------------------------------------------------------------------------------------------- the comparator
class Comparator:
    """Holds one candidate — the fp32 OracleEnv, or a kernel's outputs (extra=True) — to the float64 OracleEnv `ref`, step after step.

    step(got, t): got = dict of numpy arrays, any subset of EXACT_OUT + FLOAT_OUT (flags, done, obs, reward always); state(got): any subset
    of EXACT_STATE + FLOAT_STATE.  `live` [B] are the envs still compared; `rec` the event record (new_record()).  Raises Mismatch.
    The bars, the tie rules and the word-9 rule are the module docstring's; the measured bars (MEASURED) are total_reward 4e-5 (largest 1.672e-5), min_sep 3e-5 (largest
    1.148e-5), ep_return 3e-6 (largest 1.329e-6), term_obs 8e-7 (largest 3.576e-7): profiles/ref_diff_sweep.txt."""

    def __init__(self, ref, comp, normalize, extra=False, tag=None, rec=None, measure_only=()):
        self.ref, self.comp, self.normalize, self.extra = ref, comp, bool(normalize), bool(extra)
        self.half = bars.half_range(comp)
        self.live = np.ones(ref.B, bool)
        self.rec = new_record() if rec is None else rec
        self.ctx = {"tag": tag}
        self.measure_only = set(measure_only)     # quantities that are recorded but not asserted (the sweep that SETS a measured bar)
        self.auto_reset = bool(ref.params.mode & 8)
        self.steps_left, self.alt = 0, None
        self.scale, self.ep_scale = np.zeros(ref.B), np.zeros(ref.B)    # S of the running / of the last finished episode
        self.limited = {n: np.zeros(ref.B * ref.N) for n in ("phi", "v")}   # rate-limited steps of each aircraft since its spawn
        self.prev = {n: np.asarray(getattr(ref, n), np.float64).copy() for n in ("phi", "v")}
        self.rate = {"phi": 3.0 * ref.params.dt, "v": 5.0 * ref.params.dt}
        q = lambda rate: abs(np.rint(rate * ref.params.dt * 2.0 ** 23) - rate * ref.params.dt * 2.0 ** 23) * 2.0 ** -23   # noqa: E731
        self.rate_q = {"phi": q(3.0), "v": q(5.0)}                      # model.py:47-50: 3 deg / s, 5 kt / s

    # ---- bookkeeping
    def _dev(self, name, ratio_dev, t, idx):
        """records the largest deviation of a quantity (in the units of its bar)"""
        if ratio_dev > self.rec["maxdev"].get(name, -1.0):
            self.rec["maxdev"][name] = float(ratio_dev)
            self.rec["where"][name] = (self.ctx["tag"], t if isinstance(t, str) else int(t), tuple(int(i) for i in idx))

    def _fail(self, what, **more):
        self.ctx.update(more)
        raise Mismatch(self.ctx, what, "ref diff %s" % self.ctx.get("tag"))

    def _float(self, name, got, ref, unit, bar, t, rows):
        """|got - ref| / unit <= bar on the rows of `rows` ([B] bool); records the largest ratio"""
        if not rows.any():
            return
        dev = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / unit
        dev = np.where(np.asarray(got, np.float64) == np.asarray(ref, np.float64), 0.0, dev)     # (inf == inf, 1e30 == 1e30)
        d = dev[rows]
        i = np.unravel_index(int(np.argmax(d)), d.shape)
        self._dev(name, d[i], t, (np.flatnonzero(rows)[i[0]],) + tuple(i[1:]))
        b = np.broadcast_to(bar, dev.shape)[rows]
        if name not in self.measure_only and not np.all(d <= b):
            j = np.unravel_index(int(np.argmax(d / b)), d.shape)
            e = int(np.flatnonzero(rows)[j[0]])
            self._fail("%s beyond its bar: deviation %.3g, bar %.3g" % (name, d[j], b[j]), quantity=name, t=t, env=e, index=tuple(int(v) for v in j[1:]),
                       got=np.asarray(got)[rows][j], ref=np.asarray(ref)[rows][j])

    def _obs_like(self, name, got, ref_arr, raw_rows, bar, t, rows, count=False):
        """an observation array [B, N, 10]: normalised units, or the half range on rows whose words are raw; word 9 modulo a turn inside
        the wrap window"""
        got = np.asarray(got, np.float64).reshape(ref_arr.shape)
        g = ref_arr.astype(np.float64)
        unit = np.where(raw_rows[:, None, None], self.half[None, None, :], 1.0)
        dev = np.abs(got - g)
        turn = np.where(raw_rows, 360.0, 2.0)[:, None]
        deg = g[..., 9] * np.where(raw_rows, 1.0, 180.0)[:, None]           # word 9 in degrees: raw as it is, normalised x 180
        window = np.abs(np.abs(deg) - 180.0) <= WRAP_WINDOW_DEG
        if window.any():
            dev[..., 9] = np.where(window, np.minimum(dev[..., 9], np.abs(dev[..., 9] - turn)), dev[..., 9])
            if count:
                self.rec["wrap9"] += int((window & (got[..., 9] * g[..., 9] < 0) & rows[:, None]).sum())
        if not rows.any():
            return
        d = (dev / unit)[rows]
        i = np.unravel_index(int(np.argmax(d)), d.shape)
        self._dev(name, d[i], t, (np.flatnonzero(rows)[i[0]],) + tuple(i[1:]))
        b = np.broadcast_to(bar, dev.shape)[rows]
        if name not in self.measure_only and not np.all(d <= b):
            j = np.unravel_index(int(np.argmax(d / b)), d.shape)
            e = int(np.flatnonzero(rows)[j[0]])
            self._fail("%s word %d beyond its bar: deviation %.3g, bar %.3g" % (name, j[2], d[j], b[j]), quantity=name, t=t, env=e,
                       index=(int(j[1]), int(j[2])), got=got[rows][j], ref=g[rows][j])

    def _exclude(self, e, t, why):
        pred, k, margin, thr = why
        self.live[e] = False
        self.rec["excluded"][pred] = self.rec["excluded"].get(pred, 0) + 1
        self.rec["excluded_steps"] += max(1, self.steps_left)
        self.rec["ties"].append((self.ctx["tag"], int(t), int(e), k, pred, margin, thr))

    def _exact(self, name, got, ref_arr, t, got_all):
        got = np.asarray(got).reshape(ref_arr.shape)
        bad = (got.astype(np.int64) != ref_arr.astype(np.int64)) if name != "active_mask" else (got.astype(np.uint64) != ref_arr.astype(np.uint64))
        bad = bad.reshape(self.ref.B, -1).any(1) & self.live
        for e in np.flatnonzero(bad):
            why = attribute(self.ref, self.comp, e, got_all["flags"], got_all.get("mva"), self.alt)
            if why is None:
                self._fail("%s differs in env %d and no tie rule explains it" % (name, e), quantity=name, t=t, env=int(e),
                           got=got.reshape(self.ref.B, -1)[e].copy(), ref=ref_arr.reshape(self.ref.B, -1)[e].copy())
            self._exclude(e, t, why)

    # ---- one step's outputs
    def step(self, got, t, steps_left=0, alt=None):
        """compares the outputs of the step the float64 oracle has just taken; `got["flags"]` may carry ATC_F_PHI_LIMIT (fp32 spec only)"""
        ref, N = self.ref, self.ref.N
        self.steps_left, self.alt = steps_left, alt
        got = dict(got, flags=np.asarray(got["flags"]).astype(np.int64).reshape(ref.B, N) & 0x1ff)
        self._last_flags, self._last_mva = got["flags"], got.get("mva")
        for name in EXACT_OUT:
            if name in got:
                self._exact(name, got[name], getattr(ref, name), t, got)
        rows = self.live.copy()
        dn = ref.done.astype(bool)
        reset = dn & self.auto_reset
        x = 1.0 if self.extra else 0.0
        raw_rows = reset | (not self.normalize)
        kb = lambda arr: 1e-5 * bars.obs_scale(arr, self.normalize, self.half) / np.where(raw_rows[:, None, None], self.half, 1.0)   # noqa: E731
        self._obs_like("obs", got["obs"], ref.obs, raw_rows, 1e-5 + x * kb(ref.obs), t, rows, count="raw_obs" not in got)
        acr = np.abs(ref.ac_reward.astype(np.float64))
        unit = np.maximum(1.0, acr).sum(1)
        self.scale += unit
        self._float("reward", got["reward"], ref.reward, unit, 1e-5 + x * (1e-5 * np.maximum(1.0, np.abs(ref.reward)) + 6e-8 * N * acr.sum(1)) / unit, t, rows)
        if "raw_obs" in got:
            self._obs_like("raw_obs", got["raw_obs"], ref.raw_obs, np.ones(ref.B, bool), (1.0 + x) * 1e-5, t, rows, count=True)
        if "ac_reward" in got:
            self._float("ac_reward", np.asarray(got["ac_reward"]).reshape(ref.B, N), ref.ac_reward, np.maximum(1.0, acr), (1.0 + x) * 1e-5, t, rows)
        if "min_sep" in got:
            self._float("min_sep", got["min_sep"], ref.min_sep, np.maximum(1.0, np.abs(ref.min_sep)), MEASURED["min_sep"], t, rows)
        if "term_obs" in got and (rows & reset).any():
            bar = MEASURED["term_obs"] + x * kb(ref.term_obs)
            self._obs_like("term_obs", got["term_obs"], ref.term_obs, np.full(ref.B, not self.normalize), bar, t, rows & reset)
        self.ep_scale = np.where(reset, self.scale, self.ep_scale)
        for n in ("phi", "v"):
            now = np.asarray(getattr(ref, n), np.float64)
            moved = np.abs(now - self.prev[n]) >= self.rate[n] * (1.0 - 1e-9)
            self.limited[n] = np.where(np.repeat(reset, N), 0.0, self.limited[n] + moved)
            self.prev[n] = now.copy()
        self.scale = np.where(reset, 0.0, self.scale)
        # the event record, on the float64 side's words of the envs compared
        rec, fl = self.rec, ref.flags[rows].astype(np.int64)
        rec["env_steps"] += int(rows.sum())
        rec["ac_steps"] += int(((fl & H.F_INACTIVE) == 0).sum())
        for bit, n in FLAG_NAMES:
            rec["flags"][n] += int((fl & bit != 0).sum())
        rec["done"] += int(dn[rows].sum())
        rec["resets"] += int(reset[rows].sum())
        rec["refused"] += int((fl & REFUSED != 0).sum())
        rec["handovers"] += int((((fl & H.F_WON) != 0).any(1) & ~dn[rows]).sum())

    # ---- the persistent state
    def state(self, got, t):
        ref = self.ref
        flags_mva = {"flags": self._last_flags, "mva": self._last_mva}
        for name in EXACT_STATE:
            if name in got:
                self._exact(name, got[name], getattr(ref, name), t, {k: v for k, v in flags_mva.items() if v is not None})
        rows = self.live.copy()
        x = 1.0 if self.extra else 0.0
        acc = lambda r: x * (1e-5 * np.abs(r) + 1e-3) / np.maximum(1.0, np.abs(r))   # noqa: E731  (bars.check_state: rtol 1e-5, atol 1e-3)
        if "total_reward" in got:
            tr = ref.total_reward.astype(np.float64)
            unit = np.maximum(1.0, self.scale)
            self._float("total_reward", got["total_reward"], tr, unit, MEASURED["total_reward"] + acc(tr) * np.maximum(1.0, np.abs(tr)) / unit, t, rows)
        if "ep_return" in got:
            er = ref.ep_return.astype(np.float64)
            unit = np.maximum(1.0, self.ep_scale)
            self._float("ep_return", got["ep_return"], er, unit, MEASURED["ep_return"] + acc(er) * np.maximum(1.0, np.abs(er)) / unit, t, rows)
        ac_rows = np.repeat(rows, ref.N)
        for name in ("x", "y", "h", "phi", "v"):
            if name in got:
                g = np.asarray(getattr(ref, name), np.float64)
                unit = np.maximum(1.0, np.abs(g))
                self._float(name, got[name], g, unit, 1e-5 + (self.limited[name] * self.rate_q[name] if name in self.rate_q else 0.0) / unit, t, ac_rows)


def outputs_of(orc):
    return {k: getattr(orc, k) for k in EXACT_OUT + FLOAT_OUT}


def state_of(orc):
    return {k: getattr(orc, k) for k in EXACT_STATE + FLOAT_STATE}


# ---------------------------------------------------------------------------------------------------------------- the flight
def fly(seed, measure_only=(), max_steps=None, probe=None):
    """Flies case(seed) through both instantiations in lock-step and compares after every step.  Returns the event record: cases, env_steps
    (env-steps compared), ac_steps, flags {name: aircraft-steps}, done, resets, refused, handovers, props, wrap9 (rows on opposite sides of
    the wrap), off_grid (envs stopped because their float64 position left the position grid: no-reset cases only), excluded {predicate:
    envs}, excluded_steps (the env-steps those envs had left), ties, maxdev / where {quantity: largest deviation in the bar's units /
    (tag, step, index)}.  max_steps caps the drawn step count; probe(t, ref, spec) is called after every step, before the comparison.
    Raises Mismatch at the first comparison that fails."""
    scn, comp, kw = case(seed)
    B, N = kw["B"], kw["N"]
    steps = kw["steps"] if max_steps is None else min(kw["steps"], max_steps)
    ref, spec = make_oracle(comp, kw, np.float64), make_oracle(comp, kw, np.float32)
    cmp_ = Comparator(ref, comp, kw["normalize"], tag="seed %d" % seed, measure_only=measure_only)
    rec = cmp_.rec
    rec["cases"], rec["props"] = 1, properties(scn, kw)
    cmp_.ctx.update(seed=int(seed), kw=kw, spec=spec, ref_env=ref)
    auto_reset = kw.get("auto_reset", True)
    lo, hi = H.grid_range(comp)
    rng = np.random.default_rng(seed)
    act = None
    for t in range(steps):
        if t % kw["hold"] == 0 or act is None:
            act = draw_actions(rng, (B, N), kw["discrete"], kw.get("wild", 0.0), True)
        ref.step(act.astype(np.float64))
        spec.step(act)
        if probe is not None:
            probe(t, ref, spec)
        if not auto_reset:   # the header's documented limit: past the position grid the fp32 path pins the position (include/atc_step.h)
            on = ((ref.x >= lo[0]) & (ref.x <= hi[0]) & (ref.y >= lo[1]) & (ref.y <= hi[1])).reshape(B, N).all(1)
            rec["off_grid"] += int((cmp_.live & ~on).sum())
            cmp_.live &= on
        cmp_.step(outputs_of(spec), t, steps_left=steps - t, alt=spec)
        cmp_.state(state_of(spec), t)
        if not cmp_.live.any():
            break
    return rec



# ---------------------------------------------------------------------------------------------------------------- kernels against float64
GPU_N = (1, 3, 16, 17, 64)          # one lane group, a ragged one, a whole wavefront's worth of 16-lane groups, past 16, the full 64
GPU_FORMS = ("step fast", "step full", "rollout", "rollout_hold")


def gpu_case(i):
    """(scn, comp, kw) of the i-th drawn case of the kernel-vs-float64 flights: N and the launch form cycle (every pair within 20 cases), the
    rest is drawn: sector, lookup grid, B <= 64, 60 or 120 steps, timestep, action kind, spawn, hold, time limit, shaping, normalisation,
    separation minimum, keep_active, out-of-space actions (one case in five)"""
    from envs.atc import scenarios
    rng = np.random.default_rng([int(i), 0x52454644])
    N, form = GPU_N[i % 5], GPU_FORMS[(i // 5) % 4]
    kind = "Dense" if N > 54 else str(rng.choice(["LOWW", "LOWW_random", "Simple", "Dense"]))
    scn = scenarios.LOWWDense() if kind == "Dense" else H.make_scenario(kind)
    grid_cell = [None, 0.5, 1.0][int(rng.integers(3))]
    comp = scenarios.compile_scenario(scn, grid_cell=grid_cell)
    kw = dict(B=int(rng.integers(1, 65)), N=N, steps=int(rng.choice([60, 120])), seed=9000 + int(i), grid_cell=grid_cell, form=form,
              dt=float(rng.choice([1.0, 2.0, 5.0, 0.15, 1.3, 3.7])), discrete=bool(rng.integers(2)),
              spawn=str(rng.choice(["lattice", "random"])) if comp.n_entry > 1 else "lattice", hold=int(rng.choice([1, 7, 20])),
              timestep_limit=int(rng.choice([6000, 40])), shaping=bool(rng.integers(4) > 0), normalize=bool(rng.integers(4) > 0),
              sep_nm=float(rng.choice([3.0, 0.0, 5.0])), keep_active=bool(rng.integers(5) == 0),
              wild=float(rng.choice([0.05, 0.3])) if int(rng.integers(5)) == 0 else 0.0, full=form != "step fast" and bool(rng.integers(3) > 0))
    if form == "step full":
        kw["full"] = True
    kw["chunk"], kw["rollout_hold"] = {"rollout": (4, 1), "rollout_hold": (20, 4)}.get(form, (1, 1))
    if form == "rollout_hold":
        kw["hold"] = 4 * int(rng.choice([1, 5]))
    return scn, comp, kw


def fly_kernel(i):
    """Flies gpu_case(i) on an AtcVecEnv, the float64 oracle and the fp32 oracle in lock-step.  Every step's outputs and the final state are
    held to the FLOAT64 oracle directly (Comparator, extra=True: its bar plus the kernel-vs-fp32 bar of tests/bars.py, integer words exact
    under the tie rules) and, the side check that says which link broke, to the fp32 oracle by bars.check_step / bars.check_state.
    Returns (event record, launch record)."""
    import torch
    scn, comp, kw = gpu_case(i)
    B, N, full, chunk, rh = kw["B"], kw["N"], kw["full"], kw["chunk"], kw["rollout_hold"]
    ref, spec = make_oracle(comp, kw, np.float64), make_oracle(comp, kw, np.float32)
    cmp_ = Comparator(ref, comp, kw["normalize"], extra=True, tag="gpu case %d" % i)
    cmp_.rec["cases"], cmp_.rec["props"] = 1, properties(scn, kw) | {kw["form"]}
    with H.launches() as launched:
        env = make_env(scn, kw)
        try:
            rng = np.random.default_rng(kw["seed"])
            cpu = lambda t: t.cpu().numpy()   # noqa: E731
            act, t = None, 0
            while t < kw["steps"]:
                acts = []
                for c in range(chunk):
                    if (t + c) % kw["hold"] == 0 or act is None:
                        act = draw_actions(rng, (B, N), kw["discrete"], kw["wild"], True)
                    acts.append(act)
                if chunk > 1:
                    bufs = None if not full else {k: torch.zeros((chunk,) + shape, dtype=dt, device=env.device) for k, shape, dt in (
                        ("obs", (B, N * 10), torch.float32), ("reward", (B,), torch.float32), ("done", (B,), torch.uint8),
                        ("flags", (B, N), torch.int16), ("raw_obs", (B, N * 10), torch.float32), ("ac_reward", (B, N), torch.float32),
                        ("min_sep", (B,), torch.float32), ("term_obs", (B, N * 10), torch.float32))}
                    out = env.rollout(torch.as_tensor(np.stack(acts[::rh])), out=bufs, hold=rh)
                    outs = [{k: cpu(v[c]) for k, v in out.items() if k in ("obs", "reward", "done", "flags", "raw_obs", "ac_reward", "min_sep", "term_obs")}
                            for c in range(chunk)]
                else:
                    o, r, d, info = env.step(acts[0])
                    outs = [{"obs": cpu(o), "reward": cpu(r), "done": cpu(d), "flags": cpu(info["flags"])}]
                    if full:
                        outs[0].update(raw_obs=cpu(info["original_state"]), ac_reward=cpu(info["aircraft_reward"]),
                                       min_sep=cpu(info["min_separation"]), term_obs=cpu(info["terminal_observation"]))
                for c, got in enumerate(outs):
                    for k in ("obs", "raw_obs", "term_obs"):
                        if k in got:
                            got[k] = got[k].reshape(B, N, 10)
                    if not full:
                        got = {k: got[k] for k in ("obs", "reward", "done", "flags")}
                    ref.step(acts[c].astype(np.float64))
                    spec.step(acts[c])
                    bars.check_step(dict(got, flags=got["flags"].astype(np.uint16)), spec, kw["normalize"], cmp_.half, ("fp32 link", i, t + c))
                    cmp_.step(got, t + c, steps_left=kw["steps"] - t - c, alt=spec)
                t += chunk
                k, org = comp.pos_k, comp.pos_origin      # the state after every launch
                st = {n: cpu(getattr(env, n)) for n in ("timesteps", "actions_taken", "episodes", "ep_length", "ep_actions", "win_bits", "active_mask",
                                                        "ep_return", "total_reward")}
                st.update(x=cpu(env.ac[:, 0]).astype(np.float64) * 2.0 ** -k + org[0], y=cpu(env.ac[:, 1]).astype(np.float64) * 2.0 ** -k + org[1],
                          h=cpu(env.h), phi=cpu(env.phi_counts).astype(np.float64) / 2.0 ** 23 + 180.0,
                          v=(cpu(env.v_fix).astype(np.int64) & 0xffffffff).astype(np.float64) / 2.0 ** 23)
                cmp_.state(st, t - 1)
            bars.check_state(env, spec, total_reward=False)
        finally:
            env.close()
    return cmp_.rec, launched



# ---------------------------------------------------------------------------------------------------------------- the held-block calls
HELD_KERNELS = ("skip", "lookahead", "plan")


class HeldDiff:
    """The references of step_skip / lookahead / lookahead_plan (tests/skip_ref.py) built on the float64 oracle against the ones built on the
    fp32 oracle — or, extra=True, against what the kernels returned — under the Comparator's bars: a call's summed rewards get the per-step
    bar added up over its executed steps (ac_reward_scale, as bars.check_skip_outputs does), observations and min_sep their own.  An env
    whose n_steps / done / flags differ is re-flown step by step from the snapshot before the call until the step that flipped, and
    attribute() must name the tie; the env then leaves the case."""

    def __init__(self, o64, o32, comp, normalize, extra, tag):
        self.o64, self.o32, self.comp, self.extra = o64, o32, comp, extra
        self.c = Comparator(o64, comp, normalize, extra=extra, tag=tag)
        self.rec = self.c.rec
        self.rec.update(pairs={k: 0 for k in HELD_KERNELS}, excluded_pairs=0)

    @property
    def live(self):
        return self.c.live

    def refly(self, envs, before, segments):
        """segments: [(actions [B, N, 3], K)] of the call; before: (snapshot of o64, of o32) taken before it"""
        import skip_ref as R
        after = R.snapshot(self.o64), R.snapshot(self.o32)
        R.restore(self.o64, before[0])
        R.restore(self.o32, before[1])
        todo = set(int(e) for e in envs)
        for act, K in segments:
            for _ in range(K):
                self.o64.step(np.asarray(act, np.float64))
                self.o32.step(np.asarray(act, np.float32))
                for e in sorted(todo):
                    if np.array_equal(self.o32.flags[e] & 0x1ff, self.o64.flags[e]) and self.o32.done[e] == self.o64.done[e]:
                        continue
                    why = attribute(self.o64, self.comp, e, self.o32.flags, self.o32.mva, self.o32)
                    if why is None:
                        self.c._fail("env %d: the held call's integer words differ and no tie rule explains the step that flipped" % e, env=e)
                    self.c._exclude(e, 0, why)
                    todo.discard(e)
        if todo:
            self.c._fail("envs %s: integer words of the held call differ though no step's flags do" % sorted(todo))
        R.restore(self.o64, after[0])
        R.restore(self.o32, after[1])

    def compare(self, kernel, ref, got, ok, auto_reset, before, segments, ref32=None):
        """ref: the float64-built reference dict; got: the fp32-built one or a kernel's outputs (any subset of the keys); ok [B]: evaluated envs"""
        c, B = self.c, self.o64.B
        N = self.o64.N
        rows = c.live & ok
        g = {k: np.asarray(v).reshape(np.asarray(ref[k]).shape) for k, v in got.items() if k in ref and not k.endswith("_scale") and k != "seg_reward"}
        bad = np.zeros(B, bool)
        for k in ("n_steps", "done", "flags"):
            if k in g:
                a, b = g[k].astype(np.int64), np.asarray(ref[k]).astype(np.int64)
                if k == "flags":
                    a = a & 0x1ff
                bad |= (a != b).reshape(B, -1).any(1)
        bad &= rows
        if bad.any():
            self.refly(np.flatnonzero(bad), before, segments)
            self.rec["excluded_pairs"] += int(bad.sum())
        rows = rows & ~bad & c.live
        self.rec["pairs"][kernel] += int(rows.sum())
        x = 1.0 if self.extra else 0.0
        dn = np.asarray(ref["done"]).astype(bool)
        reset = dn & auto_reset
        raw_rows = reset | (not c.normalize)
        one = lambda arr: np.maximum(1.0, np.abs(arr)) / np.where(raw_rows[:, None, None], c.half, 1.0)   # noqa: E731  (bars.check_skip_outputs' unit)
        if "obs" in g:
            c._obs_like("obs", g["obs"], np.asarray(ref["obs"]), raw_rows, 1e-5 + x * 1e-5 * one(ref["obs"]), kernel, rows, count=True)
        if "raw_obs" in g:
            c._obs_like("raw_obs", g["raw_obs"], np.asarray(ref["raw_obs"]), np.ones(B, bool), (1.0 + x) * 1e-5, kernel, rows)
        if "term_obs" in g and (rows & reset).any():
            tr = np.full(B, not c.normalize)
            unit = np.maximum(1.0, np.abs(ref["term_obs"])) / np.where(tr[:, None, None], c.half, 1.0)
            c._obs_like("term_obs", g["term_obs"], np.asarray(ref["term_obs"]), tr, MEASURED["term_obs"] + x * 1e-5 * unit, kernel, rows & reset)
        unit = np.maximum(1.0, ref["ac_reward_scale"].sum(1))
        if "reward" in g:
            c._float("reward", g["reward"], ref["reward"], unit, 1e-5 + x * 1e-5 * ref["reward_scale"] / unit, kernel, rows)
        if "ac_reward" in g:
            c._float("ac_reward", g["ac_reward"], ref["ac_reward"], np.maximum(1.0, ref["ac_reward_scale"]), (1.0 + x) * 1e-5, kernel, rows)
        if "min_sep" in g:
            c._float("min_sep", g["min_sep"], ref["min_sep"], np.maximum(1.0, np.abs(ref["min_sep"])), MEASURED["min_sep"], kernel, rows)


def fly_held(seed, device=False):
    """held_fuzz.case(seed) — its draws untouched — flown as held_fuzz.run flies it: the flown step_skip calls, the look-ahead, the plan and
    the closing step_skip.  device=False: every call's float64-built reference against the fp32-built one.  device=True: against what the
    kernels return (extra=True), with the fp32-built reference as the side check under tests/bars.py.  Returns the record (pairs per kernel,
    excluded pairs, ties, largest deviations)."""
    import held_fuzz as F
    import skip_ref as R
    from oracle import oracle as O
    scn, comp, kw = F.case(seed)
    B, N, full, discrete, wild = kw["B"], kw["N"], kw["full"], kw["discrete"], kw["wild"]
    o64, o32 = make_oracle(comp, kw, np.float64, auto_reset=True), make_oracle(comp, kw, np.float32, auto_reset=True)
    hd = HeldDiff(o64, o32, comp, kw["normalize"], device, "held case %d" % seed)
    hd.rec["cases"], hd.rec["props"] = 1, F.properties(scn, kw)
    half = bars.half_range(comp)
    rng = np.random.default_rng([kw["seed"], 0x464C59])
    env = make_env(scn, kw, auto_reset=True) if device else None
    try:
        if device:
            import torch
            from atc_hip import lib
        auto_reset = True

        def skip_call(tag, K):
            a = F.draw_flown(rng, B, N, discrete, wild)
            before = R.snapshot(o64), R.snapshot(o32)
            r64, r32 = R.skip_reference(o64, a, K), R.skip_reference(o32, a, K)
            got = r32
            if device:
                got = F._skip_outputs(env, env.step_skip(a, K), full)
                bars.check_skip_outputs(got, r32, half, full, ("fp32 link", tag))
            hd.compare("skip", r64, got, np.ones(B, bool), auto_reset, before, [(a, K)])

        for c_, K in enumerate(kw["flown"]):
            skip_call("step_skip %d" % c_, K)
        if kw["auto_reset_off"]:
            auto_reset = False
            for o in (o64, o32):
                o.params.mode &= ~O.M_AUTO_RESET
            if device:
                H.set_auto_reset(env, False)
        ok = ~R.wide_envs(o32)
        for kernel in ("lookahead", "plan"):
            c_ = kw[kernel]
            M, K, Hn = c_["M"], c_["K"], c_.get("H")
            cand = F.draw_candidates(rng, (M, B, N) if Hn is None else (M, Hn, B, N), discrete, wild)
            before = R.snapshot(o64), R.snapshot(o32)
            build = (lambda o: R.candidate_references(o, cand, K)) if Hn is None else (lambda o: R.plan_references(o, cand, K))
            refs64, refs32 = build(o64), build(o32)
            got_all = None
            if device:
                lib.lookahead_set_mapping(c_["mapping"])
                at = torch.as_tensor(cand, device=env.device)
                res = env.lookahead(at, K, outputs=c_["outputs"]) if Hn is None else env.lookahead_plan(at, K, outputs=c_["outputs"])
                lib.lookahead_set_mapping(0)
                got_all = {k: v.cpu().numpy() for k, v in res.items()}
            for m in range(M):
                got = refs32[m]
                if device:
                    got = {k: v[m] for k, v in got_all.items() if k != "seg_reward"}
                    bars.check_candidate_outputs(got, refs32[m], ok, half, tag=("fp32 link", kernel, m))
                segments = [(cand[m], K)] if Hn is None else [(cand[m, h], K) for h in range(Hn)]
                hd.compare(kernel, refs64[m], got, ok, auto_reset, before, segments)
        skip_call("closing step_skip", kw["last"])
    finally:
        if env is not None:
            from atc_hip import lib
            lib.lookahead_set_mapping(0)
            env.close()
    return hd.rec


EXCLUDED_CAP, WRAP_CAP = 0.001, 1.0 / 50000      # of the env-steps: attributed exclusions; word-9 rows on the other side of the wrap


def check_caps(total):
    """the two caps every sweep is held to; returns the lines of what exceeds them"""
    over, steps = [], total["env_steps"] + total["excluded_steps"]
    if total["excluded_steps"] > EXCLUDED_CAP * steps:
        over.append("%d env-steps excluded as ties of %d: above %.1f %%" % (total["excluded_steps"], steps, 100 * EXCLUDED_CAP))
    if total["wrap9"] > WRAP_CAP * total["env_steps"]:
        over.append("%d word-9 wrap rows in %d env-steps: above 1 per %d" % (total["wrap9"], total["env_steps"], round(1 / WRAP_CAP)))
    return over


def report(total, seconds=None):
    """the lines of profiles/ref_diff_sweep.txt"""
    out = ["cases %d  env-steps %d  aircraft-steps %d%s" % (total["cases"], total["env_steps"], total["ac_steps"],
                                                          "" if seconds is None else "  (%.0f s on one CPU core)" % seconds),
           "done %d  auto-resets %d  refused targets %d  hand-overs %d  envs stopped off the position grid %d" % (
               total["done"], total["resets"], total["refused"], total["handovers"], total["off_grid"]),
           "flags (aircraft-steps): " + "  ".join("%s %d" % (n, total["flags"][n]) for _, n in FLAG_NAMES),
           "integer mismatches attributed to a tie: %d envs, %d env-steps excluded (%.4f %% of compared + excluded)  by predicate: %s" % (
               sum(total["excluded"].values()), total["excluded_steps"], 100.0 * total["excluded_steps"] / max(1, total["env_steps"] + total["excluded_steps"]),
               dict(total["excluded"]) or "none"),
           "word-9 rows on opposite sides of the +-180 deg wrap: %d (1 per %.0f env-steps)" % (
               total["wrap9"], total["env_steps"] / max(1, total["wrap9"]))]
    for tie in total["ties"]:
        out.append("  tie: %s step %d env %d aircraft %d: %s, float64 margin %.3g < %.3g" % tie)
    out.append("largest deviation per quantity, in the units of its bar (see tests/ref_diff.py), and where (case, step, index):")
    for k in FLOAT_OUT + FLOAT_STATE:
        if k in total["maxdev"]:
            out.append("  %-13s %.3e   %s" % (k, total["maxdev"][k], total["where"][k]))
    out.append("properties reached: " + ", ".join(sorted(total["props"])))
    return out


if __name__ == "__main__":      # python tests/ref_diff.py SEED0 CASES [--measure]: the sweep record of profiles/ref_diff_sweep.txt
    import sys
    import time
    seed0, cases = int(sys.argv[1]), int(sys.argv[2])
    only = tuple(MEASURED) if "--measure" in sys.argv else ()
    total, t0 = new_record(), time.time()
    for s in range(seed0, seed0 + cases):
        merge(total, fly(s, measure_only=only))
    print("seeds %d ... %d%s" % (seed0, seed0 + cases - 1, "  (measured quantities recorded, not asserted)" if only else ""))
    print("\n".join(report(total, time.time() - t0)))
    over = check_caps(total)
    for line in over:
        print("CAP EXCEEDED:", line)
    sys.exit(1 if over else 0)
