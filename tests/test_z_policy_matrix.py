"""One oracle-compared case per instantiation of the kernels built on the policy step loop and of the candidate loop that calls the policy.

csrc/atc_policy.inc compiles rollout_policy_body once per lane-group width W (1 ... 64) and traffic list length KT (0, 1, 2, 4) for each of
k_rollout_policy<W>, k_rollout_policy_traffic<W, KT>, k_rollout_policy_ends<W, KT> and k_policy_eval<W, KT>; csrc/atc_lookahead_policy.inc compiles
k_lookahead_policy<W, FULL> per width and form: 98 instantiations.  They differ in more than a constant — policy_decide<IN> is unrolled over
IN = 10 + 7 KT inputs and has a second, float64 form of layer 1 that a wavefront takes when one of its inputs exceeds 4; the traffic stage goes
through LDS from W = 32; W = 64 carries the high mask word; ENDS and EVAL compile stores in and out and move the kernarg re-read offsets — so
each row of MATRIX names one of them ("rollout_policy/W", "traffic/W/K", "ends/W/K", "eval/W/K", "lookahead_policy/W/fast|full") and has one case
below.  This is where per-instantiation coverage of these kernels lives; the families' own test files keep the properties that need one shape.

SHAPES are the smallest at which these kernels can still go wrong: N below W from W = 4 up (3, 5, 9, 17, 33: idle lanes in every lane group),
B = one whole 256-lane workgroup of envs plus a part (341 envs at W = 1, 5 at W = 64), T = 12 with hold = 3 and decision0 = 0xFFFFFFFE (the
decision counter wraps inside the run), a few aircraft taken out of control before decision 0 (aircraft 32 of env 1 for N > 32: the high mask
word), H.policy_env with normalize, shaping, auto_reset, timestep_limit=4, spawn="lattice".  The time limit alone (an episode's fifth step
exceeds it) ends every env at steps 4 and 9 of the first run and, the episode carried over, at steps 2 and 7 of the second: a middle, the
first, the last and a middle step of a block, whatever the policy decides.

ONE RIG per (W, K) serves four rows (_rig): four envs built alike fly TWO chained runs, the first sampled, the second deterministic from the
state the first left, decision0 advanced by 4 and obs0 = the first run's last observation, the way a trainer chains launches (no further env
is built for it).  Per run: rollout_policy / rollout_policy_traffic on env 1 (the "old" side), rollout_policy_ends on env 2,
atc_policy_eval on env 3 (first run: ATC_EVAL_CLEAR over junk; second run: no clear, on the same record), and on env 4, the ORACLE, the loop
they replace: observe_traffic(), then rollout(clamp(action), hold) with term_obs requested, decision by decision.  Every launch is counted from
lib.launch_records() before and after: the call under test moved exactly its own record, at the row's slot, by one; the oracle's launches are
counted apart.
  dynamics   obs, reward, done, flags and the six state arrays bit for bit against the oracle; traffic records bit for bit against
             observe_traffic() at each decision's state
  decisions  tests/policy_ref.py's float64 restatement on the inputs each decision saw, at that file's bars (mu_bar per decision, Z_BAR, LOGP_BAR)
  ends       term_flags and control from tests/policy_ends_ref.py on the oracle's per-step arrays, term_obs the oracle's term_obs at each block's
             ending step with the sentinel kept elsewhere, every older output and the state bit for bit the call without the three outputs
  eval       the record word for word tests/policy_eval_ref.py's fold over the rollout_policy_ends arrays (the second run folded onto the first
             run's record), the state and obs_last bit for bit that twin's
  lookahead  tests/lookahead_policy_compose.py: the composition on a child batch of M B envs (M = 3, H = 2, first given, no auto-reset, B capped
             at 24), every candidate compared; full rows also against lookahead_plan on the flown actions

BOTH FORMS OF LAYER 1, per row, from the oracle's arrays (_forms: which wavefronts, 64 consecutive lane slots, held an input above 4 at each
decision; an idle lane mirrors the batch's last aircraft row).  Decision 0 of the first run sees what observe() left, a raw observation, and
decision 1 of the second run the raw reset observation that the time limit's end on step 2 stored: every wavefront takes the float64 form
there, the W = 64 rows with one env per wavefront included; every other decision sees normalised rows and is fp32.  So each run has both forms,
the float64 one once sampled and once deterministic, and no normalize=False run is needed for the 84 rows.  The
look-ahead rows have no reset: each has a second, normalize=False run in which every row a decision saw is raw, so every wavefront that holds a
live lane — on the child batch and in the candidate tiles — sums layer 1 in float64, where a lane's result depends on its own row only; bit
equality with the composition is asserted there as well.

test_matrix_is_complete (no GPU) reads the symbols of these five templates in the built library and fails unless they are exactly MATRIX.
test_the_runs_contain_what_they_are_meant_to_test asserts the events above on the oracles' arrays; test_every_row_was_launched closes the run.

MEASURED on one MI355X.  Inside the whole -m gpu suite: 0.8 s for this module's 98 cases and their closing tests, the slowest five 0.04 s
(test_the_runs_contain_what_they_are_meant_to_test) and 0.02 s each (traffic/2/4, traffic/2/2, traffic/2/1, traffic/1/1); tests/test_kernel_matrix.py
took 2.5 s in the same run.  Run on its own, first in the process, 3.1 s, of which 2.2 s are the first case (rollout_policy/1), which loads
the library; no other case took more than 0.02 s.  No row has failed so far: 98 of 98 launched and compared."""
import functools
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import helpers as H
import lookahead_policy_compose as LC
import policy_ends_ref as E
import policy_eval_ref as V
import policy_ref as P
import policy_traffic_ref as PT
from atc_hip import layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "atc-reinforcement-learning_amd", "atc_hip", "libatcstep.so")

WIDTHS = (1, 2, 4, 8, 16, 32, 64)
KS = (0, 1, 2, 4)
# kernel template -> (the family's name in a row, the launch record its launches are counted in)
FAMILIES = {"k_rollout_policy": ("rollout_policy", "atc_rollout_policy_launch_counts"),
            "k_rollout_policy_traffic": ("traffic", "atc_rollout_policy_traffic_launch_counts"),
            "k_rollout_policy_ends": ("ends", "atc_rollout_policy_ends_launch_counts"),
            "k_policy_eval": ("eval", "atc_policy_eval_launch_counts"),
            "k_lookahead_policy": ("lookahead_policy", "atc_lookahead_policy_launch_counts")}
RECORD = dict(FAMILIES.values())
MATRIX = (tuple("rollout_policy/%d" % W for W in WIDTHS) + tuple("traffic/%d/%d" % (W, K) for W in WIDTHS for K in KS if K)
          + tuple("ends/%d/%d" % (W, K) for W in WIDTHS for K in KS) + tuple("eval/%d/%d" % (W, K) for W in WIDTHS for K in KS)
          + tuple("lookahead_policy/%d/%s" % (W, f) for W in WIDTHS for f in ("fast", "full")))
assert len(MATRIX) == 98 == len(set(MATRIX))

N_OF = {1: 1, 2: 2, 4: 3, 8: 5, 16: 9, 32: 17, 64: 33}      # N = W for W = 1, 2; below W from there: idle lanes in every lane group
T, HOLD = 12, 3
D = T // HOLD
SEED, DECISION0 = 0x1234567890ABCDEF, 0xFFFFFFFE              # (decision0 + b wraps inside the first run)
CFG = dict(normalize=True, shaping=True, auto_reset=True, timestep_limit=4, spawn="lattice")
LOG_STD = (-0.5, -1.0, 0.25)
SENTINEL, JUNK = -12345.5, 0x5A5A5A5A
OUT_KEYS = ("obs", "reward", "done", "flags")
LOOK_M, LOOK_H, LOOK_B_MAX = 3, 2, 24
EVENTS = ("an end on a block's first step", "an end on a block's middle step", "an end on a block's last step",
          "a decision taken on a reset observation", "an aircraft not under control at decision 0", "the high mask word", "idle lanes",
          "a lane with no env")

_ran = {}          # row -> launches the calls under test made at the row's slot in this module's run
_t0 = [None]
_done = set()      # rows whose case ran to its end


def _batch(W):
    """one whole 256-lane workgroup of envs plus a part: a second, partly filled workgroup; lanes with no env behind the last env"""
    per = 256 // W
    return per + max(1, per // 3)


def _slot(row):
    """(family, the slot of the family's launch record, W, K or the form)"""
    fam, *a = row.split("/")
    W = int(a[0])
    if fam in ("rollout_policy", "lookahead_policy"):
        return fam, W, W, (a[1] if fam == "lookahead_policy" else 0)
    return fam, (W, int(a[1])), W, int(a[1])


# ---------------------------------------------------------------------------------------------------------------- no GPU
def _rows_in(text):
    """the rows named by the symbols of the five kernel templates in a demangled symbol table; no other symbol is looked at"""
    found = set()
    for name, args in re.findall(r"\b(%s)<([^<>]*)>\(" % "|".join(FAMILIES), text):
        a = [x.strip() for x in args.split(",")]
        fam = FAMILIES[name][0]
        assert len(a) == (1 if fam == "rollout_policy" else 2) and a[0].isdigit(), "%s<%s>: arguments this module cannot name" % (name, args)
        if fam == "lookahead_policy":
            assert a[1] in ("true", "false"), "%s<%s>" % (name, args)
            a[1] = "full" if a[1] == "true" else "fast"
        else:
            assert all(x.isdigit() for x in a), "%s<%s>" % (name, args)
        found.add("/".join([fam] + a))
    return found


def _complete(found):
    assert found == set(MATRIX), ("without a case: %s; rows without an instantiation: %s" % (sorted(found - set(MATRIX)), sorted(set(MATRIX) - found)))


def test_matrix_is_complete():
    """The instantiations of the five kernel templates in the built library (its demangled symbol table) are exactly the rows of MATRIX."""
    if not os.path.exists(LIB):
        pytest.skip("libatcstep.so not built yet (run __graft_entry__.build())")
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    found = _rows_in(text)
    assert found, "no symbol of %s found" % ", ".join(FAMILIES)
    print("instantiations found: %d" % len(found))
    _complete(found)


def test_a_new_or_a_missing_instantiation_is_named():
    """the completeness check on symbol tables written here: MATRIX's own passes; one more width or K, or one fewer, fails naming the row"""
    def symbol(row):
        fam, *a = row.split("/")
        name = next(n for n, (f, _) in FAMILIES.items() if f == fam)
        a = [{"fast": "false", "full": "true"}.get(x, x) for x in a]
        return "0000000000001000 T void %s<%s>(float const*, int)\n0000000000002000 t __device_stub__%s<%s>\n" % (name, ", ".join(a), name, ", ".join(a))
    table = "".join(symbol(r) for r in MATRIX) + "0000000000003000 T void k_step<1, true, true, false, false, false>(int)\n0000000000004000 T void k_policy_forward<4>(int)\n"
    _complete(_rows_in(table))
    for extra in ("eval/128/0", "ends/16/8", "traffic/4/8", "rollout_policy/128", "lookahead_policy/128/fast"):
        with pytest.raises(AssertionError, match=r"without a case: \['%s'\]; rows without an instantiation: \[\]" % extra):
            _complete(_rows_in(table + symbol(extra)))
    gone = "ends/32/4"
    with pytest.raises(AssertionError, match=r"without a case: \[\]; rows without an instantiation: \['%s'\]" % gone):
        _complete(_rows_in("".join(symbol(r) for r in MATRIX if r != gone)))
    with pytest.raises(AssertionError, match="cannot name"):
        _rows_in("T void k_policy_eval<4, 1, true>(int)\n")


def test_rows_name_the_slots_of_the_launch_records():
    from atc_hip import lib
    slots = {rec: {name(i) for i in range(n)} for rec, (n, name) in lib.LAUNCH_RECORDS.items() if rec in RECORD.values()}
    assert set(slots) == set(RECORD.values())
    for row in MATRIX:
        fam, slot, W, _ = _slot(row)
        assert slot in slots[RECORD[fam]], row
    # ... and every slot of the five records has a row
    assert {(RECORD[_slot(r)[0]], _slot(r)[1]) for r in MATRIX} == {(rec, s) for rec, ss in slots.items() for s in ss}


def test_shapes():
    for W in WIDTHS:
        N, B = N_OF[W], _batch(W)
        assert H.lane_width(N) == W and (N < W) == (W >= 4) and (N > 32) == (W == 64)
        assert 256 < B * W < 512 and (B * W) % 256 != 0, "a whole workgroup and a partly filled second one"
        assert H.lane_width(N) == W and min(LOOK_B_MAX, B) * LOOK_M * W >= 64
    assert {W: N for W, N in N_OF.items() if W >= 4} == {4: 3, 8: 5, 16: 9, 32: 17, 64: 33} and _batch(64) == 5
    assert (DECISION0 + D - 1) & 0xffffffff < DECISION0, "the decision counter wraps inside the run"


# ---------------------------------------------------------------------------------------------------------------- the rig
def _make(B, N, traffic=0):
    env = H.policy_env(CFG, B, N, traffic)
    # a few aircraft not under control at decision 0
    lo = env.env[:, L.ENV_MASK_LO].clone()
    if N > 1:
        lo[0] &= ~0b10
        lo[B - 1] &= ~0b01
        env.env[:, L.ENV_MASK_LO] = lo
    if N > 32:
        env.stats[1, L.STAT_MASK_HI] = 0          # aircraft 32 of env 1: the high mask word
    env.observe()
    env.synchronize()
    return env


def _gain(env, call):
    """(what call() returns, what it — and nothing else — added to the library's launch records)"""
    from atc_hip import lib
    env.synchronize()
    before = lib.launch_records()
    out = call()
    env.synchronize()
    after = lib.launch_records()
    gained = {g: {k: v - before[g].get(k, 0) for k, v in after[g].items() if v != before[g].get(k, 0)} for g in after}
    return out, {g: v for g, v in gained.items() if v}


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _rig(W, K):
    """Both runs of one (W, K), numpy: dict(B, N, w, runs=[dict(det, decision0, mask0, env0, obs0, old, ends, ev, record, ref, gained, state)])."""
    import torch
    N, B = N_OF[W], _batch(W)
    old_env, ends_env, eval_env, ref_env = _make(B, N), _make(B, N), _make(B, N), _make(B, N, traffic=K)
    for env in (ends_env, eval_env, ref_env):
        for k in H.STATE + ("obs",):
            assert torch.equal(getattr(old_env, k), getattr(env, k)), k
    dev = old_env.device
    w_np = P.random_weights(np.random.default_rng([17, K]), 1.0, LOG_STD, False, K)
    w = torch.as_tensor(w_np, device=dev)
    record = torch.full((B, L.EVAL_WORDS), JUNK, dtype=torch.int32, device=dev)
    state = lambda env: {k: getattr(env, k).cpu().numpy() for k in H.STATE}      # noqa: E731
    x0 = dict(old=old_env.obs.clone(), ends=ends_env.obs.clone(), ev=eval_env.obs.clone(), ref=ref_env.obs.clone())
    runs = []
    for r, det in enumerate((False, True)):
        dec0 = (DECISION0 + r * D) & 0xffffffff
        kw = dict(hold=HOLD, seed=SEED, decision0=dec0, deterministic=det)
        run = dict(det=det, decision0=dec0, mask0=[int(m) for m in ends_env.active_mask.cpu().numpy()], env0=ends_env.env.cpu().numpy().copy(),
                   obs0={k: v.cpu().numpy().reshape(B * N, 10) for k, v in x0.items()}, gained={})
        # the call without the three outputs
        if K:
            old, run["gained"]["old"] = _gain(old_env, lambda: old_env.rollout_policy_traffic(w, T, K, obs0=x0["old"], **kw))
        else:
            old, run["gained"]["old"] = _gain(old_env, lambda: old_env.rollout_policy(w, T, obs0=x0["old"], **kw))
        # the call with them, over sentinels
        out = ends_env._step_rows(T)
        out.update(action=torch.empty((D, B, N, 3), dtype=torch.float32, device=dev), logp=torch.empty((D, B, N), dtype=torch.float32, device=dev),
                   term_obs=torch.full((D, B, N, 10), SENTINEL, dtype=torch.float32, device=dev),
                   term_flags=torch.full((D, B), 0x5A5A, dtype=torch.int16, device=dev), control=torch.full((D, B, N), 7, dtype=torch.uint8, device=dev))
        if K:
            out["traffic"] = torch.empty((D, B, N, K, 8), dtype=torch.float32, device=dev)
        ends, run["gained"]["ends"] = _gain(ends_env, lambda: ends_env.rollout_policy_ends(w, T, K, obs0=x0["ends"], out=out, **kw))
        # the evaluation: CLEAR over junk, then once more without it on the same record
        ev, run["gained"]["ev"] = _gain(eval_env, lambda: eval_env.evaluate_policy(w, T, K, obs0=x0["ev"], record=record, clear=(r == 0), **kw))
        assert ev["record"] is record
        run["record"] = record.cpu().numpy().copy()
        # the oracle: the loop the launches replace, on the old side's clamped actions
        ref = {k: [] for k in OUT_KEYS + ("term_obs", "traffic")}

        def oracle():
            for b in range(D):
                if K:
                    tr = ref_env.observe_traffic()
                    ref_env.synchronize()
                    ref["traffic"].append(tr.clone())
                rows = ref_env._step_rows(HOLD)
                rows["term_obs"] = torch.full((HOLD, B, N * 10), SENTINEL, dtype=torch.float32, device=dev)
                got = ref_env.rollout(old["action"][b:b + 1].clamp(-1.0, 1.0), out=rows, hold=HOLD)
                for k in OUT_KEYS + ("term_obs",):
                    ref[k].append(got[k])
        _, run["gained"]["ref"] = _gain(ref_env, oracle)
        ref = {k: (torch.stack(v) if k == "traffic" else torch.cat(v)) for k, v in ref.items() if v}
        run.update(old=_np(old), ends=_np(ends), ev=dict(obs_last=ev["obs_last"].cpu().numpy()), ref=_np(ref),
                   state=dict(old=state(old_env), ends=state(ends_env), ev=state(eval_env), ref=state(ref_env)))
        x0 = dict(old=old["obs"][-1].clone(), ends=ends["obs"][-1].clone(), ev=ev["obs_last"].clone(), ref=ref["obs"][-1].clone())
        runs.append(run)
    for env in (old_env, ends_env, eval_env, ref_env):
        env.close()
    return dict(B=B, N=N, W=W, K=K, w=w_np, runs=runs)


def _same(a, b):
    return np.array_equal(H.bits(a), H.bits(b))


def _inputs(obs0, obs, traffic, B, N, K):
    """x [D, B N, 10 + 7 K]: what each decision saw — obs0, then the stored observation of step b hold - 1, widened with the stored records"""
    own = H.decision_inputs({"obs0": obs0, "A": {"obs": obs}}, T, HOLD, B * N)
    return PT.input_rows(own.reshape(D, B, N, 10), traffic).reshape(D, B * N, -1) if K else own


def _forms(rig):
    """From the ORACLE's arrays: per run, fp32 [D, waves] and f64 [D, waves] — the wavefronts (64 consecutive lane slots, those with an env) no
    lane of which saw an input above 4 at decision d, and those in which a lane with an aircraft did.  A lane without an aircraft carries the
    batch's last aircraft row (make_ids clamps its index there), so a wavefront counts as fp32 only if that row is clean as well."""
    B, N, W, K = rig["B"], rig["N"], rig["W"], rig["K"]
    slots = np.arange(-(-B * W // 64) * 64)
    e, k = slots // W, slots % W
    valid = (e < B) & (k < N)
    row = np.where(valid, e * N + k, B * N - 1)
    out = []
    for run in rig["runs"]:
        x = _inputs(run["obs0"]["ref"], run["ref"]["obs"], run["ref"].get("traffic"), B, N, K)
        dirty = ~(np.abs(x).max(axis=2) <= 4.0)                                    # [D, B N]
        lane = dirty[:, row]                                                       # [D, slots]
        f64 = (lane & valid[None, :]).reshape(D, -1, 64).any(axis=2)
        fp32 = ~lane.reshape(D, -1, 64).any(axis=2)
        out.append((fp32, f64))
    return out


def _events(rig):
    """what the oracle's arrays of one rig show, as a set of EVENTS"""
    B, N, W = rig["B"], rig["N"], rig["W"]
    seen = set()
    for r, run in enumerate(rig["runs"]):
        ref = run["ref"]
        t_end = E.ending_steps(ref["done"], HOLD)
        for pos, name in ((0, "first"), (1, "middle"), (2, "last")):
            if ((t_end >= 0) & (t_end % HOLD == pos)).any():
                seen.add("an end on a block's %s step" % name)
        # decision b > 0 sees the observation of step b hold - 1; decision 0 of the second run the first run's last one
        before = [rig["runs"][r - 1]["ref"]["done"][-1] != 0 if r else np.zeros(B, bool)] + [ref["done"][b * HOLD - 1] != 0 for b in range(1, D)]
        x = _inputs(run["obs0"]["ref"], ref["obs"], None, B, N, 0).reshape(D, B, N * 10)
        if any((ended & ~(np.abs(x[b]).max(axis=1) <= 4.0)).any() for b, ended in enumerate(before)):
            seen.add("a decision taken on a reset observation")
        control = E.control(run["mask0"], ref["flags"], ref["done"], HOLD, N)
        if r == 0 and (control[0] == 0).any():
            seen.add("an aircraft not under control at decision 0")
        if r == 0 and N > 32 and control[0, 1, 32] == 0 and control[0, 0, 32] == 1:
            seen.add("the high mask word")
    if N < W:
        seen.add("idle lanes")
    if (B * W) % 256:
        seen.add("a lane with no env")
    return seen


def _both_forms(rig, row):
    forms = _forms(rig)
    n32 = [int(f[0].sum()) for f in forms]
    n64 = [int(f[1].sum()) for f in forms]
    print("%s: wavefront-decisions on the fp32 form of layer 1 per run %s, on the float64 form %s" % (row, n32, n64))
    assert sum(n32) > 0 and sum(n64) > 0, (row, "a compared decision on each form of layer 1", n32, n64)


def _decisions(tag, rig, run, arr, obs0):
    """every decision of one launch against tests/policy_ref.py at its bars; decisions are checked independently of each other"""
    B, N, K, w = rig["B"], rig["N"], rig["K"], rig["w"]
    BN = B * N
    x = _inputs(obs0, arr["obs"], arr.get("traffic"), B, N, K)
    u = arr["action"].reshape(D, BN, 3).astype(np.float64)
    log_std = P.split(w, K)["log_std"]
    sigma = np.exp(log_std.astype(np.float64))
    z = P.z64(SEED, *H.draw_indices(run["decision0"], T, HOLD, BN))
    for d in range(D):
        bar, dev32 = P.mu_bar(w, x[d], K)
        mu = P.mlp(w, x[d], K)
        if run["det"]:
            err, allowed = np.abs(u[d] - mu), bar
        else:
            err, allowed = np.abs(u[d] - (mu + sigma * z[d])), bar + sigma * P.Z_BAR
        print("%s decision %d: float32-numpy deviation %.3g, bar %.3g, kernel deviation %.3g, max |x| %.3g" % (tag, d, dev32, bar, float(err.max()), float(np.abs(x[d]).max())))
        assert np.all(err <= allowed), (tag, d, float(err.max()), bar)
    lp = arr["logp"].reshape(D, BN).astype(np.float64)
    if run["det"]:
        assert not arr["logp"].any(), (tag, "deterministic: logp = 0")
    else:
        worst = float(np.abs(lp - P.logp64(z, log_std)).max())
        print("%s: max |logp - logp64| = %.3g (bar %.1g)" % (tag, worst, P.LOGP_BAR))
        assert worst <= P.LOGP_BAR, (tag, worst)


def _moved(row, gained):
    """the call under test moved exactly its own record, at exactly the row's slot, by one"""
    fam, slot, _, _ = _slot(row)
    assert gained == {RECORD[fam]: {slot: 1}}, (row, gained)
    _ran[row] = _ran.get(row, 0) + 1


def _old_row(row, rig):
    """rollout_policy/W and traffic/W/K: the dynamics against the loop they replace, the decisions against the restatement"""
    K = rig["K"]
    for r, run in enumerate(rig["runs"]):
        tag = "%s run %d" % (row, r)
        old, ref = run["old"], run["ref"]
        _moved(row, run["gained"]["old"])
        assert run["gained"]["ref"] and not set(run["gained"]["ref"]) & set(RECORD.values()), (tag, run["gained"]["ref"])      # the oracle's own launches, counted apart
        for k in OUT_KEYS + (("traffic",) if K else ()):
            assert _same(old[k], ref[k]), (tag, k, int((H.bits(old[k]) != H.bits(ref[k])).sum()))
        for k in H.STATE:
            assert _same(run["state"]["old"][k], run["state"]["ref"][k]), (tag, k)
        assert np.all(np.isfinite(old["obs"])) and np.all(np.isfinite(old["reward"])) and np.all(np.isfinite(old["action"]))
        _decisions(tag, rig, run, old, run["obs0"]["old"])
    _both_forms(rig, row)


def _ends_row(row, rig):
    B, N, K = rig["B"], rig["N"], rig["K"]
    for r, run in enumerate(rig["runs"]):
        tag = "%s run %d" % (row, r)
        full, old, ref = run["ends"], run["old"], run["ref"]
        _moved(row, run["gained"]["ends"])
        # every older output and the state: the call without the three outputs; the dynamics: the oracle's
        for k in OUT_KEYS + ("action", "logp") + (("traffic",) if K else ()):
            assert _same(full[k], old[k]), (tag, k)
        for k in H.STATE:
            assert _same(run["state"]["ends"][k], run["state"]["old"][k]), (tag, k)
            assert _same(run["state"]["ends"][k], run["state"]["ref"][k]), (tag, "oracle", k)
        for k in OUT_KEYS + (("traffic",) if K else ()):
            assert _same(full[k], ref[k]), (tag, "oracle", k)
        # term_flags and control: the reference on the oracle's per-step arrays
        assert np.array_equal(full["term_flags"].view(np.uint16), E.term_flags(ref["flags"], ref["done"], HOLD)), tag
        want_c = E.control(run["mask0"], ref["flags"], ref["done"], HOLD, N)
        assert np.array_equal(full["control"], want_c), (tag, np.argwhere(full["control"] != want_c)[:5])
        # term_obs: the oracle's term_obs at each block's ending step; every other row keeps the sentinel
        t_end = E.ending_steps(ref["done"], HOLD)
        want = np.full((D, B, N, 10), SENTINEL, np.float32)
        for d in range(D):
            for e in range(B):
                if t_end[d, e] >= 0:
                    want[d, e] = ref["term_obs"][t_end[d, e], e].reshape(N, 10)
        assert (t_end >= 0).any() and (want != np.float32(SENTINEL)).any()
        assert _same(full["term_obs"], want), (tag, np.argwhere(H.bits(full["term_obs"]) != H.bits(want))[:5])
        _decisions(tag, rig, run, full, run["obs0"]["ends"])
    _both_forms(rig, row)


def _eval_row(row, rig):
    carried = None
    for r, run in enumerate(rig["runs"]):
        tag = "%s run %d" % (row, r)
        twin = run["ends"]
        _moved(row, run["gained"]["ev"])
        t0 = run["env0"][:, L.ENV_TIMESTEPS]
        r0 = np.ascontiguousarray(run["env0"][:, L.ENV_TOTAL_REWARD]).view(np.float32)
        want = V.fold(twin["reward"], twin["done"], twin["flags"], t0, r0, record=carried, mask0=run["mask0"])
        assert np.array_equal(run["record"], want), (tag, np.argwhere(run["record"] != want)[:8])
        assert np.all(run["record"][:, L.EVAL_LAUNCH_STEPS] == (r + 1) * T) and np.all(run["record"][:, L.EVAL_EPISODES] >= 2 * (r + 1))
        for k in H.STATE:
            assert _same(run["state"]["ev"][k], run["state"]["ends"][k]), (tag, k)
        assert _same(run["ev"]["obs_last"].reshape(-1), twin["obs"][-1].reshape(-1)), tag
        carried = run["record"]
    _both_forms(rig, row)


def _look_case(W, form, normalize):
    N, B = N_OF[W], min(LOOK_B_MAX, _batch(W))
    return LC.case(B, N, LOOK_M, LOOK_H, True, form == "full", False, False, False, normalize), B, N


def _look_row(row, W, form):
    for normalize in (True, False):
        r, B, N = _look_case(W, form, normalize)
        _moved(row, r["gained"])
        assert r["n_decided"] > 0 and (r["plan"] is not None) == (form == "full") and set(LC.FAST_OUT) <= set(r["got"])
        assert ("flags" in r["got"]) == (form == "full")
        LC.compare(r, LOOK_M, B, N, LOOK_H, True, layer1="fp32" if normalize else "float64")      # (fp32: asserts max |x| <= 4 at every decision)


# ---------------------------------------------------------------------------------------------------------------- GPU: one case per row
@pytest.mark.gpu
@pytest.mark.parametrize("row", MATRIX)
def test_instantiation_matches_its_oracles(row):
    if _t0[0] is None:
        _t0[0] = time.time()
    fam, _, W, k = _slot(row)
    if fam == "lookahead_policy":
        _look_row(row, W, k)
    else:
        rig = _rig(W, k)
        {"rollout_policy": _old_row, "traffic": _old_row, "ends": _ends_row, "eval": _eval_row}[fam](row, rig)
    _done.add(row)


@pytest.mark.gpu
def test_the_runs_contain_what_they_are_meant_to_test():
    """from the oracles' arrays only"""
    seen = set()
    for W in WIDTHS:
        for K in KS:
            rig = _rig(W, K)
            seen |= _events(rig)
            for fam in ("rollout_policy", "ends", "eval") if K == 0 else ("traffic", "ends", "eval"):
                _both_forms(rig, "%s/%d" % (fam, W) if fam == "rollout_policy" else "%s/%d/%d" % (fam, W, K))
        for form in ("fast", "full"):
            a, b = _look_case(W, form, True)[0], _look_case(W, form, False)[0]
            assert a["n_decided"] > 0 and a["clean"].all() and a["max_x"] <= 4.0, ("lookahead_policy", W, form, "fp32")
            assert b["n_decided"] > 0 and b["raw_rows"], ("lookahead_policy", W, form, "float64")
    assert seen == set(EVENTS), set(EVENTS) - seen


@pytest.mark.gpu
def test_every_row_was_launched():
    """Runs after the cases (file order): each of the 98 instantiations was launched and compared; prints the counts once."""
    if len(_done) < len(MATRIX):
        pytest.skip("only %d of the %d matrix cases ran in this session" % (len(_done), len(MATRIX)))
    print("policy matrix: %d of %d rows launched and compared (%.1f s); launches of the calls under test per row:" % (len(_done), len(MATRIX), time.time() - _t0[0]))
    for fam in ("rollout_policy", "traffic", "ends", "eval", "lookahead_policy"):
        print("  %-17s" % fam + "  ".join("%s %d" % (row.split("/", 1)[1], _ran.get(row, 0)) for row in MATRIX if row.split("/")[0] == fam))
    assert set(_ran) <= set(MATRIX), sorted(set(_ran) - set(MATRIX))
    missing = [row for row in MATRIX if not _ran.get(row)]
    assert not missing, missing
