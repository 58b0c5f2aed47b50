"""Frame skip (include/atc_step.h: atc_step_skip; AtcVecEnv.step_skip; AtcSBVecEnv(frame_skip=)): K held steps in one launch, one
transition per env, an env stops at its first done.

CPU: the reference helper (tests/skip_ref.py) against the definition's literal loop; the events every GPU case's action stream
produces on the oracle alone; the ABI's K check, the k_skip symbols, the Python surface.
GPU: step_skip against the oracle (bars below), against the product's own single step bit for bit, K = 1 against step(), the full
65 536 x 16 batch, the refusals and the launch record, the stable-baselines adapter.

Bars (vs the oracle): flags, done, n_steps, every integer state word and the float64 altitudes exact; obs / raw obs / terminal obs
1e-5 (relative to magnitude for raw values, as tests/test_hip_parity.py does); a summed reward within 1e-5 * sum over the executed
steps of max(1, |r_j|) — the per-step bar added up, nothing else; min_sep exact (positions are bit-identical and d^2 is the same fma on both sides: the single step's own bar, tighter than 1e-5)."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bars
import held_tools as T
import helpers as H
import skip_ref as R
from atc_hip import layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "atc-reinforcement-learning_amd", "atc_hip", "libatcstep.so")
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
CALLS = 32
# block lengths of a case's consecutive calls: every K the contract names, 255 once (every case flies under a short time limit)
K_SCHEDULE = (5, 2, 1, 20, 3, 5, 1, 2) * 2 + (255,) + (5, 2, 1, 20, 3, 5, 1) + (2, 20, 5, 1, 3, 2, 5, 20)
assert len(K_SCHEDULE) == CALLS and {1, 2, 5, 20, 255} <= set(K_SCHEDULE)


def _cases():
    """[(N, B, auto_reset, full)]: N = 1 (LOWW, random entry), 3 (W = 4, idle lanes), 16, 33 (W = 64, idle lanes), 64 and one N for
    each remaining width; ragged B (a partly filled last workgroup) with every optional output, whole workgroups without any —
    so every width has a case with and one without them —, auto-reset on; auto-reset off on a few shapes, both ways."""
    out = []
    for N in (1, 2, 3, 8, 16, 32, 33, 64):
        out += [(N, H.ragged(N), True, True), (N, 2 * (256 // H.lane_width(N)), True, False)]
    out += [(1, 600, False, False), (3, 150, False, True), (16, 37, False, True), (16, 32, False, False), (33, 9, False, False),
            (64, 8, False, True)]
    return out


CASES = _cases()
# the bit-for-bit cases against the product's own single step (seed 77 + N), the K = 1 cases (seed 31, actions from seed W) and the
# full-size case: inputs shared by the GPU tests and the oracle-only events checks
TWIN_CASES = [(1, 300, True, True), (2, 131, True, False), (3, 70, False, True), (8, 75, True, True), (16, 37, True, True),
              (16, 32, False, False), (17, 19, True, False), (33, 9, True, True), (64, 8, True, False), (64, 5, False, True)]
TWIN_IDS = ["N%d B%d %s %s" % (c[0], c[1], "reset" if c[2] else "noreset", "full" if c[3] else "plain") for c in TWIN_CASES]
K1_STEPS, K1_SEED = 30, 31
FULL_SIZE = dict(B=65536, N=16, K=20, calls=4, seed=3, oracle_envs=256)
# (a time limit beyond K and a 5 nm minimum: on the oracle 145-191 of the first 256 envs end inside a block, the others run all K)
FULL_SIZE_PLAN = dict(spawn="lattice", sep_nm=5.0, timestep_limit=30)


def _k1_batch(W):
    return 2 * (256 // W) + 3


IDS = ["N%d B%d %s %s" % (N, B, "reset" if ar else "noreset", "full" if full else "plain") for N, B, ar, full in CASES]


def _seed(N, B, auto_reset, full):
    return 9000 + 13 * CASES.index((N, B, auto_reset, full))


class Events:
    def __init__(self):
        self.early = self.full_no_done = self.done_on_k = self.idle_after_reset = 0
        self.seen = 0

    def add(self, ref, K):
        n, done = ref["n_steps"].astype(int), ref["done"].astype(bool)
        self.early += int((n < K).sum())
        self.full_no_done += int(((n == K) & ~done).sum())
        self.done_on_k += int(((n == K) & done).sum())
        self.idle_after_reset += int((done & (K - n >= 1)).sum())
        executed = np.arange(K)[:, None] < n[None, :]
        self.seen |= int(np.bitwise_or.reduce(np.where(executed[:, :, None], ref["step_flags"], 0).ravel()))

    def check(self, N, auto_reset, k_is_one=False):
        """k_is_one: every block is one step long — no env can stop before its K-th step or wait after a reset; the rest holds."""
        if k_is_one:
            assert self.early == 0 and self.idle_after_reset == 0
        assert k_is_one or self.early > 0, "no env stopped before its block's K-th step"
        assert self.full_no_done > 0, "no env ran a whole block without done"
        assert self.done_on_k > 0, "no env whose done fell exactly on step K"
        assert not auto_reset or k_is_one or self.idle_after_reset > 0, "no auto-reset env that then waited for the block's end"
        assert self.seen & (H.F_INVALID_V | H.F_INVALID_H), "no refused target"
        assert N == 1 or (self.seen & H.F_CONFLICT), "no lost separation"


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_helper_equals_the_literal_loop():
    """B one-env oracles (lattice spawn: the reset draw does not depend on the env index), each run through the definition's
    loop, against the batched helper on every output and every state array, over chained calls; K = 1 is OracleEnv.step."""
    from oracle import oracle as O
    N, B = 3, 12
    scn, comp = T.skip_setup(N)
    kw = dict(spawn="lattice", sep_nm=13.0, timestep_limit=6)
    for auto_reset in (True, False):
        batch = T.skip_oracle(comp, B, N, auto_reset, 5, **kw)
        ones = [T.skip_oracle(comp, 1, N, auto_reset, 5, **kw) for _ in range(B)]
        rng = np.random.default_rng(17)
        ev = Events()
        for K in (3, 1, 8, 2, 20, 5, 1, 4):
            a = T.skip_actions(rng, B, N)
            if K == 1:
                plain = T.skip_oracle(comp, B, N, auto_reset, 5, **kw)
                for k in R.STATE:
                    getattr(plain, k)[...] = getattr(batch, k)
                plain.step(a)
            ref = R.skip_reference(batch, a, K)
            ev.add(ref, K)
            for b in range(B):
                lit = R.literal_skip(ones[b], a[b:b + 1], K)
                for k, v in lit.items():
                    assert np.array_equal(np.asarray(ref[k])[b:b + 1].reshape(v.shape), v), (auto_reset, K, b, k)
                for k in R.STATE:
                    rows = slice(b * N, b * N + N) if k in R.PER_AIRCRAFT else slice(b, b + 1)
                    assert np.array_equal(getattr(batch, k)[rows], getattr(ones[b], k)), (auto_reset, K, b, k)
            if K == 1:
                for k in R.STATE:
                    assert np.array_equal(getattr(batch, k), getattr(plain, k)), k
                for k in ("obs", "raw_obs", "reward", "ac_reward", "done", "flags", "min_sep"):
                    assert np.array_equal(ref[k].reshape(getattr(plain, k).shape), getattr(plain, k)), k
                assert np.all(ref["n_steps"] == 1)
        assert ev.early > 0 and ev.full_no_done > 0


@pytest.mark.parametrize("N,B,auto_reset,full", CASES, ids=IDS)
def test_case_events_on_the_oracle(N, B, auto_reset, full):
    """A condition on the INPUTS of the GPU cases, checked on the oracle alone: within the run an env stops with n < K, one runs all K
    steps without done, one is done exactly on step K, an auto-reset env then waits for at least a step, a target is refused and
    (N >= 2) a separation is lost — the GPU run cannot pass by flying nothing."""
    scn, comp = T.skip_setup(N)
    kw = T.skip_plan(N)
    seed = _seed(N, B, auto_reset, full)
    orc = T.skip_oracle(comp, B, N, auto_reset, seed, **kw)
    rng = np.random.default_rng(seed)
    ev = Events()
    for K in K_SCHEDULE:
        ev.add(R.skip_reference(orc, T.skip_actions(rng, B, N), K), K)
    ev.check(N, auto_reset)


@pytest.mark.parametrize("N,B,auto_reset,full", TWIN_CASES, ids=TWIN_IDS)
def test_twin_case_events_on_the_oracle(N, B, auto_reset, full):
    """The same condition on the inputs of the bit-for-bit cases (their shapes, their seed 77 + N)."""
    scn, comp = T.skip_setup(N)
    orc = T.skip_oracle(comp, B, N, auto_reset, 77 + N, **T.skip_plan(N))
    rng = np.random.default_rng(77 + N)
    ev = Events()
    for K in K_SCHEDULE:
        ev.add(R.skip_reference(orc, T.skip_actions(rng, B, N), K), K)
    ev.check(N, auto_reset)


@pytest.mark.parametrize("W", WIDTHS)
def test_k1_case_events_on_the_oracle(W):
    """... and of the K = 1 cases: episodes end and restart, others go on, a target is refused, a separation is lost."""
    scn, comp = T.skip_setup(W)
    orc = T.skip_oracle(comp, _k1_batch(W), W, True, K1_SEED, **T.skip_plan(W))
    rng = np.random.default_rng(W)
    ev = Events()
    for t in range(K1_STEPS):
        ev.add(R.skip_reference(orc, T.skip_actions(rng, _k1_batch(W), W), 1), 1)
    ev.check(W, True, k_is_one=True)


def test_full_size_case_events_on_the_oracle():
    """... and of the full-size case, on the envs it compares with the oracle (envs are independent: the first 256 of 65 536)."""
    f = FULL_SIZE
    scn, comp = T.skip_setup(f["N"])
    orc = T.skip_oracle(comp, f["oracle_envs"], f["N"], True, f["seed"], **FULL_SIZE_PLAN)
    rng = np.random.default_rng(f["seed"])
    ev = Events()
    for c in range(f["calls"]):
        ev.add(R.skip_reference(orc, T.skip_actions(rng, f["B"], f["N"])[:f["oracle_envs"]], f["K"]), f["K"])
    ev.check(f["N"], True)


def test_k_out_of_range_is_refused_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    for K in (0, 256, -3):
        assert h.atc_step_skip(None, 1, 1, K, None, None, None, None, None, None) == -1   # ATC_ERR_ARG, before any pointer is looked at
        assert b"K" in h.atc_last_error() and b"255" in h.atc_last_error()
    assert h.atc_step_skip(None, 1, 1, 1, None, None, None, None, None, None) == -1        # K in range: now the null pointers
    assert b"null" in h.atc_last_error()
    buf = (C.c_uint64 * L.SKIP_LAUNCH_SLOTS)()
    assert h.atc_skip_launch_counts(buf, L.SKIP_LAUNCH_SLOTS) == 0 and isinstance(lib.skip_launch_counts(), dict)
    assert L.ABI_VERSION == 22 and L.LAUNCH_SLOTS == 57


def test_library_has_k_skip_for_the_seven_widths():
    assert os.path.exists(LIB)
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    found = {int(a.split(",")[0]) for a in re.findall(r"\bvoid k_skip<([^>]*)>\(", text)}
    assert found == set(WIDTHS), found


def test_python_surface():
    from atc_hip import lib
    from atc_hip.sb_adapter import AtcSBVecEnv
    from atc_hip.vec_env import AtcVecEnv
    assert hasattr(AtcVecEnv, "step_skip") and list(inspect.signature(AtcVecEnv.step_skip).parameters) == ["self", "actions", "skip"]
    assert inspect.signature(AtcSBVecEnv.__init__).parameters["frame_skip"].default == 1
    assert {"atc_step_skip", "atc_skip_launch_counts"} <= set(lib.EXPORTS) and callable(lib.skip_launch_counts)


def test_stale_library_is_a_rebuild_error(tmp_path):
    """The ABI number did not change with atc_step_skip, so a library built before it passes the version check: the binding turns
    the missing symbol into the same "rebuild" error.  (A child process: the library can be loaded once per process.)"""
    code = ("import sys; sys.path[:0] = %r\n"
            "from atc_hip import lib\n"
            "lib.EXPORTS = lib.EXPORTS + ('atc_symbol_of_a_newer_header',)\n"
            "try:\n    lib.load()\nexcept RuntimeError as e:\n    assert 'rebuild' in str(e) and 'atc_symbol_of_a_newer_header' in str(e); print('refused')\n"
            % [os.path.join(ROOT, "atc-reinforcement-learning_amd")])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused" in r.stdout, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------- GPU
def _compare_outputs(env, ret, ref, comp, full, rows=slice(None), tag=None):
    """the bars of this file's docstring, kept in tests/bars.py (the call-sequence tests apply them too)"""
    B, N = ref["obs"].shape[0], env.N
    obs, rew, done, info = ret
    cpu = lambda t: t.cpu().numpy()[rows]   # noqa: E731
    got = {"flags": cpu(info["flags"]), "done": cpu(done), "n_steps": cpu(info["frame_steps"]), "obs": cpu(obs).reshape(B, N, 10),
           "reward": cpu(rew)}
    if full:
        got.update(raw_obs=cpu(info["original_state"]).reshape(B, N, 10), ac_reward=cpu(info["aircraft_reward"]),
                   min_sep=cpu(info["min_separation"]), term_obs=cpu(info["terminal_observation"]).reshape(B, N, 10))
    bars.check_skip_outputs(got, ref, bars.half_range(comp), full, tag)


_compare_state = bars.check_state


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("N,B,auto_reset,full", CASES, ids=IDS)
def test_step_skip_matches_oracle(N, B, auto_reset, full):
    from atc_hip import lib
    scn, comp = T.skip_setup(N)
    kw = T.skip_plan(N)
    seed = _seed(N, B, auto_reset, full)
    env = T.skip_env(scn, B, N, auto_reset, seed, full, **kw)
    orc = T.skip_oracle(comp, B, N, auto_reset, seed, **kw)
    rng = np.random.default_rng(seed)
    ev = Events()
    skip0, step0 = lib.skip_launch_counts(), lib.launch_counts()
    for c, K in enumerate(K_SCHEDULE):
        a = T.skip_actions(rng, B, N)
        ref = R.skip_reference(orc, a, K)
        ev.add(ref, K)
        _compare_outputs(env, env.step_skip(a, K), ref, comp, full, tag=(c, K))
        _compare_state(env, orc)
    ev.check(N, auto_reset)
    # counted in the slot of the case's width, by the skip record only
    W = H.lane_width(N)
    now = lib.skip_launch_counts()
    assert {w: n - skip0.get(w, 0) for w, n in now.items() if n != skip0.get(w, 0)} == {W: CALLS}
    assert lib.launch_counts() == step0
    env.close()


def _host_loop_skip(twin, a, K):
    """The definition on the product itself: K plain step() calls (held from the second on), every step's state and outputs cloned,
    each env's rows selected at its n, the selected state copied back.  Returns the call's outputs as CPU tensors."""
    torch = twin.torch
    B, N = twin.B, twin.N
    state_names = ("ac", "alt", "last_act", "env", "stats", "phi_wide")
    out_names = [k for k in ("obs", "raw_obs", "reward", "ac_reward", "done", "flags", "min_sep", "term_obs") if getattr(twin, k) is not None]
    term_before = twin.term_obs.clone() if twin.term_obs is not None else None
    states, outs = [], []
    for j in range(K):
        twin.step(a, held=j > 0)
        states.append({k: getattr(twin, k).clone() for k in state_names})
        outs.append({k: getattr(twin, k).clone() for k in out_names})
    done = torch.stack([o["done"] for o in outs]) != 0                                    # [K, B]
    steps = torch.arange(1, K + 1, device=done.device)[:, None]
    n = torch.where(done.any(0), torch.where(done, steps, K + 1).min(0).values, torch.full_like(steps[0], K).expand(B))
    last, rows = n - 1, torch.arange(B, device=done.device)
    res = {"n_steps": n.to(torch.uint8)}
    pick = lambda name: torch.stack([o[name] for o in outs])[last, rows]   # noqa: E731
    for k in ("obs", "raw_obs", "done"):
        if k in out_names:
            res[k] = pick(k)
    for k in ("reward", "ac_reward"):
        if k in out_names:
            acc = outs[0][k].clone()
            for j in range(1, K):
                live = (j < n) if acc.dim() == 1 else (j < n)[:, None]
                acc = torch.where(live, acc + outs[j][k], acc)    # plain float32 additions in step order
            res[k] = acc
    executed = torch.arange(K, device=done.device)[:, None] < n[None, :]
    fl = torch.stack([o["flags"] for o in outs])
    acc = torch.zeros_like(fl[0])
    for j in range(K):
        acc = torch.where(executed[j][:, None], acc | fl[j], acc)
    res["flags"] = acc
    if "min_sep" in out_names:
        ms = torch.stack([o["min_sep"] for o in outs])
        res["min_sep"] = torch.where(executed, ms, torch.full_like(ms, float("inf"))).min(0).values
    if "term_obs" in out_names:
        ended = done[last, rows]
        res["term_obs"] = torch.where(ended[:, None], pick("term_obs"), term_before)
        twin.term_obs.copy_(res["term_obs"])   # (the loop's steps beyond an env's n wrote there too: the next call starts from the call's result)
    last_ac = last.repeat_interleave(N)
    ac_rows = torch.arange(B * N, device=done.device)
    for k in state_names:
        stack = torch.stack([s[k] for s in states])
        getattr(twin, k).copy_(stack[last_ac, ac_rows] if k in ("ac", "alt", "last_act", "phi_wide") else stack[last, rows])
    return res


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("N,B,auto_reset,full", TWIN_CASES, ids=TWIN_IDS)
def test_step_skip_equals_host_loop_of_steps_bit_for_bit(N, B, auto_reset, full):
    """Pins the summation order and "a stopped env is not touched again": torch.equal on every output and state tensor."""
    import torch
    scn, comp = T.skip_setup(N)
    kw = T.skip_plan(N)
    seed = 77 + N
    env = T.skip_env(scn, B, N, auto_reset, seed, full, **kw)
    twin = T.skip_env(scn, B, N, auto_reset, seed, full, **kw)
    rng = np.random.default_rng(seed)
    early = 0
    for c, K in enumerate(K_SCHEDULE):
        a = torch.as_tensor(T.skip_actions(rng, B, N), device=env.device)
        ref = _host_loop_skip(twin, a, K)
        obs, rew, done, info = env.step_skip(a, K)
        got = {"obs": obs, "reward": rew, "done": done, "flags": info["flags"], "n_steps": info["frame_steps"],
               "raw_obs": info.get("original_state"), "ac_reward": info.get("aircraft_reward"), "min_sep": info.get("min_separation"),
               "term_obs": info.get("terminal_observation")}
        for k, v in ref.items():
            assert torch.equal(got[k].view(v.shape), v), (c, K, k)
        for k in ("ac", "alt", "last_act", "env", "stats", "phi_wide"):
            assert torch.equal(getattr(env, k), getattr(twin, k)), (c, K, "state", k)
        early += int((ref["n_steps"] < K).sum())
    assert early > 0
    env.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("W", WIDTHS)
def test_k1_is_step_bit_for_bit(W):
    import torch
    N = W
    scn, comp = T.skip_setup(N)
    kw = T.skip_plan(N)
    B = _k1_batch(W)
    for full in (True, False):
        env = T.skip_env(scn, B, N, True, K1_SEED, full, **kw)
        twin = T.skip_env(scn, B, N, True, K1_SEED, full, **kw)
        rng = np.random.default_rng(W)
        for t in range(K1_STEPS):
            a = torch.as_tensor(T.skip_actions(rng, B, N), device=env.device)
            o1, r1, d1, i1 = env.step_skip(a, 1)
            o2, r2, d2, i2 = twin.step(a)
            assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(i1["flags"], i2["flags"]), t
            assert torch.all(i1["frame_steps"] == 1)
            for k in i2:
                assert torch.equal(i1[k], i2[k]), (t, k)
            for k in ("ac", "alt", "last_act", "env", "stats", "phi_wide"):
                assert torch.equal(getattr(env, k), getattr(twin, k)), (t, k)
        assert int(env.episodes.sum()) > 0
        env.close()
        twin.close()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_full_size_batch():
    """65 536 x 16, K = 20: the first 256 envs against the oracle (envs are independent and the sampler is keyed by the env index),
    all of them through properties."""
    import torch
    from envs.atc import scenarios
    B, N, K = FULL_SIZE["B"], FULL_SIZE["N"], FULL_SIZE["K"]
    scn, comp = T.skip_setup(N)
    kw = FULL_SIZE_PLAN
    env = T.skip_env(scn, B, N, True, 3, False, **kw)
    orc = T.skip_oracle(comp, 256, N, True, 3, **kw)
    rng = np.random.default_rng(3)
    term = L.F_BELOW_MVA | L.F_OUTSIDE | L.F_CONFLICT | L.F_TIMEOUT | L.F_WON
    for c in range(4):
        a = T.skip_actions(rng, B, N)
        t_before = env.timesteps.clone()
        ref = R.skip_reference(orc, a[:256], K)
        ret = env.step_skip(torch.as_tensor(a, device=env.device), K)
        _compare_outputs(env, ret, ref, comp, False, rows=slice(0, 256), tag=("full size", c))
        _compare_state(env, orc, rows_env=slice(0, 256), rows_ac=slice(0, 256 * N))
        n = ret[3]["frame_steps"].to(torch.int32)
        done = ret[2] != 0
        flags = ret[3]["flags"].to(torch.int32) & 0xffff
        assert bool(((n >= 1) & (n <= K)).all())
        assert bool((flags[done] & term).any(dim=1).all()), "done without a terminal bit in the env's flags"
        assert bool((n[~done] == K).all())
        assert bool(torch.where(done, env.timesteps == 0, env.timesteps == t_before + n).all())
        assert int(done.sum()) > 0 and int((~done).sum()) > 0
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_refusals_and_launch_record():
    import torch
    from atc_hip import lib
    from atc_hip.vec_env import AtcVecEnv
    env = AtcVecEnv(8, 1, host_mapped=True, want_packet=True)
    a = np.zeros((8, 1, 3), np.float32)
    before = (lib.skip_launch_counts(), lib.launch_counts())
    with pytest.raises(RuntimeError, match="packet"):
        env.step_skip(a, 4)
    env.close()
    env = AtcVecEnv(8, 3)
    h = lib.load()
    act = torch.zeros(72, device=env.device)
    for K in (0, 256):
        with pytest.raises(ValueError, match="skip"):    # the Python surface checks the range itself ...
            env.step_skip(a.repeat(3, axis=1), K)
        rc = h.atc_step_skip(env.sector.handle, env.B, env.N, K, C.byref(env._state), act.data_ptr(), C.byref(env._out), None,
                             C.byref(env.params), None)       # ... and so does the library, with every other argument in order
        assert rc == -1 and b"K (" in h.atc_last_error()
    held = type(env.params).from_buffer_copy(env._params_held)
    rc = h.atc_step_skip(env.sector.handle, env.B, env.N, 4, C.byref(env._state), act.data_ptr(), C.byref(env._out), None,
                         C.byref(held), None)
    assert rc == -1 and b"ATC_M_ACTIONS_HELD" in h.atc_last_error()
    assert (lib.skip_launch_counts(), lib.launch_counts()) == before          # a refused call is not counted
    env.step_skip(a.repeat(3, axis=1), 4)
    env.step_skip(a.repeat(3, axis=1), 1)
    assert lib.skip_launch_counts().get(4, 0) - before[0].get(4, 0) == 2 and lib.launch_counts() == before[1]
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_envs", [8, 600])
def test_sb_adapter_frame_skip(n_envs):
    """AtcSBVecEnv(frame_skip=5) under the runner loop of tests/sb_shim's VecEnv contract: transitions and Monitor's episode records
    equal those of a frame_skip=1 env driven with each action repeated until done-or-5; episode["l"] counts ENV steps and
    episode["r"] is the episode return.  (8 envs: host-mapped, dense infos; 600: HBM, sparse infos.)"""
    import importlib
    here = os.path.dirname(os.path.abspath(__file__))
    added = [os.path.join(here, "sb_shim"), os.path.join(here, "oracle_shims")]
    had_gym = "gym" in sys.modules
    sys.path[:0] = added
    try:
        vmod = importlib.import_module("stable_baselines.common.vec_env")
        import atc_hip.sb_adapter as sba
        sba = importlib.reload(sba)
        skip, plain = sba.AtcSBVecEnv(n_envs, frame_skip=5, timestep_limit=23), sba.AtcSBVecEnv(n_envs, timestep_limit=23)
        assert isinstance(skip, vmod.VecEnv) and skip.frame_skip == 5 and plain.frame_skip == 1
        assert np.array_equal(skip.reset(), plain.reset())
        rng = np.random.default_rng(1)
        episodes = 0
        ret, length = np.zeros(n_envs, np.float32), np.zeros(n_envs, np.int64)
        for t in range(40):
            actions = np.clip(rng.normal(0.0, 0.8, (n_envs, 3)), -1.0, 1.0).astype(np.float32)
            obs, rew, dones, infos = skip.step(actions)
            # the same decision on the plain env: repeat until done-or-5, per env (envs that are through wait: their step is undone)
            want_obs, want_rew, want_done = np.zeros_like(obs), np.zeros(n_envs, np.float32), np.zeros(n_envs, bool)
            want_n, want_ep = np.zeros(n_envs, np.int64), [None] * n_envs
            live = np.ones(n_envs, bool)
            vec = plain.vec
            for j in range(5):
                saved = {k: getattr(vec, k).clone() for k in ("ac", "alt", "last_act", "env", "stats", "phi_wide")}
                o, r, d, inf = plain.step(actions)
                for k, v in saved.items():   # envs that had stopped are put back: the plain env has no way not to step them
                    cur = getattr(vec, k)
                    idle = vec.torch.as_tensor(~live).repeat_interleave(cur.shape[0] // n_envs).to(cur.device)
                    cur[idle] = v[idle]
                want_rew = np.where(live, (want_rew + r).astype(np.float32) if j else r, want_rew)
                want_obs[live], want_n[live] = o[live], j + 1
                for b in np.nonzero(live & d)[0]:
                    want_done[b], want_ep[b] = True, inf[b]["episode"]
                live = live & ~d
            assert np.array_equal(obs, want_obs) and np.array_equal(rew, want_rew) and np.array_equal(dones, want_done), t
            ret, length = (ret + rew).astype(np.float32), length + want_n
            for b in range(n_envs):
                if dones[b]:
                    ep = infos[b]["episode"]
                    assert ep["l"] == want_ep[b]["l"] == length[b] and ep["r"] == want_ep[b]["r"], (t, b, ep, want_ep[b], length[b])
                    assert abs(ep["r"] - ret[b]) <= 1e-5 * max(1.0, abs(ep["r"])) * max(1, length[b])   # the summed transitions' rewards
                    assert infos[b]["frame_steps"] == want_n[b]
                    ret[b], length[b] = 0.0, 0
                    episodes += 1
                elif not skip.sparse_infos:
                    assert infos[b]["frame_steps"] == 5 and "episode" not in infos[b]
        assert episodes >= n_envs // 2
        skip.close()
        plain.close()
    finally:
        for p in added:
            sys.path.remove(p)
        for m in [m for m in sys.modules if m == "stable_baselines" or m.startswith("stable_baselines.")]:
            del sys.modules[m]
        if not had_gym:
            for m in [m for m in sys.modules if m == "gym" or m.startswith("gym.")]:
                del sys.modules[m]
        import atc_hip.sb_adapter as sba2
        importlib.reload(sba2)
