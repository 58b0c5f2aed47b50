"""The tile / candidate-group decode of the candidate kernels (csrc/atc_lookahead.inc: look_tile; csrc/atc_step.hip: cand_grid) past
one chunk of tiles, on EVERY env and candidate.

k_lookahead, k_plan, k_plan_sampled and k_branch share one launch shape: 256-slot tiles of the batch x groups of `cpg` candidates,
workgroup id = (chunk * groups + g) * 8 + j serving tile 8 chunk + j, the grid padded to whole chunks of 8 tiles.  The rest of the suite
compares every env only where chunk == 0 (at most 8 tiles), and 16 tiles at W = 16 with the default mapping.  Here each case has 9 tiles
(one whole chunk, then one tile in a chunk that is 7/8 padding) or 17 tiles (two whole chunks, then a tile in a padded chunk), always
with a partial last tile (held_tools.look_tiles) — the smallest shapes at which every term of the decode is non-zero — under the
mappings cpg = 0 (the library's 1: 5 groups), 2 (3 groups, the last of one candidate) and M (1 group) at M = 5, and cpg = 64 at M = 70
(the drawn-plan kernel only: groups of 64 and 6).  CASES is a covering design, asserted below on the table itself: each (kernel, W,
form), each (kernel, mapping, tile count), each (W, tile count); one case per kernel with N below W; k_skip (the plain step_grid) for
each (W, form) at 17 tiles.  test_table_is_the_instantiation_set (no GPU) reads the built library's symbol table and fails unless the
k_lookahead / k_plan / k_plan_sampled / k_branch / k_skip instantiations are exactly the table's (kernel, W, form) set.

A case: the env of held_tools.look_env (held_tools.skip_env for k_skip, whose form follows the env's bound outputs) on the dense
sector, a short time limit, auto-reset on, lattice spawn from 9 aircraft up; two frame-skip calls are flown (3 + 1 steps) on the env and
the fp32 oracle, then ONE call of the kernel with every output between sentinel guard rows and filled with sentinels:
  lookahead, plan   skip_ref.candidate_references / plan_references on the oracle, bars.check_candidate_outputs / check_plan_segments
  sampled           plan_draw_ref.draw flown through skip_ref.plan_references, the same bars
  branch            branch_ref.clone_reference (the product's own step_skip per candidate), outputs and child state bit for bit
  skip              skip_ref.skip_reference, bars.check_skip_outputs and bars.check_state
on every env and candidate; envs that are WIDE at the start (not evaluated) return zeros and, for branch, the source's rows; no
sentinel is left; the source state is byte-equal afterwards; the kernel's launch record moved by exactly {W: 1}.  No tolerance is
this module's own.

The flown calls draw fuzz_space.draw_actions with a third of the components outside the action space.  With the heading component in
that draw in every env (held_tools.skip_actions: a wild heading target is WIDE) the plain draw cannot stay under the cap on WIDE pairs:
no env of 16 or more aircraft would be evaluated (tests/test_tree_sequences.py states the shares).  So the heading takes part only in
the envs e % 16 == 5 — tests/test_tree_sequences.py's wild-heading draw in a sixteenth of the envs instead of a fifth, and a fixed
pattern instead of a drawn one, because the cap here holds per case, down to 33 envs.  Candidates keep their headings inside the
action space.

The CPU twin (test_case_on_the_oracle) flies each case on the oracle alone and asserts, over the envs of tiles 8 and up: an env that
stops early, an env that resets inside the block, two candidates that differ in reward in at least half of those envs, an env of the
last tile that is evaluated and not done at its first step; and at most test_fuzz_held.WIDE_CAP of the case's (candidate, env) pairs
WIDE.  Measured on the oracle, all 75 cases, evaluated envs of tiles 8 and up (1 or 3 envs in a 9-tile case, 31 .. 2 051 in a 17-tile
case): every (candidate, env) pair stops early and resets inside the block (the time limit falls inside the call: n_steps differs with
the env's age); the candidates differ in reward in 65 % (sampled, N = 1) to 100 % of the envs; every env of the last tile flies past
its first step; WIDE pairs are 1.1 % .. 6.2 % of a case's pairs, none of them in tiles 8 and up of a 9-tile case (its last tile starts
at a multiple of 16) and 2 .. 32 envs there in every 17-tile case (test_wide_envs_past_the_first_chunk)."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import bars
import branch_ref as BR
import held_tools as T
import helpers as H
import plan_draw_ref as P
import skip_ref as R
from atc_hip import layout as L
from fuzz_space import draw_actions
from held_tools import LIB
from test_fuzz_held import WIDE_CAP
from test_kernel_matrix import N_BELOW

WIDTHS = (1, 2, 4, 8, 16, 32, 64)
KERNELS = ("lookahead", "plan", "sampled", "branch")
SYMBOL = {"lookahead": "k_lookahead", "plan": "k_plan", "sampled": "k_plan_sampled", "branch": "k_branch", "skip": "k_skip"}
TILES = (9, 17)
M_CAND, M_MANY = 5, 70
MAPPINGS = (0, 2, M_CAND)          # cpg: the library's choice (1), 3 groups with a last one of one candidate, one group
FLOWN = (3, 1)                     # the frame-skip calls flown before the case's call
K_ONE, H_PLAN, K_PLAN = 10, 3, 4   # one block of 10 steps; plans of 3 segments of 4: both run past the time limits of 7 / 12 steps
WILD_EVERY, WILD_AT = 16, 5        # envs e % 16 == 5: the heading component takes part in the flown calls' out-of-space draw
STD = 0.3
LOOK_ALL = ("flags", "min_sep", "ac_reward", "obs")
PLAN_ALL = ("seg_reward",) + LOOK_ALL


def _table():
    """[(id, kernel, N, tiles, full, M, mapping)]"""
    out = []
    for ki, kernel in enumerate(KERNELS):
        for wi, W in enumerate(WIDTHS):
            for fi, full in enumerate((False, True)):
                out.append((kernel, W, TILES[(ki + wi + fi) % 2], full, M_CAND, MAPPINGS[(wi + fi) % 3]))
        W = (8, 16, 32, 64)[ki]      # an aircraft count below W: idle lanes in every lane group
        out.append((kernel, N_BELOW[W], 17, True, M_CAND, 2))
    out.append(("sampled", 16, 17, True, M_MANY, 64))
    out += [("skip", W, 17, full, 1, 0) for W in WIDTHS for full in (False, True)]
    name = lambda k, N, t, f, M, c: "%s N%d %s %dt%s" % (k, N, "full" if f else "fast", t, "" if k == "skip" else " M%d cpg%d" % (M, c))   # noqa: E731
    return [(name(*c),) + c for c in out]


CASES = _table()
IDS = [c[0] for c in CASES]
_CAND = [c for c in CASES if c[1] != "skip"]
_triple = lambda c: (c[1], H.lane_width(c[2]), c[4])   # noqa: E731  (kernel, W, form)
assert len(set(IDS)) == len(CASES) == 75
assert {_triple(c) for c in _CAND} == {(k, W, f) for k in KERNELS for W in WIDTHS for f in (False, True)}
assert all(c[2] == H.lane_width(c[2]) or c[2] == N_BELOW[H.lane_width(c[2])] for c in CASES)
assert all(sum(1 for c in _CAND if c[1] == k and c[2] != H.lane_width(c[2])) == 1 for k in KERNELS)
assert {(c[1], c[6], c[3]) for c in _CAND if c[5] == M_CAND} == {(k, m, t) for k in KERNELS for m in MAPPINGS for t in TILES}
assert {(H.lane_width(c[2]), c[3]) for c in _CAND} == {(W, t) for W in WIDTHS for t in TILES}
assert [c[1:] for c in _CAND if c[5] != M_CAND] == [("sampled", 16, 17, True, M_MANY, 64)]
assert sorted(_triple(c) + (c[3],) for c in CASES if c[1] == "skip") == sorted(("skip", W, f, 17) for W in WIDTHS for f in (False, True))
assert all(c[3] >= 9 for c in CASES)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_table_is_the_instantiation_set():
    """The k_lookahead, k_plan, k_plan_sampled, k_branch and k_skip instantiations of the built library (its demangled symbol table) are
    exactly the (kernel, W, form) set of CASES."""
    if not os.path.exists(LIB):
        pytest.skip("libatcstep.so not built yet (run __graft_entry__.build())")
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    kernel_of = {v: k for k, v in SYMBOL.items()}
    found = {(kernel_of[k], int(w), f == "true") for k, w, f in re.findall(r"\bvoid (%s)<(\d+), (true|false)>\(" % "|".join(SYMBOL.values()), text)}
    assert len(found) == 5 * 7 * 2, sorted(found)
    table = {_triple(c) for c in CASES}
    assert found == table, ("without a case: %s; cases without an instantiation: %s" % (sorted(found - table), sorted(table - found)))


def test_shape_helper():
    for W, B9, B17 in ((64, 33, 65), (1, 2051, 4099), (16, 131, 259)):
        assert (T.look_tiles(W, 9, True), T.look_tiles(W, 17, True)) == (B9, B17)
    assert T.look_tiles(33, 17, True) == 65 and T.look_tiles(16, 9, False) == 144 and T.look_tiles(64, 17, False) == 68


def _spawn(N):
    return "random" if N <= 8 else "lattice"


def _limit(N):
    return 7 if N <= 8 else 12


def _sep(N):
    return 5.0 if N <= 8 else 13.0 if N <= 16 else 3.0     # (held_tools.look_env's rule)


def _comp():
    from envs.atc import scenarios
    if "tiles" not in H._compiled:
        H._compiled["tiles"] = scenarios.compile_scenario(T.look_scenario(), grid_cell=0.5)
    return H._compiled["tiles"]


@functools.lru_cache(maxsize=None)
def _oracle_side(case):
    """Case `case` flown on the oracle alone; nothing in the record is changed afterwards.  flown: the actions of the flown calls;
    ok [B]: envs that are evaluated; cand / (mean, key): the call's input; refs: the reference dict per candidate (skip: one), orc: the
    oracle in the state the call starts from (skip: ends in)."""
    from oracle import oracle as O
    name, kernel, N, tiles, full, M, mapping = CASES[case]
    B, seed = T.look_tiles(N, tiles, True), 7000 + case
    orc = O.OracleEnv(_comp(), B, N, O.make_params(auto_reset=True, random_entry=_spawn(N) == "random", seed=seed, timestep_limit=_limit(N),
                                                   sep_nm=_sep(N)), np.float32)
    rng = np.random.default_rng(seed)
    rec = dict(B=B, seed=seed, flown=[], orc=orc)
    for Kf in FLOWN:
        a = draw_actions(rng, (B, N), False, 0.33, np.arange(B) % WILD_EVERY == WILD_AT)
        R.skip_reference(orc, a, Kf)
        rec["flown"].append((a, Kf))
    rec["ok"] = ~R.wide_envs(orc)

    def draw(*lead):    # candidates: speed and altitude components partly outside the action space (refused), headings inside it
        a = draw_actions(rng, lead + (B, N), False, 0.33, False)
        a[..., 2] = np.clip(a[..., 2], -1.0, 1.0)
        return a

    if kernel == "skip":
        rec["cand"] = draw_actions(rng, (B, N), False, 0.33, np.arange(B) % WILD_EVERY == WILD_AT)
        rec["refs"] = [R.skip_reference(orc, rec["cand"], K_ONE)]
    elif kernel in ("lookahead", "branch"):
        rec["cand"] = draw(M)
        rec["refs"] = R.candidate_references(orc, rec["cand"], K_ONE)
    elif kernel == "plan":
        rec["cand"] = draw(M, H_PLAN)
        rec["refs"] = R.plan_references(orc, rec["cand"], K_PLAN)
    else:
        rec["mean"] = np.clip(draw(H_PLAN), -1.0, 1.0)
        rec["key"] = dict(seed=seed, iteration=case, mean_first=True)
        rec["cand"] = P.draw(rec["mean"], STD, M, **rec["key"])
        rec["refs"] = R.plan_references(orc, rec["cand"], K_PLAN)
    return rec


def _shares(case):
    """what the twin asserts, as numbers: over the envs of tiles 8 and up"""
    name, kernel, N, tiles, full, M, mapping = CASES[case]
    rec = _oracle_side(case)
    B, W = rec["B"], H.lane_width(N)
    per = 256 // W
    limit = K_ONE if kernel in ("skip", "lookahead", "branch") else H_PLAN * K_PLAN
    ok = rec["ok"] if kernel != "skip" else np.ones(B, bool)     # (k_skip evaluates WIDE headings)
    hi = (np.arange(B) >= 8 * per) & ok
    last = (np.arange(B) >= (tiles - 1) * per) & ok
    n = np.stack([r["n_steps"].astype(int) for r in rec["refs"]])
    done = np.stack([r["done"].astype(bool) for r in rec["refs"]])
    rew = np.stack([r["reward"] for r in rec["refs"]])
    return dict(hi=int(hi.sum()), early=int((n < limit)[:, hi].sum()), reset=int((done & (n < limit))[:, hi].sum()),
                differ=int((rew.min(0) != rew.max(0))[hi].sum()), last_flying=int(((n > 1).all(0) & last).sum()),
                wide=int((~rec["ok"]).sum()), wide_hi=int((~rec["ok"])[8 * per:].sum()), B=B, pairs=int(n[:, hi].size))


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_case_on_the_oracle(case):
    """No GPU: the case's configuration on the oracle alone holds something to get wrong in the tiles past the first chunk."""
    kernel = CASES[case][1]
    s = _shares(case)
    print("tiles twin", IDS[case], s)
    assert s["hi"] > 0
    assert s["early"] > 0, "no env of tiles 8 and up stops early"
    assert s["reset"] > 0, "no env of tiles 8 and up resets inside the block"
    assert kernel == "skip" or 2 * s["differ"] >= s["hi"], "candidates differ in reward in fewer than half of the envs of tiles 8 and up"
    assert s["last_flying"] > 0, "the last tile holds no env that is evaluated and not done at its first step"
    assert s["wide"] <= WIDE_CAP * s["B"], ("more than a tenth of the (candidate, env) pairs are WIDE", s["wide"], s["B"])


def test_wide_envs_past_the_first_chunk():
    """every kernel has a case with an env that is not evaluated in tiles 8 and up: the zeros are written through the same decode"""
    for kernel in KERNELS:
        assert any(_shares(i)["wide_hi"] for i, c in enumerate(CASES) if c[1] == kernel), kernel


# ---------------------------------------------------------------------------------------------------------------- GPU
_SENTINEL = {"reward": 7.5, "done": 0xA5, "flags": 0x5A5A, "ac_reward": 7.5, "min_sep": 7.5, "obs": 7.5, "seg_reward": 7.5}
_times = {}


def _guarded_sampled(env, mean, std, K, M, key, outputs):
    """atc_lookahead_plan_sampled through ctypes into sentinel-filled tensors with guard rows (held_tools.guarded_call's layout)"""
    import torch
    from atc_hip import lib
    Hn, B, N, G = mean.shape[0], env.B, env.N, T.GUARD
    shapes = {"reward": ((B,), torch.float32, 7.5), "done": ((B,), torch.uint8, 0xA5), "n_steps": ((B,), torch.int16, 0x5A5A),
              "flags": ((B, N), torch.int16, 0x5A5A), "ac_reward": ((B, N), torch.float32, 7.5), "min_sep": ((B,), torch.float32, 7.5),
              "obs": ((B, N * 10), torch.float32, 7.5), "seg_reward": ((Hn, B), torch.float32, 7.5)}
    buf = {k: torch.full((M + 2 * G,) + shapes[k][0], shapes[k][2], dtype=shapes[k][1], device=env.device)
           for k in ("reward", "done", "n_steps") + tuple(outputs)}
    out = lib.AtcPlanOut(*[buf[k][G:].data_ptr() if k in buf else None for k in lib.PLAN_FIELDS])
    dr = lib.AtcPlanDraw(key["seed"], key["iteration"], L.DRAW_MEAN_FIRST if key["mean_first"] else 0)
    lib.check(lib.load().atc_lookahead_plan_sampled(env.sector.handle, B, N, K, Hn, M, C.byref(env._state), mean.data_ptr(), std.data_ptr(),
                                                    C.byref(dr), C.byref(out), C.byref(env.params), torch.cuda.current_stream().cuda_stream))
    env.synchronize()
    res = {}
    for k, t in buf.items():
        g = torch.cat([t[:G], t[G + M:]])
        assert bool((g == torch.full_like(g, shapes[k][2])).all()), "guard rows of %s overwritten" % k
        res[k] = t[G:G + M].cpu()
    return res


def _no_sentinel(got, n_steps_sentinel):
    """every row between the guard rows was written: the calls return zeros for an env that is not evaluated, and behind a plan's stop"""
    for k, v in got.items():
        s = n_steps_sentinel if k == "n_steps" else _SENTINEL[k]
        assert not bool((v == s).any()), ("a sentinel is left in output " + k, int((v == s).sum()))


def _moved(before, now):
    return {w: n - before.get(w, 0) for w, n in now.items() if n != before.get(w, 0)}


def _zeros(v):
    import torch
    return not bool(v.contiguous().view(torch.uint8).any())


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_every_env_past_the_first_chunk(case):
    import torch
    from atc_hip import lib
    t0 = time.time()
    name, kernel, N, tiles, full, M, mapping = CASES[case]
    rec = _oracle_side(case)
    B, seed, ok, orc = rec["B"], rec["seed"], rec["ok"], rec["orc"]
    W, comp = H.lane_width(N), _comp()
    half = bars.half_range(comp)
    if kernel == "skip":
        env = T.skip_env(T.look_scenario(), B, N, True, seed, full, spawn=_spawn(N), sep_nm=_sep(N), timestep_limit=_limit(N))
    else:
        env = T.look_env(N, B, _spawn(N), True, seed=seed, timestep_limit=_limit(N))
    try:
        assert -(-env.B * W // 256) == tiles
        for a, Kf in rec["flown"]:
            env.step_skip(a, Kf)
        dev = lambda a: torch.as_tensor(a, device=env.device)   # noqa: E731
        if kernel == "skip":
            outs = ("obs", "reward", "done", "flags") + (("raw_obs", "ac_reward", "min_sep") if full else ())
            for k in outs:          # (term_obs keeps what an env that does not end inside the call had: no sentinel there)
                getattr(env, k).fill_(0x5A5A if k == "flags" else 0xA5 if k == "done" else 7.5)
            env.frame_steps.fill_(0xA5)
            before = lib.skip_launch_counts()
            ret = env.step_skip(rec["cand"], K_ONE)
            env.synchronize()
            assert _moved(before, lib.skip_launch_counts()) == {W: 1}
            obs, rew, done, info = ret
            cpu = lambda t: t.cpu().numpy()   # noqa: E731
            got = {"flags": cpu(info["flags"]), "done": cpu(done), "n_steps": cpu(info["frame_steps"]), "obs": cpu(obs).reshape(B, N, 10),
                   "reward": cpu(rew)}
            if full:
                got.update(raw_obs=cpu(info["original_state"]).reshape(B, N, 10), ac_reward=cpu(info["aircraft_reward"]),
                           min_sep=cpu(info["min_separation"]), term_obs=cpu(info["terminal_observation"]).reshape(B, N, 10))
            assert not (got["n_steps"] == 0xA5).any() and not (got["done"] == 0xA5).any() and not (got["flags"].astype(np.uint16) == 0x5A5A).any()
            assert not any((got[k] == 7.5).any() for k in got if got[k].dtype == np.float32 and k != "term_obs"), "a sentinel is left"
            bars.check_skip_outputs(got, rec["refs"][0], half, full, name)
            bars.check_state(env, orc)
            return
        bars.check_state(env, orc)
        snap = H.snapshot(env)
        records = {"lookahead": lib.lookahead_launch_counts, "plan": lib.plan_launch_counts, "sampled": lib.plan_sampled_launch_counts,
                   "branch": lib.branch_launch_counts}
        if kernel == "branch":      # the reference first: the product's own step_skip per candidate, on the env's state (put back)
            ref, ref_state = BR.clone_reference(env, dev(rec["cand"]), K_ONE)
            H.bytes_equal(env, snap)
        before = {k: f() for k, f in records.items()}
        lib.lookahead_set_mapping(mapping)
        try:
            if kernel == "lookahead":
                got = T.guarded_call(env, "lookahead", dev(rec["cand"]), K_ONE, LOOK_ALL if full else ())
            elif kernel == "plan":
                got = T.guarded_call(env, "plan", dev(rec["cand"]), K_PLAN, PLAN_ALL if full else ("seg_reward",))
            elif kernel == "sampled":
                got = _guarded_sampled(env, dev(rec["mean"]), torch.full(rec["mean"].shape, STD, device=env.device), K_PLAN, M, rec["key"],
                                       PLAN_ALL if full else ("seg_reward",))
            else:
                got, rows = BR.guarded_branch(env, dev(rec["cand"]), K_ONE, LOOK_ALL if full else ())
        finally:
            lib.lookahead_set_mapping(0)
        assert {k: _moved(before[k], f()) for k, f in records.items() if _moved(before[k], f())} == {kernel: {W: 1}}
        H.bytes_equal(env, snap)
        _no_sentinel(got, 0xA5 if kernel in ("lookahead", "branch") else 0x5A5A)
        if kernel == "branch":
            okt = torch.as_tensor(ok)
            mask = okt[None].expand(M, B)
            T.assert_equal(got, ref, name, mask=mask)
            assert all(_zeros(v[~mask]) for v in got.values()), "an env that is not evaluated must return zeros"
            BR.assert_state_equal(rows, ref_state, name, env_mask=okt.repeat(M), N=N)
            src = {k: torch.cat([v.cpu()] * M) for k, v in snap.items()}      # not evaluated: the child's rows are the source's
            BR.assert_state_equal(rows, src, name + ", not evaluated", env_mask=~okt.repeat(M), N=N)
            for state, env_mask in ((ref_state, okt), (src, ~okt)):             # phi_wide is specified for saturated aircraft
                sat = BR.saturated(state) & env_mask.repeat(M).repeat_interleave(N)
                words = lambda st: st["phi_wide"][sat][:, :2].contiguous().view(torch.int64)   # noqa: E731
                assert torch.equal(words(rows), words(state))
            assert (ref["n_steps"].numpy()[:, ok] == np.stack([r["n_steps"] for r in rec["refs"]])[:, ok]).all()   # (the oracle agrees)
        else:
            g = {k: v.numpy() for k, v in got.items()}
            for m in range(M):
                bars.check_candidate_outputs({k: v[m] for k, v in g.items() if k != "seg_reward"}, rec["refs"][m], ok, half, tag=(name, m))
                if "seg_reward" in g:
                    bars.check_plan_segments(g["seg_reward"][m], rec["refs"][m], ok, K_PLAN, tag=(name, m))
        bars.check_state(env, orc)
    finally:
        env.close()
        _times[name] = time.time() - t0


@pytest.mark.gpu
def test_wall_times():
    """Runs after the cases (file order): prints each case's wall time once."""
    for name, t in sorted(_times.items(), key=lambda kv: -kv[1]):
        print("tiles case %-44s %.2f s" % (name, t))
    if _times:
        print("tiles cases: %d ran, slowest %.2f s, total %.1f s" % (len(_times), max(_times.values()), sum(_times.values())))
