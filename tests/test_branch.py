"""Branch (include/atc_step.h: atc_branch; AtcVecEnv.branch): M candidate decisions per env, K held steps each, every outcome KEPT as an
env of a second batch.

CPU: the exported symbols and kernel instantiations, the header's constants and prototypes against atc_hip/layout.py / lib.py, the
refusal order through ctypes with NULL and made-up pointer values (the overlap check reads no memory), the Python surface.
GPU: child rows [m B, (m + 1) B) of ac, alt, last_act, env, stats and every output BIT-IDENTICAL to the product's own step_skip run once
per candidate on the env's own state (tests/branch_ref.py::clone_reference; that path is held to the oracle by
tests/test_frame_skip.py); sentinel-filled dst with guard envs; src bytes; every launch record; every mapping, a permuted candidate
axis, M = 1; WIDE headings; branch + select against step_skip; two levels against lookahead_plan(H = 2).

Inputs are valid only if the REFERENCE shows, where the case can have them: candidates of one env with different n_steps, a reset inside
the call with the per-episode record advanced, a conflict flag and a handed-over aircraft.  _check_events asserts it."""
import ctypes as C
import inspect
import re
import shutil
import subprocess

import numpy as np
import pytest

import branch_ref as BR
import bars
import held_tools as T
import helpers as H
import skip_ref as R
from atc_hip import layout as L
from held_tools import HEADER, LIB

ALL = ("flags", "min_sep", "ac_reward", "obs")
NEW = ("atc_branch", "atc_branch_launch_counts", "atc_state_select", "atc_select_launch_counts")


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_exports_and_kernel_symbols():
    from atc_hip import lib
    assert set(NEW) <= set(lib.EXPORTS)
    h = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    found = set(re.findall(r"\bvoid k_branch<(\d+), (true|false)>\(", text))
    assert found == {(str(w), f) for w in (1, 2, 4, 8, 16, 32, 64) for f in ("true", "false")}, found
    assert re.search(r"\bk_select\(", text)


def test_header_constants_and_prototypes():
    from atc_hip import lib
    text = open(HEADER).read()
    assert L.BRANCH_LAUNCH_SLOTS == int(re.search(r"ATC_BRANCH_LAUNCH_SLOTS = (\d+)", text).group(1)) == 7
    assert L.SELECT_LAUNCH_SLOTS == int(re.search(r"ATC_SELECT_LAUNCH_SLOTS = (\d+)", text).group(1)) == 1
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("atc_branch", "atc_state_select"):
        proto = re.search(r"\bint %s\((.*?)\);" % name, flat, flags=re.S).group(1)
        assert len(proto.split(",")) == len(getattr(lib.load(), name).argtypes), name
    h = lib.load()
    assert h.atc_branch.argtypes[5]._type_ is lib.AtcState and h.atc_branch.argtypes[7]._type_ is lib.AtcState
    assert h.atc_branch.argtypes[8]._type_ is lib.AtcLookaheadOut


def test_branch_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    err = h.atc_last_error
    call = lambda K, M, src=None, dst=None, out=None, B=4, N=2: h.atc_branch(None, B, N, K, M, src, None, dst, out, None, None)   # noqa: E731
    for K in (0, 256, -3):
        for M in (0, 1, 65):    # K is looked at before M
            assert call(K, M) == -1 and b"K (" in err() and b"255" in err()
    for M in (0, 65, -1):
        assert call(1, M) == -1 and b"M (" in err() and b"64" in err()
    assert call(1, 1) == -1 and b"reward" in err()                       # out NULL
    assert call(1, 1, out=C.byref(lib.AtcLookaheadOut())) == -1 and b"reward" in err()
    out = lib.AtcLookaheadOut(reward=0x1000, done=0x2000)
    assert call(1, 3, out=C.byref(out)) == -1 and b"dst" in err()        # dst NULL
    src, end = BR.fake_state(0x10000000, 4, 2, lib)
    dst, _ = BR.fake_state(end, 12, 2, lib)
    hole = lib.AtcState(*[getattr(dst, n) for n in lib.STATE_FIELDS])
    hole.stats = None
    assert call(1, 3, C.byref(src), C.byref(hole), C.byref(out)) == -1 and b"dst" in err()
    # overlap: each dst array in turn starts inside a src array (its last byte), and a dst range that ends inside one
    for field in lib.STATE_FIELDS:
        over = lib.AtcState(*[getattr(dst, n) for n in lib.STATE_FIELDS])
        setattr(over, field, src.env + 4 * 16 - 1)
        assert call(1, 3, C.byref(src), C.byref(over), C.byref(out)) == -1 and b"overlaps" in err(), field
    over = lib.AtcState(*[getattr(dst, n) for n in lib.STATE_FIELDS])
    over.ac = src.ac - 12 * 2 * 16 + 1
    assert call(1, 3, C.byref(src), C.byref(over), C.byref(out)) == -1 and b"overlaps" in err()
    over.ac = src.ac - 12 * 2 * 16     # ends where src.ac begins: no shared byte, so the next check speaks (actions NULL)
    assert call(1, 3, C.byref(src), C.byref(over), C.byref(out)) == -1 and b"overlaps" not in err() and b"null" in err()
    # disjoint: M * B too large comes before the argument errors of atc_step
    big, _ = BR.fake_state(1 << 40, 4, 2, lib)
    assert call(1, 64, C.byref(src), C.byref(big), C.byref(out), B=1 << 20, N=64) == -1 and b"M*B" in err()
    assert call(1, 3, C.byref(src), C.byref(dst), C.byref(out)) == -1 and b"null" in err()
    buf = (C.c_uint64 * L.BRANCH_LAUNCH_SLOTS)()
    assert h.atc_branch_launch_counts(buf, L.BRANCH_LAUNCH_SLOTS) == 0 and isinstance(lib.branch_launch_counts(), dict)


def test_python_surface():
    import torch
    from atc_hip import sb_adapter
    from atc_hip.vec_env import AtcVecEnv
    assert list(inspect.signature(AtcVecEnv.branch).parameters) == ["self", "actions", "K", "into"]
    assert list(inspect.signature(AtcVecEnv.select).parameters) == ["self", "src", "index", "mask"]
    assert inspect.signature(AtcVecEnv.select).parameters["mask"].default is None
    for name in ("branch", "select"):
        assert not hasattr(sb_adapter.AtcSBVecEnv, name)     # deliberately out of scope
    env = object.__new__(AtcVecEnv)     # the checks that come before anything touches a device
    env.B, env.N, env.torch = 4, 2, torch
    a = np.zeros((3, 4, 2, 3), np.float32)
    for K in (0, 256):
        with pytest.raises(ValueError):
            env.branch(a, K, into=None)
    with pytest.raises(ValueError):
        env.branch(np.zeros((65, 4, 2, 3), np.float32), 4, into=None)
    for other in (None, object(), env):
        with pytest.raises(ValueError):
            env.branch(a, 4, into=other)
        with pytest.raises(ValueError):
            env.select(other, np.zeros(4, np.int32))


# ---------------------------------------------------------------------------------------------------------------- GPU
def _check_events(ref, state, src_stats, N, M, K, auto_reset):
    n = ref["n_steps"].numpy().astype(int)
    fl = ref["flags"].numpy().astype(np.uint16)
    assert n.min() >= 1 and n.max() <= K
    if M > 1 and K >= 4:
        assert (n.min(0) != n.max(0)).any(), "no env whose candidates stop at different n"
    if auto_reset:
        done = ref["done"].numpy().astype(bool)
        assert done.any(), "no reset inside the call"
        ep = state["stats"][:, L.STAT_EPISODES].numpy().reshape(M, -1)
        assert (ep[done] == np.broadcast_to(src_stats[:, L.STAT_EPISODES].numpy(), ep.shape)[done] + 1).all(), "episodes + 1 on a reset"
        assert (ep[~done] == np.broadcast_to(src_stats[:, L.STAT_EPISODES].numpy(), ep.shape)[~done]).all()
    if N > 1:
        assert (fl & H.F_CONFLICT).any(), "no conflict flag"
        assert (fl & H.F_INACTIVE).any(), "no handed-over aircraft"


# (N, M, K, auto_reset, spawn, normalize, outputs): every N of the grid, M in {1, 3}, K in {1, 4, 20}, each switch both ways, the fast form
# (no optional output) and the full form with each optional output absent in at least one case
CASES = [
    (1, 3, 4, True, "random", True, ()),
    (1, 3, 20, False, "lattice", False, ALL),
    (2, 1, 1, True, "lattice", True, ("flags",)),
    (2, 3, 4, True, "random", False, ("min_sep", "obs")),
    (3, 3, 20, True, "random", True, ALL),
    (3, 1, 4, False, "lattice", True, ()),
    (8, 3, 20, True, "lattice", False, ("ac_reward",)),
    (8, 3, 1, False, "random", True, ("flags", "min_sep")),
    (16, 3, 4, True, "lattice", True, ALL),
    (16, 3, 20, True, "random", False, ()),
    (16, 1, 20, False, "lattice", True, ("obs",)),
    (32, 3, 4, True, "lattice", True, ALL),
    (32, 3, 20, False, "random", False, ()),
    (33, 3, 20, True, "lattice", True, ("flags", "ac_reward")),
    (33, 1, 4, True, "random", False, ()),
    (64, 3, 4, True, "lattice", False, ALL),
    (64, 3, 20, False, "lattice", True, ()),
]
IDS = ["N%d M%d K%d %s %s %s %s" % (c[0], c[1], c[2], "reset" if c[3] else "noreset", c[4], "norm" if c[5] else "raw",
                                    "+".join(c[6]) or "fast") for c in CASES]


def _records():
    from atc_hip import lib
    return (lib.branch_launch_counts(), lib.select_launch_counts(), lib.lookahead_launch_counts(), lib.plan_launch_counts(),
            lib.skip_launch_counts(), lib.launch_counts(), lib.traffic_launch_counts())


def _case(N, spawn, normalize, auto_reset, rng, M):
    import torch
    B = T.look_ragged(N)
    env = T.look_env(N, B, spawn, normalize)
    T.look_fly(env, rng)
    H.set_auto_reset(env, auto_reset)
    actions = torch.as_tensor(T.look_draw(rng, M, B, N), device=env.device)
    if M > 1:   # env 0: candidate 0 descends as fast as it may, candidate 1 climbs
        actions[0, 0, 0, 1], actions[1, 0, 0, 1] = -0.9, 0.9
    return env, actions


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N,M,K,auto_reset,spawn,normalize,outputs", CASES, ids=IDS)
def test_branch_equals_step_skip_on_copies(N, M, K, auto_reset, spawn, normalize, outputs):
    import torch
    from atc_hip import lib
    case = CASES.index((N, M, K, auto_reset, spawn, normalize, outputs))
    rng = np.random.default_rng(2000 + 7 * case)
    env, actions = _case(N, spawn, normalize, auto_reset, rng, M)
    B = env.B
    ref, ref_state = BR.clone_reference(env, actions, K)
    _check_events(ref, ref_state, env.stats.cpu(), N, M, K, auto_reset)
    snap = H.snapshot(env)
    before = _records()
    got, rows = BR.guarded_branch(env, actions, K, outputs, n_steps=(case % 4 != 3))
    assert set(got) >= {"reward", "done"} | set(outputs)
    T.assert_equal(got, ref, "guarded")
    BR.assert_state_equal(rows, ref_state, "guarded")
    H.bytes_equal(env, snap)
    now = _records()
    W = H.lane_width(N)
    assert {w: n - before[0].get(w, 0) for w, n in now[0].items() if n != before[0].get(w, 0)} == {W: 1}
    assert now[1:] == before[1:]
    # the Python surface into a real child env: every mapping, a permuted candidate axis, M = 1
    child = BR.child_of(env, M, lambda b: T.look_env(N, b, spawn, normalize))
    one = BR.child_of(env, 1, lambda b: T.look_env(N, b, spawn, normalize))
    bound = {k: getattr(env, k).clone() for k in ("obs", "reward", "done", "flags")}
    perm = torch.as_tensor(rng.permutation(M), device=env.device)

    def check(ch, r, rs, tag):
        obs, rew, done, info = r
        res = {"obs": obs.view(-1, B, N * 10), "reward": rew.view(-1, B), "done": done.view(-1, B), "n_steps": info["frame_steps"].view(-1, B),
               "flags": info["flags"].view(-1, B, N), "ac_reward": info["aircraft_reward"].view(-1, B, N), "min_sep": info["min_separation"].view(-1, B)}
        T.assert_equal({k: v.cpu() for k, v in res.items()}, rs[0], tag)
        BR.assert_state_equal({k: getattr(ch, k).cpu() for k in H.STATE}, rs[1], tag)

    pc = perm.cpu()
    sel = lambda st, idx: {k: v.view(M, -1, *v.shape[1:])[idx].reshape(-1, *v.shape[1:]) for k, v in st.items()}   # noqa: E731
    for cpg in (1, M, 2, 0):
        lib.lookahead_set_mapping(cpg)
        check(child, env.branch(actions.view(M, B, N * 3), K, into=child), (ref, ref_state), ("python", cpg))
        check(child, env.branch(actions[perm], K, into=child), ({k: v[pc] for k, v in ref.items()}, sel(ref_state, pc)), ("permuted", cpg))
        check(one, env.branch(actions[:1], K, into=one), ({k: v[:1] for k, v in ref.items()}, sel(ref_state, slice(0, 1))), ("M = 1", cpg))
    for k, v in bound.items():
        assert torch.equal(getattr(env, k), v), k
    H.bytes_equal(env, snap)
    for e in (env, child, one):
        e.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N", [1, 16, 33])
def test_wide_headings_are_not_evaluated(N):
    import torch
    B, M, K = T.look_ragged(N), 3, 4
    rng = np.random.default_rng(177 + N)
    env = T.look_env(N, B, "lattice", True)
    T.look_fly(env, rng, steps=40)
    e_wide = B - 1
    env.set_state(e_wide, N - 1, *H.FAR_B[:3], 500.0, H.FAR_B[4])    # 500 deg: beyond the 32-bit heading field
    assert int(env.phi_fix[e_wide * N + N - 1]) == L.I32_MAX
    actions = torch.as_tensor(T.look_draw(rng, M, B, N), device=env.device)
    actions[1, 3, 0, 2] = 3.0          # candidate 1, env 3: a heading target of 720 deg saturates the accepted target in step one
    bad = torch.zeros((M, B), dtype=torch.bool)
    bad[:, e_wide] = True
    bad[1, 3] = True
    ref, ref_state = BR.clone_reference(env, actions, K)    # (step_skip evaluates WIDE headings: its rows of `bad` are not compared)
    snap = H.snapshot(env)
    got, rows = BR.guarded_branch(env, actions, K, ALL)
    H.bytes_equal(env, snap)
    T.assert_equal(got, ref, "evaluated", mask=~bad)
    BR.assert_state_equal(rows, ref_state, "evaluated", env_mask=~bad.reshape(-1), N=N)
    for k, v in got.items():
        assert not bool(v[bad].view(torch.uint8 if v.dtype == torch.uint8 else torch.int32 if v.dtype == torch.float32 else torch.int16).any()), k
    assert bool((got["n_steps"][~bad] >= 1).all())
    # not evaluated: the child's rows are the source's, the side record of the saturated aircraft included (words 0..1)
    src = {k: torch.cat([v.cpu()] * M) for k, v in snap.items()}
    BR.assert_state_equal(rows, src, "not evaluated", env_mask=bad.reshape(-1), N=N)
    sat = BR.saturated(src) & bad.reshape(-1).repeat_interleave(N)
    assert int(sat.sum()) == M
    assert torch.equal(rows["phi_wide"][sat][:, :2].contiguous().view(torch.int64), src["phi_wide"][sat][:, :2].contiguous().view(torch.int64))
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N", [1, 16, 33])
def test_branch_then_select_commits_without_recomputation(N):
    """root.branch(cand, K, into=child); root.select(child, best * B + e) == root.step_skip(cand[best], K) on a clone: state bytes and obs"""
    import torch
    M, K = 3, 4
    rng = np.random.default_rng(300 + N)
    env, actions = _case(N, "lattice", True, True, rng, M)
    B = env.B
    child = BR.child_of(env, M, lambda b: T.look_env(N, b, "lattice", True))
    _, reward, _, _ = env.branch(actions, K, into=child)
    best = reward.view(M, B).argmax(0)
    best[0] = 0          # env 0 commits the candidate that descends below its floor: a reset inside the committed block
    assert len(set(best.tolist())) > 1
    pick = actions[best, torch.arange(B, device=env.device)]
    ref, ref_state = BR.clone_reference(env, pick[None], K)
    assert ref["done"].any()
    env.select(child, best * B + torch.arange(B, device=env.device))
    BR.assert_state_equal({k: getattr(env, k).cpu() for k in H.STATE}, ref_state, "committed")
    assert torch.equal(env.obs.cpu().view(torch.int32), ref["obs"][0].view(torch.int32))
    for e in (env, child):
        e.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_two_levels_equal_a_plan_of_two_segments():
    """reward of level 1 + level 2 == lookahead_plan(H = 2)'s seg_reward, bit for bit, on every env not done in segment 0"""
    import torch
    N, M, K = 16, 2, 6
    rng = np.random.default_rng(41)
    env, c1 = _case(N, "lattice", True, True, rng, M)
    B = env.B
    c2 = torch.as_tensor(T.look_draw(rng, M, M * B, N), device=env.device)
    l1 = BR.child_of(env, M, lambda b: T.look_env(N, b, "lattice", True))
    l2 = BR.child_of(env, M * M, lambda b: T.look_env(N, b, "lattice", True))
    _, r1, d1, _ = env.branch(c1, K, into=l1)
    r1, d1 = r1.clone().view(M, B), d1.clone().view(M, B)
    _, r2, _, _ = l1.branch(c2, K, into=l2)
    r2 = r2.view(M, M, B)          # [second decision, first decision, env]
    assert bool(d1.any()) and not bool(d1.all())
    for m2 in range(M):
        plans = torch.stack([c1, c2[m2].view(M, B, N, 3)], dim=1)         # [M, H = 2, B, N, 3]: first decision m1, then m2
        seg = env.lookahead_plan(plans, K, outputs=("seg_reward",))["seg_reward"]
        alive = d1 == 0
        assert torch.equal(seg[:, 0].view(torch.int32), r1.view(torch.int32))
        assert torch.equal(seg[:, 1][alive].view(torch.int32), r2[m2][alive].view(torch.int32))
    for e in (env, l1, l2):
        e.close()


def _child_outputs(child, M):
    B, N = child.B // M, child.N
    return {"obs": child.obs.view(M, B, N * 10), "reward": child.reward.view(M, B), "done": child.done.view(M, B),
            "n_steps": child.frame_steps.view(M, B), "flags": child.flags.view(M, B, N), "ac_reward": child.ac_reward.view(M, B, N),
            "min_sep": child.min_sep.view(M, B)}


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("N", [1, 2, 3, 8, 16, 32, 64])
def test_branch_against_the_oracle(N):
    """A second reference, one case per width: tests/skip_ref.py on the CPU oracle — outputs at the frame-skip bars of tests/bars.py, the
    integer state of every child env exact (bars.check_state).  Device and oracle fly the same frame-skip calls from the same seed, then
    every candidate is flown on the oracle from a snapshot."""
    import torch
    scn, comp = T.skip_setup(N)
    kw = T.skip_plan(N)
    B, M, K, seed = T.look_ragged(N), 3, 10, 6321 + N    # (4 steps flown + K exceed the plans' time limits of 7 / 12: envs stop early)
    env = T.skip_env(scn, B, N, True, seed, True, **kw)
    child = T.skip_env(scn, M * B, N, True, seed, True, **kw)
    orc = T.skip_oracle(comp, B, N, True, seed, **kw)
    rng = np.random.default_rng(seed)
    for Kf in (3, 1):
        a = T.skip_actions(rng, B, N)
        a[..., 2] = np.clip(a[..., 2], -1.0, 1.0)    # (headings inside the action space: nothing is WIDE when the branch starts)
        R.skip_reference(orc, a, Kf)
        env.step_skip(a, Kf)
    bars.check_state(env, orc)
    cand = T.skip_actions(rng, M * B, N).reshape(M, B, N, 3)
    cand[..., 2] = np.clip(cand[..., 2], -1.0, 1.0)
    ok = ~R.wide_envs(orc)
    assert ok.all()
    snap = H.snapshot(env)
    env.branch(torch.as_tensor(cand, device=env.device), K, into=child)
    got = {k: v.cpu().numpy() for k, v in _child_outputs(child, M).items()}
    refs = BR.oracle_branch(orc, cand, K, ok, BR.child_check(child, orc, got, bars.half_range(comp), ok, N))
    assert sum(int((r["n_steps"] < K).sum()) for r in refs) > 0
    assert any(r["done"].any() for r in refs)
    H.bytes_equal(env, snap)
    bars.check_state(env, orc)
    for e in (env, child):
        e.close()


def _branches(env):
    """the branch calls of both forms that tests/held_tools.py::scripted makes between its calls, into child envs of its own"""
    import torch
    cand = torch.as_tensor(T.look_draw(np.random.default_rng(10), 3, env.B, env.N), device=env.device)
    make = lambda b: type(env)(b, env.N, scenario=T.look_scenario(), auto_reset=True, spawn="lattice", seed=5, grid_cell=0.5, timestep_limit=15,   # noqa: E731
                               sep_nm=13.0)
    c3, c2 = BR.child_of(env, 3, make), BR.child_of(env, 2, make)

    def branch():
        env.branch(cand, 6, into=c3)
        env.branch(cand[:2], 3, into=c2)
        c2.select(c3, torch.arange(c2.B, device=env.device))
    return branch


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_branches_between_calls_change_nothing():
    """the parent's trajectory — every output of a scripted call sequence and the final state — is the same with and without branch calls"""
    import torch
    plain, mixed = T.scripted(), T.scripted(_branches)
    assert len(plain) == len(mixed)
    for j, (a, b) in enumerate(zip(plain, mixed)):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), j
    assert any(bool(t.any()) for t in plain if t.dtype == torch.uint8)    # an episode ended inside the script


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_full_size_batch():
    """65 536 x 16, M = 2, K = 2 in one call: the first 256 envs of each candidate against step_skip on copies, the rest through properties
    (1 <= n_steps <= K, n_steps == K unless done, the child's timestep and episode records consistent with them) and the src bytes.
    (The exact check of the tile decode past one chunk, on every env: tests/test_candidate_tiles.py.)"""
    import torch
    B, N, M, K = 65536, 16, 2, 2
    rng = np.random.default_rng(3)
    make = lambda b: T.look_env(N, b, "lattice", True, seed=3, timestep_limit=30)   # noqa: E731
    env, small = make(B), make(256)
    a0 = T.look_draw(rng, 3, B, N)
    env.rollout(torch.as_tensor(a0, device=env.device), hold=9)
    small.rollout(torch.as_tensor(a0[:, :256].copy(), device=env.device), hold=9)
    for k in H.STATE:     # envs are independent and the sampler is keyed by the env index: the small env IS the first 256
        rows = 256 * N if getattr(env, k).shape[0] == B * N else 256
        assert torch.equal(getattr(env, k)[:rows], getattr(small, k))
    actions = torch.as_tensor(T.look_draw(rng, M, B, N), device=env.device)
    ref, ref_state = BR.clone_reference(small, actions[:, :256].contiguous(), K)
    assert ref["done"].any()
    child = BR.child_of(env, M, make)
    snap = H.snapshot(env)
    env.branch(actions, K, into=child)
    H.bytes_equal(env, snap)
    out = _child_outputs(child, M)
    T.assert_equal({k: v[:, :256].cpu() for k, v in out.items()}, ref, "full size")
    first = {k: torch.cat([getattr(child, k).view(M, B, -1)[m, :256].reshape(-1, *getattr(child, k).shape[1:]) for m in range(M)]).cpu() for k in H.STATE}
    BR.assert_state_equal(first, ref_state, "full size")
    n, done = out["n_steps"], out["done"]
    assert bool(((n >= 1) & (n <= K)).all()) and bool((n[done == 0] == K).all())
    t0, ep0 = env.timesteps.reshape(1, B), env.episodes.reshape(1, B)
    t1, ep1 = child.timesteps.reshape(M, B), child.episodes.reshape(M, B)
    assert bool((ep1 == ep0 + done.int()).all())
    assert bool((t1[done == 0] == (t0 + n.int())[done == 0]).all()) and bool((t1[done != 0] == 0).all())
    for e in (env, small, child):
        e.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_branch_leaves_the_childs_raw_and_terminal_observation_alone():
    """atc_lookahead_out_t has neither: AtcVecEnv.branch documents that into.raw_obs / into.term_obs keep what they held"""
    import torch
    scn, _ = T.skip_setup(16)
    kw = T.skip_plan(16)
    env, child = T.skip_env(scn, 8, 16, True, 1, True, **kw), T.skip_env(scn, 16, 16, True, 1, True, **kw)
    child.raw_obs.fill_(7.5)
    child.term_obs.fill_(-7.5)
    env.branch(torch.as_tensor(T.look_draw(np.random.default_rng(1), 2, 8, 16), device=env.device), 20, into=child)
    assert bool(child.done.any())
    assert bool((child.raw_obs == 7.5).all()) and bool((child.term_obs == -7.5).all())
    for e in (env, child):
        e.close()
