"""What-if look-ahead (include/atc_step.h: atc_lookahead; AtcVecEnv.lookahead): M candidate decisions per env, K held steps each, in
one launch that never writes state.

CPU: the exported symbols, the header's constants against atc_hip/layout.py, the refusal order (K before M before pointers) through
ctypes with NULL pointers, the Python surface.
GPU: every output BIT-IDENTICAL to the product's own atc_step_skip run once per candidate on torch.clones of the six state tensors
(that path is held to the oracle by tests/test_frame_skip.py; sums in a fixed order and integer words: no tolerance applies); one
case per width also against tests/skip_ref.py on the oracle (the bars of tests/bars.py); guard rows; the six state tensors byte for
byte; the launch record; permutation of the candidate axis; both candidate mappings; WIDE headings; a scripted call sequence with and
without look-aheads in between; 65 536 x 16.

Inputs are valid only if the REFERENCE results show, where the case can have them: an env whose candidates stop at different n
(M > 1, K >= 4), a look-ahead reset (auto-reset), a conflict flag and a handed-over aircraft (N > 1).  _check_events asserts it."""
import ctypes as C
import inspect
import re
import shutil
import subprocess

import numpy as np
import pytest

import bars
import held_tools as T
import helpers as H
import skip_ref as R
from atc_hip import layout as L
from held_tools import HEADER, LIB

OPTIONAL = ("flags", "min_sep", "ac_reward", "obs")
ALL = OPTIONAL


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_exports_and_kernel_symbols():
    from atc_hip import lib
    assert {"atc_lookahead", "atc_lookahead_launch_counts", "atc_lookahead_set_mapping"} <= set(lib.EXPORTS)
    h = C.CDLL(LIB)
    for name in ("atc_lookahead", "atc_lookahead_launch_counts", "atc_lookahead_set_mapping"):
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    found = set(re.findall(r"\bvoid k_lookahead<(\d+), (true|false)>\(", text))
    assert found == {(str(w), f) for w in (1, 2, 4, 8, 16, 32, 64) for f in ("true", "false")}, found


def test_header_constants_match_layout():
    text = open(HEADER).read()
    assert L.LOOKAHEAD_MAX_M == int(re.search(r"#define ATC_LOOKAHEAD_MAX_M (\d+)", text).group(1)) == 64
    assert L.LOOKAHEAD_LAUNCH_SLOTS == int(re.search(r"ATC_LOOKAHEAD_LAUNCH_SLOTS = (\d+)", text).group(1)) == 7
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22
    from atc_hip import lib
    body = re.search(r"typedef struct atc_lookahead_out \{(.*?)\} atc_lookahead_out_t;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == list(lib.LOOKAHEAD_FIELDS) == [f[0] for f in lib.AtcLookaheadOut._fields_]


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    call = lambda K, M, out=None: h.atc_lookahead(None, 1, 1, K, M, None, None, out, None, None)   # noqa: E731
    for K in (0, 256, -3):
        for M in (0, 1, 65):    # K is looked at before M
            assert call(K, M) == -1 and b"K (" in h.atc_last_error() and b"255" in h.atc_last_error()
    for M in (0, 65, -1):
        assert call(1, M) == -1 and b"M (" in h.atc_last_error() and b"64" in h.atc_last_error()
    assert call(1, 1) == -1 and b"null" in h.atc_last_error()             # K and M in range: now the pointers
    out = lib.AtcLookaheadOut()                                            # reward / done NULL comes before everything else's NULL
    assert call(255, 64, C.byref(out)) == -1 and b"reward" in h.atc_last_error()
    buf = (C.c_uint64 * L.LOOKAHEAD_LAUNCH_SLOTS)()
    assert h.atc_lookahead_launch_counts(buf, L.LOOKAHEAD_LAUNCH_SLOTS) == 0
    assert isinstance(lib.lookahead_launch_counts(), dict)
    assert h.atc_lookahead_set_mapping(65) == -1 and h.atc_lookahead_set_mapping(-1) == -1 and h.atc_lookahead_set_mapping(0) == 0


def test_python_surface():
    from atc_hip.vec_env import AtcVecEnv
    sig = inspect.signature(AtcVecEnv.lookahead)
    assert list(sig.parameters) == ["self", "actions", "K", "outputs"]
    assert sig.parameters["outputs"].default == ("flags", "min_sep")
    from atc_hip import sb_adapter
    assert not hasattr(sb_adapter.AtcSBVecEnv, "lookahead")   # deliberately out of scope


# ---------------------------------------------------------------------------------------------------------------- GPU
def _reference(env, actions, K):
    """held_tools.chained_skip_reference at H = 1, without its per-segment keys; n_steps as atc_lookahead's uint8 (assert_equal reinterprets
    the reference by the result's dtype)"""
    import torch
    ref = T.chained_skip_reference(env, actions[:, None], K)
    return {k: (v.to(torch.uint8) if k == "n_steps" else v) for k, v in ref.items() if not k.startswith("seg_")}


def _check_events(ref, N, M, K, auto_reset):
    n = ref["n_steps"].numpy().astype(int)
    fl = ref["flags"].numpy().astype(np.uint16)
    assert n.min() >= 1 and n.max() <= K
    if M > 1 and K >= 4:
        assert (n.min(0) != n.max(0)).any(), "no env whose candidates stop at different n"
    if auto_reset:
        assert ref["done"].numpy().any(), "no look-ahead reset"
    if N > 1:
        assert (fl & H.F_CONFLICT).any(), "no conflict flag"
        assert (fl & H.F_INACTIVE).any(), "no handed-over aircraft"


# (N, M, K, auto_reset, spawn, normalize, outputs): every N of the grid, M in {1, 3, 8}, K in {1, 4, 20}, each switch both ways, the fast
# form (no optional output) and the full form with each optional output absent in at least one case
CASES = [
    (1, 3, 4, True, "random", True, ()),
    (1, 8, 20, False, "lattice", False, ALL),
    (2, 1, 1, True, "lattice", True, ("flags",)),
    (2, 8, 4, True, "random", False, ("min_sep", "obs")),
    (3, 3, 20, True, "random", True, ALL),
    (3, 1, 4, False, "lattice", True, ()),
    (8, 8, 20, True, "lattice", False, ("ac_reward",)),
    (8, 3, 1, False, "random", True, ("flags", "min_sep")),
    (16, 8, 4, True, "lattice", True, ALL),
    (16, 3, 20, True, "random", False, ()),
    (16, 1, 20, False, "lattice", True, ("obs",)),
    (32, 3, 4, True, "lattice", True, ALL),
    (32, 8, 20, False, "random", False, ()),
    (33, 3, 20, True, "lattice", True, ("flags", "ac_reward")),
    (33, 1, 4, True, "random", False, ()),
    (64, 8, 4, True, "lattice", False, ALL),
    (64, 3, 20, False, "lattice", True, ()),
]
IDS = ["N%d M%d K%d %s %s %s %s" % (c[0], c[1], c[2], "reset" if c[3] else "noreset", c[4], "norm" if c[5] else "raw",
                                    "+".join(c[6]) or "fast") for c in CASES]


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N,M,K,auto_reset,spawn,normalize,outputs", CASES, ids=IDS)
def test_lookahead_equals_step_skip_on_copies(N, M, K, auto_reset, spawn, normalize, outputs):
    import torch
    from atc_hip import lib
    B = T.look_ragged(N)
    rng = np.random.default_rng(1000 + 7 * CASES.index((N, M, K, auto_reset, spawn, normalize, outputs)))
    env = T.look_env(N, B, spawn, normalize)
    T.look_fly(env, rng)
    H.set_auto_reset(env, auto_reset)
    actions = torch.as_tensor(T.look_draw(rng, M, B, N), device=env.device)
    if M > 1:   # env 0: candidate 0 descends as fast as it may, candidate 1 climbs
        actions[0, 0, 0, 1], actions[1, 0, 0, 1] = -0.9, 0.9
    ref = _reference(env, actions, K)
    _check_events(ref, N, M, K, auto_reset)
    snap = H.snapshot(env)
    before = (lib.lookahead_launch_counts(), lib.skip_launch_counts(), lib.launch_counts(), lib.traffic_launch_counts())
    got = T.guarded_call(env, "lookahead", actions, K, outputs, n_steps=(CASES.index((N, M, K, auto_reset, spawn, normalize, outputs)) % 4 != 3))
    assert set(got) >= {"reward", "done"} | set(outputs)
    T.assert_equal(got, ref, "guarded")
    H.bytes_equal(env, snap)
    now = lib.lookahead_launch_counts()
    W = H.lane_width(N)
    assert {w: n - before[0].get(w, 0) for w, n in now.items() if n != before[0].get(w, 0)} == {W: 1}
    assert (lib.skip_launch_counts(), lib.launch_counts(), lib.traffic_launch_counts()) == before[1:]
    # the Python surface: the same numbers, env outputs untouched; both candidate mappings; a permuted candidate axis; M = 1
    bound = {k: getattr(env, k).clone() for k in ("obs", "reward", "done", "flags")}
    perm = torch.as_tensor(rng.permutation(M), device=env.device)
    for cpg in (1, M, 2, 0):
        lib.lookahead_set_mapping(cpg)
        res = env.lookahead(actions.view(M, B, N * 3), K, outputs=outputs)
        assert set(res) == {"reward", "done", "n_steps"} | set(outputs)
        assert res["reward"].shape == (M, B) and res["n_steps"].dtype == torch.uint8
        T.assert_equal({k: v.cpu() for k, v in res.items()}, ref, ("python", cpg))
        first = env.lookahead(actions, K, outputs=outputs)
        assert all(first[k].data_ptr() == res[k].data_ptr() for k in res), "output tensors are allocated once per (M, outputs)"
        p = env.lookahead(actions[perm], K, outputs=outputs)
        T.assert_equal({k: v.cpu() for k, v in p.items()}, {k: v[perm.cpu()] for k, v in ref.items()}, ("permuted", cpg))
        one = env.lookahead(actions[:1], K, outputs=outputs)
        T.assert_equal({k: v.cpu() for k, v in one.items()}, {k: v[:1] for k, v in ref.items()}, ("M = 1", cpg))
    for k, v in bound.items():
        assert torch.equal(getattr(env, k), v), k
    H.bytes_equal(env, snap)
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("N", [1, 2, 3, 8, 16, 32, 64])
def test_lookahead_against_the_oracle(N):
    """A second reference, one case per width: tests/skip_ref.py on the CPU oracle, under the bars of tests/bars.py — device and oracle
    fly the same frame-skip calls from the same seed, then every candidate is evaluated on the oracle from a snapshot."""
    import torch
    scn, comp = T.skip_setup(N)
    kw = T.skip_plan(N)
    B, M, K, seed = T.look_ragged(N), 3, 10, 4321 + N    # (4 steps flown + K exceed the plans' time limits of 7 / 12: envs stop early)
    env = T.skip_env(scn, B, N, True, seed, True, **kw)
    orc = T.skip_oracle(comp, B, N, True, seed, **kw)
    rng = np.random.default_rng(seed)
    for Kf in (3, 1):
        a = T.skip_actions(rng, B, N)
        a[..., 2] = np.clip(a[..., 2], -1.0, 1.0)    # (headings inside the action space: nothing is WIDE when the look-ahead starts)
        R.skip_reference(orc, a, Kf)
        env.step_skip(a, Kf)
    bars.check_state(env, orc)
    # headings inside the action space (a WIDE target is not evaluated: its own test), speeds and altitudes partly refused
    cand = T.skip_actions(rng, M * B, N).reshape(M, B, N, 3)
    cand[..., 2] = np.clip(cand[..., 2], -1.0, 1.0)
    wide0 = R.wide_envs(orc)
    assert not wide0.all()
    res = env.lookahead(torch.as_tensor(cand, device=env.device), K, outputs=ALL)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    early = 0
    for m, ref in enumerate(R.candidate_references(orc, cand, K)):
        bars.check_candidate_outputs({k: v[m] for k, v in got.items()}, ref, ~wide0, bars.half_range(comp), tag=(N, m))
        early += int((ref["n_steps"][~wide0] < K).sum())
    assert early > 0
    bars.check_state(env, orc)
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N", [1, 16, 33])
def test_wide_headings_are_not_evaluated(N):
    import torch
    B, M, K = T.look_ragged(N), 3, 4
    rng = np.random.default_rng(77 + N)
    env = T.look_env(N, B, "lattice", True)
    T.look_fly(env, rng, steps=40)
    e_wide = B - 1
    env.set_state(e_wide, N - 1, *H.FAR_B[:3], 500.0, H.FAR_B[4])    # 500 deg: beyond the 32-bit heading field
    assert int(env.phi_fix[e_wide * N + N - 1]) == L.I32_MAX
    actions = torch.as_tensor(T.look_draw(rng, M, B, N), device=env.device)
    actions[1, 3, 0, 2] = 3.0          # candidate 1, env 3: a heading target of 720 deg saturates the accepted target
    bad = torch.zeros((M, B), dtype=torch.bool)
    bad[:, e_wide] = True
    bad[1, 3] = True
    ref = _reference(env, actions, K)    # (step_skip evaluates WIDE headings: its rows of `bad` are not compared)
    snap = H.snapshot(env)
    got = T.guarded_call(env, "lookahead", actions, K, ALL)
    H.bytes_equal(env, snap)
    T.assert_equal(got, ref, "evaluated", mask=~bad)
    for k, v in got.items():
        assert not bool(v[bad].view(torch.uint8 if v.dtype == torch.uint8 else torch.int32 if v.dtype == torch.float32 else torch.int16).any()), k
    assert bool((got["n_steps"][~bad] >= 1).all())
    env.close()


def _lookaheads(env):
    """the look-ahead calls of both forms that tests/held_tools.py::scripted makes between its calls"""
    import torch
    cand = torch.as_tensor(T.look_draw(np.random.default_rng(10), 3, env.B, env.N), device=env.device)

    def look():
        env.lookahead(cand, 6, outputs=ALL)
        env.lookahead(cand[:2], 3, outputs=())
    return look


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_lookaheads_between_calls_change_nothing():
    import torch
    plain, mixed = T.scripted(), T.scripted(_lookaheads)
    assert len(plain) == len(mixed)
    for j, (a, b) in enumerate(zip(plain, mixed)):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), j
    assert any(bool(t.any()) for t in plain if t.dtype == torch.uint8)    # an episode ended inside the script


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_full_size_batch():
    """65 536 x 16, M = 4, K = 4: the first 256 envs against step_skip on copies, the state bytes of all of them; the envs beyond 256 by
    properties.  (The exact check of the tile decode past one chunk, on every env: tests/test_candidate_tiles.py.)"""
    import torch
    B, N, M, K = 65536, 16, 4, 4
    rng = np.random.default_rng(3)
    env = T.look_env(N, B, "lattice", True, seed=3, timestep_limit=30)
    small = T.look_env(N, 256, "lattice", True, seed=3, timestep_limit=30)
    a0 = T.look_draw(rng, 3, B, N)
    env.rollout(torch.as_tensor(a0, device=env.device), hold=9)
    small.rollout(torch.as_tensor(a0[:, :256].copy(), device=env.device), hold=9)
    for k in H.STATE:     # envs are independent and the sampler is keyed by the env index: the small env IS the first 256
        rows = 256 * N if getattr(env, k).shape[0] == B * N else 256
        assert torch.equal(getattr(env, k)[:rows], getattr(small, k))
    actions = torch.as_tensor(T.look_draw(rng, M, B, N), device=env.device)
    ref = _reference(small, actions[:, :256].contiguous(), K)
    assert ref["done"].any()
    snap = H.snapshot(env)
    res = env.lookahead(actions, K, outputs=ALL)
    T.assert_equal({k: v[:, :256].cpu() for k, v in res.items()}, ref, "full size")
    fast = env.lookahead(actions, K, outputs=())
    T.assert_equal({k: v[:, :256].cpu() for k, v in fast.items()}, ref, "full size, fast form")
    H.bytes_equal(env, snap)
    n = res["n_steps"]
    assert bool(((n >= 1) & (n <= K)).all()) and bool((n[res["done"] == 0] == K).all())
    env.close()
    small.close()
