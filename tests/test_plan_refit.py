"""The refit on drawn plans (include/atc_step.h: atc_plan_refit; AtcVecEnv.refit_plans; atc_hip/cem.py: cem_plan_launch, mppi_plan): the
weighted mean and standard deviation of the M drawn candidates of one iteration, none materialised.

CPU: the exports and the kernel symbol; the constant and the argtypes across the header, atc_hip/layout.py and atc_hip/lib.py; the whole
refusal order through ctypes with NULL and made-up pointers; the bounds on M; the launch record.  tests/plan_refit_ref.py (the numpy
restatement) held to a float64 evaluation within the sequential-summation bound of its own operations, against a scalar loop, and on
NaN inputs, mean_first, junk weights, an env without participants and appended zero-weight candidates.
GPU: every word of both outputs BIT-IDENTICAL to the restatement (fp32 operations rounded once, in candidate order: no tolerance applies)
over N x B x H x M x mean_first x seven weight families, guard rows and kept rows included; in place against out of place; refusals;
the launch records; M = 1024; cem_plan_launch and mppi_plan against the same loops written with the restatement; the env state.

The grid's inputs are valid only if the REFERENCE shows a component whose new_std == 0 and one whose mean moved away from ctr."""
import ctypes as C
import functools
import inspect
import re
import shutil
import subprocess

import numpy as np
import pytest

import held_tools as T
import helpers as H
import plan_draw_ref as P
import plan_refit_ref as R
from atc_hip import layout as L
from held_tools import GUARD, HEADER, LIB

NAMES = ("atc_plan_refit", "atc_plan_refit_launch_counts")
FAKE = C.c_void_p(0x100000)     # a made-up pointer: a call that is refused never follows it
FILL = 7.5                      # what output rows hold before a call


# ---------------------------------------------------------------------------------------------------------------- CPU: the ABI
def test_exports_and_kernel_symbol():
    from atc_hip import lib
    assert set(NAMES) <= set(lib.EXPORTS)
    h = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bk_plan_refit\(", text)
    assert re.search(r"\bk_plan_draw\(", text)


def test_header_constant_and_argtypes():
    from atc_hip import lib
    text = open(HEADER).read()
    assert L.PLAN_REFIT_LAUNCH_SLOTS == int(re.search(r"ATC_PLAN_REFIT_LAUNCH_SLOTS = (\d+)", text).group(1)) == 1
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22
    decl = re.search(r"^int atc_plan_refit\((.*?)\);", text, flags=re.S | re.M).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "B", "N", "H", "M", "mean", "std", "dr", "weight", "new_mean", "new_std", "p", "stream"]
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    want = [ci if a.startswith("int ") else C.POINTER(lib.AtcPlanDraw) if "atc_plan_draw_t" in a else C.POINTER(lib.AtcParams) if "atc_params_t" in a
            else vp for a in args]
    assert list(h.atc_plan_refit.argtypes) == want
    assert h.atc_plan_refit.restype is ci and h.atc_plan_refit_launch_counts.restype is ci
    assert list(h.atc_plan_refit_launch_counts.argtypes) == [C.POINTER(C.c_uint64), ci]
    assert callable(lib.plan_refit_launch_counts)


# every launch record of the library (helpers.launch_records), the ones this module indexes first
_records = functools.partial(H.launch_records, "plan_refit")


ARGS = ("s", "mean", "std", "d", "weight", "new_mean", "new_std", "p")


def _refit_call(h):
    def call(Hn, M, B=1, N=1, **kw):
        a = dict.fromkeys(ARGS)
        a.update(kw)
        return h.atc_plan_refit(a["s"], B, N, Hn, M, a["mean"], a["std"], a["d"], a["weight"], a["new_mean"], a["new_std"], a["p"], None)
    return call


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    dr, p = lib.AtcPlanDraw(1, 2, 0), lib.make_params()
    at = lambda k: C.c_void_p(0x100000 + k * 0x100000)     # noqa: E731  (made-up ranges 1 MiB apart: no overlap at these shapes)
    ok = dict(s=FAKE, mean=at(1), std=at(2), d=C.byref(dr), weight=at(3), new_mean=at(4), new_std=at(5), p=C.byref(p))
    call, err = _refit_call(h), h.atc_last_error
    for Hn in (0, 17, -1):
        for M in (0, 1, 1025):     # H is looked at before M, both before any pointer
            assert call(Hn, M) == -1 and b"H (" in err() and b"16" in err()
    for M in (0, 1025, -1, 1 << 20):
        assert call(16, M) == -1 and b"M (" in err() and b"1024" in err()
    for M in (1, 65, 1024):        # accepted as far as the first pointer check
        assert call(1, M) == -1 and b"null pointer: s" in err()
        assert call(16, M, **dict(ok, s=None)) == -1 and b"null pointer: s" in err()
    # the pointers, in their order: with every earlier one given and every later one NULL, the first NULL is the one named
    for j, name in enumerate(ARGS):
        named = re.compile(rb"null pointer: %s\b" % (b"dr" if name == "d" else name.encode()))      # (\b: "s" is not "std")
        assert call(1, 1, **{k: ok[k] for k in ARGS[:j]}) == -1 and named.search(err()), (name, err())
        assert call(1, 1, **dict(ok, **{name: None})) == -1 and named.search(err()), (name, err())
    # ATC_M_DISCRETE before the batch shape, the batch shape before the overlap rule
    pd = lib.make_params(discrete=True)
    assert call(1, 1, N=65, **dict(ok, p=C.byref(pd))) == -1 and b"ATC_M_DISCRETE" in err()
    same = dict(ok, new_std=ok["mean"])
    assert call(1, 1, N=65, **same) == -1 and b"N <= 64" in err()
    assert call(1, 1, B=0, **same) == -1 and b"B >= 1" in err()
    assert call(1, 1, B=1 << 30, N=64, **same) == -1 and b"too large" in err()
    # the overlap rule (pointer values only): equal pointers are allowed for (mean, new_mean) and (std, new_std) alone
    rows = 2 * 3 * 5 * 12       # H = 2, B = 3, N = 5
    base = 0x100000
    ptr = lambda v: C.c_void_p(v)     # noqa: E731
    for a, b in [("mean", "std"), ("mean", "new_std"), ("std", "new_mean"), ("new_mean", "new_std"), ("mean", "weight"), ("weight", "new_std")]:
        assert call(2, 4, B=3, N=5, **dict(ok, **{b: ok[a]})) == -1 and b"overlaps" in err() and a.encode() in err() and b.encode() in err(), (a, b)
    for name, other in (("new_mean", "mean"), ("new_std", "std")):      # a partial overlap of the pair that may be equal
        for off in (4, rows - 4, -4, -(rows - 4)):
            assert call(2, 4, B=3, N=5, **dict(ok, **{name: ptr(ok[other].value + off)})) == -1 and b"overlaps" in err(), (name, off)
    # weight's range is M B 4 bytes (ranges that only touch are accepted: test_python_arguments_refusals_and_the_largest_m, on a device)
    w_bytes = 4 * 3 * 4
    assert call(2, 4, B=3, N=5, **dict(ok, weight=ptr(base), mean=ptr(base + w_bytes - 4))) == -1 and b"overlaps" in err()
    assert call(2, 4, B=3, N=5, **dict(ok, mean=ptr(base), weight=ptr(base + rows - 4))) == -1 and b"overlaps" in err()
    assert _records() == before, "a refused call moved a launch record"


def test_launch_record_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    buf = (C.c_uint64 * 8)(*([99] * 8))
    assert h.atc_plan_refit_launch_counts(buf, 8) == 0
    assert buf[0] != 99 and all(v == 99 for v in buf[1:])
    assert h.atc_plan_refit_launch_counts(None, 1) == -1
    assert isinstance(lib.plan_refit_launch_counts(), dict)


def test_python_surface():
    from atc_hip import cem, sb_adapter
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import atc_gym
    sig = inspect.signature(AtcVecEnv.refit_plans)
    assert list(sig.parameters) == ["self", "mean", "std", "M", "weight", "seed", "iteration", "mean_first", "out", "std_min"]
    assert [sig.parameters[k].default for k in ("seed", "iteration", "mean_first", "out", "std_min")] == [0, 0, True, None, 0.0]
    sig = inspect.signature(cem.mppi_plan)
    assert list(sig.parameters) == ["env", "mean", "std", "K", "M", "iters", "temperature", "gamma", "seed", "std_min"]
    assert [sig.parameters[k].default for k in ("gamma", "seed", "std_min")] == [1.0, 0, 0.0]
    assert list(inspect.signature(cem.cem_plan_launch).parameters) == list(inspect.signature(cem.cem_plan).parameters)
    for cls in (sb_adapter.AtcSBVecEnv, atc_gym.AtcGym):       # deliberately out of scope
        assert not hasattr(cls, "refit_plans")


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatement
def _weights(kind, rng, M, B, E=16, temperature=1.0):
    if kind == "elites":
        w = np.zeros((M, B), np.float32)
        for e in range(B):
            w[rng.choice(M, min(E, M), replace=False), e] = 1.0
        return w
    score = rng.normal(0.0, 2.0, (M, B))
    return np.exp((score - score.max(0)) / temperature).astype(np.float32)


@pytest.mark.parametrize("std", [0.3, 1e-2, 1e-4])
@pytest.mark.parametrize("kind", ["elites", "softmax"])
def test_restatement_within_the_summation_bound_of_float64(std, kind):
    """M = 256: the float32 loop against the float64 moments of the same draws.  The bar is plan_refit_ref.bounds — the sequential
    summation bound gamma(n) = n u / (1 - n u), u = 2^-24, over the roundings each accumulator's terms carry, on sum |w d| / W — and
    never a measured number.  The unshifted E[a^2] - E[a]^2 in float32 is shown to miss it at std = 1e-4: the reason for the shift."""
    M, Hn, B, N = 256, 2, 6, 3
    rng = np.random.default_rng(int(std * 1e5) + len(kind))
    mean = rng.uniform(-0.6, 0.6, (Hn, B, N, 3)).astype(np.float32)
    w = _weights(kind, rng, M, B)
    key = dict(seed=41, iteration=3, mean_first=True)
    got_m, got_s = R.refit(mean, std, M, w, **key)
    r64 = R.refit64(mean, std, M, w, **key)
    e_m, e_s = R.bounds(M, r64)
    err_m, err_s = np.abs(got_m - r64["mean"]), np.abs(got_s - r64["std"])
    print("std %g %s: mean error max %.3g (bound %.3g), std relative error max %.3g (bound %.3g)" % (
        std, kind, err_m.max(), e_m.max(), (err_s / r64["std"]).max(), (e_s / r64["std"]).max()))
    assert (r64["std"] > 0.2 * std).all() and (err_m <= e_m).all() and (err_s <= e_s).all()
    assert e_m.max() < 0.05 * std and (e_s / r64["std"]).max() < 0.05      # (the bar is a small fraction of the spread it is about)
    if kind == "elites":
        # the parent's recipe — the elites' rows, then mean and std — in float64: the same two numbers
        idx = np.stack([np.nonzero(w[:, e])[0] for e in range(B)], 1)
        rows = P.draw(mean, std, M, index=idx, **key).astype(np.float64)
        assert (np.abs(got_m - rows.mean(0)) <= e_m).all() and (np.abs(got_s - rows.std(0)) <= e_s).all()
    if std == 1e-4:
        a = P.draw(mean, std, M, **key)
        wb = w[:, None, :, None, None]
        Wt = wb.sum(0, dtype=np.float32)
        naive = np.sqrt(np.fmax((wb * a * a).sum(0, dtype=np.float32) / Wt - ((wb * a).sum(0, dtype=np.float32) / Wt) ** 2, 0))
        assert (np.abs(naive - r64["std"]) > e_s).mean() > 0.5


def _scalar_loop(mean, std, M, w, key, h, e, k, c, B, N):
    """one output word by a plain loop on numpy float32 scalars: the header's pseudocode, line for line"""
    f = np.float32
    ctr = f(min(max(mean[h, e, k, c], f(-1)), f(1))) if not np.isnan(mean[h, e, k, c]) else f(-1)
    W = s1 = s2 = f(0)
    for m in range(M):
        wt = w[m, e]
        if not (wt > 0 and wt <= R.FLT_MAX):
            continue
        if key["mean_first"] and m == 0:
            a = ctr
        else:
            a = P.clamp(mean[h, e, k, c] + std[h, e, k, c] * P.draw_z(key["seed"], key["iteration"], m, h, e * N + k, c))
        d = f(a - ctr)
        t = f(wt * d)
        s1, s2, W = f(s1 + t), f(s2 + f(t * d)), f(W + wt)
    q = f(s1 / W)
    return f(ctr + q), f(np.sqrt(max(f(f(s2 / W) - f(q * q)), f(0))))


def test_restatement_equals_a_scalar_loop_and_handles_junk_weights():
    M, Hn, B, N = 12, 2, 4, 3
    rng = np.random.default_rng(8)
    mean = rng.uniform(-1.2, 1.2, (Hn, B, N, 3)).astype(np.float32)
    std = rng.uniform(0.0, 0.5, (Hn, B, N, 3)).astype(np.float32)
    w = rng.uniform(0.1, 2.0, (M, B)).astype(np.float32)
    # zeros, negatives, NaN, +Inf, -Inf and a subnormal: only the subnormal participates
    w[1, 0], w[2, 0], w[3, 0], w[4, 0], w[5, 0], w[6, 0] = 0.0, -1.0, np.nan, np.inf, 1e-40, -np.inf
    w[:, 2] = [0.0, -0.0, -3.0, np.nan, np.inf, -np.inf] * 2          # env 2: no participant
    w[:, 3] = 0.0
    w[7, 3] = 2.0                                                      # env 3: one participant (a power of two: w d / w is d exactly)
    part = R.participates(w)
    assert part[5, 0] and not part[1:5, 0].any() and not part[6, 0] and not part[:, 2].any() and part[:, 3].sum() == 1
    for mean_first in (True, False):
        key = dict(seed=77, iteration=1, mean_first=mean_first)
        into = (np.full(mean.shape, FILL, np.float32), np.full(mean.shape, -FILL, np.float32))
        got_m, got_s = R.refit(mean, std, M, w, into=into, **key)
        assert got_m.dtype == got_s.dtype == np.float32 and got_m.shape == mean.shape
        assert (got_m[:, 2] == FILL).all() and (got_s[:, 2] == -FILL).all()
        keep_m, keep_s = R.refit(mean, std, M, w, **key)
        assert np.array_equal(keep_m[:, 2], mean[:, 2]) and np.array_equal(keep_s[:, 2], std[:, 2])      # without `into`: the inputs
        for e in (0, 1, 3):
            for h, k, c in ((0, 0, 0), (1, 2, 1), (1, 1, 2)):
                want = _scalar_loop(mean, std, M, w, key, h, e, k, c, B, N)
                assert (got_m[h, e, k, c].view(np.uint32), got_s[h, e, k, c].view(np.uint32)) == (want[0].view(np.uint32), want[1].view(np.uint32)), (e, h, k, c)
        # one participant: its action exactly, and a standard deviation of exactly 0
        one = P.draw(mean, std, M, **key)[7][:, 3]
        assert np.array_equal(got_m[:, 3], (P.clamp(mean)[:, 3] + (one - P.clamp(mean)[:, 3]))) and not got_s[:, 3].any()
        # appended zero-weight (or junk-weight) candidates change nothing
        for tail in (np.zeros((5, B), np.float32), np.full((3, B), np.nan, np.float32), np.full((1, B), -2.0, np.float32)):
            more = R.refit(mean, std, M + len(tail), np.concatenate([w, tail]), into=into, **key)
            assert np.array_equal(more[0].view(np.uint32), got_m.view(np.uint32)) and np.array_equal(more[1].view(np.uint32), got_s.view(np.uint32))


def test_restatement_mean_first_and_nan_inputs():
    M, Hn, B, N = 6, 2, 3, 2
    rng = np.random.default_rng(9)
    mean = rng.uniform(-1.4, 1.4, (Hn, B, N, 3)).astype(np.float32)
    std = np.full(mean.shape, 0.3, np.float32)
    only0 = np.zeros((M, B), np.float32)
    only0[0] = 2.0                                                                 # (a power of two: w d / w is d exactly)
    m1, s1 = R.refit(mean, std, M, only0, seed=3, mean_first=True)
    assert np.array_equal(m1, P.clamp(mean)) and not s1.any()                      # candidate 0 is the clamped mean
    m0, s0 = R.refit(mean, std, M, only0, seed=3, mean_first=False)
    a0 = P.draw(mean, std, 1, seed=3, mean_first=False)[0]
    assert np.array_equal(m0, P.clamp(mean) + (a0 - P.clamp(mean))) and np.abs(m0 - a0).max() < 1e-7 and not s0.any() and not np.array_equal(m0, m1)
    w = np.ones((M, B), np.float32)
    a, b = R.refit(mean, std, M, w, seed=3, mean_first=True), R.refit(mean, std, M, w, seed=3, mean_first=False)
    assert not np.array_equal(a[0], b[0])
    # a NaN mean: every draw and ctr are -1; a NaN std: every DRAWN candidate is -1 (candidate 0 stays the mean under mean_first)
    bad_m, bad_s = mean.copy(), std.copy()
    bad_m[1, 2, 0, 1] = np.nan
    bad_s[0, 1, 1, 2], bad_m[0, 1, 1, 2] = np.nan, 0.25
    for mean_first in (True, False):
        gm, gs = R.refit(bad_m, bad_s, M, w, seed=3, mean_first=mean_first)
        assert np.isfinite(gm).all() and np.isfinite(gs).all()
        assert gm[1, 2, 0, 1] == -1.0 and gs[1, 2, 0, 1] == 0.0
        if not mean_first:
            assert abs(gm[0, 1, 1, 2] + 1.0) < 1e-6 and gs[0, 1, 1, 2] < 1e-3
        else:
            assert gm[0, 1, 1, 2] > -1.0 and gs[0, 1, 1, 2] > 0.0


# ---------------------------------------------------------------------------------------------------------------- the grid's inputs
GRID_B, GRID_H, GRID_M = (5, 70), (1, 4), (1, 8, 65)
FAMILIES = ("elites1", "elites3", "softmax", "equal", "hole", "last", "junk")


def _grid_inputs(N, B, Hn):
    """mean, std [H, B, N, 3] (device-independent): means beyond +-1, std = 0, components that clamp in every draw (|mean| = 1.5, std
    0.01: new_std == 0 whatever the weights), and a NaN in each"""
    rng = np.random.default_rng(1000 * N + 10 * B + Hn)
    mean = rng.uniform(-1.3, 1.3, (Hn, B, N, 3)).astype(np.float32)
    std = rng.uniform(0.0, 0.4, (Hn, B, N, 3)).astype(np.float32)
    std[rng.uniform(size=std.shape) < 0.1] = 0.0
    pin = rng.uniform(size=std.shape) < 0.1
    mean[pin] = np.where(rng.uniform(size=int(pin.sum())) < 0.5, 1.5, -1.5)
    std[pin] = 0.01
    mean[0, 1, 0, 0], std[0, 2, 0, 1] = np.nan, np.nan
    std[0, 0, 0, 2] = 0.0              # (env 0 has a participant in every family)
    return mean, std


def _grid_weights(family, N, B, M, rng):
    """[M, B] float32.  hole: every third env has no participant (with N <= 32 every wavefront holds such an env next to others; N = 33
    puts one across a wavefront boundary; N = 64 makes it a wavefront of its own).  last: candidate M - 1 alone.  junk: softmax with
    zeros, negatives, NaN, +-Inf and subnormals written over a third of it."""
    if family.startswith("elites"):
        return _weights("elites", rng, M, B, E=int(family[6:]))
    if family == "softmax":
        return _weights("softmax", rng, M, B, temperature=0.7)
    if family == "equal":
        return np.full((M, B), 0.25, np.float32)
    if family == "hole":
        w = _weights("elites", rng, M, B, E=2)
        w[:, 1::3] = 0.0
        return w
    if family == "last":
        w = np.zeros((M, B), np.float32)
        w[M - 1] = 3.0
        return w
    w = _weights("softmax", rng, M, B)
    junk = np.array([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf, 1e-40, 1e-44], np.float32)
    hit = rng.uniform(size=w.shape) < 0.35
    w[hit] = junk[rng.integers(0, len(junk), int(hit.sum()))]
    return w


def _grid_cases(N, B):
    for Hn in GRID_H:
        mean, std = _grid_inputs(N, B, Hn)
        for M in GRID_M:
            for mean_first in (True, False):
                key = dict(seed=500 + N, iteration=B + M, mean_first=mean_first)
                draws = P.draw(mean, std, M, **key)
                rng = np.random.default_rng(N + 7 * B + 13 * Hn + 17 * M)
                for family in FAMILIES:
                    yield Hn, M, key, family, mean, std, _grid_weights(family, N, B, M, rng), draws


def _events(mean, want_m, want_s, w):
    """(a written component with new_std == 0, a written component whose mean moved away from ctr)"""
    some = np.broadcast_to(R.participates(w).any(0)[None, :, None, None], mean.shape)
    return bool(((want_s == 0) & some).any()), bool(((want_m != P.clamp(mean)) & some).any())


@pytest.mark.parametrize("N", [1, 3])
def test_grid_inputs_show_their_events_on_the_restatement(N):
    """A condition on the INPUTS of the GPU grid, checked without a GPU: for every (B, H, M > 1, mean_first) the restatement shows a
    written component with new_std == 0 and one whose mean moved away from ctr; a hole family leaves envs unwritten."""
    for B in GRID_B:
        for Hn, M, key, family, mean, std, w, draws in _grid_cases(N, B):
            want_m, want_s = R.refit(mean, std, M, w, draws=draws, **key)
            zero, moved = _events(mean, want_m, want_s, w)
            if M > 1:
                assert zero and moved, (B, Hn, M, key, family)
            if family == "hole" and B > 1:
                assert not R.participates(w)[:, 1::3].any() and R.participates(w)[:, 0::3].any()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _guarded_refit(env, tm, ts, M, w, key, Hn):
    """atc_plan_refit through ctypes into FILL-ed outputs with GUARD rows of [B N 3] in front and behind"""
    import torch
    from atc_hip import lib
    B, N = env.B, env.N
    bufs = [torch.full((Hn + 2 * GUARD, B, N, 3), v, dtype=torch.float32, device=env.device) for v in (FILL, -FILL)]
    dr = lib.AtcPlanDraw(key["seed"], key["iteration"], L.DRAW_MEAN_FIRST if key["mean_first"] else 0)
    lib.check(lib.load().atc_plan_refit(env.sector.handle, B, N, Hn, M, tm.data_ptr(), ts.data_ptr(), C.byref(dr), w.data_ptr(),
                                        bufs[0][GUARD:].data_ptr(), bufs[1][GUARD:].data_ptr(), C.byref(env.params),
                                        torch.cuda.current_stream().cuda_stream))
    env.synchronize()
    for t, v in zip(bufs, (FILL, -FILL)):
        g = torch.cat([t[:GUARD], t[GUARD + Hn:]])
        assert bool((g == v).all()), "guard rows overwritten"
    return bufs[0][GUARD:GUARD + Hn].cpu().numpy(), bufs[1][GUARD:GUARD + Hn].cpu().numpy()


def _same(got, want, tag):
    for name, g, x in zip(("new_mean", "new_std"), got, want):
        g, x = np.asarray(g).reshape(x.shape), np.asarray(x)
        bad = np.nonzero(g.view(np.uint32) != x.view(np.uint32))
        assert not len(bad[0]), "%s %r: %d words differ, first at %r: got %r want %r" % (
            name, tag, len(bad[0]), tuple(int(b[0]) for b in bad), g[bad][0], x[bad][0])


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N", [1, 3, 16, 33, 64])
def test_refit_equals_the_restatement(N):
    import torch
    seen_zero = seen_moved = seen_kept = False
    for B in GRID_B:
        env = T.look_env(N, B)
        snap = H.snapshot(env)
        into = (np.full((1, B, N, 3), FILL, np.float32), np.full((1, B, N, 3), -FILL, np.float32))
        for Hn, M, key, family, mean, std, w, draws in _grid_cases(N, B):
            tm, ts, tw = (torch.as_tensor(x, device=env.device) for x in (mean, std, w))
            keep = tuple(np.broadcast_to(x, mean.shape) for x in into)
            want = R.refit(mean, std, M, w, into=keep, draws=draws, **key)
            zero, moved = _events(mean, want[0], want[1], w)
            seen_zero, seen_moved = seen_zero or zero, seen_moved or moved
            seen_kept = seen_kept or bool((want[0] == FILL).any())
            before = _records()
            got = _guarded_refit(env, tm, ts, M, tw, key, Hn)
            _same(got, want, (B, Hn, M, key["mean_first"], family))
            now = _records()
            assert now[0] == {"refit": before[0].get("refit", 0) + 1} and now[1:] == before[1:], "only the refit's launch record moves"
            if family in ("softmax", "hole"):      # the Python surface: out of place (kept rows = the inputs), then in place, byte-equal
                py = env.refit_plans(tm.view(Hn, B, N * 3), ts, M, tw, **key)
                assert py[0].shape == py[1].shape == (Hn, B, N, 3) and py[0].data_ptr() != tm.data_ptr()
                _same([t.cpu().numpy() for t in py], R.refit(mean, std, M, w, draws=draws, **key), ("python", B, Hn, M, family))
                im, isd = tm.clone(), ts.clone()
                back = env.refit_plans(im, isd, M, tw, out=(im, isd), **key)
                assert back[0].data_ptr() == im.data_ptr() and back[1].data_ptr() == isd.data_ptr()
                assert torch.equal(im.view(torch.int32), py[0].view(torch.int32)) and torch.equal(isd.view(torch.int32), py[1].view(torch.int32))
                assert torch.equal(tm.view(torch.int32), torch.as_tensor(mean).view(torch.int32).to(tm.device)), "the inputs are read only"
        H.bytes_equal(env, snap)
        env.close()
    assert seen_zero, "no written component with new_std == 0 in this grid"
    assert seen_moved, "no written component whose mean moved away from ctr in this grid"
    assert seen_kept, "no env without a participant in this grid"


@pytest.mark.gpu
@pytest.mark.timeout(60)
def test_python_arguments_refusals_and_the_largest_m():
    import torch
    from atc_hip import lib
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import model
    B, N, Hn, M = 5, 3, 2, 1024
    env = T.look_env(N, B)
    rng = np.random.default_rng(1024)
    mean = rng.uniform(-1.1, 1.1, (Hn, B, N, 3)).astype(np.float32)
    std = rng.uniform(0.0, 0.5, (Hn, B, N, 3)).astype(np.float32)
    w = _weights("softmax", rng, M, B)
    w[:, 4] = 0.0
    w[1023, 4] = 1.0
    tm, ts = torch.as_tensor(mean, device=env.device), torch.as_tensor(std, device=env.device)
    key = dict(seed=8, iteration=2, mean_first=True)
    got = env.refit_plans(tm, ts, M, w.astype(np.float64), **key)                      # (a float64 numpy weight: converted)
    _same([t.cpu().numpy() for t in got], R.refit(mean, std, M, w, **key), "M = 1024")
    # std_min, a python-float std, out= given
    lo = env.refit_plans(tm, 0.2, M, torch.as_tensor(w), std_min=0.05, **key)
    want = R.refit(mean, 0.2, M, w, **key)
    _same((lo[0].cpu().numpy(), lo[1].cpu().numpy()), (want[0], np.maximum(want[1], np.float32(0.05))), "std_min")
    assert float(lo[1].min()) == np.float32(0.05)
    for bad in (dict(M=0), dict(M=1025), dict(weight=w[:8]), dict(weight=w.T), dict(out=(tm,)), dict(out=(tm, ts[:1])),
                dict(out=(tm.cpu(), ts.cpu())), dict(out=(tm.double(), ts.double()))):
        args = dict(dict(M=M, weight=w), **bad)
        with pytest.raises(ValueError):
            env.refit_plans(tm, ts, args.pop("M"), args.pop("weight"), **args)
    with pytest.raises(ValueError):
        env.refit_plans(tm.repeat(9, 1, 1, 1)[:17], 0.3, 8, w[:8])
    # the partial overlap, refused by the library: new_mean one aircraft into mean
    before = _records()
    big = torch.zeros(Hn * B * N * 3 + 3, device=env.device)
    big[:Hn * B * N * 3] = tm.flatten()
    with pytest.raises(RuntimeError, match="overlaps"):
        env.refit_plans(big[:-3].view(Hn, B, N, 3), ts, 8, w[:8], out=(big[3:], torch.empty_like(ts)))
    with pytest.raises(RuntimeError, match="overlaps"):
        env.refit_plans(tm, ts, 8, w[:8], out=(ts, tm))
    assert _records() == before
    # ranges that only touch are accepted: new_std right behind new_mean
    n = Hn * B * N * 3
    buf = torch.empty(2 * n, device=env.device)
    touch = env.refit_plans(tm, ts, M, w, out=(buf[:n], buf[n:]), **key)
    assert touch[0].data_ptr() == buf.data_ptr() and torch.equal(touch[0], got[0]) and torch.equal(touch[1], got[1])
    env.close()
    # a discrete env: the method's ValueError and the library's refusal
    denv = AtcVecEnv(4, 2, sim_parameters=model.SimParameters(1, discrete_action_space=True), scenario=T.look_scenario(), grid_cell=0.5)
    denv.reset()
    dm = torch.zeros((2, 4, 2, 3), device=denv.device)
    dw = torch.ones((4, 4), device=denv.device)
    before = _records()
    with pytest.raises(ValueError):
        denv.refit_plans(dm, 0.3, 4, dw)
    dr, dsd, o1, o2 = lib.AtcPlanDraw(0, 0, 0), torch.full_like(dm, 0.3), torch.empty_like(dm), torch.empty_like(dm)
    h = lib.load()
    assert h.atc_plan_refit(denv.sector.handle, 4, 2, 2, 4, dm.data_ptr(), dsd.data_ptr(), C.byref(dr), dw.data_ptr(), o1.data_ptr(), o2.data_ptr(),
                            C.byref(denv.params), None) == -1 and b"ATC_M_DISCRETE" in h.atc_last_error()
    assert _records() == before
    denv.close()


def _planner_env(rng):
    env = T.look_env(16, 37)
    T.look_fly(env, rng)
    return env


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_cem_plan_launch_equals_the_loop_on_the_restatement():
    """Three CEM iterations against the same loop written with draw_plans' rows and plan_refit_ref: refit and decision, bit for bit;
    the refit agrees with cem_plan's (torch on the materialised elites) to rounding"""
    import torch
    from atc_hip import cem
    B, N, K, Hn, M, E, gamma = 37, 16, 3, 3, 16, 4, 0.9
    rng = np.random.default_rng(31)
    env = _planner_env(rng)
    mean0 = torch.as_tensor(rng.uniform(-0.5, 0.5, (Hn, B, N, 3)).astype(np.float32), device=env.device)
    snap = H.snapshot(env)
    with pytest.raises(ValueError):
        cem.cem_plan_launch(env, mean0, 0.4, K, M, 0, E)
    with pytest.raises(ValueError):
        cem.cem_plan_launch(env, mean0, 0.4, K, M, 1, M + 1)
    got = cem.cem_plan_launch(env, mean0, 0.4, K, M, 3, E, gamma=gamma, seed=12)
    H.bytes_equal(env, snap)
    mean, std = mean0.cpu().numpy(), np.full(mean0.shape, 0.4, np.float32)
    disc = torch.tensor([gamma ** h for h in range(Hn)], dtype=torch.float32, device=env.device)
    for t in range(3):
        tm, ts = torch.as_tensor(mean, device=env.device), torch.as_tensor(std, device=env.device)
        plans = env.draw_plans(tm, ts, M, seed=12, iteration=t)
        seg = env.lookahead_plan(plans, K, outputs=("seg_reward",))["seg_reward"]
        idx = (seg * disc[None, :, None]).sum(1).topk(E, dim=0).indices.cpu().numpy()
        w = np.zeros((M, B), np.float32)
        np.put_along_axis(w, idx, 1.0, 0)
        assert (w.sum(0) == E).all()
        rows = plans.cpu().numpy()
        best = rows[idx[0], 0, np.arange(B)]
        mean, std = R.refit(mean, std, M, w, seed=12, iteration=t, draws=rows)
    _same((got[0].cpu().numpy(), got[1].cpu().numpy()), (mean, std), "cem_plan_launch")
    assert got[2].shape == (B, N, 3) and np.array_equal(got[2].cpu().numpy().view(np.uint32), best.view(np.uint32))
    ref = cem.cem_plan(env, mean0, 0.4, K, M, 1, E, gamma=gamma, seed=12)
    one = cem.cem_plan_launch(env, mean0, 0.4, K, M, 1, E, gamma=gamma, seed=12)
    assert torch.equal(ref[2], one[2]) and float((ref[0] - one[0]).abs().max()) < 1e-6 and float((ref[1] - one[1]).abs().max()) < 1e-5
    H.bytes_equal(env, snap)
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_mppi_plan_equals_the_loop_on_the_restatement():
    """Two MPPI iterations against the loop written with lookahead_plan_sampled, the same torch weights and plan_refit_ref"""
    import torch
    from atc_hip import cem
    B, N, K, Hn, M, temp, gamma, floor = 37, 16, 3, 3, 24, 5.0, 0.9, 0.02
    rng = np.random.default_rng(32)
    env = _planner_env(rng)
    mean0 = torch.as_tensor(rng.uniform(-0.5, 0.5, (Hn, B, N, 3)).astype(np.float32), device=env.device)
    snap = H.snapshot(env)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(iters=0)):
        with pytest.raises(ValueError):
            cem.mppi_plan(env, mean0, 0.4, K, M, **dict(dict(iters=1, temperature=temp), **bad))
    got = cem.mppi_plan(env, mean0, 0.4, K, M, 2, temp, gamma=gamma, seed=5, std_min=floor)
    H.bytes_equal(env, snap)
    mean, std = mean0.cpu().numpy(), np.full(mean0.shape, 0.4, np.float32)
    disc = torch.tensor([gamma ** h for h in range(Hn)], dtype=torch.float32, device=env.device)
    spread = []
    for t in range(2):
        tm, ts = torch.as_tensor(mean, device=env.device), torch.as_tensor(std, device=env.device)
        res = env.lookahead_plan_sampled(tm, ts, K, M, seed=5, iteration=t, outputs=("seg_reward",))
        score = (res["seg_reward"] * disc[None, :, None]).sum(1)
        w = torch.exp((score - score.max(0).values) / temp)
        w = torch.where(res["n_steps"] == 0, torch.zeros_like(w), w).cpu().numpy()
        spread.append(int((w > 0).sum(0).max()))
        winner = score.argmax(0).cpu().numpy()
        best = P.draw(mean, std, M, seed=5, iteration=t)[winner, 0, np.arange(B)]
        mean, std = R.refit(mean, std, M, w, seed=5, iteration=t)
        std = np.maximum(std, np.float32(floor))
    assert min(spread) > 1, "in every env the softmax weight sits on one candidate"
    _same((got[0].cpu().numpy(), got[1].cpu().numpy()), (mean, std), "mppi_plan")
    assert got[2].shape == (B, N, 3) and np.array_equal(got[2].cpu().numpy().view(np.uint32), best.view(np.uint32))
    H.bytes_equal(env, snap)
    env.close()
