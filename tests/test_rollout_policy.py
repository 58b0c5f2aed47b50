"""The policy rollout (include/atc_step.h: atc_rollout_policy; AtcVecEnv.rollout_policy; atc_hip/policy.py): T steps in one launch with
the decisions of a 10 -> 64 -> 64 -> 3 tanh MLP and a diagonal Gaussian taken inside it.

CPU: the exports and one k_rollout_policy instantiation per width; the constants, both structs and the argtypes across the header,
atc_hip/layout.py and atc_hip/lib.py; the refusal order through ctypes with NULL and made-up pointers as far as it goes without a sector
on a device (the time increment, the mode bits and the overlap rule need one: test_refusals_on_the_device); the launch record;
pack_mlp / from_torch; tests/policy_ref.py's key against a scalar loop and the moments of its z over 10^6 draws.
GPU, DYNAMICS: two envs built alike; env A calls rollout_policy, env B the existing rollout(clamp(action_A), hold) — every word of obs,
reward, done, flags and of the state equal, over the mode space, so the env half is pinned to the oracle-tested path however the policy's
roundings fall; only atc_rollout_policy_launch_counts moves.
GPU, POLICY: every decision restated by tests/policy_ref.py on the inputs the kernel stored (obs0, or obs[b hold - 1]) — decisions are
checked independently of each other — against the bars stated there.  Each test prints its largest deviation before it asserts.
Per-instantiation coverage — every (W) this call is compiled for, each against its oracle — lives in tests/test_z_policy_matrix.py."""
import ctypes as C
import functools
import inspect
import re
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import policy_ref as P
from atc_hip import layout as L
from held_tools import HEADER, LIB, struct_fields

NAMES = ("atc_rollout_policy", "atc_rollout_policy_launch_counts")
FAKE = C.c_void_p(0x100000)     # a made-up pointer: a call that is refused never follows it
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
_records = functools.partial(H.launch_records, "rollout_policy")


# ---------------------------------------------------------------------------------------------------------------- CPU: the ABI
def test_exports_and_one_kernel_per_width():
    from atc_hip import lib
    assert set(NAMES) <= set(lib.EXPORTS)
    h = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    assert {int(w) for w in re.findall(r"\bk_rollout_policy<(\d+)>\(", text)} == set(WIDTHS)
    blob = open(LIB, "rb").read()       # ... and the kernels' names in the embedded code object
    for w in WIDTHS:
        assert b"_Z16k_rollout_policyILi%dEEv" % w in blob, w


def test_header_constants_structs_and_argtypes():
    from atc_hip import lib, policy
    text = open(HEADER).read()
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, text).group(1))      # noqa: E731
    assert (L.POLICY_IN, L.POLICY_HIDDEN, L.POLICY_WORDS) == (define("ATC_POLICY_IN"), define("ATC_POLICY_HIDDEN"), define("ATC_POLICY_WORDS")) == (10, 64, 5062)
    assert L.POLICY_IN == L.OBS_DIM and L.POLICY_WORDS == 10 * 64 + 64 + 64 * 64 + 64 + 3 * 64 + 3 + 3
    assert L.POLICY_DETERMINISTIC == define("ATC_POLICY_DETERMINISTIC") == 1
    assert L.ROLLOUT_POLICY_LAUNCH_SLOTS == int(re.search(r"ATC_ROLLOUT_POLICY_LAUNCH_SLOTS = (\d+)", text).group(1)) == 7
    assert L.ABI_VERSION == 22 and define("ATC_ABI_VERSION") == 22          # a new entry point: the ABI number stays
    ctype = {"const float": C.c_void_p, "float": C.c_void_p, "uint8_t": C.c_void_p, "uint16_t": C.c_void_p}
    scalar = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    pol = struct_fields(text, "atc_policy")
    assert [f[1].lstrip("*") for f in pol] == list(lib.POLICY_FIELDS) == [f[0] for f in lib.AtcPolicy._fields_]
    assert [ctype[f[0]] if f[1].startswith("*") else scalar[f[0]] for f in pol] == [f[1] for f in lib.AtcPolicy._fields_]
    assert C.sizeof(lib.AtcPolicy) == 32 and lib.AtcPolicy.seed.offset == 16 and lib.AtcPolicy.decision0.offset == 24
    out = struct_fields(text, "atc_policy_out")
    assert all(f[1].startswith("*") for f in out)
    assert [f[1].lstrip("*") for f in out] == list(lib.POLICY_OUT_FIELDS) == [f[0] for f in lib.AtcPolicyOut._fields_]
    assert C.sizeof(lib.AtcPolicyOut) == 48
    decl = re.search(r"^int atc_rollout_policy\((.*?)\);", text, flags=re.S | re.M).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "B", "N", "T", "hold", "st", "obs0", "pol", "out", "p", "stream"]
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    ptr = {"atc_state_t": lib.AtcState, "atc_policy_t": lib.AtcPolicy, "atc_policy_out_t": lib.AtcPolicyOut, "atc_params_t": lib.AtcParams}
    want = [ci if a.startswith("int ") else next((C.POINTER(t) for n, t in ptr.items() if n in a), vp) for a in args]
    assert list(h.atc_rollout_policy.argtypes) == want
    assert h.atc_rollout_policy.restype is ci and h.atc_rollout_policy_launch_counts.restype is ci
    assert list(h.atc_rollout_policy_launch_counts.argtypes) == [C.POINTER(C.c_uint64), ci]
    assert callable(lib.rollout_policy_launch_counts) and "atc_rollout_policy_launch_counts" in lib.LAUNCH_RECORDS
    assert [(n, s) for n, s in policy.SHAPES] == [(n, s) for n, s in P.SHAPES]


def _call(h, T=1, hold=1, B=1, N=1, s=None, st=None, obs0=None, pol=None, out=None, p=None):
    return h.atc_rollout_policy(s, B, N, T, hold, st, obs0, pol, out, p, None)


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    err = h.atc_last_error
    at = lambda k: 0x1000000 * (k + 1)      # noqa: E731
    pol = lib.AtcPolicy(at(1), 64, 0, 0, 0, 0)
    out = lib.AtcPolicyOut(at(2), at(3), at(4), at(5), at(6), None)
    st, p = H.fake_state(), lib.make_params()
    ok = dict(s=FAKE, st=C.byref(st), obs0=C.c_void_p(at(7)), pol=C.byref(pol), out=C.byref(out), p=C.byref(p))
    # 1. T and hold, before any pointer is looked at
    for T, hold in ((0, 1), (-1, 1), (1, 0), (4, -2), (0, 0)):
        assert _call(h, T, hold) == -1 and b"T >= 1" in err() and b"hold >= 1" in err()
    for T, hold in ((5, 2), (1, 2), (7, 3)):
        assert _call(h, T, hold) == -1 and b"multiple of hold" in err()
        assert _call(h, T, hold, **ok) == -1 and b"multiple of hold" in err()
    # 2. the pointers, in their order: pol, pol->w, obs0, out, the four step outputs, action
    assert _call(h, 6, 3) == -1 and b"null pointer: pol " in err()
    assert _call(h, **dict(ok, pol=None)) == -1 and b"null pointer: pol " in err()
    now = lib.AtcPolicy(None, 7, 0xff, 0, 0, 0)      # (n_hidden and the flags wrong as well: the NULL is named first)
    assert _call(h, pol=C.byref(now)) == -1 and b"null pointer: pol->w" in err()
    assert _call(h, **dict(ok, pol=C.byref(now))) == -1 and b"null pointer: pol->w" in err()
    assert _call(h, pol=C.byref(pol)) == -1 and b"null pointer: obs0" in err()
    assert _call(h, **dict(ok, obs0=None, out=None)) == -1 and b"null pointer: obs0" in err()
    assert _call(h, **dict(ok, out=None)) == -1 and b"null pointer: out " in err()
    for k, name in enumerate(("obs", "reward", "done", "flags")):
        o = lib.AtcPolicyOut(*[None if j == k else at(2 + j) for j in range(4)], None, None)      # (action NULL as well)
        assert _call(h, **dict(ok, out=C.byref(o))) == -1 and b"atc_policy_out_t.obs, .reward, .done and .flags" in err(), name
    o = lib.AtcPolicyOut(at(2), at(3), at(4), at(5), None, at(6))
    bad = lib.AtcPolicy(at(1), 32, 2, 0, 0, 0)
    assert _call(h, **dict(ok, out=C.byref(o), pol=C.byref(bad))) == -1 and b"atc_policy_out_t.action" in err()
    # 3. n_hidden, then the flag bits — with everything later wrong as well (s NULL, B = 0)
    for nh in (0, 32, 63, 65, 128, -64):
        bad = lib.AtcPolicy(at(1), nh, 2, 0, 0, 0)
        assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"n_hidden" in err()
    for fl in (2, 3, 0x80000000, 0xfffffffe):
        bad = lib.AtcPolicy(at(1), 64, fl, 0, 0, 0)
        assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"pol->flags" in err()
    # 4. the argument errors of atc_rollout_hold, as far as they need no sector: s / st / p, the batch shape, a NULL state field
    dis = lib.make_params(discrete=True)
    for kw in (dict(s=None), dict(st=None), dict(p=None)):
        assert _call(h, B=0, **dict(ok, **kw)) == -1 and err().endswith(b": null pointer")
    for B, N in ((0, 1), (-1, 1), (1, 0), (1, 65)):
        assert _call(h, B=B, N=N, **dict(ok, p=C.byref(dis))) == -1 and b"B >= 1" in err()       # (before ATC_M_DISCRETE)
    hole = H.fake_state()
    hole.stats = None
    assert _call(h, **dict(ok, st=C.byref(hole), p=C.byref(dis))) == -1 and b"null field" in err()
    assert _call(h, B=1 << 21, N=64, **dict(ok, p=C.byref(dis))) == -1 and b"too large" in err()
    assert _records() == before, "a refused call moved a launch record"


def test_launch_record_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    buf = (C.c_uint64 * 9)(*([99] * 9))
    assert h.atc_rollout_policy_launch_counts(buf, 9) == 0
    assert all(v != 99 for v in buf[:7]) and all(v == 99 for v in buf[7:])
    assert h.atc_rollout_policy_launch_counts(None, 1) == -1
    assert isinstance(lib.rollout_policy_launch_counts(), dict)


def test_python_surface():
    from atc_hip.sb_adapter import AtcSBVecEnv
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc.atc_gym import AtcGym
    sig = inspect.signature(AtcVecEnv.rollout_policy)
    assert list(sig.parameters) == ["self", "weights", "T", "hold", "seed", "decision0", "deterministic", "obs0", "out"]
    assert [sig.parameters[k].default for k in ("hold", "seed", "decision0", "deterministic", "obs0", "out")] == [1, 0, 0, False, None, None]
    assert not hasattr(AtcSBVecEnv, "rollout_policy") and not hasattr(AtcGym, "rollout_policy")


# ---------------------------------------------------------------------------------------------------------------- CPU: packing
def test_pack_mlp_and_from_torch_lay_the_words_out():
    import torch
    from torch import nn
    from atc_hip import policy
    rng = np.random.default_rng(3)
    parts = [rng.normal(size=s).astype(np.float32) for _, s in P.SHAPES]
    w = policy.pack_mlp(*parts)
    assert w.dtype == torch.float32 and tuple(w.shape) == (L.POLICY_WORDS,) and w.is_contiguous() and w.device.type == "cpu"
    assert np.array_equal(w.numpy(), P.pack(*parts))
    off = policy.offsets()
    assert [off[n][0] for n, _ in P.SHAPES] == [0, 640, 704, 4800, 4864, 5056, 5059]
    # [out][in]: word W1 + j * 10 + c is the weight from input c to hidden neuron j, i.e. Linear.weight[j, c]
    assert w[7 * 10 + 3] == parts[0][7, 3] and w[704 + 5 * 64 + 9] == parts[2][5, 9] and w[4864 + 2 * 64 + 1] == parts[4][2, 1]
    for k, (name, shape) in enumerate(P.SHAPES):
        got = P.split(w.numpy())[name]
        assert got.shape == shape and np.array_equal(got, parts[k]), name
    net = nn.Sequential(nn.Linear(10, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 3))
    log_std = torch.tensor([-0.5, 0.25, 0.0])
    w2 = policy.from_torch(net, log_std)
    sp = P.split(w2.numpy())
    for j, (wn, bn) in enumerate((("W1", "b1"), ("W2", "b2"), ("W3", "b3"))):
        assert np.array_equal(sp[wn], net[2 * j].weight.detach().numpy()) and np.array_equal(sp[bn], net[2 * j].bias.detach().numpy())
    assert np.array_equal(sp["log_std"], log_std.numpy())
    # the module's forward is the restatement's MLP (float32 against float64: a loose bar, this is about the layout)
    x = torch.as_tensor(rng.normal(size=(50, 10)).astype(np.float32))
    assert np.allclose(net(x).detach().numpy(), P.mlp(w2.numpy(), x.numpy()), atol=1e-5)
    # wrong shapes are refused: a transposed matrix, a short bias, a wrong log_std, a module of another make
    for k, shape in ((0, (10, 64)), (1, (63,)), (2, (64, 65)), (4, (64, 3)), (5, (1,)), (6, (1,)), (6, (3, 1))):
        bad = list(parts)
        bad[k] = np.zeros(shape, np.float32)
        with pytest.raises(ValueError):
            policy.pack_mlp(*bad)
    for bad in (nn.Sequential(nn.Linear(10, 64), nn.ReLU(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 3)),
                nn.Sequential(nn.Linear(10, 64), nn.Tanh(), nn.Linear(64, 3)),
                nn.Sequential(nn.Linear(10, 32), nn.Tanh(), nn.Linear(32, 32), nn.Tanh(), nn.Linear(32, 3)),
                nn.Sequential(nn.Linear(10, 64), nn.Tanh(), nn.Linear(64, 64, bias=False), nn.Tanh(), nn.Linear(64, 3))):
        with pytest.raises(ValueError):
            policy.from_torch(bad, log_std)
    with pytest.raises(ValueError):
        policy.from_torch(net, torch.zeros(2))


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatement
def _mix_scalar(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_key_and_uniforms_equal_a_scalar_loop():
    rng = np.random.default_rng(8)
    for seed in (0, 1, 2 ** 63 + 12345, 2 ** 64 - 1):
        dec = np.array([0, 1, 7, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5], np.int64)        # (the last two wrap to 0 and 5)
        i = rng.integers(0, 2 ** 22, 6)
        got = P.key(seed, dec[:, None], i[None, :])
        n1, n2 = P.uniforms(seed, dec[:, None, None], i[None, :, None], np.arange(3)[None, None, :])
        for a, d in enumerate(dec):
            for b, ii in enumerate(i):
                k = _mix_scalar(_mix_scalar(seed ^ (int(d) & 0xffffffff)) ^ int(ii))
                assert int(got[a, b]) == k
                for c in range(3):
                    w = _mix_scalar(k ^ (c + 1))
                    assert int(n1[a, b, c]) == (w >> 40) + 1 and int(n2[a, b, c]) == (w >> 16) & 0xffffff
        assert np.array_equal(got[4], got[0]) and not np.array_equal(got[5], got[1])
    assert n1.min() >= 1 and n1.max() <= 2 ** 24 and n2.min() >= 0 and n2.max() < 2 ** 24


def test_z_is_a_gaussian_over_a_million_draws():
    n = 1_000_000
    z = P.z64(12345, np.arange(4)[:, None, None], np.arange(n // 12 + 1)[None, :, None], np.arange(3)[None, None, :]).reshape(-1)[:n]
    assert np.all(np.isfinite(z)) and np.abs(z).max() <= P.Z_MAX
    # sampling error of the moments of n standard normals: mean 1 / sqrt(n), variance sqrt(2 / n), kurtosis sqrt(24 / n); five sigma each
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    print("z over %d draws: mean %.5f variance %.5f kurtosis %.5f" % (n, mean, var, kurt))
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n) and abs(kurt - 3) <= 5 * np.sqrt(24 / n)
    # the three components and successive decisions are not copies of each other
    z3 = P.z64(1, np.arange(2)[:, None, None], np.arange(1000)[None, :, None], np.arange(3)[None, None, :])
    assert abs(np.corrcoef(z3[0, :, 0], z3[0, :, 1])[0, 1]) < 0.15 and abs(np.corrcoef(z3[0, :, 0], z3[1, :, 0])[0, 1]) < 0.15


# ---------------------------------------------------------------------------------------------------------------- GPU: the runs
SHAPES = ((3, 1), (7, 5), (40, 16), (4, 64))      # idle lanes at N = 5; three workgroups with a partial last one at 640 slots
CONFIGS = H.POLICY_CONFIGS
RUNS = ((6, 1), (6, 3), (1, 1))                   # (T, hold)
# variant -> (weights' gain, zero head, log_std, deterministic).  "z": mu is exactly 0 and sigma exactly 1, so the stored u IS z
VARIANTS = {"z": (1.0, True, (0.0, 0.0, 0.0), False), "det1": (1.0, False, (-0.5, -1.0, 0.0), True), "det8": (8.0, False, (-0.5, -1.0, 0.0), True),
            "sampled": (1.0, False, (-0.5, -1.0, 0.25), False)}
SEED, DECISION0 = 0x1234567890ABCDEF, 0xFFFFFFFE     # (decision0 + b wraps inside every run of more than two decisions)
OUT_KEYS = ("obs", "reward", "done", "flags")
STATE5 = ("ac", "alt", "last_act", "env", "stats")


def _weights(variant):
    gain, zero_head, log_std, _ = VARIANTS[variant]
    return P.random_weights(np.random.default_rng([17, int(gain)]), gain, log_std, zero_head)


@functools.lru_cache(maxsize=None)
def _runs(cfg_name, B, N):
    """Every run of one (mode, shape): {(T, hold, variant): dict(w, obs0, A outputs, B outputs, both states, the records' gain)}, numpy."""
    import torch
    from atc_hip import lib
    cfg = CONFIGS[cfg_name]
    A, Bv = H.policy_env(cfg, B, N), H.policy_env(cfg, B, N)
    for k in H.STATE + ("obs",):
        assert torch.equal(getattr(A, k), getattr(Bv, k)), k
    snap, obs0 = H.snapshot(A), A.obs.clone()
    res = {}
    for T, hold in RUNS:
        for variant in (("sampled",) if T == 1 else tuple(VARIANTS)):
            w = _weights(variant)
            H.restore(A, snap)
            H.restore(Bv, snap)
            A.obs.copy_(obs0)
            before = lib.launch_records()
            out = A.rollout_policy(torch.as_tensor(w, device=A.device), T, hold=hold, seed=SEED, decision0=DECISION0, deterministic=VARIANTS[variant][3])
            A.synchronize()
            after = lib.launch_records()
            assert tuple(out["action"].shape) == (T // hold, B, N, 3) and tuple(out["logp"].shape) == (T // hold, B, N)
            assert tuple(out["obs"].shape) == (T, B, N * 10) and tuple(out["flags"].shape) == (T, B, N)
            ref = Bv.rollout(out["action"].clamp(-1.0, 1.0), hold=hold)
            Bv.synchronize()
            gained = {g: {k: v - before[g].get(k, 0) for k, v in after[g].items() if v != before[g].get(k, 0)} for g in after}
            res[(T, hold, variant)] = dict(
                w=w, obs0=obs0.cpu().numpy().reshape(B * N, 10), A={k: v.cpu().numpy() for k, v in out.items()}, B={k: ref[k].cpu().numpy() for k in OUT_KEYS},
                stA={k: getattr(A, k).cpu().numpy() for k in H.STATE}, stB={k: getattr(Bv, k).cpu().numpy() for k in H.STATE},
                gained={g: v for g, v in gained.items() if v})
    A.close()
    Bv.close()
    return res


GRID = [(c, B, N) for c in CONFIGS for B, N in SHAPES]
_grid = pytest.mark.parametrize("cfg,B,N", GRID, ids=["%s-%dx%d" % g for g in GRID])


@pytest.mark.gpu
@_grid
def test_dynamics_equal_rollout_on_the_clamped_actions(cfg, B, N):
    events = set()
    for (T, hold, variant), r in _runs(cfg, B, N).items():
        tag = (cfg, B, N, T, hold, variant)
        for k in OUT_KEYS:
            assert np.array_equal(H.bits(r["A"][k]), H.bits(r["B"][k])), (tag, k, int((H.bits(r["A"][k]) != H.bits(r["B"][k])).sum()))
        for k in STATE5:
            assert np.array_equal(H.bits(r["stA"][k]), H.bits(r["stB"][k])), (tag, k)
        if CONFIGS[cfg].get("wide"):        # the side record of an aircraft whose heading field is still saturated: its exact counts
            for i in np.nonzero(np.isin(r["stA"]["ac"][:, L.AC_PHI], (L.I32_MIN, L.I32_MAX)))[0]:
                assert r["stA"]["phi_wide"][i, 0] == r["stB"]["phi_wide"][i, 0], (tag, i)
        # only the policy rollout's own record moved, in slot log2(W)
        assert r["gained"] == {"atc_rollout_policy_launch_counts": {H.lane_width(N): 1}}, (tag, r["gained"])
        assert np.all(np.isfinite(r["A"]["obs"])) and np.all(np.isfinite(r["A"]["reward"]))
        if r["A"]["done"].any():
            events.add("done")
        if T > hold and hold > 1 and r["A"]["done"].reshape(T // hold, hold, B)[:, :-1].any():
            events.add("reset inside a held block")
    if CONFIGS[cfg]["auto_reset"] and CONFIGS[cfg]["timestep_limit"] == 4:
        assert {"done", "reset inside a held block"} <= events, (cfg, B, N, events)      # (T = 6 > the time limit of 4: every env ends once)


@pytest.mark.gpu
@_grid
def test_z_and_logp_within_their_bars(cfg, B, N):
    worst_z = worst_lp = 0.0
    for (T, hold, variant), r in _runs(cfg, B, N).items():
        if VARIANTS[variant][3]:
            continue
        BN = B * N
        z_ref = P.z64(SEED, *H.draw_indices(DECISION0, T, hold, BN))
        log_std = P.split(r["w"])["log_std"]
        lp = r["A"]["logp"].reshape(T // hold, BN).astype(np.float64)
        worst_lp = max(worst_lp, float(np.abs(lp - P.logp64(z_ref, log_std)).max()))
        if variant == "z":
            u = r["A"]["action"].reshape(T // hold, BN, 3).astype(np.float64)      # mu == 0 and sigma == 1 exactly: u is the kernel's z
            worst_z = max(worst_z, float(np.abs(u - z_ref).max()))
            assert np.abs(u).max() <= P.Z_MAX
    print("%s %dx%d: max |z - z64| = %.3g (bar %.1g), max |logp - logp64| = %.3g (bar %.1g)" % (cfg, B, N, worst_z, P.Z_BAR, worst_lp, P.LOGP_BAR))
    assert worst_z <= P.Z_BAR
    assert worst_lp <= P.LOGP_BAR


@pytest.mark.gpu
@_grid
def test_mu_and_sampled_u_within_the_bar(cfg, B, N):
    for (T, hold, variant), r in _runs(cfg, B, N).items():
        if variant == "z":
            continue
        BN = B * N
        x = H.decision_inputs(r, T, hold, BN)
        bar, dev32 = P.mu_bar(r["w"], x)
        mu = P.mlp(r["w"], x)
        u = r["A"]["action"].reshape(T // hold, BN, 3).astype(np.float64)
        if VARIANTS[variant][3]:
            err, allowed = np.abs(u - mu), bar
            assert not r["A"]["logp"].any(), "deterministic: logp = 0"
        else:
            sigma = np.exp(P.split(r["w"])["log_std"].astype(np.float64))
            err = np.abs(u - (mu + sigma * P.z64(SEED, *H.draw_indices(DECISION0, T, hold, BN))))
            allowed = bar + sigma * P.Z_BAR
        print("%s %dx%d T=%d hold=%d %s: float32-numpy deviation %.3g, bar %.3g, kernel deviation %.3g, max |x| %.3g"
              % (cfg, B, N, T, hold, variant, dev32, bar, float(err.max()), float(np.abs(x).max())))
        assert np.all(err <= allowed), (cfg, B, N, T, hold, variant, float(err.max()), bar)
        if variant == "det8":
            assert np.abs(u).max() > 1.0      # the saturating weights leave the action space: the clamp is at work in these runs


# ---------------------------------------------------------------------------------------------------------------- GPU: the other properties


@pytest.mark.gpu
def test_repeatable_seeded_and_splittable():
    import torch
    env = H.policy_one_env()
    w = torch.as_tensor(_weights("sampled"), device=env.device)
    snap, obs0 = H.snapshot(env), env.obs.clone()

    def run(T, hold=2, **kw):
        return H.results_and_state(env, env.rollout_policy(w, T, hold=hold, **kw))

    one, st_one = run(8, seed=5, decision0=10)
    H.restore(env, snap)
    env.obs.copy_(obs0)
    two, st_two = run(8, seed=5, decision0=10)
    assert H.same_bytes(one, two) and H.same_bytes(st_one, st_two), "two runs from the same state differ"
    for kw in (dict(seed=6, decision0=10), dict(seed=5, decision0=11)):
        H.restore(env, snap)
        other, _ = run(8, obs0=obs0, **kw)
        assert not torch.equal(other["action"], one["action"]), kw
    # two launches of T / 2, decision0 advanced and obs0 = the first launch's last observation, are one launch of T
    H.restore(env, snap)
    h1, _ = run(4, seed=5, decision0=10, obs0=obs0)
    h2, st_h = run(4, seed=5, decision0=12, obs0=h1["obs"][-1])
    for k in one:
        assert torch.equal(torch.cat([h1[k], h2[k]]).view(torch.uint8), one[k].view(torch.uint8)), k
    assert H.same_bytes(st_h, st_one)
    # deterministic: logp = 0, no noise: another seed gives the same words
    H.restore(env, snap)
    d1, _ = run(4, seed=1, deterministic=True, obs0=obs0)
    H.restore(env, snap)
    d2, _ = run(4, seed=2, deterministic=True, obs0=obs0)
    assert H.same_bytes(d1, d2) and not d1["logp"].any()
    # obs0 defaults to the env's bound observation tensor
    H.restore(env, snap)
    env.obs.copy_(obs0)
    d3, _ = run(4, seed=1, deterministic=True)
    assert H.same_bytes(d1, d3)
    env.close()


@pytest.mark.gpu
def test_nan_weights_fly_minus_one_and_keep_the_state_finite():
    import torch
    A, Bv = H.policy_one_env(7, 5), H.policy_one_env(7, 5)
    w = torch.full((L.POLICY_WORDS,), float("nan"), device=A.device)
    out = A.rollout_policy(w, 6, hold=3, seed=3)
    assert bool(torch.isnan(out["action"]).all())
    ref = Bv.rollout(torch.full((2, 7, 5, 3), -1.0, device=Bv.device), hold=3)      # a = -1 everywhere
    for k in OUT_KEYS:
        assert torch.equal(out[k].view(torch.uint8), ref[k].view(torch.uint8)), k
    for k in STATE5:
        assert torch.equal(getattr(A, k).view(torch.uint8), getattr(Bv, k).view(torch.uint8)), k
    assert bool(torch.isfinite(out["obs"]).all()) and bool(torch.isfinite(out["reward"]).all()) and bool(torch.isfinite(A.alt).all())
    A.close()
    Bv.close()


@pytest.mark.gpu
def test_refusals_on_the_device():
    """the refusals behind the first use of the sector: the time increment (an argument error of atc_rollout_hold), then the mode bits, then
    the overlap rule — each with every later one wrong as well; nothing is launched and no record moves"""
    import torch
    from atc_hip import lib
    env = H.policy_one_env(7, 5)
    h, err = lib.load(), lib.load().atc_last_error
    B, N, T = env.B, env.N, 4
    w = torch.zeros(L.POLICY_WORDS, device=env.device)
    buf = {"obs": torch.zeros((T + 1, B, N * 10), device=env.device), "reward": torch.zeros((T, B), device=env.device),
           "done": torch.zeros((T, B), dtype=torch.uint8, device=env.device), "flags": torch.zeros((T, B, N), dtype=torch.int16, device=env.device),
           "action": torch.zeros((T, B, N, 3), device=env.device), "logp": None}
    pol = lib.AtcPolicy(w.data_ptr(), 64, 0, 0, 0, 0)
    snap, before = H.snapshot(env), _records()

    def call(p, obs0, obs_out):
        o = lib.AtcPolicyOut(obs_out, *[buf[k].data_ptr() if buf[k] is not None else None for k in lib.POLICY_OUT_FIELDS[1:]])
        return h.atc_rollout_policy(env.sector.handle, B, N, T, 1, C.byref(env._state), obs0, C.byref(pol), C.byref(o), C.byref(p), None)

    base = buf["obs"].data_ptr()
    row = B * N * 40
    P_ = lambda: type(env.params).from_buffer_copy(env.params)      # noqa: E731
    p = P_()
    p.dt, p.mode = 0.0, p.mode | L.M_DISCRETE | L.M_ACTIONS_HELD
    assert call(p, base, base) == -1 and b"dt" in err()
    p = P_()
    p.mode |= L.M_DISCRETE | L.M_ACTIONS_HELD
    assert call(p, base, base) == -1 and b"ATC_M_DISCRETE" in err()
    p = P_()
    p.mode |= L.M_ACTIONS_HELD
    assert call(p, base, base) == -1 and b"ATC_M_ACTIONS_HELD" in err()
    p = P_()
    for off in (0, row - 4, T * row - 4, -(row - 4)):        # obs0 inside out->obs, or sharing its first / last word
        assert call(p, base + row + off, base + row) == -1 and b"obs0 overlaps out->obs" in err(), off
    assert _records() == before
    H.bytes_equal(env, snap)
    # ranges that only touch are accepted: obs0 is the row in front of out->obs (how a caller chains launches in one buffer)
    buf["obs"][0].copy_(env.obs)
    assert call(p, base, base + row) == 0
    env.synchronize()
    after, W = _records(), H.lane_width(N)
    assert after[0].get(W, 0) == before[0].get(W, 0) + 1 and after[1:] == before[1:]
    # the Python method checks what it hands over
    with pytest.raises(ValueError):
        env.rollout_policy(w[:-1], 4)
    with pytest.raises(ValueError):
        env.rollout_policy(w.cpu(), 4)
    with pytest.raises(ValueError):
        env.rollout_policy(w, 4, obs0=torch.zeros(3, device=env.device))
    with pytest.raises(RuntimeError, match="multiple of hold"):
        env.rollout_policy(w, 5, hold=2)
    env.close()
