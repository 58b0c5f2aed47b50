"""The policy rollout with traffic (include/atc_step.h: atc_rollout_policy_traffic; AtcVecEnv.rollout_policy_traffic; atc_hip/policy.py):
atc_rollout_policy whose policy also sees each aircraft's K nearest intruders, found inside the launch at every decision.

CPU: the exports and one k_rollout_policy_traffic instantiation per (width, K); the macros, both structs and the argtypes across the header,
atc_hip/layout.py and atc_hip/lib.py; the words formula against offsets(); the refusal order through ctypes as far as it needs no sector
(traffic_k next to n_hidden); the launch record's size; pack_mlp / from_torch / input_rows with a first layer of distinct integers; the
Python method's own refusals.
GPU, TRAFFIC AND DYNAMICS, bit for bit: two envs built alike, B with traffic=K.  A calls rollout_policy_traffic once; B loops over the
decisions — observe_traffic() must equal A's stored records on the uint32 view, then rollout(clamp(A.action[b]), hold) must equal A's
rows of obs / reward / done / flags — and the states are equal at the end.  Only the new launch record moves.
GPU, POLICY: every decision restated by tests/policy_traffic_ref.py on the inputs the kernel stored, input_rows(obs0 or obs[b hold - 1],
traffic[b]), against policy_ref's bars.  Each test prints its largest deviation before it asserts.
Per-instantiation coverage — every (W, K) this call is compiled for, each against its oracle — lives in tests/test_z_policy_matrix.py."""
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
import policy_traffic_ref as PT
import traffic_ref as R
from atc_hip import layout as L
from held_tools import HEADER, LIB, struct_fields

NAMES = ("atc_rollout_policy_traffic", "atc_rollout_policy_traffic_launch_counts")
FAKE = C.c_void_p(0x100000)     # a made-up pointer: a call that is refused never follows it
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
KS = (1, 2, 4)
_records = functools.partial(H.launch_records, "rollout_policy_traffic")


# ---------------------------------------------------------------------------------------------------------------- CPU: the ABI
def test_exports_and_one_kernel_per_width_and_k():
    from atc_hip import lib
    assert set(NAMES) <= set(lib.EXPORTS)
    h = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(h, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    want = {(w, k) for w in WIDTHS for k in KS}
    assert {(int(w), int(k)) for w, k in re.findall(r"\bk_rollout_policy_traffic<(\d+), (\d+)>\(", text)} == want
    blob = open(LIB, "rb").read()       # ... and the kernels' names in the embedded code object
    for w, k in want:
        assert b"_Z24k_rollout_policy_trafficILi%dELi%dEEv" % (w, k) in blob, (w, k)
    # atc_rollout_policy's kernels are still there, one per width
    assert {int(w) for w in re.findall(r"\bk_rollout_policy<(\d+)>\(", text)} == set(WIDTHS)


def test_header_constants_structs_and_argtypes():
    from atc_hip import lib, policy
    text = open(HEADER).read()
    assert re.search(r"#define ATC_POLICY_TRAFFIC_IN\(K\) \(10 \+ 7 \* \(K\)\)", text)
    assert re.search(r"#define ATC_POLICY_TRAFFIC_WORDS\(K\) \(4422 \+ 64 \* ATC_POLICY_TRAFFIC_IN\(K\)\)", text)
    assert [L.policy_in(k) for k in (0,) + KS] == [10, 17, 24, 38] and [L.policy_words(k) for k in (0,) + KS] == [5062, 5510, 5958, 6854]
    assert all(L.policy_words(k) == 4422 + 64 * L.policy_in(k) for k in (0,) + KS) and L.policy_words() == L.POLICY_WORDS and L.policy_in() == L.POLICY_IN
    assert L.POLICY_TRAFFIC_K == KS == PT.KS
    assert L.ROLLOUT_POLICY_TRAFFIC_LAUNCH_SLOTS == int(re.search(r"ATC_ROLLOUT_POLICY_TRAFFIC_LAUNCH_SLOTS = (\d+)", text).group(1)) == 21 == 3 * len(WIDTHS)
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22     # a new entry point: the ABI number stays
    # the words formula against offsets(), for every K: each part begins where the one before it ends, the last ends at policy_words(K)
    for k in (0,) + KS:
        off = policy.offsets(k)
        assert list(off) == [n for n, _ in P.SHAPES]
        at = 0
        for name, shape in PT.shapes(k):
            assert off[name] == (at, shape), (k, name)
            at += int(np.prod(shape))
        assert at == L.policy_words(k) == PT.words(k)
        assert off["W1"][1] == (64, L.policy_in(k)) and off["b1"][0] == 64 * L.policy_in(k)
    ctype = {"const float": C.c_void_p, "float": C.c_void_p, "uint8_t": C.c_void_p, "uint16_t": C.c_void_p}
    scalar = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    pol = struct_fields(text, "atc_policy_traffic")
    assert [f[1].lstrip("*") for f in pol] == list(lib.POLICY_TRAFFIC_FIELDS) == [f[0] for f in lib.AtcPolicyTraffic._fields_]
    assert [f[1].lstrip("*") for f in pol] == [f[1].lstrip("*") for f in struct_fields(text, "atc_policy")] + ["traffic_k"]
    assert [ctype[f[0]] if f[1].startswith("*") else scalar[f[0]] for f in pol] == [f[1] for f in lib.AtcPolicyTraffic._fields_]
    assert C.sizeof(lib.AtcPolicyTraffic) == 40 and lib.AtcPolicyTraffic.seed.offset == 16 and lib.AtcPolicyTraffic.traffic_k.offset == 32
    out = struct_fields(text, "atc_policy_traffic_out")
    assert all(f[1].startswith("*") for f in out)
    assert [f[1].lstrip("*") for f in out] == list(lib.POLICY_TRAFFIC_OUT_FIELDS) == [f[0] for f in lib.AtcPolicyTrafficOut._fields_]
    assert [f[1].lstrip("*") for f in out] == [f[1].lstrip("*") for f in struct_fields(text, "atc_policy_out")] + ["traffic"]
    assert C.sizeof(lib.AtcPolicyTrafficOut) == 56
    decl = re.search(r"^int atc_rollout_policy_traffic\((.*?)\);", text, flags=re.S | re.M).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "B", "N", "T", "hold", "st", "obs0", "pol", "out", "p", "stream"]
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    ptr = {"atc_state_t": lib.AtcState, "atc_policy_traffic_t": lib.AtcPolicyTraffic, "atc_policy_traffic_out_t": lib.AtcPolicyTrafficOut,
           "atc_params_t": lib.AtcParams}
    want = [ci if a.startswith("int ") else next((C.POINTER(t) for n, t in ptr.items() if n in a), vp) for a in args]
    assert list(h.atc_rollout_policy_traffic.argtypes) == want
    assert h.atc_rollout_policy_traffic.restype is ci and h.atc_rollout_policy_traffic_launch_counts.restype is ci
    assert list(h.atc_rollout_policy_traffic_launch_counts.argtypes) == [C.POINTER(C.c_uint64), ci]
    assert callable(lib.rollout_policy_traffic_launch_counts) and "atc_rollout_policy_traffic_launch_counts" in lib.LAUNCH_RECORDS


def _call(h, T=1, hold=1, B=1, N=1, s=None, st=None, obs0=None, pol=None, out=None, p=None):
    return h.atc_rollout_policy_traffic(s, B, N, T, hold, st, obs0, pol, out, p, None)


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = _records()
    err = h.atc_last_error
    at = lambda k: 0x1000000 * (k + 1)      # noqa: E731
    pol = lib.AtcPolicyTraffic(at(1), 64, 0, 0, 0, 0, 4)
    out = lib.AtcPolicyTrafficOut(at(2), at(3), at(4), at(5), at(6), None, None)
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
    assert _call(h, **dict(ok, pol=None)) == -1 and b"null pointer: pol " in err() and b"atc_policy_traffic_t" in err()
    now = lib.AtcPolicyTraffic(None, 7, 0xff, 0, 0, 0, 3)      # (n_hidden, traffic_k and the flags wrong as well: the NULL is named first)
    assert _call(h, pol=C.byref(now)) == -1 and b"null pointer: pol->w" in err()
    assert _call(h, **dict(ok, pol=C.byref(now))) == -1 and b"null pointer: pol->w" in err()
    assert _call(h, pol=C.byref(pol)) == -1 and b"null pointer: obs0" in err()
    assert _call(h, **dict(ok, obs0=None, out=None)) == -1 and b"null pointer: obs0" in err()
    assert _call(h, **dict(ok, out=None)) == -1 and b"null pointer: out " in err()
    for k, name in enumerate(("obs", "reward", "done", "flags")):
        o = lib.AtcPolicyTrafficOut(*[None if j == k else at(2 + j) for j in range(4)], None, None, None)      # (action NULL as well)
        assert _call(h, **dict(ok, out=C.byref(o))) == -1 and b"atc_policy_traffic_out_t.obs, .reward, .done and .flags" in err(), name
    o = lib.AtcPolicyTrafficOut(at(2), at(3), at(4), at(5), None, at(6), at(8))
    bad = lib.AtcPolicyTraffic(at(1), 32, 2, 0, 0, 0, 3)
    assert _call(h, **dict(ok, out=C.byref(o), pol=C.byref(bad))) == -1 and b"atc_policy_traffic_out_t.action" in err()
    # 3. n_hidden, then traffic_k, then the flag bits — with everything later wrong as well (s NULL, B = 0)
    for nh in (0, 32, 63, 65, 128, -64):
        bad = lib.AtcPolicyTraffic(at(1), nh, 2, 0, 0, 0, 3)
        assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"n_hidden" in err()
    for k in (0, 3, 8, -1, 5, 16):
        bad = lib.AtcPolicyTraffic(at(1), 64, 2, 0, 0, 0, k)
        assert _call(h, B=0, **dict(ok, s=None, pol=C.byref(bad))) == -1 and b"traffic_k" in err(), k
    for fl in (2, 3, 0x80000000, 0xfffffffe):
        for k in KS:
            bad = lib.AtcPolicyTraffic(at(1), 64, fl, 0, 0, 0, k)
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
    buf = (C.c_uint64 * 24)(*([99] * 24))
    assert h.atc_rollout_policy_traffic_launch_counts(buf, 24) == 0
    assert all(v != 99 for v in buf[:21]) and all(v == 99 for v in buf[21:])
    assert h.atc_rollout_policy_traffic_launch_counts(None, 1) == -1
    assert isinstance(lib.rollout_policy_traffic_launch_counts(), dict)
    slots, name = lib.LAUNCH_RECORDS["atc_rollout_policy_traffic_launch_counts"]
    assert slots == 21 and [name(s) for s in range(21)] == [(w, k) for w in WIDTHS for k in KS]      # slot = 3 log2(W) + log2(K)


def test_python_surface():
    from atc_hip.vec_env import AtcVecEnv
    sig = inspect.signature(AtcVecEnv.rollout_policy_traffic)
    assert list(sig.parameters) == ["self", "weights", "T", "traffic", "hold", "seed", "decision0", "deterministic", "obs0", "out"]
    assert [sig.parameters[k].default for k in ("hold", "seed", "decision0", "deterministic", "obs0", "out")] == [1, 0, 0, False, None, None]


class _NoLibrary:
    """an env stand-in whose library handle fails the test when anything is called through it"""
    B, N, device = 3, 2, "cpu"

    class _lib:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    _lib = _lib()

    def __init__(self):
        import torch
        self.torch = torch
        self.obs = torch.zeros(3, 20)


def test_the_method_refuses_before_any_library_call():
    import torch
    from atc_hip.vec_env import AtcVecEnv
    env = _NoLibrary()
    env.device = torch.device("cpu")
    for k in (3, 8, -1, 5):
        with pytest.raises(ValueError, match="traffic"):
            AtcVecEnv.rollout_policy_traffic(env, torch.zeros(L.policy_words(4)), 4, traffic=k)
    for k in KS:      # a weight tensor of another K's size, of the 10-input policy's, one word short
        for n in (L.POLICY_WORDS, L.policy_words(k) - 1, L.policy_words(k) + 1, L.policy_words({1: 2, 2: 4, 4: 1}[k])):
            with pytest.raises(ValueError, match="weights"):
                AtcVecEnv.rollout_policy_traffic(env, torch.zeros(n), 4, traffic=k)
        with pytest.raises(ValueError, match="weights"):
            AtcVecEnv.rollout_policy_traffic(env, torch.zeros(L.policy_words(k), dtype=torch.float64), 4, traffic=k)
        with pytest.raises(ValueError, match="obs0"):
            AtcVecEnv.rollout_policy_traffic(env, torch.zeros(L.policy_words(k)), 4, traffic=k, obs0=torch.zeros(7))
        with pytest.raises(ValueError, match="traffic"):
            AtcVecEnv.rollout_policy_traffic(env, torch.zeros(L.policy_words(k)), 4, traffic=k, out={"traffic": torch.zeros(5)})


# ---------------------------------------------------------------------------------------------------------------- CPU: packing
def test_pack_mlp_from_torch_and_input_rows_lay_the_words_out():
    import torch
    from torch import nn
    from atc_hip import policy
    rng = np.random.default_rng(3)
    for K in KS:
        IN = L.policy_in(K)
        parts = [rng.normal(size=s).astype(np.float32) for _, s in PT.shapes(K)]
        parts[0] = np.arange(64 * IN, dtype=np.float32).reshape(64, IN)          # a first layer of distinct integers: word j IN + c is W1[j, c]
        w = policy.pack_mlp(*parts, traffic=K)
        assert w.dtype == torch.float32 and tuple(w.shape) == (L.policy_words(K),) and w.is_contiguous() and w.device.type == "cpu"
        assert np.array_equal(w.numpy(), PT.pack(*parts, K=K))
        assert np.array_equal(w.numpy()[:64 * IN], np.arange(64 * IN, dtype=np.float32))
        assert w[7 * IN + 3] == 7 * IN + 3 and w[63 * IN + IN - 1] == 64 * IN - 1
        off = policy.offsets(K)
        assert w[off["W2"][0] + 5 * 64 + 9] == parts[2][5, 9] and w[off["W3"][0] + 2 * 64 + 1] == parts[4][2, 1] and w[off["log_std"][0] + 2] == parts[6][2]
        for k, (name, shape) in enumerate(PT.shapes(K)):
            got = PT.split(w.numpy(), K)[name]
            assert got.shape == shape and np.array_equal(got, parts[k]), name
        net = nn.Sequential(nn.Linear(IN, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 3))
        with torch.no_grad():
            net[0].weight.copy_(torch.arange(64 * IN, dtype=torch.float32).reshape(64, IN))
        log_std = torch.tensor([-0.5, 0.25, 0.0])
        w2 = policy.from_torch(net, log_std, traffic=K)
        sp = PT.split(w2.numpy(), K)
        for j, (wn, bn) in enumerate((("W1", "b1"), ("W2", "b2"), ("W3", "b3"))):
            assert np.array_equal(sp[wn], net[2 * j].weight.detach().numpy()) and np.array_equal(sp[bn], net[2 * j].bias.detach().numpy())
        assert np.array_equal(sp["log_std"], log_std.numpy()) and np.array_equal(w2.numpy()[:64 * IN], np.arange(64 * IN, dtype=np.float32))
        # a first layer of another K's width (or the 10-input one) is refused, by both
        for other in (0,) + KS:
            if other != K:
                with pytest.raises(ValueError):
                    policy.pack_mlp(*parts, traffic=other)
                with pytest.raises(ValueError):
                    policy.from_torch(net, log_std, traffic=other)
        # input_rows: own words, then words 0..6 of each record; word 7 is left out.  Distinct integers again; tensors and arrays alike
        lead, N = (5, 3), 4
        obs = np.arange(5 * 3 * N * 10, dtype=np.float32).reshape(lead + (N * 10,))
        rec = 10000 + np.arange(5 * 3 * N * K * 8, dtype=np.float32).reshape(lead + (N, K, 8))
        x = policy.input_rows(obs, rec)
        assert x.shape == lead + (N, IN) and np.array_equal(x, PT.input_rows(obs, rec))
        assert np.array_equal(x[..., :10], obs.reshape(lead + (N, 10)))
        for r in range(K):
            assert np.array_equal(x[..., 10 + 7 * r:17 + 7 * r], rec[..., r, :7])
        assert not np.isin(rec[..., 7], x).any()
        xt = policy.input_rows(torch.from_numpy(obs), torch.from_numpy(rec))
        assert torch.is_tensor(xt) and np.array_equal(xt.numpy(), x)
        # the module's forward on such rows is the restatement's MLP (a loose bar: this is about the layout)
        net2 = nn.Sequential(nn.Linear(IN, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 3))
        w3 = policy.from_torch(net2, log_std, traffic=K)
        rows = torch.as_tensor(rng.normal(size=(50, IN)).astype(np.float32))
        assert np.allclose(net2(rows).detach().numpy(), PT.mlp(w3.numpy(), rows.numpy(), K), atol=1e-5)
    # traffic=0 is the packing as it was
    parts = [rng.normal(size=s).astype(np.float32) for _, s in P.SHAPES]
    assert np.array_equal(policy.pack_mlp(*parts).numpy(), P.pack(*parts)) and np.array_equal(policy.pack_mlp(*parts, traffic=0).numpy(), P.pack(*parts))
    assert policy.offsets() == policy.offsets(0) and [policy.offsets()[n][0] for n, _ in P.SHAPES] == [0, 640, 704, 4800, 4864, 5056, 5059]
    with pytest.raises(ValueError):
        policy.offsets(3)


def test_widen_keeps_the_ten_input_policy():
    rng = np.random.default_rng(5)
    w10 = P.random_weights(rng)
    for K in KS:
        w = PT.widen(w10, K)
        x = rng.normal(size=(20, L.policy_in(K)))
        assert np.array_equal(PT.mlp(w, x, K), P.mlp(w10, x[:, :10]))


# ---------------------------------------------------------------------------------------------------------------- GPU: the runs
SHAPES = ((3, 1), (5, 2), (7, 3), (9, 8), (40, 16), (5, 32), (3, 33), (4, 64))      # ragged B; (40, 16): three workgroups, the last one partial
CONFIGS = H.POLICY_CONFIGS
FULL = {(40, 16): 4, (4, 64): 2}                  # the five-way product runs at these (shape, K) only
RUNS = ((6, 1), (6, 3), (1, 1))                   # (T, hold)
# variant -> (weights' gain, zero head, log_std, deterministic).  "z": mu is exactly 0 and sigma exactly 1, so the stored u IS z
VARIANTS = {"z": (1.0, True, (0.0, 0.0, 0.0), False), "det1": (1.0, False, (-0.5, -1.0, 0.0), True), "det8": (8.0, False, (-0.5, -1.0, 0.0), True),
            "sampled": (1.0, False, (-0.5, -1.0, 0.25), False), "sampled8": (8.0, False, (-0.5, -1.0, 0.25), False)}
RUN_VARIANTS = {(6, 1): ("z", "det1", "det8", "sampled"), (6, 3): ("sampled", "sampled8"), (1, 1): ("sampled",)}
SEED, DECISION0 = 0x1234567890ABCDEF, 0xFFFFFFFE     # (decision0 + b wraps inside every run of more than two decisions)
OUT_KEYS = ("obs", "reward", "done", "flags")
STATE5 = ("ac", "alt", "last_act", "env", "stats")


def _grid():
    cfgs, grid, n = list(CONFIGS), [], 0
    for B, N in SHAPES:
        for K in KS:
            if FULL.get((B, N)) == K:
                grid += [(c, B, N, K) for c in cfgs]
            else:
                grid.append((cfgs[n % len(cfgs)], B, N, K))      # one configuration per (shape, K), rotating
                n += 1
    return grid


GRID = _grid()
_on_grid = pytest.mark.parametrize("cfg,B,N,K", GRID, ids=["%s-%dx%d-K%d" % g for g in GRID])


def _weights(variant, K):
    gain, zero_head, log_std, _ = VARIANTS[variant]
    return PT.random_weights(np.random.default_rng([17, int(gain), K]), K, gain, log_std, zero_head)


def _put_lattice(envs, B, N):
    """traffic_ref's clustered family — an 8 x 8 integer-nm lattice, exact d^2 ties, coincident aircraft, some WIDE headings, masks with
    0 .. N bits — written into the live state of every env of `envs` alike"""
    st = R.clustered_family(np.random.default_rng([23, B, N]), B, N, envs[0].compiled.pos_k)
    phi_fix, wide = R.phi_fields(st["P"])
    ac = np.stack([st["x_fix"], st["y_fix"], phi_fix, st["v_fix"].view(np.int32)], axis=-1).reshape(B * N, 4).astype(np.int32)
    pw = np.full((B * N, 4), 1e300)
    pw[:, 0] = np.where(wide, st["P"], 1e300).reshape(-1)
    m = st["mask"].astype(np.uint64)
    for env in envs:
        t = env.torch
        env.ac.copy_(t.from_numpy(ac))
        env.alt.copy_(t.from_numpy(np.ascontiguousarray(st["h"].reshape(-1))))
        env.phi_wide.copy_(t.from_numpy(pw))
        env.env[:, L.ENV_MASK_LO] = t.from_numpy((m & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)).to(env.device)
        env.stats[:, L.STAT_MASK_HI] = t.from_numpy((m >> np.uint64(32)).astype(np.uint32).view(np.int32)).to(env.device)
        env.synchronize()
    return st


@functools.lru_cache(maxsize=None)
def _runs(cfg_name, B, N, K, lattice=False):
    """Every run of one (mode, shape, K): {(T, hold, variant): dict(w, obs0, A outputs, per-decision mismatches against env B, both states,
    the records' gain)}, numpy.  Env B is built with traffic=K and walks the decisions: observe_traffic(), then rollout(clamp(action), hold)."""
    import torch
    from atc_hip import lib
    cfg = CONFIGS[cfg_name]
    A, Bv = H.policy_env(cfg, B, N), H.policy_env(cfg, B, N, traffic=K)
    if lattice:
        _put_lattice((A, Bv), B, N)
    for k in H.STATE + ("obs",):
        assert torch.equal(getattr(A, k), getattr(Bv, k)), k
    snap, obs0 = H.snapshot(A), A.obs.clone()
    res = {}
    for T, hold in RUNS:
        for variant in RUN_VARIANTS[(T, hold)]:
            w = _weights(variant, K)
            H.restore(A, snap)
            H.restore(Bv, snap)
            A.obs.copy_(obs0)
            before = lib.launch_records()
            out = A.rollout_policy_traffic(torch.as_tensor(w, device=A.device), T, K, hold=hold, seed=SEED, decision0=DECISION0, deterministic=VARIANTS[variant][3])
            A.synchronize()
            after = lib.launch_records()
            D = T // hold
            assert tuple(out["action"].shape) == (D, B, N, 3) and tuple(out["logp"].shape) == (D, B, N) and tuple(out["traffic"].shape) == (D, B, N, K, 8)
            assert tuple(out["obs"].shape) == (T, B, N * 10) and tuple(out["flags"].shape) == (T, B, N)
            gained = {g: {k: v - before[g].get(k, 0) for k, v in after[g].items() if v != before[g].get(k, 0)} for g in after}
            mismatch = []
            for b in range(D):
                tr = Bv.observe_traffic()
                Bv.synchronize()
                if not torch.equal(tr.contiguous().view(torch.int32), out["traffic"][b].view(torch.int32)):
                    mismatch.append(("traffic", b, int((tr.contiguous().view(torch.int32) != out["traffic"][b].view(torch.int32)).sum())))
                ref = Bv.rollout(out["action"][b:b + 1].clamp(-1.0, 1.0), hold=hold)
                Bv.synchronize()
                for k in OUT_KEYS:
                    got = out[k][b * hold:(b + 1) * hold]
                    if not np.array_equal(H.bits(got.cpu().numpy()), H.bits(ref[k].cpu().numpy())):
                        mismatch.append((k, b, int((H.bits(got.cpu().numpy()) != H.bits(ref[k].cpu().numpy())).sum())))
            res[(T, hold, variant)] = dict(
                w=w, obs0=obs0.cpu().numpy().reshape(B * N, 10), A={k: v.cpu().numpy() for k, v in out.items()}, mismatch=mismatch,
                stA={k: getattr(A, k).cpu().numpy() for k in H.STATE}, stB={k: getattr(Bv, k).cpu().numpy() for k in H.STATE},
                gained={g: v for g, v in gained.items() if v})
    A.close()
    Bv.close()
    return res


def _check_traffic_and_dynamics(runs, tag0, B, N, K, from_reset):
    events = set()
    for (T, hold, variant), r in runs.items():
        tag = tag0 + (T, hold, variant)
        assert not r["mismatch"], (tag, r["mismatch"])
        for k in STATE5:
            assert np.array_equal(H.bits(r["stA"][k]), H.bits(r["stB"][k])), (tag, k)
        for i in np.nonzero(np.isin(r["stA"]["ac"][:, L.AC_PHI], (L.I32_MIN, L.I32_MAX)))[0]:      # the exact counts of a heading still saturated
            assert r["stA"]["phi_wide"][i, 0] == r["stB"]["phi_wide"][i, 0], (tag, i)
        # only the new record moved, in slot (W, K)
        assert r["gained"] == {"atc_rollout_policy_traffic_launch_counts": {(H.lane_width(N), K): 1}}, (tag, r["gained"])
        assert np.all(np.isfinite(r["A"]["obs"])) and np.all(np.isfinite(r["A"]["reward"])) and np.all(np.isfinite(r["A"]["traffic"]))
        tr = r["A"]["traffic"]
        if from_reset:      # every slot is under control: exactly min(K, N - 1) records present per aircraft at decision 0
            assert np.array_equal((tr[0][..., 0] == 1.0).sum(-1), np.full((B, N), min(K, N - 1))), tag
        present = tr[..., 0] == 1.0
        assert np.all((tr[..., 0] == 0.0) | present) and np.all(tr[..., 7][~present] == -1.0) and np.all(tr[..., 7][present] >= 0)
        if r["A"]["done"].any():
            events.add("done")
    return events


@pytest.mark.gpu
@_on_grid
def test_traffic_and_dynamics_equal_the_loop_they_replace(cfg, B, N, K):
    events = _check_traffic_and_dynamics(_runs(cfg, B, N, K), (cfg, B, N, K), B, N, K, True)
    if CONFIGS[cfg]["auto_reset"] and CONFIGS[cfg]["timestep_limit"] == 4:
        assert "done" in events, (cfg, B, N, K)      # (T = 6 > the time limit of 4: every env auto-resets inside the launch)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,K", ((40, 16, 4), (7, 3, 2), (4, 64, 4), (5, 32, 1)))
def test_from_a_lattice_state_with_ties_and_coincident_aircraft(B, N, K):
    runs = _runs("norm-shaped-reset4", B, N, K, lattice=True)
    _check_traffic_and_dynamics(runs, ("lattice", B, N, K), B, N, K, False)
    tr = runs[(6, 1, "sampled")]["A"]["traffic"][0]
    if N >= 16:      # the family's point: coincident aircraft (distance exactly 0) are among the records
        assert np.any((tr[..., 0] == 1.0) & (tr[..., 1] == 0.0))


def _decision_inputs(r, T, hold, B, N):
    """x [T / hold, B N, 10 + 7 K]: what decision b saw — obs0 or the kernel's own stored observation of step b hold - 1, and its stored records"""
    own = H.decision_inputs(r, T, hold, B * N)
    return PT.input_rows(own.reshape(T // hold, B, N, 10), r["A"]["traffic"]).reshape(T // hold, B * N, -1)


@pytest.mark.gpu
@_on_grid
def test_z_and_logp_within_their_bars(cfg, B, N, K):
    worst_z = worst_lp = 0.0
    for (T, hold, variant), r in _runs(cfg, B, N, K).items():
        if VARIANTS[variant][3]:
            continue
        BN = B * N
        z_ref = PT.z64(SEED, *H.draw_indices(DECISION0, T, hold, BN))
        log_std = PT.split(r["w"], K)["log_std"]
        lp = r["A"]["logp"].reshape(T // hold, BN).astype(np.float64)
        worst_lp = max(worst_lp, float(np.abs(lp - PT.logp64(z_ref, log_std)).max()))
        if variant == "z":
            u = r["A"]["action"].reshape(T // hold, BN, 3).astype(np.float64)      # mu == 0 and sigma == 1 exactly: u is the kernel's z
            worst_z = max(worst_z, float(np.abs(u - z_ref).max()))
            assert np.abs(u).max() <= PT.Z_MAX
    print("%s %dx%d K=%d: max |z - z64| = %.3g (bar %.1g), max |logp - logp64| = %.3g (bar %.1g)" % (cfg, B, N, K, worst_z, PT.Z_BAR, worst_lp, PT.LOGP_BAR))
    assert worst_z <= PT.Z_BAR
    assert worst_lp <= PT.LOGP_BAR


@pytest.mark.gpu
@_on_grid
def test_mu_and_sampled_u_within_the_bar(cfg, B, N, K):
    for (T, hold, variant), r in _runs(cfg, B, N, K).items():
        if variant == "z":
            continue
        BN = B * N
        x = _decision_inputs(r, T, hold, B, N)
        bar, dev32 = PT.mu_bar(r["w"], x, K)
        mu = PT.mlp(r["w"], x, K)
        u = r["A"]["action"].reshape(T // hold, BN, 3).astype(np.float64)
        if VARIANTS[variant][3]:
            err, allowed = np.abs(u - mu), bar
            assert not r["A"]["logp"].any(), "deterministic: logp = 0"
        else:
            sigma = np.exp(PT.split(r["w"], K)["log_std"].astype(np.float64))
            err = np.abs(u - (mu + sigma * PT.z64(SEED, *H.draw_indices(DECISION0, T, hold, BN))))
            allowed = bar + sigma * PT.Z_BAR
        print("%s %dx%d K=%d T=%d hold=%d %s: float32-numpy deviation %.3g, bar %.3g, kernel deviation %.3g, max |x| %.3g"
              % (cfg, B, N, K, T, hold, variant, dev32, bar, float(err.max()), float(np.abs(x).max())))
        assert np.all(err <= allowed), (cfg, B, N, K, T, hold, variant, float(err.max()), bar)
        if variant == "det8":
            assert np.abs(u).max() > 1.0      # the saturating weights leave the action space: the clamp is at work in these runs
        if not CONFIGS[cfg]["normalize"]:
            assert np.abs(x).max() > 4.0      # raw rows (ft, kt, nm): these runs sum layer 1 in float64; normalised decision-0 rows in fp32


# ---------------------------------------------------------------------------------------------------------------- GPU: the other properties


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,K", ((40, 16, 4), (4, 64, 2)))
def test_two_launches_of_half_equal_one(B, N, K):
    import torch
    env = H.policy_one_env(B, N)
    w = torch.as_tensor(_weights("sampled", K), device=env.device)
    snap, obs0 = H.snapshot(env), env.obs.clone()

    def run(T, hold=2, **kw):
        return H.results_and_state(env, env.rollout_policy_traffic(w, T, K, hold=hold, **kw))

    one, st_one = run(8, seed=5, decision0=10)
    assert set(one) == {"obs", "reward", "done", "flags", "action", "logp", "traffic"}
    H.restore(env, snap)
    env.obs.copy_(obs0)
    two, st_two = run(8, seed=5, decision0=10)
    assert H.same_bytes(one, two) and H.same_bytes(st_one, st_two), "two runs from the same state differ"
    H.restore(env, snap)
    h1, _ = run(4, seed=5, decision0=10, obs0=obs0)
    h2, st_h = run(4, seed=5, decision0=12, obs0=h1["obs"][-1])
    for k in one:
        assert torch.equal(torch.cat([h1[k], h2[k]]).view(torch.uint8), one[k].view(torch.uint8)), k
    assert H.same_bytes(st_h, st_one)
    assert bool(one["done"].any()), "no env auto-reset inside the launch"
    # out= may carry the buffers; "traffic" None stores no records and changes nothing else
    H.restore(env, snap)
    bufs = {k: torch.full_like(v, 7) for k, v in one.items()}
    got = env.rollout_policy_traffic(w, 8, K, hold=2, seed=5, decision0=10, obs0=obs0, out=bufs)
    assert got is bufs and H.same_bytes(bufs, one)
    H.restore(env, snap)
    bufs = {k: torch.full_like(v, 7) for k, v in one.items()}
    guard = bufs.pop("traffic")
    env.rollout_policy_traffic(w, 8, K, hold=2, seed=5, decision0=10, obs0=obs0, out=dict(bufs, traffic=None))
    assert H.same_bytes(bufs, {k: one[k] for k in bufs}) and H.same_bytes(H.snapshot(env), st_one) and bool((guard == 7).all())
    # traffic=0 is rollout_policy
    w10 = torch.as_tensor(P.random_weights(np.random.default_rng(4)), device=env.device)
    H.restore(env, snap)
    a, _ = H.results_and_state(env, env.rollout_policy_traffic(w10, 4, 0, hold=2, seed=5, obs0=obs0))
    H.restore(env, snap)
    b, _ = H.results_and_state(env, env.rollout_policy(w10, 4, hold=2, seed=5, obs0=obs0))
    assert set(a) == set(b) and H.same_bytes(a, b)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,K,cfg", ((40, 16, 4, "norm-shaped-reset4"), (7, 3, 2, "raw-unshaped-noreset"), (3, 1, 1, "norm-shaped-reset4"), (4, 64, 1, "noise-area")))
def test_the_traffic_columns_are_what_the_traffic_changes(B, N, K, cfg):
    """W1's 7 K traffic columns zero and the rest a 10-input policy's: rollout_policy with that policy, within the mu bar (the summation may
    differ); only the traffic columns changed: another action for N >= 2, the same words for N = 1 (no record is ever present)"""
    import torch
    env = H.policy_one_env(B, N, cfg)
    snap, obs0 = H.snapshot(env), env.obs.clone()
    w10 = P.random_weights(np.random.default_rng([31, K]))
    dev = lambda w: torch.as_tensor(w, device=env.device)      # noqa: E731
    T, hold = 4, 2
    base = H.results_and_state(env, env.rollout_policy(dev(w10), T, hold=hold, seed=9, obs0=obs0))[0]
    H.restore(env, snap)
    zero = H.results_and_state(env, env.rollout_policy_traffic(dev(PT.widen(w10, K)), T, K, hold=hold, seed=9, obs0=obs0))[0]
    # decision 0 saw the same ten words in both; later ones may follow a trajectory that differs by the bar: compared on decision 0, and
    # on every decision whose input rows are equal
    own = [obs0.reshape(B * N, 10).cpu().numpy()] + [base["obs"][b * hold - 1].reshape(B * N, 10).cpu().numpy() for b in range(1, T // hold)]
    own_z = [own[0]] + [zero["obs"][b * hold - 1].reshape(B * N, 10).cpu().numpy() for b in range(1, T // hold)]
    worst = 0.0
    for b in range(T // hold):
        if b and not np.array_equal(own[b], own_z[b]):
            continue
        bar, _ = P.mu_bar(w10, own[b])
        du = np.abs(zero["action"][b].reshape(B * N, 3).cpu().numpy().astype(np.float64) - base["action"][b].reshape(B * N, 3).cpu().numpy().astype(np.float64))
        worst = max(worst, float(du.max()))
        assert np.all(du <= bar), (b, float(du.max()), bar)      # (the draw is the same code on the same key: only mu may differ)
        dl = np.abs(zero["logp"][b].cpu().numpy().astype(np.float64) - base["logp"][b].cpu().numpy().astype(np.float64))
        assert dl.max() <= P.LOGP_BAR
    print("%dx%d K=%d %s: zero traffic columns against rollout_policy: max |du| = %.3g" % (B, N, K, cfg, worst))
    cols = np.random.default_rng(6).normal(0.0, 1.0, (64, 7 * K)).astype(np.float32)
    H.restore(env, snap)
    full = H.results_and_state(env, env.rollout_policy_traffic(dev(PT.widen(w10, K, cols)), T, K, hold=hold, seed=9, obs0=obs0))[0]
    if N == 1:
        assert H.same_bytes(full, zero)
        assert not bool(full["traffic"][..., 0].any())
    else:
        assert not torch.equal(full["action"][0], zero["action"][0])
        assert torch.equal(full["traffic"][0].view(torch.int32), zero["traffic"][0].view(torch.int32))      # (the same state at decision 0)
    env.close()


@pytest.mark.gpu
def test_nan_weights_fly_minus_one_and_keep_the_state_finite():
    import torch
    A, Bv = H.policy_one_env(7, 5), H.policy_one_env(7, 5)
    w = torch.full((L.policy_words(2),), float("nan"), device=A.device)
    out = A.rollout_policy_traffic(w, 6, 2, hold=3, seed=3)
    assert bool(torch.isnan(out["action"]).all())
    ref = Bv.rollout(torch.full((2, 7, 5, 3), -1.0, device=Bv.device), hold=3)      # a = -1 everywhere
    for k in OUT_KEYS:
        assert torch.equal(out[k].view(torch.uint8), ref[k].view(torch.uint8)), k
    for k in STATE5:
        assert torch.equal(getattr(A, k).view(torch.uint8), getattr(Bv, k).view(torch.uint8)), k
    assert bool(torch.isfinite(out["obs"]).all()) and bool(torch.isfinite(out["reward"]).all()) and bool(torch.isfinite(A.alt).all())
    assert bool(torch.isfinite(out["traffic"]).all())
    A.close()
    Bv.close()


@pytest.mark.gpu
def test_refusals_on_the_device():
    """the refusals behind the first use of the sector: the time increment, then the mode bits, then the overlap rule — obs0 against
    out->obs, then out->traffic against obs0, out->obs and the state arrays; nothing is launched and no record moves"""
    import torch
    from atc_hip import lib
    env = H.policy_one_env(7, 5)
    h, err = lib.load(), lib.load().atc_last_error
    B, N, T, K = env.B, env.N, 4, 2
    w = torch.zeros(L.policy_words(K), device=env.device)
    buf = {"obs": torch.zeros((T + 1, B, N * 10), device=env.device), "reward": torch.zeros((T, B), device=env.device),
           "done": torch.zeros((T, B), dtype=torch.uint8, device=env.device), "flags": torch.zeros((T, B, N), dtype=torch.int16, device=env.device),
           "action": torch.zeros((T, B, N, 3), device=env.device), "logp": None, "traffic": torch.zeros((T, B, N, K, 8), device=env.device)}
    pol = lib.AtcPolicyTraffic(w.data_ptr(), 64, 0, 0, 0, 0, K)
    snap, before = H.snapshot(env), _records()

    def call(p, obs0, obs_out, traffic=None):
        ptrs = {k: (buf[k].data_ptr() if buf[k] is not None else None) for k in lib.POLICY_TRAFFIC_OUT_FIELDS}
        ptrs.update(obs=obs_out, traffic=traffic)
        o = lib.AtcPolicyTrafficOut(*[ptrs[k] for k in lib.POLICY_TRAFFIC_OUT_FIELDS])
        return h.atc_rollout_policy_traffic(env.sector.handle, B, N, T, 1, C.byref(env._state), obs0, C.byref(pol), C.byref(o), C.byref(p), None)

    base = buf["obs"].data_ptr()
    row = B * N * 40
    P_ = lambda: type(env.params).from_buffer_copy(env.params)      # noqa: E731
    p = P_()
    p.dt, p.mode = 0.0, p.mode | L.M_DISCRETE | L.M_ACTIONS_HELD
    assert call(p, base, base, base) == -1 and b"dt" in err()
    p = P_()
    p.mode |= L.M_DISCRETE | L.M_ACTIONS_HELD
    assert call(p, base, base, base) == -1 and b"ATC_M_DISCRETE" in err()
    p = P_()
    p.mode |= L.M_ACTIONS_HELD
    assert call(p, base, base, base) == -1 and b"ATC_M_ACTIONS_HELD" in err()
    p = P_()
    for off in (0, row - 4, T * row - 4, -(row - 4)):        # obs0 inside out->obs, or sharing its first / last word (named before out->traffic)
        assert call(p, base + row + off, base + row, base) == -1 and b"obs0 overlaps out->obs" in err(), off
    tbytes = T * B * N * K * 32
    assert call(p, base, base + row, base + row - 4) == -1 and b"out->traffic overlaps obs0" in err()
    assert call(p, base, base + row, base + row) == -1 and b"out->traffic overlaps out->obs" in err()
    assert call(p, base, base + row, base + (T + 1) * row - 4) == -1 and b"out->traffic overlaps out->obs" in err()
    # (the records' range is longer than a state array and the arrays are neighbours in memory: which of them is named is not pinned)
    for name, t in (("ac", env.ac), ("alt", env.alt), ("last_act", env.last_act), ("env", env.env), ("stats", env.stats), ("phi_wide", env.phi_wide)):
        for ptr in (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size() - 4, t.data_ptr() - tbytes + 4):
            assert call(p, base, base + row, ptr) == -1 and b"out->traffic overlaps st->" in err(), name
    assert _records() == before
    H.bytes_equal(env, snap)
    # ranges that only touch are accepted; a null traffic is accepted
    buf["obs"][0].copy_(env.obs)
    assert call(p, base, base + row, buf["traffic"].data_ptr()) == 0
    assert call(p, base, base + row, None) == 0
    env.synchronize()
    after, W = _records(), H.lane_width(N)
    assert after[0].get((W, K), 0) == before[0].get((W, K), 0) + 2 and after[1:] == before[1:]
    # the Python method checks what it hands over
    with pytest.raises(ValueError):
        env.rollout_policy_traffic(w, 4, 3)
    with pytest.raises(ValueError):
        env.rollout_policy_traffic(w[:-1], 4, K)
    with pytest.raises(ValueError):
        env.rollout_policy_traffic(w.cpu(), 4, K)
    with pytest.raises(RuntimeError, match="multiple of hold"):
        env.rollout_policy_traffic(w, 5, K, hold=2)
    env.close()
