"""The stand-alone policy forward without a GPU (include/atc_step.h: atc_policy_forward; AtcVecEnv.policy_forward / act; atc_hip.policy and
atc_hip.value: unpack, to_torch; atc_hip.checkpoint; atc_hip.agent): the way back from the packed arrays to torch and to a file, bit for bit;
tests/policy_forward_ref.py's keys against policy_ref.key on a rollout's [D, B, N] numbering; the constants, structs and argtypes across the
header, atc_hip/layout.py and atc_hip/lib.py; every ATC_ERR_ARG refusal through ctypes in the header's order, with made-up pointers; the launch
record; the Python surface and its refusals before any library call."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import helpers as H  # noqa: F401  (sys.path)
import policy_forward_ref as PF
import policy_ref as P
import ppo_value_ref as PV
from atc_hip import layout as L
from held_tools import HEADER, struct_fields

KS = (0, 1, 2, 4)
FAKE = C.c_void_p(0x100000)
RECORD = "atc_policy_forward_launch_counts"


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- round trips
@pytest.mark.parametrize("K", KS)
def test_policy_unpack_to_torch_from_torch_round_trip(K):
    import torch
    from atc_hip import policy
    w_np = P.random_weights(np.random.default_rng(40 + K), 1.0, (-1.0, 0.5, -0.25), K=K)
    w_np[3] = np.float32("nan")      # (a bit pattern that arithmetic would not keep)
    w = torch.from_numpy(w_np.copy())
    parts = policy.unpack(w)
    assert list(parts) == [n for n, _ in policy.shapes(K)] and [tuple(v.shape) for v in parts.values()] == [s for _, s in policy.shapes(K)]
    ref = P.split(w_np, K)
    for name, v in parts.items():
        assert np.array_equal(_bits(v), ref[name].view(np.uint32)), name
    parts["b3"][1] = 7.0      # views: writing to one writes to w
    assert float(w[policy.offsets(K)["b3"][0] + 1]) == 7.0
    w[policy.offsets(K)["b3"][0] + 1] = float(w_np[policy.offsets(K)["b3"][0] + 1])
    assert policy.traffic_of(w.numel()) == K and list(policy.unpack(w_np, K)) == list(parts)      # (arrays as well)
    with pytest.raises(ValueError):
        policy.unpack(w[:-1])
    with pytest.raises(ValueError):
        policy.unpack(w, traffic=(K + 1) % 3)
    net, log_std = policy.to_torch(w)
    back = policy.from_torch(net, log_std, traffic=K)
    assert back.dtype == torch.float32 and np.array_equal(_bits(back), w_np.view(np.uint32))
    # the module in float64 is the restatement's MLP
    w_np[3] = 0.25
    net, _ = policy.to_torch(torch.from_numpy(w_np))
    x = np.random.default_rng(1).uniform(-1, 1, (33, L.policy_in(K)))
    got = net.double()(torch.from_numpy(x)).detach().numpy()
    assert np.abs(got - P.mlp(w_np, x, K)).max() <= 1e-12


@pytest.mark.parametrize("K", KS)
def test_value_unpack_to_torch_from_torch_round_trip(K):
    import torch
    from atc_hip import value
    w_np = np.random.default_rng(50 + K).normal(0, 0.2, L.value_words(K)).astype(np.float32)
    w = torch.from_numpy(w_np.copy())
    parts = value.unpack(w)
    assert list(parts) == [n for n, _ in value.shapes(K)] and [tuple(v.shape) for v in parts.values()] == [s for _, s in value.shapes(K)]
    at = 0
    for name, v in parts.items():
        assert np.array_equal(_bits(v).reshape(-1), w_np[at:at + v.numel()].view(np.uint32)), name
        at += v.numel()
    assert at == w.numel() and value.traffic_of(w.numel()) == K
    with pytest.raises(ValueError):
        value.unpack(w[:-1])
    net = value.to_torch(w)
    assert np.array_equal(_bits(value.from_torch(net, traffic=K)), w_np.view(np.uint32))
    x = np.random.default_rng(2).uniform(-1, 1, (17, L.policy_in(K)))
    got = net.double()(torch.from_numpy(x)).detach().numpy().reshape(-1)
    assert np.abs(got - np.asarray(PV.forward(w_np, x, K)).reshape(-1)).max() <= 1e-12


@pytest.mark.parametrize("K,VK", [(0, None), (2, 2), (4, 0)])
def test_checkpoint_round_trip_without_pickle(tmp_path, K, VK):
    import torch
    from atc_hip import checkpoint
    rng = np.random.default_rng(60 + K)
    w = P.random_weights(rng, 1.0, (-1.0, 0.5, 0.0), K=K)
    vw = None if VK is None else rng.normal(0, 0.3, L.value_words(VK)).astype(np.float32)
    path = str(tmp_path / "agent.npz")
    checkpoint.save(path, torch.from_numpy(w), vw, steps=12345, sector="LOWW", sim={"normalize": True})
    with np.load(path, allow_pickle=False) as z:      # a plain .npz: no pickle anywhere in it
        assert "policy/W1" in z.files and "policy/log_std" in z.files and int(z["policy/traffic"]) == K
        assert ("value/W3" in z.files) == (vw is not None)
        assert all(z[n].dtype != object for n in z.files)
    got = checkpoint.load(path)
    assert got["meta"] == {"steps": 12345, "sector": "LOWW", "sim": {"normalize": True}} and got["traffic"] == K and got["value_traffic"] == VK
    assert got["policy"].dtype == torch.float32 and np.array_equal(_bits(got["policy"]), w.view(np.uint32))
    assert (got["value"] is None) if vw is None else np.array_equal(_bits(got["value"]), vw.view(np.uint32))
    with pytest.raises(ValueError):
        checkpoint.save(path, w.astype(np.float64))
    with pytest.raises(ValueError):
        checkpoint.save(path, w[:-1])


# ---------------------------------------------------------------------------------------------------------------- the keys
def test_keys_are_the_rollouts_on_its_numbering():
    D, B, N, seed, d0 = 5, 3, 4, 0x1234567890ABCDEF, 0xFFFFFFFE      # (decision0 + d wraps)
    R, BN = D * B * N, B * N
    dec, i = PF.keys(R, BN, 1, d0)
    want_d, want_i, _ = H.draw_indices(d0, D, 1, BN)
    assert np.array_equal(dec[0].reshape(D, BN), np.broadcast_to(want_d[:, :, 0] & 0xffffffff, (D, BN)))
    assert np.array_equal(i[0].reshape(D, BN), np.broadcast_to(want_i[:, :, 0], (D, BN)))
    assert np.array_equal(P.key(seed, dec[0], i[0]).reshape(D, BN), P.key(seed, want_d[:, :, 0], want_i[:, :, 0]))
    # further samples continue the decision counter: no two (decision, i) of a call are equal
    for R, Pr, S in ((60, 12, 3), (65, 7, 3), (1, 1, 3), (10, 10, 3), (64, 1, 3)):
        dec, i = PF.keys(R, Pr, S, 9)
        pairs = set(zip(dec.reshape(-1).tolist(), i.reshape(-1).tolist()))
        assert len(pairs) == S * R, (R, Pr, S)
        assert np.array_equal(dec[0], PF.keys(R, Pr, 1, 9)[0][0])      # sample 0 is the S = 1 call
        assert dec.min() == 9 and dec.max() == 9 + (S - 1) * ((R + Pr - 1) // Pr) + (R - 1) // Pr
    keys = P.key(5, *PF.keys(65, 7, 3, 9))
    assert len(set(keys.reshape(-1).tolist())) == 3 * 65


# ---------------------------------------------------------------------------------------------------------------- the ABI
def _decl(text, name):
    decl = re.search(r"^int %s\((.*?)\);" % name, text, flags=re.S | re.M).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return [" ".join(a.split()) for a in decl.split(",")]


def test_header_constants_structs_and_argtypes():
    from atc_hip import lib
    text = open(HEADER).read()
    assert L.POLICY_FWD_MAX_SAMPLES == int(re.search(r"ATC_POLICY_FWD_MAX_SAMPLES = (\d+)", text).group(1)) == 64
    assert L.POLICY_FORWARD_LAUNCH_SLOTS == int(re.search(r"ATC_POLICY_FORWARD_LAUNCH_SLOTS = (\d+)", text).group(1)) == 4
    assert L.ABI_VERSION == 22 and int(re.search(r"#define ATC_ABI_VERSION (\d+)", text).group(1)) == 22      # a new entry point: the ABI number stays
    f = struct_fields(text, "atc_policy_fwd")
    assert [x[1] for x in f] == list(lib.POLICY_FWD_FIELDS) == [x[0] for x in lib.AtcPolicyFwd._fields_]
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    assert [ctype[x[0]] for x in f] == [x[1] for x in lib.AtcPolicyFwd._fields_] and C.sizeof(lib.AtcPolicyFwd) == 32
    assert lib.AtcPolicyFwd.seed.offset == 16 and lib.AtcPolicyFwd.decision0.offset == 24
    o = struct_fields(text, "atc_policy_fwd_out")
    assert [x[1].lstrip("*") for x in o] == list(lib.POLICY_FWD_OUT_FIELDS) == [x[0] for x in lib.AtcPolicyFwdOut._fields_] == ["mean", "action", "flown", "logp"]
    assert all(x[1].startswith("*") and x[0] == "float" for x in o) and C.sizeof(lib.AtcPolicyFwdOut) == 32
    h = lib.load()
    vp, ci = C.c_void_p, C.c_int
    args = _decl(text, "atc_policy_forward")
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "R", "w", "obs_rows", "traffic", "f", "out", "stream"]
    want = [ci if a.startswith("int ") else C.POINTER(lib.AtcPolicyFwdOut) if "atc_policy_fwd_out_t" in a else
            C.POINTER(lib.AtcPolicyFwd) if "atc_policy_fwd_t" in a else vp for a in args]
    assert list(h.atc_policy_forward.argtypes) == want and h.atc_policy_forward.restype is ci
    assert {"atc_policy_forward", RECORD} <= set(lib.EXPORTS)
    assert list(getattr(h, RECORD).argtypes) == [C.POINTER(C.c_uint64), ci]
    slots, slot_name = lib.LAUNCH_RECORDS[RECORD]
    assert slots == 4 and [slot_name(i) for i in range(4)] == [0, 1, 2, 4] and callable(lib.policy_forward_launch_counts)


def test_launch_record_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    buf = (C.c_uint64 * 8)(*([99] * 8))
    assert getattr(h, RECORD)(buf, 8) == 0
    assert all(v != 99 for v in buf[:4]) and all(v == 99 for v in buf[4:])
    assert getattr(h, RECORD)(None, 1) == -1
    assert RECORD in lib.launch_records() and isinstance(lib.policy_forward_launch_counts(), dict)


def _at(k):
    return 0x100000 + k * 0x10000000      # made-up ranges 256 MiB apart


PTRS = ("s", "w", "obs_rows", "f", "out")      # the pointers that may not be NULL, in the order they are looked at


def test_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    before = lib.launch_records()
    err = h.atc_last_error
    DET = L.POLICY_DETERMINISTIC

    def fwd(K=0, S=1, Pr=0, flags=0):
        return lib.AtcPolicyFwd(K, S, Pr, flags, 5, 9, 0)

    def call(R=1, traffic=None, **a):
        return h.atc_policy_forward(a.get("s"), R, a.get("w"), a.get("obs_rows"), traffic, a.get("f"), a.get("out"), None)
    none = lib.AtcPolicyFwdOut(None, None, None, None)
    shared = lib.AtcPolicyFwdOut(_at(2), _at(2), _at(2), _at(2))      # every output ON obs_rows: the last refusal of all
    bad = fwd(3, 0, -1, DET | 8)      # everything behind the pointers wrong as well
    ok = dict(s=FAKE, w=C.c_void_p(_at(1)), obs_rows=C.c_void_p(_at(2)), f=C.byref(bad), out=C.byref(none))
    # 1. the pointers in their order
    for j, name in enumerate(PTRS):
        named = re.compile(rb"null pointer: %s\b" % name.encode())
        assert call(0, **{k: ok[k] for k in PTRS[:j]}) == -1 and named.search(err()), (name, err())
        assert call(0, **dict(ok, **{name: None})) == -1 and named.search(err()), (name, err())
    # 2. traffic_k, 3. R, 4. samples, rows_per_decision, 5. deterministic with S > 1, 6. unknown flags, 7. traffic iff K > 0, 8. no output,
    # 9. overlaps: each with every later one wrong as well
    for K in (3, -1, 5, 8):
        assert call(0, **dict(ok, f=C.byref(fwd(K, 0, -1, DET | 8)))) == -1 and b"traffic_k" in err()
    for R in (0, -1):
        assert call(R, **dict(ok, f=C.byref(fwd(1, 0, -1, DET | 8)))) == -1 and b"R (" in err()
    for S in (0, -1, 65):
        assert call(5, **dict(ok, f=C.byref(fwd(1, S, -1, DET | 8)))) == -1 and b"samples" in err() and b"64" in err()
    for Pr in (-1, 6):
        assert call(5, **dict(ok, f=C.byref(fwd(1, 2, Pr, DET | 8)))) == -1 and b"rows_per_decision" in err()
    for Pr in (0, 1, 5):      # 0 means R; 1 .. R pass: the next refusal is the deterministic one
        assert call(5, **dict(ok, f=C.byref(fwd(1, 2, Pr, DET | 8)))) == -1 and b"DETERMINISTIC" in err()
    assert call(5, **dict(ok, f=C.byref(fwd(1, 64, 5, DET)))) == -1 and b"DETERMINISTIC" in err()
    for flags in (DET | 8, 2, 0x80000000):
        assert call(5, **dict(ok, f=C.byref(fwd(1, 1, 5, flags)))) == -1 and b"unknown bits" in err()
    assert call(5, **dict(ok, f=C.byref(fwd(1, 1, 5, DET)))) == -1 and b"traffic is required" in err()
    assert call(5, traffic=C.c_void_p(_at(3)), **dict(ok, f=C.byref(fwd(0, 64, 0, 0)))) == -1 and b"traffic must be NULL" in err()
    assert call(5, **dict(ok, f=C.byref(fwd(0, 64, 0, 0)))) == -1 and b"no output" in err()
    assert call(5, traffic=C.c_void_p(_at(3)), **dict(ok, f=C.byref(fwd(4, 1, 0, DET)))) == -1 and b"no output" in err()
    assert call(5, **dict(ok, f=C.byref(fwd(0, 1, 0, 0)), out=C.byref(shared))) == -1 and b"overlaps" in err()
    # 9. the overlap rule, on pointer values: every output against every input and every other output; the inputs may share
    R, K, S = 7, 2, 3
    size = dict(w=L.policy_words(K) * 4, obs_rows=R * 40, traffic=R * K * 32, mean=R * 12, action=S * R * 12, flown=S * R * 12, logp=S * R * 4)
    base = {n: _at(k + 1) for k, n in enumerate(size)}
    fk = fwd(K, S, 0, 0)

    def run(p):
        o = lib.AtcPolicyFwdOut(p["mean"], p["action"], p["flown"], p["logp"])
        return h.atc_policy_forward(FAKE, R, C.c_void_p(p["w"]), C.c_void_p(p["obs_rows"]), C.c_void_p(p["traffic"]), C.byref(fk), C.byref(o), None)
    names, n = list(size), 0
    for b in ("mean", "action", "flown", "logp"):
        for a in names[:names.index(b)]:
            for off in (0, size[a] - 1, -(size[b] - 1)):
                assert run(dict(base, **{b: base[a] + off})) == -1 and b"overlaps" in err() and a.encode() in err() and b.encode() in err(), (a, b, off, err())
                n += 1
    assert n == (3 + 4 + 5 + 6) * 3
    assert lib.launch_records() == before, "a refused call moved a launch record"


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_python_surface():
    from atc_hip import agent, checkpoint, policy, value
    from atc_hip.vec_env import AtcVecEnv
    sig = inspect.signature(AtcVecEnv.policy_forward)
    assert list(sig.parameters) == ["self", "weights", "obs_rows", "traffic", "samples", "rows_per_decision", "seed", "decision0", "deterministic", "outputs", "out"]
    kw = list(sig.parameters)[3:]
    assert [sig.parameters[k].default for k in kw] == [None, 1, None, 0, 0, False, ("flown", "logp"), None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kw)
    sig = inspect.signature(AtcVecEnv.act)
    assert list(sig.parameters) == ["self", "weights", "samples", "seed", "decision", "deterministic", "out"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, 0, 0, False, None]
    assert list(inspect.signature(agent.Agent.predict).parameters) == ["self", "obs", "state", "mask", "deterministic"]
    assert list(inspect.signature(checkpoint.save).parameters) == ["path", "w", "vw", "meta"] and list(inspect.signature(checkpoint.load).parameters) == ["path", "device"]
    for mod in (policy, value):
        assert list(inspect.signature(mod.unpack).parameters) == ["w", "traffic"] and list(inspect.signature(mod.to_torch).parameters)[0] == "w"
    # no existing signature changed
    assert list(inspect.signature(policy.from_torch).parameters) == ["module", "log_std", "device", "traffic"]
    assert list(inspect.signature(value.from_torch).parameters) == ["module", "device", "traffic"]


class _NoLibrary:
    """an env stand-in whose library handle fails the test when anything is called through it"""
    B, N, traffic_k = 3, 2, 0

    class _lib:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)
    _lib = _lib()

    class sector:
        handle = None

    class params:
        mode = 0

    def __init__(self):
        import torch
        self.torch = torch
        self.device = torch.device("cpu")
        self.obs = torch.zeros(self.B, self.N * 10)
        self.traffic = None

    def _stream(self):
        return None


def test_policy_forward_and_act_refuse_before_any_library_call():
    import torch
    from atc_hip.vec_env import AtcVecEnv
    env = _NoLibrary()
    w0, w2 = torch.zeros(L.policy_words(0)), torch.zeros(L.policy_words(2))
    rows = torch.zeros(4, 3, 10)

    def refused(match, w=w0, x=rows, **kw):
        with pytest.raises(ValueError, match=match):
            AtcVecEnv.policy_forward(env, w, x, **kw)
    for w in (torch.zeros(L.value_words(0)), w0.double(), torch.zeros(2 * L.policy_words(0))[::2], np.zeros(L.policy_words(0), np.float32),
              torch.zeros(L.policy_words(0), device="meta")):
        refused("weights", w=w)
    for x in (torch.zeros(5, 9), torch.zeros(0, 10), torch.zeros(5, 10, dtype=torch.float64), torch.zeros(10, 5).t(), np.zeros((5, 10), np.float32)):
        refused("obs_rows", x=x)
    refused("traffic", traffic=torch.zeros(4, 3, 2, 8))      # the ten-word policy with records
    refused("traffic", w=w2)      # a traffic policy without
    for t in (torch.zeros(4, 3, 4, 8), torch.zeros(4, 3, 2, 7), torch.zeros(4, 2, 2, 8), torch.zeros(4, 3, 2, 8, dtype=torch.float64)):
        refused("traffic", w=w2, traffic=t)
    for S in (0, 65):
        refused("samples", samples=S)
    refused("samples", samples=2, deterministic=True)
    for Pr in (0, 13, -1):
        refused("rows_per_decision", rows_per_decision=Pr)
    refused("outputs", outputs=())
    refused("outputs", outputs=("flown", "value"))
    refused("out", out={})
    refused("out", out={"value": torch.zeros(4, 3)})
    refused(r"out\['flown'\]", out={"flown": torch.zeros(4, 3, 3)})      # (the sample axis is missing)
    refused(r"out\['logp'\]", out={"logp": torch.zeros(1, 4, 3, dtype=torch.float64)})
    refused(r"out\['mean'\]", out={"mean": torch.zeros(1, 4, 3, 3)})
    good = {"mean": torch.zeros(4, 3, 3), "action": torch.zeros(2, 4, 3, 3), "flown": torch.zeros(2, 4, 3, 3), "logp": torch.zeros(2, 4, 3)}
    with pytest.raises(AssertionError, match="the library was called"):
        AtcVecEnv.policy_forward(env, w0, rows, samples=2, rows_per_decision=6, out=good)
    with pytest.raises(AssertionError, match="the library was called"):
        AtcVecEnv.policy_forward(env, w2, rows, traffic=torch.zeros(4, 3, 2, 8), outputs="mean")
    # act: the policy's K against the env's, a discrete env, out's shape
    with pytest.raises(ValueError, match="traffic"):
        AtcVecEnv.act(env, w2)
    with pytest.raises(ValueError, match="out"):
        AtcVecEnv.act(env, w0, samples=2, out=torch.zeros(3, 2, 3))
    with pytest.raises(AssertionError, match="the library was called"):
        AtcVecEnv.act(env, w0, samples=2, out=torch.zeros(2, 3, 2, 3))
    env.params.mode = L.M_DISCRETE
    with pytest.raises(ValueError, match="discrete"):
        AtcVecEnv.act(env, w0)
    env.params.mode = 0
