"""The traffic observation (include/atc_step.h: atc_observe_traffic; AtcVecEnv(traffic=K), AtcSBVecEnv(traffic=K)): for every
aircraft its K nearest other aircraft under control, nearest first, as 8-word records in its own frame.

The kernel reads only state, so the tests write state tensors directly (the named views of AtcVecEnv are live memory) and compare
with the numpy reference of tests/traffic_ref.py, which evaluates the ordering key exactly and the features in float64.
CPU: hand-computed known answers pin the reference; the conditions the GPU cases' inputs must contain, asserted on the reference
alone; the ABI's K check, the launch record, the k_traffic symbols, the Python surface.
GPU: every lane-group width with idle lanes, ragged batches, K in {1, 3, 4, 8}, normalisation on and off, two state families
(random / clustered: exact ties and coincident aircraft), buffer guards, state untouched, the launch record; the env and adapter
surface; the full 65 536 x 16 batch once.

Bars (no case is left out of any comparison): words 0 and 7 and the whole absent pattern exact; word 4 exact (normalised: the
fp32 quotient of the exact difference); words 1..3 within 1e-5 max(1, d) — the operands' magnitude: ahead / right are sums of
products of size d; words 5..6 within 1e-5 max(1, v_i + v_j); normalised words the same bars divided by the scale."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import traffic_ref as R
from atc_hip import layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "atc-reinforcement-learning_amd", "atc_hip", "libatcstep.so")
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
NS = (1, 2, 3, 8, 16, 32, 33, 64)       # every width, idle lanes for 3 and 33
KS = (1, 3, 4, 8)
FULL_SIZE = dict(B=65536, N=16, K=4, seed=5, compared=256)


@functools.lru_cache(maxsize=None)
def _sector():
    from envs.atc import scenarios
    scn = scenarios.LOWW()
    return scn, scenarios.compile_scenario(scn, grid_cell=0.5)


@functools.lru_cache(maxsize=None)
def _case(N, family):
    """(state, reference) of one shape-matrix case: computed once, shared by the CPU conditions and the GPU comparisons, never changed"""
    comp = _sector()[1]
    rng = np.random.default_rng(1000 * N + len(family))
    st = R.FAMILIES[family](rng, H.ragged(N), N, comp.pos_k)
    return st, R.traffic_reference(st, comp.pos_origin, comp.pos_k)


# ---------------------------------------------------------------------------------------------------------------- CPU
def _place(aircraft, mask, K=None):
    """aircraft: [(x nm, y nm, h ft, heading deg, v kt)] of ONE env on LOWW's grid (integer nm / deg / kt) -> the reference's records"""
    comp = _sector()[1]
    a = np.array(aircraft, dtype=np.int64)
    st = dict(x_fix=((a[:, 0] - int(comp.pos_origin[0])) << comp.pos_k).astype(np.int32)[None],
              y_fix=((a[:, 1] - int(comp.pos_origin[1])) << comp.pos_k).astype(np.int32)[None],
              h=a[:, 2].astype(np.float64)[None], P=((a[:, 3] - 180) << 23).astype(np.float64)[None],
              v_fix=(a[:, 4] << 23).astype(np.uint32)[None], mask=np.array([mask], np.uint64))
    return R.traffic_reference(st, comp.pos_origin, comp.pos_k)


def test_reference_known_answers():
    near = lambda a, b: abs(a - b) <= 1e-12 * max(1.0, abs(b))   # noqa: E731
    me = (40, 40, 5000, 90, 250)
    # an intruder 3 nm east of an aircraft heading east: dead ahead; 500 ft above, same velocity
    r = _place([me, (43, 40, 5500, 90, 250)], 0b11)
    rec = r["rec"][0, 0, 0]
    assert rec[L.T_PRESENT] == 1 and near(rec[L.T_DIST], 3) and near(rec[L.T_AHEAD], 3) and abs(rec[L.T_RIGHT]) < 1e-12
    assert rec[L.T_DH] == 500 and abs(rec[L.T_DV_AHEAD]) < 1e-9 and abs(rec[L.T_DV_RIGHT]) < 1e-9 and rec[L.T_SLOT] == 1
    back = r["rec"][0, 1, 0]     # and seen from the intruder: 3 nm behind, 500 ft below
    assert near(back[L.T_AHEAD], -3) and back[L.T_DH] == -500 and back[L.T_SLOT] == 0
    # 4 nm north of an aircraft heading east: on its left
    rec = _place([me, (40, 44, 5000, 0, 250)], 0b11)["rec"][0, 0, 0]
    assert near(rec[L.T_DIST], 4) and abs(rec[L.T_AHEAD]) < 1e-12 and near(rec[L.T_RIGHT], -4)
    # the same intruder seen by an aircraft heading north (0) / south (180): ahead / behind
    assert near(_place([(40, 40, 0, 0, 250), (40, 44, 0, 0, 250)], 0b11)["rec"][0, 0, 0, L.T_AHEAD], 4)
    assert near(_place([(40, 40, 0, 180, 250), (40, 44, 0, 0, 250)], 0b11)["rec"][0, 0, 0, L.T_AHEAD], -4)
    # two intruders at exactly 3 nm: the lower slot first, whichever way round they are placed
    for a, b in (((43, 40), (40, 43)), ((40, 43), (43, 40))):
        r = _place([me, a + (5000, 0, 250), b + (5000, 0, 250)], 0b111)
        assert list(r["rec"][0, 0, :3, L.T_SLOT]) == [1, 2, -1] and r["d2"][0, 0, 0] == r["d2"][0, 0, 1] == 9.0
    # a nearer intruder in a higher slot still comes first
    assert list(_place([me, (43, 40, 0, 0, 250), (41, 40, 0, 0, 250)], 0b111)["rec"][0, 0, :2, L.T_SLOT]) == [2, 1]
    # a coincident intruder: d = 0
    rec = _place([me, (40, 40, 7000, 180, 300)], 0b11)["rec"][0, 0, 0]
    assert rec[L.T_PRESENT] == 1 and rec[L.T_DIST] == 0 and rec[L.T_AHEAD] == 0 and rec[L.T_RIGHT] == 0 and rec[L.T_DH] == 2000
    # head-on at 250 kt each: closing at 500 kt
    rec = _place([me, (50, 40, 5000, 270, 250)], 0b11)["rec"][0, 0, 0]
    assert near(rec[L.T_AHEAD], 10) and near(rec[L.T_DV_AHEAD], -500) and abs(rec[L.T_DV_RIGHT]) < 1e-9
    # a handed-over intruder is skipped; a handed-over observer gets nothing
    r = _place([me, (41, 40, 5000, 0, 250), (45, 40, 5000, 0, 250)], 0b101)
    assert list(r["rec"][0, 0, :2, L.T_SLOT]) == [2, -1] and r["ncand"][0, 0] == 1
    assert not r["present"][0, 1].any() and np.all(r["rec"][0, 1, :, :7] == 0) and np.all(r["rec"][0, 1, :, 7] == -1)
    # K beyond the candidates: absent tails (words 0..6 = 0, word 7 = -1)
    r = _place([me, (41, 40, 5000, 0, 250), (45, 40, 5000, 0, 250)], 0b111)
    assert list(r["present"][0, 0]) == [True, True] + [False] * 6
    assert np.all(r["rec"][0, 0, 2:, :7] == 0) and np.all(r["rec"][0, 0, 2:, 7] == -1)
    # one aircraft: nothing to see
    assert not _place([me], 0b1)["present"].any()


def test_reference_key_is_the_single_rounding_fma():
    """the exact key against cases where float64 arithmetic rounds twice, and against float64 where it cannot"""
    rng = np.random.default_rng(0)
    for _ in range(2000):
        dx, dy = np.float32(rng.normal(0, 30)), np.float32(rng.normal(0, 30))
        p = dy * dy
        exact = R.fma_sq_f32(dx, p)
        assert np.float32(exact) == exact                                          # a float32 value
        lo, hi = np.nextafter(np.float32(exact), np.float32(-1)), np.nextafter(np.float32(exact), np.float32(np.inf))
        true = float(dx) * float(dx) + float(p)                                    # (float64: good to 2^-53 relative)
        assert abs(true - exact) <= min(abs(true - float(lo)), abs(true - float(hi))) * (1 + 1e-9)
    assert R.fma_sq_f32(np.float32(3), np.float32(0)) == 9.0 and R.fma_sq_f32(np.float32(0), np.float32(0)) == 0.0
    # a tie that only ONE rounding gets right: 1 + 2^-24 + 2^-60 must round up to 1 + 2^-23
    assert R._round_f32((1 << 60) + (1 << 36) + 1, 60) == 1.0 + 2.0 ** -23 and R._round_f32((1 << 60) + (1 << 36), 60) == 1.0


def test_gpu_case_inputs_contain_the_edge_cases():
    """on the reference alone: what the shape-matrix cases must exercise is in their inputs"""
    tie_at = {K: 0 for K in KS}
    coincident = few = inactive = wide = 0
    for N in NS:
        for family in R.FAMILIES:
            st, ref = _case(N, family)
            act = R.active_bits(st["mask"], N)
            assert st["x_fix"].shape == (H.ragged(N), N)
            counts = act.sum(1)
            assert counts.min() == 0 and counts.max() == N, "masks with no and with every bit set"
            inactive += int((~act).sum())
            for K in KS:
                tie_at[K] += int(np.sum(np.isfinite(ref["d2"][:, :, K]) & (ref["d2"][:, :, K - 1] == ref["d2"][:, :, K])))
                few += int(np.sum(act & (ref["ncand"] < K)))
            coincident += int(np.sum(ref["present"] & (ref["d"] == 0)))
            if N >= 2:
                w = R.phi_fields(st["P"])[1]
                wide += int(np.sum(w & act & (ref["ncand"] > 0)))
                assert np.any(w & act & (ref["ncand"] > 0)), "a WIDE heading on an observer with traffic"
            if N > 32:
                assert np.any((st["mask"] >> np.uint64(32)) != (np.uint64(1) << np.uint64(N - 32)) - np.uint64(1)), "a mask bit >= 32 clear"
                assert np.any(~act[:, 32:] & (counts > 1)[:, None])
    assert all(tie_at[K] > 0 for K in KS), tie_at        # an exact d2 tie across the rank K / K + 1 boundary, for every K
    assert coincident > 0 and few > 0 and inactive > 0 and wide > 0
    st, ref = _case(16, "clustered")                       # ... and in the flagship width's clustered case alone
    assert all(np.any(np.isfinite(ref["d2"][:, :, K]) & (ref["d2"][:, :, K - 1] == ref["d2"][:, :, K])) for K in KS)
    assert np.any(ref["present"] & (ref["d"] == 0))


def test_k_out_of_range_is_refused_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    for K in (0, 9, -3):
        assert h.atc_observe_traffic(None, 1, 1, K, None, None, None, None) == -1   # ATC_ERR_ARG, before any pointer is looked at
        assert b"K" in h.atc_last_error() and b"8" in h.atc_last_error()
    assert h.atc_observe_traffic(None, 1, 1, 1, None, None, None, None) == -1        # K in range: now the null pointers
    assert b"null" in h.atc_last_error()
    buf = (C.c_uint64 * L.TRAFFIC_LAUNCH_SLOTS)()
    assert h.atc_traffic_launch_counts(buf, L.TRAFFIC_LAUNCH_SLOTS) == 0 and isinstance(lib.traffic_launch_counts(), dict)
    assert h.atc_traffic_launch_counts(None, 7) == -1
    assert L.ABI_VERSION == 22 and L.LAUNCH_SLOTS == 57 and L.TRAFFIC_LAUNCH_SLOTS == 7
    assert (L.TRAFFIC_DIM, L.TRAFFIC_MAX_K) == (8, 8)
    assert (L.T_PRESENT, L.T_DIST, L.T_AHEAD, L.T_RIGHT, L.T_DH, L.T_DV_AHEAD, L.T_DV_RIGHT, L.T_SLOT) == tuple(range(8))


def test_library_has_k_traffic_for_the_seven_widths():
    assert os.path.exists(LIB)
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert nm, "no nm to read the library's symbol table with"
    text = subprocess.run([nm, "-C", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    found = {int(a.split(",")[0]) for a in re.findall(r"\bvoid k_traffic<([^>]*)>\(", text)}
    assert found == set(WIDTHS), found


def test_python_surface():
    from atc_hip import lib
    from atc_hip.sb_adapter import AtcSBVecEnv
    from atc_hip.vec_env import AtcVecEnv
    assert {"atc_observe_traffic", "atc_traffic_launch_counts"} <= set(lib.EXPORTS) and callable(lib.traffic_launch_counts)
    assert inspect.signature(AtcVecEnv.__init__).parameters["traffic"].default == 0
    assert inspect.signature(AtcSBVecEnv.__init__).parameters["traffic"].default == 0
    assert list(inspect.signature(AtcVecEnv.observe_traffic).parameters) == ["self"]
    assert "traffic" in AtcVecEnv.rollout.__doc__
    h = lib.load()
    assert len(h.atc_observe_traffic.argtypes) == 8 and len(h.atc_traffic_launch_counts.argtypes) == 2


def test_default_keeps_info_keys_and_observation_space():
    """traffic=0: no new info key (AtcVecEnv._info builds them from the env's tensors) and the adapter's space as it was"""
    from atc_hip.sb_adapter import AtcSBVecEnv
    from atc_hip.vec_env import AtcVecEnv

    class Stub:
        flags = ep_return = ep_length = raw_obs = term_obs = 1
        ac_reward = min_sep = traffic = None
    assert set(AtcVecEnv._info(Stub())) == {"flags", "ep_return", "ep_length", "original_state", "terminal_observation"}
    Stub.traffic = 1
    assert set(AtcVecEnv._info(Stub())) == {"flags", "ep_return", "ep_length", "original_state", "terminal_observation", "traffic"}
    # (the adapter's space is built from the env it wraps: with traffic=0 its traffic part has zero columns; on the GPU,
    # test_sb_adapter_widens_the_observation checks the plain adapter's shape next to the widened one)
    assert inspect.signature(AtcSBVecEnv.__init__).parameters["traffic"].default == 0


# ---------------------------------------------------------------------------------------------------------------- GPU
_ENVS = {}


def _env_for(N, B=None):
    """one plain env per shape (traffic=0: the launches below go through the C-ABI with their own buffers)"""
    from atc_hip.vec_env import AtcVecEnv
    key = (N, B or H.ragged(N))
    if key not in _ENVS:
        _ENVS[key] = AtcVecEnv(key[1], N, scenario=_sector()[0], auto_reset=True, spawn="lattice", grid_cell=0.5)
    return _ENVS[key]


def _put_state(env, st):
    """writes a reference state into the env's live state tensors; side records of headings in range get a poison value"""
    torch = env.torch
    B, N = env.B, env.N
    phi_fix, wide = R.phi_fields(st["P"])
    ac = np.stack([st["x_fix"], st["y_fix"], phi_fix, st["v_fix"].view(np.int32)], axis=-1).reshape(B * N, 4).astype(np.int32)
    env.ac.copy_(torch.from_numpy(ac))
    env.alt.copy_(torch.from_numpy(np.ascontiguousarray(st["h"].reshape(-1))))
    pw = np.full((B * N, 4), 1e300)
    pw[:, 0] = np.where(wide, st["P"], 1e300).reshape(-1)
    env.phi_wide.copy_(torch.from_numpy(pw))
    m = st["mask"].astype(np.uint64)
    env.env[:, L.ENV_MASK_LO] = torch.from_numpy((m & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)).to(env.device)
    env.stats[:, L.STAT_MASK_HI] = torch.from_numpy((m >> np.uint64(32)).astype(np.uint32).view(np.int32)).to(env.device)
    env.synchronize()


def _state_bits(env):
    t = env.torch
    return [x.clone().view(t.int64 if x.dtype == t.float64 else x.dtype) for x in (env.ac, env.alt, env.last_act, env.env, env.stats, env.phi_wide)]


SENTINEL, GUARD_ROWS = -7777.0, 5


def _launch(env, K, normalize):
    """atc_observe_traffic through the C-ABI into a sentinel-filled buffer with guard rows; returns ([B, N, K, 8], guards)"""
    from atc_hip import lib
    torch = env.torch
    rows = env.B * env.N
    buf = torch.full(((rows + GUARD_ROWS) * K * L.TRAFFIC_DIM,), SENTINEL, dtype=torch.float32, device=env.device)
    p = type(env.params).from_buffer_copy(env.params)
    p.mode = (p.mode | L.M_NORMALIZE) if normalize else (p.mode & ~L.M_NORMALIZE)
    lib.check(lib.load().atc_observe_traffic(env.sector.handle, env.B, env.N, K, C.byref(env._state), buf.data_ptr(), C.byref(p),
                                             lib.current_stream_ptr(env.device)))
    env.synchronize()
    out = buf.cpu().numpy()
    return out[:rows * K * L.TRAFFIC_DIM].reshape(env.B, env.N, K, L.TRAFFIC_DIM), out[rows * K * L.TRAFFIC_DIM:]


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
@pytest.mark.parametrize("N", NS)
def test_shape_matrix_against_the_reference(N, family):
    from atc_hip import lib
    st, ref = _case(N, family)
    env = _env_for(N)
    _put_state(env, st)
    before = _state_bits(env)
    scales = R.norm_scales(_sector()[1])
    W = H.lane_width(N)
    for K in KS:
        for normalize in (False, True):
            steps0, skips0, tr0 = lib.launch_counts(), lib.skip_launch_counts(), lib.traffic_launch_counts()
            got, guards = _launch(env, K, normalize)
            tr1 = lib.traffic_launch_counts()
            assert {w: tr1.get(w, 0) - tr0.get(w, 0) for w in WIDTHS} == {w: int(w == W) for w in WIDTHS}, "launch record"
            assert lib.launch_counts() == steps0 and lib.skip_launch_counts() == skips0
            assert np.all(guards == np.float32(SENTINEL)), "wrote beyond [B * N][K][8]"
            assert not np.any(got == np.float32(SENTINEL)), "a row of [B * N] was not written"
            bad = R.compare(got, ref, K, scales if normalize else None)
            print("N %d %s K %d normalize %d: %s" % (N, family, K, normalize, bad or "ok"))
            assert not bad, (K, normalize, bad)
    after = _state_bits(env)
    assert all(env.torch.equal(a, b) for a, b in zip(before, after)), "the query changed the state"


@pytest.mark.gpu
def test_refusals_count_nothing():
    from atc_hip import lib
    env = _env_for(16)
    h = lib.load()
    tr0 = lib.traffic_launch_counts()
    buf = env.torch.zeros(env.B * env.N * 8 * L.TRAFFIC_DIM, device=env.device)
    args = lambda K, out: (env.sector.handle, env.B, env.N, K, C.byref(env._state), out, C.byref(env.params), lib.current_stream_ptr(env.device))  # noqa: E731
    assert h.atc_observe_traffic(*args(9, buf.data_ptr())) == -1 and h.atc_observe_traffic(*args(0, buf.data_ptr())) == -1
    assert h.atc_observe_traffic(*args(4, None)) == -1 and b"null" in h.atc_last_error()
    assert h.atc_observe_traffic(env.sector.handle, env.B, 65, 4, C.byref(env._state), buf.data_ptr(), C.byref(env.params), None) == -1
    assert lib.traffic_launch_counts() == tr0


def _check_env_traffic(env, traffic, what):
    """info["traffic"] against the reference on the state copied back from the device"""
    env.synchronize()
    return R.check_traffic(traffic.cpu().numpy(), R.state_from_env(env), env.compiled, env.traffic_k, bool(env.params.mode & L.M_NORMALIZE), what)


@pytest.mark.gpu
def test_vec_env_surface():
    from atc_hip import lib
    from atc_hip.vec_env import AtcVecEnv
    env = AtcVecEnv(37, 16, scenario=_sector()[0], auto_reset=True, spawn="lattice", grid_cell=0.5, traffic=4, timestep_limit=7,
                    sep_nm=0.05, seed=2)
    assert tuple(env.traffic.shape) == (37, 16, 4, 8) and env.traffic.is_cuda
    rng = np.random.default_rng(4)
    tr0 = lib.traffic_launch_counts().get(16, 0)
    _check_env_traffic(env, env.traffic, "after the constructor's reset")
    obs = env.reset()
    ref = _check_env_traffic(env, env.traffic, "reset")
    assert ref["present"].all(), "16 aircraft under control: 4 records each"
    calls = 1
    for t in range(6):
        obs, rew, done, info = env.step(rng.uniform(-1, 1, (37, 16, 3)).astype(np.float32))
        assert info["traffic"] is env.traffic
        _check_env_traffic(env, info["traffic"], "step %d" % t)
        calls += 1
    obs, rew, done, info = env.step_skip(rng.uniform(-1, 1, (37, 16, 3)).astype(np.float32), 5)
    assert info["traffic"] is env.traffic and "frame_steps" in info
    _check_env_traffic(env, info["traffic"], "step_skip")
    assert done.cpu().numpy().any() and int(env.episodes.min()) >= 2, "envs restarted inside the calls"
    # restarted envs: the traffic describes the fresh spawn state, like the raw reset observation the step returned
    fresh = np.nonzero(done.cpu().numpy())[0]
    assert np.all(env.timesteps.cpu().numpy()[fresh] == 0)
    t = env.observe_traffic()
    assert t is env.traffic
    _check_env_traffic(env, t, "observe_traffic")
    env.observe()
    _check_env_traffic(env, env.traffic, "observe")
    assert lib.traffic_launch_counts().get(16, 0) - tr0 == calls + 3
    env.close()
    plain = _env_for(16)
    assert plain.traffic is None and "traffic" not in plain._info()
    with pytest.raises(ValueError):
        plain.observe_traffic()
    with pytest.raises(ValueError):
        AtcVecEnv(4, 2, scenario=_sector()[0], grid_cell=0.5, traffic=9)


@pytest.mark.gpu
def test_host_mapped_env_gets_traffic_in_host_memory():
    from atc_hip.vec_env import AtcVecEnv
    env = AtcVecEnv(5, 3, scenario=_sector()[0], auto_reset=True, spawn="lattice", grid_cell=0.5, traffic=2, host_mapped=True)
    assert not env.traffic.is_cuda and env.traffic.is_pinned()
    obs, rew, done, info = env.step(np.zeros((5, 3, 3), np.float32))
    _check_env_traffic(env, info["traffic"], "host-mapped step")
    env.close()


@pytest.mark.gpu
def test_sb_adapter_widens_the_observation():
    from atc_hip.sb_adapter import AtcSBVecEnv
    kw = dict(scenario=_sector()[0], seed=11, grid_cell=0.5, spawn="lattice", timestep_limit=5, sep_nm=0.05)
    wide, plain = AtcSBVecEnv(8, 3, traffic=2, **kw), AtcSBVecEnv(8, 3, **kw)
    own, tw = 3 * L.OBS_DIM, 3 * 2 * 7
    assert wide.observation_space.shape == (own + tw,) and plain.observation_space.shape == (own,)
    o_w, o_p = wide.reset(), plain.reset()
    assert o_w.shape == (8, own + tw) and o_p.shape == (8, own) and np.array_equal(o_w[:, :own], o_p)
    assert np.array_equal(o_w[:, own:], wide.vec.traffic.cpu().numpy()[..., :7].reshape(8, tw))
    rng = np.random.default_rng(3)
    seen_done = False
    for t in range(7):
        a = rng.uniform(-1, 1, (8, 9)).astype(np.float32)
        (o_w, r_w, d_w, i_w), (o_p, r_p, d_p, i_p) = wide.step(a), plain.step(a)
        assert o_w.shape == (8, own + tw) and np.array_equal(o_w[:, :own], o_p) and np.array_equal(r_w, r_p) and np.array_equal(d_w, d_p)
        ref = _check_env_traffic(wide.vec, wide.vec.traffic, "adapter step %d" % t)
        assert np.array_equal(o_w[:, own:], wide.vec.traffic.cpu().numpy()[..., :7].reshape(8, tw))
        assert np.all(o_w[:, own::7].reshape(8, 3, 2) == ref["present"][:, :, :2])
        for b in np.nonzero(d_w)[0]:
            seen_done = True
            term = i_w[b]["terminal_observation"]
            assert term.shape == (own + tw,) and np.array_equal(term[:own], i_p[b]["terminal_observation"])
            assert np.all(term[own:] == 0), "the traffic part of a terminal observation is absent records"
    assert seen_done
    wide.close()
    plain.close()


@pytest.mark.gpu
def test_full_size_batch():
    """65 536 x 16, K = 4, the random family: the first and the last 256 envs against the reference, every row written"""
    f = FULL_SIZE
    from atc_hip.vec_env import AtcVecEnv
    comp = _sector()[1]
    env = AtcVecEnv(f["B"], f["N"], scenario=_sector()[0], auto_reset=True, spawn="lattice", grid_cell=0.5)
    st = R.random_family(np.random.default_rng(f["seed"]), f["B"], f["N"], comp.pos_k)
    _put_state(env, st)
    got, guards = _launch(env, f["K"], True)
    assert np.all(guards == np.float32(SENTINEL)) and not np.any(got == np.float32(SENTINEL))
    assert np.all((got[..., L.T_PRESENT] == 0) | (got[..., L.T_PRESENT] == 1))
    n = f["compared"]
    for rows in (slice(0, n), slice(f["B"] - n, f["B"])):
        ref = R.traffic_reference({k: v[rows] for k, v in st.items()}, comp.pos_origin, comp.pos_k)
        bad = R.compare(got[rows], ref, f["K"], R.norm_scales(comp))
        print("full size, envs %s: %s" % (rows, bad or "ok"))
        assert not bad, bad
    env.close()


def _episode(info):
    return (info["episode"]["r"], info["episode"]["l"]) if "episode" in info else None


@pytest.mark.gpu
@pytest.mark.parametrize("frame_skip", [1, 5])
@pytest.mark.parametrize("n_envs,N,K,host_mapped", [(40, 8, 3, False), (600, 2, 1, None)], ids=["40x8 K3 dense infos", "600x2 K1 sparse infos"])
def test_sb_adapter_device_path_with_traffic(n_envs, N, K, host_mapped, frame_skip):
    """The adapter's DEVICE path (state in HBM: one packed device-to-host tensor per step, sliced by offsets — frame_steps at 3 d + 4,
    the traffic words in the last traffic_dim columns) with traffic, with and without frame_skip, next to a plain twin fed the same
    actions: own words, rewards, dones, frame_steps and episode records equal the twin's; the traffic columns are vec.traffic's words
    0..6, themselves checked against the reference on the state copied back; terminal observations carry zero traffic."""
    from atc_hip.sb_adapter import AtcSBVecEnv
    kw = dict(scenario=_sector()[0], seed=11, grid_cell=0.5, spawn="lattice", timestep_limit=6, sep_nm=0.05, frame_skip=frame_skip,
              host_mapped=host_mapped)
    wide, plain = AtcSBVecEnv(n_envs, N, traffic=K, **kw), AtcSBVecEnv(n_envs, N, **kw)
    assert not wide.vec.host_mapped and not plain.vec.host_mapped and wide.sparse_infos == plain.sparse_infos == (n_envs > 512)
    own, tw = N * L.OBS_DIM, N * K * 7
    assert wide.traffic_dim == tw and wide.observation_space.shape == (own + tw,)

    def traffic_columns(o, what):
        _check_env_traffic(wide.vec, wide.vec.traffic, what)
        assert np.array_equal(o[:, own:], wide.vec.traffic.cpu().numpy()[..., :7].reshape(n_envs, tw)), what

    o_w, o_p = wide.reset(), plain.reset()
    assert o_w.shape == (n_envs, own + tw) and np.array_equal(o_w[:, :own], o_p)
    traffic_columns(o_w, "reset")
    rng = np.random.default_rng(7)
    ends = 0
    for t in range(14 if frame_skip == 1 else 6):
        a = rng.uniform(-1, 1, (n_envs, 3 * N)).astype(np.float32)
        (o_w, r_w, d_w, i_w), (o_p, r_p, d_p, i_p) = wide.step(a), plain.step(a)
        assert o_w.shape == (n_envs, own + tw) and o_w.dtype == np.float32
        assert np.array_equal(o_w[:, :own], o_p) and np.array_equal(r_w, r_p) and np.array_equal(d_w, d_p), t
        traffic_columns(o_w, "step %d" % t)
        for b in range(n_envs):
            assert _episode(i_w[b]) == _episode(i_p[b]) and i_w[b].get("frame_steps") == i_p[b].get("frame_steps"), (t, b)
            assert ("episode" in i_w[b]) == bool(d_w[b])
            if d_w[b]:
                ends += 1
                term = i_w[b]["terminal_observation"]
                assert term.shape == (own + tw,) and np.array_equal(term[:own], i_p[b]["terminal_observation"])
                assert np.all(term[own:] == 0), "the traffic part of a terminal observation is absent records"
                assert frame_skip == 1 or 1 <= i_w[b]["frame_steps"] <= frame_skip
            elif wide.sparse_infos:
                assert i_w[b] == {} and i_p[b] == {}
            elif frame_skip > 1:
                assert i_w[b]["frame_steps"] == frame_skip
    assert ends >= n_envs, "episodes ended in every env"
    # env_method("reset", indices=...): [own | traffic] rows of the reset envs, the traffic that of the fresh state
    idx = [1, 5, n_envs - 1]
    rows_w, rows_p = wide.env_method("reset", indices=idx), plain.env_method("reset", indices=idx)
    _check_env_traffic(wide.vec, wide.vec.traffic, "env_method reset")
    tr = wide.vec.traffic.cpu().numpy()[..., :7].reshape(n_envs, tw)
    assert np.all(wide.vec.timesteps.cpu().numpy()[idx] == 0)
    for i, rw, rp in zip(idx, rows_w, rows_p):
        assert rw.shape == (own + tw,) and np.array_equal(rw[:own], rp) and np.array_equal(rw[own:], tr[i])
        assert rw[own] == 1.0, "a fresh env of %d aircraft: the first record of aircraft 0 is present" % N
    wide.close()
    plain.close()


@pytest.mark.gpu
def test_device_tensor_fast_path_with_traffic_on_a_side_stream():
    """AtcVecEnv(traffic=4).step / .step_skip handed a contiguous float32 DEVICE tensor (the fast path: no argument handling, the
    launches go to torch's current stream) under torch.cuda.stream(side): once that stream has drained, info["traffic"] matches the
    reference on the state, and everything — outputs, traffic, state — equals a twin env's numpy-actions path bit for bit."""
    import torch
    from atc_hip.vec_env import AtcVecEnv
    kw = dict(scenario=_sector()[0], auto_reset=True, spawn="lattice", grid_cell=0.5, traffic=4, timestep_limit=7, sep_nm=0.05, seed=2,
              want_raw_obs=True, want_term_obs=True)
    env, twin = AtcVecEnv(37, 16, **kw), AtcVecEnv(37, 16, **kw)
    side = torch.cuda.Stream(device=env.device)
    rng = np.random.default_rng(12)
    dones = 0
    for t in range(10):
        a = rng.uniform(-1, 1, (37, 16, 3)).astype(np.float32)
        at = torch.as_tensor(a, device=env.device)
        assert at.is_cuda and at.is_contiguous() and at.dtype is torch.float32
        side.wait_stream(torch.cuda.current_stream(env.device))     # the tensor was filled on the current stream
        skip = t % 3 == 2
        with torch.cuda.stream(side):
            obs, rew, done, info = env.step_skip(at, 4) if skip else env.step(at, held=False)
        side.synchronize()
        assert info["traffic"] is env.traffic
        _check_env_traffic(env, info["traffic"], "fast path %s %d" % ("step_skip" if skip else "step", t))
        o2, r2, d2, i2 = twin.step_skip(a, 4) if skip else twin.step(a)
        twin.synchronize()
        assert torch.equal(obs, o2) and torch.equal(rew, r2) and torch.equal(done, d2), t
        assert set(info) == set(i2)
        for k in info:
            assert torch.equal(info[k], i2[k]), (t, k)
        for k in ("ac", "alt", "last_act", "env", "stats", "phi_wide"):
            assert torch.equal(getattr(env, k), getattr(twin, k)), (t, k)
        dones += int(done.sum())
    assert dones > 0
    env.close()
    twin.close()
