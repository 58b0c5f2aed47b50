"""State gather (include/atc_step.h: atc_state_select; AtcVecEnv.select): dst env e takes src env index[e]'s rows.

CPU: the refusal order through ctypes with NULL and made-up pointer values.
GPU: against torch indexing of the six state tensors, byte for byte — every width, B_dst != B_src, repeated, negative and too-large
indices, the mask, sentinel rows untouched, the side records of WIDE aircraft, the overlap refusal, the launch records."""
import ctypes as C

import numpy as np
import pytest

import branch_ref as BR
import held_tools as T
import helpers as H
from atc_hip import layout as L


def test_select_refusal_order_without_a_gpu():
    from atc_hip import lib
    h = lib.load()
    err = h.atc_last_error
    src, end = BR.fake_state(0x20000000, 5, 3, lib)
    dst, _ = BR.fake_state(end, 7, 3, lib)
    call = lambda N, Bd, Bs, d=dst, s=src, idx=0x1000: h.atc_state_select(None, N, Bd, C.byref(d) if d else None, Bs, C.byref(s) if s else None, idx, None, None)   # noqa: E731
    for N, Bd, Bs in ((0, 7, 5), (65, 7, 5), (3, 0, 5), (3, 7, 0), (3, -1, 5)):
        assert h.atc_state_select(None, N, Bd, None, Bs, None, None, None, None) == -1 and b"B_dst" in err()    # the shape before any pointer
    assert call(3, 7, 5, idx=None) == -1 and b"null" in err()
    assert call(3, 7, 5, d=None) == -1 and b"null" in err()
    assert call(3, 7, 5, s=None) == -1 and b"null" in err()
    hole = lib.AtcState(*[getattr(src, n) for n in lib.STATE_FIELDS])
    hole.phi_wide = None
    assert call(3, 7, 5, s=hole) == -1 and b"null" in err()
    for field in lib.STATE_FIELDS:
        over = lib.AtcState(*[getattr(dst, n) for n in lib.STATE_FIELDS])
        setattr(over, field, src.stats + 5 * 32 - 1)
        assert call(3, 7, 5, d=over) == -1 and b"overlaps" in err(), field
    assert call(3, 7, 5) == -1 and b"overlaps" not in err() and b"null" in err()     # disjoint: only the scenario is missing
    buf = (C.c_uint64 * L.SELECT_LAUNCH_SLOTS)()
    assert h.atc_select_launch_counts(buf, L.SELECT_LAUNCH_SLOTS) == 0 and isinstance(lib.select_launch_counts(), dict)


def _expected(dst, src, idx, mask, N, B_src):
    """torch indexing of the six tensors; phi_wide rows only for aircraft with a saturated field (the others keep dst's bytes)"""
    import torch
    ok = (idx >= 0) & (idx < B_src)
    if mask is not None:
        ok &= mask != 0
    rows = idx.clamp(0, B_src - 1).long()
    ac_rows = (rows[:, None] * N + torch.arange(N)).reshape(-1)
    ok_ac = ok.repeat_interleave(N)
    want = {}
    for k in H.STATE:
        per_env = k in ("env", "stats")
        g = src[k][rows if per_env else ac_rows]
        o = ok if per_env else ok_ac
        if k == "phi_wide":
            o = o & BR.saturated({"ac": src["ac"][ac_rows], "last_act": src["last_act"][ac_rows]})
        want[k] = torch.where(o.view(-1, *([1] * (g.dim() - 1))), g, dst[k])
    return want


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("N", [1, 2, 3, 8, 16, 32, 33, 64])
def test_select_equals_torch_indexing(N):
    import torch
    from atc_hip import lib
    rng = np.random.default_rng(500 + N)
    B_src, B_dst = T.look_ragged(N), T.look_ragged(N) + 5
    src = T.look_env(N, B_src, "lattice", True)
    T.look_fly(src, rng, steps=40)
    src.set_state(B_src - 1, N - 1, *H.FAR_B[:3], 500.0, H.FAR_B[4])     # a WIDE heading: its side record travels
    src.set_last_action(1, 0, [250.0, 9000.0, -400.0])                    # a WIDE last heading target
    src.synchronize()
    s_cpu = {k: getattr(src, k).cpu() for k in H.STATE}
    assert int(BR.saturated(s_cpu).sum()) == 2
    idx = torch.as_tensor(rng.integers(0, B_src, B_dst), dtype=torch.int32)
    idx[0], idx[1], idx[2], idx[3], idx[4] = B_src - 1, B_src - 1, 1, -1, B_src       # repeats, the WIDE envs, negative, too large
    idx[5] = -2 ** 31
    mask = torch.as_tensor(rng.integers(0, 2, B_dst), dtype=torch.uint8)
    mask[:6] = 1
    mask[6] = 0
    snap = H.snapshot(src)
    for m in (None, mask):
        st = BR.sentinel_state(B_dst + 2 * BR.GUARD, N, src.device)
        per = {k: (1 if k in ("env", "stats") else N) for k in H.STATE}
        dst = lib.AtcState(*[st[k][BR.GUARD * per[k]:].data_ptr() for k in lib.STATE_FIELDS])
        before_cpu = {k: v.cpu() for k, v in st.items()}
        before = (lib.select_launch_counts(), lib.branch_launch_counts(), lib.launch_counts(), lib.skip_launch_counts())
        d_idx, d_mask = idx.to(src.device), (m.to(src.device) if m is not None else None)
        lib.check(lib.load().atc_state_select(src.sector.handle, N, B_dst, C.byref(dst), B_src, C.byref(src._state), d_idx.data_ptr(),
                                              d_mask.data_ptr() if m is not None else None, torch.cuda.current_stream().cuda_stream))
        src.synchronize()
        assert lib.select_launch_counts().get("select", 0) == before[0].get("select", 0) + 1
        assert (lib.branch_launch_counts(), lib.launch_counts(), lib.skip_launch_counts()) == before[1:]
        inner = {k: before_cpu[k][BR.GUARD * per[k]:(BR.GUARD + B_dst) * per[k]] for k in H.STATE}
        want = _expected(inner, s_cpu, idx, m, N, B_src)
        for k in H.STATE:
            full = before_cpu[k].clone()
            full[BR.GUARD * per[k]:(BR.GUARD + B_dst) * per[k]] = want[k]
            assert torch.equal(st[k].cpu().contiguous().view(torch.uint8), full.contiguous().view(torch.uint8)), (k, m is not None)
        H.bytes_equal(src, snap)
    # the overlap refusal on real tensors: dst = src
    rc = lib.load().atc_state_select(src.sector.handle, N, B_src, C.byref(src._state), B_src, C.byref(src._state), d_idx.data_ptr(), None, None)
    assert rc == -1 and b"overlaps" in lib.load().atc_last_error()
    src.close()


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_python_select_gathers_obs_and_refuses_strangers():
    import torch
    N = 16
    rng = np.random.default_rng(9)
    a, b = T.look_env(N, 20, "lattice", True), T.look_env(N, 33, "lattice", True)
    T.look_fly(b, rng, steps=40)
    b.step(torch.as_tensor(T.look_draw(rng, 33, N), device=b.device))
    idx = torch.as_tensor(rng.integers(0, 33, 20), device=a.device)
    assert idx.dtype == torch.int64
    idx[3] = -1
    idx[7] = 2 ** 32 + 3      # int64: beyond 32 bits, not env 3
    mask = np.ones(20, np.uint8)
    mask[5] = 0
    keep = {k: getattr(a, k).clone() for k in H.STATE + ("obs",)}
    a.select(b, idx, mask=mask)
    for e in range(20):
        j = int(idx[e])
        for k in ("ac", "alt", "last_act", "env", "stats", "obs"):
            per = 1 if k in ("env", "stats", "obs") else N
            mine = getattr(a, k)[e * per:(e + 1) * per]
            want = keep[k][e * per:(e + 1) * per] if (e in (3, 5, 7)) else getattr(b, k)[j * per:(j + 1) * per]
            assert torch.equal(mine.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), (e, k)
    other = T.look_env(N, 20, "lattice", False)          # other parameters (normalisation)
    fewer = T.look_env(8, 20, "lattice", True)
    for bad in (other, fewer):
        with pytest.raises(ValueError):
            a.select(bad, idx)
        with pytest.raises(ValueError):
            a.branch(torch.zeros((1, 20, N, 3)), 2, into=bad)
    with pytest.raises(ValueError):
        a.branch(torch.zeros((2, 20, N, 3)), 2, into=b)       # 33 != 2 * 20
    with pytest.raises(ValueError):
        a.select(b, idx[:5])
    with pytest.raises(ValueError):
        a.select(b, idx.float())
    for e in (a, b, other, fewer):
        e.close()
