"""The fill-phase prefetch of the fast single-step launch (csrc/atc_step.hip: ATC_FILL_PREFETCH) changes no result.

Batches sit just around the point where the prefetch switches on — a grid of more workgroups than the device holds at once, a number
the library reports (atc_fill_prefetch_info: the runtime's occupancy x CUs, rounded down to a multiple of 8) — on LOWW with random
entry points, 25 single steps each: one fresh action block, then held launches, auto-reset on (a time limit of 10 steps resets
every env twice).  Every case is compared
  * bit for bit — obs, reward, done, flags of every step, the final ac / alt / last_act / env / stats records — with the same
    library run with ATC_NO_FILL_PREFETCH=1 in a fresh child process (the knob is read once per process), and
  * on its first and last 256 envs with the fp32 oracle at the project's bars: integers exact, obs / reward within 1e-5 (lattice
    spawn does not depend on the env's index, so a 512-env oracle fed those envs' actions is their reference)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H  # noqa: F401  (sys.path)
import fill_prefetch_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _resident(N):
    from atc_hip import lib
    from envs.atc import scenarios
    key = ("fill_prefetch", N)
    if key not in H._compiled:
        sector = lib.Scenario(scenarios.compile_scenario(scenarios.LOWW(random_entrypoints=True), grid_cell=W.GRID_CELL))
        H._compiled[key] = lib.fill_prefetch_info(sector, 256, N)[0]
        sector.close()
    return H._compiled[key]


def _cases():
    """name -> (N, workgroups, seed, prefetch expected on)"""
    r16, r8 = _resident(16), _resident(8)
    assert r16 >= 8 and r16 % 8 == 0 and r8 >= 8 and r8 % 8 == 0
    return {"one workgroup more than resident": (16, r16 + 1, 11, True),
            "two rounds less one": (16, 2 * r16 - 1, 12, True),
            "count not a multiple of 8": (16, r16 + 13, 13, True),
            "8 aircraft": (8, r8 + 5, 14, True),
            "exactly resident: off": (16, r16, 15, False)}


@pytest.fixture(scope="module")
def knob_off():
    """Every case in ONE fresh child process with the prefetch switched off."""
    import tempfile
    cases = _cases()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "off.json")
        env = dict(os.environ, ATC_NO_FILL_PREFETCH="1")
        subprocess.run([sys.executable, os.path.join(HERE, "fill_prefetch_worker.py"), out] +
                       ["%d:%d:%d" % c[:3] for c in cases.values()], check=True, env=env, timeout=600)
        res = json.load(open(out))
    return {name: res["%d:%d:%d" % c[:3]] for name, c in cases.items()}


@pytest.mark.parametrize("name", ["one workgroup more than resident", "two rounds less one", "count not a multiple of 8", "8 aircraft",
                                  "exactly resident: off"])
def test_prefetch_changes_nothing(name, knob_off):
    from envs.atc import scenarios
    from oracle import oracle as O
    N, wgs, seed, on = _cases()[name]
    assert "ATC_NO_FILL_PREFETCH" not in os.environ
    got = W.run_case(N, wgs, seed, keep_edges=True)
    off = knob_off[name]
    B = wgs * 256 // N
    print("%s: %d x %d, %d workgroups, resident %d, stride %d (knob off: %d)" % (name, B, N, wgs, got["resident"], got["stride"], off["stride"]))
    assert got["launches"] == off["launches"] == W.STEPS, "the case did not run the fast all-valid single-step kernel"
    assert off["stride"] == 0 and off["resident"] == got["resident"]
    assert got["stride"] == (got["resident"] if on else 0) and (wgs > got["resident"]) == on
    for t in range(W.STEPS):
        assert got["steps"][t] == off["steps"][t], ("obs / reward / done / flags differ from the knob-off run", t)
    assert got["state"] == off["state"], "final ac / alt / last_act / env / stats differ from the knob-off run"
    # the batch's two ends against the fp32 oracle
    comp = scenarios.compile_scenario(scenarios.LOWW(random_entrypoints=True), grid_cell=W.GRID_CELL)
    a = W.actions_for(N, B, seed)
    a = np.concatenate([a[:W.EDGE], a[B - W.EDGE:]])
    orc = O.OracleEnv(comp, 2 * W.EDGE, N, O.make_params(auto_reset=True, seed=seed, timestep_limit=W.TIME_LIMIT), np.float32)
    n_done = 0
    for t in range(W.STEPS):
        orc.step(a)
        obs, rew, done, flags = got["edges"][t]
        assert np.array_equal(flags.astype(np.uint16), orc.flags), ("flags", t)
        assert np.array_equal(done, orc.done), ("done", t)
        o = obs.reshape(2 * W.EDGE, N, 10)
        assert np.all(np.abs(o - orc.obs) <= 1e-5 * np.maximum(1.0, np.abs(orc.obs))), ("obs", t)
        assert np.all(np.abs(rew - orc.reward) <= 1e-5 * np.maximum(1.0, np.abs(orc.reward)) + 6e-8 * N * np.abs(orc.ac_reward).sum(1)), ("reward", t)
        n_done += int(orc.done.sum())
    assert np.array_equal(got["edge_actions_taken"], orc.actions_taken)
    assert n_done >= 2 * 2 * W.EDGE, "the envs were not auto-reset inside the case"
