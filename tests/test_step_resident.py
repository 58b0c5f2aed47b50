"""The residency cap of the fast single-step launch (csrc/atc_step.hip: step_residency, ATC_STEP_RESIDENT) changes no result.

A cap of k workgroups per CU is made with padding in the launch's dynamic LDS request; the fill-phase prefetch stride follows it.
For k in {4, 5, 6} the library, in a fresh child process with ATC_STEP_RESIDENT=k (the knob is read once per process), must report
a residency of r_k = (k x CUs) & ~7.  Batches sit around the points where the pad and the prefetch switch on — on LOWW with random
entry points, the worker's 25 single steps each: one fresh action block, then held launches, auto-reset on (a time limit of 10
steps resets every env twice).  Every case is compared
  * bit for bit — obs, reward, done, flags of every step, the final ac / alt / last_act / env / stats records — with the same
    library run with ATC_STEP_RESIDENT=0 (no padding) in another child process, and
  * on its first and last 256 envs with the fp32 oracle at the project's bars: integers exact, obs / reward within 1e-5.

    python test_step_resident.py OUT.pkl K       (the capped side: this file run as a child process)"""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import fill_prefetch_worker as W

pytestmark = pytest.mark.gpu
CAPS = (4, 5, 6)
NAMES = ("one workgroup more than resident", "two rounds less one", "count not a multiple of 8", "8 aircraft", "exactly resident: off")


def cases_for(k, r16, r8):
    """name -> (N, workgroups, seed, pad and prefetch expected on)"""
    return {"one workgroup more than resident": (16, r16 + 1, 100 + k, True),
            "two rounds less one": (16, 2 * r16 - 1, 110 + k, True),
            "count not a multiple of 8": (16, r16 + 13, 120 + k, True),
            "8 aircraft": (8, r8 + 5, 130 + k, True),
            "exactly resident: off": (16, r16, 140 + k, False)}


def _child_main(out, k):
    """ATC_STEP_RESIDENT=k is in the environment: the residency the library reports, then every case with its edges kept."""
    from atc_hip import lib
    from envs.atc import scenarios
    assert os.environ.get("ATC_STEP_RESIDENT") == str(k)
    sector = lib.Scenario(scenarios.compile_scenario(scenarios.LOWW(random_entrypoints=True), grid_cell=W.GRID_CELL))
    r16, r8 = lib.fill_prefetch_info(sector, 256, 16)[0], lib.fill_prefetch_info(sector, 256, 8)[0]
    sector.close()
    res = {"r16": r16, "r8": r8, "cases": {}}
    if r16 >= 8 and r8 >= 8:
        for name, (N, wgs, seed, _) in cases_for(k, r16, r8).items():
            res["cases"][name] = W.run_case(N, wgs, seed, keep_edges=True)
    with open(out, "wb") as f:
        pickle.dump(res, f)


@pytest.fixture(scope="module")
def capped():
    """k -> what a fresh child process with ATC_STEP_RESIDENT=k reported and computed."""
    import tempfile
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k in CAPS:
            out = os.path.join(tmp, "k%d.pkl" % k)
            subprocess.run([sys.executable, os.path.abspath(__file__), out, str(k)], check=True,
                           env=dict(os.environ, ATC_STEP_RESIDENT=str(k)), timeout=600)
            with open(out, "rb") as f:
                res[k] = pickle.load(f)
    return res


@pytest.fixture(scope="module")
def uncapped(capped):
    """(k, name) -> the worker's digests of the same case, from ONE fresh child process with ATC_STEP_RESIDENT=0."""
    import tempfile
    specs = {(k, name): "%d:%d:%d" % c[:3] for k in CAPS for name, c in cases_for(k, capped[k]["r16"], capped[k]["r8"]).items()}
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k0.json")
        subprocess.run([sys.executable, os.path.join(HERE, "fill_prefetch_worker.py"), out] + sorted(set(specs.values())), check=True,
                       env=dict(os.environ, ATC_STEP_RESIDENT="0"), timeout=600)
        res = json.load(open(out))
    return {key: res[spec] for key, spec in specs.items()}


@pytest.mark.parametrize("k", CAPS)
def test_reported_residency(k, capped):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("ATC_STEP_RESIDENT=%d: resident %d (16 aircraft), %d (8 aircraft); %d CUs" % (k, capped[k]["r16"], capped[k]["r8"], cus))
    assert capped[k]["r16"] == (k * cus) & ~7
    assert capped[k]["r8"] == (k * cus) & ~7


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("k", CAPS)
def test_cap_changes_nothing(k, name, capped, uncapped):
    from envs.atc import scenarios
    from oracle import oracle as O
    assert "ATC_NO_FILL_PREFETCH" not in os.environ
    r16, r8 = capped[k]["r16"], capped[k]["r8"]
    N, wgs, seed, on = cases_for(k, r16, r8)[name]
    r_k = r16 if N == 16 else r8
    got, off = capped[k]["cases"][name], uncapped[(k, name)]
    B = wgs * 256 // N
    print("k = %d, %s: %d x %d, %d workgroups, resident %d, stride %d (uncapped: resident %d, stride %d)"
          % (k, name, B, N, wgs, got["resident"], got["stride"], off["resident"], off["stride"]))
    assert got["launches"] == off["launches"] == W.STEPS, "the case did not run the fast all-valid single-step kernel"
    assert got["resident"] == r_k and got["stride"] == (r_k if on else 0) and (wgs > r_k) == on
    assert off["resident"] > r_k and off["stride"] == (off["resident"] if wgs > off["resident"] else 0)
    for t in range(W.STEPS):
        assert got["steps"][t] == off["steps"][t], ("obs / reward / done / flags differ from the uncapped run", t)
    assert got["state"] == off["state"], "final ac / alt / last_act / env / stats differ from the uncapped run"
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


if __name__ == "__main__":
    _child_main(sys.argv[1], int(sys.argv[2]))
