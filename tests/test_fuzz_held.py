"""Randomised differential test of the held-block kernels (k_skip, k_lookahead, k_plan) and k_traffic against the fp32 oracle over
the mode space tests/test_fuzz_parity.py sweeps for k_step: sectors, lookup grids (none / 0.25 / 0.5 / 1.0 / the shipped 0.125 / "auto"),
dyadic and non-dyadic timesteps, discrete actions, shaping, normalisation, separation minimum 0 / 3 / 5, keep_active, time limits that
end episodes inside held blocks, actions far outside the action space, auto-reset switched off after flying.  tests/held_fuzz.py draws
and flies the cases; every comparison is one of tests/bars.py.

GPU: ATC_HELD_FUZZ_CASES cases (default 60) from seed ATC_HELD_FUZZ_SEED (default 5000) on; each prints its configuration and the launch
records it moved (tools/held_fuzz_summary.py summarises the `-s` logs of a wider sweep).  tests/fuzz_debug.py --held <seed> replays one.
CPU: the default sweep flown on the oracle alone must contain what it is for — every (kernel, property) pair, the events inside held
blocks for each kernel, and at most a tenth of its (candidate, env) pairs left out as WIDE; one small oracle-only run per sector."""
import functools
import os

import pytest

import helpers as H
import held_fuzz as F

SEED0 = int(os.environ.get("ATC_HELD_FUZZ_SEED", "5000"))
CASES = int(os.environ.get("ATC_HELD_FUZZ_CASES", "60"))
DEFAULT_SEEDS = range(5000, 5060)
PROPERTIES = ("discrete actions", "no lookup grid", "0.125 nm grid", "non-dyadic dt", "shaping off", "sep_nm 0", "keep_active",
              "auto-reset off", "SimpleScenario") + tuple("W=%d" % w for w in F.WIDTHS)
# what each kernel must have met inside its held blocks somewhere in the sweep (held_fuzz.run's event names)
EVENTS = {"skip": ("early", "reset_in_block", "conflict", "refused_repeated"),
          "lookahead": ("early", "differ", "reset_in_block", "conflict", "refused_repeated"),
          "plan": ("early", "differ", "reset_in_block", "conflict", "refused_repeated", "late_stop", "late_reset")}
WIDE_CAP = 0.10


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [SEED0 + i for i in range(CASES)])
def test_random_held_calls_match_oracle(seed):
    scn, comp, kw = F.case(seed)
    print("held fuzz case", seed, type(scn).__name__, kw)
    rec = F.run(seed, device=True)
    got = rec["launches"]
    print("held fuzz case", seed, "launched", got)
    W = H.lane_width(kw["N"])
    assert all(name.startswith("%d/" % W) for name in got.get("step", {})), got
    n_skip = len(kw["flown"]) + 1
    assert got["skip"] == {W: n_skip} and got["lookahead"] == {W: 1} and got["plan"] == {W: 1}, got
    # (an env with the traffic observation launches it after its reset and every frame-skip call, and once for observe_traffic)
    assert got.get("traffic", {}) == ({W: n_skip + 2} if kw["traffic"] else {}), got


@functools.lru_cache(maxsize=None)
def _oracle_record(seed):
    return F.run(seed, device=False)


def test_default_sweep_contains_what_it_is_for():
    recs = [_oracle_record(seed) for seed in DEFAULT_SEEDS]
    seen = {(k, p) for r in recs for k in F.KERNELS if r["events"][k]["pairs"] for p in r["props"]}
    missing = [(k, p) for k in F.KERNELS for p in PROPERTIES if (k, p) not in seen]
    assert not missing, missing
    for kernel, names in EVENTS.items():
        total = {n: sum(r["events"][kernel][n] for r in recs) for n in names}
        print(kernel, total)
        assert all(total.values()), (kernel, total)
    for kernel in ("lookahead", "plan"):
        excluded, pairs = (sum(r["wide"][kernel][i] for r in recs) for i in (0, 1))
        print(kernel, "pairs excluded as WIDE: %d of %d" % (excluded, pairs))
        assert excluded <= WIDE_CAP * pairs, (kernel, excluded, pairs)
        assert excluded > 0, "no WIDE env in the sweep: the not-evaluated path is not exercised"
        for r in recs:
            assert r["wide"][kernel][0] < r["wide"][kernel][1], ("every pair of a case excluded", r["seed"], kernel)
    assert any(r["traffic_short"] for r in recs), "no aircraft with fewer than K others under control"


def _first_seed_of(sector):
    for seed in DEFAULT_SEEDS:
        scn = F.case(seed)[0]
        name = type(scn).__name__ + ("_random" if type(scn).__name__ == "LOWW" and len(scn.entrypoints) > 1 else "")
        if name == sector:
            return seed
    raise AssertionError("the default sweep has no case on " + sector)


@pytest.mark.parametrize("sector", ["LOWW", "LOWW_random", "SimpleScenario", "LOWWDense"])
def test_harness_runs_on_the_oracle_alone(sector):
    """the harness itself, without a GPU: the first default case on each drawn sector flies, and its record is consistent"""
    rec = _oracle_record(_first_seed_of(sector))
    kw = rec["kw"]
    assert "launches" not in rec
    ev = rec["events"]
    assert ev["skip"]["pairs"] == kw["B"] * (len(kw["flown"]) + 1)
    for kernel in ("lookahead", "plan"):
        excluded, pairs = rec["wide"][kernel]
        assert pairs == kw[kernel]["M"] * kw["B"] and ev[kernel]["pairs"] == pairs - excluded
        limit = kw[kernel]["K"] * kw[kernel].get("H", 1)
        assert sum(ev[kernel]["n_hist"].values()) == ev[kernel]["pairs"] and all(1 <= n <= limit for n in ev[kernel]["n_hist"])
        assert ev[kernel]["early"] == sum(c for n, c in ev[kernel]["n_hist"].items() if n < limit)
