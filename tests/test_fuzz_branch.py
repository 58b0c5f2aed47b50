"""Randomised differential test of k_branch (atc_branch) against the fp32 oracle over the mode space of tests/test_fuzz_held.py: 40 cases
drawn and flown exactly as tests/held_fuzz.py draws and flies them (tests/branch_fuzz.py), the case's look-ahead draw flown as one
atc_branch into a child env; outputs and child state at the bars of tests/bars.py.

At most 1 % of the sweep's (candidate, env) pairs may be left out as not evaluated (WIDE at the start): the flown calls' heading
components take part in the out-of-space draw in a quarter of the envs only, never env 0.  The GPU test asserts the bound on what it
flew; the CPU twin flies the same 40 cases on the oracle alone and asserts the bound and that the cases contain an early stop, a reset
inside a block and a conflict."""
import functools

import pytest

import branch_fuzz as BF
import helpers as H

NOT_EVALUATED_CAP = 0.01


def _bound(recs, key="excluded"):
    excluded, pairs = sum(r[key] for r in recs), sum(r["pairs"] for r in recs)
    print("pairs not evaluated: %d of %d" % (excluded, pairs))
    assert pairs > 0 and excluded <= NOT_EVALUATED_CAP * pairs, (excluded, pairs)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_random_branches_match_oracle():
    recs = []
    for seed in BF.SEEDS:
        rec = BF.run(seed, device=True)
        print("branch fuzz case", seed, rec["kw"]["N"], rec["kw"]["B"], rec["kw"]["lookahead"], "launched", rec["launches"])
        assert rec["launches"] == {H.lane_width(rec["kw"]["N"]): 1}, rec["launches"]
        recs.append(rec)
    _bound(recs, "not_evaluated")     # the device's own count of pairs with n_steps == 0


@functools.lru_cache(maxsize=None)
def _oracle_records():
    return [BF.run(seed, device=False) for seed in BF.SEEDS]


def test_the_forty_cases_contain_what_they_are_for():
    recs = _oracle_records()
    assert len(recs) == 40
    _bound(recs)
    total = {n: sum(r["events"][n] for r in recs) for n in ("early", "reset_in_block", "conflict", "differ", "done")}
    print(total)
    assert total["early"] and total["reset_in_block"] and total["conflict"], total
    for r in recs:
        assert "launches" not in r and r["excluded"] < r["pairs"], r["seed"]
