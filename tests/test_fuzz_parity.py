"""Randomised differential test of the HIP step path against the fp32 oracle: random batch shapes, aircraft counts,
sectors, lookup-grid cells, modes (dt, discrete, shaping, normalisation, spawn, timeout limit, separation minimum),
kernel variant (fast / full), launch form (single steps / fused rollout / fused rollout with held action blocks), one case in 50
no reset at all and, one in 25 of those with a power-of-two aircraft count, a batch just above the latency-bound limit of the device.
Every case prints the kernel instantiations it launched (the library's launch record).  ATC_FUZZ_CASES sets the number of cases
(default: a short pass), ATC_FUZZ_SEED the first seed; every case is reproducible from its seed
(the draw is tests/fuzz_space.py::parity_case; tests/fuzz_debug.py <seed> flies exactly that case again and prints the first
deviation with its context).

Since ABI 11 the fp32 spec (include/atc_step.h: fixed-point position grid, shared heading kinematics) makes the aircraft
state of the HIP path BIT-IDENTICAL to the fp32 oracle's, so flags / done / counters agree structurally, not statistically:
the round-1 knife-edge case (seed 52960: an aircraft within one fp32 ulp of a vertical MVA border binned on different
sides because the two float64 positions differed by 4e-8 nm) cannot occur any more.  The default run does 200 cases; a
sweep of 10 000 cases is recorded in profiles/ (see profiles/README.md)."""
import os

import pytest

import helpers as H
from fuzz_space import parity_case, run_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [int(os.environ.get("ATC_FUZZ_SEED", "1000")) + i
                                  for i in range(int(os.environ.get("ATC_FUZZ_CASES", "200")))])
def test_random_configuration_matches_oracle(seed):
    scn, comp, kw = parity_case(seed)
    print("fuzz case", seed, type(scn).__name__, kw)
    with H.launches() as got:
        run_vs_oracle(scn, comp, **kw)
    print("fuzz case", seed, "launched", got)
    W = H.lane_width(kw["N"])
    assert got and all(name.startswith("%d/" % W) for name in got), got
