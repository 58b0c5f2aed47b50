"""The fuzz draws are pinned: seed -> case and seed -> actions must not move, or the sweeps recorded under profiles/ (*fuzz*.txt,
ref_diff_sweep.txt) name cases that no longer exist and a failing seed cannot be flown again.  No GPU."""
import hashlib

import numpy as np

import fuzz_space as S
import held_fuzz as F
import ref_diff as D

# Taken on the parent of the commit that gathered the draws in tests/fuzz_space.py, from the copies they had then
# (test_fuzz_parity._case, the draw inside test_hip_parity._run_vs_oracle, held_fuzz.draw_actions, ref_diff.draw_actions).
DIGEST = "2891ad724bf2e2107ca951e1c148937d66faf39c8badb036ded109c728bd779b"


def test_case_and_action_draws_are_what_they_were():
    """Per seed 1000 .. 1039: the case kw of test_fuzz_parity with the scenario's class, the first two action blocks of run_vs_oracle's
    stream for it (B capped at 64), and kw and first drawn block of held_fuzz.case and ref_diff.case."""
    h = hashlib.sha256()

    def put(scn, kw):
        h.update(repr((type(scn).__name__, sorted(kw.items()))).encode())

    for seed in range(1000, 1040):
        scn, comp, kw = S.parity_case(seed, n_cu=256)
        put(scn, kw)
        rng = np.random.default_rng(kw["seed"])
        for _ in range(2):
            h.update(S.draw_actions(rng, (min(kw["B"], 64), kw["N"]), kw["discrete"], kw.get("wild", 0.0), True).tobytes())
        scn, comp, kw = F.case(seed)
        put(scn, kw)
        rng = np.random.default_rng([kw["seed"], 0x464C59])
        h.update(F.draw_flown(rng, kw["B"], kw["N"], kw["discrete"], kw["wild"]).tobytes())
        scn, comp, kw = D.case(seed)
        put(scn, kw)
        rng = np.random.default_rng(seed)
        h.update(S.draw_actions(rng, (kw["B"], kw["N"]), kw["discrete"], kw.get("wild", 0.0), True).tobytes())
    assert h.hexdigest() == DIGEST
