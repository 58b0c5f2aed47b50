#!/usr/bin/env python3
"""Developer tool: anatomy of ONE held single-step launch (65 536 x 16 by default) from the per-wavefront stamps of the ATC_TRACE
build in mode 3 (stamp 0 wavefront start, 1 state arrived, 5 observation store begins, 7 last store issued).
  bash tools/build_variant.sh trace3 -DATC_TRACE=1 -DATC_TRACE_MODE=3 ; python tools/trace_fill.py [envs] [aircraft] [--json FILE]
Prints, per XCD-aligned 0.5 us bin: wavefronts started / waiting for their state loads / in arithmetic / storing / ended in the bin,
and the two derived times (launch start -> first bulk of stores, last workgroup's start -> kernel end)."""
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "atc-reinforcement-learning_amd")]
import numpy as np
import torch
from atc_hip import lib as _binding
_binding.use_library(os.environ.get("ATC_TRACE_LIB") or os.path.join(ROOT, "build_variants", "libatcstep_trace3.so"))
from atc_hip.vec_env import AtcVecEnv
from envs.atc import scenarios

argv = [a for a in sys.argv[1:]]
out_json = None
if "--json" in argv:
    k = argv.index("--json")
    out_json = argv[k + 1]
    del argv[k:k + 2]
B, N = (int(argv[0]) if len(argv) > 0 else 65536), (int(argv[1]) if len(argv) > 1 else 16)
BIN = 0.5
GHZ = float(os.environ.get("ATC_TRACE_GHZ", "2.1"))   # s_memtime counts shader-clock cycles (tools/trace_phases.py)
W = 1 << max(0, (N - 1).bit_length())
env = AtcVecEnv(B, N, scenario=scenarios.LOWW(random_entrypoints=N > 1), auto_reset=True)
resident, stride = _binding.fill_prefetch_info(env.sector, B, N)
acts = [(torch.rand((B, N, 3), device="cuda") * 2 - 1) for _ in range(4)]
for t in range(300):
    env.step(acts[(t // 20) % 4], held=t % 20 != 0)
n_waves = (B * W + 255) // 256 * 4
LAUNCHES = 5   # traced launches: the table is of the median one by kernel length, the derived times are given for all
rows = []
for rep in range(LAUNCHES):
    trace = torch.zeros((n_waves, 8), dtype=torch.int64, device="cuda")
    ptr = trace.data_ptr()
    env.params.reserved0 = ptr & 0xffffffff
    env.params.reserved1 = struct.unpack("f", struct.pack("I", (ptr >> 32) & 0xffffffff))[0]
    env.refresh_params()
    torch.cuda.synchronize()
    env.step(acts[rep % 4])               # first launch of a block (its stamps are overwritten)
    env.step(acts[rep % 4], held=True)    # the traced launch: a repeat
    torch.cuda.synchronize()
    rows.append(trace.cpu().numpy())

def domains(raw):
    """The stamps are per-XCD clocks that are not aligned with each other, and which workgroups share one is not assumed: rows whose
    start stamps lie within one launch length of each other form a clock domain (the clocks are milliseconds apart)."""
    order = np.argsort(raw[:, 0])
    gap = np.diff(raw[order, 0].astype(np.float64)) > 200.0 * GHZ * 1e3   # > 200 us: another clock
    dom = np.zeros(len(raw), np.int64)
    dom[order] = np.concatenate([[0], np.cumsum(gap)])
    return dom


def anatomy(raw):
    """Times in us from the first wavefront start of the row's clock domain; columns: start, state arrived, store begin, end."""
    global xcd
    xcd = domains(raw)
    t = np.zeros((n_waves, 4))
    for x in np.unique(xcd):
        m = xcd == x
        r = raw[m][:, [0, 1, 5, 7]].astype(np.float64)
        t[m] = (r - r[:, 0].min()) / (GHZ * 1e3)
    return t


def derived(t):
    length = t[:, 3].max()
    first_round = np.sort(t[:, 0])[: max(1, resident * 4 if resident else n_waves // 2)]
    fr = t[:, 0] <= first_round.max()
    bulk = float(np.percentile(t[fr, 2], 10))      # a tenth of the first round's wavefronts have begun to store
    # the last workgroup to start, per XCD (aligned clocks only inside one), to that XCD's last store issue: the largest
    tail = max(float(t[xcd == x, 3].max() - t[xcd == x, 0].max()) for x in np.unique(xcd))
    second = np.sort(t[:, 0])[min(len(t) - 1, len(first_round))]   # start of the first wavefront BEYOND the first round
    return {"clock_domains": int(len(np.unique(xcd))), "length_us": round(float(length), 2), "first_store_bulk_us": round(bulk, 2), "first_store_min_us": round(float(t[:, 2].min()), 2),
            "last_start_to_end_us": round(tail, 2), "first_round_started_by_us": round(float(first_round.max()), 2),
            "second_round_begins_us": round(float(second), 2), "state_wait_first_round_median_us": round(float(np.median((t[:, 1] - t[:, 0])[fr])), 2),
            "state_wait_later_median_us": round(float(np.median((t[:, 1] - t[:, 0])[~fr])), 2) if (~fr).any() else None}


good = [(r > 0).all(axis=1).all() and (np.diff(r[:, [0, 1, 5, 7]], axis=1) >= 0).all() for r in rows]
ts = [anatomy(r) for r in rows]
ds = [derived(t) for t in ts]
order = np.argsort([d["length_us"] for d in ds])
mid = int(order[len(order) // 2])
t = ts[mid]
table = []
for b in np.arange(0.0, min(t[:, 3].max(), 100.0) + BIN, BIN):
    m = b + BIN / 2
    table.append({"t_us": float(b),
                  "started": int(((t[:, 0] >= b) & (t[:, 0] < b + BIN)).sum()),
                  "load_wait": int(((t[:, 0] <= m) & (m < t[:, 1])).sum()),
                  "arithmetic": int(((t[:, 1] <= m) & (m < t[:, 2])).sum()),
                  "storing": int(((t[:, 2] <= m) & (m < t[:, 3])).sum()),
                  "ended": int(((t[:, 3] >= b) & (t[:, 3] < b + BIN)).sum())})
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
env.params.reserved0 = 0
env.params.reserved1 = 0.0
env.refresh_params()
ev0.record()
for k in range(200):
    env.step(acts[(k // 20) % 4], held=k % 20 != 0)
ev1.record()
torch.cuda.synchronize()
res = {"envs": B, "aircraft": N, "wavefronts": n_waves, "resident_workgroups": resident, "prefetch_stride": stride,
       "ghz_assumed": GHZ, "launch_to_launch_us_untraced": round(ev0.elapsed_time(ev1) / 200 * 1e3, 2),
       "rows_usable": [bool(g) for g in good], "derived_all_launches": ds, "table_of_launch": mid, "bin_us": BIN, "table": table}
print("launch %d of %d (median length); stride %d, resident %d; all launches:" % (mid, LAUNCHES, stride, resident))
for d in ds:
    print("  ", json.dumps(d))
print("%6s %8s %10s %11s %8s %6s" % ("t [us]", "started", "load wait", "arithmetic", "storing", "ended"))
for r in table:
    print("%6.1f %8d %10d %11d %8d %6d" % (r["t_us"], r["started"], r["load_wait"], r["arithmetic"], r["storing"], r["ended"]))
if out_json:
    np.save(os.path.splitext(out_json)[0] + "_stamps.npy", rows[mid])   # (git-ignored: the raw stamps of the tabulated launch)
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(res, f, indent=1)
