#!/usr/bin/env python3
"""Summary of a held-fuzz sweep (tests/test_fuzz_held.py run with `-s`): reads the logs of its pytest invocations and prints the cases,
the mismatches, the property values the cases had and the launch records seen per kernel and lane-group width.
    python tools/held_fuzz_summary.py LOG [LOG ...]"""
import ast
import collections
import re
import sys

CASE = re.compile(r"held fuzz case (\d+) (\w+) (\{.*\})\s*$")
LAUNCHED = re.compile(r"held fuzz case (\d+) launched (\{.*\})\s*$")
TAIL = re.compile(r"(\d+ (?:passed|failed).*) in [\d.]+s")

cases, launched, tails, failed = {}, {}, [], []
for path in sys.argv[1:]:
    for line in open(path, errors="replace"):
        m = CASE.search(line)
        if m:
            cases[int(m.group(1))] = (m.group(2), ast.literal_eval(m.group(3)))
        m = LAUNCHED.search(line)
        if m:
            launched[int(m.group(1))] = ast.literal_eval(m.group(2))
        m = TAIL.search(line)
        if m:
            tails.append("%s: %s" % (path.split("/")[-1], m.group(0).strip("= ")))
        if line.startswith("FAILED "):
            failed.append(line.strip())

print("held-fuzz sweep: %d cases drawn, %d flown to the end, %d mismatches" % (len(cases), len(launched), len(failed)))
if cases:
    print("seeds %d .. %d" % (min(cases), max(cases)))
for t in tails:
    print("  " + t)
for f in failed:
    print("  " + f)
width = lambda N: 1 << max(0, (N - 1).bit_length())   # noqa: E731
props = collections.Counter()
for seed, (sector, kw) in cases.items():
    if seed not in launched:
        continue
    for name in ("sector " + sector, "grid_cell %s" % kw["grid_cell"], "dt %s" % kw["dt"], "discrete %s" % kw["discrete"], "shaping %s" % kw["shaping"],
                 "normalize %s" % kw["normalize"], "sep_nm %s" % kw["sep_nm"], "keep_active %s" % kw["keep_active"], "spawn " + kw["spawn"],
                 "timestep_limit %d" % kw["timestep_limit"], "auto_reset_off %s" % kw["auto_reset_off"], "wild %s" % kw["wild"],
                 "full %s" % kw["full"], "W %d" % width(kw["N"]), "lookahead outputs %s" % ("+".join(kw["lookahead"]["outputs"]) or "none"),
                 "plan outputs %s" % ("+".join(kw["plan"]["outputs"]) or "none"),
                 "lookahead M %d K %d" % (kw["lookahead"]["M"], kw["lookahead"]["K"]),
                 "plan M %d H %d K %d" % (kw["plan"]["M"], kw["plan"]["H"], kw["plan"]["K"])):
        props[name] += 1
print("\ncases per property value (every case flies step_skip, lookahead and lookahead_plan; observe_traffic at N > 1):")
for name in sorted(props):
    print("  %-50s %d" % (name, props[name]))
records = collections.defaultdict(collections.Counter)
for seed, got in launched.items():
    for kernel, by in got.items():
        for name, n in by.items():
            records[kernel][name] += n
print("\nlaunches per record (kernel) and lane-group width / instantiation, summed over the cases:")
for kernel in sorted(records):
    print("  %-10s %s" % (kernel, dict(sorted(records[kernel].items(), key=lambda kv: str(kv[0])))))
