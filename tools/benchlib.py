"""What tools/frame_skip_bench.py, lookahead_bench.py, plan_bench.py and traffic_bench.py share: the command line, the library
choice and GPU check, the alternating sampler, the records of a measurement and the JSON writer.  Importing it (and a tool's
--help) needs neither torch nor a GPU; it puts the package on sys.path for the tools."""
import argparse
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "atc-reinforcement-learning_amd")]

WARMUP = 2   # rounds of every variant before the first kept sample


def parser(out_name, inner=None, quick=None):
    """--out (default profiles/<out_name>), --samples, --lib; --inner with that default and --quick with that help where given"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
    ap.add_argument("--samples", type=int, default=15)
    if inner:
        ap.add_argument("--inner", type=int, default=inner)
    if quick:
        ap.add_argument("--quick", action="store_true", help=quick)
    ap.add_argument("--lib", help="a build variant of libatcstep.so to measure instead of the in-tree one (A/B runs)")
    return ap


def start(a, tool):
    """Names the --lib variant before the first load, then imports torch and ends the run where there is no GPU; returns torch."""
    if a.lib:
        from atc_hip import lib as _lib
        _lib.use_library(a.lib)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("%s needs the GPU: nothing is measured without one" % tool)
    return torch


def same_work_actions(rng, shape):
    """The "same work" action family, [*shape, 3] float32: speed towards 150-200 kt, altitude towards 30 000 ft and up, any heading
    (from a reset, almost no episode ends within 60 steps of it)"""
    return np.stack([rng.uniform(-0.5, 0.0, shape), rng.uniform(0.6, 1.0, shape), rng.uniform(-1.0, 1.0, shape)], axis=-1).astype(np.float32)


def hip_clock(torch, stream):
    """clock(run) for sample(): the device time of run() in us, HIP events on `stream` around it"""
    def clock(run):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        run()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0
    return clock


def sample(calls, samples, inner, clock, prepare=None, after=None):
    """The variants of `calls` ({name: fn()}) take turns sample by sample; a sample is clock's time of `inner` calls back to back,
    divided by inner.  prepare(name) runs before every sample, outside the clock; after(name) behind every KEPT sample (the n_steps
    means).  The first WARMUP rounds of every variant are dropped.  Returns {name: [`samples` times]}."""
    times = {v: [] for v in calls}

    def burst(fn):
        for _ in range(inner):
            fn()
    for s in range(-WARMUP, samples):
        for v, fn in calls.items():
            if prepare:
                prepare(v)
            t = clock(lambda: burst(fn)) / inner
            if s >= 0:
                times[v].append(t)
                if after:
                    after(v)
    return times


def quartiles(t):
    q1, med, q3 = (float(x) for x in np.percentile(t, (25, 50, 75)))
    return {"median": med, "q1": q1, "q3": q3, "min": float(min(t)), "max": float(max(t))}


def box(torch):
    return {"host": socket.gethostname(), "device": torch.cuda.get_device_name(0),
            "cus": torch.cuda.get_device_properties(0).multi_processor_count, "torch": torch.__version__}


def write_json(path, doc):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(path)
