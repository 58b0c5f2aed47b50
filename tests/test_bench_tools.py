"""tools/benchlib.py and the four bench tools built on it (frame_skip, lookahead, plan, traffic): the records and the sampling
order, on the CPU — plain callables and an injected clock stand in for the launches and the HIP events."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
BENCH_TOOLS = ("frame_skip_bench", "lookahead_bench", "plan_bench", "traffic_bench")


def load_tool(name, monkeypatch):
    monkeypatch.syspath_prepend(TOOLS)   # the tools import benchlib as a script next to it would
    spec = importlib.util.spec_from_file_location("_tool_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_quartile_record(monkeypatch):
    benchlib = load_tool("benchlib", monkeypatch)
    t = [7.5, 1.0, 12.25, 3.0, 9.0, 2.5, 30.0]
    rec = benchlib.quartiles(t)
    q1, med, q3 = np.percentile(t, (25, 50, 75))
    assert rec == {"median": med, "q1": q1, "q3": q3, "min": 1.0, "max": 30.0}
    assert list(rec) == ["median", "q1", "q3", "min", "max"] and all(type(v) is float for v in rec.values())


@pytest.mark.parametrize("samples,inner", [(3, 2), (1, 1), (5, 4)])
def test_sampler_alternates_and_drops_two_warmup_rounds(monkeypatch, samples, inner):
    benchlib = load_tool("benchlib", monkeypatch)
    log, ticks = [], iter(range(1, 10 ** 6))
    calls = {v: (lambda v=v: log.append(("call", v))) for v in ("a", "b", "c")}

    def clock(run):   # sample n (counted over all variants, warm-up included) "takes" n * inner us
        log.append("t0")
        run()
        log.append("t1")
        return float(next(ticks) * inner)
    times = benchlib.sample(calls, samples, inner, clock, prepare=lambda v: log.append(("prepare", v)), after=lambda v: log.append(("after", v)))
    rounds = samples + 2
    # the variants take turns sample by sample; prepare runs outside the clock, `inner` calls inside it, after() behind kept samples only
    want = []
    for r in range(rounds):
        for v in ("a", "b", "c"):
            want += [("prepare", v), "t0"] + [("call", v)] * inner + ["t1"] + ([("after", v)] if r >= 2 else [])
    assert log == want
    # exactly the first two rounds are dropped, the kept times are per call (clock / inner), in order
    for k, v in enumerate(("a", "b", "c")):
        assert times[v] == [float(3 * r + k + 1) for r in range(2, rounds)] and len(times[v]) == samples
    assert list(times) == ["a", "b", "c"]


def test_sampler_without_hooks(monkeypatch):
    benchlib = load_tool("benchlib", monkeypatch)
    n = {"x": 0, "y": 0}
    times = benchlib.sample({v: (lambda v=v: n.__setitem__(v, n[v] + 1)) for v in n}, 4, 3, lambda run: (run(), 6.0)[1])
    assert times == {"x": [2.0] * 4, "y": [2.0] * 4} and n == {"x": 18, "y": 18}


def test_same_work_actions_draw(monkeypatch):
    """the one draw behind the three tools' action families: per component one uniform block, in the order speed, altitude, heading"""
    benchlib = load_tool("benchlib", monkeypatch)
    a = benchlib.same_work_actions(np.random.default_rng(11), (2, 3, 5))
    rng = np.random.default_rng(11)
    want = np.stack([rng.uniform(-0.5, 0.0, (2, 3, 5)), rng.uniform(0.6, 1.0, (2, 3, 5)), rng.uniform(-1.0, 1.0, (2, 3, 5))], axis=-1)
    assert a.dtype == np.float32 and a.shape == (2, 3, 5, 3) and np.array_equal(a, want.astype(np.float32))


@pytest.mark.parametrize("tool", BENCH_TOOLS)
def test_help_exits_zero(tool):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, tool + ".py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    for flag in ("--out", "--samples", "--lib"):
        assert flag in r.stdout


@pytest.mark.parametrize("tool", BENCH_TOOLS)
def test_imports_without_torch(tool, monkeypatch):
    """nothing reaches torch before main() has parsed its arguments"""
    monkeypatch.setitem(sys.modules, "torch", None)   # `import torch` now raises ImportError
    monkeypatch.delitem(sys.modules, "benchlib", raising=False)
    with pytest.raises(ImportError):
        import torch  # noqa: F401
    mod = load_tool(tool, monkeypatch)
    assert callable(mod.main) and callable(mod.measure)
