"""Developer measurement: what the traffic observation costs (traffic observation).

    python tools/traffic_bench.py [--out profiles/traffic_bench.json] [--samples 15] [--inner 10] [--lib VARIANT.so]

For 65 536 x 16 and 4 096 x 64 and K in {1, 2, 4, 8}, on the state a few hundred random steps leave behind:
  1. kernel   atc_observe_traffic(K)                      us per launch, and its bytes (24 read + 32 K written per aircraft) / time
                                                          against 8 TB/s
  2. step     atc_step of the same env, same run          the launch it would ride next to
  3. torch    the same records from stock torch ops on the same state tensors: fp32 positions, pairwise d2, masking, topk,
              gathers, the rotation into each aircraft's frame, one stacked [B, N, K, 8] result
A sample is the device time (HIP events) of `inner` launches back to back; the three take turns sample by sample after a warm-up;
medians and quartiles.  The kernel has to beat the torch composition at both shapes for K = 4 to be worth carrying: the file says
whether it does (`kernel_faster_than_torch_at_K4`).
Each shape is measured by a child process of its own under `timeout -k 10`, one after the other; the first that fails ends the run
(nothing more is started on the device).  One JSON file; needs the GPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

import benchlib

CONFIGS = ((65536, 16), (4096, 64))
KS = (1, 2, 4, 8)
HBM_BYTES_PER_S = 8.0e12
CHILD_SECONDS = 240


def torch_traffic(torch, env, K, scales):
    """the stock-torch composition (ties are broken however topk breaks them: a timing yardstick, not the reference)"""
    from atc_hip import layout as L
    B, N = env.B, env.N
    ac = env.ac.view(B, N, 4)
    x = (ac[..., 0].double() * 2.0 ** -env.pos_k + env.pos_origin[0]).float()
    y = (ac[..., 1].double() * 2.0 ** -env.pos_k + env.pos_origin[1]).float()
    h = env.alt.view(B, N).float()
    th = torch.deg2rad(env.phi.view(B, N))
    sn, cs = torch.sin(th).float(), torch.cos(th).float()
    v = env.v.view(B, N).float()
    vx, vy = v * sn, v * cs
    act = ((env.active_mask[:, None] >> torch.arange(N, device=x.device)[None, :]) & 1).bool()
    dx, dy = x[:, None, :] - x[:, :, None], y[:, None, :] - y[:, :, None]
    d2 = dx * dx + dy * dy
    off = ~act[:, None, :] | ~act[:, :, None] | torch.eye(N, dtype=torch.bool, device=x.device)[None]
    d2 = d2.masked_fill(off, float("inf"))
    k = min(K, N)
    best, j = torch.topk(d2, k, dim=2, largest=False)
    if k < K:
        best = torch.cat([best, best.new_full((B, N, K - k), float("inf"))], dim=2)
        j = torch.cat([j, j.new_zeros((B, N, K - k))], dim=2)
    pres = torch.isfinite(best)
    g = lambda t: torch.gather(t[:, None, :].expand(B, N, N), 2, j)   # noqa: E731
    ddx, ddy = g(x) - x[..., None], g(y) - y[..., None]
    dvx, dvy = g(vx) - vx[..., None], g(vy) - vy[..., None]
    s, c = sn[..., None], cs[..., None]
    sp, sh, sv = scales
    rec = torch.stack([pres.float(), torch.sqrt(best) / sp, (ddx * s + ddy * c) / sp, (ddx * c - ddy * s) / sp, (g(h) - h[..., None]) / sh,
                       (dvx * s + dvy * c) / sv, (dvx * c - dvy * s) / sv, j.float()], dim=-1)
    rec = torch.where(pres[..., None], rec, rec.new_tensor([0, 0, 0, 0, 0, 0, 0, -1.0]))
    return rec


def measure(B, N, samples, inner, seed=11):
    import torch
    from atc_hip import lib as _lib
    from atc_hip import layout as L
    from atc_hip.vec_env import AtcVecEnv
    from envs.atc import scenarios
    env = AtcVecEnv(B, N, scenario=scenarios.LOWWDense(), auto_reset=True, seed=seed, traffic=L.TRAFFIC_MAX_K)
    dev = env.device
    rng = np.random.default_rng(seed)
    acts = [torch.as_tensor(rng.uniform(-1, 1, (B, N, 3)).astype(np.float32), device=dev) for _ in range(4)]
    for t in range(200):   # spread the aircraft out; envs end and restart on the way
        env.step(acts[(t // 20) % 4])
    env.traffic_k = 0      # (from here on the launches are made below, one at a time)
    h = _lib.load()
    stream = torch.cuda.current_stream(dev)
    q = C.c_void_p(stream.cuda_stream)
    b = env.compiled.blob32
    nrm = bool(env.params.mode & L.M_NORMALIZE)
    scales = (float(b[L.C_WORLD_DIAG]), float(b[L.C_H_MAX]), 2.0 * float(b[L.C_V_MAX])) if nrm else (1.0, 1.0, 1.0)
    step = env.make_launcher(acts[0])
    rows = []
    for K in KS:
        out = torch.empty((B, N, K, L.TRAFFIC_DIM), dtype=torch.float32, device=dev)
        args = (env.sector.handle, B, N, K, C.byref(env._state), C.c_void_p(out.data_ptr()), C.byref(env.params), q)
        calls = {"kernel": lambda: _lib.check(h.atc_observe_traffic(*args)), "step": step,
                 "torch": lambda: torch_traffic(torch, env, K, scales)}
        # the two agree on the state they are timed on (order aside where distances tie: compared on the distances)
        calls["kernel"]()
        ref = torch_traffic(torch, env, K, scales)
        agree = float((out[..., L.T_DIST] - ref[..., L.T_DIST]).abs().max())
        times = benchlib.sample(calls, samples, inner, benchlib.hip_clock(torch, stream))
        nbytes = B * N * (24 + 32 * K)
        row = {"B": B, "N": N, "K": K, "normalize": nrm, "samples": samples, "launches_per_sample": inner, "bytes_per_launch": nbytes,
               "max_abs_distance_difference_kernel_vs_torch": agree}
        for v, t in times.items():
            row[v] = {"us_per_launch": benchlib.quartiles(t)}
        med = row["kernel"]["us_per_launch"]["median"]
        row["kernel"]["bytes_per_s"] = nbytes / (med * 1e-6)
        row["kernel"]["share_of_8TBps"] = nbytes / (med * 1e-6) / HBM_BYTES_PER_S
        rows.append(row)
        print("%6d x %-2d K=%d  kernel %8.1f  step %8.1f  torch %9.1f us per launch (medians); kernel at %.2f of 8 TB/s"
              % (B, N, K, med, row["step"]["us_per_launch"]["median"], row["torch"]["us_per_launch"]["median"], row["kernel"]["share_of_8TBps"]),
              flush=True)
    env.close()
    return {"rows": rows, "box": benchlib.box(torch)}


def main():
    ap = benchlib.parser("traffic_bench.json", inner=10)
    ap.add_argument("--shape", type=int, nargs=2, metavar=("B", "N"), help="(internal) measure this shape in this process, print JSON to --part")
    ap.add_argument("--part")
    a = ap.parse_args()
    if a.shape:
        benchlib.start(a, "traffic_bench")
        with open(a.part, "w") as f:
            json.dump(measure(a.shape[0], a.shape[1], a.samples, a.inner), f)
        return
    rows, box = [], None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for B, N in CONFIGS:   # one child per shape, each under its own time limit; a failure ends the run
        part = "%s.part_%dx%d" % (a.out, B, N)
        cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--shape", str(B), str(N), "--part", part,
               "--samples", str(a.samples), "--inner", str(a.inner)] + (["--lib", a.lib] if a.lib else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("traffic_bench: %d x %d ended with status %d; nothing more is started" % (B, N, rc))
        with open(part) as f:
            doc = json.load(f)
        os.remove(part)
        rows += doc["rows"]
        box = doc["box"]
    at4 = {"%dx%d" % (r["B"], r["N"]): r["kernel"]["us_per_launch"]["median"] < r["torch"]["us_per_launch"]["median"] for r in rows if r["K"] == 4}
    doc = {"what": "us per launch of atc_observe_traffic(K) | atc_step of the same env | the same records from stock torch ops on the same state",
           "method": "HIP events around `launches_per_sample` back-to-back launches, the three alternating per sample, 2 warm-up rounds; "
                     "state: 200 random steps after reset (LOWWDense)",
           "bytes": "24 B read + 32 K B written per aircraft; share_of_8TBps = bytes / time / 8e12",
           "kernel_faster_than_torch_at_K4": at4, "box": box, "library": a.lib or "in-tree build", "rows": rows}
    benchlib.write_json(a.out, doc)
    if not all(at4.values()):
        raise SystemExit("the hand kernel is NOT faster than the torch composition at K = 4: %r" % at4)


if __name__ == "__main__":
    main()
