#!/usr/bin/env python3
"""Seconds per Lanczos step on the reduced Hessian of the 2D engine: the device-resident iteration (Engine2D.hess_lanczos)
beside the host iteration of reduced_hessian_extremes_2d's default path (one Engine2D.hessvec of order 2 per step through
host arrays, two rounds of Gram-Schmidt in NumPy), here written out for a batch, on the same context, the same base point
and the same start vector.  Every node is free (a control inside the box and off zero), k steps, the runs alternating in
one process; medians of `reps`.  The device path's time is split into the transposed sweeps, the Krylov kernels (HIP event
pairs around every launch of their profiling class, in one more run of their own) and what is left of the wall time (the
upload of q0, the looks).  The Krylov kernels' traffic is counted per node and step as 8 (8 + 3 nv) bytes, nv the basis
vectors of the step's Gram-Schmidt rounds: w and the basis read in each of the three passes, w written in two, the scaled
vector read once and written twice.  One JSON line.
   python scripts/krylov_2d_timing.py [reps] [N] [steps] [batch] [k] [mode]
mode: both (default), or device0: the three-term recurrence alone beside one hessvec of order 2 (the shape of DESIGN.md 10d)"""
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import vch_amd

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
REPS, N, M, B, K = arg(1, 3), arg(2, 256), arg(3, 100), arg(4, 1), arg(5, 10)
MODE = sys.argv[6] if len(sys.argv) > 6 else "both"
dt = 1e-3
t, dts = vch_amd.time_grid(M * dt, dt)
rows = len(t)
eng = vch_amd.Engine2D(N, N, batch=B, max_steps=len(dts))
phi0 = np.stack([vch_amd.module("Vch_control_2D.Forward2_solver").init_phi_random(N, N, 1e-2, amp=0.1, seed=42 + b)
                 for b in range(B)])
xs = np.linspace(0.0, 1.0, N + 1)
pat = 0.2 + 0.1 * np.cos(np.pi * xs)[:, None] * np.cos(np.pi * xs)[None, :]
plane = np.random.default_rng(0).standard_normal((N + 1, N + 1))
u = np.empty((B, rows, N + 1, N + 1))
q0 = np.empty((B, rows, N + 1, N + 1))
for b in range(B):
    np.multiply((1.0 + 0.1 * np.cos(0.3 * np.arange(rows) + b))[:, None, None], pat[None], out=u[b])
    np.multiply(np.cos(0.3 * np.arange(rows) + b)[:, None, None], plane[None], out=q0[b])
opt = vch_amd.make_opt()
_, fst = eng.forward(phi0, dts, u=u, store=False)
del u
nodes = B * rows * (N + 1) ** 2


def device(reorth, prof=False):
    if prof:
        eng.prof_begin(400000)
    w0 = time.perf_counter()
    R = eng.hess_lanczos(q0, K, dts, t, opt, reorth=reorth)
    wall = time.perf_counter() - w0
    out = dict(wall=wall, device=R["stats"]["seconds"], steps=int(R["steps"].min()), stats=R["stats"],
               n_free=int(R["n_free"][0]), alpha=R["alpha"][0, :3].tolist())
    if prof:
        ms, cnt = np.zeros(21), np.zeros(21, dtype=np.int64)
        eng.lib.vch2d_prof_end(eng.ctx, ms.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_int64)), 21)
        noop = ms[14] / max(cnt[14], 1)                  # the event pair around an empty kernel
        out.update(krylov_ms=float(ms[20] - noop * cnt[20]), krylov_launches=int(cnt[20]), pair_us=float(1e3 * noop))
    return out


def host():
    """The loop of reduced_hessian_extremes_2d's default path, for a batch."""
    w0 = time.perf_counter()
    dev = 0.0
    Q = [q0 / np.sqrt((q0 * q0).reshape(B, -1).sum(axis=1))[:, None, None, None]]
    alphas = []
    for j in range(K):
        r = eng.hessvec(Q[j], dts, t, opt)
        dev += r["stats"]["seconds"]
        w = r["hv"]
        alphas.append((Q[j] * w).reshape(B, -1).sum(axis=1))
        for _ in range(2):
            for v in Q:
                w -= (v * w).reshape(B, -1).sum(axis=1)[:, None, None, None] * v
        beta = np.sqrt((w * w).reshape(B, -1).sum(axis=1))
        if j + 1 < K:
            Q.append(w / beta[:, None, None, None])
    return dict(wall=time.perf_counter() - w0, device=dev, steps=K, alpha=[float(a[0]) for a in alphas[:3]])


def traffic(reorth):
    nv = [(j + 1) if reorth else min(j + 1, 2) for j in range(K)]
    return float(sum(8 * (8 + 3 * n) for n in nv)) * nodes


res = dict(cfg=dict(N=N, steps=len(dts), dt=dt, batch=B, k=K, mode=MODE, nodes=nodes), forward=fst["seconds"])
if MODE == "both":
    runs = dict(device=[], host=[])
    for _ in range(REPS):
        runs["device"].append(device(True))
        runs["host"].append(host())
    p = device(True, prof=True)
    med = lambda name, key: float(np.median([r[key] for r in runs[name]]))
    dsteps = runs["device"][0]["steps"]
    res.update(device=dict(wall_per_step=med("device", "wall") / dsteps, device_per_step=med("device", "device") / dsteps,
                           all_wall=[r["wall"] for r in runs["device"]], stats=runs["device"][0]["stats"],
                           alpha=runs["device"][0]["alpha"], n_free=runs["device"][0]["n_free"]),
               host=dict(wall_per_step=med("host", "wall") / K, device_per_step=med("host", "device") / K,
                         all_wall=[r["wall"] for r in runs["host"]], alpha=runs["host"][0]["alpha"]),
               krylov=dict(ms_per_step=p["krylov_ms"] / dsteps, launches=p["krylov_launches"], pair_us=p["pair_us"],
                           bytes=traffic(True), TB_per_s=traffic(True) / (1e-3 * p["krylov_ms"]) / 1e12,
                           fraction_of_8TBs=traffic(True) / (1e-3 * p["krylov_ms"]) / 8e12,
                           device_seconds_under_profiling=p["device"]))
    res["speedup_wall"] = res["host"]["wall_per_step"] / res["device"]["wall_per_step"]
else:
    runs = [device(False) for _ in range(REPS)]
    p = device(False, prof=True)
    hv = eng.hessvec(q0, dts, t, opt)["stats"]
    steps = runs[0]["steps"]
    grad = eng.hessvec(None, dts, t, opt, order=1)["stats"]["seconds"]
    dev = float(np.median([r["device"] for r in runs]))
    res.update(device0=dict(device_seconds=dev, steps=steps, per_step_all_in=dev / steps, gradient_sweep=grad,
                            per_step_without_the_gradient_sweep=(dev - grad) / steps, wall=[r["wall"] for r in runs],
                            stats=runs[0]["stats"]),
               hessvec2=dict(seconds=hv["seconds"], linear_solves=hv["linear_solves"]),
               krylov=dict(ms_per_step=p["krylov_ms"] / steps, bytes=traffic(False),
                           TB_per_s=traffic(False) / (1e-3 * p["krylov_ms"]) / 1e12))
    res["per_step_over_hessvec2"] = res["device0"]["per_step_without_the_gradient_sweep"] / hv["seconds"]
print(json.dumps(res), flush=True)
eng.close()
