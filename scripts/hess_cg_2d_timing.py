#!/usr/bin/env python3
"""Seconds per conjugate-gradient iteration of the device-resident Newton-CG step of the 2D engine (Engine2D.hess_cg with
the Newton right-hand side built on the device) beside a Lanczos step without reorthogonalisation
(Engine2D.hess_lanczos(reorth=False)) on the same context and base point: both run the tangent march and the second
transposed sweep per step, after the gradient sweep once.  Every node is free (a control inside the box and off zero).
K steps each (cg_tol far below reach), the runs alternating in one process; medians of `reps`.  The share of the streaming
kernels (k_kr_mask, k_ncg_*; HIP event pairs around every launch of their profiling class, in one more run of their own)
and the iterations to a relative residual of 1e-6 with and without the preconditioner follow.  One JSON line, appended to
profiles/hess_cg_2d_timing.txt (or the path in VCH_TIMING_OUT).
   python scripts/hess_cg_2d_timing.py [reps] [N] [steps] [batch] [k] [mode]
mode: both (default), or cg: one preconditioned run to 1e-6 of at most k steps alone (the headline shape)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import vch_amd

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
REPS, N, M, B, K = arg(1, 3), arg(2, 256), arg(3, 100), arg(4, 1), arg(5, 10)
MODE = sys.argv[6] if len(sys.argv) > 6 else "both"
OUT = os.environ.get("VCH_TIMING_OUT", "profiles/hess_cg_2d_timing.txt")
dt = 1e-3
t, dts = vch_amd.time_grid(M * dt, dt)
rows = len(t)
eng = vch_amd.Engine2D(N, N, batch=B, max_steps=len(dts))
phi0 = np.stack([vch_amd.module("Vch_control_2D.Forward2_solver").init_phi_random(N, N, 1e-2, amp=0.1, seed=42 + b)
                 for b in range(B)])
xs = np.linspace(0.0, 1.0, N + 1)
pat = 0.2 + 0.1 * np.cos(np.pi * xs)[:, None] * np.cos(np.pi * xs)[None, :]
u = np.empty((B, rows, N + 1, N + 1))
for b in range(B):
    np.multiply((1.0 + 0.1 * np.cos(0.3 * np.arange(rows) + b))[:, None, None], pat[None], out=u[b])
opt = vch_amd.make_opt()
_, fst = eng.forward(phi0, dts, u=u, store=False)
nodes = B * rows * (N + 1) ** 2


def cg(k, cg_tol, precond, prof=False):
    if prof:
        eng.prof_begin(400000)
    w0 = time.perf_counter()
    R = eng.hess_cg(k, cg_tol=cg_tol, precond=precond, dt=dts, t_hist=t, opt=opt)
    out = dict(wall=time.perf_counter() - w0, device=R["stats"]["seconds"], steps=R["steps"].tolist(), status=R["status"].tolist(),
               resid=[float(R["resid"][b, max(int(s) - 1, 0)]) for b, s in enumerate(R["steps"])], n_free=int(R["n_free"][0]),
               curv=[float(np.nanmin(R["curv"])), float(np.nanmax(R["curv"]))], linear_solves=R["stats"]["linear_solves"])
    if prof:
        ms, cnt = np.zeros(21), np.zeros(21, dtype=np.int64)
        eng.lib.vch2d_prof_end(eng.ctx, ms.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_int64)), 21)
        noop = ms[14] / max(cnt[14], 1)                  # the event pair around an empty kernel
        out.update(krylov_ms=float(ms[20] - noop * cnt[20]), krylov_launches=int(cnt[20]))
    return out


res = dict(cfg=dict(N=N, steps=len(dts), dt=dt, batch=B, k=K, mode=MODE, nodes=nodes, history_bytes=8 * nodes), forward=fst["seconds"])
if MODE == "both":
    q0 = np.empty_like(u)
    plane = np.random.default_rng(0).standard_normal((N + 1, N + 1))
    for b in range(B):
        np.multiply(np.cos(0.3 * np.arange(rows) + b)[:, None, None], plane[None], out=q0[b])
    del u
    runs = dict(cg=[], lanczos=[])
    for _ in range(REPS):
        runs["cg"].append(cg(K, 1e-30, True))
        runs["lanczos"].append(eng.hess_lanczos(q0, K, dts, t, opt, reorth=False)["stats"]["seconds"])
    grad = eng.hessvec(None, dts, t, opt, order=1)["stats"]["seconds"]
    p = cg(K, 1e-30, True, prof=True)
    dev = float(np.median([r["device"] for r in runs["cg"]]))
    lan = float(np.median(runs["lanczos"]))
    # per CG iteration the streaming kernels move 17 + 49 + 32 bytes per node (the last iteration has no k_ncg_dir); once:
    # the mask from the control 9, the start 49 (gradient, control and mask read, x, r, p and the direction written)
    counted = (98.0 * K - 32.0 + 49.0 + 9.0) * nodes
    res.update(cg=dict(device_seconds=dev, per_iteration_all_in=dev / K, gradient_sweep=grad,
                       per_iteration_without_the_gradient_sweep=(dev - grad) / K, all=[r["device"] for r in runs["cg"]],
                       steps=runs["cg"][0]["steps"], linear_solves=runs["cg"][0]["linear_solves"]),
               lanczos0=dict(device_seconds=lan, per_step_all_in=lan / K, per_step_without_the_gradient_sweep=(lan - grad) / K,
                             all=runs["lanczos"]),
               streaming=dict(ms=p["krylov_ms"], launches=p["krylov_launches"], ms_per_iteration=p["krylov_ms"] / K,
                              share_of_the_call=1e-3 * p["krylov_ms"] / p["device"], counted_bytes=counted,
                              TB_per_s=counted / (1e-3 * p["krylov_ms"]) / 1e12))
    res["cg_over_lanczos0"] = (dev - grad) / (lan - grad)
    res["to_1e-6"] = {name: {k: r[k] for k in ("steps", "status", "resid", "device", "curv")}
                      for name, r in (("precond", cg(80, 1e-6, True)), ("plain", cg(80, 1e-6, False)))}
else:
    del u
    res["cg"] = cg(K, 1e-6, True)      # "device": the whole call, the gradient sweep included; (linear_solves / (B M) - 1) / 2 products ran
line = json.dumps(res)
print(line, flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "a") as fh:
    fh.write(line + "\n")
eng.close()
