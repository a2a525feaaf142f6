#!/usr/bin/env python3
"""Seconds per damped Newton round on the free set of the 2D engine: the device-resident rounds (Engine2D.pgd_newton about
a resident PGD problem) at batch 1 and batch 8, and the host loop GD2_configured.newton_refine (one context per march and
per cost, the step pulled through cg_vector, the trial formed in NumPy) at batch 1, on the same problem: N x N nodes,
`steps` time steps, the ramp target, a control inside the box and off zero (every node free), at most K conjugate-gradient
steps per round.  Wall-clock seconds of the whole call over the rounds it ran; the device call's own split (solves, trial
kernel, marches, costs) beside it.  Recorded, not asserted.  One JSON line, appended to profiles/newton_2d_timing.txt (or
the path in VCH_TIMING_OUT).
   python scripts/newton_2d_timing.py [N] [steps] [rounds] [k]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import vch_amd

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
N, M, ROUNDS, K = arg(1, 256), arg(2, 100), arg(3, 2), arg(4, 10)
OUT = os.environ.get("VCH_TIMING_OUT", "profiles/newton_2d_timing.txt")
dt = 1e-3
K2 = vch_amd.module("Vch_control_2D.config")
G2 = vch_amd.module("Vch_control_2D.GD2_configured")
F2 = vch_amd.module("Vch_control_2D.Forward2_solver")
cfg = K2.ForwardSolverConfig(Nx=N, Ny=N, T=M * dt, dt_initial=dt)
ocfg = K2.OptimizationConfig()
t, dts = vch_amd.time_grid(float(cfg.T), float(cfg.dt_initial))
rows = len(t)
xs, ys = np.linspace(0.0, cfg.Lx, N + 1), np.linspace(0.0, cfg.Ly, N + 1)
pat = 0.2 + 0.1 * np.cos(np.pi * xs / cfg.Lx)[:, None] * np.cos(np.pi * ys / cfg.Ly)[None, :]


def problem(B):
    phi0 = np.stack([F2.init_phi_random(N, N, F2.DELTA_SEP, amp=0.1, seed=42 + b) for b in range(B)])
    u = np.empty((B, rows, N + 1, N + 1))
    for b in range(B):
        np.multiply((1.0 + 0.1 * np.cos(0.3 * np.arange(rows) + b))[:, None, None], pat[None], out=u[b])
    tg = [G2.build_targets(xs, ys, t, phi0[b], cfg.Lx, cfg.Ly, cfg.T) for b in range(B)]
    return phi0, u, np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])


def device(B):
    phi0, u, phi_T, phi_Q = problem(B)
    eng = vch_amd.Engine2D.from_config(cfg, batch=B, max_steps=len(dts))
    eng.pgd_init(phi0, phi_T, t, [vch_amd.make_opt(ocfg)], phi_Q=phi_Q, ramp=False, u0=u)
    del u, phi_Q
    w0 = time.perf_counter()
    R = eng.pgd_newton(ROUNDS, k=K)
    wall = time.perf_counter() - w0
    eng.close()
    n = max(int(R["rounds"]), 1)
    return dict(batch=B, wall=wall, rounds=int(R["rounds"]), seconds_per_round=wall / n, split={k: float(v) for k, v in R["seconds"].items()},
                status=R["status"].tolist(), s=R["s"].tolist(), halvings=R["halvings"].tolist(), cg_steps=R["cg_steps"].tolist(),
                cg_status=R["cg_status"].tolist(), n_free=R["n_free"][:, 0].tolist(), cost=R["cost"][:, 0].tolist(),
                cost_new=[float(np.nanmin(c)) for c in R["cost_new"]])


def host():
    phi0, u, phi_T, phi_Q = problem(1)
    w0 = time.perf_counter()
    _, recs = G2.newton_refine(cfg, ocfg, u[0], phi_Q[0], phi_T[0], n_newton=ROUNDS, k=K)
    wall = time.perf_counter() - w0
    return dict(batch=1, wall=wall, rounds=len(recs), seconds_per_round=wall / max(len(recs), 1), status=[r["status"] for r in recs],
                s=[r["s"] for r in recs], cg_steps=[r["steps"] for r in recs], n_free=recs[0]["n_free"], cost=recs[0]["cost"],
                cost_new=recs[-1]["cost_new"])


res = dict(cfg=dict(N=N, steps=len(dts), dt=dt, rounds=ROUNDS, k=K, nodes=rows * (N + 1) ** 2, history_bytes=8 * rows * (N + 1) ** 2))
device(1)                                   # warm-up: code objects, plans
res["device_b1"] = device(1)
res["device_b8"] = device(8)
res["host_b1"] = host()
res["host_over_device_b1"] = res["host_b1"]["seconds_per_round"] / res["device_b1"]["seconds_per_round"]
line = json.dumps(res)
print(line, flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "a") as fh:
    fh.write(line + "\n")
