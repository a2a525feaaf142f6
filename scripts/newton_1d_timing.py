#!/usr/bin/env python3
"""Seconds per damped Newton round on the free set of the 1D engine: the device-resident rounds (Engine1D.pgd_newton about a
resident PGD problem) and the host loop GD_1D.newton_refine (one context per march and per cost, the step pulled through
cg_vector, the trial formed in NumPy; batch 1 only), at the two shapes of DESIGN.md 10h: N = 4096 x 1000 steps (device and
host at batch 1) and N = 256 x 100 steps (device at batch 1 and 256, host at batch 1).  The start state is the default
start of the 1D march, the control is off zero almost everywhere inside a wide box (every node free but a few), and the
targets are the marched state itself, so that the Hessian is its Gauss-Newton part plus b3 times the mass and no round
ends on the curvature.  `rounds` rounds of at most `k` conjugate-gradient steps.  Wall-clock seconds of the whole call
over the rounds it ran; the device call's own split (solves, trial kernel, marches, costs) beside it.  Recorded, not
asserted.  One JSON line per shape, appended to profiles/newton_1d_timing.txt (or the path in VCH_TIMING_OUT).
   python scripts/newton_1d_timing.py [rounds] [k]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import vch_amd

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
ROUNDS, K = arg(1, 2), arg(2, 10)
SHAPES = [dict(N=4096, M=1000, dt=1e-3, batches=(1,)), dict(N=256, M=100, dt=5e-3, batches=(1, 256))]
OUT = os.environ.get("VCH_TIMING_OUT", os.path.join("profiles", "newton_1d_timing.txt"))
K1 = vch_amd.module("Vch_control_1D.config")
G1 = vch_amd.module("Vch_control_1D.GD_1D")
F1 = vch_amd.module("Vch_control_1D.Forward_solver")
ocfg = K1.OptimizationConfig(u_min=-1e3, u_max=1e3)


def problem(cfg, B):
    """phi0 (the default start), the controls, and the marched states as targets."""
    N = int(cfg.N)
    tg, dts = vch_amd.time_grid(float(cfg.T), float(cfg.dt_initial))
    t = np.concatenate([[0.0], tg])
    rows = len(t)
    x = np.linspace(0.0, float(cfg.Lx), N + 1)
    phi0 = F1.init_phi_random(N, F1.delta_sep, amp=0.01, seed=42, enforce_zero_mean=True)
    U = np.stack([5.0 * np.cos(np.pi * x * (1 + b % 3))[None, :] * np.sin(1 + 0.01 * np.arange(rows) + b)[:, None] for b in range(B)])
    eng = vch_amd.Engine1D.from_config(cfg, batch=B, max_steps=len(dts))
    phi = eng.forward(np.repeat(phi0[None], B, axis=0), dts, u=U, store=True)[0].reshape(B, rows, N + 1)
    eng.close()
    return t, dts, x, phi0, U, phi


def device(cfg, B):
    t, dts, x, phi0, U, phi = problem(cfg, B)
    eng = vch_amd.Engine1D.from_config(cfg, batch=B, max_steps=len(dts))
    eng.pgd_init(np.repeat(phi0[None], B, axis=0), np.ascontiguousarray(phi[:, -1]), t, dts, [vch_amd.make_opt(ocfg)], phi_Q=phi, x=x, u0=U)
    w0 = time.perf_counter()
    R = eng.pgd_newton(ROUNDS, k=K)
    wall = time.perf_counter() - w0
    eng.close()
    n = max(int(R["rounds"]), 1)
    return dict(batch=B, wall=wall, rounds=int(R["rounds"]), seconds_per_round=wall / n, split={k: float(v) for k, v in R["seconds"].items()},
                status=sorted(set(int(v) for v in R["status"].ravel())), s=sorted(set(float(v) for v in R["s"].ravel() if np.isfinite(v))),
                halvings=int(R["halvings"].max()), cg_steps=[int(R["cg_steps"].min()), int(R["cg_steps"].max())],
                cg_status=sorted(set(int(v) for v in R["cg_status"].ravel())), n_free=[int(R["n_free"][:, 0].min()), int(R["n_free"][:, 0].max())],
                cost=float(R["cost"][0, 0]), cost_new=float(np.nanmin(R["cost_new"][0])))


def host(cfg):
    t, dts, x, phi0, U, phi = problem(cfg, 1)
    w0 = time.perf_counter()
    _, recs = G1.newton_refine(cfg, ocfg, U[0], phi[0], phi[0, -1], n_newton=ROUNDS, k=K)
    wall = time.perf_counter() - w0
    return dict(batch=1, wall=wall, rounds=len(recs), seconds_per_round=wall / max(len(recs), 1), status=[r["status"] for r in recs],
                s=[r["s"] for r in recs], cg_steps=[r["steps"] for r in recs], n_free=recs[0]["n_free"], cost=recs[0]["cost"],
                cost_new=recs[-1]["cost_new"])


lines = []
for shape in SHAPES:
    cfg = K1.ForwardSolverConfig(N=shape["N"], T=shape["M"] * shape["dt"], dt_initial=shape["dt"])
    res = dict(cfg=dict(N=shape["N"], steps=shape["M"], dt=shape["dt"], rounds=ROUNDS, k=K))
    device(cfg, 1)                              # warm-up: code objects
    for B in shape["batches"]:
        res[f"device_b{B}"] = device(cfg, B)
    host(cfg)                                   # warm-up of the host loop's cached context
    res["host_b1"] = host(cfg)
    res["host_over_device_b1"] = res["host_b1"]["seconds_per_round"] / res["device_b1"]["seconds_per_round"]
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "a") as fh:
    fh.write("\n".join(lines) + "\n")
