#!/usr/bin/env python3
"""Seconds per round of the trust-region rounds of the 2D engine (Engine2D.pgd_trust) beside the damped Newton rounds
(Engine2D.pgd_newton), both about a resident PGD problem, at the shape of DESIGN.md 10g / 10i: N x N nodes, `steps` time
steps, batch 1 and batch 8, and how the rounds of either end.  The start is the timing start of DESIGN.md 10g (the control
0.2 +- 0.1 of scripts/hess_cg_2d_timing.py, every node free, default weights) with the targets of
scripts/newton_2d_timing.py, once with dt = 1e-3 (T = 0.1, the horizon of 10g's 256^2 table and of 10i) and once with
dt = 1e-2 (T = 1, the horizon of 10g's headline run, where that section found the reduced Hessian indefinite).
`rounds` rounds of at most `k` conjugate-gradient steps; the first radius is a tenth of ||u||_D.  One warm-up call per
shape, then `reps` calls of either kind alternating, each from a fresh pgd_init; wall-clock seconds of the whole call over the
rounds it ran (median and all), the call's own split, every member-round's status and CG exit, the cost before and after.
Recorded, not asserted.  One JSON line per horizon and batch, appended to profiles/trust_2d_timing.txt (or the path in
VCH_TIMING_OUT).
   python scripts/trust_2d_timing.py [N] [steps] [rounds] [k] [reps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import vch_amd

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
N, M, ROUNDS, K, REPS = arg(1, 256), arg(2, 100), arg(3, 3), arg(4, 10), arg(5, 3)
OUT = os.environ.get("VCH_TIMING_OUT", os.path.join("profiles", "trust_2d_timing.txt"))
K2 = vch_amd.module("Vch_control_2D.config")
G2 = vch_amd.module("Vch_control_2D.GD2_configured")
F2 = vch_amd.module("Vch_control_2D.Forward2_solver")
ocfg = K2.OptimizationConfig()
E = vch_amd.Engine2D


def trapezoid(v):
    d = np.diff(v)
    w = np.zeros(len(v))
    w[:-1] += 0.5 * d
    w[1:] += 0.5 * d
    return w


def problem(cfg, B):
    t, dts = vch_amd.time_grid(float(cfg.T), float(cfg.dt_initial))
    rows = len(t)
    xs, ys = np.linspace(0.0, cfg.Lx, N + 1), np.linspace(0.0, cfg.Ly, N + 1)
    pat = 0.2 + 0.1 * np.cos(np.pi * xs / cfg.Lx)[:, None] * np.cos(np.pi * ys / cfg.Ly)[None, :]
    phi0 = np.stack([F2.init_phi_random(N, N, F2.DELTA_SEP, amp=0.1, seed=42 + b) for b in range(B)])
    u = np.empty((B, rows, N + 1, N + 1))
    for b in range(B):
        np.multiply((1.0 + 0.1 * np.cos(0.3 * np.arange(rows) + b))[:, None, None], pat[None], out=u[b])
    tg = [G2.build_targets(xs, ys, t, phi0[b], cfg.Lx, cfg.Ly, cfg.T) for b in range(B)]
    radius0 = 0.1 * np.sqrt(np.einsum("k,i,j,bkij->b", trapezoid(t), trapezoid(xs), trapezoid(ys), u * u))
    return t, dts, phi0, u, np.stack([a for a, _ in tg]), np.stack([q for _, q in tg]), radius0


def run(cfg, prob, trust):
    t, dts, phi0, u, phi_T, phi_Q, radius0 = prob
    eng = E.from_config(cfg, batch=len(phi0), max_steps=len(dts))
    eng.pgd_init(phi0, phi_T, t, [vch_amd.make_opt(ocfg)], phi_Q=phi_Q, ramp=False, u0=u)
    w0 = time.perf_counter()
    R = eng.pgd_trust(ROUNDS, radius0, k=K) if trust else eng.pgd_newton(ROUNDS, k=K)      # returns after a device synchronise
    wall = time.perf_counter() - w0
    eng.close()
    n = max(int(R["rounds"]), 1)
    live = R["status"] != 5
    count = lambda names, a: {names[s]: int(((a == s) & live).sum()) for s in sorted(set(int(v) for v in a[live].ravel()))}
    first, last = R["cost"][:, 0], np.array([row[np.isfinite(row)][-1] for row in R["cost_new"]])
    out = dict(wall=wall, rounds=int(R["rounds"]), seconds_per_round=wall / n, split={k: float(v) for k, v in R["seconds"].items()},
               status=count(E.TRUST_STATUS, R["status"]), cg_status=count(E.TRUST_CG_STATUS, R["cg_status"]), idle=int((~live).sum()),
               cg_steps=R["cg_steps"].tolist(), moved=int((last < first).sum()), cost=first.tolist(), cost_new=last.tolist())
    if trust:
        out.update(radius=R["radius"].tolist(), ratio=R["ratio"].tolist())
    return out


lines = []
for dt in (1e-3, 1e-2):
    cfg = K2.ForwardSolverConfig(Nx=N, Ny=N, T=M * dt, dt_initial=dt)
    for B in (1, 8):
        prob = problem(cfg, B)
        res = dict(cfg=dict(N=N, steps=M, dt=dt, batch=B, rounds=ROUNDS, k=K, reps=REPS, radius0=prob[-1].tolist()))
        run(cfg, prob, True)                    # warm-up: code objects, plans
        runs = dict(newton=[], trust=[])
        for _ in range(REPS):
            runs["newton"].append(run(cfg, prob, False))
            runs["trust"].append(run(cfg, prob, True))
        for name, rr in runs.items():
            per = [r["seconds_per_round"] for r in rr]
            res[name] = dict(rr[0], seconds_per_round=float(np.median(per)), seconds_per_round_all=per)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "a") as fh:
    fh.write("\n".join(lines) + "\n")
