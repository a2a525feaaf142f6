#!/usr/bin/env python3
"""Seconds per round of the trust-region rounds of the 1D engine (Engine1D.pgd_trust) beside the damped Newton rounds
(Engine1D.pgd_newton), both about a resident PGD problem, at the two shapes of DESIGN.md 10j: N = 4096 x 1000 steps at batch
1 and N = 256 x 100 steps at batch 256, and how the rounds of either end from the start of DESIGN.md 10h.  Two problems per
shape, both from the default start of the 1D march with the control of amplitude 5 of scripts/newton_1d_timing.py inside a
wide box:
    definite     the marched state as targets (the problem of newton_1d_timing.py: no round ends on the curvature);
    indefinite   the default targets of GD_1D.build_targets_1d, where the reduced Hessian about this control is indefinite.
`rounds` rounds of at most `k` conjugate-gradient steps; the first radius is a tenth of ||u||_D.  Wall-clock seconds of the
whole call over the rounds it ran, the call's own split beside it, and the counts of every round status.  Recorded, not
asserted.  One JSON line per shape, appended to profiles/trust_1d_timing.txt (or the path in VCH_TIMING_OUT).
   python scripts/trust_1d_timing.py [rounds] [k]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import vch_amd

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
ROUNDS, K = arg(1, 4), arg(2, 10)
SHAPES = [dict(N=4096, M=1000, dt=1e-3, B=1), dict(N=256, M=100, dt=5e-3, B=256)]
OUT = os.environ.get("VCH_TIMING_OUT", os.path.join("profiles", "trust_1d_timing.txt"))
K1 = vch_amd.module("Vch_control_1D.config")
G1 = vch_amd.module("Vch_control_1D.GD_1D")
F1 = vch_amd.module("Vch_control_1D.Forward_solver")
ocfg = K1.OptimizationConfig(u_min=-1e3, u_max=1e3)


def trapezoid(v):
    d = np.diff(v)
    w = np.zeros(len(v))
    w[:-1] += 0.5 * d
    w[1:] += 0.5 * d
    return w


def problem(cfg, B, definite):
    N = int(cfg.N)
    tg, dts = vch_amd.time_grid(float(cfg.T), float(cfg.dt_initial))
    t = np.concatenate([[0.0], tg])
    rows = len(t)
    x = np.linspace(0.0, float(cfg.Lx), N + 1)
    phi0 = F1.init_phi_random(N, F1.delta_sep, amp=0.01, seed=42, enforce_zero_mean=True)
    U = np.stack([5.0 * np.cos(np.pi * x * (1 + b % 3))[None, :] * np.sin(1 + 0.01 * np.arange(rows) + b)[:, None] for b in range(B)])
    if definite:
        eng = vch_amd.Engine1D.from_config(cfg, batch=B, max_steps=len(dts))
        phi_Q = eng.forward(np.repeat(phi0[None], B, axis=0), dts, u=U, store=True)[0].reshape(B, rows, N + 1)
        eng.close()
        phi_T = np.ascontiguousarray(phi_Q[:, -1])
    else:
        pT, pQ = G1.build_targets_1d(x, t, phi0, float(cfg.Lx), float(cfg.T))
        phi_T, phi_Q = np.repeat(pT[None], B, axis=0), np.repeat(pQ[None], B, axis=0)
    wt = trapezoid(t)
    wt[0] = wt[1]
    radius0 = 0.1 * np.sqrt(np.einsum("k,i,bki->b", wt, trapezoid(x), U * U))
    return t, dts, x, phi0, U, phi_Q, phi_T, radius0


def run(cfg, B, definite, trust):
    t, dts, x, phi0, U, phi_Q, phi_T, radius0 = problem(cfg, B, definite)
    eng = vch_amd.Engine1D.from_config(cfg, batch=B, max_steps=len(dts))
    eng.pgd_init(np.repeat(phi0[None], B, axis=0), phi_T, t, dts, [vch_amd.make_opt(ocfg)], phi_Q=phi_Q, x=x, u0=U)
    w0 = time.perf_counter()
    R = eng.pgd_trust(ROUNDS, radius0, k=K) if trust else eng.pgd_newton(ROUNDS, k=K)
    wall = time.perf_counter() - w0
    eng.close()
    names = vch_amd.Engine1D.TRUST_STATUS
    n = max(int(R["rounds"]), 1)
    first, last = R["cost"][:, 0], np.array([row[np.isfinite(row)][-1] for row in R["cost_new"]])
    return dict(wall=wall, rounds=int(R["rounds"]), seconds_per_round=wall / n, split={k: float(v) for k, v in R["seconds"].items()},
                status={names[s]: int((R["status"] == s).sum()) for s in sorted(set(int(v) for v in R["status"].ravel()))},
                cg_status={vch_amd.Engine1D.TRUST_CG_STATUS[s]: int(((R["cg_status"] == s) & (R["status"] != 5)).sum())
                           for s in sorted(set(int(v) for v in R["cg_status"].ravel()))},
                moved=int((last < first).sum()), cost=float(first[0]), cost_new=float(last[0]))


lines = []
for shape in SHAPES:
    cfg = K1.ForwardSolverConfig(N=shape["N"], T=shape["M"] * shape["dt"], dt_initial=shape["dt"])
    B = shape["B"]
    res = dict(cfg=dict(N=shape["N"], steps=shape["M"], dt=shape["dt"], batch=B, rounds=ROUNDS, k=K))
    run(cfg, 1, True, True)                     # warm-up: code objects
    for definite in (True, False):
        for trust in (False, True):
            res[("definite" if definite else "indefinite") + ("_trust" if trust else "_newton")] = run(cfg, B, definite, trust)
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "a") as fh:
    fh.write("\n".join(lines) + "\n")
