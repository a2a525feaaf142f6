#!/usr/bin/env python3
"""Seconds per conjugate-gradient iteration of the device-resident Newton-CG step of the 1D engine (Engine1D.hess_cg with the
Newton right-hand side built on the device) beside a Lanczos step without reorthogonalisation
(Engine1D.hess_lanczos(reorth=False)) on the same context and base point, for the two shapes of DESIGN.md 10f:
N = 4096, M = 1000 at batch 1 and N = 256, M = 100 at batch 256.  Both run the tangent march and the second transposed
sweep per step after the gradient sweep once, so by solve count a CG iteration costs a Lanczos step.  Every node is free
(an uploaded mask of ones; the control is off zero almost everywhere and the box is wide), k = 10 steps each with cg_tol far
below reach, the runs alternating in one process, median of `reps`.  The targets are the marched state itself: the
misfit vanishes, the Hessian is its Gauss-Newton part plus b3 times the mass, and no trajectory leaves early on the
curvature (about an arbitrary control the reduced Hessian is indefinite and most trajectories would); the kernels' work
does not depend on the data.  The steps and statuses are recorded.  The seconds are
vch_stats.seconds (device time between the call's two events, the set-up launch included) over the products taken.
Writes profiles/hess_cg_1d_timing.txt (one JSON line per shape; or the path in VCH_TIMING_OUT) and prints it.
   python scripts/hess_cg_1d_timing.py [reps]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
import vch_amd

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
K = 10
SHAPES = [dict(N=4096, M=1000, dt=1e-3, B=1), dict(N=256, M=100, dt=5e-3, B=256)]
OUT = os.environ.get("VCH_TIMING_OUT", os.path.join("profiles", "hess_cg_1d_timing.txt"))

lines = []
for s in SHAPES:
    N, M, dt, B = s["N"], s["M"], s["dt"], s["B"]
    tg, dts = vch_amd.time_grid(M * dt, dt)
    t = np.concatenate([[0.0], tg])
    rows = len(t)
    x = np.linspace(0.0, 1.0, N + 1)
    phi0 = np.stack([0.2 * np.cos(np.pi * x + 0.4 * b) for b in range(B)])
    U = np.stack([5.0 * np.cos(np.pi * x * (1 + b % 3))[None, :] * np.sin(1 + 0.01 * np.arange(rows) + b)[:, None] for b in range(B)])
    q0 = np.random.default_rng(0).standard_normal((B, rows, N + 1))
    mask = np.ones((B, rows, N + 1), dtype=bool)
    opt = vch_amd.make_opt(u_min=-1e3, u_max=1e3)
    eng = vch_amd.Engine1D(N=N, batch=B, max_steps=len(dts))
    phi = eng.forward(phi0, dts, u=U, store=True)[0].reshape(B, rows, N + 1)
    base = dict(u=U, dt=dts, phi_Q=phi, phi_T=np.ascontiguousarray(phi[:, -1]))
    sec = dict(cg=[], lanczos0=[])
    info = {}
    for _ in range(REPS):
        R = eng.hess_cg(K, t, opt, cg_tol=1e-30, precond=True, mask=mask, **base)
        products = (R["stats"]["linear_solves"] / len(dts) - B) / 2.0 / B          # per trajectory, on average
        sec["cg"].append(R["stats"]["seconds"] / products)
        info = dict(steps=[int(R["steps"].min()), int(R["steps"].max())], status=sorted(set(int(v) for v in R["status"])),
                    products_per_trajectory=products, stats=R["stats"])
        L = eng.hess_lanczos(q0, K, t, opt, mask=mask, reorth=False, **base)
        assert list(L["steps"]) == [K] * B
        sec["lanczos0"].append(L["stats"]["seconds"] / K)
    eng.close()
    med = {k: float(np.median(v)) for k, v in sec.items()}
    spread = {k: float(max(v) - min(v)) for k, v in sec.items()}
    lines.append(json.dumps(dict(cfg=dict(N=N, steps=len(dts), dt=dt, batch=B, k=K), seconds_per_step=med, spread=spread, all=sec,
                                 cg=info, cg_over_lanczos0=med["cg"] / med["lanczos0"])))
    print(lines[-1], flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as fh:
    fh.write("scripts/hess_cg_1d_timing.py: seconds per CG iteration (Newton right-hand side, preconditioned) and per Lanczos step "
             "without reorthogonalisation, k = %d, median of %d alternating runs; both include the set-up launch (mask, the "
             "gradient sweep once) spread over the steps\n" % (K, REPS))
    fh.write("\n".join(lines) + "\n")
