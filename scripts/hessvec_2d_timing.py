#!/usr/bin/env python3
"""Device time of vch2d_hessvec (order 1: the exact gradient field; order 2: gradient and H h) beside vch2d_second_order
(order 2) and the forward march on the same context, at the shape of DESIGN.md 10: 512^2 x 1000 steps x 8 trajectories, no
control, white-noise planes times cos(0.3 k + b) as directions, default rtol.  The four histories the call keeps beyond
the direction (G, H h, the raw tangent solves, the tangent after the mean removal) take 16.8 GB each at this shape and fit
beside the state history.  Median of `reps` from vch_stats.seconds, the calls alternating in one process.  One JSON line.
   python scripts/hessvec_2d_timing.py [reps] [N] [steps] [batch]"""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import vch_amd

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
REPS, N, M, B = arg(1, 3), arg(2, 512), arg(3, 1000), arg(4, 8)
dt = 1e-3
t, dts = vch_amd.time_grid(M * dt, dt)
rows = len(t)
eng = vch_amd.Engine2D(N, N, batch=B, max_steps=len(dts))
phi0 = np.stack([vch_amd.module("Vch_control_2D.Forward2_solver").init_phi_random(N, N, 1e-2, amp=0.1, seed=42 + b)
                 for b in range(B)])
plane = np.random.default_rng(0).standard_normal((N + 1, N + 1))
H = np.empty((B, rows, N + 1, N + 1))
for b in range(B):
    np.multiply(np.cos(0.3 * np.arange(rows) + b)[:, None, None], plane[None], out=H[b])
opt = vch_amd.make_opt()
sec = dict(forward=[], second_order2=[], hessvec1=[], hessvec2=[])
stats = {}
for _ in range(REPS):
    _, st = eng.forward(phi0, dts, store=False)
    sec["forward"].append(st["seconds"])
    so = eng.second_order(H, dts, t, opt, order=2)
    sec["second_order2"].append(so["stats"]["seconds"])
    stats["second_order2"] = so["stats"]
    for order in (1, 2):
        r = eng.hessvec(H, dts, t, opt, order=order)
        sec[f"hessvec{order}"].append(r["stats"]["seconds"])
        stats[f"hessvec{order}"] = r["stats"]
        if order == 1:
            slope = r["slope"].copy()
        del r["grad"]
med = {k: float(np.median(v)) for k, v in sec.items()}
print(json.dumps(dict(cfg=dict(N=N, steps=len(dts), dt=dt, batch=B), seconds=med, all=sec, stats=stats,
                      hessvec1_over_second_order2=med["hessvec1"] / med["second_order2"],
                      hessvec2_over_second_order2=med["hessvec2"] / med["second_order2"],
                      hessvec2_over_forward=med["hessvec2"] / med["forward"],
                      slope_dev=float(np.abs(slope / so["slope"] - 1.0).max()),
                      curvature_dev=float(np.abs(r["curvature"] / so["curvature"] - 1.0).max()))), flush=True)
eng.close()
