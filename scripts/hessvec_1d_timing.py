#!/usr/bin/env python3
"""Device time of vch1d_hessvec (order 1: the exact gradient; order 2: gradient and H h) beside vch1d_second_order (order 2)
and vch1d_forward on the same context, for the two shapes of DESIGN.md 10b / 10c: N = 4096, M = 1000 at batch 1 and
N = 256, M = 100 at batch 256.  Median of `reps` from vch_stats.seconds.  One JSON line per shape.
   python scripts/hessvec_1d_timing.py [reps]"""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import vch_amd

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
SHAPES = [dict(N=4096, M=1000, dt=1e-3, B=1), dict(N=256, M=100, dt=5e-3, B=256)]

for s in SHAPES:
    N, M, dt, B = s["N"], s["M"], s["dt"], s["B"]
    tg, dts = vch_amd.time_grid(M * dt, dt)
    t = np.concatenate([[0.0], tg])
    rows = len(t)
    x = np.linspace(0.0, 1.0, N + 1)
    eng = vch_amd.Engine1D(N=N, batch=B, max_steps=len(dts))
    phi0 = np.stack([0.2 * np.cos(np.pi * x + 0.4 * b) for b in range(B)])
    U = np.stack([5.0 * np.cos(np.pi * x * (1 + b % 3))[None, :] * np.sin(1 + 0.01 * np.arange(rows) + b)[:, None] for b in range(B)])
    rng = np.random.default_rng(0)
    H = rng.standard_normal((B, rows, N + 1)) * np.cos(0.3 * np.arange(rows))[None, :, None]
    opt = vch_amd.make_opt()
    sec = dict(forward=[], second_order2=[], hessvec1=[], hessvec2=[])
    for _ in range(REPS):
        phi, st = eng.forward(phi0, dts, u=U, store=False)
        sec["forward"].append(st["seconds"])
        so = eng.second_order(H, t, opt, u=U, dt=dts, order=2)
        sec["second_order2"].append(so["stats"]["seconds"])
        for order in (1, 2):
            r = eng.hessvec(H, t, opt, u=U, dt=dts, order=order)
            sec[f"hessvec{order}"].append(r["stats"]["seconds"])
    med = {k: float(np.median(v)) for k, v in sec.items()}
    print(json.dumps(dict(cfg=dict(N=N, steps=len(dts), dt=dt, batch=B), seconds=med, all=sec,
                          hessvec_solves=r["stats"]["linear_solves"],
                          hessvec2_over_second_order2=med["hessvec2"] / med["second_order2"],
                          hessvec1_over_second_order2=med["hessvec1"] / med["second_order2"],
                          hessvec2_over_forward=med["hessvec2"] / med["forward"],
                          hessvec1_over_forward=med["hessvec1"] / med["forward"],
                          hHh_minus_curvature=float(r["hHh"][0] - so["curvature"][0]), curvature_sample=float(so["curvature"][0]))),
          flush=True)
    eng.close()
