#!/usr/bin/env python3
"""The three `seconds` buckets of Engine1D.pgd_iterate (adjoint sweep, optimistic round, backtracking rounds) at N = 256,
M = 100, B = 256 over 3 iterations with a single parameter set, after one untimed init + 3 iterations on the same context:
the A/B of the per-trajectory parameter table against the commit before it.  One JSON line.  Where the engine has
pgd_kkt, the wall time of one pgd_kkt(refresh=False) call (launch, kernel, 48 B bytes back) beside pulling u and r through
pgd_get and counting in NumPy.
   python scripts/pgd_1d_timing.py [label]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vch_amd

F1 = vch_amd.module("Vch_control_1D.Forward_solver")
G1 = vch_amd.module("Vch_control_1D.GD_1D")
K1 = vch_amd.module("Vch_control_1D.config")

LABEL = sys.argv[1] if len(sys.argv) > 1 else "run"
N, M, DT, B, ITERS = 256, 100, 5e-3, 256, 3
tg, dts = vch_amd.time_grid(M * DT, DT)
t = np.concatenate([[0.0], tg])
x = np.linspace(0.0, 1.0, N + 1)
phi0 = np.stack([F1.init_phi_random(N, 1e-2, amp=0.01, seed=42 + b) for b in range(B)])
phi_T = np.repeat(G1.build_targets_1d(x, t, phi0[0], 1.0, M * DT, choice_q=2)[0][None], B, axis=0)
O = K1.OptimizationConfig()
opt = vch_amd.make_opt(O)
eng = vch_amd.Engine1D(N=N, batch=B, max_steps=len(dts))
runs = []
for rep in range(2):                      # rep 0 warms the context up (lazy buffers, code objects)
    eng.pgd_init(phi0, phi_T, t, dts, opt, x=x)
    res = eng.pgd_iterate(ITERS)
    runs.append(res)
res = runs[-1]
out = dict(label=LABEL, cfg=dict(N=N, steps=len(dts), dt=DT, batch=B, iters=ITERS), seconds=res["seconds"],
           total=float(sum(res["seconds"].values())), trials=np.bincount(res["trials"].ravel()).tolist(),
           cost_sum=float(res["cost"][:, -1].sum()))
if hasattr(eng, "pgd_kkt"):
    kkt_s, np_s = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        k = eng.pgd_kkt(refresh=False)
        kkt_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        u, r = eng.pgd_get("u"), eng.pgd_get("r")
        z, s = np.abs(u) < 1e-6, np.abs(r) <= O.kappa_sparsity
        counts = np.stack([z.sum(axis=(1, 2)), s.sum(axis=(1, 2)), (z == s).sum(axis=(1, 2))], axis=1)
        np_s.append(time.perf_counter() - t0)
        assert np.array_equal(counts, np.stack([k["n_zero"], k["n_small"], k["n_match"]], axis=1))
    out["kkt_call_wall_s"] = float(np.median(kkt_s))
    out["pull_u_r_and_numpy_wall_s"] = float(np.median(np_s))
print(json.dumps(out), flush=True)
eng.close()
