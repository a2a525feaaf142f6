#!/usr/bin/env python3
"""One PGD iteration of the 1D engine in each sparsity mode (Engine1D.pgd_init(sparsity=...)) on the same
problem: the `seconds` buckets of Engine1D.pgd_iterate (adjoint sweep, optimistic round, backtracking rounds) over ITERS
iterations, after one untimed init + iterations on the same context.  Shapes: N = 4096 x 1000 steps at batch 1 and N = 256
x 100 steps at batch 256.  kappa_sparsity is set per mode from the adjoint at u = 0, the median of its node values / row
norms / column norms, so that about half the groups vanish in every mode.  One JSON line per (shape, mode).
   python scripts/dirsparse_1d_timing.py"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vch_amd

F1 = vch_amd.module("Vch_control_1D.Forward_solver")
G1 = vch_amd.module("Vch_control_1D.GD_1D")

ITERS = 2


def trapz_w(t):
    w = np.zeros(t.size)
    d = np.diff(t)
    w[:-1] += 0.5 * d
    w[1:] += 0.5 * d
    return w


for N, M, DT, B in ((4096, 1000, 1e-3, 1), (256, 100, 5e-3, 256)):
    tg, dts = vch_amd.time_grid(M * DT, DT)
    t = np.concatenate([[0.0], tg])
    x = np.linspace(0.0, 1.0, N + 1)
    phi0 = np.stack([F1.init_phi_random(N, 1e-2, amp=0.01, seed=42 + b) for b in range(B)])
    phi_T = np.repeat(G1.build_targets_1d(x, t, phi0[0], 1.0, M * DT, choice_q=2)[0][None], B, axis=0)
    eng = vch_amd.Engine1D(N=N, batch=B, max_steps=len(dts))
    eng.pgd_init(phi0, phi_T, t, dts, vch_amd.make_opt(alpha_max=100.0), x=x)
    eng.pgd_kkt(refresh=True)
    r = eng.pgd_get("r").reshape(B, len(t), N + 1)[0]
    ks = dict(full=float(np.median(np.abs(r[1:]))), time=float(np.median(np.sqrt((trapz_w(x) * r * r).sum(axis=1))[1:])),
              space=float(np.median(np.sqrt((trapz_w(t)[:, None] * r * r).sum(axis=0)))))
    for mode in vch_amd.Engine1D.SPARSITY:
        opt = vch_amd.make_opt(alpha_max=100.0, kappa_sparsity=ks[mode])
        for rep in range(2):                  # rep 0 warms the context up (lazy buffers, code objects)
            eng.pgd_init(phi0, phi_T, t, dts, [opt], x=x, sparsity=mode)
            res = eng.pgd_iterate(ITERS)
        k = eng.pgd_kkt(refresh=True)
        print(json.dumps(dict(cfg=dict(N=N, steps=len(dts), batch=B, iters=ITERS), mode=mode, kappa_sparsity=ks[mode],
                              seconds=res["seconds"], total=float(sum(res["seconds"].values())),
                              trials=np.bincount(res["trials"].ravel()).tolist(),
                              zero_share=float(np.mean(k["n_zero"] / k["total"])))), flush=True)
    eng.close()
