#!/usr/bin/env python3
"""Per-call time of the 2D prox in each sparsity mode (Engine2D.pgd_init(sparsity=...)) against the node-wise
k_grad_prox on the same context: the `gradprox` bucket of Engine2D.pgd_iterate (device events around the prox launches, the
fold of their change sums included) over ITERS iterations, divided by the prox calls made (one per line-search round),
after an untimed init + iterations of every mode on that context.  Shapes: 256^2 x 100 steps x 8 and the benchmark's
512^2 x 1000 x 8.  kappa_sparsity is set per mode from the adjoint at u = 0 (the median of its node values / level norms /
pencil norms, so that about half the groups vanish) and the box from its step, so that part of the live groups is held by it.
At the first shape the groups of trajectory 0's first prox call (u = 0, alpha = alpha0) are classified on the host and a
NumPy port of gp_step counts the steps of the box-active ones.  One JSON line per (shape, mode).
   python scripts/dirsparse_2d_timing.py [--small-only]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vch_amd

F2 = vch_amd.module("Vch_control_2D.Forward2_solver")
G2 = vch_amd.module("Vch_control_2D.GD2_configured")

ITERS, ALPHA0 = 3, 50.0


def trapz_w(t):
    w = np.zeros(t.size)
    d = np.diff(t)
    w[:-1] += 0.5 * d
    w[1:] += 0.5 * d
    return w


def gp_steps(V, w, lam, lo, hi, cap=100):
    """The kinds of the groups V (G, m) under the weights w and, for the box-active ones, the steps gp_step takes (a port of
    csrc/vch_gp.h, all groups side by side)."""
    cone = V.copy()
    if hi == 0.0:
        cone[cone > 0] = 0.0
    if lo == 0.0:
        cone[cone < 0] = 0.0
    live = np.sqrt((w * cone * cone).sum(axis=1)) > lam
    with np.errstate(divide="ignore", invalid="ignore"):
        s0 = np.where(live, 1.0 - lam / np.sqrt((w * V * V).sum(axis=1)), 0.0)
    box = live & ((s0 * V.max(axis=1) > hi) | (s0 * V.min(axis=1) < lo))
    Vb, s = V[box], s0[box]
    a, b, steps, act = np.zeros(s.size), np.ones(s.size), np.zeros(s.size, dtype=int), np.ones(s.size, dtype=bool)
    for _ in range(cap):
        if not act.any():
            break
        sv = s[:, None] * Vb
        cl = np.clip(sv, lo, hi)
        Q, A = (w * cl * cl).sum(axis=1), (w * Vb * Vb * (cl == sv)).sum(axis=1)
        rho = np.sqrt(Q)
        h = rho * (1.0 - s) - lam * s
        steps += act
        done = h == 0.0
        a, b = np.where(act & (h > 0), s, a), np.where(act & (h < 0), s, b)
        with np.errstate(divide="ignore", invalid="ignore"):
            dh = np.where(rho > 0, A * s / rho, 0.0) * (1.0 - s) - rho - lam
            st = -h / dh
        inside = lambda z: (z > a) & (z < b)
        sn = np.where(np.abs(st) < 0.25 * (b - a), s + 2.0 * st, s + st)
        sn = np.where(inside(sn), sn, s + st)
        sn = np.where(inside(sn), sn, a + 0.5 * (b - a))
        done |= ~inside(sn)
        s = np.where(act & ~done, sn, s)
        act &= ~done
    return dict(groups=int(V.shape[0]), zero=int((~live).sum()), closed=int((live & ~box).sum()), box=int(box.sum()),
                steps_mean=float(steps.mean()) if steps.size else 0.0, steps_max=int(steps.max()) if steps.size else 0)


def main():
    shapes = [(256, 100, 1e-2, 8)] + ([] if "--small-only" in sys.argv else [(512, 1000, 1e-3, 8)])
    for N, M, DT, B in shapes:
        t, dts = vch_amd.time_grid(M * DT, DT)
        x = np.linspace(0.0, 1.0, N + 1)
        phi0 = np.stack([F2.init_phi_random(N, N, 1e-2, amp=0.1, seed=42 + b) for b in range(B)])
        phi_T = np.repeat(G2.build_targets(x, x, t, phi0[0], 1.0, 1.0, M * DT, choice_t=1, choice_q=2)[0][None], B, axis=0)
        eng = vch_amd.Engine2D(Nx=N, Ny=N, batch=B, max_steps=len(dts))
        small = N <= 256
        if small:       # the adjoint at u = 0 places kappa_sparsity and the box
            eng.pgd_init(phi0, phi_T, t, vch_amd.make_opt(alpha_max=ALPHA0), T=M * DT)
            eng.pgd_kkt(refresh=True)
            r = eng.pgd_get("r")[0]
            W, wt = np.outer(trapz_w(x), trapz_w(x)).ravel(), trapz_w(t)
            flat = r.reshape(len(t), -1)
            ks = dict(full=float(np.median(np.abs(r))), time=float(np.median(np.sqrt((W * flat * flat).sum(axis=1)))),
                      space=float(np.median(np.sqrt((wt[:, None] * flat * flat).sum(axis=0)))))
            bound = float(ALPHA0 * np.quantile(np.abs(r), 0.9))
            main.ks, main.bound = ks, bound
        else:           # no history leaves the device at this size: kappa_sparsity and the box of the first shape
            ks, bound = main.ks, main.bound
        per_call = {}
        for rep in range(2):                      # rep 0 warms the context up in every mode (lazy buffers, code objects)
            for mode in vch_amd.Engine2D.SPARSITY:
                opt = vch_amd.make_opt(alpha_max=ALPHA0, kappa_sparsity=ks[mode], u_min=-bound, u_max=bound)
                eng.pgd_init(phi0, phi_T, t, [opt], T=M * DT, sparsity=mode)
                res = eng.pgd_iterate(ITERS)
                if rep == 0:
                    continue
                calls = int(np.sum(1 + res["attempts"].max(axis=0)))
                per_call[mode] = res["seconds"]["gradprox"] / calls
                k = eng.pgd_kkt(refresh=True)
                rec = dict(cfg=dict(N=N, steps=len(dts), batch=B, iters=ITERS), mode=mode, kappa_sparsity=ks[mode], box=bound,
                           prox_calls=calls, gradprox_seconds=res["seconds"]["gradprox"], per_call_ms=1e3 * per_call[mode],
                           ratio_to_full=per_call[mode] / per_call["full"], zero_share=float(np.mean(k["n_zero"] / k["total"])))
                if small and mode != "full":
                    v = -ALPHA0 * flat                # u = 0: v = -alpha0 r
                    V, w = (v, W) if mode == "time" else (np.ascontiguousarray(v.T), wt)
                    rec["first_call_groups_of_trajectory_0"] = gp_steps(V, w, ALPHA0 * ks[mode], -bound, bound)
                print(json.dumps(rec), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
