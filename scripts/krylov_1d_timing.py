#!/usr/bin/env python3
"""Seconds per Lanczos step of vch1d_hess_lanczos (device path: vch_stats.seconds / steps) against the host path of
reduced_hessian_extremes (one Engine1D.hessvec call plus the NumPy reorthogonalisation, wall clock per step), against
vch1d_hessvec order 2 alone (vch_stats.seconds) and with VCH_KRYLOV_NOCACHE=1, for the two shapes of DESIGN.md 10c:
N = 4096, M = 1000 at batch 1 and N = 256, M = 100 at batch 256.  k = 10, reorth 1 and 0, every node free, all in one
process, median of `reps`.  Writes profiles/krylov_1d_timing.txt (one JSON line per shape) and prints it.
   python scripts/krylov_1d_timing.py [reps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import vch_amd

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
K = 10
SHAPES = [dict(N=4096, M=1000, dt=1e-3, B=1), dict(N=256, M=100, dt=5e-3, B=256)]
OUT = os.path.join("profiles", "krylov_1d_timing.txt")


def host_steps(eng, q0, t, opt, base, k):
    """k steps of the driver's host loop for every trajectory of the batch: one hessvec call per step, Gram-Schmidt twice
    against the whole basis in NumPy.  Returns (wall seconds per step, engine seconds per step)."""
    B = q0.shape[0]
    Q = [[q0[b] / np.linalg.norm(q0[b])] for b in range(B)]
    dev = 0.0
    t0 = time.perf_counter()
    for j in range(k):
        r = eng.hessvec(np.stack([Q[b][j] for b in range(B)]), t, opt, **base)
        dev += r["stats"]["seconds"]
        for b in range(B):
            w = r["hv"][b]
            for _ in range(2):
                for v in Q[b]:
                    w -= np.sum(v * w) * v
            Q[b].append(w / np.linalg.norm(w))
    return (time.perf_counter() - t0) / k, dev / k


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
    sec = dict(host_wall=[], host_engine=[], hessvec2=[], device_reorth1=[], device_reorth0=[], nocache_reorth1=[])
    stats = {}
    for nocache in (0, 1):
        if nocache:
            os.environ["VCH_KRYLOV_NOCACHE"] = "1"
        eng = vch_amd.Engine1D(N=N, batch=B, max_steps=len(dts))
        os.environ.pop("VCH_KRYLOV_NOCACHE", None)
        eng.forward(phi0, dts, u=U, store=False)
        base = dict(u=U, dt=dts)
        for _ in range(REPS):
            if nocache:
                L = eng.hess_lanczos(q0, K, t, opt, mask=mask, **base)
                sec["nocache_reorth1"].append(L["stats"]["seconds"] / K)
                stats["nocache_reorth1"] = L["stats"]
                continue
            wall, dev = host_steps(eng, q0, t, opt, base, K)
            sec["host_wall"].append(wall)
            sec["host_engine"].append(dev)
            sec["hessvec2"].append(eng.hessvec(q0, t, opt, **base)["stats"]["seconds"])
            for reorth in (1, 0):
                L = eng.hess_lanczos(q0, K, t, opt, mask=mask, reorth=bool(reorth), **base)
                assert list(L["steps"]) == [K] * B
                sec[f"device_reorth{reorth}"].append(L["stats"]["seconds"] / K)
                stats[f"device_reorth{reorth}"] = L["stats"]
        eng.close()
    med = {k: float(np.median(v)) for k, v in sec.items()}
    lines.append(json.dumps(dict(cfg=dict(N=N, steps=len(dts), dt=dt, batch=B, k=K), seconds_per_step=med, all=sec, stats=stats,
                                 host_over_device=med["host_wall"] / med["device_reorth1"],
                                 device_over_hessvec2=med["device_reorth1"] / med["hessvec2"],
                                 device0_over_hessvec2=med["device_reorth0"] / med["hessvec2"],
                                 nocache_over_hessvec2=med["nocache_reorth1"] / med["hessvec2"])))
    print(lines[-1], flush=True)
with open(OUT, "w") as fh:
    fh.write("scripts/krylov_1d_timing.py: seconds per Lanczos step, k = %d, median of %d; the device path's seconds include the "
             "set-up launch (mask, q_0, the gradient sweep once) spread over the k steps\n" % (K, REPS))
    fh.write("\n".join(lines) + "\n")
