#!/usr/bin/env python3
"""Golden vectors of the 2D march at the benched grid, made by the CPU oracle (oracle/vch2d_oracle.py, itself pinned to
the reference by tests/test_oracle_golden_2d.py).  TEST INFRASTRUCTURE: imports only the oracle, writes .npz data files.

    python tests/golden/make_golden_plans.py

  g2d_march_512.npz   512^2 (fast-axis and slow-axis DCT-I of length 1024 on the engine's FFT path), amp = 0.1 start of seed
                      42, 4 steps of dt = 1e-3 under the control 3 (t/T) sin(2 pi x) cos(pi y) (the |u| ~ 3 shape of the line
                      search); the adjoint sweep on that history with the targets of build_targets(..., 1, 1).  Stores
                        phi_sub, r_sub        every level at a ::8 subsample
                        phi_lines_<k>         full rows phi[k][LINES, :] and columns phi[k][:, LINES] at levels 1 and M
                        r_lines_<k>           the same of r at levels 0 and M-1 (r[M] = 0)
                        phi_norm, phi_mass    per-level L2 norm (plain 2-norm of the field) and trapezoid mass; r likewise
                        step_counts           per step: residual norms recorded, linear solves, Armijo trials
                      LINES are the tile edges (64-node tiles), the workgroup boundaries and the last node.  One oracle Newton
                      step at this size takes about a minute (two SuperLU solves of the 526k-row Newton system).

The file is written with fixed zip timestamps, so a rerun reproduces it bit for bit.
"""
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
from oracle import vch2d_oracle as O2          # noqa: E402

LINES = np.array([0, 1, 2, 62, 63, 64, 65, 127, 128, 255, 256, 257, 510, 511, 512])


def save(name, **arrs):
    """np.savez layout (one .npy member per array, deflated) with a fixed member timestamp: byte-reproducible."""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrs):
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(zi, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrs[k]), allow_pickle=False)
    print(f"  wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB", flush=True)


def march_control(N, M, amp_u):
    xs = np.linspace(0.0, 1.0, N + 1)
    shape = np.sin(2 * np.pi * xs)[:, None] * np.cos(np.pi * xs)[None, :]
    return amp_u * np.linspace(0.0, 1.0, M + 1)[:, None, None] * shape[None]


def gen_march512():
    N, M, dt, seed, amp, amp_u = 512, 4, 1e-3, 42, 0.1, 3.0
    P = O2.Params2D(Nx=N, Ny=N, T=M * dt, dt_initial=dt)
    Op = O2.OptParams()
    u = march_control(N, M, amp_u)
    st = {}
    t0 = time.perf_counter()
    phi, (x, y), t = O2.forward(P, control=u, seed=seed, amp=amp, stats=st)
    assert phi.shape[0] == M + 1
    print(f"    forward: {time.perf_counter() - t0:.0f} s, per step (norms, solves, trials) {st['step_counts']}", flush=True)
    phi_T, phi_Q = O2.build_targets(x, y, t, phi[0].copy(), P.Lx, P.Ly, P.T, 1, 1)
    t0 = time.perf_counter()
    _, _, r = O2.backward(phi, x, y, t, P, Op.b1, Op.b2, phi_Q, phi_T)
    print(f"    backward: {time.perf_counter() - t0:.0f} s", flush=True)
    wts = np.outer(O2.trapz_weights(N + 1), O2.trapz_weights(N + 1)) / (N * N)
    out = dict(Nx=N, Ny=N, Lx=P.Lx, Ly=P.Ly, dt=dt, T=P.T, seed=seed, amp=amp, amp_u=amp_u, t_hist=t, lines=LINES,
               phi_sub=phi[:, ::8, ::8], r_sub=r[:, ::8, ::8],
               phi_norm=np.linalg.norm(phi.reshape(M + 1, -1), axis=1), phi_mass=np.sum(wts * phi, axis=(1, 2)),
               r_norm=np.linalg.norm(r.reshape(M + 1, -1), axis=1), r_mass=np.sum(wts * r, axis=(1, 2)),
               step_counts=np.array(st["step_counts"], dtype=np.int64))
    for k in (1, M):
        out[f"phi_rows_{k}"], out[f"phi_cols_{k}"] = phi[k][LINES, :], phi[k][:, LINES]
    for k in (0, M - 1):
        out[f"r_rows_{k}"], out[f"r_cols_{k}"] = r[k][LINES, :], r[k][:, LINES]
    save("g2d_march_512.npz", **out)


if __name__ == "__main__":
    gen_march512()
