"""CPU reference of the 1D tangent (linearised) march behind vch1d_second_order, built from the oracle's Newton matrix
(o.newton_rows) and its high-precision banded solve (o.hp_solve: banded LU is not componentwise stable on this matrix,
DESIGN.md 4b, so plain solve_banded would not do as a reference at N ~ 1000-2000).  Shared by test_tangent_cpu_1d.py (which
pins it against central differences of the oracle's nonlinear march) and test_gpu_second_order_1d.py (which compares the
engine with it).

The history has rows = M + 2 rows (t = 0 twice, F1:329-336).  Step n = 0..M-1 takes row n+1 to row n+2 with dt_n, driven by
the direction rows (h_n, h_{n+1}) (F1:347-353); phi* = phi_hist[n+2], J = the matrix of o.jac_dense / o.newton_rows.  All
tangent fields start at zero; per step:
    dw'  = w_filter(dw, dt, gamma, h_n, h_{n+1})
    J [dphi*; dmu']   = [tau dphi/dt + kappa/2 L dphi + 2 c2 dphi + dmu/2 + (dw' + dw)/2 ;  dphi/dt + L dmu / 2]
    J [d2phi*; d2mu'] = [tau d2phi/dt + kappa/2 L d2phi + 2 c2 d2phi + d2mu/2 - c1 rho(phi*) dphi*^2 ;  d2phi/dt + L d2mu / 2]
    rho(p) = 4 p / (1 - p^2)^2
    dphi' = dphi* - sum(wts dphi*) / Lx,   d2phi' = d2phi* - sum(wts d2phi*) / Lx,      wts = h trapz
The concave term -2 c2 phi_old is explicit in 1D (F1:99-109): +2 c2 dphi is on the right-hand side.  The mean removal is the
linearisation of the uniform mass shift (F1:366); the clip (F1:361) is taken as the identity (callers assert
max|phi| < 1 - delta_sep - 0.1)."""
import numpy as np

from oracle import vch1d_oracle as o

KEYS = ("s_state", "s_ctrl", "c_gn", "c_state", "c_ctrl", "n_h")


def tangent_reference_1d(P, phi_hist, t_hist, h, dts=None, omit=()):
    """(dphi_hist, d2phi_hist), both shaped like phi_hist (rows, N+1), for the direction h (rows, N+1).  dts (M,): the
    step sizes (None: t_hist[n+2] - t_hist[n+1]).  `omit` drops a term of the scheme, for the tests that show the check can
    fail: "rho" the source -c1 rho(phi*) dphi*^2 of the second solve, "c2" the explicit +2 c2 dphi of the first."""
    rows, n = phi_hist.shape
    M = rows - 2
    hx = P.Lx / (n - 1)
    assert h.shape == phi_hist.shape and len(t_hist) == rows
    wts = hx * o.trapz_weights(n)
    d1, d2 = np.zeros_like(phi_hist), np.zeros_like(phi_hist)
    z = np.zeros(n)
    dphi, dmu, dw, ephi, emu = z, z, z, z, z
    c2_first = 0.0 if "c2" in omit else 2.0 * P.c2

    def solve(J, rp, rm):
        b = np.empty(2 * n)
        b[0::2], b[1::2] = rp, rm
        s = o.hp_solve(J, b)
        return s[0::2].copy(), s[1::2].copy()

    for k in range(M):
        dt = float(t_hist[k + 2] - t_hist[k + 1]) if dts is None else float(dts[k])
        p = phi_hist[k + 2]
        J = o.newton_rows(p, dt, P, hx)
        dw_new = o.w_filter(dw, dt, P.gamma, h[k], h[k + 1])
        rp = P.tau * dphi / dt + 0.5 * P.kappa * o.lap(dphi, hx) + c2_first * dphi + 0.5 * dmu + 0.5 * (dw_new + dw)
        nphi, nmu = solve(J, rp, dphi / dt + 0.5 * o.lap(dmu, hx))
        rp = P.tau * ephi / dt + 0.5 * P.kappa * o.lap(ephi, hx) + 2.0 * P.c2 * ephi + 0.5 * emu
        if "rho" not in omit:
            rp = rp - P.c1 * (4.0 * p / (1.0 - p * p) ** 2) * nphi ** 2
        nephi, nemu = solve(J, rp, ephi / dt + 0.5 * o.lap(emu, hx))
        dphi, dmu, dw = nphi - np.dot(wts, nphi) / P.Lx, nmu, dw_new
        ephi, emu = nephi - np.dot(wts, nephi) / P.Lx, nemu
        d1[k + 2], d2[k + 2] = dphi, ephi
    return d1, d2


def tangent_scalars_1d(phi_hist, d1, d2, u, h, phi_Q, phi_T, x, t_hist, b1, b2, b3):
    """The six scalars of the second-order call plus slope and curvature, with the cost's quadrature (C1:55-73): trapezoid
    in x, then in t_hist over all rows."""
    sp = lambda f: o._trapz(f, x, -1)
    tt = lambda f: o._trapz(sp(f), t_hist)
    e, eT = phi_hist - phi_Q, phi_hist[-1] - phi_T
    r = dict(s_state=b1 * tt(e * d1) + b2 * sp(eT * d1[-1]),
             s_ctrl=b3 * tt(u * h),
             c_gn=b1 * tt(d1 * d1) + b2 * sp(d1[-1] ** 2),
             c_state=b1 * tt(e * d2) + b2 * sp(eT * d2[-1]),
             c_ctrl=b3 * tt(h * h),
             n_h=tt(h * h))
    r = {k: float(v) for k, v in r.items()}
    r["slope"] = r["s_state"] + r["s_ctrl"]
    r["curvature"] = r["c_gn"] + r["c_state"] + r["c_ctrl"]
    return r


# The driver-level setup shared by the CPU pin (which measures how far the central second difference of the oracle's cost
# is from the exact curvature) and the GPU test of exact_second_order_condition (which holds the engine to 10 x that).
DRIVER = dict(N=32, T=0.1, dt=0.02, seed=7, num_directions=3, eps=3e-2, u_min=-1.0, u_max=1.0)


def driver_problem():
    """(P, phi0, u_star, r_star): N = 32, 5 steps, defaults; the smooth start 0.2 cos(pi x), a control of amplitude 1.4
    clipped to the box [-1, 1] (so that the critical cone is not the whole space) and a smooth stand-in for the adjoint."""
    D = DRIVER
    P = o.Params1D(N=D["N"], T=D["T"], dt_initial=D["dt"])
    x = np.linspace(0.0, P.Lx, P.N + 1)
    rows = int(round(D["T"] / D["dt"])) + 2
    u_star = np.clip(np.stack([1.4 * np.cos(np.pi * x * (1 + k % 3)) * np.sin(1 + k) for k in range(rows)]),
                     D["u_min"], D["u_max"])
    r_star = 1e-3 * np.stack([np.sin(np.pi * x) * (1 + k) for k in range(rows)])
    return P, 0.2 * np.cos(np.pi * x / P.Lx), u_star, r_star
