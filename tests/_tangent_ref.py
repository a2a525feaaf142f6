"""CPU reference of the tangent (linearised) march behind the exact second-order check, built from the oracle's assembled
Newton matrix and a sparse direct solve.  Shared by test_tangent_cpu.py (which pins it against central differences of the
oracle's nonlinear march) and test_gpu_second_order.py (which compares the engine with it).

With dphi_0 = dmu_0 = dw_0 = 0 and d2phi_0 = d2mu_0 = 0, per step n (dt = t_{n+1} - t_n), with s_n the shift the march's
mass fix subtracted at the end of step n ON THE NODES OF ITS SET I_n ONLY (the interior nodes |phi_c| < 1 - delta_sep - 5e-3 of
the clipped Newton solution phi_c; every node in the all-node form), phi* = phi_{n+1} + (s_n on I_n, 0 elsewhere) the Newton
solution before it, J = jac_matrix(phi*):
    dw'  = w_filter(dw, dt, gamma, h_n, h_{n+1})                       rows (n, n+1) while n < len(h) - 1, zeros afterwards
    J [dphi*; dmu']   = [tau dphi/dt + kappa/2 L dphi + 2 c2 dphi + dmu/2 + (dw' + dw)/2 ;  dphi/dt + L dmu / 2]
    J [d2phi*; d2mu'] = [tau d2phi/dt + kappa/2 L d2phi + 2 c2 d2phi + d2mu/2 - c1 rho(phi*) dphi*^2 ;  d2phi/dt + L d2mu / 2]
    rho(p) = 4 p / (1 - p^2)^2
    dphi' = dphi* - sum(wts dphi*) / W_int,   d2phi' = d2phi* - sum(wts d2phi*) / W_int       (where s_n != 0)
wts = hx hy outer(trapz_x, trapz_y) are the mass fix's own weights and W_int their sum over I_n, on which alone the mean
is subtracted; dmu' and dw' are carried as they are, like the march carries mu (F2:579).  I_n is the march's own (`masks`,
from o.forward's stats): it is NOT recoverable from phi_{n+1} and s_n -- a skipped node within |s_n| of the threshold looks
like an interior one that was shifted outward -- so the re-derivation |phi_{n+1} + s_n| < 1 - delta_sep - 5e-3 (masks=None)
is right only where no skipped node lies that close.  The mass fix is NOT the identity: the linearised step conserves the mass of dphi only in the weights
of the Laplacian (its Kronecker-order quirk, oracle.lap), which are the fix's weights only for Nx == Ny.  The clip is taken
as the identity (callers assert max|phi_c| < 1 - delta_sep) and the set I_n as locally constant in u."""
import numpy as np
from scipy.sparse.linalg import splu

from oracle import vch2d_oracle as o

KEYS = ("s_state", "s_ctrl", "c_gn", "c_state", "c_ctrl", "n_h")


def march_with_shifts(P, **kw):
    """o.forward plus the per-step shifts of its mass fix: (phi_hist, (x, y), t_hist, shifts)."""
    st = {}
    phi, xy, t = o.forward(P, stats=st, **kw)
    return phi, xy, t, np.array(st.get("mass_shifts", []), dtype=float)


THR = 1.0 - o.DELTA_SEP - 5e-3


def march_with_fix(P, **kw):
    """o.forward plus everything its mass fix did: (phi_hist, (x, y), t_hist, shifts, fix) with fix = dict(masks=the M boolean
    planes the shift was subtracted on, w_int=the M weights it divided by, interior=the M flags "interior form",
    phi_c=the M clipped Newton solutions the sets were read from, newton_its=per-step residual counts)."""
    st = {}
    phi, xy, t = o.forward(P, stats=st, **kw)
    fix = dict(masks=np.array(st["mass_masks"]), w_int=np.array(st["mass_w_int"]),
               interior=np.array(st["mass_shift_interior"]), phi_c=np.array(st["phi_clipped"]),
               newton_its=np.array([c[0] for c in st["step_counts"]]))
    return phi, xy, t, np.array(st["mass_shifts"], dtype=float), fix


def fix_sets(phi_hist, shifts, masks=None, pstar_all=False):
    """Per step (phi*, I_n).  masks None: I_n re-derived as |phi_{n+1} + s_n| < THR (every node where that leaves none: the
    all-node form), which is what can be known from the history and the shifts alone.  pstar_all: phi* = phi_{n+1} + s_n at
    every node (the scheme as it was; for the tests that show the difference)."""
    out = []
    for k, s in enumerate(shifts):
        p1 = phi_hist[k + 1]
        if masks is None:
            I = np.abs(p1 + s) < THR
            if not I.any():
                I = np.ones(p1.shape, dtype=bool)
        else:
            I = np.asarray(masks[k], dtype=bool)
        out.append((p1 + s if pstar_all else p1 + np.where(I, s, 0.0), I))
    return out


def tangent_reference(P, phi_hist, t_hist, h, shifts=None, masks=None, pstar_all=False):
    """(dphi_hist, d2phi_hist), both shaped like phi_hist, for the direction h (rows, Nx+1, Ny+1).  `shifts` (M,): what the
    march's mass fix subtracted at the end of each step (None or zeros: the fix taken as the identity); `masks`, `pstar_all`:
    fix_sets."""
    Nx, Ny = int(P.Nx), int(P.Ny)
    hx, hy = P.Lx / Nx, P.Ly / Ny
    L = o.lap_matrix(Nx, Ny, hx, hy)
    n = (Nx + 1) * (Ny + 1)
    M = len(t_hist) - 1
    shifts = np.zeros(M) if shifts is None else np.asarray(shifts, dtype=float)
    assert shifts.shape == (M,)
    wts = hx * hy * np.outer(o.trapz_weights(Nx + 1), o.trapz_weights(Ny + 1))
    sets = fix_sets(phi_hist, shifts, masks, pstar_all)
    d1 = np.zeros_like(phi_hist)
    d2 = np.zeros_like(phi_hist)
    z = np.zeros(phi_hist.shape[1:])
    dphi, dmu, dw, ephi, emu = z, z, z, z, z

    def rhs(a, m, dt):
        return (P.tau * a / dt + 0.5 * P.kappa * o.lap(a, hx, hy) + 2.0 * P.c2 * a + 0.5 * m,
                a / dt + 0.5 * o.lap(m, hx, hy))

    def solve(J, rp, rm):
        s = J.solve(np.concatenate([rp.ravel(), rm.ravel()]))
        return s[:n].reshape(z.shape), s[n:].reshape(z.shape)

    def unmean(a, interior):
        a = a.copy()
        a[interior] -= np.sum(wts * a) / float(np.sum(wts[interior]))
        return a

    for k in range(M):
        dt = float(t_hist[k + 1] - t_hist[k])
        hn, hp = (h[k], h[k + 1]) if k < h.shape[0] - 1 else (z, z)
        dw_new = o.w_filter(dw, dt, P.gamma, hn, hp)
        p, interior = sets[k]
        J = splu(o.jac_matrix(p, dt, P, L).tocsc())         # one factorisation serves both solves of the step
        rp, rm = rhs(dphi, dmu, dt)
        nphi, nmu = solve(J, rp + 0.5 * (dw_new + dw), rm)
        rp, rm = rhs(ephi, emu, dt)
        ephi, emu = solve(J, rp - P.c1 * (4.0 * p / (1.0 - p * p) ** 2) * nphi ** 2, rm)
        if shifts[k] != 0.0:
            nphi, ephi = unmean(nphi, interior), unmean(ephi, interior)
        dphi, dmu, dw = nphi, nmu, dw_new
        d1[k + 1], d2[k + 1] = dphi, ephi
    return d1, d2


def pad_rows(a, rows):
    """a cut or zero-padded to `rows` leading rows (a direction or control counts as zero beyond its last row)."""
    out = np.zeros((rows,) + a.shape[1:])
    k = min(rows, a.shape[0])
    out[:k] = a[:k]
    return out


def tangent_scalars(phi_hist, d1, d2, u, h, phi_Q, phi_T, x, y, t_hist, b1, b2, b3):
    """The six scalars of the second-order call plus slope and curvature, with the cost's nested trapezoid rule."""
    rows = phi_hist.shape[0]
    u, h = pad_rows(u, rows), pad_rows(h, rows)
    sp_int = lambda f: o._trapz(o._trapz(f, y, -1), x, -1)
    tt = lambda f: o._trapz(sp_int(f), t_hist)
    e, eT = phi_hist - phi_Q, phi_hist[-1] - phi_T
    r = dict(s_state=b1 * tt(e * d1) + b2 * sp_int(eT * d1[-1]),
             s_ctrl=b3 * tt(u * h),
             c_gn=b1 * tt(d1 * d1) + b2 * sp_int(d1[-1] ** 2),
             c_state=b1 * tt(e * d2) + b2 * sp_int(eT * d2[-1]),
             c_ctrl=b3 * tt(h * h),
             n_h=tt(h * h))
    r = {k: float(v) for k, v in r.items()}
    r["slope"] = r["s_state"] + r["s_ctrl"]
    r["curvature"] = r["c_gn"] + r["c_state"] + r["c_ctrl"]
    return r
