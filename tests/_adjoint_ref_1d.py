"""CPU reference of the transposed tangent sweeps behind vch1d_hessvec: the exact gradient field G = d(J1+J2+J3)/du and
the Hessian-vector product H h of the discrete 1D cost, built from the oracle's Newton matrix (o.newton_rows) transposed
and its high-precision banded solve (o.hp_solve: plain banded LU is not componentwise stable on this matrix beyond
N ~ 1000).  Shared by test_adjoint_cpu_1d.py (which pins it against tests/_tangent_ref_1d.py by four
identities) and test_gpu_hessvec_1d.py (which compares the engine with it).

Notation of _tangent_ref_1d.py: rows = M + 2, step k = 0..M-1 takes history row k+1 to row k+2 with dt_k, driven by the
direction rows (h_k, h_{k+1}); phi* = phi_hist[k+2], J = the matrix of o.newton_rows.  The tangent step is a linear map on
(dphi, dmu, dw); the sweeps run its transpose backwards.  With wx the trapezoid weights of x, wt those of t_hist (row 0 has
weight 0), e = phi - phi_Q, al = (gamma/dt - 1/2)/(gamma/dt + 1/2), be = (1/2)/(gamma/dt + 1/2), Kp = (tau/dt + 2 c2) I +
kappa/2 L, all multipliers zero, G = b3 wt (x) wx . u, Hh = b3 wt (x) wx . h, and for k = M-1 .. 0:
    l_phi += wt[k+2] b1 wx . e[k+2]                   (+ b2 wx . (phi_M - phi_T) at k = M-1)
    l_v    = l_phi - wx sum(l_phi) / Lx               (transpose of the mean removal)
    J^T [yp; ym] = [l_v; l_mu]
    l_dw   = yp/2 + l_w;   G[k] += be l_dw;   G[k+1] += be l_dw
    (l_phi, l_mu, l_w) <- (Kp^T yp + ym/dt,  yp/2 + L^T ym / 2,  yp/2 + al l_dw)
  and beside it, with v_k = dphi* of step k of the tangent of h BEFORE its mean removal and dphi the tangent history:
    L_phi += wt[k+2] b1 wx . dphi[k+2]                (+ b2 wx . dphi_M at k = M-1)
    L_v    = L_phi - wx sum(L_phi) / Lx - c1 rho(phi*) yp v_k,         rho(p) = 4 p / (1 - p^2)^2
    J^T [Yp; Ym] = [L_v; L_mu];   Hh and (L_phi, L_mu, L_w) as above.
G and Hh are Euclidean: derivatives with respect to the entries of u, not divided by quadrature weights, so that
J'(u)h = sum(G h) and J''(u)[h,h] = sum(h Hh) as plain node sums."""
import numpy as np

from oracle import vch1d_oracle as o


def trapz_nodes(g):
    """np.trapezoid's weight of every node of the grid g."""
    w = np.zeros(len(g))
    d = np.diff(np.asarray(g, dtype=np.float64))
    w[:-1] += 0.5 * d
    w[1:] += 0.5 * d
    return w


def transpose_rows(rows):
    """Row-wise offset coefficients (o._rows_to_banded convention: rows[k + off][i] = A[i, i + off]) of A^T."""
    k = (len(rows) - 1) // 2
    n = rows[0].size
    out = tuple(np.zeros(n) for _ in rows)
    for off in range(-k, k + 1):
        i = np.arange(max(0, -off), min(n, n - off))
        out[k + off][i] = rows[k - off][i + off]            # A^T[i, i + off] = A[i + off, i]
    return out


def lap_t(v, hx):
    """L^T v for the mirrored-Neumann L of o.lap (not symmetric: rows 0 and n-1 carry a 2)."""
    lo, dg, up = o._lap_rows(v.size, hx)
    out = dg * v
    out[1:] += up[:-1] * v[:-1]
    out[:-1] += lo[1:] * v[1:]
    return out


def adjoint_reference_1d(P, phi_hist, t_hist, x, u, phi_Q, phi_T, b1, b2, b3, h=None, dts=None, omit=()):
    """(G, Hh), both shaped like phi_hist (rows, N+1); Hh is None without a direction h.  u / phi_Q (rows, N+1), phi_T
    (N+1,).  dts (M,): the step sizes (None: t_hist[k+2] - t_hist[k+1]).  `omit` drops a term of the scheme, for the test
    that shows the check can fail: "rho" the source -c1 rho(phi*) yp v_k of the second sweep."""
    rows, n = phi_hist.shape
    M = rows - 2
    hx = P.Lx / (n - 1)
    wx, wt = trapz_nodes(x), trapz_nodes(t_hist)
    step = lambda k: float(t_hist[k + 2] - t_hist[k + 1]) if dts is None else float(dts[k])

    def solve(Jrows, r0, r1):
        b = np.empty(2 * n)
        b[0::2], b[1::2] = r0, r1
        s = o.hp_solve(Jrows, b)
        return s[0::2].copy(), s[1::2].copy()

    second = h is not None
    wts_mass = hx * o.trapz_weights(n)
    V, D1 = np.zeros_like(phi_hist), np.zeros_like(phi_hist)
    if second:                                                      # the order-1 tangent of h, keeping v_k
        z = np.zeros(n)
        dphi, dmu, dw = z, z, z
        for k in range(M):
            dt = step(k)
            J = o.newton_rows(phi_hist[k + 2], dt, P, hx)
            dw_new = o.w_filter(dw, dt, P.gamma, h[k], h[k + 1])
            rp = P.tau * dphi / dt + 0.5 * P.kappa * o.lap(dphi, hx) + 2.0 * P.c2 * dphi + 0.5 * dmu + 0.5 * (dw_new + dw)
            v, nmu = solve(J, rp, dphi / dt + 0.5 * o.lap(dmu, hx))
            dphi, dmu, dw = v - np.dot(wts_mass, v) / P.Lx, nmu, dw_new
            V[k + 2], D1[k + 2] = v, dphi
    G = b3 * (wt[:, None] * wx[None, :]) * u
    Hh = b3 * (wt[:, None] * wx[None, :]) * h if second else None
    z = np.zeros(n)
    lphi, lmu, lw, Lphi, Lmu, Lw = z, z, z, z, z, z
    for k in range(M - 1, -1, -1):
        dt = step(k)
        g = P.gamma / dt
        al, be = (g - 0.5) / (g + 0.5), 0.5 / (g + 0.5)
        p = phi_hist[k + 2]
        JT = transpose_rows(o.newton_rows(p, dt, P, hx))
        kd = P.tau / dt + 2.0 * P.c2

        def back(yp, ym, lw_):
            ldw = 0.5 * yp + lw_
            return (be * ldw, kd * yp + 0.5 * P.kappa * lap_t(yp, hx) + ym / dt, 0.5 * yp + 0.5 * lap_t(ym, hx),
                    0.5 * yp + al * ldw)

        lphi = lphi + wt[k + 2] * b1 * wx * (p - phi_Q[k + 2])
        if k == M - 1:
            lphi = lphi + b2 * wx * (p - phi_T)
        yp, ym = solve(JT, lphi - wx * (lphi.sum() / P.Lx), lmu)
        if second:
            Lphi = Lphi + wt[k + 2] * b1 * wx * D1[k + 2]
            if k == M - 1:
                Lphi = Lphi + b2 * wx * D1[k + 2]
            Lv = Lphi - wx * (Lphi.sum() / P.Lx)
            if "rho" not in omit:
                Lv = Lv - P.c1 * (4.0 * p / (1.0 - p * p) ** 2) * yp * V[k + 2]
            Yp, Ym = solve(JT, Lv, Lmu)
            add, Lphi, Lmu, Lw = back(Yp, Ym, Lw)
            Hh[k] += add
            Hh[k + 1] += add
        add, lphi, lmu, lw = back(yp, ym, lw)
        G[k] += add
        G[k + 1] += add
    return G, Hh
