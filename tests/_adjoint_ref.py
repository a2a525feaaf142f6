"""CPU reference of the discrete adjoint of the tangent march (tests/_tangent_ref.py): the exact gradient field
G = d(J1+J2+J3)/du and the Hessian-vector product H h as Euclidean fields, in the PLAIN-transpose form -- every transposed
solve is a sparse direct solve with jac_matrix(...).T and every transposed stencil is lap_matrix(...).T -- so that the
engine's scaled form (J^T = S J S^-1) is checked against an independent one.

Backward sweep, k = M-1 .. 0, on the flat memory of the (Nx+1, Ny+1) arrays (the layout the Laplacian acts on):
    lam_phi += wt[k+1] b1 Wc e[k+1]                         (+ b2 Wc (phi_M - phi_T) at k = M-1)
    lam_v    = lam_phi - wts sum_int(lam_phi) / W_k         (where s_k != 0: transpose of the linearised mass fix)
    J(phi*)^T [yp; ym] = [lam_v; lam_mu]
    lam_dw   = yp / 2 + lam_w;   G[k] += beta lam_dw,  G[k+1] += beta lam_dw        (while k < g_rows - 1)
    lam     <- (Kp^T yp + ym / dt,  yp / 2 + L^T ym / 2,  yp / 2 + alpha lam_dw)
second order beside it, with v_k the tangent's dphi* of step k BEFORE its mean removal and dphi' its history after it:
    Lam_phi += wt[k+1] b1 Wc dphi'[k+1]                     (+ b2 Wc dphi'_M)
    Lam_v    = Lam_phi - wts sum_int(Lam_phi) / W_k - c1 rho(phi*) yp v_k
    the same solve and updates into Hh (while k < h_rows - 1)
G starts as b3 wt (x) Wc u and Hh as b3 wt (x) Wc h.  J'(u)h = sum G h and J''(u)[h,h] = sum h Hh are plain node sums."""
import numpy as np
from scipy.sparse.linalg import splu

from oracle import vch2d_oracle as o
from _tangent_ref import fix_sets


def trapz_w(x):
    """Weights w with sum(w f) = np.trapz(f, x)."""
    x = np.asarray(x, dtype=float)
    w = np.zeros(x.size)
    d = np.diff(x)
    w[:-1] += d / 2.0
    w[1:] += d / 2.0
    return w


def adjoint_reference(P, phi_hist, t_hist, shifts, u, phi_Q, phi_T, x, y, b1, b2, b3, h=None, g_rows=None,
                      rho_source=True, fix_transpose=True, cache=None, masks=None, pstar_all=False):
    """(G, Hh): G (g_rows, Nx+1, Ny+1) and, with a direction h (h_rows, Nx+1, Ny+1), Hh shaped like h (else None).
    u: the control of the march (rows beyond its last count as zero; None = zero control).  The two switches leave a term
    of the scheme out, for the tests that show the term is needed.  cache: a dict that keeps the factorisations between calls
    about one base point (a dense Hessian is one call per unit direction).  masks, pstar_all: the nodes the march's mass fix
    shifted and phi* on the others (_tangent_ref.fix_sets)."""
    Nx, Ny = int(P.Nx), int(P.Ny)
    hx, hy = P.Lx / Nx, P.Ly / Ny
    shape = phi_hist.shape[1:]
    n = shape[0] * shape[1]
    M = len(t_hist) - 1
    shifts = np.zeros(M) if shifts is None else np.asarray(shifts, dtype=float)
    L = o.lap_matrix(Nx, Ny, hx, hy).tocsr()
    LT = L.T.tocsr()
    wts = (hx * hy * np.outer(o.trapz_weights(Nx + 1), o.trapz_weights(Ny + 1))).ravel()
    Wc = np.outer(trapz_w(x), trapz_w(y)).ravel()
    wt = trapz_w(t_hist)
    if g_rows is None:
        g_rows = M + 1 if u is None else min(u.shape[0], M + 1)
    phi = phi_hist.reshape(M + 1, n)
    pq = np.zeros_like(phi) if phi_Q is None else np.asarray(phi_Q).reshape(M + 1, n)
    pT = np.zeros(n) if phi_T is None else np.asarray(phi_T).reshape(n)
    G = np.zeros((g_rows, n))
    if u is not None:
        r = min(g_rows, u.shape[0])
        G[:r] = b3 * wt[:r, None] * Wc * u[:r].reshape(r, n)

    sets = fix_sets(phi_hist, shifts, masks, pstar_all)
    pstar = [p.reshape(n) for p, _ in sets]
    interior = [I.reshape(n) for _, I in sets]
    dts = [float(t_hist[k + 1] - t_hist[k]) for k in range(M)]

    cache = {} if cache is None else cache

    def lu(k, transposed):
        key = (k, transposed)
        if key not in cache:
            J = o.jac_matrix(pstar[k].reshape(shape), dts[k], P, L)
            cache[key] = splu((J.T if transposed else J).tocsc())
        return cache[key]

    Hh = V = DP = None
    if h is not None:
        h_rows = h.shape[0]
        hf = h.reshape(h_rows, n)
        Hh = b3 * wt[:h_rows, None] * Wc * hf
        # the order-1 tangent of h, keeping each step's raw solve output
        V, DP = np.zeros((M, n)), np.zeros((M + 1, n))
        dphi, dmu, dw = np.zeros(n), np.zeros(n), np.zeros(n)
        z = np.zeros(n)
        for k in range(M):
            dt = dts[k]
            hn, hp = (hf[k], hf[k + 1]) if k < h_rows - 1 else (z, z)
            dw_new = o.w_filter(dw, dt, P.gamma, hn, hp)
            J = lu(k, False)
            A = P.tau * dphi / dt + 0.5 * P.kappa * (L @ dphi) + 2.0 * P.c2 * dphi + 0.5 * dmu + 0.5 * (dw_new + dw)
            Bv = dphi / dt + 0.5 * (L @ dmu)
            s = J.solve(np.concatenate([A, Bv]))
            v, dmu, dw = s[:n], s[n:], dw_new
            V[k] = v
            dphi = v.copy()
            if shifts[k] != 0.0:
                dphi[interior[k]] -= np.sum(wts * v) / float(np.sum(wts[interior[k]]))
            DP[k + 1] = dphi

    def fixT(lam, k):
        if shifts[k] == 0.0 or not fix_transpose:
            return lam
        return lam - wts * (np.sum(lam[interior[k]]) / float(np.sum(wts[interior[k]])))

    lam = [np.zeros(n), np.zeros(n), np.zeros(n)]
    Lam = [np.zeros(n), np.zeros(n), np.zeros(n)]
    for k in range(M - 1, -1, -1):
        dt = dts[k]
        g = P.gamma / dt
        alpha, beta = (g - 0.5) / (g + 0.5), 0.5 / (g + 0.5)
        JT = lu(k, True)
        kp = P.tau / dt + 2.0 * P.c2

        def back(lm, src, extra, out, rows):
            lphi = lm[0] + src
            s = JT.solve(np.concatenate([fixT(lphi, k) + extra, lm[1]]))
            yp, ym = s[:n], s[n:]
            ldw = 0.5 * yp + lm[2]
            if k < rows - 1:
                out[k] += beta * ldw
                out[k + 1] += beta * ldw
            return yp, [kp * yp + 0.5 * P.kappa * (LT @ yp) + ym / dt, 0.5 * yp + 0.5 * (LT @ ym), 0.5 * yp + alpha * ldw]

        src = wt[k + 1] * b1 * Wc * (phi[k + 1] - pq[k + 1])
        if k == M - 1:
            src = src + b2 * Wc * (phi[M] - pT)
        yp, lam = back(lam, src, 0.0, G, g_rows)
        if h is not None:
            src = wt[k + 1] * b1 * Wc * DP[k + 1]
            if k == M - 1:
                src = src + b2 * Wc * DP[M]
            p = pstar[k]
            extra = -P.c1 * (4.0 * p / (1.0 - p * p) ** 2) * yp * V[k] if rho_source else 0.0
            _, Lam = back(Lam, src, extra, Hh, h.shape[0])
    G = G.reshape((g_rows,) + shape)
    return G, (None if h is None else Hh.reshape(h.shape))
