"""NumPy restatement of the directional sparsity functionals of the 2D engine on top of
_group_prox_ref.group_prox_many, which takes any (G, m) block of groups and any weight vector.

A control is (rows, Nx+1, Ny+1).  "time": group k is level k, ||z||^2 = sum_ij wx_i wy_j z_ij^2 (the product trapezoid
weights of x and y).  "space": group (i, j) is the pencil u[:, i, j], ||z||^2 = sum_k wt_k z_k^2 (the trapezoid weights of
t_hist).  The prox is taken in the L2(Q) metric, so the threshold lam = alpha kappa_s is the same for every group.  Nothing
here is shared with the engine.
"""
import numpy as np

import _group_prox_ref as G1

MODES = G1.MODES
trapz_w = G1.trapz_w


def plane_w(x, y):
    """W_ij = wx_i wy_j as one vector over the raveled plane."""
    return np.outer(trapz_w(x), trapz_w(y)).ravel()


def groups(a, mode):
    """(G, m) block of the groups of a (rows, nx1, ny1) array: the raveled levels, or the pencils as rows."""
    a = np.asarray(a)
    flat = a.reshape(a.shape[0], -1)
    return flat if mode == "time" else np.ascontiguousarray(flat.T)


def ungroup(blk, shape, mode):
    return blk.reshape(shape) if mode == "time" else np.ascontiguousarray(blk.T).reshape(shape)


def weights(mode, x, y, t_hist):
    return plane_w(x, y) if mode == "time" else trapz_w(t_hist)


def prox(u, r, alpha, b3, ks, lo, hi, mode, x, y, t_hist, dtype=np.float64):
    """(u+, s, kinds) of one (rows, nx1, ny1) control: the gradient step v = u - alpha (r + b3 u) in doubles, then the prox
    of the mode.  s is (rows,) for "time" and (nx1, ny1) for "space"; kinds is the flat list of group_prox_many."""
    u = np.asarray(u, dtype=np.float64)
    v = u - alpha * (r + b3 * u)
    out, s, kinds = G1.group_prox_many(groups(v, mode), weights(mode, x, y, t_hist), alpha * ks, lo, hi, dtype)
    return ungroup(out, u.shape, mode), (s if mode == "time" else s.reshape(u.shape[1:])), kinds


def group_norms(a, x, y, t_hist, mode):
    """||a_g|| of every group: (rows,) for "time", (nx1, ny1) for "space"."""
    a = np.asarray(a, dtype=np.float64)
    n = np.sqrt(np.sum(weights(mode, x, y, t_hist) * groups(a, mode) ** 2, axis=1))
    return n if mode == "time" else n.reshape(a.shape[1:])


def j4(u, x, y, t_hist, ks, mode):
    """kappa_s * trapezoid in t of ||u(., t)||_W ("time") or kappa_s sum_ij W_ij ||u[:, i, j]||_wt ("space")."""
    n = group_norms(u, x, y, t_hist, mode)
    outer = trapz_w(t_hist) if mode == "time" else plane_w(x, y)
    return ks * float(np.sum(outer * n.ravel()))


def cost(O2, phi, u, phi_Q, phi_T, x, y, t_hist, O, mode):
    """J1 + J2 + J3 of the oracle (O2 = oracle.vch2d_oracle) + J4 of the mode."""
    if mode == "full":
        return O2.cost(phi, u, phi_Q, phi_T, x, y, t_hist, O)
    return float(np.sum(O2.cost_parts(phi, u, phi_Q, phi_T, x, y, t_hist, O)[:3])) + j4(u, x, y, t_hist, O.kappa_sparsity, mode)


def kkt(u, r, x, y, t_hist, b3, ks, lo, hi, mode, tol=1e-6):
    """counts {#groups ||u_g|| < tol, #groups ||r_g|| <= ks, #agree, #groups} and the stationarity
    ||prox_1(u) - u|| / (||u|| + 1e-9) with the mode's prox at alpha = 1."""
    zero = group_norms(u, x, y, t_hist, mode).ravel() < tol
    small = group_norms(r, x, y, t_hist, mode).ravel() <= ks
    p1 = prox(u, r, 1.0, b3, ks, lo, hi, mode, x, y, t_hist)[0]
    stat = float(np.linalg.norm(p1 - u) / (np.linalg.norm(u) + 1e-9))
    return np.array([zero.sum(), small.sum(), (zero == small).sum(), zero.size], dtype=np.int64), stat


def pgd(O2, P, O, mode, n_iter, phi0=None, u0=None, alpha0=None, seed=42, amp=0.1):
    """The loop of vch_pgd.h's 2D rule (optimistic step with alpha_prev; else backtracking from 0.8 alpha_prev with beta
    0.8 and at most 10 trials, the last try taken if none improves; growth 1.2) over the oracle's forward / backward, with
    the prox and J4 of the mode.  `u0` (rows, nx1, ny1): the start control, taken as given (default zeros); `alpha0`: the
    first step, capped at alpha_max.  Short runs only: the plateau and stop rules are left out.
    -> dict(costs, alphas, attempts, change, u, phi, r, x, y, t_hist, phi_Q, phi_T)."""
    fwd = lambda u: O2.forward(P, control=u, phi0=phi0, seed=seed, amp=amp)
    phi_k, (x, y), t_hist = fwd(None if u0 is None else np.asarray(u0, dtype=np.float64))
    u_k = np.zeros_like(phi_k) if u0 is None else np.array(u0, dtype=np.float64)
    phi_T, phi_Q = O2.build_targets(x, y, t_hist, phi_k[0].copy(), P.Lx, P.Ly, P.T, 1, 1)
    J = lambda phi, u: cost(O2, phi, u, phi_Q, phi_T, x, y, t_hist, O, mode)
    if mode == "full":
        step = lambda u, r, a: O2.prox_step(u, O2.gradient(r, u, O), a, O)
    else:
        step = lambda u, r, a: prox(u, r, a, O.b3, O.kappa_sparsity, O.u_min, O.u_max, mode, x, y, t_hist)[0]
    cost_k = J(phi_k, u_k)
    costs, alphas, attempts, change = [cost_k], [], [], []
    alpha_prev = O.alpha_max if alpha0 is None else min(float(alpha0), O.alpha_max)
    r_k = None
    for _ in range(n_iter):
        r_k = O2.backward(phi_k, x, y, t_hist, P, O.b1, O.b2, phi_Q, phi_T)[2]
        alpha, att = alpha_prev, 0
        u_n = step(u_k, r_k, alpha)
        phi_n = fwd(u_n)[0]
        c_n = J(phi_n, u_n)
        if not c_n < cost_k:
            alpha = 0.8 * alpha_prev
            for _ in range(10):
                att += 1
                u_n = step(u_k, r_k, alpha)
                phi_n = fwd(u_n)[0]
                c_n = J(phi_n, u_n)
                if c_n < cost_k:
                    break
                alpha *= 0.8
        costs.append(c_n)
        alphas.append(alpha)
        attempts.append(att)
        change.append(float(np.linalg.norm(u_n - u_k) / (np.linalg.norm(u_k) + 1e-9)))
        alpha_prev = min(O.alpha_max, alpha * 1.2)
        u_k, cost_k, phi_k = u_n, c_n, phi_n
    return dict(costs=costs, alphas=alphas, attempts=attempts, change=change, u=u_k, phi=phi_k, r=r_k, x=x, y=y,
                t_hist=t_hist, phi_Q=phi_Q, phi_T=phi_T)
