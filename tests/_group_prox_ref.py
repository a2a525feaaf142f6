"""NumPy restatement of the directional sparsity functionals of the 1D engine.

g(u) = kappa_s * sum over groups of ||u_g||, a group being a row of the (rows, n) control ("time", ||z||^2 = sum_i wx_i
z_i^2) or a column ("space", ||z||^2 = sum_k wt_k z_k^2), wx / wt the trapezoid weights of x / t_hist.  The prox is taken in
the L2(Q) metric, so the threshold lam = alpha kappa_s is the same for every group.  Everything here is plain NumPy: the
root of a group is found by bisection to adjacent doubles, nothing is shared with the engine.
"""
import numpy as np

MODES = ("full", "time", "space")


def trapz_w(t):
    """np.trapezoid's weights of the abscissae t."""
    t = np.asarray(t, dtype=np.float64)
    w = np.zeros(t.size)
    d = np.diff(t)
    w[:-1] += 0.5 * d
    w[1:] += 0.5 * d
    return w


def cone(v, lo, hi):
    c = v.copy()
    if hi == 0.0:
        c[c > 0.0] = 0.0
    if lo == 0.0:
        c[c < 0.0] = 0.0
    return c


def wnorm(z, w):
    return float(np.sqrt(np.sum(w * z * z)))


def group_prox(v, w, lam, lo, hi):
    """prox of lam ||.||_w + the indicator of [lo, hi]^n (lo <= 0 <= hi) at v in the metric of w -> (u+, s, kind):
    kind "zero" (c <= lam), "closed" (s = 1 - lam / ||v||, box inactive) or "box" (root of h by bisection)."""
    v = np.asarray(v, dtype=np.float64)
    if wnorm(cone(v, lo, hi), w) <= lam:
        return np.zeros_like(v), 0.0, "zero"
    s0 = 1.0 - lam / wnorm(v, w)
    if np.array_equal(np.clip(s0 * v, lo, hi), s0 * v):
        return s0 * v, s0, "closed"
    h = lambda s: wnorm(np.clip(s * v, lo, hi), w) * (1.0 - s) - lam * s
    a, b = 0.0, 1.0                       # h(a) > 0 >= h(b): h(s) / s decreases from c - lam > 0 to -lam
    while True:
        m = a + 0.5 * (b - a)
        if not (a < m < b):
            break
        if h(m) > 0.0:
            a = m
        else:
            b = m
    return np.clip(b * v, lo, hi), b, "box"


def group_prox_many(V, w, lam, lo, hi, dtype=np.float64):
    """group_prox of every row of V (G, m), the same formulas with the bisection of all box-active rows run side by side
    -> (U (G, m), s (G,), kinds: list of G names).  `dtype` np.longdouble: the same V, w and lam (doubles) with every
    product, sum, square root and the bisection (to adjacent long doubles) in extended precision; U and s come back in it.
    That variant is the yardstick of this restatement's own rounding: its sums carry 11 more bits than any order of a
    double sum loses on a row of a few thousand nodes."""
    V, w, lam = np.asarray(V, dtype=np.float64).astype(dtype), np.asarray(w, dtype=np.float64).astype(dtype), dtype(lam)
    one = dtype(1.0)
    nrm = lambda Z: np.sqrt(np.sum(w * Z * Z, axis=1))
    live = nrm(cone(V, lo, hi)) > lam
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(live, one - lam / nrm(V), dtype(0.0))
    S0 = s[:, None] * V
    box = live & np.any(np.clip(S0, lo, hi) != S0, axis=1)
    Vb, a, b = V[box], np.zeros(int(box.sum()), dtype=dtype), np.ones(int(box.sum()), dtype=dtype)
    while Vb.size:
        m = a + dtype(0.5) * (b - a)
        go = (a < m) & (m < b)
        if not go.any():
            break
        pos = nrm(np.clip(m[:, None] * Vb, lo, hi)) * (one - m) - lam * m > 0.0
        a, b = np.where(go & pos, m, a), np.where(go & ~pos, m, b)
    s[box] = b
    U = np.where(live[:, None], np.clip(s[:, None] * V, lo, hi), dtype(0.0))
    return U, s, ["box" if x else ("closed" if y else "zero") for x, y in zip(box, live)]


def prox(u, r, alpha, b3, ks, lo, hi, mode, x=None, t_hist=None, dtype=np.float64):
    """(u+, s, kinds) of one (rows, n) control: the gradient step v = u - alpha (r + b3 u) in doubles, then the prox of the
    mode (in `dtype`, see group_prox_many)."""
    u = np.asarray(u, dtype=np.float64)
    v = u - alpha * (r + b3 * u)
    if mode == "time":
        return group_prox_many(v, trapz_w(x), alpha * ks, lo, hi, dtype)
    out, s, kinds = group_prox_many(np.ascontiguousarray(v.T), trapz_w(t_hist), alpha * ks, lo, hi, dtype)
    return np.ascontiguousarray(out.T), s, kinds


def j4(u, x, t_hist, ks, mode):
    wx, wt = trapz_w(x), trapz_w(t_hist)
    if mode == "time":
        return ks * float(np.sum(wt * np.sqrt(np.sum(wx * u * u, axis=1))))
    return ks * float(np.sum(wx * np.sqrt(np.sum(wt[:, None] * u * u, axis=0))))


def cost(O1, phi, u, phi_Q, phi_T, x, t_hist, b1, b2, b3, ks, mode):
    """J1 + J2 + J3 of the oracle (O1 = oracle.vch1d_oracle) + J4 of the mode."""
    if mode == "full":
        return O1.cost(phi, u, phi_Q, phi_T, x, t_hist, b1, b2, b3, ks)
    return float(np.sum(O1.cost_parts(phi, u, phi_Q, phi_T, x, t_hist, b1, b2, b3, ks)[:3])) + j4(u, x, t_hist, ks, mode)


def group_norms(a, x, t_hist, mode):
    if mode == "time":
        return np.sqrt(np.sum(trapz_w(x) * a * a, axis=1))
    return np.sqrt(np.sum(trapz_w(t_hist)[:, None] * a * a, axis=0))


def kkt(u, r, x, t_hist, b3, ks, lo, hi, mode, tol=1e-6):
    """counts {#groups ||u_g|| < tol, #groups ||r_g|| <= ks, #agree, #groups} and the stationarity
    ||prox_1(u) - u|| / (||u|| + 1e-9) with the mode's prox at alpha = 1."""
    zero, small = group_norms(u, x, t_hist, mode) < tol, group_norms(r, x, t_hist, mode) <= ks
    p1 = prox(u, r, 1.0, b3, ks, lo, hi, mode, x, t_hist)[0]
    stat = float(np.linalg.norm(p1 - u) / (np.linalg.norm(u) + 1e-9))
    return np.array([zero.sum(), small.sum(), (zero == small).sum(), zero.size], dtype=np.int64), stat


def pgd(O1, P, O, mode, n_iter, initial_phi=None, u0=None, alpha0=None):
    """The loop of vch_pgd.h's 1D rule (optimistic step with alpha_prev, else backtracking with beta 0.8 and at most 5
    trials, growth 1.2) over the oracle's forward / backward, with the prox and J4 of the mode.  `u0` (rows, n): the start
    control, taken as given (not clipped; default zeros); `alpha0`: the first step, capped at alpha_max (default alpha_max).
    Short runs only: the plateau and stop rules need k > 10 and are left out.  -> dict(costs, trials, change, u, phi, x,
    t_hist, phi_Q, phi_T), change[k] = ||u_{k+1} - u_k||_F / (||u_k||_F + 1e-9), the stop rule's quantity."""
    fwd = lambda u: O1.forward(P, control=u, initial_phi=initial_phi)
    phi_k, x, t_hist = fwd(None if u0 is None else np.asarray(u0, dtype=np.float64))
    u_k = np.zeros_like(phi_k) if u0 is None else np.array(u0, dtype=np.float64)
    phi_T, phi_Q = O1.build_targets(x, t_hist, phi_k[0].copy(), P.Lx, P.T, 1, 1)
    J = lambda phi, u: cost(O1, phi, u, phi_Q, phi_T, x, t_hist, O.b1, O.b2, O.b3, O.kappa_sparsity, mode)
    step = lambda u, r, a: prox(u, r, a, O.b3, O.kappa_sparsity, O.u_min, O.u_max, mode, x, t_hist)[0]
    cost_k = J(phi_k, u_k)
    costs, trials, change = [cost_k], [], []
    alpha_prev = O.alpha_max if alpha0 is None else min(float(alpha0), O.alpha_max)
    for _ in range(n_iter):
        r_k = O1.backward(phi_k, x, t_hist, O.b1, O.b2, phi_Q, phi_T)[2]
        alpha, nt = alpha_prev, 0
        for _ in range(5):
            nt += 1
            u_n = step(u_k, r_k, alpha)
            phi_n = fwd(u_n)[0]
            c_n = J(phi_n, u_n)
            if c_n < cost_k:
                break
            alpha *= 0.8
        costs.append(c_n)
        trials.append(nt)
        change.append(float(np.linalg.norm(u_n - u_k) / (np.linalg.norm(u_k) + 1e-9)))
        alpha_prev = min(O.alpha_max, alpha * 1.2)
        u_k, cost_k, phi_k = u_n, c_n, phi_n
    return dict(costs=costs, trials=trials, change=change, u=u_k, phi=phi_k, x=x, t_hist=t_hist, phi_Q=phi_Q, phi_T=phi_T)


def brute_force_improvement(v, w, lam, lo, hi, u, rng, tries=400):
    """The largest decrease of F(z) = 1/2 ||z - v||_w^2 + lam ||z||_w over random feasible perturbations of u at
    scales 1e-1 .. 1e-7 (0 when none improves).  Nodes of zero weight do not enter F and are left alone."""
    F = lambda z: 0.5 * np.sum(w * (z - v) ** 2) + lam * wnorm(z, w)
    f0, best = F(u), 0.0
    for _ in range(tries):
        z = np.clip(u + 10.0 ** rng.uniform(-7, -1) * rng.standard_normal(u.size) * (rng.random(u.size) < 0.5), lo, hi)
        best = max(best, f0 - F(z))
    return best, f0
