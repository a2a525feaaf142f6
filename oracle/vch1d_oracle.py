"""CPU oracle for the 1D hot path — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

From-scratch numpy restatement of the reference's 1D algorithm; same role and
same import rule as oracle/vch2d_oracle.py (only tests/, smoke() and the
cpu_baseline leg of bench.py may import it).  Pinned against golden vectors made
by the reference itself (tests/golden/g1d_*.npz, tests/test_oracle_golden_1d.py).

The reference solves dense systems with numpy/LAPACK `dgesv` (Forward_solver.py:185,
backward_solver.py:94,116).  `solver="dense"` follows it literally; `solver="banded"`
solves the same matrices in LAPACK banded storage (`scipy.linalg.solve_banded`) so that
the N=4096 checks finish in seconds — same matrix, different elimination order.

Reference abbreviations: F1 = src/1D/Vch_control_1D/Forward_solver.py,
B1 = backward_solver.py, C1 = cost_and_function.py, G1 = GD_1D.py, K1 = config.py.
"""
from __future__ import annotations

from dataclasses import dataclass, field
import numpy as np
from scipy.linalg import solve_banded

DELTA_SEP = 1e-2       # F1:42
NEWTON_TOL = 1e-6      # F1:143
NEWTON_MAXIT = 50      # F1:144
ARMIJO_ETA = 1e-3      # F1:215


@dataclass
class Params1D:
    """K1:93-102."""
    N: int = 128
    Lx: float = 1.0
    T: float = 1.0
    dt_initial: float = 1e-2
    tau: float = 0.05
    gamma: float = 10.0
    c1: float = 0.75
    c2: float = 1.0
    kappa: float = 0.03 ** 2


@dataclass
class OptParams1D:
    """K1:115-123."""
    b1: float = 0.3
    b2: float = 13.0
    b3: float = 0.0019
    kappa_sparsity: float = 0.00009
    alpha_max: float = 100.0
    max_iter: int = 1000
    u_min: float = -1.0
    u_max: float = 1.0


# The reference's backward solver freezes c1, c2, tau, gamma from a DEFAULT config at
# import time and ignores the run-time one (B1:29-33).  Reproduced.
_FROZEN = Params1D()


def trapz_weights(n):
    w = np.ones(n)
    w[0] = w[-1] = 0.5
    return w


def lap(v, h):
    """Mirrored-Neumann second difference (F1:64-80), last axis."""
    a = 1.0 / (h * h)
    out = np.empty_like(v)
    out[..., 1:-1] = a * v[..., :-2] + (-2.0 * a) * v[..., 1:-1] + a * v[..., 2:]
    out[..., 0] = (-2.0 * a) * v[..., 0] + (2.0 * a) * v[..., 1]
    out[..., -1] = (2.0 * a) * v[..., -2] + (-2.0 * a) * v[..., -1]
    return out


def lap_dense(N, h):
    a = 1.0 / (h * h)
    L = np.zeros((N + 1, N + 1))
    i = np.arange(1, N)
    L[i, i - 1] = a; L[i, i] = -2 * a; L[i, i + 1] = a
    L[0, 0], L[0, 1] = -2 * a, 2 * a
    L[N, N - 1], L[N, N] = 2 * a, -2 * a
    return L


def reg_log(phi, eps=None):
    """F1:57-62."""
    if eps is None:
        eps = max(1e-8, 0.5 * DELTA_SEP)
    p = np.clip(phi, -1 + eps, 1 - eps)
    return np.log((1 + p) / (1 - p))


def fpp(phi, eps=1e-8):
    """B1:36-46 with the frozen default c1, c2."""
    p = np.clip(phi, -1 + eps, 1 - eps)
    return 2.0 * _FROZEN.c1 / (1.0 - p ** 2) - 2.0 * _FROZEN.c2


def mu_init(phi, w, P, h):
    """F1:82-86."""
    return -P.kappa * lap(phi, h) + (P.c1 * reg_log(phi) - 2.0 * P.c2 * phi) - w


def w_filter(w_old, dt, gamma, u_n, u_np1):
    g = gamma / dt
    return ((g - 0.5) * w_old + 0.5 * (u_np1 + u_n)) / (g + 0.5)


def residual_mu(pn, po, mn, mo, dt, h):
    """F1:93-97."""
    return (pn - po) / dt - 0.5 * (lap(mn, h) + lap(mo, h))


def residual_phi(pn, po, mn, mo, wn, wo, dt, P, h):
    """F1:99-109."""
    return ((P.tau * (pn - po) / dt) - 0.5 * P.kappa * (lap(pn, h) + lap(po, h))
            + (P.c1 * reg_log(pn) + (-2.0 * P.c2 * po)) - 0.5 * (mn + mo) - 0.5 * (wn + wo))


def jac_diag(pn, dt, P):
    """tau/dt + 2c1/(1-phi^2), NOT clipped in 1D (F1:122-124)."""
    return P.tau / dt + 2.0 * P.c1 / (1.0 - pn ** 2)


def jac_apply(pn, dphi, dmu, dt, P, h):
    top = -0.5 * P.kappa * lap(dphi, h) + jac_diag(pn, dt, P) * dphi - 0.5 * dmu
    bot = dphi / dt - 0.5 * lap(dmu, h)
    return top, bot


def jac_dense(pn, dt, P, L):
    """F1:111-137, unknown order [dphi; dmu]."""
    n = pn.size
    J = np.zeros((2 * n, 2 * n))
    Kpp = -0.5 * P.kappa * L.copy()
    np.fill_diagonal(Kpp, np.diag(Kpp) + jac_diag(pn, dt, P))
    J[:n, :n] = Kpp
    J[:n, n:] = -0.5 * np.eye(n)
    J[n:, :n] = (1.0 / dt) * np.eye(n)
    J[n:, n:] = -0.5 * L
    return J


def newton_rows(pn, dt, P, h):
    """Row-wise coefficients (offsets -3..3, the convention of _rows_to_banded) of jac_dense's matrix with the
    unknowns interleaved (dphi_0, dmu_0, dphi_1, dmu_1, ...): row 2i is the phi equation of node i, row 2i+1 its
    mu equation.  Offsets +-3 are structurally zero (the bandwidth is 2); they keep LAPACK's band (3, 3)."""
    n = pn.size
    lo, dg, up = _lap_rows(n, h)
    rows = tuple(np.zeros(2 * n) for _ in range(7))
    m2, m1, d0, p1, p2 = rows[1:6]
    m2[0::2], d0[0::2], p1[0::2], p2[0::2] = (-0.5 * P.kappa * lo, -0.5 * P.kappa * dg + jac_diag(pn, dt, P), -0.5,
                                              -0.5 * P.kappa * up)
    m2[1::2], m1[1::2], d0[1::2], p2[1::2] = -0.5 * lo, 1.0 / dt, -0.5 * dg, -0.5 * up
    return rows


def _solve_newton_banded(pn, dt, P, h, R):
    """Same matrix as jac_dense with unknowns interleaved (phi_i, mu_i), newton_rows."""
    n = pn.size
    rhs = np.empty(2 * n)
    rhs[0::2], rhs[1::2] = -R[:n], -R[n:]
    sol = solve_banded((3, 3), _rows_to_banded(newton_rows(pn, dt, P, h)), rhs)
    return np.concatenate([sol[0::2], sol[1::2]])


def free_energy(phi, kappa, c1, c2, h, w=None, eps=None):
    """Discrete free energy with forward-difference gradient (F1:243-262)."""
    phi = np.asarray(phi)
    wts = trapz_weights(len(phi))
    E = (kappa / (2.0 * h)) * np.sum(np.diff(phi) ** 2)
    eps = 1e-8 if eps is None else eps
    p = np.clip(phi, -1 + eps, 1 - eps)
    E += h * np.dot(wts, c1 * ((1 + p) * np.log(1 + p) + (1 - p) * np.log(1 - p)) - c2 * p ** 2)
    if w is not None:
        E -= h * np.dot(wts, np.asarray(w) * phi)
    return E


def init_phi_random(N, delta_sep=DELTA_SEP, amp=0.1, seed=42, enforce_zero_mean=True):
    """F1:264-277."""
    rng = np.random.default_rng(seed)
    phi0 = amp * rng.standard_normal(N + 1)
    if enforce_zero_mean:
        wts = trapz_weights(N + 1)
        phi0 -= np.dot(wts, phi0) / wts.sum()
    return np.clip(phi0, -1 + delta_sep, 1 - delta_sep)


def newton_step(phi_old, mu_old, w_old, w_new, dt, P, h, solver="dense", return_history=False,
                stats=None):
    """F1:139-235.  Initial guess (phi_old, mu_old) (F1:141-142); step
    alpha = min(1, 0.9*alpha_max) (F1:198-212); Armijo eta=1e-3 with the extra admissibility
    test all|phi_t| < 1-delta (F1:219); 12 failed halvings END the whole Newton loop with
    the current iterate (F1:227-229).

    `stats` (optional dict) accumulates the engine's counts under vch2d_oracle's names: "solves", "newton_its"
    (residual norms recorded, the initial one included), "armijo_trials" (trial points that pass the admissibility
    test, whose residual is evaluated), "failed_ls" (loops left through the line-search-failure return); and
    appends the loop's last residual norm to "last_norms".

    Decision margins: "min_margin" is the smallest relative distance to its threshold over every comparison the loops
    took -- |nR / NEWTON_TOL - 1| at each stop test, |max|phi_t| / (1 - DELTA_SEP) - 1| at each admissibility test,
    |nt / ((1 - eta alpha) nR) - 1| at each Armijo test, and |amax| (relative to 1) where a finite amax is tested
    against 0.  (min(1, 0.9 amax) is continuous in amax: no decision.)  Two correct implementations whose iterates
    differ by much less than min_margin take the same path.  "exits" gets one tuple per loop: (kind, iterations,
    halvings, capped) with kind "conv" | "maxit" | "failed_ls", iterations the residual norms recorded (this loop's
    share of "newton_its": one more than its solves after "conv", equal to them otherwise), halvings the step
    halvings of all its line searches, capped the iterations whose first step was cut by the ceiling 0.9 amax < 1."""
    pn, mn = phi_old.copy(), mu_old.copy()
    margin = np.inf
    halvings = capped = 0
    kind = "maxit"
    n = pn.size
    wts_h = h * trapz_weights(n)
    L = lap_dense(n - 1, h) if solver == "dense" else None
    hist = []
    nsolve = ntrial = 0
    failed = False
    for k in range(NEWTON_MAXIT):
        R = np.concatenate([residual_phi(pn, phi_old, mn, mu_old, w_new, w_old, dt, P, h),
                            residual_mu(pn, phi_old, mn, mu_old, dt, h)])
        nR = np.linalg.norm(R)
        hist.append(nR)
        if k % 10 == 0 and not np.isfinite(np.dot(wts_h, R[n:])):
            raise RuntimeError("Non-finite mass_defect; check phi bounds/log regularization.")
        margin = min(margin, abs(nR / NEWTON_TOL - 1.0))
        if nR < NEWTON_TOL:
            kind = "conv"
            break
        if solver == "dense":
            J = jac_dense(pn, dt, P, L)
            try:
                delta = np.linalg.solve(J, -R)
            except np.linalg.LinAlgError:
                delta = np.linalg.solve(J + 1e-10 * np.eye(2 * n), -R)
        else:
            delta = _solve_newton_banded(pn, dt, P, h, R)
        nsolve += 1
        dphi, dmu = delta[:n], delta[n:]
        with np.errstate(divide="ignore", invalid="ignore"):
            pos, neg = dphi > 0, dphi < 0
            a_pos = np.min((1 - DELTA_SEP - pn[pos]) / dphi[pos]) if np.any(pos) else np.inf
            a_neg = np.min((-1 + DELTA_SEP - pn[neg]) / dphi[neg]) if np.any(neg) else np.inf
            amax = min(a_pos, a_neg)
        if np.isfinite(amax):
            margin = min(margin, abs(amax))
        reset = not np.isfinite(amax) or amax <= 0
        if reset:
            amax = 1.0
        alpha = min(1.0, 0.9 * amax)
        capped += int(not reset and 0.9 * amax < 1.0)       # after a reset alpha = 0.9 comes from no ceiling
        ok = False
        for _ in range(12):
            pt, mt = pn + alpha * dphi, mn + alpha * dmu
            margin = min(margin, abs(np.max(np.abs(pt)) / (1 - DELTA_SEP) - 1.0))
            if np.all(np.abs(pt) < 1 - DELTA_SEP):
                ntrial += 1
                Rt = np.concatenate([residual_phi(pt, phi_old, mt, mu_old, w_new, w_old, dt, P, h),
                                     residual_mu(pt, phi_old, mt, mu_old, dt, h)])
                nt = np.linalg.norm(Rt)
                margin = min(margin, abs(nt / ((1 - ARMIJO_ETA * alpha) * nR) - 1.0))
                if nt <= (1 - ARMIJO_ETA * alpha) * nR:
                    pn, mn, ok = pt, mt, True
                    break
            alpha *= 0.5
            halvings += 1
        if not ok:
            failed = True
            kind = "failed_ls"
            break
    if stats is not None:
        stats["solves"] = stats.get("solves", 0) + nsolve
        stats["newton_its"] = stats.get("newton_its", 0) + len(hist)
        stats["armijo_trials"] = stats.get("armijo_trials", 0) + ntrial
        stats["failed_ls"] = stats.get("failed_ls", 0) + int(failed)
        stats.setdefault("last_norms", []).append(hist[-1])
        stats["min_margin"] = min(stats.get("min_margin", np.inf), float(margin))
        stats.setdefault("exits", []).append((kind, len(hist), halvings, capped))
    return (pn, mn, hist) if return_history else (pn, mn)


def forward(P: Params1D, control=None, initial_phi=None, seed=42, amp=0.01, solver="dense",
            max_steps=None, stats=None, dts=None):
    """F1:286-386.  History has M+2 rows: t=0 appears twice (F1:329-336).  Control rows
    (u[step], u[step+1]) while step < len(u)-1, else hold u[step] (F1:347-353; an array
    shorter than that raises IndexError as in the reference).  Post-step: clip, then a
    uniform shift by mass_error/Lx, always (F1:361-366).

    `dts` (optional sequence): the march takes exactly these steps, whatever P.T and P.dt_initial say, and t_hist
    accumulates them after the duplicated t = 0 row; None is the reference's rule dt = min(dt_initial, T - t) while
    t < T - 1e-10."""
    N, h = int(P.N), P.Lx / int(P.N)
    x = np.linspace(0, P.Lx, N + 1)
    if initial_phi is not None and initial_phi.shape == (N + 1,):
        phi = initial_phi.copy()
    else:
        phi = init_phi_random(N, DELTA_SEP, amp=amp, seed=seed)
    w = np.zeros(N + 1)
    wts_h = h * trapz_weights(N + 1)
    mass0 = np.dot(wts_h, phi)
    mu = mu_init(phi, w, P, h)
    t, step = 0.0, 0
    ts = [0.0, 0.0]
    hist = [phi.copy(), phi.copy()]
    zero = np.zeros(N + 1)
    given = None if dts is None else [float(d) for d in dts]
    while (t < P.T - 1e-10) if given is None else (step < len(given)):
        if max_steps is not None and step >= max_steps:
            break
        dt = min(P.dt_initial, P.T - t) if given is None else given[step]
        if control is not None:
            if step < control.shape[0] - 1:
                u_n, u_np1 = control[step, :], control[step + 1, :]
            else:
                u_n = u_np1 = control[step, :]
        else:
            u_n = u_np1 = zero
        w_new = w_filter(w, dt, P.gamma, u_n, u_np1)
        pn, mn = newton_step(phi, mu, w, w_new, dt, P, h, solver=solver, stats=stats)
        phi = np.clip(pn, -1 + DELTA_SEP, 1 - DELTA_SEP)
        mu, w = mn, w_new
        phi -= (np.dot(wts_h, phi) - mass0) / P.Lx
        t += dt
        step += 1
        hist.append(phi.copy())
        ts.append(min(t, P.T) if given is None else t)
    return np.array(hist), x, np.array(ts)


def _lap_rows(n, h):
    """Row-wise tridiagonal coefficients of the mirrored-Neumann operator:
    (Lv)[i] = lo[i] v[i-1] + dg[i] v[i] + up[i] v[i+1]."""
    a = 1.0 / (h * h)
    lo = np.full(n, a); lo[-1] = 2 * a; lo[0] = 0.0
    up = np.full(n, a); up[0] = 2 * a; up[-1] = 0.0
    dg = np.full(n, -2.0 * a)
    return lo, dg, up


def _penta_rows(n, h):
    """Row-wise coefficients (offsets -2..2) of L@L from the tridiagonal rows of L."""
    lo, dg, up = _lap_rows(n, h)
    sh = lambda v, k: np.concatenate([v[k:], np.zeros(k)]) if k > 0 else np.concatenate([np.zeros(-k), v[:k]])
    m2 = lo * sh(lo, -1)
    m1 = lo * sh(dg, -1) + dg * lo
    d0 = lo * sh(up, -1) + dg * dg + up * sh(lo, 1)
    p1 = dg * up + up * sh(dg, 1)
    p2 = up * sh(up, 1)
    return m2, m1, d0, p1, p2


def _rows_to_banded(rows):
    """Row-wise offset coefficients -> LAPACK banded storage ab[u + i - j, j] = A[i, j]."""
    k = (len(rows) - 1) // 2
    n = rows[0].size
    ab = np.zeros((2 * k + 1, n))
    for off, v in zip(range(-k, k + 1), rows):
        i = np.arange(max(0, -off), min(n, n - off))
        ab[k - off, i + off] = v[i]
    return ab


def _rows_matvec(rows, x):
    k = (len(rows) - 1) // 2
    n = x.size
    y = np.zeros(n)
    for off, v in zip(range(-k, k + 1), rows):
        i = np.arange(max(0, -off), min(n, n - off))
        y[i] += v[i] * x[i + off]
    return y


def _adjoint_comb(n, h, cL2, D):
    """Row-wise coefficients (offsets -2..2) of I - tau L + cL2 L@L + diag(D) L with the frozen tau (B1:29-33);
    D = None: no diagonal term."""
    lo, dg, up = _lap_rows(n, h)
    z, one = np.zeros(n), np.ones(n)
    cL = -_FROZEN.tau + (0.0 if D is None else D)
    return tuple(e + cL * l + cL2 * l2 for e, l, l2 in zip((z, z, one, z, z), (z, lo, dg, up, z), _penta_rows(n, h)))


def adjoint_rows(phi_n, dt, h, n=None):
    """Rows of the adjoint step matrix A(phi_n) = I - tau L + dt/2 L@L - dt/2 diag(fpp(phi_n)) L (B1:99-101, 116);
    dt = 0 gives the terminal matrix I - tau L (B1:94), for which phi_n may be None if n is given."""
    n = phi_n.size if n is None else n
    return _adjoint_comb(n, h, 0.5 * dt, None if dt == 0 else -0.5 * dt * fpp(phi_n))


def adjoint_rhs_rows(phi_np1, dt, h):
    """Rows of B(phi_np1) = I - tau L - dt/2 L@L + dt/2 diag(fpp(phi_np1)) L, the step's right-hand side operator
    (B1:103-113)."""
    return _adjoint_comb(phi_np1.size, h, -0.5 * dt, 0.5 * dt * fpp(phi_np1))


# ---------------------------------------------------------------------------------------
# checkers for the engine's banded solves (test infrastructure)
# ---------------------------------------------------------------------------------------
def _residual_ld(rows, x, b):
    """(b - A x, |A||x| + |b|) accumulated in np.longdouble."""
    k = (len(rows) - 1) // 2
    x, b = np.asarray(x, np.longdouble), np.asarray(b, np.longdouble)
    n = x.size
    r, s = b.copy(), np.abs(b)
    for off, v in zip(range(-k, k + 1), rows):
        i = np.arange(max(0, -off), min(n, n - off))
        t = np.asarray(v[i], np.longdouble) * x[i + off]
        r[i] -= t
        s[i] += np.abs(t)
    return r, s


def backward_error(rows, x, b, f=None):
    """Componentwise (Oettli-Prager) backward error of x as a solution of A x = b, A given by its rows
    (_rows_to_banded convention):  omega = max_i |b - A x|_i / (|A||x| + f)_i, the smallest omega such that
    (A + E) x = b + e with |E| <= omega |A|, |e| <= omega f.  f defaults to |b|; a right-hand side formed as
    b = B y + s passes f = |B||y| + |s|, the size of the data it is made of.  A backward-stable solve gives a few eps.

    The residual and the denominator are accumulated in np.longdouble, which is 80-bit extended on x86-64
    (eps 1.1e-19): omega is then exact to ~1e-3 eps.  Where longdouble is only double, omega is still accurate to a
    few eps.  b may be a longdouble array (a right-hand side formed in extended precision)."""
    r, s = _residual_ld(rows, x, b)
    if f is not None:
        s = s - np.abs(np.asarray(b, np.longdouble)) + np.asarray(f, np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(s > 0, np.abs(r) / s, np.where(r == 0, 0.0, np.inf))
    return float(np.max(w))


def hp_solve(rows, b, steps=2):
    """High-precision reference solution of A x = b: LAPACK banded LU (solve_banded) followed by `steps` steps of
    iterative refinement with the residual computed in np.longdouble."""
    k = (len(rows) - 1) // 2
    ab = _rows_to_banded(rows)
    x = solve_banded((k, k), ab, np.asarray(b, np.float64))
    for _ in range(steps):
        x = x + solve_banded((k, k), ab, _residual_ld(rows, x, b)[0].astype(np.float64))
    return x


def _rows_to_csc(rows):
    from scipy import sparse
    k = (len(rows) - 1) // 2
    n = rows[0].size
    offs = list(range(-k, k + 1))
    return sparse.diags([v[max(0, -o):min(n, n - o)] for o, v in zip(offs, rows)], offs, shape=(n, n), format="csc")


def cond_estimate(rows, x, b):
    """Condition number of A x = b for componentwise perturbations (Skeel):
    cond = || |A^-1| (|A||x| + |b|) ||_inf / ||x||_inf, so that a solution with backward error omega has the
    normwise relative forward error  ||x_hat - x||_inf / ||x||_inf <= omega * cond  (to first order).  Invariant
    under row scaling, unlike ||A|| ||A^-1||.  || |A^-1| g ||_inf = || A^-1 diag(g) ||_inf is estimated with the
    Hager-Higham 1-norm estimator (scipy onenormest, t = 1: deterministic) applied to its transpose, with A^-1 from
    a sparse LU."""
    from scipy.sparse.linalg import LinearOperator, onenormest, splu
    lu = splu(_rows_to_csc(rows))
    g = _residual_ld(rows, x, b)[1].astype(np.float64)
    n = g.size
    op = LinearOperator((n, n), dtype=np.float64, matvec=lambda v: g * lu.solve(np.ravel(v), trans="T"),
                        rmatvec=lambda v: lu.solve(g * np.ravel(v)))
    return float(onenormest(op, t=1)) / float(np.max(np.abs(x)))


def backward(phi_hist, x, t_hist, b1, b2, phi_Q=None, phi_T=None, solver="dense", max_steps=None):
    """B1:48-126.  Physical parameters are the frozen defaults (B1:29-33); dt_n <= 0
    rows are skipped and stay zero (B1:110), so row 0 of p, q, r is zero because of the
    duplicated t=0 entry."""
    M1, n = phi_hist.shape
    tau, gamma = _FROZEN.tau, _FROZEN.gamma
    if phi_Q is None:
        phi_Q = np.zeros_like(phi_hist)
    if phi_T is None:
        phi_T = np.zeros(n)
    h = x[1] - x[0]
    p = np.zeros_like(phi_hist); q = np.zeros_like(phi_hist); r = np.zeros_like(phi_hist)
    last = 0 if max_steps is None else max(0, M1 - 1 - max_steps)
    if solver == "dense":
        L = lap_dense(n - 1, h)
        I = np.eye(n)
        L2 = L @ L
        p[-1] = np.linalg.solve(I - tau * L, b2 * (phi_hist[-1] - phi_T))
        q[-1] = -(L @ p[-1])
    else:
        p[-1] = solve_banded((2, 2), _rows_to_banded(adjoint_rows(None, 0.0, h, n=n)), b2 * (phi_hist[-1] - phi_T))
        q[-1] = -lap(p[-1], h)
    for k in range(M1 - 2, last - 1, -1):
        dt = t_hist[k + 1] - t_hist[k]
        if dt <= 0:
            continue
        src = 0.5 * dt * b1 * ((phi_hist[k] - phi_Q[k]) + (phi_hist[k + 1] - phi_Q[k + 1]))
        if solver == "dense":
            A = I - tau * L + 0.5 * dt * L2 - 0.5 * dt * (fpp(phi_hist[k])[:, None] * L)
            Bm = I - tau * L - 0.5 * dt * L2 + 0.5 * dt * (fpp(phi_hist[k + 1])[:, None] * L)
            rhs = Bm @ p[k + 1] + src
            try:
                p[k] = np.linalg.solve(A, rhs)
            except np.linalg.LinAlgError:
                p[k] = np.linalg.solve(A + 1e-10 * I, rhs)
            q[k] = -(L @ p[k])
        else:
            rhs = _rows_matvec(adjoint_rhs_rows(phi_hist[k + 1], dt, h), p[k + 1]) + src
            p[k] = solve_banded((2, 2), _rows_to_banded(adjoint_rows(phi_hist[k], dt, h)), rhs)
            q[k] = -lap(p[k], h)
        r[k] = ((gamma - 0.5 * dt) / (gamma + 0.5 * dt)) * r[k + 1] \
            + ((dt * 0.5) / (gamma + 0.5 * dt)) * (q[k] + q[k + 1])
    return p, q, r


def adjoint_A_apply(phi_n, v, dt, h):
    Lv = lap(v, h)
    return v - _FROZEN.tau * Lv + 0.5 * dt * lap(Lv, h) - 0.5 * dt * fpp(phi_n) * Lv


def adjoint_B_apply(phi_np1, v, dt, h):
    Lv = lap(v, h)
    return v - _FROZEN.tau * Lv - 0.5 * dt * lap(Lv, h) + 0.5 * dt * fpp(phi_np1) * Lv


def _trapz(f, x, axis=-1):
    f = np.moveaxis(np.asarray(f), axis, -1)
    d = np.diff(np.asarray(x))
    return np.sum(d * (f[..., 1:] + f[..., :-1]) / 2.0, axis=-1)


def cost_parts(phi_hist, u, phi_Q, phi_T, x, t_hist, b1, b2, b3, kappa):
    """C1:55-73."""
    J1 = (b1 / 2.0) * _trapz(_trapz((phi_hist - phi_Q) ** 2, x, 1), t_hist)
    J2 = (b2 / 2.0) * _trapz((phi_hist[-1] - phi_T) ** 2, x)
    J3 = (b3 / 2.0) * _trapz(_trapz(u ** 2, x, 1), t_hist)
    J4 = kappa * _trapz(_trapz(np.abs(u), x, 1), t_hist)
    return np.array([J1, J2, J3, J4])


def cost(phi_hist, u, phi_Q, phi_T, x, t_hist, b1, b2, b3, kappa):
    return float(np.sum(cost_parts(phi_hist, u, phi_Q, phi_T, x, t_hist, b1, b2, b3, kappa)))


def gradient(r, u, b3):
    """C1:99."""
    return r + b3 * u


def gradient_step(u, g, alpha):
    """C1:111."""
    return u - alpha * g


def prox_project(u_temp, alpha, kappa, u_min, u_max):
    """G1:56-71."""
    s = np.sign(u_temp) * np.maximum(np.abs(u_temp) - alpha * kappa, 0)
    return np.clip(s, u_min, u_max)


def build_targets(x, t_hist, phi_initial, Lx, T, choice_t=1, choice_q=1, A_T=0.7, k_tan=0.45):
    """G1:210-252 (ramp uses t_hist/t_hist[-1], not the config T)."""
    if choice_t == 1:
        phi_T = A_T * np.sin(2.0 * np.pi * x / Lx)
    elif choice_t == 2:
        phi_T = A_T * np.cos(2.0 * np.pi * x / Lx)
    else:
        tr = np.tan(2.0 * np.pi * k_tan * (x / Lx - 0.5))
        sc = np.max(np.abs(tr))
        phi_T = A_T * (tr / (sc if sc > 1e-12 else 1.0))
    if choice_q == 1:
        tp = (t_hist / (t_hist[-1] if t_hist[-1] > 0 else 1.0))[:, None]
        phi_Q = (1.0 - tp) * phi_initial + tp * phi_T
    else:
        phi_Q = np.zeros((len(t_hist), len(x)))
    return phi_T, phi_Q


def error_metrics(phi_hist, phi_Q, phi_T, x, t_hist):
    """Relative tracking / terminal errors of the driver loop, G1:425-450: space-time L2 of phi - phi_Q (trapezoid in x
    per level, then in t) over that of phi_Q -- replaced by the RMS scale sqrt(|Omega| T) when the target is ~0 -- and
    the L2 of phi(T) - phi_T over that of phi_T, each denominator + 1e-12."""
    l2xt = lambda a: float(np.sqrt(_trapz(_trapz(a ** 2, x, 1), t_hist)))
    l2x = lambda a: float(np.sqrt(_trapz(a ** 2, x)))
    rms = float(np.sqrt(max(float(x[-1] - x[0]), 1e-30) * max(float(t_hist[-1] - t_hist[0]), 1e-30)))
    den = l2xt(phi_Q)
    if den < 1e-9 * rms:
        den = rms
    return l2xt(phi_hist - phi_Q) / (den + 1e-12), l2x(phi_hist[-1] - phi_T) / (l2x(phi_T) + 1e-12)


@dataclass
class PGDResult:
    costs: list = field(default_factory=list)
    alphas: list = field(default_factory=list)
    alphas_used: list = field(default_factory=list)   # the step the accepted control was made with, see pgd
    trials: list = field(default_factory=list)
    changes: list = field(default_factory=list)       # relative control change of every iteration (the stop rule's input)
    tracking: list = field(default_factory=list)
    terminal: list = field(default_factory=list)
    u: np.ndarray = None
    phi: np.ndarray = None
    r: np.ndarray = None
    converged: bool = False


def pgd(P: Params1D, O: OptParams1D, n_iter=None, choice_t=1, choice_q=1, solver="dense", initial_phi=None,
        stats=None):
    """G1:333-477: optimistic step with alpha_prev; on failure backtracking from
    alpha_prev (beta 0.8, <=5 trials, G1:73-113); alpha growth 1.2, plateau (10 its,
    |dJ|<1e-7) -> 2.0; stop when the relative control change < 1e-5 and k > 10.
    `initial_phi` replaces the seeded initial state of every march (as in forward); `stats` accumulates the
    counts of every march (forward's stats) and "min_cost_gap", the smallest relative gap |c_trial - cost_k| / cost_k
    over the acceptance tests c_trial < cost_k.  A search that runs out returns its fifth try, made with
    alpha_prev 0.8^4, but reports a_k after one more `alpha *= 0.8` (G1:107-113); `alphas` keeps the reported values,
    `alphas_used` the step each accepted control was really made with."""
    fwd = lambda u: forward(P, control=u, initial_phi=initial_phi, solver=solver, stats=stats)
    phi_k, x, t_hist = fwd(None)
    u_k = np.zeros_like(phi_k)
    phi_T, phi_Q = build_targets(x, t_hist, phi_k[0].copy(), P.Lx, P.T, choice_t, choice_q)
    cargs = (O.b1, O.b2, O.b3, O.kappa_sparsity)
    cost_k = cost(phi_k, u_k, phi_Q, phi_T, x, t_hist, *cargs)
    res = PGDResult(costs=[cost_k])
    alpha_prev, plateau = O.alpha_max, 0
    r_k = None

    def gap(c):
        if stats is not None:
            stats["min_cost_gap"] = min(stats.get("min_cost_gap", np.inf), abs(c - cost_k) / cost_k)

    for k in range(O.max_iter if n_iter is None else n_iter):
        _, _, r_k = backward(phi_k, x, t_hist, O.b1, O.b2, phi_Q, phi_T, solver=solver)
        g = gradient(r_k, u_k, O.b3)
        u_o = prox_project(gradient_step(u_k, g, alpha_prev), alpha_prev, O.kappa_sparsity,
                           O.u_min, O.u_max)
        phi_o, _, _ = fwd(u_o)
        c_o = cost(phi_o, u_o, phi_Q, phi_T, x, t_hist, *cargs)
        gap(c_o)
        if c_o < cost_k:
            a_k, u_n, c_n, phi_n, nt = alpha_prev, u_o, c_o, phi_o, 1
            a_used = alpha_prev
        else:
            alpha, nt = alpha_prev, 0
            for _ in range(5):
                nt += 1
                a_used = alpha
                u_n = prox_project(gradient_step(u_k, g, alpha), alpha, O.kappa_sparsity,
                                   O.u_min, O.u_max)
                phi_n, _, _ = fwd(u_n)
                c_n = cost(phi_n, u_n, phi_Q, phi_T, x, t_hist, *cargs)
                gap(c_n)
                if c_n < cost_k:
                    break
                alpha *= 0.8
            a_k = alpha
        res.costs.append(c_n); res.alphas.append(a_k); res.trials.append(nt); res.alphas_used.append(a_used)
        e1, e2 = error_metrics(phi_n, phi_Q, phi_T, x, t_hist)
        res.tracking.append(e1); res.terminal.append(e2)
        if k > 0 and abs(res.costs[-1] - res.costs[-2]) < 1e-7:
            plateau += 1
        else:
            plateau = 0
        if plateau >= 10:
            alpha_prev, plateau = min(O.alpha_max, a_k * 2.0), 0
        else:
            alpha_prev = min(O.alpha_max, a_k * 1.2)
        change = np.linalg.norm(u_n - u_k) / (np.linalg.norm(u_k) + 1e-9)
        res.changes.append(change)
        if change < 1e-5 and k > 10:
            u_k = u_n.copy()
            res.converged = True
            break
        u_k, cost_k, phi_k = u_n.copy(), c_n, phi_n
    res.u, res.phi, res.r = u_k, phi_k, r_k
    res.phi_T, res.phi_Q, res.t_hist, res.x = phi_T, phi_Q, t_hist, x
    return res
