"""NumPy restatement of the iteration of vch2d_hess_cg: (preconditioned) conjugate gradients on
P A P x = P b from x_0 = 0 with the device's stop rules and its order of updates.  Pinned by test_cg_ref_cpu.py;
test_gpu_hess_cg_2d.py compares the engine's steps with it.

    r = P b, z = D^-1 r, p = z, rho = r . z
    step j: c = p . P A p, n = p . D p, curv[j] = c / n
            c not finite: BREAKDOWN;  not c > 0: NEGCURV (x and p stay as they are)
            alpha = rho / c, x += alpha p, r -= alpha P A p, pred += alpha rho / 2, resid[j] = ||r|| / ||P b||
            resid[j] not finite: BREAKDOWN;  resid[j] <= cg_tol: CONVERGED
            beta = rho_new / rho, p = z + beta p
    LIMIT after k steps (no cap at n_free); P b == 0: zero steps, CONVERGED"""
import numpy as np

LIMIT, CONVERGED, NEGCURV, BREAKDOWN = 0, 1, 2, 3


def cg(apply, mask, b, k, cg_tol=0.0, D=None):
    """apply: v -> A v on flat vectors; mask: flat booleans; b: flat right-hand side; D: flat positive diagonal or None (I).
    Returns dict(x, r, p; resid, curv: [k] with NaN beyond steps (curv[steps] is the stopping curvature of NEGCURV);
    pred; rnorm0; steps; status; n_free)."""
    mask = np.asarray(mask, dtype=bool).ravel()
    n_free = int(mask.sum())
    if n_free == 0:
        raise ValueError("the free set is empty")
    D = np.ones(mask.size) if D is None else np.asarray(D, dtype=np.float64).ravel()
    tol = cg_tol if cg_tol > 0 else 1e-8
    r = np.where(mask, np.asarray(b, dtype=np.float64).ravel(), 0.0)
    rnorm0 = float(np.linalg.norm(r))
    if not np.isfinite(rnorm0):
        raise ValueError("the right-hand side is not finite on the free set")
    x = np.zeros_like(r)
    p = r / D
    rho = float(np.dot(r, p))
    resid, curv = np.full(k, np.nan), np.full(k, np.nan)
    pred, steps, status = 0.0, 0, CONVERGED if rnorm0 == 0.0 else LIMIT
    for j in range(int(k) if rnorm0 > 0.0 else 0):
        Ap = np.where(mask, apply(p), 0.0)
        c, n = float(np.dot(p, Ap)), float(np.dot(p, D * p))
        curv[j] = c / n
        if not np.isfinite(c):
            status = BREAKDOWN
            break
        if not c > 0.0:
            status = NEGCURV
            break
        alpha = rho / c
        x = x + alpha * p
        r = r - alpha * Ap
        pred += 0.5 * alpha * rho
        z = r / D
        rho_new = float(np.dot(r, z))
        resid[j] = float(np.linalg.norm(r)) / rnorm0
        steps = j + 1
        if not np.isfinite(resid[j]) or not np.isfinite(rho_new):
            status = BREAKDOWN
            break
        if resid[j] <= tol:
            status = CONVERGED
            break
        p = z + (rho_new / rho) * p
        rho = rho_new
    return dict(x=x, r=r, p=p, resid=resid, curv=curv, pred=pred, rnorm0=rnorm0, steps=steps, status=status, n_free=n_free)
