"""NumPy restatement of vch1d_hess_cg_tr and of the rounds of vch1d_pgd_trust: Steihaug-Toint truncated
conjugate gradients in the preconditioner's norm ||x||_D^2 = sum D x^2, the iteration of _cg_ref.cg with the device's
recurrences for xx = ||x||_D^2 and xp = x . D p (x_0 = 0: both start at 0).  Pinned by test_trust_ref_cpu.py;
test_gpu_trust_1d.py compares the engine with it.

    step j: c = p . P A p, pp = p . D p, curv[j] = c / pp
            c not finite: BREAKDOWN
            not c > 0: tau = the positive root of xx + 2 tau xp + tau^2 pp = radius^2, exit NEGCURV after the step tau
                       (a tau that is not finite, radius = inf: NEGCURV at once, x as it is, as _cg_ref.cg)
            alpha = rho / c;  xx + 2 alpha xp + alpha^2 pp >= radius^2: the same tau, exit BOUNDARY after the step tau
            a step to the boundary: x += tau p, r -= tau P A p, pred += tau rho - tau^2 c / 2, resid[j], steps = j + 1
            otherwise the step of _cg_ref.cg, then xx += 2 alpha xp + alpha^2 pp, xp = beta (xp + alpha pp)"""
import math

import numpy as np

import _newton_ref as N
from _cg_ref import BREAKDOWN, CONVERGED, LIMIT, NEGCURV

BOUNDARY = 4
ACCEPTED, STATIONARY, NT_NEGCURV, NT_BREAKDOWN, STALLED, IDLE, REJECTED = range(7)        # VCH_NEWTON_*
ARMIJO = 1e-4


def tau_of(xx, xp, pp, d2):
    """tau >= 0 with xx + 2 tau xp + tau^2 pp = d2, in the form without cancellation for either sign of xp."""
    gap = max(d2 - xx, 0.0)
    disc = math.sqrt(xp * xp + pp * gap)
    with np.errstate(invalid="ignore"):
        return float(np.float64(gap) / np.float64(xp + disc)) if xp > 0.0 else (disc - xp) / pp


def steihaug(apply, mask, b, k, radius, cg_tol=0.0, D=None):
    """The arguments of _cg_ref.cg plus radius (> 0, inf allowed).  Returns its dict plus xnorm (||x||_D by the recurrence)."""
    mask = np.asarray(mask, dtype=bool).ravel()
    n_free = int(mask.sum())
    if n_free == 0:
        raise ValueError("the free set is empty")
    if not radius > 0.0:
        raise ValueError("radius must be > 0")
    D = np.ones(mask.size) if D is None else np.asarray(D, dtype=np.float64).ravel()
    tol = cg_tol if cg_tol > 0 else 1e-8
    d2 = radius * radius
    r = np.where(mask, np.asarray(b, dtype=np.float64).ravel(), 0.0)
    rnorm0 = float(np.linalg.norm(r))
    if not np.isfinite(rnorm0):
        raise ValueError("the right-hand side is not finite on the free set")
    x = np.zeros_like(r)
    p = r / D
    rho = float(np.dot(r, p))
    resid, curv = np.full(k, np.nan), np.full(k, np.nan)
    pred, steps, status = 0.0, 0, CONVERGED if rnorm0 == 0.0 else LIMIT
    xx = xp = 0.0
    for j in range(int(k) if rnorm0 > 0.0 else 0):
        Ap = np.where(mask, apply(p), 0.0)
        c, pp = float(np.dot(p, Ap)), float(np.dot(p, D * p))
        curv[j] = c / pp
        if not np.isfinite(c):
            status = BREAKDOWN
            break
        pend = LIMIT
        if not c > 0.0:
            pend = NEGCURV
        else:
            alpha = rho / c
            if xx + 2.0 * alpha * xp + alpha * alpha * pp >= d2:
                pend = BOUNDARY
        if pend:
            alpha = tau_of(xx, xp, pp, d2)
            if not np.isfinite(alpha):
                status = NEGCURV
                break
        x = x + alpha * p
        r = r - alpha * Ap
        z = r / D
        rho_new = float(np.dot(r, z))
        resid[j] = float(np.linalg.norm(r)) / rnorm0
        steps = j + 1
        xx_new = xx + 2.0 * alpha * xp + alpha * alpha * pp
        if pend:
            pred += alpha * rho - 0.5 * (alpha * alpha) * c
            xx, status = xx_new, pend
            break
        pred += 0.5 * alpha * rho
        if not np.isfinite(resid[j]) or not np.isfinite(rho_new):
            xx, status = xx_new, BREAKDOWN
            break
        if resid[j] <= tol:
            xx, status = xx_new, CONVERGED
            break
        beta = rho_new / rho
        p = z + beta * p
        rho = rho_new
        xx, xp = xx_new, beta * (xp + alpha * pp)
    return dict(x=x, r=r, p=p, resid=resid, curv=curv, pred=pred, rnorm0=rnorm0, steps=steps, status=status, n_free=n_free,
                xnorm=math.sqrt(xx))


def judge(cost, pred, c_new, xnorm, cg_status, radius, radius_max, radius_min):
    """The verdict of vch_trust_state::judge -> (status, ratio, new radius, ended)."""
    with np.errstate(all="ignore"):
        ratio = float((np.float64(cost) - np.float64(c_new)) / np.float64(pred))
    accept = math.isfinite(c_new) and c_new <= cost - ARMIJO * pred
    if not math.isfinite(ratio) or ratio < 0.25:
        radius = 0.25 * min(radius, xnorm)
    elif ratio > 0.75 and cg_status in (BOUNDARY, NEGCURV):
        radius = min(2.0 * radius, radius_max)
    small = radius < radius_min
    if accept:
        return ACCEPTED, ratio, radius, small
    return (STALLED if small else REJECTED), ratio, radius, small


def trust_rounds(A, c, kappa, w, u, lo, hi, n_rounds, radius0, radius_max=None, radius_min=None, k=50, cg_tol=1e-8, D=None,
                 tol=1e-8):
    """The rounds of vch1d_pgd_trust for one trajectory over the dense model of _newton_ref.py (its cost, free set and
    trial): the Steihaug step inside the radius, one trial at s = 1, the verdicts of `judge`.  -> (u, records): the rounds
    until the trajectory ends; the rounds after that are IDLE records."""
    radius_max = 1024.0 * radius0 if radius_max is None else radius_max
    radius_min = 1e-10 * radius0 if radius_min is None else radius_min
    u, radius, recs, ended = np.asarray(u, dtype=np.float64).copy(), float(radius0), [], False
    for _ in range(int(n_rounds)):
        if ended:
            recs.append(dict(status=IDLE))
            continue
        free = N.free_set(u, lo, hi, tol)
        J = N.cost(A, c, kappa, w, u)
        rec = dict(cost=J, cost_new=J, radius=radius, ratio=float("nan"), n_free=int(free.sum()), status=STATIONARY, pred=0.0,
                   xnorm=0.0, cg_status=None, cg_steps=0, rnorm0=0.0, pinned=0, clipped=0)
        recs.append(rec)
        ended = True
        if not free.any():
            continue
        b = -(A @ u - c + kappa * w * np.sign(u))
        S = steihaug(lambda v: A @ v, free, b, k, radius, cg_tol, D)
        rec.update(pred=S["pred"], xnorm=S["xnorm"], cg_status=S["status"], cg_steps=S["steps"], rnorm0=S["rnorm0"])
        if S["rnorm0"] == 0.0:
            continue
        if S["status"] == BREAKDOWN:
            rec["status"] = NT_BREAKDOWN
            continue
        t, rec["pinned"], rec["clipped"] = N.trial(u, S["x"], 1.0, lo, hi, free)
        Jt = N.cost(A, c, kappa, w, t)
        rec["status"], rec["ratio"], radius, ended = judge(J, S["pred"], Jt, S["xnorm"], S["status"], radius, radius_max, radius_min)
        if rec["status"] == ACCEPTED:
            u, rec["cost_new"] = t, Jt
    return u, recs
