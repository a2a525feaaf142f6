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
            otherwise the step of _cg_ref.cg, then xx += 2 alpha xp + alpha^2 pp, xp = beta (xp + alpha pp)

radius^2 is formed in a double, as on the device: a radius whose square is not finite (>= 2^512) has no boundary and acts as
inf; a radius whose square underflows gives tau = 0, one counted step that moves nothing."""
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


def replay(R, i, radius_max, radius_min):
    """Member i of the record against `judge`, exactly: the status of every judged round and the radius (or
    IDLE) of the round after it."""
    n = R["status"].shape[1]
    for r in range(n):
        st = int(R["status"][i, r])
        if st in (IDLE, STATIONARY, NT_BREAKDOWN):
            assert all(R["status"][i, r + 1:] == IDLE)
            return
        cost, pred, ratio, xnorm, cgs, radius = (R[key][i, r] for key in ("cost", "pred", "ratio", "xnorm", "cg_status", "radius"))
        c_new = R["cost_new"][i, r] if st == ACCEPTED else cost - ratio * pred
        assert judge(cost, pred, c_new, xnorm, cgs, radius, radius_max, radius_min)[0] == st, (i, r)
        _, same, new_radius, ended = judge(ratio, 1.0, 0.0, xnorm, cgs, radius, radius_max, radius_min)       # (ratio - 0) / 1: the ratio itself
        assert same == ratio or (np.isnan(same) and np.isnan(ratio))
        assert (st == STALLED) == (ended and st != ACCEPTED), (i, r)
        if st != ACCEPTED:
            assert R["cost_new"][i, r] == cost, (i, r)
        if r + 1 < n:
            if ended:
                assert R["status"][i, r + 1] == IDLE, (i, r)
            else:
                assert R["radius"][i, r + 1] == new_radius and R["cost"][i, r + 1] == R["cost_new"][i, r], (i, r)


def host_rounds(march, solve, trial, full_cost, u0, n_rounds, radius0, radius_max, radius_min):
    """The host loop of GD_1D.trust_refine / GD2_configured.trust_refine over three engine calls, with the verdicts of
    `judge`: march(u) makes u the base point, solve(u, radius) -> the dict of hess_cg_trust (batch 1), trial() -> the control
    of newton_trial(1), full_cost(u) -> J of a march of u.  -> (u, records); the loop ends with the trajectory."""
    u, radius = np.array(u0), float(radius0)
    cost = full_cost(u)
    recs = []
    for _ in range(n_rounds):
        march(u)
        S = solve(u, radius)
        rec = dict(cost=cost, cost_new=cost, radius=radius, steps=int(S["steps"][0]), cg_status=int(S["status"][0]),
                   n_free=int(S["n_free"][0]), status=None)
        recs.append(rec)
        assert rec["n_free"] >= 1 and S["rnorm0"][0] > 0.0 and rec["cg_status"] in (LIMIT, CONVERGED, NEGCURV, BOUNDARY)
        t = trial()
        J = full_cost(t)
        rec["status"], _, radius, ended = judge(cost, float(S["pred"][0]), J, float(S["xnorm"][0]), rec["cg_status"], radius, radius_max,
                                                radius_min)
        if rec["status"] == ACCEPTED:
            u, cost, rec["cost_new"] = t, J, J
        if ended:
            break
    return u, recs


def off_block_members(q, box_cut, dnorm):
    """The batch of three of the rounds off one block, for either engine (box_cut and dnorm are the engine's helpers).
    Member 0: b3 = 1 from the control cut to 0.7 of its amplitude inside the box at 0.75 of it, in a twentieth of its norm:
    the Newton step is about -u, so the solve leaves the region (BOUNDARY).  Member 1: the same start with b3 = -100, far
    below the reduced Hessian of the tracking terms in the mass norm (b1 T^2 + b2 T, 0.3 at T = 0.03 and 2.2 at T = 0.2,
    bounds it for a march that does not amplify): the first CG direction has negative curvature (NEGCURV).  Member 2: the
    box-cut start of the damped rounds' tests inside ten times its norm: the trial is clipped to the bound 2^-20 below, gains
    less than a quarter of pred, and the radius is quartered.  -> (opts, u0, radius0)."""
    mk = q.V.make_opt
    top = float(np.abs(q.u).max())
    u = np.clip(q.u, -0.7 * top, 0.7 * top)
    cut, half = box_cut(q)
    opts = [mk(b3=1.0, u_min=-0.75 * top, u_max=0.75 * top), mk(b3=-100.0, u_min=-0.75 * top, u_max=0.75 * top), cut]
    return opts, np.stack([u, u, half]), np.array([0.05 * dnorm(q, u, True), 0.02 * dnorm(q, u, True), 10.0 * dnorm(q, half, True)])
