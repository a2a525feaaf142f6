"""NumPy restatement of the damped Newton rounds of vch2d_pgd_newton for one trajectory over a dense
matrix: the cost is J(u) = u.Au / 2 - c.u + kappa sum_i w_i |u_i| on the box [lo, hi], its smooth part has the Hessian A.
The solve of a round is tests/_cg_ref.py; the verdicts are those of csrc/vch_newton.h.  Pinned by test_newton_ref_cpu.py.

    round:  free = u > lo + tol and u < hi - tol and |u| > tol
            b = -(A u - c + kappa w sign(u)) on the free set;  x = CG(P A P x = P b), at most k steps to cg_tol
            empty free set or ||P b|| == 0: STATIONARY;  CG broke down: BREAKDOWN;  first direction without positive
            curvature: NEGCURV;  otherwise x (converged, limit, or the iterate before a later negative direction) is the step
            trials s = 1, 1/2, ..., at most max_halvings halvings: t = clip(u + s x, lo, hi), a free node with t u < 0 -> 0
            the first s with J(t) <= J(u) - 1e-4 s pred is ACCEPTED;  none: STALLED, u unmoved
    a trajectory that has ended is IDLE in all later rounds"""
import numpy as np

from _cg_ref import BREAKDOWN as CG_BREAKDOWN, NEGCURV as CG_NEGCURV, cg

ACCEPTED, STATIONARY, NEGCURV, BREAKDOWN, STALLED, IDLE = range(6)


def cost(A, c, kappa, w, u):
    return float(0.5 * u @ (A @ u) - c @ u + kappa * np.sum(w * np.abs(u)))


def free_set(u, lo, hi, tol=1e-8):
    return (u > lo + tol) & (u < hi - tol) & (np.abs(u) > tol)


def trial(u, x, s, lo, hi, free):
    """-> (t, pinned, clipped): the trial control, the nodes set to the kink, the nodes the clip moved."""
    v = u + s * x
    t = np.clip(v, lo, hi)
    clipped = int(np.sum(t != v))
    pin = free & (t * u < 0.0)
    t[pin] = 0.0
    return t, int(pin.sum()), clipped


def newton_round(A, c, kappa, w, u, lo, hi, k=50, cg_tol=1e-8, D=None, tol=1e-8, max_halvings=10):
    """One round from u.  -> (u_new, record): record has cost, cost_new, s (None when nothing moved), pred, rnorm0,
    halvings, cg_steps, cg_status (None for an empty free set), status, n_free, pinned, clipped."""
    free = free_set(u, lo, hi, tol)
    J = cost(A, c, kappa, w, u)
    rec = dict(cost=J, cost_new=J, s=None, pred=0.0, rnorm0=0.0, halvings=0, cg_steps=0, cg_status=None, status=STATIONARY,
               n_free=int(free.sum()), pinned=0, clipped=0)
    if not free.any():
        return u, rec
    b = -(A @ u - c + kappa * w * np.sign(u))
    R = cg(lambda v: A @ v, free, b, k, cg_tol, D)
    rec.update(pred=R["pred"], rnorm0=R["rnorm0"], cg_steps=R["steps"], cg_status=R["status"])
    if R["rnorm0"] == 0.0:
        return u, rec
    if R["status"] == CG_BREAKDOWN:
        rec["status"] = BREAKDOWN
        return u, rec
    if R["status"] == CG_NEGCURV and R["steps"] == 0:
        rec["status"] = NEGCURV
        return u, rec
    s = 1.0
    for h in range(int(max_halvings) + 1):
        t, rec["pinned"], rec["clipped"] = trial(u, R["x"], s, lo, hi, free)
        rec["halvings"] = h
        Jt = cost(A, c, kappa, w, t)
        if Jt <= J - 1e-4 * s * R["pred"]:
            rec.update(status=ACCEPTED, s=s, cost_new=Jt)
            return t, rec
        s *= 0.5
    rec["status"] = STALLED
    return u, rec


def newton_rounds(A, c, kappa, w, u, lo, hi, n_rounds, **kw):
    """-> (u, records): the rounds until the trajectory ends; the rounds after that are IDLE records."""
    records, ended = [], False
    for _ in range(int(n_rounds)):
        if ended:
            records.append(dict(status=IDLE, s=None))
            continue
        u, rec = newton_round(A, c, kappa, w, u, lo, hi, **kw)
        records.append(rec)
        ended = rec["status"] != ACCEPTED
    return u, records
