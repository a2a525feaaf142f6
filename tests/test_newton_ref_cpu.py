"""CPU side of the device-resident damped Newton rounds of the 2D engine (vch2d_pgd_newton).  No GPU.

1. The NumPy restatement tests/_newton_ref.py on a small convex problem: J(u) = u.Au / 2 - c.u + kappa sum w_i |u_i| on a
   box, A symmetric positive definite (48 unknowns, condition 20), the weights w also the preconditioner D.  As in its use
   after the PGD loop, the rounds start from a proximal-gradient iterate (60 steps of length 1 / lambda_max from zero),
   whose zeros and bound nodes are exact and are not free.  The minimiser is checked by its KKT conditions with
   g = A u - c: on free nodes g + kappa w sign(u) = 0, on zeros |g| <= kappa w, on the lower / upper bound the one-sided
   sign.  For a quadratic the full step from a converged solve leaves the free gradient at the recurrence residual, at
   most cg_tol ||P b|| with ||P b|| the first round's right-hand side; asserted at the solve class 1.2e-8 (cg_tol = 1e-8
   and the 20 % margin of DESIGN.md 10g) relative to that norm.  The inequalities are asserted with the same slack.
2. Each end state of a round on a problem made for it.
3. The entry points exist at every layer."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

import _newton_ref as nr
from _cg_ref import CONVERGED

SOLVE = 1.2e-8


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(11)
    n = 48
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.geomspace(1.0, 20.0, n)
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    w = 0.5 + rng.random(n)
    c = 3.0 * rng.standard_normal(n)
    kappa, lo, hi = 1.0, -0.6, 0.8
    # the proximal-gradient iterate the rounds start from
    u, step = np.zeros(n), 1.0 / lam[-1]
    for _ in range(60):
        v = u - step * (A @ u - c)
        u = np.clip(np.sign(v) * np.maximum(np.abs(v) - step * kappa * w, 0.0), lo, hi)
    return dict(A=A, c=c, w=w, kappa=kappa, lo=lo, hi=hi, u0=u)


def kkt(p, u):
    """-> the largest violation of each KKT condition and the node counts (free, zero, lower, upper)."""
    g = p["A"] @ u - p["c"]
    kw = p["kappa"] * p["w"]
    zero, low, up = u == 0.0, u == p["lo"], u == p["hi"]
    free = ~(zero | low | up)
    assert ((u >= p["lo"]) & (u <= p["hi"])).all()
    v_free = np.abs(g + kw * np.sign(u))[free].max(initial=0.0)
    v_zero = np.maximum(np.abs(g) - kw, 0.0)[zero].max(initial=0.0)
    # J may not fall inwards: at the lower bound (< 0) g - kw >= 0, at the upper bound (> 0) g + kw <= 0
    assert p["lo"] < 0.0 < p["hi"]
    v_low = np.maximum(-(g - kw), 0.0)[low].max(initial=0.0)
    v_up = np.maximum(g + kw, 0.0)[up].max(initial=0.0)
    return (v_free, v_zero, v_low, v_up), (int(free.sum()), int(zero.sum()), int(low.sum()), int(up.sum()))


def test_rounds_from_a_pgd_iterate_reach_the_minimiser(problem):
    p = problem
    viol0, counts = kkt(p, p["u0"])
    assert min(counts) >= 3, counts                              # every kind of node is there
    u, recs = nr.newton_rounds(p["A"], p["c"], p["kappa"], p["w"], p["u0"].copy(), p["lo"], p["hi"], 3, k=200, cg_tol=1e-8,
                               D=p["w"])
    viol, counts1 = kkt(p, u)
    rn0 = recs[0]["rnorm0"]
    print(f"MEASURE newton restatement: start violations {viol0}, counts {counts} -> {counts1}; rounds "
          f"{[(r['status'], r['s'], r.get('cg_steps')) for r in recs]}; rnorm0 {rn0:.3e}; final violations {viol}")
    assert recs[0]["status"] == nr.ACCEPTED and recs[0]["s"] == 1.0 and recs[0]["cg_status"] == CONVERGED
    assert recs[0]["n_free"] == counts[0]
    assert viol0[0] > 1e3 * SOLVE * rn0                          # the start is not the minimiser: the rounds have work to do
    costs = [recs[0]["cost"]] + [r["cost_new"] for r in recs if r["status"] != nr.IDLE]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert max(viol) <= SOLVE * rn0
    # after the first full step the free gradient is the recurrence residual of the solve
    u1, _ = nr.newton_round(p["A"], p["c"], p["kappa"], p["w"], p["u0"].copy(), p["lo"], p["hi"], k=200, cg_tol=1e-8, D=p["w"])
    assert kkt(p, u1)[0][0] <= SOLVE * rn0


def test_trial_clips_and_pins():
    u = np.array([0.5, -0.5, 0.3, 0.0, 0.7])
    x = np.array([-1.0, 1.0, 1.0, 1.0, -0.1])
    free = nr.free_set(u, -0.6, 0.8)
    assert free.tolist() == [True, True, True, False, True]
    t, pinned, clipped = nr.trial(u, x, 1.0, -0.6, 0.8, free)
    assert t.tolist() == [0.0, 0.0, 0.8, 0.8, 0.7 - 0.1] and (pinned, clipped) == (2, 2)
    t, pinned, clipped = nr.trial(u, x, 0.5, -0.6, 0.8, free)
    assert t.tolist() == [0.0, 0.0, 0.8, 0.5, 0.7 - 0.05] and (pinned, clipped) == (0, 0)


def test_end_states():
    n = 6
    A, w, c = np.diag(2.0 ** np.arange(n)), np.ones(n), np.ones(n)      # powers of two: the gradients below are exact
    # an empty free set (u = 0) and a vanishing right-hand side are both STATIONARY; later rounds are IDLE
    u, recs = nr.newton_rounds(A, c, 0.5, w, np.zeros(n), -1.0, 1.0, 2)
    assert [r["status"] for r in recs] == [nr.STATIONARY, nr.IDLE] and recs[0]["n_free"] == 0 and not u.any()
    ustar = (c - 0.5) / np.diag(A)
    u, recs = nr.newton_rounds(A, c, 0.5, w, ustar, -1.0, 2.0, 1)
    assert recs[0]["status"] == nr.STATIONARY and recs[0]["n_free"] == n and recs[0]["rnorm0"] == 0.0
    assert np.array_equal(u, ustar)
    # non-positive curvature in the first direction
    _, recs = nr.newton_rounds(-A, c, 0.0, w, np.full(n, 0.5), -1.0, 1.0, 2)
    assert [r["status"] for r in recs] == [nr.NEGCURV, nr.IDLE] and recs[0]["cg_steps"] == 0 and recs[0]["s"] is None
    # a breakdown: a finite right-hand side (5e119) whose curvature p.Ap = 1e120 (5e119)^2 overflows; no trial is made
    B = A.copy()
    B[0, 0] = 1e120
    with np.errstate(over="ignore", invalid="ignore"):
        u, recs = nr.newton_rounds(B, c, 0.0, w, np.full(n, 0.5), -1.0, 1.0, 1)
    assert recs[0]["status"] == nr.BREAKDOWN and recs[0]["s"] is None and np.array_equal(u, np.full(n, 0.5))


def test_a_step_the_box_cuts_short_is_halved_or_stalls():
    """One unknown, J = u^2 / 2 - u from u = 0.5 with the upper bound 1e-6 above it: the Newton step is 0.5 with
    pred = 0.125, every trial is clipped to the bound and gains about 5e-7, which is a sufficient decrease
    1e-4 s pred = 1.25e-5 s only from s = 1/32 on, the fifth halving."""
    A, c, w, u0, hi = np.array([[1.0]]), np.array([1.0]), np.array([1.0]), np.array([0.5]), 0.5 + 2.0 ** -20
    u, recs = nr.newton_rounds(A, c, 0.0, w, u0, -1.0, hi, 2, max_halvings=3)
    assert [r["status"] for r in recs] == [nr.STALLED, nr.IDLE] and recs[0]["halvings"] == 3 and recs[0]["clipped"] == 1
    assert recs[0]["pred"] == 0.125 and recs[0]["cost_new"] == recs[0]["cost"] and np.array_equal(u, u0)
    u, recs = nr.newton_rounds(A, c, 0.0, w, u0, -1.0, hi, 1, max_halvings=10)
    assert recs[0]["status"] == nr.ACCEPTED and recs[0]["s"] == 1.0 / 32 and recs[0]["halvings"] == 5 and u[0] == hi
    assert recs[0]["cost_new"] < recs[0]["cost"]


def test_the_entry_points_exist_at_every_layer():
    import vch_amd
    vch_amd.build()
    lib = ctypes.CDLL(vch_amd.LIB_PATH)
    sigs = import_module(vch_amd.PKG_NAME + "._lib").SIGNATURES
    for name in ("vch2d_pgd_newton", "vch2d_newton_trial"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in sigs, f"{name} has no ctypes signature"
    assert callable(getattr(vch_amd.Engine2D, "pgd_newton", None)) and callable(getattr(vch_amd.Engine2D, "newton_trial", None))
    assert vch_amd.Engine2D.NEWTON_STATUS == ("accepted", "stationary", "negcurv", "breakdown", "stalled", "idle")
    import inspect
    gd2 = vch_amd.module("Vch_control_2D.GD2_configured")
    assert inspect.signature(gd2.newton_refine).parameters["on_device"].default is False
    assert inspect.signature(gd2.run_sweep).parameters["n_newton"].default == 0
