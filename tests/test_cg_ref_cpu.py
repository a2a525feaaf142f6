"""Pins tests/_cg_ref.py, the NumPy restatement of the device-resident Newton-CG iteration: on synthetic symmetric
matrices with a random mask it solves the masked block (SPD), reports the model decrease b.x - x.Ax / 2, leaves masked-off
nodes exact zeros, and on an indefinite matrix it exits with a direction of non-positive curvature; the other stops fire.

Bounds.  A converged run ends with the recurrence residual at most cg_tol ||P b||; in exact arithmetic that is the true
residual, in floating point the two differ by the accumulated round-off of the updates, O(steps eps cond) relative to
||P b|| (Greenbaum 1997), far below the cg_tol = 1e-10 used here at cond <= 1e3, so the true residual is asserted at
2 cg_tol and the solution at 2 cg_tol cond."""
import numpy as np
import pytest

from _cg_ref import BREAKDOWN, CONVERGED, LIMIT, NEGCURV, cg

EPS = 2.3e-16


def _matrix(n, seed, lam):
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (U * lam) @ U.T
    return 0.5 * (A + A.T), rng


def _mask(n, n_free, rng):
    mask = np.zeros(n, dtype=bool)
    mask[rng.choice(n, n_free, replace=False)] = True
    return mask


@pytest.mark.parametrize("n_free", [3, 24, 190])
@pytest.mark.parametrize("precond", [False, True])
def test_spd_solve_and_the_model_decrease(n_free, precond):
    n = 2 * n_free + 5
    A, rng = _matrix(n, n_free, np.logspace(-9, -6, n))
    D = rng.uniform(0.25, 1.0, n) if precond else None
    if precond:                                                     # a matrix whose spread is mostly its diagonal scaling
        A = np.sqrt(D)[:, None] * A * np.sqrt(D)[None, :]
    mask, b = _mask(n, n_free, rng), rng.standard_normal(n)
    blk = A[np.ix_(mask, mask)]
    cond = np.linalg.cond(blk)
    R = cg(lambda v: A @ v, mask, b, k=4 * n, cg_tol=1e-10, D=D)
    assert R["status"] == CONVERGED and R["n_free"] == n_free and 1 <= R["steps"] <= 4 * n
    x, m = R["x"], R["steps"]
    assert not x[~mask].any() and not R["r"][~mask].any() and not R["p"][~mask].any()
    true = np.linalg.norm(b[mask] - blk @ x[mask]) / np.linalg.norm(b[mask])
    want = np.linalg.solve(blk, b[mask])
    err = np.abs(x[mask] - want).max() / np.abs(want).max()
    print(f"MEASURE n_free {n_free} precond {precond}: steps {m} cond {cond:.1e} true residual {true:.2e} error {err:.2e}")
    assert R["resid"][m - 1] <= 1e-10 and true <= 2e-10 and err <= 2e-10 * cond
    assert np.isfinite(R["resid"][:m]).all() and np.isnan(R["resid"][m:]).all()
    assert np.isfinite(R["curv"][:m]).all() and np.isnan(R["curv"][m:]).all()
    assert R["rnorm0"] == np.linalg.norm(np.where(mask, b, 0.0))
    # pred is the decrease of the quadratic model at x
    model = float(b @ x - 0.5 * x @ (A @ x))
    assert abs(R["pred"] - model) <= 10 * n * EPS * abs(model) + 2e-10 * abs(model)
    # every curvature is a Rayleigh quotient of D^-1/2 A D^-1/2 on the free set
    s = np.ones(n_free) if D is None else 1.0 / np.sqrt(D[mask])
    ev = np.linalg.eigvalsh(s[:, None] * blk * s[None, :])
    assert (R["curv"][:m] >= ev[0] * (1 - 1e-12)).all() and (R["curv"][:m] <= ev[-1] * (1 + 1e-12)).all()


def test_the_preconditioner_removes_a_diagonal_spread():
    n = 60
    A0, rng = _matrix(n, 7, np.linspace(1.0, 1.5, n))
    D = rng.choice([0.25, 0.5, 1.0], n)
    A = np.sqrt(D)[:, None] * A0 * np.sqrt(D)[None, :]
    b, mask = rng.standard_normal(n), np.ones(n, dtype=bool)
    plain = cg(lambda v: A @ v, mask, b, k=200, cg_tol=1e-10)
    pre = cg(lambda v: A @ v, mask, b, k=200, cg_tol=1e-10, D=D)
    print(f"MEASURE steps without {plain['steps']} with {pre['steps']}")
    assert plain["status"] == pre["status"] == CONVERGED and pre["steps"] < plain["steps"]


def test_an_indefinite_matrix_exits_with_a_direction_of_non_positive_curvature():
    n = 40
    A, rng = _matrix(n, 8, np.concatenate([-np.logspace(-8, -7, 12), np.logspace(-9, -6, n - 12)]))
    mask, b = _mask(n, 30, rng), rng.standard_normal(n)
    R = cg(lambda v: A @ v, mask, b, k=200)
    j, p = R["steps"], R["p"]
    assert R["status"] == NEGCURV and j < 30
    assert p @ (A @ p) <= 0.0 and not p[~mask].any()
    assert R["curv"][j] == (p @ np.where(mask, A @ p, 0.0)) / (p @ p) and R["curv"][j] <= 0.0
    assert np.isnan(R["resid"][j:]).all() and np.isnan(R["curv"][j + 1:]).all() and (R["curv"][:j] > 0).all()
    # x is the iterate before that direction: the model decrease of the steps taken
    x = R["x"]
    model = float(np.where(mask, b, 0.0) @ x - 0.5 * x @ (A @ x))
    assert abs(R["pred"] - model) <= 1e-10 * abs(model) + 1e-300


def test_a_negative_definite_matrix_exits_at_step_zero_with_p_the_scaled_right_hand_side():
    n = 12
    A, rng = _matrix(n, 9, -np.logspace(-9, -6, n))
    D, b, mask = rng.uniform(0.25, 1.0, n), rng.standard_normal(n), _mask(n, 7, rng)
    R = cg(lambda v: A @ v, mask, b, k=5, D=D)
    assert R["status"] == NEGCURV and R["steps"] == 0 and not R["x"].any() and R["pred"] == 0.0
    assert np.array_equal(R["p"], np.where(mask, b, 0.0) / D) and R["curv"][0] < 0 and np.isnan(R["resid"]).all()


def test_the_step_limit_a_zero_right_hand_side_and_a_non_finite_product():
    n = 30
    A, rng = _matrix(n, 10, np.logspace(-9, -3, n))
    mask, b = np.ones(n, dtype=bool), rng.standard_normal(n)
    R = cg(lambda v: A @ v, mask, b, k=4, cg_tol=1e-12)
    assert R["status"] == LIMIT and R["steps"] == 4 and np.isfinite(R["resid"]).all() and R["resid"][-1] > 1e-12
    Z = cg(lambda v: A @ v, _mask(n, 5, rng), np.zeros(n), k=4)
    assert Z["status"] == CONVERGED and Z["steps"] == 0 and not Z["x"].any() and Z["rnorm0"] == 0.0 and np.isnan(Z["resid"]).all()
    calls = []

    def apply(v):
        calls.append(1)
        return A @ v if len(calls) < 3 else np.full(n, np.nan)

    N = cg(apply, mask, b, k=9, cg_tol=1e-12)
    assert N["status"] == BREAKDOWN and N["steps"] == 2 and np.isnan(N["curv"][2])


def test_empty_free_set_and_non_finite_right_hand_side_are_errors():
    A, rng = _matrix(5, 11, np.logspace(-3, 0, 5))
    with pytest.raises(ValueError):
        cg(lambda v: A @ v, np.zeros(5, dtype=bool), np.ones(5), k=3)
    mask = np.array([True, True, False, False, False])
    with pytest.raises(ValueError):
        cg(lambda v: A @ v, mask, np.array([np.inf, 1.0, 1.0, 1.0, 1.0]), k=3)
    ok = cg(lambda v: A @ v, mask, np.array([1.0, 1.0, np.nan, 1.0, 1.0]), k=9)     # off the free set: not read
    assert ok["status"] == CONVERGED
