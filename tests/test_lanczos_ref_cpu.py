"""Pins tests/_lanczos_ref.py, the NumPy restatement of the device-resident Lanczos iteration: on synthetic symmetric
matrices of order 3, 24 and 190 with spectra from 1e-9 to 1e-3 (the range of the reduced Hessian of the 12 x 9 driver
problem) and a random mask, k = n_free steps give eigvalsh of the masked block at both ends, and the early stops fire."""
import numpy as np
import pytest

from _lanczos_ref import lanczos, ritz

EPS = 2.3e-16


def _matrix(n, seed):
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(-9, -3, n)
    A = (U * lam) @ U.T
    return 0.5 * (A + A.T), rng


@pytest.mark.parametrize("n_free", [3, 24, 190])
def test_full_run_gives_the_spectrum_of_the_masked_block(n_free):
    n = 2 * n_free + 5
    A, rng = _matrix(n, n_free)
    mask = np.zeros(n, dtype=bool)
    mask[rng.choice(n, n_free, replace=False)] = True
    ev = np.linalg.eigvalsh(A[np.ix_(mask, mask)])
    R = lanczos(lambda v: A @ v, mask, rng.standard_normal(n), k=n + 7)
    assert R["n_free"] == n_free and R["steps"] <= n_free
    theta, S, res = ritz(R["alpha"], R["beta"], R["steps"])
    dev = max(abs(theta[0] - ev[0]), abs(theta[-1] - ev[-1])) / ev[-1]
    print(f"MEASURE n_free {n_free}: steps {R['steps']} extremes {dev:.2e}")
    assert dev < 10 * n * EPS
    assert np.isnan(R["alpha"][R["steps"]:]).all() and np.isnan(R["beta"][R["steps"]:]).all()
    assert not R["Q"][:, ~mask].any()                               # masked-off nodes are exact zeros
    Q = R["Q"]
    assert np.abs(Q @ Q.T - np.eye(len(Q))).max() < 10 * n * EPS


def test_the_step_limit_stops_with_a_valid_next_vector():
    A, rng = _matrix(40, 1)
    mask = np.ones(40, dtype=bool)
    R = lanczos(lambda v: A @ v, mask, rng.standard_normal(40), k=6)
    assert R["steps"] == 6 and len(R["Q"]) == 7
    Q, a, b = R["Q"], R["alpha"], R["beta"]
    for j in range(6):                                              # the three-term relation, q_6 included
        r = A @ Q[j] - a[j] * Q[j] - b[j] * Q[j + 1] - (b[j - 1] * Q[j - 1] if j else 0.0)
        assert np.abs(r).max() < 10 * 40 * EPS * 1e-3


def test_an_invariant_subspace_stops_the_iteration():
    # A = diag(A1, A2) with a 3 x 3 block A1 of norm 1e-3 and a start vector supported on it: the Krylov space is that block
    # exactly, beta_2 is round-off of size eps ||A1|| = 2e-19 and the rule's threshold 1e-14 max|alpha| is about 6e-18
    A, rng = _matrix(30, 2)
    A[:3, :] = A[:, :3] = 0.0
    A[:3, :3] = np.diag([1e-3, 5e-4, 2.5e-4])
    q0 = np.zeros(30)
    q0[:3] = 1.0
    R = lanczos(lambda v: A @ v, np.ones(30, dtype=bool), q0, k=20)
    assert R["steps"] == 3 and len(R["Q"]) == 3
    theta, _, _ = ritz(R["alpha"], R["beta"], 3)
    assert np.abs(theta - np.array([2.5e-4, 5e-4, 1e-3])).max() < 10 * 30 * EPS * 1e-3


def test_a_non_finite_product_stops_the_iteration():
    A, rng = _matrix(12, 3)
    calls = []

    def apply(v):
        calls.append(1)
        return A @ v if len(calls) < 3 else np.full(12, np.inf)

    R = lanczos(apply, np.ones(12, dtype=bool), rng.standard_normal(12), k=9)
    assert R["steps"] == 3 and not np.isfinite(R["beta"][2]) and np.isnan(R["beta"][3:]).all()


def test_the_short_recurrence_finds_the_extremes():
    A, rng = _matrix(24, 4)
    ev = np.linalg.eigvalsh(A)
    R = lanczos(lambda v: A @ v, np.ones(24, dtype=bool), rng.standard_normal(24), k=24, reorth=False)
    theta, S, res = ritz(R["alpha"], R["beta"], R["steps"])
    for th, rs in zip(theta, res):                                  # every Ritz value within its residual of an eigenvalue
        assert np.abs(ev - th).min() <= rs + 10 * 24 * EPS * ev[-1]


def test_empty_free_set_and_vanishing_start_are_errors():
    A, rng = _matrix(5, 5)
    with pytest.raises(ValueError):
        lanczos(lambda v: A @ v, np.zeros(5, dtype=bool), np.ones(5), k=3)
    mask = np.array([True, False, False, False, False])
    with pytest.raises(ValueError):
        lanczos(lambda v: A @ v, mask, np.array([0.0, 1.0, 1.0, 1.0, 1.0]), k=3)
