"""Self-test of the 1D solve checker (oracle/vch1d_oracle.py: newton_rows, adjoint_rows, backward_error, hp_solve,
cond_estimate) that tests/test_gpu_1d_levels.py holds the engine to.  CPU only.

The checker must see a one-node error at the sizes of cyclic-reduction depths 1 and 2: a solution of a system whose
last row has the interior weight 1 instead of the Neumann weight 2, or that lacks the coupling of nodes n-2 and n-1,
has a backward error >= 1e-6 in the true system, while hp_solve's has a few eps."""
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.linalg import splu

from conftest import relerr
from oracle import vch1d_oracle as O1

EPS = np.finfo(np.float64).eps
DT = 1e-3


def _lap_sparse(n, h, tail):
    """The mirrored-Neumann L as a sparse matrix; tail = "weight1": last row with the interior weight 1 on node n-2;
    "cut": no coupling between nodes n-2 and n-1."""
    lo, dg, up = O1._lap_rows(n, h)
    lo, up = lo.copy(), up.copy()
    if tail == "weight1":
        lo[-1] *= 0.5
    elif tail == "cut":
        lo[-1] = up[-2] = 0.0
    return sparse.diags([lo[1:], dg, up[:-1]], [-1, 0, 1], format="csc")


def _adjoint_sparse(phi, dt, h, tail=None):
    n = phi.size
    L = _lap_sparse(n, h, tail)
    I = sparse.identity(n, format="csc")
    return (I - O1._FROZEN.tau * L + 0.5 * dt * (L @ L) - 0.5 * dt * sparse.diags(O1.fpp(phi)) @ L).tocsc()


def _newton_wrong(rows, tail):
    rows = [v.copy() for v in rows]
    m = rows[0].size                                   # 2n, row 2i: phi equation of node i, 2i + 1: mu equation
    if tail == "weight1":
        rows[1][m - 2:] *= 0.5                         # coefficient of node n-2 in node n-1's rows
    else:
        rows[1][m - 2:] = 0.0
        rows[5][m - 4:m - 2] = 0.0                     # coefficient of node n-1 in node n-2's rows
    return rows


@pytest.mark.parametrize("N", [1025, 2051, 4095])
def test_backward_error_sees_a_one_node_tail_error(N):
    n, h = N + 1, 1.0 / N
    rng = np.random.default_rng(N)
    phi = rng.uniform(-0.9, 0.9, n)
    P = O1.Params1D(N=N)
    from scipy.linalg import solve_banded
    # adjoint step system (B1:116) and terminal system (B1:94)
    for dt in (DT, 0.0):
        rows = O1.adjoint_rows(phi, dt, h)
        b = rng.standard_normal(n)
        x_hp = O1.hp_solve(rows, b)
        assert O1.backward_error(rows, x_hp, b) <= 4 * EPS
        assert O1.backward_error(rows, solve_banded((2, 2), O1._rows_to_banded(rows), b), b) <= 4 * EPS
        # an independent assembly of the same matrix solves it as well
        A = _adjoint_sparse(phi, dt, h)
        assert O1.backward_error(rows, splu(A).solve(b), b) <= 4 * EPS
        for tail in ("weight1", "cut"):
            x_bad = splu(_adjoint_sparse(phi, dt, h, tail)).solve(b)
            assert O1.backward_error(rows, x_bad, b) >= 1e-6, (dt, tail)
    # Newton system (F1:111-137), interleaved unknowns.  LAPACK's partial pivoting is normwise, not componentwise,
    # backward stable: its omega here is 1e3 ... 1e5 eps; two steps of refinement bring it to < 1 eps.
    rows = O1.newton_rows(phi, DT, P, h)
    b = rng.standard_normal(2 * n)
    x_hp = O1.hp_solve(rows, b)
    assert O1.backward_error(rows, x_hp, b) <= 4 * EPS
    x_lu = solve_banded((3, 3), O1._rows_to_banded(rows), b)
    assert O1.backward_error(rows, x_lu, b) > 100 * EPS
    assert relerr(x_lu, x_hp) < 20 * EPS * O1.cond_estimate(rows, x_hp, b)
    for tail in ("weight1", "cut"):
        bad = _newton_wrong(rows, tail)
        x_bad = solve_banded((3, 3), O1._rows_to_banded(bad), b)
        assert O1.backward_error(rows, x_bad, b) >= 1e-6, tail


def test_newton_rows_are_jac_dense():
    """newton_rows is jac_dense with the unknowns interleaved."""
    N, h = 24, 1.0 / 24
    phi = np.random.default_rng(3).uniform(-0.9, 0.9, N + 1)
    P = O1.Params1D(N=N)
    J = O1.jac_dense(phi, DT, P, O1.lap_dense(N, h))
    perm = np.empty(2 * N + 2, dtype=int)
    perm[0::2], perm[1::2] = np.arange(N + 1), np.arange(N + 1) + N + 1
    assert np.array_equal(O1._rows_to_csc(O1.newton_rows(phi, DT, P, h)).toarray(), J[np.ix_(perm, perm)])


def test_cond_estimate_matches_dense():
    """The Skeel condition estimate against its dense value on a small adjoint system."""
    N, h = 48, 1.0 / 48
    rng = np.random.default_rng(5)
    phi = rng.uniform(-0.9, 0.9, N + 1)
    rows = O1.adjoint_rows(phi, 5e-2, h)
    b = rng.standard_normal(N + 1)
    A = O1._rows_to_csc(rows).toarray()
    x = np.linalg.solve(A, b)
    exact = np.max(np.abs(np.linalg.inv(A)) @ (np.abs(A) @ np.abs(x) + np.abs(b))) / np.max(np.abs(x))
    est = O1.cond_estimate(rows, x, b)
    assert exact / 3 <= est <= exact * (1 + 1e-12), (est, exact)


def test_stats_and_initial_phi():
    """newton_step's counts (the engine's names) and pgd's initial_phi."""
    N = 32
    P = O1.Params1D(N=N, T=0.02, dt_initial=1e-2)
    st = {}
    phi, _, _ = O1.forward(P, solver="banded", stats=st)
    assert len(st["last_norms"]) == 2 and st["failed_ls"] == 0
    assert st["newton_its"] == st["solves"] + 2 and st["armijo_trials"] >= st["solves"]
    ic = 0.3 * np.cos(np.pi * np.linspace(0, 1, N + 1))
    r0 = O1.pgd(P, O1.OptParams1D(), n_iter=1, solver="banded")
    r1 = O1.pgd(P, O1.OptParams1D(), n_iter=1, solver="banded", initial_phi=ic)
    assert np.array_equal(r0.phi[0], phi[0]) and np.array_equal(r1.phi[0], ic)
