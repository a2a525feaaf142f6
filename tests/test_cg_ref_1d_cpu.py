"""CPU side of the device-resident Newton-CG step of the 1D engine (vch1d_hess_cg).  No GPU.

1. The NumPy restatement tests/_cg_ref.py with the 1D preconditioner D = diag(wt'_k wx_i), wt' the trapezoid weights of
   t_hist with wt'_0 := wt_1 (row 0 has quadrature weight zero but is a real unknown), on the dense Hessian of J1 + J2 + J3
   at N = 8, 3 steps (5 rows of 9 nodes), assembled column by column from the NumPy transposed-sweep reference
   tests/_adjoint_ref_1d.py and symmetrised.  With b3 = 1 every block that leaves a node of row 0 out is positive definite.
   The whole matrix is not: a control that is constant in x on row 0 alone shifts the mass of step 0, which the mean
   removal takes out again, and row 0 has no b3 term of its own (wt_0 = 0), so that direction has no curvature at all
   (asserted below).  The free sets here leave node (0, N) out.  Bounds: a converged run ends
   with the recurrence residual at most cg_tol ||P b||, so x is within cond cg_tol of np.linalg.solve; asserted at
   cond 1.2e-8 for cg_tol = 1e-8 (the 20 % margin of DESIGN.md 10g).  pred = b.x - x.Ax / 2 holds in exact arithmetic for
   every CG iterate; both sides are sums of at most 45 + steps terms of size |b|.|x|, asserted at 100 eps of that.
2. The entry points exist at every layer: the shared library exports vch1d_hess_cg and vch1d_cg_vector, _lib.SIGNATURES
   binds both, Engine1D has hess_cg and cg_vector, the drivers have reduced_newton_step and newton_refine."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

from oracle import vch1d_oracle as o
from _adjoint_ref_1d import adjoint_reference_1d, trapz_nodes
from _cg_ref import CONVERGED, cg

EPS = np.finfo(np.float64).eps
SOLVE = 1.2e-8
WEIGHTS = (5.0, 10.0, 1.0)


def mass_1d(t_hist, x):
    """D of vch1d_hess_cg in the shape of a control: wt'_k wx_i with wt'_0 := wt_1."""
    wt = trapz_nodes(t_hist)
    wt[0] = wt[1]
    return wt[:, None] * trapz_nodes(x)[None, :]


@pytest.fixture(scope="module")
def dense():
    P = o.Params1D(N=8, T=0.03, dt_initial=0.01)
    x = np.linspace(0.0, P.Lx, P.N + 1)
    rows = 5
    u = np.stack([0.5 * np.cos(np.pi * x * (1 + k % 2)) * np.sin(1 + k) for k in range(rows)])
    phi, x, t = o.forward(P, control=u, initial_phi=0.2 * np.cos(np.pi * x / P.Lx))
    assert phi.shape == u.shape == (rows, 9) and np.abs(phi).max() < 1.0 - o.DELTA_SEP - 0.1
    rng = np.random.default_rng(3)
    phi_Q, phi_T = 0.1 * rng.standard_normal(phi.shape), 0.1 * rng.standard_normal(9)
    cols = []
    for j in range(u.size):
        e = np.zeros(u.size)
        e[j] = 1.0
        cols.append(adjoint_reference_1d(P, phi, t, x, u, phi_Q, phi_T, *WEIGHTS, h=e.reshape(u.shape))[1].ravel())
    H = np.array(cols).T
    assert np.abs(H - H.T).max() <= 1e-10 * np.abs(H).max()
    return dict(A=0.5 * (H + H.T), D=mass_1d(t, x).ravel(), t=t, shape=u.shape, rng=rng)


def test_row_zero_takes_the_weight_of_row_one(dense):
    D = dense["D"].reshape(dense["shape"])
    assert (D > 0).all() and np.array_equal(D[0], D[1])
    assert trapz_nodes(dense["t"])[0] == 0.0                        # the weight the preconditioner must not divide by


def test_a_constant_on_row_zero_has_no_curvature(dense):
    A = dense["A"]
    h = np.zeros(dense["shape"])
    h[0] = 1.0
    assert np.abs(A @ h.ravel()).max() <= 1e-12 * np.abs(A).max()


@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("n_free", [3, 12, 40])
def test_restatement_with_the_1d_preconditioner_solves_the_block(dense, precond, n_free):
    A, D, rng = dense["A"], dense["D"], np.random.default_rng(n_free)
    n = A.shape[0]
    mask = np.zeros(n, dtype=bool)
    last0 = dense["shape"][1] - 1                                   # node (0, N) stays out: see the docstring
    mask[rng.choice(np.delete(np.arange(n), last0), n_free, replace=False)] = True
    mask[0] = True                                                  # a node of row 0 is always among the free ones
    free = np.flatnonzero(mask)
    blk = A[np.ix_(free, free)]
    ev = np.linalg.eigvalsh(blk)
    assert ev[0] > 0.0
    cond = ev[-1] / ev[0]
    b = rng.standard_normal(n)
    R = cg(lambda v: A @ v, mask, b, 4 * n, 1e-8, D if precond else None)
    want = np.linalg.solve(blk, b[free])
    err = np.abs(R["x"][free] - want).max() / np.abs(want).max()
    model = float(b[free] @ R["x"][free] - 0.5 * R["x"] @ (A @ R["x"]))
    scale = float(np.abs(b[free]) @ np.abs(R["x"][free]))
    print(f"MEASURE 1d restatement n_free {len(free)} precond {precond}: steps {R['steps']} cond {cond:.3g} error {err:.2e} "
          f"pred dev {abs(R['pred'] - model) / scale:.2e}")
    assert R["status"] == CONVERGED and R["n_free"] == len(free) and np.isfinite(R["resid"][:R["steps"]]).all()
    assert not R["x"][~mask].any() and not R["r"][~mask].any() and not R["p"][~mask].any()
    assert err <= cond * SOLVE
    assert abs(R["pred"] - model) <= 100 * EPS * scale


def test_the_entry_points_exist_at_every_layer():
    import vch_amd
    vch_amd.build()
    lib = ctypes.CDLL(vch_amd.LIB_PATH)
    sigs = import_module(vch_amd.PKG_NAME + "._lib").SIGNATURES
    for name in ("vch1d_hess_cg", "vch1d_cg_vector"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in sigs, f"{name} has no ctypes signature"
    assert callable(getattr(vch_amd.Engine1D, "hess_cg", None)) and callable(getattr(vch_amd.Engine1D, "cg_vector", None))
    assert vch_amd.Engine1D.CG_STATUS == vch_amd.Engine2D.CG_STATUS
    assert callable(getattr(vch_amd.module("Vch_control_1D.second_order_conditions"), "reduced_newton_step", None))
    assert callable(getattr(vch_amd.module("Vch_control_1D.GD_1D"), "newton_refine", None))
