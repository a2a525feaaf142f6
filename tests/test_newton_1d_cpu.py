"""CPU side of the device-resident damped Newton rounds of the 1D engine (vch1d_pgd_newton).  No GPU.

1. The entry points exist at every layer: the two exported symbols with their ctypes signatures, Engine1D.pgd_newton /
   newton_trial / NEWTON_STATUS, GD_1D.newton_refine(on_device=False) and GD_1D.run_sweep(n_newton=0).
2. The NumPy restatement tests/_newton_ref.py with some weights w_i = 0.  Row 0 of a 1D control has quadrature weight zero
   (the duplicated t = 0 row) but is a real unknown: it drives step 0.  A free node with w_i = 0 carries no L1 term, so its
   right-hand side is the plain gradient; it must still move with the step, and the sign test pins it only when the trial
   flips its sign.  The preconditioner follows vch1d_hess_cg: D = w except that a zero weight takes a positive one.
   Tolerance: for a quadratic the full step of a converged solve leaves the free gradient at the recurrence residual, at
   most cg_tol ||P b||; asserted at the solve class 1.2e-8 (cg_tol = 1e-8 with the 20 % margin of DESIGN.md 10g)."""
import ctypes
import inspect
from importlib import import_module

import numpy as np

import _newton_ref as nr
from _cg_ref import CONVERGED

SOLVE = 1.2e-8


def test_the_entry_points_exist_at_every_layer():
    import vch_amd
    vch_amd.build()
    lib = ctypes.CDLL(vch_amd.LIB_PATH)
    sigs = import_module(vch_amd.PKG_NAME + "._lib").SIGNATURES
    for name in ("vch1d_pgd_newton", "vch1d_newton_trial"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in sigs, f"{name} has no ctypes signature"
    assert len(sigs["vch1d_pgd_newton"][1]) == 18 and len(sigs["vch1d_newton_trial"][1]) == 5
    assert callable(getattr(vch_amd.Engine1D, "pgd_newton", None)) and callable(getattr(vch_amd.Engine1D, "newton_trial", None))
    assert vch_amd.Engine1D.NEWTON_STATUS == vch_amd.Engine2D.NEWTON_STATUS
    assert vch_amd.Engine1D.NEWTON_STATUS == ("accepted", "stationary", "negcurv", "breakdown", "stalled", "idle")
    p1, p2 = inspect.signature(vch_amd.Engine1D.pgd_newton).parameters, inspect.signature(vch_amd.Engine2D.pgd_newton).parameters
    assert [n for n in p2 if n != "rtol"] == list(p1) and "rtol" not in p1             # the 1D solves are direct
    gd1 = vch_amd.module("Vch_control_1D.GD_1D")
    assert inspect.signature(gd1.newton_refine).parameters["on_device"].default is False
    assert inspect.signature(gd1.run_sweep).parameters["n_newton"].default == 0


def _problem():
    rng = np.random.default_rng(5)
    n = 24
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.geomspace(1.0, 10.0, n)) @ Q.T
    A = 0.5 * (A + A.T)
    w = 0.5 + rng.random(n)
    w[:6] = 0.0                                          # "row 0": quadrature weight zero, real unknowns
    c = 2.0 * rng.standard_normal(n)
    u0 = 0.2 * np.sign(rng.standard_normal(n))           # every node free, off the kink and inside the box
    D = np.where(w > 0.0, w, w[6])                       # wt'_0 := wt_1
    return A, c, w, u0, D


def test_nodes_of_weight_zero_are_free_move_and_are_not_pinned_without_a_sign_flip():
    A, c, w, u0, D = _problem()
    kappa, lo, hi = 0.3, -5.0, 5.0
    zero_w = w == 0.0
    free = nr.free_set(u0, lo, hi)
    assert free.all() and zero_w.sum() == 6
    u1, rec = nr.newton_round(A, c, kappa, w, u0.copy(), lo, hi, k=200, cg_tol=1e-8, D=D)
    assert rec["status"] == nr.ACCEPTED and rec["s"] == 1.0 and rec["cg_status"] == CONVERGED and rec["n_free"] == len(u0)
    assert rec["clipped"] == 0
    # every node of weight zero moved; it sits at 0 exactly when the step flipped its sign, and the same holds for the rest
    assert (u1[zero_w] != u0[zero_w]).all()
    assert (u1[u1 != 0.0] * u0[u1 != 0.0] > 0.0).all()
    assert rec["pinned"] == int((u1 == 0.0).sum())
    assert ((u1[zero_w] == 0.0) | (u1[zero_w] * u0[zero_w] > 0.0)).all()
    # the trial itself, node by node, against the step of the solve
    from _cg_ref import cg
    b = -(A @ u0 - c + kappa * w * np.sign(u0))
    R = cg(lambda q: A @ q, free, b, 200, 1e-8, D)
    t, pinned, clipped = nr.trial(u0, R["x"], 1.0, lo, hi, free)
    assert np.array_equal(t, u1) and pinned == rec["pinned"] and clipped == 0
    flips = (u0 + R["x"]) * u0 < 0.0
    assert np.array_equal(t == 0.0, flips), "a node is pinned exactly when the trial flips its sign, whatever its weight"
    assert flips[zero_w].any() and (~flips[zero_w]).any(), "both kinds of weight-zero node are in the case"
    # where nothing was pinned the full step is the Newton point: the gradient of the smooth model vanishes on those nodes
    g = A @ (u0 + R["x"]) - c + kappa * w * np.sign(u0)
    assert np.abs(g).max() <= SOLVE * rec["rnorm0"] * np.linalg.cond(A)
    # on a weight-zero node the right-hand side is the plain gradient: no L1 term
    assert np.array_equal(b[zero_w], -(A @ u0 - c)[zero_w])


def test_a_weight_zero_node_is_pinned_only_by_its_own_sign_flip():
    """Two unknowns, both of weight zero, A = I: the step is c - u.  Node 0 crosses zero and is pinned, node 1 moves towards
    zero without crossing and keeps its value; with s = 1/2 neither crosses."""
    A, c, w = np.eye(2), np.array([-0.25, 0.125]), np.zeros(2)
    u0 = np.array([0.5, 0.5])
    free = nr.free_set(u0, -1.0, 1.0)
    x = c - u0
    t, pinned, clipped = nr.trial(u0, x, 1.0, -1.0, 1.0, free)
    assert t.tolist() == [0.0, 0.125] and (pinned, clipped) == (1, 0)
    t, pinned, clipped = nr.trial(u0, x, 0.5, -1.0, 1.0, free)
    assert t.tolist() == [0.125, 0.3125] and (pinned, clipped) == (0, 0)
    u1, rec = nr.newton_round(A, c, 0.7, w, u0.copy(), -1.0, 1.0, D=np.ones(2))
    assert rec["status"] == nr.ACCEPTED and rec["s"] == 1.0 and u1.tolist() == [0.0, 0.125] and rec["pinned"] == 1
    # the next round: node 0 sits on the kink and is not free, node 1 is stationary
    u2, rec2 = nr.newton_round(A, c, 0.7, w, u1.copy(), -1.0, 1.0, D=np.ones(2))
    assert rec2["n_free"] == 1 and rec2["status"] == nr.STATIONARY and np.array_equal(u2, u1)
