"""Pins the 1D CPU oracle away from the default parameters (Lx != 1, c2 != 1, ...) to golden vectors produced by the
reference itself (tests/golden/make_golden_1d_off.py), at the tolerances of test_oracle_golden_1d.py and with both of the
oracle's solvers.  CPU only.  The fixtures' inputs are the recipes of tests/_offpoint_1d.py, which the GPU tests of
test_gpu_1d_offpoint.py run the engine on."""
import numpy as np
import pytest

import _offpoint_1d as X
from conftest import golden, relerr
from oracle import vch1d_oracle as O1

TIGHT = 5e-13
SOLVE = 1e-9
POINTS = ["off", "off2"]


def _P(g):
    return O1.Params1D(N=int(g["N"]), Lx=float(g["Lx"]), T=float(g["T"]), dt_initial=float(g["dt"]), tau=float(g["tau"]),
                       gamma=float(g["gamma"]), c1=float(g["c1"]), c2=float(g["c2"]), kappa=float(g["kappa"]))


@pytest.mark.parametrize("point", POINTS)
def test_fixture_inputs_are_the_shared_recipes(point):
    g = golden(f"g1d_{point}_33.npz")
    P = _P(g)
    assert P == X.params(point, 33)
    assert np.array_equal(g["u"], X.control(P, 12.0))
    assert np.array_equal(g["phi0"], X.start(P, "smooth")) and np.array_equal(g["phi0_sep"], X.start(P, "sep"))
    c = X.capped_case(point, 33, int(g["nr_seed"]))
    assert np.array_equal(g["nr_phi"], c["phi"]) and np.array_equal(g["nr_w_new"], c["w_new"])
    assert relerr(c["mu"], g["nr_mu"]) < TIGHT


@pytest.mark.parametrize("point", POINTS)
def test_operators_off_default(point):
    g = golden(f"g1d_{point}_33.npz")
    P = _P(g)
    N, h, dt, n = P.N, P.Lx / P.N, 1e-2, P.N + 1
    assert relerr(O1.lap(g["v"], h), g["Lv"]) < TIGHT
    assert relerr(O1.lap_dense(N, h) @ g["v"], g["Lv"]) < TIGHT
    assert relerr(O1.mu_init(g["phi_old"], g["w_new"], P, h), g["mu0"]) < TIGHT
    assert relerr(O1.w_filter(g["w_old"], dt, P.gamma, g["w_new"], g["v"]), g["w_filt"]) < TIGHT
    Rp = O1.residual_phi(g["phi_new"], g["phi_old"], g["mu_new"], g["mu_old"], g["w_new"], g["w_old"], dt, P, h)
    Rm = O1.residual_mu(g["phi_new"], g["phi_old"], g["mu_new"], g["mu_old"], dt, h)
    assert relerr(Rp, g["Rphi"]) < TIGHT and relerr(Rm, g["Rmu"]) < TIGHT
    d = g["dvec"]
    J = O1.jac_dense(g["phi_new"], dt, P, O1.lap_dense(N, h))
    assert relerr(np.linalg.solve(J, d), g["Jsol"]) < 1e-10
    assert relerr(O1._solve_newton_banded(g["phi_new"], dt, P, h, -d), g["Jsol"]) < SOLVE
    top, bot = O1.jac_apply(g["phi_new"], g["Jsol"][:n], g["Jsol"][n:], dt, P, h)
    assert relerr(np.concatenate([top, bot]), d) < SOLVE
    assert relerr(O1.fpp(g["phi_old"]), g["fpp"]) < TIGHT
    assert relerr(O1.adjoint_A_apply(g["phi_new"], g["Asol"], dt, h), g["v"]) < SOLVE
    assert relerr(O1.hp_solve(O1.adjoint_rows(g["phi_new"], dt, h), g["v"]), g["Asol"]) < SOLVE
    assert relerr(O1.hp_solve(O1.adjoint_rows(None, 0.0, h, n=n), g["v"]), g["ATsol"]) < SOLVE


@pytest.mark.parametrize("point", POINTS)
def test_free_energy_history_off_default(point):
    g = golden(f"g1d_{point}_33.npz")
    P = _P(g)
    h = P.Lx / P.N
    for key, hist, kw in (("E", g["phi_u"], [{}] * 7), ("E_w", g["phi_u"], [dict(w=w) for w in g["w_hist"]]),
                          ("E_sep_eps", g["phi_sep_u"], [dict(eps=0.5 * O1.DELTA_SEP)] * 7)):
        E = np.array([O1.free_energy(ph, P.kappa, P.c1, P.c2, h, **k) for ph, k in zip(hist, kw)])
        assert np.all(np.abs(E - g[key]) <= 1e-13 * np.maximum(1.0, np.abs(g[key]))), key
    assert np.max(np.abs(g["E"] - g["E_w"])) > 1e-3            # the coupling term is there


@pytest.mark.parametrize("solver", ["dense", "banded"])
@pytest.mark.parametrize("point", POINTS)
def test_newton_call_off_default(point, solver):
    """The capped-step call: the first step is cut by the ceiling 0.9 amax < 1."""
    g = golden(f"g1d_{point}_33.npz")
    P = _P(g)
    st = {}
    pn, mn, hist = O1.newton_step(g["nr_phi"], g["nr_mu"], g["nr_w_old"], g["nr_w_new"], float(g["nr_dt"]), P, P.Lx / P.N,
                                  solver=solver, return_history=True, stats=st)
    assert len(hist) == len(g["nr_hist"]) and np.allclose(hist[:-1], g["nr_hist"][:-1], rtol=1e-6)
    assert relerr(pn, g["nr_phi_new"]) < SOLVE and relerr(mn, g["nr_mu_new"]) < SOLVE
    assert st["exits"] == [("conv", len(hist), 0, 1)]


@pytest.mark.parametrize("solver", ["dense", "banded"])
@pytest.mark.parametrize("point", POINTS)
def test_forward_backward_cost_off_default(point, solver):
    g = golden(f"g1d_{point}_33.npz")
    P = _P(g)
    o = X.PGD_OPT
    for kind, nat, ctl in (("smooth", "phi_nat", "phi_u"), ("sep", "phi_sep_nat", "phi_sep_u")):
        ic = X.start(P, kind)
        phi, x, t = O1.forward(P, initial_phi=ic, solver=solver)
        assert np.array_equal(t, g["t_hist"]) and np.array_equal(x, g["x"]) and t[0] == t[1] == 0.0
        assert relerr(phi, g[nat]) < SOLVE, kind
        phi_u, _, _ = O1.forward(P, control=g["u"], initial_phi=ic, solver=solver)
        assert relerr(phi_u, g[ctl]) < SOLVE, kind
    phi_s, _, _ = O1.forward(P, control=g["u"][:X.M], initial_phi=X.start(P, "smooth"), solver=solver)
    assert relerr(phi_s, g["phi_ushort"]) < SOLVE
    assert relerr(g["phi_ushort"], g["phi_u"]) > 1e-6                      # the hold-last branch is visible
    phi_T, phi_Q = O1.build_targets(x, t, g["phi_nat"][0], P.Lx, P.T, 1, 1)
    assert relerr(phi_T, g["phi_T"]) < 1e-15 and relerr(phi_Q, g["phi_Q"]) < 1e-15
    p, q, r = O1.backward(g["phi_u"], x, t, o["b1"], o["b2"], g["phi_Q"], g["phi_T"], solver=solver)
    assert relerr(p, g["p"]) < SOLVE and relerr(q, g["q"]) < SOLVE and relerr(r, g["r"]) < SOLVE
    assert not r[0].any() and not p[0].any()                                # B1:110 quirk
    p0, q0, r0 = O1.backward(g["phi_u"], x, t, 1.3, 0.7, None, None, solver=solver)
    assert relerr(p0, g["p_none"]) < SOLVE and relerr(q0, g["q_none"]) < SOLVE and relerr(r0, g["r_none"]) < SOLVE
    J = O1.cost(g["phi_u"], g["u_cost"], g["phi_Q"], g["phi_T"], x, t, o["b1"], o["b2"], o["b3"], o["kappa_sparsity"])
    assert abs(J - float(g["J"])) < 1e-12 * abs(float(g["J"]))
    gr = O1.gradient(g["r"], g["u_cost"], o["b3"])
    assert np.array_equal(gr, g["grad"])
    a = float(g["prox_alpha"])
    px = O1.prox_project(O1.gradient_step(g["u_cost"], gr, a), a, o["kappa_sparsity"], o["u_min"], o["u_max"])
    assert np.array_equal(px, g["prox"])
    assert (px == 0).any() and (px == o["u_min"]).any() and (px == o["u_max"]).any()
