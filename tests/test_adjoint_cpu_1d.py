"""Pins the CPU reference of the transposed tangent sweeps (tests/_adjoint_ref_1d.py: the exact gradient field G and the
Hessian-vector product H h behind vch1d_hessvec) against the tangent reference (tests/_tangent_ref_1d.py, itself pinned
against central differences of the oracle's march by test_tangent_cpu_1d.py).  No GPU.

Problems: `n32` and `n33_off` of test_gpu_second_order_1d.py (trajectory 0: its start, its control), the history marched
by the oracle; phi_Q, phi_T and the directions h, g are seeded standard-normal fields.  Four identities, each deviation
relative to the sum of the absolute values of the terms of the node sum on its left:
    gh     sum(G h)    = s_state + s_ctrl                                  of tangent_scalars_1d
    hHh    sum(h Hh)   = c_gn + c_state + c_ctrl
    polar  sum(g Hh)   = (J''[g+h, g+h] - J''[g-h, g-h]) / 4               by three more tangent references
    sym    sum(g Hh)   = sum(h Hg)
Measured / asserted (10 x measured, rounded up, and no less than EPS = 2.3e-16: one rounding of the sum itself, which a
measured 0 or a lucky cancellation of roundings must not undercut):
                gh                    hHh                   polar                 sym
    n32         2.05e-17 / 2.3e-16    1.32e-16 / 1.4e-15    1.13e-17 / 2.3e-16    1.69e-17 / 2.3e-16
    n33_off     3.37e-17 / 3.4e-16    7.77e-17 / 7.8e-16    0        / 2.3e-16    4.27e-17 / 4.3e-16
Without the source -c1 rho(phi*) yp v_k of the second sweep the hHh identity misses by 3.02e-3 relative, twelve orders
above its bound: the check can fail."""
import numpy as np
import pytest

from oracle import vch1d_oracle as o
from _adjoint_ref_1d import adjoint_reference_1d, lap_t, transpose_rows, trapz_nodes
from _tangent_ref_1d import tangent_reference_1d, tangent_scalars_1d
from test_gpu_second_order_1d import _problem

#              gh, hHh, polar, sym
EPS = 2.3e-16
BOUNDS = {"n32": (EPS, 1.4e-15, EPS, EPS), "n33_off": (3.4e-16, 7.8e-16, EPS, 4.3e-16)}
WEIGHTS = (5.0, 10.0, 1e-4)
RHO_MISS = 1e-3          # without the rho source hHh is off by more than this (measured 3.02e-3)


@pytest.fixture(scope="module")
def setups():
    import vch_amd
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        pr = _problem(vch_amd, name)
        P, u = pr["P"], pr["U"][0]
        phi, x, t = o.forward(P, control=u, initial_phi=pr["phi0"][0])
        assert phi.shape == u.shape and np.abs(phi).max() < 1.0 - o.DELTA_SEP - 0.1
        rng = np.random.default_rng(11)
        phi_Q, phi_T = rng.standard_normal(phi.shape), rng.standard_normal(phi.shape[1])
        h, g = rng.standard_normal(phi.shape), rng.standard_normal(phi.shape)
        ref = lambda d, omit=(): adjoint_reference_1d(P, phi, t, x, u, phi_Q, phi_T, *WEIGHTS, h=d, omit=omit)

        def curvature(d):
            d1, d2 = tangent_reference_1d(P, phi, t, d)
            return tangent_scalars_1d(phi, d1, d2, u, d, phi_Q, phi_T, x, t, *WEIGHTS)

        cache[name] = dict(P=P, u=u, phi=phi, x=x, t=t, h=h, g=g, ref=ref, curvature=curvature, Gh=ref(h), Gg=ref(g))
        return cache[name]

    return get


def _dev(field_a, field_b, want):
    """|sum(a b) - want| relative to sum |a b|."""
    return abs(float(np.sum(field_a * field_b)) - want) / float(np.sum(np.abs(field_a * field_b)))


@pytest.mark.parametrize("name", list(BOUNDS))
def test_four_identities_against_the_tangent_reference(setups, name):
    m = setups(name)
    h, g = m["h"], m["g"]
    (G, Hh), (G2, Hg) = m["Gh"], m["Gg"]
    assert np.array_equal(G, G2)                                     # the gradient does not depend on the direction
    S = m["curvature"](h)
    polar = (m["curvature"](g + h)["curvature"] - m["curvature"](g - h)["curvature"]) / 4.0
    devs = (_dev(G, h, S["slope"]), _dev(h, Hh, S["curvature"]), _dev(g, Hh, polar), _dev(g, Hh, float(np.sum(h * Hg))))
    print(f"{name}: gh {devs[0]:.2e} hHh {devs[1]:.2e} polar {devs[2]:.2e} sym {devs[3]:.2e}")
    for d, b, what in zip(devs, BOUNDS[name], ("gh", "hHh", "polar", "sym")):
        assert d < b, (what, d, b)
    # Euclidean convention: row 0 has quadrature weight 0 but drives step 0; the last row keeps its b3 term alone
    assert G[0].any() and Hh[0].any()
    last = WEIGHTS[2] * (trapz_nodes(m["t"])[-1] * trapz_nodes(m["x"])) * m["u"][-1]
    assert np.array_equal(G[-1], last) and trapz_nodes(m["t"])[0] == 0.0
    without_h = adjoint_reference_1d(m["P"], m["phi"], m["t"], m["x"], m["u"], np.zeros_like(h), np.zeros(h.shape[1]), 0.0, 0.0,
                                     WEIGHTS[2])
    assert without_h[1] is None and np.array_equal(without_h[0][-1], last)


def test_the_check_can_fail_without_the_curvature_source(setups):
    m = setups("n32")
    h = m["h"]
    _, Hh = m["ref"](h, omit=("rho",))
    d = _dev(h, Hh, m["curvature"](h)["curvature"])
    print(f"n32 without rho: hHh {d:.2e}")
    assert d > RHO_MISS > 1e9 * BOUNDS["n32"][1]


def test_transposes():
    """transpose_rows and lap_t against dense transposes."""
    P = o.Params1D(N=9, Lx=1.3)
    hx = P.Lx / P.N
    rng = np.random.default_rng(2)
    p, v = 0.5 * rng.uniform(-1, 1, P.N + 1), rng.standard_normal(P.N + 1)
    rows = o.newton_rows(p, 0.01, P, hx)
    dense = lambda r: np.stack([o._rows_matvec(r, e) for e in np.eye(2 * (P.N + 1))], axis=1)
    assert np.array_equal(dense(transpose_rows(rows)), dense(rows).T)
    want = o.lap_dense(P.N, hx).T @ v
    assert np.abs(lap_t(v, hx) - want).max() <= 4 * np.finfo(float).eps * np.abs(want).max()


def test_zero_direction_gives_zero_product(setups):
    m = setups("n33_off")
    G, Hz = m["ref"](np.zeros_like(m["h"]))
    assert not Hz.any() and np.array_equal(G, m["Gh"][0])
