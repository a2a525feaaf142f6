"""Pins the CPU adjoint reference (tests/_adjoint_ref.py: exact gradient field G and Hessian-vector product H h of the
discrete cost, plain-transpose form) against the tangent reference (tests/_tangent_ref.py), which test_tangent_cpu.py pins
against central differences of the oracle's march.

Points: PINS["14x11"], PINS["14x11_offA"], PINS["16x16_offA"] of test_tangent_cpu (10 steps each; the mass fix is at work
on every step of the two rectangular ones), random phi_Q, phi_T, directions h and g, weights b1, b2, b3 = 0.7, 1.9, 2.3e-3.
Four identities, each error relative to the sum of the absolute values of the terms of the two sums compared:
    1. sum G h    = s_state + s_ctrl
    2. sum h Hh   = c_gn + c_state + c_ctrl        (also for a direction of 4 rows)
    3. sum g Hh   = (J''[h+g, h+g] - J''[h-g, h-g]) / 4
    4. sum g Hh   = sum h Hg
Measured (worst over the three points): 1: 3.6e-16, 2: 9.8e-17 (4 rows: 7.8e-17), 3: 2.9e-16, 4: 1.4e-16.
Bounds: ten times those, 4e-15, 1e-15, 3e-15, 1.5e-15.
Without the rho source identity 2 misses by 2.9e-4 .. 1.5e-2; without the fix's transpose identity 1 misses on 14x11 by 3.0e-4."""
import numpy as np
import pytest

from oracle import vch2d_oracle as o
import _fix_band as fb
from _adjoint_ref import adjoint_reference
from _tangent_ref import march_with_shifts, tangent_reference, tangent_scalars
from test_tangent_cpu import PINS, DT

POINTS = ("14x11", "14x11_offA", "16x16_offA")
B1, B2, B3 = 0.7, 1.9, 2.3e-3
BOUND = {1: 4e-15, 2: 1e-15, 3: 3e-15, 4: 1.5e-15}


def _build(name):
    kw, amp = PINS[name]
    P = o.Params2D(dt_initial=DT, **kw)
    xx, yy = np.meshgrid(np.linspace(0.0, 1.0, P.Nx + 1), np.linspace(0.0, 1.0, P.Ny + 1), indexing="ij")
    M = len(o.time_grid(P.T, P.dt_initial)[1])
    u = amp * np.stack([np.cos(np.pi * xx * (1 + k % 3)) * np.cos(np.pi * yy) * np.sin(1 + k) for k in range(M + 1)])
    phi, (x, y), t, shifts = march_with_shifts(P, control=u)
    rng = np.random.default_rng(7)
    m = dict(P=P, u=u, phi=phi, x=x, y=y, t=t, shifts=shifts,
             phi_Q=0.3 * rng.standard_normal(phi.shape), phi_T=0.3 * rng.standard_normal(phi.shape[1:]),
             h=rng.standard_normal(u.shape), g=rng.standard_normal(u.shape))
    return m


@pytest.fixture(scope="module")
def points():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _build(name)
        return cache[name]

    return get


def _scalars(m, h):
    d1, d2 = tangent_reference(m["P"], m["phi"], m["t"], h, m["shifts"])
    return tangent_scalars(m["phi"], d1, d2, m["u"], h, m["phi_Q"], m["phi_T"], m["x"], m["y"], m["t"], B1, B2, B3)


def _adj(m, h=None, **kw):
    return adjoint_reference(m["P"], m["phi"], m["t"], m["shifts"], m["u"], m["phi_Q"], m["phi_T"], m["x"], m["y"],
                             B1, B2, B3, h=h, **kw)


def _rel(a_terms, b):
    """|sum a_terms - b| relative to sum |a_terms| + |b|."""
    return abs(float(np.sum(a_terms)) - b) / (float(np.sum(np.abs(a_terms))) + abs(b))


@pytest.mark.parametrize("name", POINTS)
def test_shifts_are_at_work_on_the_rectangles(points, name):
    m = points(name)
    if m["P"].Nx != m["P"].Ny:
        assert np.abs(m["shifts"]).min() > 1e-6
    assert np.abs(m["phi"]).max() < 0.985 - np.abs(m["shifts"]).max()


@pytest.mark.parametrize("name", POINTS)
def test_identities(points, name):
    m = points(name)
    h, g = m["h"], m["g"]
    G, Hh = _adj(m, h)
    _, Hg = _adj(m, g)
    S = _scalars(m, h)
    e1 = _rel(G * h, S["slope"])
    e2 = _rel(h * Hh, S["curvature"])
    pol = 0.25 * (_scalars(m, h + g)["curvature"] - _scalars(m, h - g)["curvature"])
    e3 = _rel(g * Hh, pol)
    e4 = abs(float(np.sum(g * Hh)) - float(np.sum(h * Hg))) / (float(np.sum(np.abs(g * Hh))) + float(np.sum(np.abs(h * Hg))))
    h4 = h[:4]
    _, Hh4 = _adj(m, h4)
    e2r = _rel(h4 * Hh4, _scalars(m, h4)["curvature"])
    print(f"{name}: identity 1 {e1:.2e}  2 {e2:.2e} (4 rows {e2r:.2e})  3 {e3:.2e}  4 {e4:.2e}")
    assert Hh4.shape == h4.shape
    assert e1 < BOUND[1]
    assert e2 < BOUND[2] and e2r < BOUND[2]
    assert e3 < BOUND[3]
    assert e4 < BOUND[4]


def test_gradient_alone_equals_the_gradient_beside_hessvec(points):
    m = points("14x11")
    G1, none = _adj(m)
    G2, _ = _adj(m, m["h"])
    assert none is None and np.array_equal(G1, G2)


def test_without_the_rho_source_the_curvature_is_missed(points):
    for name in POINTS:
        m = points(name)
        _, Hh = _adj(m, m["h"], rho_source=False)
        e2 = _rel(m["h"] * Hh, _scalars(m, m["h"])["curvature"])
        print(f"{name}: identity 2 without the rho source {e2:.2e}")
        assert e2 > 1e3 * BOUND[2]


def test_without_the_transposed_fix_the_slope_is_missed_on_a_rectangle(points):
    m = points("14x11")
    G, _ = _adj(m, fix_transpose=False)
    e1 = _rel(G * m["h"], _scalars(m, m["h"])["slope"])
    print(f"14x11: identity 1 without the fix's transpose {e1:.2e}")
    assert e1 > 1e3 * BOUND[1]


# ------------------------------------------------------------------------------------------------------------------------
# States outside the interior band of the mass fix (tests/_fix_band.py).  The adjoint reference takes phi* and the fix's
# sets through the same _tangent_ref.fix_sets as the tangent reference, and the march's own sets from the oracle.
# Measured on the band inputs (random targets, directions and the weights above), identities 1 / 2 / 3 / 4:
#     32x16 4.2e-16 1.0e-16 4.8e-18 4.9e-18   50x36 3.9e-17 8.5e-17 1.1e-18 0   12x9 1.6e-17 1.3e-16 1.6e-16 7.2e-18
#     ambiguous (the march's own sets) 9.2e-17 0 9.8e-17 1.2e-18                  under the file's BOUND.
# Identity 1 with phi* shifted on every node: 7.2e-5 (12x9), 5.6e-4 (ambiguous); with re-derived sets on the ambiguous
# input: 2.4e-4.  Against central differences of the oracle's cost at fb.EPS = 1e-2 (test_tangent_cpu's bound 1e-5), worst over
# the five inputs and both directions: slope 9.5e-8, curvature 1.8e-6.
# ------------------------------------------------------------------------------------------------------------------------

BAND_POINTS = ("32x16", "50x36", "12x9", fb.AMBIGUOUS)


@pytest.fixture(scope="module")
def band_points():
    cache = {}

    def get(name):
        if name not in cache:
            b = fb.build(name)
            rng = np.random.default_rng(7)
            cache[name] = dict(P=b["P"], u=b["u"], phi=b["phi"], x=b["x"], y=b["y"], t=b["t"], shifts=b["shifts"],
                               masks=b["masks"], phi_Q=0.3 * rng.standard_normal(b["phi"].shape),
                               phi_T=0.3 * rng.standard_normal(b["phi"].shape[1:]), h=rng.standard_normal(b["u"].shape),
                               g=rng.standard_normal(b["u"].shape))
        return cache[name]

    return get


def _band_scalars(m, h, **kw):
    d1, d2 = tangent_reference(m["P"], m["phi"], m["t"], h, m["shifts"], masks=m["masks"], **kw)
    return tangent_scalars(m["phi"], d1, d2, m["u"], h, m["phi_Q"], m["phi_T"], m["x"], m["y"], m["t"], B1, B2, B3)


@pytest.mark.parametrize("name", BAND_POINTS)
def test_identities_outside_the_interior_band(band_points, name):
    m = band_points(name)
    h, g = m["h"], m["g"]
    G, Hh = _adj(m, h, masks=m["masks"])
    _, Hg = _adj(m, g, masks=m["masks"])
    S = _band_scalars(m, h)
    e1 = _rel(G * h, S["slope"])
    e2 = _rel(h * Hh, S["curvature"])
    pol = 0.25 * (_band_scalars(m, h + g)["curvature"] - _band_scalars(m, h - g)["curvature"])
    e3 = _rel(g * Hh, pol)
    e4 = abs(float(np.sum(g * Hh)) - float(np.sum(h * Hg))) / (float(np.sum(np.abs(g * Hh))) + float(np.sum(np.abs(h * Hg))))
    print(f"{name}: identity 1 {e1:.2e}  2 {e2:.2e}  3 {e3:.2e}  4 {e4:.2e}")
    assert e1 < BOUND[1]
    assert e2 < BOUND[2]
    assert e3 < BOUND[3]
    assert e4 < BOUND[4]
    # the transposes of the two former schemes are the transposes of other marches: each misses identity 1 against the
    # corrected tangent
    if name in (fb.AMBIGUOUS, "12x9"):
        Ga, _ = _adj(m, masks=m["masks"], pstar_all=True)
        ea = _rel(Ga * h, S["slope"])
        print(f"{name}: identity 1 with phi* shifted on every node {ea:.2e}")
        assert ea > 1e3 * BOUND[1]
    if name == fb.AMBIGUOUS:
        Gr, _ = _adj(m)
        er = _rel(Gr * h, S["slope"])
        print(f"{name}: identity 1 with re-derived sets {er:.2e}")
        assert er > 1e3 * BOUND[1]


@pytest.mark.parametrize("dirname", ["smooth", "noise"])
@pytest.mark.parametrize("name", fb.QUALIFIED + [fb.AMBIGUOUS])
def test_adjoint_reference_outside_the_interior_band_is_the_derivative_of_the_cost(name, dirname):
    """sum G h and sum h Hh against central differences of the oracle's cost (fb's targets and weights)."""
    b = fb.build(name)
    h, O = b["dirs"][dirname], b["O"]
    G, Hh = adjoint_reference(b["P"], b["phi"], b["t"], b["shifts"], b["u"], b["phi_Q"], b["phi_T"], b["x"], b["y"],
                              O.b1, O.b2, O.b3, h=h, masks=b["masks"])
    EPS = fb.EPS
    (_, c0), ((_, cp), (_, cm)) = b["base"], fb.central(b, dirname)
    es = abs((cp - cm) / (2 * EPS) / float(np.sum(G * h)) - 1.0)
    ec = abs((cp - 2 * c0 + cm) / EPS ** 2 / float(np.sum(h * Hh)) - 1.0)
    print(f"{name} {dirname}: slope {es:.2e} curvature {ec:.2e}")
    assert es < 1e-5
    assert ec < 1e-5
