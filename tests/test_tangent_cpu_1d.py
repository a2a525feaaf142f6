"""Pins the 1D CPU tangent reference (tests/_tangent_ref_1d.py) against central differences of the oracle's nonlinear march
and cost: the linearised scheme of vch1d_second_order IS the derivative of the discrete 1D march.

Setups (control amp cos(pi x / Lx (1 + k % 3)) sin(1 + k) per row k; a smooth direction cos(2 pi x / Lx) cos(0.3 k) and a
white-noise one of unit max-norm; the smooth start 0.2 cos(pi x / Lx)):
    n32         N = 32, defaults, T = 0.2, dt = 0.02, control 20
    n33_off     N = 33, Lx 1.3, c2 0.5, gamma 3, kappa 1e-3, c1 0.9, tau 0.01, T = 0.1, dt = 0.02, control 10
    n64         N = 64, defaults, T = 0.2, dt = 0.02, control 50
    n32_ragged  N = 32, defaults, T = 0.09, dt = 0.02 (last step 0.01), control 20
Fields: central differences of o.forward at eps = 1e-2, relative max-norm error.  Sums: J'(u)h and J''(u)[h,h] against
central differences of sum(o.cost_parts[:3]) at eps = 3e-2, relative deviation.

Measured (worse of the two directions) / asserted (10 x measured, rounded up: the factor covers the noise of the Newton stop
rule ||R|| < 1e-6 across platforms).  No bound exceeds the floors of the 2D file, 1e-5 for dphi and the sums, 3e-4 for d2phi:
                  dphi                d2phi               J'(u)h              J''(u)[h,h]
    n32           5.22e-8 / 5.3e-7    2.50e-6 / 2.5e-5    5.14e-8 / 5.2e-7    1.01e-7 / 1.1e-6
    n33_off       5.26e-9 / 5.3e-8    1.82e-6 / 1.9e-5    7.99e-8 / 8.0e-7    3.38e-8 / 3.4e-7
    n64           3.26e-7 / 3.3e-6    6.04e-6 / 6.1e-5    9.10e-8 / 9.2e-7    3.94e-7 / 4.0e-6
    n32_ragged    9.93e-9 / 1.0e-7    5.98e-6 / 6.0e-5    7.00e-9 / 7.0e-8    1.68e-8 / 1.7e-7
What the central difference of the march differs by is the last Newton update, not round-off: the march stops at
||R|| < 1e-6 and its iterate is not the root the tangent scheme differentiates.  From the smooth start every step takes two
solves and ends at ||R|| of 1e-11 .. 1e-7 (printed per setup); a start from which the last residual is 5e-7 at every step
(0.5 cos(2 pi x) + ...) measures 3e-6 / 2e-5 / 2e-6 / 5e-5 at every eps from 3e-3 to 1e-1.

Driver level (_tangent_ref_1d.driver_problem: N = 32, 5 steps, box-clipped control, three unit-Euclidean directions of
_generate_direction with seed 7): the central second difference of the oracle's J1 + J2 + J3 at eps = 3e-2 deviates from
the exact curvature by 5.82e-7 relative (worst direction); DRIVER_TOL = 5.9e-6 = 10 x that is the bound that
test_gpu_second_order_1d.py holds the engine's forward + cost to.  It is set by the oracle here, not by the engine.

Every setup keeps max|phi| < 1 - delta_sep - 0.1, so the end-of-step clip, which the scheme takes as the identity, is
inactive."""
import numpy as np
import pytest

from oracle import vch1d_oracle as o
from _tangent_ref_1d import DRIVER, driver_problem, tangent_reference_1d, tangent_scalars_1d

EPS_F, EPS_C = 1e-2, 3e-2
FLOOR_D1, FLOOR_D2, FLOOR_S = 1e-5, 3e-4, 1e-5

OFF = dict(Lx=1.3, c2=0.5, gamma=3.0, kappa=1e-3, c1=0.9, tau=0.01)
SETUPS = {
    #             Params1D fields                           control    bounds: dphi, d2phi, slope, curvature
    "n32":        (dict(N=32, T=0.2, dt_initial=0.02), 20.0, (5.3e-7, 2.5e-5, 5.2e-7, 1.1e-6)),
    "n33_off":    (dict(N=33, T=0.1, dt_initial=0.02, **OFF), 10.0, (5.3e-8, 1.9e-5, 8.0e-7, 3.4e-7)),
    "n64":        (dict(N=64, T=0.2, dt_initial=0.02), 50.0, (3.3e-6, 6.1e-5, 9.2e-7, 4.0e-6)),
    "n32_ragged": (dict(N=32, T=0.09, dt_initial=0.02), 20.0, (1.0e-7, 6.0e-5, 7.0e-8, 1.7e-7)),
}
DRIVER_TOL = 5.9e-6


def _build(kw, amp):
    P = o.Params1D(**kw)
    xs = np.linspace(0.0, 1.0, P.N + 1)
    phi0 = 0.2 * np.cos(np.pi * xs)
    fwd = lambda uu, **k: o.forward(P, control=uu, initial_phi=phi0, **k)
    _, x, t = fwd(None)
    rows = len(t)
    u = amp * np.stack([np.cos(np.pi * xs * (1 + k % 3)) * np.sin(1 + k) for k in range(rows)])
    st = {}
    phi = fwd(u, stats=st)[0]
    phi_T, phi_Q = o.build_targets(x, t, phi[0], P.Lx, P.T)
    O = o.OptParams1D()

    def run(uu):
        ph = fwd(uu)[0]
        return ph, float(np.sum(o.cost_parts(ph, uu, phi_Q, phi_T, x, t, O.b1, O.b2, O.b3, 0.0)[:3]))

    noise = np.random.default_rng(1).standard_normal(u.shape)
    dirs = dict(smooth=np.stack([np.cos(2 * np.pi * xs) * np.cos(0.3 * k) for k in range(rows)]),
                noise=noise / np.abs(noise).max())
    return dict(P=P, u=u, phi=phi, x=x, t=t, phi_T=phi_T, phi_Q=phi_Q, O=O, run=run, dirs=dirs, stats=st)


@pytest.fixture(scope="module")
def setups():
    cache = {}

    def get(name):
        if name not in cache:
            kw, amp, _ = SETUPS[name]
            cache[name] = _build(kw, amp)
        return cache[name]

    return get


def _errors(m, h, omit=()):
    """Relative errors of the reference against central differences: dphi, d2phi (max-norm, relative to the full
    scheme's field), slope, curvature."""
    d1, d2 = tangent_reference_1d(m["P"], m["phi"], m["t"], h, omit=omit)
    n1, n2 = (d1, d2) if not omit else tangent_reference_1d(m["P"], m["phi"], m["t"], h)
    O = m["O"]
    S = tangent_scalars_1d(m["phi"], d1, d2, m["u"], h, m["phi_Q"], m["phi_T"], m["x"], m["t"], O.b1, O.b2, O.b3)
    p0 = m["phi"]
    pp, pm = m["run"](m["u"] + EPS_F * h)[0], m["run"](m["u"] - EPS_F * h)[0]
    c0 = m["run"](m["u"])[1]
    cp, cm = m["run"](m["u"] + EPS_C * h)[1], m["run"](m["u"] - EPS_C * h)[1]
    return (np.abs((pp - pm) / (2 * EPS_F) - d1).max() / np.abs(n1).max(),
            np.abs((pp - 2 * p0 + pm) / EPS_F ** 2 - d2).max() / np.abs(n2).max(),
            abs((cp - cm) / (2 * EPS_C) / S["slope"] - 1.0),
            abs((cp - 2 * c0 + cm) / EPS_C ** 2 / S["curvature"] - 1.0))


def test_bounds_stay_under_the_floors():
    for _, _, (b1, b2, bs, bc) in SETUPS.values():
        assert b1 <= FLOOR_D1 and b2 <= FLOOR_D2 and bs <= FLOOR_S and bc <= FLOOR_S
    assert DRIVER_TOL <= FLOOR_S


@pytest.mark.parametrize("name", list(SETUPS))
def test_tangent_reference_is_the_derivative_of_the_march(setups, name):
    m = setups(name)
    assert np.abs(m["phi"]).max() < 1.0 - o.DELTA_SEP - 0.1          # the clip the scheme ignores is inactive
    assert np.array_equal(m["phi"][0], m["phi"][1]) and m["t"][0] == m["t"][1] == 0.0
    worst = np.zeros(4)
    for dname, h in m["dirs"].items():
        assert abs(np.abs(h).max() - 1.0) < 1e-12
        e = np.array(_errors(m, h))
        print(f"{name} {dname}: dphi {e[0]:.2e} d2phi {e[1]:.2e} slope {e[2]:.2e} curvature {e[3]:.2e}; "
              f"max|phi| {np.abs(m['phi']).max():.3f}")
        worst = np.maximum(worst, e)
    st = m["stats"]
    print(f"{name}: Newton solves per step {st['solves'] / (len(m['t']) - 2):.2f}, last residual norms "
          + " ".join(f"{v:.0e}" for v in st["last_norms"]))
    print(f"{name}: worst dphi {worst[0]:.2e} d2phi {worst[1]:.2e} slope {worst[2]:.2e} curvature {worst[3]:.2e}")
    bounds = SETUPS[name][2]
    for e, b, what in zip(worst, bounds, ("dphi", "d2phi", "slope", "curvature")):
        assert e < b, (what, e, b)


def test_the_check_can_fail_without_the_curvature_source(setups):
    """The source -c1 rho(phi*) dphi*^2 of the second solve dropped: d2phi misses its bound (dphi does not depend on it)."""
    m = setups("n32")
    b = SETUPS["n32"][2]
    for h in m["dirs"].values():
        e1, e2, _, _ = _errors(m, h, omit=("rho",))
        print(f"n32 without rho: dphi {e1:.2e} d2phi {e2:.2e}")
        assert e1 < b[0] and e2 > b[1]


def test_the_check_can_fail_without_the_explicit_concave_term(setups):
    """The explicit +2 c2 dphi of the first right-hand side dropped: dphi misses its bound."""
    m = setups("n32")
    b = SETUPS["n32"][2]
    for h in m["dirs"].values():
        e1, _, _, _ = _errors(m, h, omit=("c2",))
        print(f"n32 without the 2 c2 dphi term: dphi {e1:.2e}")
        assert e1 > b[0]


def test_linearity_zero_direction_and_first_rows(setups):
    m = setups("n32_ragged")
    h = m["dirs"]["noise"]
    d1, d2 = tangent_reference_1d(m["P"], m["phi"], m["t"], h)
    a1, a2 = tangent_reference_1d(m["P"], m["phi"], m["t"], -2.0 * h, dts=np.diff(m["t"])[1:])
    assert np.abs(a1 + 2.0 * d1).max() <= 1e-12 * np.abs(d1).max()
    assert np.abs(a2 - 4.0 * d2).max() <= 1e-12 * np.abs(d2).max()
    assert not d1[:2].any() and not d2[:2].any() and d1[2].any()
    z1, z2 = tangent_reference_1d(m["P"], m["phi"], m["t"], np.zeros_like(h))
    assert not z1.any() and not z2.any()


def test_driver_level_discrepancy_of_the_central_second_difference():
    """What DRIVER_TOL rests on: the oracle's own central second difference of J1 + J2 + J3 against the exact curvature,
    for the directions the driver-level GPU test draws."""
    import vch_amd
    S1 = vch_amd.module("Vch_control_1D.second_order_conditions")
    D = DRIVER
    P, phi0, u_star, r_star = driver_problem()
    phi, x, t = o.forward(P, control=u_star, initial_phi=phi0)
    assert np.abs(phi).max() < 1.0 - o.DELTA_SEP - 0.1
    phi_T, phi_Q = o.build_targets(x, t, phi[0], P.Lx, P.T)
    O = o.OptParams1D()
    J = lambda uu: float(np.sum(o.cost_parts(o.forward(P, control=uu, initial_phi=phi0)[0], uu, phi_Q, phi_T, x, t, O.b1, O.b2, O.b3, 0.0)[:3]))
    rng = np.random.default_rng(D["seed"])
    worst = 0.0
    for k in range(D["num_directions"]):
        h = S1._generate_direction(u_star, r_star, D["u_min"], D["u_max"], O.kappa_sparsity, O.b3, rng)
        assert abs(np.linalg.norm(h) - 1.0) < 1e-12
        d1, d2 = tangent_reference_1d(P, phi, t, h)
        S = tangent_scalars_1d(phi, d1, d2, u_star, h, phi_Q, phi_T, x, t, O.b1, O.b2, O.b3)
        e = D["eps"]
        fd = (J(u_star + e * h) - 2.0 * J(u_star) + J(u_star - e * h)) / e ** 2
        dev = abs(fd / S["curvature"] - 1.0)
        print(f"driver direction {k}: exact {S['curvature']:.8e} central difference {fd:.8e} rel.dev {dev:.2e}")
        worst = max(worst, dev)
    print(f"driver: worst {worst:.2e}, DRIVER_TOL {DRIVER_TOL:.1e}")
    assert worst < DRIVER_TOL
