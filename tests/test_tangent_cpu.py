"""Pins the CPU tangent reference (tests/_tangent_ref.py) against central differences of the oracle's nonlinear march and
cost: the linearised scheme of the exact second-order check IS the derivative of the discrete march.

Setup: 16 x 16, T = 0.2, dt = 0.02 (10 steps), default parameters, control 20 cos(pi x (1 + k % 3)) cos(pi y) sin(1 + k) per
row k, a smooth direction and a white-noise one of unit max-norm, central differences at eps = 1e-2 with kappa_sparsity = 0
(the L1 term has no curvature away from its kink and is not part of the check).

Measured (max-norm, relative): dphi 1.2e-6 / 1.2e-6, d2phi 1.3e-5 / 2.6e-5, curvature 3.8e-7 / 6.9e-7 (smooth / noise).
Bounds: 1e-5, 3e-4, 1e-5 -- the measured values times ~10 for the slack of the Newton stop rule ||R|| < 1e-6, which is what
limits a difference quotient of the march.  The slope J'(u)h is linear in dphi, so it gets dphi's bound against the central
difference of the cost (measured 2.5e-7 / 1.4e-6, the latter being the eps^2 J'''/6 truncation of the difference quotient:
the same J''' explains the 1.2e-3 by which the one-sided formula misses the curvature at this eps).
max|phi| = 0.56 on this march, so the end-of-step clip, which the tangent scheme takes as the identity, is inactive.

Off the square grid the march's interior mass fix is not the identity (tests/_tangent_ref.py): the reference linearises it
with the shifts the oracle's march records.  PINS holds the points where the scheme without that term misses the central
difference by up to 2e-2: two rectangular grids at the defaults, two rectangular off-default points and a square
off-default one (control and directions in the unit-square coordinates x / Lx, y / Ly), under the same three bounds."""
import numpy as np
import pytest

from oracle import vch2d_oracle as o
from _tangent_ref import march_with_shifts, tangent_reference, tangent_scalars

N, T, DT, EPS = 16, 0.2, 0.02, 1e-2

OFF_A = dict(c2=0.5, gamma=3.0, kappa=1e-3, c1=0.9, tau=0.01)
OFF_B = dict(c2=1.5, gamma=3.0, kappa=1e-3, c1=0.9, tau=0.2)
PINS = {
    #              Params2D fields                                            control amplitude
    "14x11":      (dict(Nx=14, Ny=11, T=0.2), 20.0),
    "32x16":      (dict(Nx=32, Ny=16, T=0.1), 20.0),
    "14x11_offA": (dict(Nx=14, Ny=11, T=0.2, Lx=1.3, Ly=0.9, **OFF_A), 20.0),
    "14x11_offB": (dict(Nx=14, Ny=11, T=0.1, Lx=1.3, Ly=0.9, **OFF_B), 10.0),
    "16x16_offA": (dict(Nx=16, Ny=16, T=0.2, **OFF_A), 20.0),
}


def _build(P, amp):
    xx, yy = np.meshgrid(np.linspace(0.0, 1.0, P.Nx + 1), np.linspace(0.0, 1.0, P.Ny + 1), indexing="ij")
    M = len(o.time_grid(P.T, P.dt_initial)[1])
    u = amp * np.stack([np.cos(np.pi * xx * (1 + k % 3)) * np.cos(np.pi * yy) * np.sin(1 + k) for k in range(M + 1)])
    phi, (x, y), t, shifts = march_with_shifts(P, control=u)
    phi_T, phi_Q = o.build_targets(x, y, t, phi[0], P.Lx, P.Ly, P.T)
    O0 = o.OptParams(kappa_sparsity=0.0)

    def run(uu):
        ph = o.forward(P, control=uu)[0]
        return ph, o.cost(ph, uu, phi_Q, phi_T, x, y, t, O0)

    noise = np.random.default_rng(1).standard_normal(u.shape)
    dirs = dict(smooth=np.stack([np.cos(2 * np.pi * xx) * np.cos(np.pi * yy) * np.cos(0.3 * k) for k in range(M + 1)]),
                noise=noise / np.abs(noise).max())
    return dict(P=P, u=u, phi=phi, x=x, y=y, t=t, phi_T=phi_T, phi_Q=phi_Q, O=O0, run=run, base=run(u), dirs=dirs,
                shifts=shifts)


@pytest.fixture(scope="module")
def march():
    return _build(o.Params2D(Nx=N, Ny=N, T=T, dt_initial=DT), 20.0)


@pytest.fixture(scope="module")
def pins():
    cache = {}

    def get(name):
        if name not in cache:
            kw, amp = PINS[name]
            cache[name] = _build(o.Params2D(dt_initial=DT, **kw), amp)
        return cache[name]

    return get


def _errors(m, h, shifts):
    """Relative max-norm errors of the reference against central differences: dphi, d2phi, curvature, slope."""
    d1, d2 = tangent_reference(m["P"], m["phi"], m["t"], h, shifts)
    O = m["O"]
    S = tangent_scalars(m["phi"], d1, d2, m["u"], h, m["phi_Q"], m["phi_T"], m["x"], m["y"], m["t"], O.b1, O.b2, O.b3)
    (p0, c0), (pp, cp), (pm, cm) = m["base"], m["run"](m["u"] + EPS * h), m["run"](m["u"] - EPS * h)
    return (np.abs((pp - pm) / (2 * EPS) - d1).max() / np.abs(d1).max(),
            np.abs((pp - 2 * p0 + pm) / EPS ** 2 - d2).max() / np.abs(d2).max(),
            abs((cp - 2 * c0 + cm) / EPS ** 2 / S["curvature"] - 1.0),
            abs((cp - cm) / (2 * EPS) / S["slope"] - 1.0))


def test_clip_is_inactive(march):
    assert np.abs(march["phi"]).max() < 0.6 < 1.0 - o.DELTA_SEP


@pytest.mark.parametrize("name", ["smooth", "noise"])
def test_tangent_reference_is_the_derivative_of_the_march(march, name):
    m, h = march, march["dirs"][name]
    assert abs(np.abs(h).max() - 1.0) < 1e-12
    assert not m["shifts"].any()                 # square grid, defaults: the drift stays under the fix's 1e-16 threshold
    d1, d2 = tangent_reference(m["P"], m["phi"], m["t"], h)
    O = m["O"]
    S = tangent_scalars(m["phi"], d1, d2, m["u"], h, m["phi_Q"], m["phi_T"], m["x"], m["y"], m["t"], O.b1, O.b2, O.b3)
    (p0, c0), (pp, cp), (pm, cm) = m["base"], m["run"](m["u"] + EPS * h), m["run"](m["u"] - EPS * h)
    e1 = np.abs((pp - pm) / (2 * EPS) - d1).max() / np.abs(d1).max()
    e2 = np.abs((pp - 2 * p0 + pm) / EPS ** 2 - d2).max() / np.abs(d2).max()
    ec = abs((cp - 2 * c0 + cm) / EPS ** 2 / S["curvature"] - 1.0)
    es = abs((cp - cm) / (2 * EPS) / S["slope"] - 1.0)
    one_sided = (cp - c0 - EPS * S["slope"]) / (0.5 * EPS ** 2)
    print(f"{name}: dphi {e1:.2e} d2phi {e2:.2e} curvature {ec:.2e} slope {es:.2e}; curvature {S['curvature']:.8e}, "
          f"one-sided formula with the exact slope {one_sided:.8e}")
    assert e1 < 1e-5
    assert e2 < 3e-4
    assert ec < 1e-5
    assert es < 1e-5


@pytest.mark.parametrize("name", ["smooth", "noise"])
@pytest.mark.parametrize("pin", list(PINS))
def test_tangent_reference_off_the_square_default_grid(pins, pin, name):
    m, h = pins(pin), pins(pin)["dirs"][name]
    s = np.abs(m["shifts"]).max()
    # every node interior for the fix, before and after it, and the clip inactive
    assert np.abs(m["phi"]).max() < 0.985 - s
    if m["P"].Nx != m["P"].Ny:
        assert np.abs(m["shifts"]).min() > 1e-6       # the fix is at work on every step
    e1, e2, ec, es = _errors(m, h, m["shifts"])
    print(f"{pin} {name}: dphi {e1:.2e} d2phi {e2:.2e} curvature {ec:.2e} slope {es:.2e}; max|phi| "
          f"{np.abs(m['phi']).max():.3f}, shifts {np.abs(m['shifts']).min():.2e} .. {s:.2e}")
    assert e1 < 1e-5
    assert e2 < 3e-4
    assert ec < 1e-5
    assert es < 1e-5


def test_without_the_shifts_the_scheme_is_not_the_derivative_on_a_rectangle(pins):
    """The mass fix taken as the identity (shifts zeroed: what the scheme was) misses the central difference on 14 x 11 by
    more than 1e-3 in dphi and d2phi, a hundred times the bound the corrected scheme keeps."""
    m = pins("14x11")
    for name in ("smooth", "noise"):
        e1, e2, _, _ = _errors(m, m["dirs"][name], np.zeros_like(m["shifts"]))
        g1, g2, _, _ = _errors(m, m["dirs"][name], m["shifts"])
        print(f"14x11 {name}: shifts zeroed dphi {e1:.2e} d2phi {e2:.2e}; with the shifts {g1:.2e} {g2:.2e}")
        assert e1 > 1e-3 and e2 > 1e-3
        assert g1 < 1e-5 and g2 < 3e-4


def test_direction_row_rule_and_linearity(march):
    """Rows beyond the direction's last are zeros (and the last row alone drives no step, F2:545-548); dphi is linear and
    d2phi quadratic in h."""
    m, h = march, march["dirs"]["smooth"]
    P, phi, t = m["P"], m["phi"], m["t"]
    d1, d2 = tangent_reference(P, phi, t, h)
    a1, a2 = tangent_reference(P, phi, t, -2.0 * h)
    assert np.abs(a1 + 2.0 * d1).max() <= 1e-12 * np.abs(d1).max()
    assert np.abs(a2 - 4.0 * d2).max() <= 1e-12 * np.abs(d2).max()
    # four rows drive steps 0..2 only; padded with zero rows, step 3 is driven by (h[3], 0) as well
    s1, _ = tangent_reference(P, phi, t, h[:4])
    c1, _ = tangent_reference(P, phi, t, np.concatenate([h[:4], np.zeros_like(h[4:])]))
    assert np.array_equal(s1[:4], c1[:4])
    assert np.abs(s1[4] - c1[4]).max() > 1e-3 * np.abs(s1[4]).max()
    z1, z2 = tangent_reference(P, phi, t, np.zeros_like(h))
    assert not z1.any() and not z2.any()
