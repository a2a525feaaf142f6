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
import _fix_band as fb
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


# ------------------------------------------------------------------------------------------------------------------------
# States OUTSIDE the interior band of the mass fix (tests/_fix_band.py): plateaus in [0.985, 0.99), fronts inside the band.
# The fix shifts the interior nodes only, so phi* = phi_{n+1} + s_n there and phi_{n+1} elsewhere, and the linearised fix
# subtracts its mean on the march's own set.
#
# Measured against central differences at EPS = 1e-2 (relative max-norm: dphi, d2phi, curvature, slope; smooth / noise):
#     32x16    2.7e-7 1.5e-5 1.0e-7 9.5e-8  /  1.2e-7 4.0e-5 2.9e-7 1.1e-8
#     128x32   1.3e-9 1.3e-5 2.1e-8 4.5e-11 /  7.9e-10 9.6e-5 1.8e-7 1.5e-10
#     50x36    3.6e-8 3.4e-5 4.2e-8 5.6e-8  /  6.8e-8 4.0e-5 9.6e-8 1.8e-9
#     12x9     3.7e-8 1.9e-5 2.7e-7 2.1e-9  /  1.3e-7 9.5e-5 1.8e-6 7.3e-8
#     ambiguous, with the march's own sets   2.2e-7 1.6e-5 7.6e-9 1.1e-8  /  2.4e-7 7.3e-5 8.7e-8 4.4e-8
# under the file's own bounds 1e-5, 3e-4, 1e-5, 1e-5 (d2phi needs no higher floor here).  The scheme as it was
# (phi* = phi_{n+1} + s_n at every node, sets re-derived from it) misses dphi by 5.2e-3 / 6.1e-3 on 12x9 and by
# 4.5e-3 / 7.2e-3 on the ambiguous input; with phi* corrected and the sets still re-derived the ambiguous input misses by
# 3.0e-3 / 5.8e-3.
# ------------------------------------------------------------------------------------------------------------------------


def _band_errors(m, h, **kw):
    d1, d2 = tangent_reference(m["P"], m["phi"], m["t"], h, m["shifts"], **kw)
    O = m["O"]
    S = tangent_scalars(m["phi"], d1, d2, m["u"], h, m["phi_Q"], m["phi_T"], m["x"], m["y"], m["t"], O.b1, O.b2, O.b3)
    assert EPS == fb.EPS
    (p0, c0), ((pp, cp), (pm, cm)) = m["base"], fb.central(m, next(k for k, v in m["dirs"].items() if v is h))
    return (np.abs((pp - pm) / (2 * EPS) - d1).max() / np.abs(d1).max(),
            np.abs((pp - 2 * p0 + pm) / EPS ** 2 - d2).max() / np.abs(d2).max(),
            abs((cp - 2 * c0 + cm) / EPS ** 2 / S["curvature"] - 1.0),
            abs((cp - cm) / (2 * EPS) / S["slope"] - 1.0))


@pytest.mark.parametrize("name", fb.QUALIFIED)
def test_band_inputs_meet_their_premises(name):
    """Every premise of tests/_fix_band.py, measured on the oracle's march; the sets are the same at u +- EPS h, so the
    central differences below differentiate one smooth branch of the march."""
    m = fb.build(name)
    q = fb.qualify(m)
    print(name, q, "shifts", m["shifts"])
    assert q["converged"] and q["interior_form"]
    assert q["max_phi_c"] < 1.0 - o.DELTA_SEP - fb.CLIP_MARGIN
    assert q["frac_in"] >= 0.1 and q["frac_out"] >= 0.1
    assert q["min_shift"] > 1e-6
    assert not any(q["ambiguous"]) and not any(q["near"]) and all(q["rederived_ok"])
    assert fb.is_qualified(q)
    for h in m["dirs"].values():
        for sg in (1.0, -1.0):
            masks = fb.march_with_fix(m["P"], control=m["u"] + sg * EPS * h, phi0=m["phi0"])[4]["masks"]
            assert np.array_equal(masks, m["masks"])


def test_band_diagonals_exceed_the_right_scaling_threshold():
    """The engine's CG-form solves run right-scaled where Dmax > 4 Dmin (cg_scale_ratio).  On the FFT band inputs the Newton
    diagonal tau / dt + 2 c1 / (1 - phi*^2) spans 6.2 (128x32) and 7.5 (32x16): 5 + 30 on the plateaus against 5 + 0.8 on the
    fronts; no state of init_phi_random(amp=0.1) comes near (1.01)."""
    for name in ("32x16", "128x32"):
        r = fb.diag_ratio(fb.build(name))
        print(f"{name}: Dmax / Dmin {r:.2f}")
        assert r > 4.0
    P = fb.params("32x16")
    flat = o.jac_diag(o.init_phi_random(P.Nx, P.Ny, o.DELTA_SEP, amp=0.1, seed=43), fb.DT, P)
    assert flat.max() / flat.min() < 1.1


def test_the_ambiguous_input_is_ambiguous():
    """The issue's own recipe: converged, clip inactive, the fix at work -- and skipped nodes that the re-derivation
    |phi_{n+1} + s_n| < THR takes for interior ones (it can only ADD nodes: it is a superset of the march's set)."""
    m = fb.build(fb.AMBIGUOUS)
    q = fb.qualify(m)
    print(q)
    assert q["converged"] and q["interior_form"] and q["max_phi_c"] < 1.0 - o.DELTA_SEP - fb.CLIP_MARGIN
    assert q["frac_in"] >= 0.1 and q["frac_out"] >= 0.1 and q["min_shift"] > 1e-6
    assert not all(q["rederived_ok"]) and not fb.is_qualified(q)
    for k, s in enumerate(m["shifts"]):
        red = np.abs(m["phi"][k + 1] + s) < fb.THR
        assert not np.any(m["masks"][k] & ~red)


@pytest.mark.parametrize("dirname", ["smooth", "noise"])
@pytest.mark.parametrize("name", fb.QUALIFIED + [fb.AMBIGUOUS])
def test_tangent_reference_outside_the_interior_band(name, dirname):
    m = fb.build(name)
    h = m["dirs"][dirname]
    e1, e2, ec, es = _band_errors(m, h, masks=m["masks"])
    print(f"{name} {dirname}: dphi {e1:.2e} d2phi {e2:.2e} curvature {ec:.2e} slope {es:.2e}")
    assert e1 < 1e-5
    assert e2 < 3e-4
    assert ec < 1e-5
    assert es < 1e-5
    if name != fb.AMBIGUOUS:        # qualified: what the history and the shifts alone tell is the march's own set
        a1, a2 = tangent_reference(m["P"], m["phi"], m["t"], h, m["shifts"])
        b1, b2 = tangent_reference(m["P"], m["phi"], m["t"], h, m["shifts"], masks=m["masks"])
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2)


@pytest.mark.parametrize("dirname", ["smooth", "noise"])
def test_phi_star_shifted_on_every_node_is_not_the_derivative(dirname):
    """phi* = phi_{n+1} + s_n at every node -- the scheme as it was -- with the march's own sets misses dphi by more than
    1e-3 on the ambiguous input and on 12x9, where D = 2 c1 / (1 - phi^2) is at its steepest on the skipped plateaus."""
    for name in (fb.AMBIGUOUS, "12x9"):
        m = fb.build(name)
        e1 = _band_errors(m, m["dirs"][dirname], masks=m["masks"], pstar_all=True)[0]
        g1 = _band_errors(m, m["dirs"][dirname], masks=m["masks"])[0]
        print(f"{name} {dirname}: dphi with phi* shifted everywhere {e1:.2e}, corrected {g1:.2e}")
        assert e1 > 1e-3
        assert g1 < 1e-5


@pytest.mark.parametrize("dirname", ["smooth", "noise"])
def test_sets_rederived_from_the_history_are_not_the_marchs_on_the_ambiguous_input(dirname):
    """phi* corrected, but the sets re-derived as |phi_{n+1} + s_n| < THR: misses dphi by more than 1e-3."""
    m = fb.build(fb.AMBIGUOUS)
    e1 = _band_errors(m, m["dirs"][dirname])[0]
    g1 = _band_errors(m, m["dirs"][dirname], masks=m["masks"])[0]
    print(f"{dirname}: dphi with re-derived sets {e1:.2e}, with the march's {g1:.2e}")
    assert e1 > 1e-3
    assert g1 < 1e-5


@pytest.mark.parametrize("dirname", ["smooth", "noise"])
def test_tangent_reference_in_the_all_node_form_of_the_fix(dirname):
    """fb.FALLBACK: no node inside the band at any step, the clip inactive before and after the shift, and the march takes
    err / (Lx Ly) ~ 1e-6 off every node.  phi* = phi_{n+1} + s_n at every node and the plain weighted mean is removed.
    Measured: dphi 3.1e-6 / 3.2e-6, d2phi 1.6e-4 / 1.4e-4, curvature 2.3e-7 / 4.6e-7, slope 1.3e-7 / 9.0e-10."""
    m = fb.build(fb.FALLBACK)
    fix = m["fix"]
    hi = 1.0 - o.DELTA_SEP - fb.CLIP_MARGIN
    assert not fix["interior"].any() and fix["masks"].all()
    assert np.all(fix["newton_its"] < o.NEWTON_MAXIT)
    assert fb.THR + 1e-4 < np.abs(fix["phi_c"]).min() and np.abs(fix["phi_c"]).max() < hi
    assert fb.THR + 1e-4 < np.abs(m["phi"][1:]).min() and np.abs(m["phi"][1:]).max() < hi
    assert np.abs(m["shifts"]).min() > 1e-6
    assert np.allclose(fix["w_int"], m["P"].Lx * m["P"].Ly, rtol=0, atol=0)
    h = m["dirs"][dirname]
    e1, e2, ec, es = _band_errors(m, h, masks=m["masks"])
    print(f"fallback {dirname}: dphi {e1:.2e} d2phi {e2:.2e} curvature {ec:.2e} slope {es:.2e}")
    assert e1 < 1e-5
    assert e2 < 3e-4
    assert ec < 1e-5
    assert es < 1e-5
    # what the history and the shifts alone tell (no node passes |phi_{n+1} + s_n| < THR: every node) is the same scheme
    a1, a2 = tangent_reference(m["P"], m["phi"], m["t"], h, m["shifts"])
    b1, b2 = tangent_reference(m["P"], m["phi"], m["t"], h, m["shifts"], masks=m["masks"])
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
