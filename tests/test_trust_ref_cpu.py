"""tests/_trust_ref.py, the NumPy restatement of vch1d_hess_cg_tr and of the rounds of vch1d_pgd_trust, on
small dense matrices: without a boundary it is _cg_ref.cg exactly, a boundary exit lies on the boundary, a negative-definite
block gives the step tau D^-1 b, the model's decrease is at least the Cauchy point's, and the rounds never raise the cost of
an indefinite boxed quadratic.

BOUNDARY_DEV is the restatement's own deviation of ||x||_D, computed directly from x, from the radius on its boundary exits
(the recurrence says ||x||_D = radius to rounding): the figure DESIGN.md 10k records, and ten times it is the bound of
test_gpu_trust_1d.py for the engine on blocks of this kind."""
import math

import numpy as np
import pytest

import _newton_ref as N
from _cg_ref import CONVERGED, LIMIT, NEGCURV, cg
from _trust_ref import ACCEPTED, BOUNDARY, IDLE, REJECTED, STALLED, STATIONARY, judge, steihaug, tau_of, trust_rounds

EPS = np.finfo(np.float64).eps
BOUNDARY_DEV = 2 * EPS          # measured below: at most 0.99 eps over the cases of test_boundary_exits_lie_on_the_boundary


def _spd(n, seed, cond=50.0):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * np.geomspace(1.0, cond, n)) @ Q.T


def _indefinite(n, seed, neg=3):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.geomspace(0.5, 20.0, n)
    ev[:neg] = -np.linspace(1.0, 3.0, neg)
    return (Q * ev) @ Q.T


def _case(n, seed):
    rng = np.random.default_rng(seed + 100)
    mask = rng.random(n) > 0.2
    return mask, rng.standard_normal(n), rng.uniform(0.5, 2.0, n)


@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("k, cg_tol", [(40, 1e-10), (5, 1e-10), (40, 1e-3)])
def test_an_infinite_radius_is_the_plain_iteration_exactly(precond, k, cg_tol):
    A = _spd(24, 1)
    mask, b, D = _case(24, 1)
    D = D if precond else None
    want = cg(lambda v: A @ v, mask, b, k, cg_tol, D)
    got = steihaug(lambda v: A @ v, mask, b, k, math.inf, cg_tol, D)
    assert want["status"] in (CONVERGED, LIMIT)
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    Dv = np.ones(24) if D is None else D
    direct = math.sqrt(float(np.sum(Dv * got["x"] ** 2)))
    # The recurrence rests on x'.r' = 0, which rounding loses as the run goes on, as any CG loses orthogonality (measured on
    # this matrix with D: 2e-16 relative up to 8 steps, 6e-9 after the 18 steps to 1e-3).  Asserted on the short run only.
    if k == 5:
        assert abs(got["xnorm"] - direct) <= 16 * EPS * direct


def test_an_infinite_radius_stops_on_negative_curvature_as_the_plain_iteration():
    A = _indefinite(24, 2)
    mask, b, _ = _case(24, 2)
    want = cg(lambda v: A @ v, mask, b, 40)
    got = steihaug(lambda v: A @ v, mask, b, 40, math.inf)
    assert want["status"] == NEGCURV == got["status"]
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key


@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("matrix", ["spd", "indefinite"])
@pytest.mark.parametrize("frac", [0.05, 0.3, 0.7, 0.95])
def test_boundary_exits_lie_on_the_boundary(precond, matrix, frac):
    A = _spd(24, 3) if matrix == "spd" else _indefinite(24, 3)
    mask, b, D = _case(24, 3)
    Dv = D if precond else np.ones(24)
    if matrix == "spd":
        full = cg(lambda v: A @ v, mask, b, 200, 1e-12, D if precond else None)
        radius = frac * math.sqrt(float(np.sum(Dv * full["x"] ** 2)))
    else:
        radius = 10.0 * frac
    S = steihaug(lambda v: A @ v, mask, b, 200, radius, 1e-12, D if precond else None)
    assert S["status"] in (BOUNDARY, NEGCURV) and S["steps"] >= 1
    assert S["status"] == BOUNDARY or matrix == "indefinite"
    direct = math.sqrt(float(np.sum(Dv * S["x"] ** 2)))
    dev = max(abs(direct - radius), abs(S["xnorm"] - radius)) / radius
    print(f"MEASURE boundary {matrix} precond {precond} frac {frac}: steps {S['steps']} status {S['status']} dev {dev / EPS:.2f} eps")
    assert dev <= BOUNDARY_DEV
    assert not S["x"][~mask].any()
    # r = P b - P A P x, and pred = b.x - x.Ax / 2
    r = np.where(mask, b - A @ S["x"], 0.0)
    assert np.abs(S["r"] - r).max() <= 1e-13 * np.abs(b).max() * np.linalg.cond(A)
    model = float(b @ S["x"] - 0.5 * S["x"] @ (A @ S["x"]))
    assert abs(S["pred"] - model) <= 1e-13 * abs(model) * np.linalg.cond(A)
    assert np.isnan(S["resid"][S["steps"]:]).all() and np.isfinite(S["resid"][:S["steps"]]).all()


@pytest.mark.parametrize("precond", [False, True])
def test_negative_definite_block_steps_along_the_preconditioned_gradient(precond):
    A = -_spd(16, 4)
    mask, b, D = _case(16, 4)
    Dv = D if precond else np.ones(16)
    radius = 0.75
    S = steihaug(lambda v: A @ v, mask, b, 10, radius, 0.0, D if precond else None)
    g = np.where(mask, b, 0.0) / Dv
    tau = radius / math.sqrt(float(np.sum(Dv * g * g)))
    assert S["status"] == NEGCURV and S["steps"] == 1 and S["curv"][0] < 0
    assert np.abs(S["x"] - tau * g).max() <= 4 * EPS * np.abs(tau * g).max()
    assert abs(S["xnorm"] - radius) <= 4 * EPS * radius
    assert S["pred"] > 0                                  # tau rho - tau^2 c / 2 with c < 0


@pytest.mark.parametrize("precond", [False, True])
def test_a_radius_whose_square_is_not_finite_has_no_boundary(precond):
    """d2 = radius * radius: 2^600 squares to +inf, tau is not finite and the call is the radius = inf call (NEGCURV at once,
    x = 0); 2^500 squares to 2^1000 and the direction of negative curvature is followed to the boundary."""
    A = -_spd(16, 4)
    mask, b, D = _case(16, 4)
    D = D if precond else None
    inf = steihaug(lambda v: A @ v, mask, b, 10, math.inf, 0.0, D)
    big = steihaug(lambda v: A @ v, mask, b, 10, 2.0 ** 600, 0.0, D)
    assert inf["status"] == NEGCURV and inf["steps"] == 0 and not inf["x"].any() and inf["pred"] == 0.0 and inf["xnorm"] == 0.0
    assert set(big) == set(inf)
    for key in inf:
        assert np.array_equal(big[key], inf[key], equal_nan=True), key
    mid = steihaug(lambda v: A @ v, mask, b, 10, 2.0 ** 500, 0.0, D)
    Dv = np.ones(16) if D is None else D
    direct = math.sqrt(float(np.sum(Dv * mid["x"] ** 2)))
    assert mid["status"] == NEGCURV and mid["steps"] == 1 and np.isfinite(mid["x"]).all() and np.isfinite(mid["pred"]) and mid["pred"] > 0
    assert abs(mid["xnorm"] - 2.0 ** 500) <= 4 * EPS * 2.0 ** 500 and abs(direct - 2.0 ** 500) <= 4 * EPS * 2.0 ** 500


@pytest.mark.parametrize("precond", [False, True])
def test_a_radius_whose_square_underflows_gives_a_zero_step(precond):
    """d2 = 0 for radius 2^-600: the first step already leaves the region, tau = 0, and the exit is BOUNDARY after one step
    that moves nothing."""
    A = _spd(24, 3)
    mask, b, D = _case(24, 3)
    S = steihaug(lambda v: A @ v, mask, b, 10, 2.0 ** -600, 0.0, D if precond else None)
    assert S["status"] == BOUNDARY and S["steps"] == 1
    assert not S["x"].any() and S["pred"] == 0.0 and S["xnorm"] == 0.0 and S["resid"][0] == 1.0
    assert np.array_equal(S["r"], np.where(mask, b, 0.0))
    assert all(np.isfinite(S[key]).all() for key in ("x", "r", "p", "pred", "rnorm0", "xnorm")) and np.isfinite(S["curv"][0])
    assert np.isnan(S["resid"][1:]).all()


@pytest.mark.parametrize("matrix", ["spd", "indefinite"])
@pytest.mark.parametrize("radius", [0.01, 0.5, 3.0, 1e3])
def test_the_decrease_is_at_least_the_cauchy_point_s(matrix, radius):
    A = _spd(24, 5) if matrix == "spd" else _indefinite(24, 5)
    mask, b, D = _case(24, 5)
    S = steihaug(lambda v: A @ v, mask, b, 100, radius, 1e-12, D)
    g = np.where(mask, b, 0.0)
    z = g / D
    gBg, gz = float(z @ (A @ z)), float(g @ z)
    t = radius / math.sqrt(float(np.sum(D * z * z)))
    if gBg > 0:
        t = min(t, gz / gBg)
    cauchy = t * gz - 0.5 * t * t * gBg
    assert cauchy > 0 and S["pred"] >= cauchy * (1 - 1e-12)


def test_tau_is_the_root_for_either_sign_of_xp():
    for xx, xp, pp, d2 in [(0.0, 0.0, 2.0, 9.0), (1.0, 0.7, 2.0, 9.0), (1.0, -0.7, 2.0, 9.0), (8.999, 3.0, 0.5, 9.0)]:
        t = tau_of(xx, xp, pp, d2)
        assert t >= 0 and abs(xx + 2 * t * xp + t * t * pp - d2) <= 8 * EPS * d2
    assert not math.isfinite(tau_of(1.0, 0.5, 2.0, math.inf)) and not math.isfinite(tau_of(1.0, -0.5, 2.0, math.inf))


def test_judge_on_its_edges():
    edge = 2.0 - 1e-4 * 0.5
    assert judge(2.0, 0.5, edge, 1.0, CONVERGED, 1.0, 8.0, 1e-3)[0] == ACCEPTED
    st, ratio, rad, ended = judge(2.0, 0.5, math.nextafter(edge, math.inf), 1.0, CONVERGED, 1.0, 8.0, 1e-3)
    assert (st, rad, ended) == (REJECTED, 0.25, False) and ratio < 0.25
    assert judge(2.0, 0.5, 1.5, 1.0, BOUNDARY, 1.0, 8.0, 1e-3)[2] == 2.0            # rho = 1 on the boundary: doubled
    assert judge(2.0, 0.5, 1.5, 1.0, NEGCURV, 6.0, 8.0, 1e-3)[2] == 8.0             # clamped at radius_max
    assert judge(2.0, 0.5, 1.5, 0.5, CONVERGED, 1.0, 8.0, 1e-3)[2] == 1.0           # an interior step: kept
    assert judge(2.0, 0.5, 1.75, 0.5, BOUNDARY, 1.0, 8.0, 1e-3)[2] == 1.0           # rho = 1/2: kept
    assert judge(2.0, 0.5, 2.5, 0.002, BOUNDARY, 1.0, 8.0, 1e-3) == (STALLED, -1.0, 0.0005, True)
    assert judge(2.0, 0.5, math.nan, 1.0, BOUNDARY, 1.0, 8.0, 1e-3)[0] == REJECTED


@pytest.mark.parametrize("seed", [6, 7, 8])
@pytest.mark.parametrize("radius0", [0.05, 1.0, 50.0])
def test_the_rounds_never_raise_the_cost_of_an_indefinite_boxed_quadratic(seed, radius0):
    n = 20
    A = _indefinite(n, seed, neg=4)
    rng = np.random.default_rng(seed)
    c, w = rng.standard_normal(n), rng.uniform(0.5, 1.5, n)
    u0 = rng.uniform(-0.5, 0.5, n)
    lo, hi, kappa = -1.0, 1.0, 0.05
    u, recs = trust_rounds(A, c, kappa, w, u0, lo, hi, 25, radius0)
    live = [r for r in recs if r["status"] != IDLE]
    assert live and (u >= lo).all() and (u <= hi).all()
    for r in live:
        assert r["cost_new"] <= r["cost"]
        assert r["status"] == ACCEPTED or r["cost_new"] == r["cost"]
    for a, b in zip(live, live[1:]):
        assert b["cost"] == a["cost_new"]
    assert any(r["status"] == ACCEPTED for r in live)
    assert N.cost(A, c, kappa, w, u) == live[-1]["cost_new"] < N.cost(A, c, kappa, w, u0)
    assert live[-1]["status"] in (ACCEPTED, REJECTED, STALLED, STATIONARY)
