"""vch1d_hess_cg_tr / vch1d_pgd_trust on the GPU: Steihaug-Toint truncated conjugate gradients in a trust region on the free
set of the 1D engine and the trust-region rounds about the resident PGD iterate, against vch1d_hess_cg bit
for bit where no boundary is met, against the NumPy restatement tests/_trust_ref.py (pinned by test_trust_ref_cpu.py) driven
by Engine1D.hessvec, against the host loop GD_1D.trust_refine, and a batch against single-trajectory contexts.

Problems (the fixtures of test_gpu_krylov_1d.py / test_gpu_hess_cg_1d.py / test_gpu_krylov_grid_1d.py; max_steps = 8 except on
the grid):
    driver   N = 32, 5 steps: 7 rows x 33 nodes = 231 nodes, 172 free, one ragged streaming chunk
    n1030    N = 1030: two chunks, 12 free nodes (uploaded mask), cyclic-reduction depth 1
    n2051    N = 2051: three chunks, the last ragged, 12 free nodes, depth 2
    grid     the eight-chunk shape of test_gpu_krylov_grid_1d.py
    refine   the driver's grid about the default start of the 1D march with b3 = 1: the problem of test_newton_refine

Tolerances (none tuned against the code under test).
    bits          radius = +inf against hess_cg, a batch member against a context of its own, the device rounds against the
                  host loop: exact.
    restatement   steps within +-1 of _trust_ref.steihaug driven by Engine1D.hessvec; resid (absolute), curv (of the largest)
                  and pred (relative): HV_TOL[depth][1] of test_gpu_hessvec_1d.TOL times cond(block), the bound of
                  test_gpu_hess_cg_1d.py (7.0e-15 cond on the driver block).
    boundary      | ||x||_D - radius | / radius with ||x||_D computed on the host from cg_vector("x"), and xnorm against the
                  radius: 10 x the restatement's own deviation (its direct norm against the radius and against its
                  recurrence) on the same block and radius, that deviation taken as at least one eps (a deviation of 0 is one
                  the double format cannot tell from half an ulp).  DESIGN.md 10k records the restatement's figures.
    identities    r = P b - P H P x (of ||P b||) and pred = b.x - x.Hx / 2 (of sum |b||x|): HV_TOL[depth][1] cond(block), as
                  the 10h table asserts them after four steps."""
import ctypes as C

import numpy as np
import pytest

from _cg_ref import CONVERGED, LIMIT, NEGCURV, cg
from _trust_ref import BOUNDARY, steihaug
from test_gpu_hess_cg_1d import KEYS as CG_KEYS, _block, _cg, _mass, _negative_b3, _weights, refine      # noqa: F401 (fixture)
from test_gpu_hessvec_1d import TOL as HV_TOL
from test_gpu_krylov_1d import V, _mask_of, _q0, _tile, driver, small                                    # noqa: F401 (fixtures)
from test_gpu_krylov_grid_1d import grid                                                                 # noqa: F401 (fixture)
from test_gpu_newton_1d import _pgd, _refine_case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ACCEPTED, STATIONARY, NT_NEGCURV, BREAKDOWN, STALLED, IDLE, REJECTED = range(7)
TR_KEYS = CG_KEYS + ("xnorm",)
OUT_KEYS = ("cost", "cost_new", "pred", "rnorm0", "radius", "ratio", "xnorm", "cg_steps", "cg_status", "status", "n_free", "pinned",
            "clipped")


def _tr(pr, eng, k, radius, nb=0, **kw):
    args = pr.kw(nb)
    args.update(kw)
    return eng.hess_cg_trust(k, radius, pr.t, args.pop("opt", pr.opt), **args)


def _vectors(eng):
    return [eng.cg_vector(w) for w in "xrp"]


def _driven(pr, nodes, b, k, radius, cg_tol, precond, opt=None):
    """The restatement on the free nodes with Engine1D.hessvec (a context of its own) as its product."""
    eng = pr.context(1)

    def apply(v):
        h = np.zeros(pr.u.size)
        h[nodes] = v
        return eng.hessvec(h.reshape((1,) + pr.shape), pr.t, opt or pr.opt, **pr.kw())["hv"][0].ravel()[nodes]

    Df = _mass(pr).ravel()[nodes]
    out = steihaug(apply, np.ones(len(nodes), dtype=bool), b.ravel()[nodes], k, radius, cg_tol, Df if precond else None)
    eng.close()
    return out


def _dnorm(pr, X, precond):
    return float(np.sqrt(np.sum((_mass(pr) if precond else 1.0) * X * X)))


# ---------------------------------------------------------------------------------------------------------------------
# 1. radius = +inf is vch1d_hess_cg bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("name, k, cg_tol", [("driver", 400, 1e-8), ("driver", 6, 1e-30), ("n1030", 48, 1e-8), ("n2051", 48, 1e-8)])
def test_an_infinite_radius_is_hess_cg_bit_for_bit(request, small, name, k, cg_tol, precond):
    pr = request.getfixturevalue("driver") if name == "driver" else small(name)
    b = _q0(pr.shape, 41)
    eng = pr.context(1)
    want = _cg(pr, eng, k, rhs=b, cg_tol=cg_tol, precond=precond, mask=pr.mask)
    Vw = _vectors(eng)
    got = _tr(pr, eng, k, np.inf, rhs=b, cg_tol=cg_tol, precond=precond, mask=pr.mask)
    Vg = _vectors(eng)
    eng.close()
    assert want["status"][0] == (LIMIT if k == 6 else CONVERGED)
    for key in CG_KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    for w, a, c in zip("xrp", Vg, Vw):
        assert np.array_equal(a, c), w
    direct = _dnorm(pr, Vg[0][0], precond)
    print(f"MEASURE inf {name} precond {precond} k {k}: steps {got['steps'][0]} xnorm {got['xnorm'][0]:.17g} direct {direct:.17g}")
    assert np.isfinite(got["xnorm"][0]) and got["xnorm"][0] > 0
    assert got["stats"]["linear_solves"] == want["stats"]["linear_solves"]


def test_an_infinite_radius_on_the_eight_chunk_grid(grid):
    pr = grid
    b = _q0((2,) + pr.shape, 42)
    mask = (np.abs(pr.u) > 1e-8) & (np.abs(pr.u) < 1.0 - 1e-8)      # uploaded, so that the restatement below has the same nodes
    masks = _tile(mask, 2)
    eng = pr.context(2)
    want = _cg(pr, eng, 5, nb=2, rhs=b, cg_tol=1e-30, mask=masks)
    Vw = _vectors(eng)
    got = _tr(pr, eng, 5, np.inf, nb=2, rhs=b, cg_tol=1e-30, mask=masks)
    Vg = _vectors(eng)
    R = _tr(pr, eng, 5, np.array([np.inf, 0.5 * got["xnorm"][1]]), nb=2, rhs=b, cg_tol=1e-30, mask=masks)
    X = eng.cg_vector("x")
    eng.close()
    assert list(want["status"]) == [LIMIT, LIMIT] and list(want["steps"]) == [5, 5]
    for key in CG_KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    for w, a, c in zip("xrp", Vg, Vw):
        assert np.array_equal(a, c), w
    # member 1 inside half the norm it reached: on the boundary; member 0 beside it is untouched by that
    assert R["status"][1] == BOUNDARY and R["status"][0] == LIMIT and np.array_equal(X[0], Vg[0][0])
    assert R["xnorm"][0] == got["xnorm"][0]
    rad = 0.5 * got["xnorm"][1]
    nodes = np.flatnonzero(mask.ravel())
    assert len(nodes) == R["n_free"][1]
    ref = _driven(pr, nodes, b[1], 5, rad, 1e-30, True)
    Df = _mass(pr).ravel()[nodes]
    ref_direct = float(np.sqrt(np.sum(Df * ref["x"] ** 2)))
    ref_dev = max(abs(ref_direct - rad), abs(ref["xnorm"] - rad), abs(ref_direct - ref["xnorm"])) / rad
    dev = max(abs(_dnorm(pr, X[1], True) - rad), abs(R["xnorm"][1] - rad)) / rad
    print(f"MEASURE grid boundary: steps {R['steps'][1]} / {ref['steps']} dev {dev / EPS:.2f} eps, restatement {ref_dev / EPS:.2f} eps")
    assert ref["status"] == BOUNDARY and abs(int(R["steps"][1]) - ref["steps"]) <= 1
    assert dev <= 10 * max(ref_dev, EPS)


# ---------------------------------------------------------------------------------------------------------------------
# 2. boundary exits against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("name, frac", [("driver", 0), ("driver", 3), ("n1030", 2), ("n2051", 2)])
def test_boundary_exits_against_the_restatement(request, small, name, frac, precond):
    """frac: the plain iteration's steps inside the region.  The radius lies halfway between ||x_frac||_D and ||x_frac+1||_D of
    the restatement on the dense block (the norms grow with the steps), so the exit is on the boundary at step frac + 1, inside
    the four steps over which test_gpu_hess_cg_1d.py asserts the same scalars at the same bound."""
    pr = request.getfixturevalue("driver") if name == "driver" else small(name)
    depth = getattr(pr, "depth", 0)
    blk = _block(pr)
    cond = np.linalg.cond(blk)
    tol = HV_TOL[depth][1] * cond
    b = _q0(pr.shape, 43)
    bf = b.ravel()[pr.free]
    Df = _mass(pr).ravel()[pr.free] if precond else np.ones(len(pr.free))
    ones = np.ones(len(pr.free), dtype=bool)
    norms = [0.0 if j == 0 else float(np.sqrt(np.sum(Df * cg(lambda v: blk @ v, ones, bf, j, 1e-30, Df if precond else None)["x"] ** 2)))
             for j in (frac, frac + 1)]
    assert norms[1] > norms[0]
    radius = 0.5 * (norms[0] + norms[1])
    k = 4 * len(pr.free)
    eng = pr.context(1)
    R = _tr(pr, eng, k, radius, rhs=b, cg_tol=1e-8, precond=precond, mask=pr.mask)
    X, Rr, _ = (v[0] for v in _vectors(eng))
    eng.close()
    ref = _driven(pr, pr.free, b, k, radius, 1e-8, precond)
    m = int(R["steps"][0])
    print(f"MEASURE boundary {name} precond {precond} frac {frac}: steps {m} / {ref['steps']} status {R['status'][0]} / {ref['status']} "
          f"cond {cond:.3g}")
    assert R["status"][0] == BOUNDARY == ref["status"] and abs(m - ref["steps"]) <= 1 and m >= 1 and ref["steps"] == frac + 1
    assert not X[~pr.mask].any() and not Rr[~pr.mask].any() and np.isfinite(X).all()
    assert np.isnan(R["resid"][0, m:]).all() and np.isnan(R["curv"][0, m:]).all() and np.isfinite(R["resid"][0, :m]).all()
    if m == ref["steps"]:
        d_res = np.abs(R["resid"][0, :m] - ref["resid"][:m]).max()
        d_curv = np.abs(R["curv"][0, :m] - ref["curv"][:m]).max() / np.abs(ref["curv"][:m]).max()
        d_pred = abs(R["pred"][0] - ref["pred"]) / abs(ref["pred"])
        print(f"MEASURE boundary {name} precond {precond} frac {frac}: resid {d_res:.2e} curv {d_curv:.2e} pred {d_pred:.2e} (bound {tol:.2e})")
        assert d_res <= tol and d_curv <= tol and d_pred <= tol
    # the boundary norm, on the host from x, against the restatement's own deviation on this block
    xf = ref["x"]
    ref_direct = float(np.sqrt(np.sum(Df * xf * xf)))
    ref_dev = max(abs(ref_direct - radius), abs(ref["xnorm"] - radius), abs(ref_direct - ref["xnorm"])) / radius
    direct = _dnorm(pr, X, precond)
    dev = max(abs(direct - radius), abs(R["xnorm"][0] - radius)) / radius
    print(f"MEASURE boundary {name} precond {precond} frac {frac}: | ||x||_D - radius | / radius {dev / EPS:.2f} eps, restatement "
          f"{ref_dev / EPS:.2f} eps")
    assert dev <= 10 * max(ref_dev, EPS)
    # r = P b - P H P x and pred = b.x - x.Hx / 2
    hx = pr.hessvec(X[None])[0]
    true_r = np.where(pr.mask, b - hx, 0.0)
    d_r = np.abs(Rr - true_r).max() / np.linalg.norm(bf)
    model = float(np.sum(b * X) - 0.5 * np.sum(X * hx))
    d_model = abs(R["pred"][0] - model) / float(np.sum(np.abs(b * X)))
    print(f"MEASURE boundary {name} precond {precond} frac {frac}: r identity {d_r:.2e} pred identity {d_model:.2e} (bound {tol:.2e})")
    assert d_r <= tol and d_model <= tol


# ---------------------------------------------------------------------------------------------------------------------
# 3. negative curvature at step 0: the step tau D^-1 P b to the boundary
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
def test_negative_definite_steps_to_the_boundary_at_step_zero(driver, precond):
    pr, Vm = driver, driver.V
    mask = pr.mask.copy()
    mask[0] = False                                                  # row 0 is not shifted by b3: left out, the block is negative definite
    nodes = np.flatnonzero(mask.ravel())
    b3 = _negative_b3(pr)
    opt = Vm.make_opt(pr.opt, b3=b3)
    W, D = _weights(pr).ravel()[nodes], (_mass(pr).ravel()[nodes] if precond else np.ones(len(nodes)))
    blk = pr.Hm[np.ix_(nodes, nodes)] + (b3 - pr.opt.b3) * np.diag(W)
    assert np.linalg.eigvalsh(blk)[-1] < 0
    b = _q0(pr.shape, 26)
    radius = 0.75
    eng = pr.context(1)
    R = _tr(pr, eng, 5, radius, rhs=b, precond=precond, mask=mask, opt=opt)
    X, Rr, _ = (v[0] for v in _vectors(eng))
    eng.close()
    g = b.ravel()[nodes] / D
    tau = radius / np.sqrt(np.sum(D * g * g))
    ref = _driven(pr, nodes, b, 5, radius, 0.0, precond, opt=opt)
    tol = HV_TOL[0][1] * np.linalg.cond(blk)
    d_x = np.abs(X.ravel()[nodes] - tau * g).max() / np.abs(tau * g).max()
    d_curv = abs(R["curv"][0, 0] - ref["curv"][0]) / abs(ref["curv"][0])
    d_pred = abs(R["pred"][0] - ref["pred"]) / abs(ref["pred"])
    d_res = abs(R["resid"][0, 0] - ref["resid"][0])
    print(f"MEASURE negative definite precond {precond}: x {d_x / EPS:.2f} eps curv {d_curv:.2e} pred {d_pred:.2e} resid {d_res:.2e} "
          f"(bound {tol:.2e}) xnorm dev {abs(R['xnorm'][0] - radius) / radius / EPS:.2f} eps")
    assert R["status"][0] == NEGCURV == ref["status"] and R["steps"][0] == 1 == ref["steps"] and R["curv"][0, 0] < 0
    assert R["pred"][0] > 0 and not X[~mask].any()
    nsum = (len(nodes) + 8) * EPS                                    # a sum of n positive terms in any order: n eps at the worst
    assert d_x <= nsum                                               # tau: a square root and a quotient of such sums
    assert d_curv <= tol and d_pred <= tol and d_res <= tol * max(1.0, ref["resid"][0])
    assert abs(R["xnorm"][0] - radius) <= 10 * EPS * radius and abs(_dnorm(pr, X, precond) - radius) <= nsum * radius
    assert R["stats"]["linear_solves"] == pr.M * 3                   # one product taken


# ---------------------------------------------------------------------------------------------------------------------
# 4. a batch of three with its own radii against three single contexts
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_of_three_equals_three_single_contexts(driver):
    pr, Vm = driver, driver.V
    no_row0 = pr.mask.copy()
    no_row0[0] = False
    masks = np.stack([_mask_of(pr.shape, pr.free[[4, 77, 150]]), pr.mask, no_row0])
    opts = [pr.opt, pr.opt, Vm.make_opt(pr.opt, b3=_negative_b3(pr))]
    b = _q0((3,) + pr.shape, 44)
    D = _mass(pr).ravel()

    def newton_norm(mask, rhs):
        n = np.flatnonzero(mask.ravel())
        xs = np.linalg.solve(pr.Hm[np.ix_(n, n)], rhs.ravel()[n])
        return float(np.sqrt(np.sum(D[n] * xs * xs)))

    # ten times the Newton step's norm: interior; three tenths of it: on the boundary (the iterates' norms grow towards it)
    radius = np.array([10.0 * newton_norm(masks[0], b[0]), 0.3 * newton_norm(masks[1], b[1]), 0.25])
    k = 14
    eng = pr.context(3)
    many = _tr(pr, eng, k, radius, nb=3, rhs=b, precond=True, mask=masks, cg_tol=1e-8, opt=opts)
    Vmany = _vectors(eng)
    eng.close()
    print(f"MEASURE batch: n_free {list(many['n_free'])} steps {list(many['steps'])} status {list(many['status'])} xnorm {list(many['xnorm'])}")
    assert list(many["status"]) == [CONVERGED, BOUNDARY, NEGCURV] and many["steps"][0] == 3 and many["steps"][2] == 1
    assert many["xnorm"][0] < radius[0] and many["stats"]["host_syncs"] == 2
    for i in range(3):
        eng = pr.context(1)
        one = _tr(pr, eng, k, radius[i], rhs=b[i], precond=True, mask=masks[i], cg_tol=1e-8, opt=opts[i])
        for key in TR_KEYS:
            assert np.array_equal(one[key][0], many[key][i], equal_nan=True), (key, i)
        for w, vm in zip("xrp", Vmany):
            assert np.array_equal(eng.cg_vector(w)[0], vm[i]), (w, i)
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the rounds: device against the host loop, a batch against single contexts, the reason for the feature
# ---------------------------------------------------------------------------------------------------------------------
def _radius_of(pr, frac):
    return frac * _dnorm(pr, pr.u, True)


def test_device_rounds_equal_the_host_loop(refine):
    pr, Vm = refine, refine.V
    G1 = Vm.module("Vch_control_1D.GD_1D")
    ocfg, box, u0 = _refine_case(pr)
    r0 = _radius_of(pr, 0.05)
    uh, host = G1.trust_refine(pr.cfg, ocfg, u0, pr.phi_Q, pr.phi_T, n_rounds=4, radius0=r0)
    ud, dev = G1.trust_refine(pr.cfg, ocfg, u0, pr.phi_Q, pr.phi_T, n_rounds=4, radius0=r0, on_device=True)
    for r, (a, b) in enumerate(zip(dev, host)):
        print(f"MEASURE round {r}: device {a}; host {b}")
    assert len(dev) == len(host) == 4
    for a, b in zip(dev, host):
        assert set(a) == set(b)
        for key in a:
            assert a[key] == b[key] or (a[key] != a[key] and b[key] != b[key]), key
    assert np.array_equal(ud, uh)
    assert any(a["status"] == "accepted" for a in dev) and any(a["cg_status"] in ("boundary", "negcurv") for a in dev)
    assert dev[-1]["cost_new"] < dev[0]["cost"]
    # the engine call itself
    eng = _pgd(pr, [box], u0[None])
    R = eng.pgd_trust(4, r0)
    assert np.array_equal(eng.pgd_get("u").reshape(ud.shape), ud) and R["rounds"] == 4
    for r, a in enumerate(dev):
        assert (a["cost"], a["cost_new"], a["radius"], a["xnorm"]) == tuple(R[key][0, r] for key in ("cost", "cost_new", "radius", "xnorm"))
        assert Vm.Engine1D.TRUST_STATUS[R["status"][0, r]] == a["status"]
    eng.close()


def _members(pr):
    """Member 0: the case of test_newton_refine inside a small radius (boundary exits).  Member 1: u0 = 0 has an empty free
    set (STATIONARY at round 0).  Member 2: a b3 so negative that the first CG direction has negative curvature."""
    _, box, u = _refine_case(pr)
    W = _weights(pr).ravel()[pr.free]
    b3 = 1.0 - 4.0 * np.linalg.eigvalsh(pr.A)[-1] / W[W > 0].min()
    opts = [box, pr.V.make_opt(pr.ocfg, kappa_sparsity=0.05, u_min=-0.5, u_max=0.5), pr.V.make_opt(pr.ocfg, b3=b3, u_min=-0.9, u_max=0.9)]
    # member 2 starts inside its box: a node outside is clipped by every trial whatever the radius, which under a negative b3
    # raises the cost by an amount that does not shrink with the radius (measured: rho = -3.2, -16, -67, -271 over four quarterings)
    return opts, np.stack([u, np.zeros_like(u), np.clip(u, -0.9, 0.9)]), np.array([_radius_of(pr, 0.05), 1.0, _radius_of(pr, 0.02)])


def test_rounds_batch_of_three_and_the_reason_for_the_feature(refine):
    pr = refine
    opts, u0, radius0 = _members(pr)
    n_rounds = 4
    eng = _pgd(pr, opts, u0)
    many = eng.pgd_trust(n_rounds, radius0)
    Um, Pm = eng.pgd_get("u"), eng.pgd_get("phi")
    eng.close()
    print(f"MEASURE rounds: status {many['status'].tolist()} cg {many['cg_status'].tolist()} in {many['cg_steps'].tolist()} radius "
          f"{many['radius'].tolist()} ratio {many['ratio'].tolist()} cost {many['cost'].tolist()} -> {many['cost_new'].tolist()}")
    assert many["rounds"] == n_rounds
    assert many["status"][1].tolist() == [STATIONARY] + [IDLE] * (n_rounds - 1) and many["n_free"][1, 0] == 0 and not Um[1].any()
    assert np.isnan(many["ratio"][1]).all() and np.isnan(many["cost"][1, 1:]).all()
    # the premise: the damped rounds end this member at once on negative curvature and do not move it
    twin = _pgd(pr, [opts[2]], u0[2][None])
    N = twin.pgd_newton(1)
    assert N["status"][0, 0] == NT_NEGCURV and N["cost_new"][0, 0] == N["cost"][0, 0] and np.array_equal(twin.pgd_get("u").reshape(u0[2].shape), u0[2])
    twin.close()
    # the trust-region rounds follow that direction to the boundary, accept, and lower the cost
    assert many["cg_status"][2, 0] == NEGCURV and many["cg_steps"][2, 0] == 1
    acc = many["status"][2] == ACCEPTED
    assert acc.any() and many["cost_new"][2, -1] < many["cost"][2, 0] and not np.array_equal(Um[2], u0[2])
    assert (many["cost_new"][2][acc] <= many["cost"][2][acc] - 1e-4 * many["pred"][2][acc]).all()
    assert (np.abs(Um) <= 0.9).all()
    live = many["status"] != IDLE
    assert (many["cost_new"][live] <= many["cost"][live]).all()
    for i in range(3):
        one = _pgd(pr, [opts[i]], u0[i][None])
        got = one.pgd_trust(n_rounds, radius0[i])
        U1, P1 = one.pgd_get("u"), one.pgd_get("phi")
        one.close()
        assert got["rounds"] == (n_rounds, 1, n_rounds)[i]
        for key in OUT_KEYS:
            assert np.array_equal(got[key][0], many[key][i], equal_nan=True), (key, i)
        assert np.array_equal(U1.reshape(Um[i].shape), Um[i]) and np.array_equal(P1.reshape(Pm[i].shape), Pm[i]), i


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors come before anything is enqueued; refused allocations
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_anything_is_enqueued_or_allocated(refine):
    pr, Vm = refine, refine.V
    lib = Vm.load()
    last_error = Vm.module("_lib").last_error
    _, box, u0 = _refine_case(pr)
    fresh = pr.context(1)
    live = lib.vch_mem_live()
    with pytest.raises(Vm.VchError, match="-3"):
        fresh.pgd_trust(1, 1.0)
    assert "vch1d_pgd_trust" in last_error() and lib.vch_mem_live() == live
    b = _q0(pr.shape, 45)
    for bad in (0.0, -1.0, np.nan, -np.inf):
        with pytest.raises(ValueError):
            _tr(pr, fresh, 3, bad, rhs=b)
        assert "vch1d_hess_cg_tr" in last_error() and "radius" in last_error() and lib.vch_mem_live() == live, bad
    with pytest.raises(Vm.VchError, match="-3"):
        fresh.cg_vector("x")                                         # nothing ran
    fresh.close()
    eng = _pgd(pr, [box], u0[None])
    U, P = eng.pgd_get("u"), eng.pgd_get("phi")
    live = lib.vch_mem_live()
    for bad in (dict(n_rounds=0), dict(k=0), dict(precond=2), dict(cg_tol=np.nan), dict(cg_tol=np.inf), dict(radius0=0.0),
                dict(radius0=-1.0), dict(radius0=np.nan), dict(radius0=np.inf), dict(radius_max=0.0), dict(radius_max=np.inf),
                dict(radius_max=np.nan), dict(radius_min=0.0), dict(radius_min=-1.0), dict(radius_min=np.nan), dict(radius_min=np.inf)):
        args = dict(n_rounds=2, radius0=1.0)
        args.update(bad)
        with pytest.raises(ValueError):
            eng.pgd_trust(**args)
        assert "vch1d_pgd_trust" in last_error(), bad
        assert lib.vch_mem_live() == live, bad
        assert np.array_equal(eng.pgd_get("u"), U) and np.array_equal(eng.pgd_get("phi"), P), bad
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    d, i32, i64 = np.zeros(8), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int64)
    ip = i32.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.vch1d_pgd_trust(eng.ctx, 1, 3, 1e-8, 1, 0.0, None, 8.0, 1e-9, dp(d), dp(d), dp(d), dp(d), dp(d), dp(d), dp(d), ip, ip, ip,
                               i64.ctypes.data_as(C.POINTER(C.c_int64)), None) == -1
    assert lib.vch1d_pgd_trust(eng.ctx, 1, 3, 1e-8, 1, 0.0, dp(np.ones(1)), 8.0, 1e-9, dp(d), dp(d), dp(d), dp(d), dp(d), None, dp(d), ip,
                               ip, ip, i64.ctypes.data_as(C.POINTER(C.c_int64)), None) == -1
    assert lib.vch_mem_live() == live and np.array_equal(eng.pgd_get("u"), U)
    eng.close()


def test_refused_allocations_and_the_balance(refine):
    pr, Vm = refine, refine.V
    lib = Vm.load()
    _, box, u0 = _refine_case(pr)
    r0 = _radius_of(pr, 0.05)
    base = lib.vch_mem_live()
    eng = _pgd(pr, [box], u0[None])
    live0 = lib.vch_mem_live()
    want = eng.pgd_trust(1, r0, k=3)
    m = lib.vch_mem_live() - live0
    u_want = eng.pgd_get("u")
    eng.pgd_trust(1, r0, k=3)
    eng.pgd_newton(1, k=3)
    assert lib.vch_mem_live() - live0 == m                # the rounds run in the storage of the damped rounds
    eng.close()
    assert lib.vch_mem_live() == base
    print("lazy requests of the first call:", m)
    assert m >= 6
    for i in range(m):
        eng = _pgd(pr, [box], u0[None])
        live0 = lib.vch_mem_live()
        lib.vch_mem_refuse_after(i)
        try:
            with pytest.raises(Vm.VchError, match="-2|-4"):
                eng.pgd_trust(1, r0, k=3)
        finally:
            lib.vch_mem_refuse_after(-1)
        assert lib.vch_mem_live() == live0, (i, lib.vch_mem_live() - live0)
        assert np.array_equal(eng.pgd_get("u").reshape(u0.shape), u0)  # the context stays usable, the iterate is as it was
        got = eng.pgd_trust(1, r0, k=3)                    # the same call then succeeds with the same bits
        assert lib.vch_mem_live() - live0 == m
        for key in OUT_KEYS:
            assert np.array_equal(got[key], want[key], equal_nan=True), key
        assert np.array_equal(eng.pgd_get("u"), u_want)
        eng.close()
        assert lib.vch_mem_live() == base


def test_run_sweep_polishes_with_trust_rounds(V):                # noqa: F811
    import test_gpu_sweep_1d as S
    K1 = V.module("Vch_control_1D.config")
    G1 = V.module("Vch_control_1D.GD_1D")
    cfg = K1.ForwardSolverConfig(N=S.N, T=S.M * S.DT, dt_initial=S.DT)
    members = [K1.OptimizationConfig(**S.MEMBERS[n]) for n in S.NAMES]
    kw = dict(n_iter=S.N_ITER, seed=42, amp=0.05, return_controls=True)
    plain = G1.run_sweep(cfg, members, **kw)
    res = G1.run_sweep(cfg, members, n_trust=2, radius0=0.05, **kw)
    assert set(res) == set(plain) | {"trust", "costs_trust"}
    for key in ("costs", "alphas", "trials", "changes", "tracking_error", "terminal_error"):
        assert np.array_equal(res[key], plain[key]), key                 # the polish comes after the PGD iterations
    ct, T = res["costs_trust"], res["trust"]
    print(f"MEASURE sweep: costs_trust {ct.tolist()} status {T['status'].tolist()} radius {T['radius'].tolist()} ratio {T['ratio'].tolist()} "
          f"cg {T['cg_status'].tolist()} steps {T['cg_steps'].tolist()}")
    assert ct.shape == (len(members), 3) and np.isfinite(ct).all()
    assert np.array_equal(ct[:, 0], plain["costs"][:, -1]) and (np.diff(ct, axis=1) <= 0.0).all()
    moved = T["status"] == ACCEPTED
    for b in range(len(members)):
        if not moved[b].any():
            assert np.array_equal(res["u"][b], plain["u"][b])
