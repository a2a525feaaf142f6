"""vch2d_hess_cg_tr / vch2d_pgd_trust on the GPU: Steihaug-Toint truncated conjugate gradients in a trust region on the free
set of the 2D engine and the trust-region rounds about the resident PGD iterate, against vch2d_hess_cg bit
for bit where no boundary is met, against the NumPy restatement tests/_trust_ref.py (pinned by test_trust_ref_cpu.py) on the
dense blocks assembled from Engine2D.hessvec, against the host loop GD2_configured.trust_refine, and a batch against
single-trajectory contexts.

Problems (the fixtures of test_gpu_krylov_2d.py and test_gpu_krylov_grid_2d.py):
    dense    12 x 9, M = 2 (390 nodes, 190 free), GEMM-DCT, one tile; with b3 = 1, box +-0.9, u0 = u + 0.75 the case of
             test_gpu_newton_2d.test_rounds_against_the_host_driver
    tiles    128 x 32, Ly 0.5, M = 2: 3 x 3 tiles, 24 free nodes
    chunks   16 x 16 (FFT), 21 levels under VCH_KR_LCHUNK=4: six chunks of levels, 12 free nodes
    grid     tiles x chunks x batch 3, max_steps above the march
    sweep    64 x 32, 4 steps: the members of test_gpu_sweep.py through GD2_configured.run_sweep

Tolerances (none tuned against the code under test).
    bits          radius = +inf against hess_cg, a batch member against a context of its own, Engine2D.pgd_trust against the
                  driver's device path: exact.
    restatement   the same step count as _trust_ref.steihaug on the dense block; resid (absolute), curv (of the largest) and
                  pred (relative) at TOL of test_gpu_hess_cg_2d.py (10 x what it measured for the same quantities from the
                  same kernels, inside the class 1.5e-11).  The block is assembled, and the step run, with the linear solves at
                  STEPS_RTOL = 1e-14, under which test_gpu_hess_cg_2d.py compares with the restatement on tiles and chunks.
                  With the fixtures' blocks (default solves, 1e-12) and the step at the default, resid missed 4.3e-13 in
                  four of the twelve cases (tiles step 3 with D: 2.09e-12; chunks: 1.07e-12, 1.76e-12, 2.46e-12).  That is
                  the reference's error: tau solves xx + 2 tau xp + tau^2 pp = radius^2, and on tiles with D the norms of
                  x_2 and x_3 differ by 7.2e-5 relative, so radius^2 - xx is a small difference; the restatement's own
                  resid at that exit moves by 2.4e-12 when its matrix moves by 1e-14 lambda_max and by 1.3e-10 at 1e-12
                  (CPU, on the fixture's block).  Measured at 1e-14 on an MI355X: resid at most 3.04e-14, curv 7.07e-15,
                  pred 1.81e-15; the two blocks differ by 2.5e-15 - 2.8e-14 of lambda_max.
    boundary      | ||x||_D - radius | / radius with ||x||_D computed on the host from cg_vector("x"), and xnorm against the
                  radius: 10 x the restatement's own deviation (its direct norm against the radius and against its
                  recurrence) on the same block and radius, that deviation taken as at least one eps.  DESIGN.md 10l records
                  both.
    identities    r = P b - A x (of ||P b||) and pred = b.x - x.Ax / 2 (of sum |b||x|): the class 1.5e-11 times cond(block).
    host loop     statuses, CG exits and n_free equal, CG steps within one; cost, cost_new and the control at 10 x MEASURED
                  below (the scheme of test_gpu_newton_2d.py: the device rounds run the kernels of the host loop on the
                  same operands)."""
import ctypes as C

import numpy as np
import pytest

from _cg_ref import CONVERGED, LIMIT, NEGCURV
from _trust_ref import BOUNDARY, steihaug
from test_gpu_hess_cg_2d import STEPS_RTOL, TOL as CG_TOL, _full, _mass
from test_gpu_hessvec_2d import DN, EPS
from test_gpu_krylov_2d import Problem, V, _mask_of, _q0, _tile, chunks, dense, tiles      # noqa: F401 (fixtures)
from test_gpu_krylov_grid_2d import grid                                                    # noqa: F401 (fixture)
from test_gpu_newton_2d import PGD_KEYS, _box_cut, _pgd, _refine_case

pytestmark = pytest.mark.gpu

CLASS = 1.5e-11
# relative differences between the device rounds and the host loop (the MEASURE lines of test 5)
MEASURED = dict(cost=0.0, cost_new=0.0, control=0.0)
TOL = {k: 10 * v for k, v in MEASURED.items()}
assert max(TOL.values()) <= CLASS and max(CG_TOL.values()) <= CLASS
ACCEPTED, STATIONARY, NT_NEGCURV, BREAKDOWN, STALLED, IDLE, REJECTED = range(7)
CG_KEYS = ("steps", "status", "n_free", "resid", "curv", "pred", "rnorm0")
TR_KEYS = CG_KEYS + ("xnorm",)
OUT_KEYS = ("cost", "cost_new", "pred", "rnorm0", "radius", "ratio", "xnorm", "cg_steps", "cg_status", "status", "n_free", "pinned",
            "clipped")


def _args(pr, nb, kw):
    args = pr.kw(nb)
    args.update(kw)
    args.setdefault("opt", pr.opt)
    return args


def _tr(pr, eng, k, radius, nb=1, **kw):
    return eng.hess_cg_trust(k, radius, **_args(pr, nb, kw))


def _cg(pr, eng, k, nb=1, **kw):
    return eng.hess_cg(k, **_args(pr, nb, kw))


def _vectors(eng):
    return [eng.cg_vector(w) for w in "xrp"]


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _dnorm(pr, X, precond):
    return float(np.sqrt(np.sum((_mass(pr) if precond else 1.0) * X * X)))


def _ref(blk, bf, k, radius, cg_tol, Df):
    return steihaug(lambda v: blk @ v, np.ones(len(bf), dtype=bool), bf, k, radius, cg_tol, Df)


def _ref_dev(ref, Df, radius):
    """The restatement's own deviation from the boundary: its direct norm and its recurrence against the radius and each other."""
    direct = float(np.sqrt(np.sum((1.0 if Df is None else Df) * ref["x"] ** 2)))
    return max(abs(direct - radius), abs(ref["xnorm"] - radius), abs(direct - ref["xnorm"])) / radius


_BLOCKS = {}


def _block_at_steps_rtol(pr, name):
    """The symmetrised block of the Hessian on the free nodes from Engine2D.hessvec with its linear solves at STEPS_RTOL, in
    calls of batch 30 at most.  The fixtures' blocks carry the default solves' residual, 1e-12: at a boundary exit the
    restatement's own resid moves by more than the asserted 4.3e-13 when its matrix moves by that much (see "restatement" in
    the docstring), so the reference and the run compared with it both take the solves test_gpu_hess_cg_2d.py compares step
    counts under."""
    if name not in _BLOCKS:
        n, nb = len(pr.free), min(30, len(pr.free))
        eng = pr.context(nb)
        A = np.empty((n, n))
        for k0 in range(0, n, nb):
            idx = np.arange(k0, min(k0 + nb, n))
            E = np.zeros((nb, pr.u.size))
            E[np.arange(len(idx)), pr.free[idx]] = 1.0
            r = eng.hessvec(E.reshape((nb,) + pr.shape), opt=pr.opt, rtol=STEPS_RTOL, **pr.kw(nb))
            assert r["stats"]["unconverged_solves"] == 0 and r["stats"]["max_lin_relres"] <= STEPS_RTOL
            A[idx] = r["hv"].reshape(nb, -1)[:len(idx)][:, pr.free]
        eng.close()
        _BLOCKS[name] = 0.5 * (A + A.T)
    return _BLOCKS[name]


def _radius_for_exit_at(blk, bf, j, Df):
    """Between the D-norms of the plain iterates x_{j-1} and x_j (they grow with the steps): their geometric mean, half of
    ||x_1||_D for j = 1.  The step that leaves the region is then step j by a wide margin."""
    norms = [0.0 if i == 0 else float(np.sqrt(np.sum((1.0 if Df is None else Df) * _ref(blk, bf, i, np.inf, 1e-30, Df)["x"] ** 2)))
             for i in (j - 1, j)]
    assert norms[1] > norms[0]
    return 0.5 * norms[1] if j == 1 else float(np.sqrt(norms[0] * norms[1]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. radius = +inf is vch2d_hess_cg bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("limit", [False, True])
@pytest.mark.parametrize("name", ["dense", "tiles", "chunks"])
def test_an_infinite_radius_is_hess_cg_bit_for_bit(request, name, limit, precond):
    pr = request.getfixturevalue(name)
    b = _q0(pr.shape, 41)
    k, cg_tol = (3, 1e-30) if limit else (2 * len(pr.free), 1e-8)
    kw = dict(rhs=b, cg_tol=cg_tol, precond=precond, mask=None if name == "dense" else pr.mask)
    eng = pr.context(1)
    want = _cg(pr, eng, k, **kw)
    Vw = _vectors(eng)
    got = _tr(pr, eng, k, np.inf, **kw)
    Vg = _vectors(eng)
    eng.close()
    assert want["status"][0] == (LIMIT if limit else CONVERGED) and want["n_free"][0] == len(pr.free)
    for key in CG_KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    for key in ("resid", "curv", "pred", "rnorm0"):
        assert _bits(got[key], want[key]), key
    for w, a, c in zip("xrp", Vg, Vw):
        assert _bits(a, c), w
    direct = _dnorm(pr, Vg[0][0], precond)
    print(f"MEASURE inf {name} precond {precond} k {k}: steps {got['steps'][0]} xnorm {got['xnorm'][0]:.17g} direct {direct:.17g} "
          f"rel. dev {abs(got['xnorm'][0] / direct - 1):.2e}")
    assert np.isfinite(got["xnorm"][0]) and got["xnorm"][0] > 0
    assert got["stats"]["linear_solves"] == want["stats"]["linear_solves"] and got["stats"]["launches"] == want["stats"]["launches"]


def test_an_infinite_radius_on_the_grid_at_batch_three(grid):
    pr = grid
    b = _q0((3,) + pr.shape, 42)
    kw = dict(rhs=b, cg_tol=1e-30, mask=pr.masks, opt=pr.opts)
    eng = pr.context(3)
    want = _cg(pr, eng, 5, nb=3, **kw)
    Vw = _vectors(eng)
    got = _tr(pr, eng, 5, np.inf, nb=3, **kw)
    Vg = _vectors(eng)
    # member 1 inside a radius its second step leaves (by the restatement on its block): on the boundary; the members beside it
    # are untouched by that
    nodes = pr.free[pr.sub[1]]
    blk, bf, Df = pr.A[np.ix_(pr.sub[1], pr.sub[1])], b[1].ravel()[nodes], _mass(pr).ravel()[nodes]
    rad = np.array([np.inf, _radius_for_exit_at(blk, bf, 2, Df), np.inf])
    R = _tr(pr, eng, 5, rad, nb=3, **kw)
    X = eng.cg_vector("x")
    eng.close()
    assert list(want["status"]) == [LIMIT] * 3 and list(want["steps"]) == [5] * 3 and list(want["n_free"]) == [27, 18, 9]
    for key in CG_KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    for w, a, c in zip("xrp", Vg, Vw):
        assert _bits(a, c), w
    assert np.isfinite(got["xnorm"]).all() and (got["xnorm"] > 0).all()
    assert list(R["status"]) == [LIMIT, BOUNDARY, LIMIT] and R["steps"][1] == 2
    for i in (0, 2):
        assert _bits(X[i], Vg[0][i]) and R["xnorm"][i] == got["xnorm"][i], i
    dev = max(abs(_dnorm(pr, X[1], True) - rad[1]), abs(R["xnorm"][1] - rad[1])) / rad[1]
    ref = _ref(blk, bf, 5, rad[1], 1e-30, Df)
    ref_dev = _ref_dev(ref, Df, rad[1])
    print(f"MEASURE grid boundary: steps {R['steps'][1]} / {ref['steps']} dev {dev / EPS:.2f} eps, restatement {ref_dev / EPS:.2f} eps")
    assert ref["status"] == BOUNDARY and ref["steps"] == 2
    assert dev <= 10 * max(ref_dev, EPS)


# ---------------------------------------------------------------------------------------------------------------------
# 2. boundary exits against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("exit_at", [1, 3])
@pytest.mark.parametrize("name", ["dense", "tiles", "chunks"])
def test_boundary_exits_against_the_restatement(request, name, exit_at, precond):
    pr = request.getfixturevalue(name)
    _, free, coarse, D = _full(pr)
    blk = _block_at_steps_rtol(pr, name)
    cond = np.linalg.cond(blk)
    print(f"MEASURE boundary {name}: the fixture's block against the one at rtol {STEPS_RTOL:g}: "
          f"{np.abs(coarse - blk).max() / np.linalg.eigvalsh(blk)[-1]:.2e} of lambda_max")
    b = _q0(pr.shape, 43)
    bf = b.ravel()[free]
    Df = D[free] if precond else None
    radius = _radius_for_exit_at(blk, bf, exit_at, Df)
    k = 2 * len(free)
    ref = _ref(blk, bf, k, radius, 1e-8, Df)
    eng = pr.context(1)
    R = _tr(pr, eng, k, radius, rhs=b, cg_tol=1e-8, precond=precond, mask=None if name == "dense" else pr.mask, rtol=STEPS_RTOL)
    X, Rr, _ = (v[0] for v in _vectors(eng))
    eng.close()
    m = int(R["steps"][0])
    print(f"MEASURE boundary {name} precond {precond} exit {exit_at}: steps {m} / {ref['steps']} status {R['status'][0]} / {ref['status']} "
          f"cond {cond:.3g} radius {radius:.6e}")
    assert ref["status"] == BOUNDARY and ref["steps"] == exit_at
    assert R["status"][0] == BOUNDARY and m == exit_at and R["n_free"][0] == len(free)
    assert not X[~pr.mask].any() and not Rr[~pr.mask].any() and np.isfinite(X).all()
    assert np.isnan(R["resid"][0, m:]).all() and np.isnan(R["curv"][0, m:]).all() and np.isfinite(R["resid"][0, :m]).all()
    d_res = np.abs(R["resid"][0, :m] - ref["resid"][:m]).max()
    d_curv = np.abs(R["curv"][0, :m] - ref["curv"][:m]).max() / np.abs(ref["curv"][:m]).max()
    d_pred = abs(R["pred"][0] - ref["pred"]) / abs(ref["pred"])
    print(f"MEASURE boundary {name} precond {precond} exit {exit_at}: resid {d_res:.2e} curv {d_curv:.2e} pred {d_pred:.2e} "
          f"(bounds {CG_TOL['resid']:.2e} {CG_TOL['curv']:.2e} {CG_TOL['pred']:.2e})")
    assert d_res < CG_TOL["resid"] and d_curv < CG_TOL["curv"] and d_pred < CG_TOL["pred"]
    # r = P b - A x and pred = b.x - x.Ax / 2
    xf = X.ravel()[free]
    ax = blk @ xf
    d_r = np.abs(Rr.ravel()[free] - (bf - ax)).max() / np.linalg.norm(bf)
    d_model = abs(R["pred"][0] - (float(bf @ xf) - 0.5 * float(xf @ ax))) / float(np.sum(np.abs(bf * xf)))
    print(f"MEASURE boundary {name} precond {precond} exit {exit_at}: r identity {d_r:.2e} pred identity {d_model:.2e} "
          f"(bound {CLASS * cond:.2e})")
    assert d_r <= CLASS * cond and d_model <= CLASS * cond
    # the boundary itself, on the host from x, against the restatement's own deviation on this block
    ref_dev = _ref_dev(ref, Df, radius)
    dev = max(abs(_dnorm(pr, X, precond) - radius), abs(R["xnorm"][0] - radius)) / radius
    print(f"MEASURE boundary {name} precond {precond} exit {exit_at}: | ||x||_D - radius | / radius {dev / EPS:.2f} eps, restatement "
          f"{ref_dev / EPS:.2f} eps")
    assert dev <= 10 * max(ref_dev, EPS)


# ---------------------------------------------------------------------------------------------------------------------
# 3. negative curvature is followed to the boundary
# ---------------------------------------------------------------------------------------------------------------------
def _shifted(pr, b3):
    """(opt, block): H(b3') = H(b3) + (b3' - b3) diag(wt (x) W) on the free nodes of `dense`."""
    Df = _mass(pr).ravel()[pr.free]
    return (pr.V.make_opt(pr.ocfg, u_min=DN["u_min"], u_max=DN["u_max"], b3=b3),
            pr.Hm[np.ix_(pr.free, pr.free)] + (b3 - pr.opt.b3) * np.diag(Df))


@pytest.mark.parametrize("precond", [False, True])
def test_negative_definite_steps_to_the_boundary_at_step_zero(dense, precond):
    pr = dense
    opt, blk = _shifted(pr, -6e-5)
    assert np.linalg.eigvalsh(blk)[-1] < 0
    b = _q0(pr.shape, 24)
    bf = b.ravel()[pr.free]
    Df = _mass(pr).ravel()[pr.free] if precond else None
    D = Df if precond else np.ones(len(bf))
    radius = 0.75
    eng = pr.context(1)
    R = _tr(pr, eng, 5, radius, rhs=b, precond=precond, opt=opt)
    X = eng.cg_vector("x")[0]
    Rinf = _tr(pr, eng, 5, np.inf, rhs=b, precond=precond, opt=opt)
    Xinf = eng.cg_vector("x")[0]
    eng.close()
    ref = _ref(blk, bf, 5, radius, 0.0, Df)
    g = bf / D
    tau = radius / np.sqrt(np.sum(D * g * g))
    d_x = np.abs(X.ravel()[pr.free] - tau * g).max() / np.abs(tau * g).max()
    ref_dev = _ref_dev(ref, Df, radius)
    dev = max(abs(_dnorm(pr, X, precond) - radius), abs(R["xnorm"][0] - radius)) / radius
    d_curv = abs(R["curv"][0, 0] - ref["curv"][0]) / abs(ref["curv"][0])
    d_pred = abs(R["pred"][0] - ref["pred"]) / abs(ref["pred"])
    print(f"MEASURE negative definite precond {precond}: x {d_x / EPS:.2f} eps curv {d_curv:.2e} pred {d_pred:.2e}; boundary {dev / EPS:.2f} eps, "
          f"restatement {ref_dev / EPS:.2f} eps; pred {R['pred'][0]:.6e}")
    assert ref["status"] == NEGCURV and ref["steps"] == 1
    assert R["status"][0] == NEGCURV and R["steps"][0] == 1 and R["curv"][0, 0] < 0 and np.isnan(R["curv"][0, 1:]).all()
    assert R["pred"][0] > 0 and not X[~pr.mask].any()
    assert d_x <= (len(bf) + 8) * EPS             # tau: a square root and a quotient of sums of n positive terms in any order
    assert d_curv < CG_TOL["curv"] and d_pred < CG_TOL["pred"]
    assert dev <= 10 * max(ref_dev, EPS)
    assert R["stats"]["linear_solves"] == pr.M * 3                   # one product taken
    # without a boundary the call stops as hess_cg does
    assert Rinf["status"][0] == NEGCURV and Rinf["steps"][0] == 0 and not Xinf.any() and Rinf["pred"][0] == 0.0 and Rinf["xnorm"][0] == 0.0


@pytest.mark.parametrize("precond", [False, True])
def test_an_indefinite_direction_is_followed_to_the_boundary(dense, precond):
    pr = dense
    opt, blk = _shifted(pr, -1e-6)
    b = _q0(pr.shape, 25)
    bf = b.ravel()[pr.free]
    Df = _mass(pr).ravel()[pr.free] if precond else None
    plain = _ref(blk, bf, 60, np.inf, 0.0, Df)       # stops before the direction of non-positive curvature, x as it is
    assert plain["status"] == NEGCURV and 2 <= plain["steps"] <= 5
    radius = 10.0 * plain["xnorm"]                  # far outside every iterate before that direction
    ref = _ref(blk, bf, 60, radius, 0.0, Df)
    eng = pr.context(1)
    R = _tr(pr, eng, 60, radius, rhs=b, precond=precond, opt=opt)
    X = eng.cg_vector("x")[0]
    eng.close()
    m = int(R["steps"][0])
    ref_dev = _ref_dev(ref, Df, radius)
    dev = max(abs(_dnorm(pr, X, precond) - radius), abs(R["xnorm"][0] - radius)) / radius
    print(f"MEASURE indefinite precond {precond}: exit after {m} steps (restatement {ref['steps']}, plain {plain['steps']}) status "
          f"{R['status'][0]} / {ref['status']}; boundary {dev / EPS:.2f} eps, restatement {ref_dev / EPS:.2f} eps")
    assert ref["status"] == NEGCURV and ref["steps"] == plain["steps"] + 1
    assert abs(m - ref["steps"]) <= 1 and R["status"][0] in (NEGCURV, BOUNDARY)
    if m == ref["steps"]:
        assert R["status"][0] == NEGCURV and R["curv"][0, m - 1] <= 0 and (R["curv"][0, :m - 1] > 0).all()
    assert R["pred"][0] > 0 and np.isnan(R["curv"][0, m:]).all() and np.isfinite(R["resid"][0, :m]).all()
    assert dev <= 10 * max(ref_dev, EPS)


# ---------------------------------------------------------------------------------------------------------------------
# 4. a batch of three with its own radii against three single contexts
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_of_three_equals_three_single_contexts(dense):
    pr, Vm = dense, dense.V
    masks = np.stack([_mask_of(pr.shape, pr.free[[4, 77, 150]]), pr.mask, pr.mask])
    opts = [pr.opt, pr.opt, _shifted(pr, -6e-5)[0]]
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
    assert list(many["status"]) == [CONVERGED, BOUNDARY, NEGCURV] and many["steps"][0] <= 4 and many["steps"][2] == 1
    assert many["xnorm"][0] < radius[0]
    for i in range(3):
        eng = pr.context(1)
        one = _tr(pr, eng, k, radius[i], rhs=b[i], precond=True, mask=masks[i], cg_tol=1e-8, opt=opts[i])
        for key in TR_KEYS:
            assert np.array_equal(one[key][0], many[key][i], equal_nan=True), (key, i)
        for w, vm in zip("xrp", Vmany):
            assert _bits(eng.cg_vector(w)[0], vm[i]), (w, i)
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the device rounds equal the host loop
# ---------------------------------------------------------------------------------------------------------------------
def _radius_of(pr, u, frac):
    return frac * _dnorm(pr, u, True)


def test_device_rounds_equal_the_host_loop(dense):
    pr, Vm = dense, dense.V
    G2 = Vm.module("Vch_control_2D.GD2_configured")
    ocfg, box, u0 = _refine_case(pr)
    r0 = _radius_of(pr, u0, 0.05)
    n = 4
    uh, host = G2.trust_refine(pr.cfg, ocfg, u0, pr.phi_Q, pr.phi_T, n_trust=n, radius0=r0)
    ud, dev = G2.trust_refine(pr.cfg, ocfg, u0, pr.phi_Q, pr.phi_T, n_trust=n, radius0=r0, on_device=True)
    rel = lambda a, b: abs(a - b) / abs(b)
    worst = dict(cost=0.0, cost_new=0.0)
    assert len(dev) == len(host) == n and ud.shape == uh.shape
    for r, (a, b) in enumerate(zip(dev, host)):
        print(f"MEASURE round {r}: device {a}; host {b}")
        assert set(a) == set(b)
        assert (a["status"], a["cg_status"], a["n_free"]) == (b["status"], b["cg_status"], b["n_free"]), r
        assert abs(a["steps"] - b["steps"]) <= 1, r
        for key in worst:
            worst[key] = max(worst[key], rel(a[key], b[key]))
    worst["control"] = float(np.abs(ud - uh).max() / np.abs(uh).max())
    print(f"MEASURE against the host loop: {worst}")
    for key in worst:
        assert worst[key] <= TOL[key], key
    assert any(a["status"] == "accepted" for a in dev) and any(a["cg_status"] in ("boundary", "negcurv") for a in dev)
    assert dev[-1]["cost_new"] < dev[0]["cost"] and (np.abs(ud) <= 0.9).all()
    # the engine call itself: the records of the driver's device path, bit for bit
    eng = _pgd(pr, [box], u0[None])
    R = eng.pgd_trust(n, r0)
    assert _bits(eng.pgd_get("u").reshape(ud.shape), ud) and R["rounds"] == n
    for r, a in enumerate(dev):
        for key in ("cost", "cost_new", "pred", "rnorm0", "radius", "xnorm"):
            assert a[key] == R[key][0, r], (key, r)
        assert a["ratio"] == R["ratio"][0, r] or (np.isnan(a["ratio"]) and np.isnan(R["ratio"][0, r]))
        assert Vm.Engine2D.TRUST_STATUS[R["status"][0, r]] == a["status"] and Vm.Engine2D.TRUST_CG_STATUS[R["cg_status"][0, r]] == a["cg_status"]
        assert (a["steps"], a["n_free"]) == (R["cg_steps"][0, r], R["n_free"][0, r])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the reason for the feature: a batch of three against three single contexts
# ---------------------------------------------------------------------------------------------------------------------
def _members(pr):
    """Member 0: b3 = -1e-3 inside the box +-2 from u0 = u, the member of test_gpu_newton_2d.py that the damped rounds leave on
    NEGCURV; it starts strictly inside its box (a node outside is clipped by every trial whatever the radius).
    Member 1: a sparsity parameter under which u0 = 0 has an empty free set (STATIONARY at round 0).  Member 2: the box-cut
    start of test_gpu_newton_2d.py inside a radius ten times its norm: the Newton step is interior, every node of the trial
    is clipped to the bound 2^-20 below and gains about 4e-6 of pred, so the trial is rejected and the radius quartered."""
    V = pr.V
    cut, half = _box_cut(pr)
    opts = [V.make_opt(pr.ocfg, b3=-1e-3, u_min=-2.0, u_max=2.0), V.make_opt(pr.ocfg, kappa_sparsity=1e3, u_min=-0.5, u_max=0.5), cut]
    u0 = np.stack([pr.u, np.zeros_like(pr.u), half])
    assert (np.abs(u0[0]) < 2.0).all()
    return opts, u0, np.array([_radius_of(pr, pr.u, 0.1), 1.0, _radius_of(pr, half, 10.0)])


def test_rounds_batch_of_three_and_the_reason_for_the_feature(dense):
    pr = dense
    opts, u0, radius0 = _members(pr)
    n_rounds = 4
    eng = _pgd(pr, opts, u0)
    many = eng.pgd_trust(n_rounds, radius0)
    Um, Pm = eng.pgd_get("u"), eng.pgd_get("phi")
    eng.close()
    print(f"MEASURE rounds: status {many['status'].tolist()} cg {many['cg_status'].tolist()} in {many['cg_steps'].tolist()} radius "
          f"{many['radius'].tolist()} xnorm {many['xnorm'].tolist()} ratio {many['ratio'].tolist()} cost {many['cost'].tolist()} -> "
          f"{many['cost_new'].tolist()} clipped {many['clipped'].tolist()} pinned {many['pinned'].tolist()}")
    assert 1 <= many["rounds"] <= n_rounds
    # member 1: stationary, then idle
    assert many["status"][1].tolist() == [STATIONARY] + [IDLE] * (n_rounds - 1) and many["n_free"][1, 0] == 0 and not Um[1].any()
    assert many["rnorm0"][1, 0] == 0.0 and many["xnorm"][1, 0] == 0.0 and many["cg_steps"][1].tolist() == [0] * n_rounds
    for key in ("cost", "cost_new", "pred", "rnorm0", "radius", "xnorm"):
        assert np.isnan(many[key][1, 1:]).all(), key
    assert np.isnan(many["ratio"][1]).all() and not many["n_free"][1, 1:].any()
    # the premise: the damped rounds end member 0 at once on negative curvature and do not move it
    twin = _pgd(pr, [opts[0]], u0[0][None])
    N = twin.pgd_newton(1)
    assert N["status"][0, 0] == NT_NEGCURV and N["cost_new"][0, 0] == N["cost"][0, 0] and np.array_equal(twin.pgd_get("u").reshape(u0[0].shape), u0[0])
    twin.close()
    # the trust-region rounds follow that direction to the boundary, accept, and lower the cost
    acc = many["status"][0] == ACCEPTED
    assert acc.any() and many["cost_new"][0, -1] < many["cost"][0, 0] and not np.array_equal(Um[0], u0[0])
    assert many["clipped"][0, np.flatnonzero(acc)[0]] == 0
    assert many["cg_status"][0, 0] == NEGCURV and many["cg_steps"][0, 0] >= 1
    assert (many["cost_new"][0][acc] <= many["cost"][0][acc] - 1e-4 * many["pred"][0][acc]).all()
    # member 2: rejected, unmoved, and on with a quarter of min(radius, ||x||_D)
    st = many["status"][2]
    assert st[0] == REJECTED and many["cost_new"][2, 0] == many["cost"][2, 0] and many["clipped"][2, 0] == pr.u.size
    for r in range(n_rounds - 1):
        if st[r] == REJECTED:
            assert st[r + 1] != IDLE and many["radius"][2, r + 1] < many["radius"][2, r]
            assert many["radius"][2, r + 1] == 0.25 * min(many["radius"][2, r], many["xnorm"][2, r]), r
            assert many["cost"][2, r + 1] == many["cost"][2, r]
    live = many["status"] != IDLE
    assert (many["cost_new"][live] <= many["cost"][live]).all()
    for i in range(3):
        one = _pgd(pr, [opts[i]], u0[i][None])
        got = one.pgd_trust(n_rounds, radius0[i])
        U1, P1 = one.pgd_get("u"), one.pgd_get("phi")
        one.close()
        assert got["rounds"] <= many["rounds"]                  # alone, a trajectory that has ended ends the call
        for key in OUT_KEYS:
            assert np.array_equal(got[key][0], many[key][i], equal_nan=True), (key, i)
        assert _bits(U1.reshape(Um[i].shape), Um[i]) and _bits(P1.reshape(Pm[i].shape), Pm[i]), i


# ---------------------------------------------------------------------------------------------------------------------
# 7. state
# ---------------------------------------------------------------------------------------------------------------------
def test_a_call_that_accepts_nothing_leaves_the_pgd_run_undisturbed(dense):
    """Member 0 is stationary (empty free set), member 1 is the box-cut start, whose one trial is rejected: nothing moves, and
    the iteration that follows is that of a run without the call."""
    pr, Vm = dense, dense.V
    cut, half = _box_cut(pr)
    opts = [Vm.make_opt(pr.ocfg, kappa_sparsity=1e3, u_min=-0.5, u_max=0.5), cut]
    u0 = np.stack([np.zeros_like(pr.u), half])
    plain = _pgd(pr, opts, u0)
    want = plain.pgd_iterate(1)
    u_want, phi_want = plain.pgd_get("u"), plain.pgd_get("phi")
    plain.close()
    eng = _pgd(pr, opts, u0)
    phi0 = eng.pgd_get("phi")
    R = eng.pgd_trust(1, _radius_of(pr, half, 10.0))
    assert R["rounds"] == 1 and R["status"][:, 0].tolist() == [STATIONARY, REJECTED]
    assert np.array_equal(R["cost"][:, 0], R["cost_new"][:, 0])
    assert np.array_equal(eng.pgd_get("u"), u0) and np.array_equal(eng.pgd_get("phi"), phi0)
    got = eng.pgd_iterate(1)
    for key in PGD_KEYS:
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(eng.pgd_get("u"), u_want) and np.array_equal(eng.pgd_get("phi"), phi_want)
    eng.close()


def test_the_adjoint_of_the_replaced_iterate_is_invalid(dense):
    pr, Vm = dense, dense.V
    _, box, u0 = _refine_case(pr)
    eng = _pgd(pr, [box], u0[None], alpha0=1e-3)         # a short first step: the iterate keeps a free set
    eng.pgd_iterate(1)
    eng.pgd_kkt(refresh=False)                           # the sweep of the iteration left r resident
    R = eng.pgd_trust(1, _radius_of(pr, u0, 0.05))
    assert R["status"][0, 0] == ACCEPTED
    with pytest.raises(Vm.VchError, match="-3"):
        eng.pgd_kkt(refresh=False)
    k = eng.pgd_kkt(refresh=True)
    assert k["total"][0] == pr.u.size
    eng.pgd_kkt(refresh=False)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors come before anything is enqueued or allocated; refused allocations
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_anything_is_enqueued_or_allocated(dense):
    pr, Vm = dense, dense.V
    lib = Vm.load()
    last_error = Vm.module("_lib").last_error
    _, box, u0 = _refine_case(pr)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    fresh = pr.context(1)
    live, c0 = lib.vch_mem_live(), fresh.counters()
    with pytest.raises(Vm.VchError, match="-3"):
        fresh.pgd_trust(1, 1.0)
    assert "vch2d_pgd_trust" in last_error() and lib.vch_mem_live() == live and fresh.counters() == c0
    b = _q0(pr.shape, 45)
    for bad in (0.0, -1.0, np.nan, -np.inf):
        with pytest.raises(ValueError):
            _tr(pr, fresh, 3, bad, rhs=b)
        assert "vch2d_hess_cg_tr" in last_error() and "radius" in last_error(), bad
        assert lib.vch_mem_live() == live and fresh.counters() == c0, bad
    # NULL radius or xnorm_out, at the C boundary
    arr = (type(pr.opt) * 1)(pr.opt)
    buf, i32, i64 = np.zeros(8), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64)
    ip, lp = i32.ctypes.data_as(C.POINTER(C.c_int32)), i64.ctypes.data_as(C.POINTER(C.c_int64))
    for radius, xnorm in ((None, buf), (np.ones(1), None)):
        rc = lib.vch2d_hess_cg_tr(fresh.ctx, dp(np.ascontiguousarray(pr.dts, dtype=np.float64)), pr.M,
                                  dp(np.ascontiguousarray(pr.t, dtype=np.float64)), dp(np.ascontiguousarray(pr.x)),
                                  dp(np.ascontiguousarray(pr.y)), None, None, arr, 1, 0.0, None, 0.0, None, 4, 0.0, 1, dp(buf), dp(buf),
                                  dp(buf), dp(buf), ip, ip, lp, None, dp(radius), dp(xnorm))
        assert rc == -1 and "vch2d_hess_cg_tr" in last_error() and lib.vch_mem_live() == live and fresh.counters() == c0
    with pytest.raises(Vm.VchError, match="-3"):
        fresh.cg_vector("x")                                         # nothing ran
    fresh.close()
    eng = _pgd(pr, [box], u0[None])
    U, P = eng.pgd_get("u"), eng.pgd_get("phi")
    live, c0 = lib.vch_mem_live(), eng.counters()
    for bad in (dict(n_rounds=0), dict(n_rounds=-2), dict(k=0), dict(precond=2), dict(precond=-1), dict(cg_tol=np.nan), dict(cg_tol=np.inf),
                dict(radius0=0.0), dict(radius0=-1.0), dict(radius0=np.nan), dict(radius0=np.inf), dict(radius_max=0.0),
                dict(radius_max=np.inf), dict(radius_max=np.nan), dict(radius_min=0.0), dict(radius_min=-1.0), dict(radius_min=np.nan),
                dict(radius_min=np.inf)):
        args = dict(n_rounds=2, radius0=1.0)
        args.update(bad)
        with pytest.raises(ValueError):
            eng.pgd_trust(**args)
        assert "vch2d_pgd_trust" in last_error(), bad
        assert lib.vch_mem_live() == live and eng.counters() == c0, bad
    d = np.zeros(8)
    full = [dp(d)] * 7 + [ip] * 3 + [lp]
    for hole in range(len(full)):
        outs = list(full)
        outs[hole] = None
        assert lib.vch2d_pgd_trust(eng.ctx, 1, 3, 1e-8, 1, 0.0, 0.0, dp(np.ones(1)), 8.0, 1e-9, *outs, None) == -1, hole
        assert eng.counters() == c0, hole
    assert lib.vch2d_pgd_trust(eng.ctx, 1, 3, 1e-8, 1, 0.0, 0.0, None, 8.0, 1e-9, *full, None) == -1
    assert lib.vch_mem_live() == live and eng.counters() == c0
    assert np.array_equal(eng.pgd_get("u"), U) and np.array_equal(eng.pgd_get("phi"), P)
    eng.close()


def test_refused_allocations_and_the_balance(dense):
    pr, Vm = dense, dense.V
    lib = Vm.load()
    _, box, u0 = _refine_case(pr)
    r0 = _radius_of(pr, u0, 0.05)
    base = lib.vch_mem_live()
    eng = _pgd(pr, [box], u0[None])
    live0 = lib.vch_mem_live()
    want = eng.pgd_trust(1, r0, k=3)
    m = lib.vch_mem_live() - live0
    u_want = eng.pgd_get("u")
    eng.pgd_trust(1, r0, k=3)
    eng.pgd_newton(1, k=3)
    eng.hess_cg(3, opt=[box])
    assert lib.vch_mem_live() - live0 == m                # the rounds run in the storage of the damped rounds and of hess_cg
    eng.close()
    assert lib.vch_mem_live() == base
    ref = _pgd(pr, [box], u0[None])
    live1 = lib.vch_mem_live()
    ref.pgd_newton(1, k=3)
    assert lib.vch_mem_live() - live1 == m                # and ask for nothing the damped rounds do not ask for
    ref.close()
    print("lazy requests of the first call:", m)
    assert m >= 4
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
        assert np.array_equal(eng.pgd_get("u").reshape(u0.shape), u0)     # the context stays usable, the iterate is as it was
        got = eng.pgd_trust(1, r0, k=3)                    # the same call then succeeds with the same bits
        assert lib.vch_mem_live() - live0 == m
        for key in OUT_KEYS:
            assert np.array_equal(got[key], want[key], equal_nan=True), (key, i)
        assert _bits(eng.pgd_get("u"), u_want)
        eng.close()
        assert lib.vch_mem_live() == base
    # the step alone: the requests of hess_cg, given back when one is refused
    b = _q0(pr.shape, 46)
    eng = pr.context(1)
    live0 = lib.vch_mem_live()
    want = _tr(pr, eng, 3, 0.5, rhs=b)
    m = lib.vch_mem_live() - live0
    eng.close()
    eng = pr.context(1)
    _cg(pr, eng, 3, rhs=b)
    assert lib.vch_mem_live() - live0 == m
    eng.close()
    for i in range(m):
        eng = pr.context(1)
        live0 = lib.vch_mem_live()
        lib.vch_mem_refuse_after(i)
        try:
            with pytest.raises(Vm.VchError, match="-2|-4"):
                _tr(pr, eng, 3, 0.5, rhs=b)
        finally:
            lib.vch_mem_refuse_after(-1)
        assert lib.vch_mem_live() == live0, (i, lib.vch_mem_live() - live0)
        got = _tr(pr, eng, 3, 0.5, rhs=b)
        for key in TR_KEYS:
            assert np.array_equal(got[key], want[key], equal_nan=True), (key, i)
        eng.close()
        assert lib.vch_mem_live() == base


# ---------------------------------------------------------------------------------------------------------------------
# 9. run_sweep(n_trust)
# ---------------------------------------------------------------------------------------------------------------------
def test_run_sweep_polishes_with_trust_rounds(V):                # noqa: F811
    import test_gpu_sweep as S
    K2 = V.module("Vch_control_2D.config")
    G2 = V.module("Vch_control_2D.GD2_configured")
    cfg = K2.ForwardSolverConfig(Nx=S.NX, Ny=S.NY, Lx=S.LX, Ly=S.LY, T=S.M * S.DT, dt_initial=S.DT, tau=S.TAU)
    members = [K2.OptimizationConfig(**S.MEMBERS[n]) for n in S.NAMES]
    plain = G2.run_sweep(cfg, members, n_iter=S.N_ITER, return_controls=True)
    res = G2.run_sweep(cfg, members, n_iter=S.N_ITER, return_controls=True, n_trust=2, radius0=0.05)
    assert set(res) == set(plain) | {"trust", "costs_trust"}
    for key in ("costs", "alphas", "attempts", "changes", "tracking_error", "terminal_error"):
        assert np.array_equal(res[key], plain[key]), key                 # the polish comes after the PGD iterations
    ct, T = res["costs_trust"], res["trust"]
    print(f"MEASURE sweep: costs_trust {ct.tolist()} status {T['status'].tolist()} radius {T['radius'].tolist()} ratio {T['ratio'].tolist()} "
          f"cg {T['cg_status'].tolist()} steps {T['cg_steps'].tolist()}")
    assert ct.shape == (len(members), 3) and np.isfinite(ct).all()
    assert T["status"].shape == T["radius"].shape == (len(members), 2)
    assert np.array_equal(ct[:, 0], plain["costs"][:, -1]) and (np.diff(ct, axis=1) <= 0.0).all()
    moved = T["status"] == ACCEPTED
    for b in range(len(members)):
        if not moved[b].any():
            assert np.array_equal(res["u"][b], plain["u"][b])
