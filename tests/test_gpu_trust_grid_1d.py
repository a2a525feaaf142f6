"""vch1d_hess_cg_tr / vch1d_pgd_trust where tests/test_gpu_trust_1d.py does not reach: boundary exits on the
eight-chunk grid at batch 3, the rounds off the one-chunk grid (depths 1 and 2, two and three chunks), radii at the ends of
the double range, and the scale equivariance of the step.  The fixtures and helpers are those of the existing files.

Problems: `driver`, `n1030`, `n2051`, `grid` as in test_gpu_trust_1d.py.

Tolerances (none tuned against the code under test).
    bits          a batch member against a context of its own, member 0 (radius = +inf) against hess_cg, radius 2^600 against
                  +inf, the scaled calls against the unscaled one, an accepted control against NumPy's clip: exact.
    boundary      | ||x||_D - radius | / radius and xnorm against the radius: 10 x the restatement's own deviation on the same
                  nodes and radius, that deviation taken as at least one eps (the bound of test_gpu_trust_1d.py).
    identity      r = P b - P H P x (of ||P b||) on the grid: HV_TOL[2][1] times a LOWER bound of cond(block), the ratio of
                  the largest to the smallest Rayleigh quotient the unpreconditioned restatement meets in its five steps (the
                  free set has 21276 nodes, its block is not assembled); test_gpu_trust_1d.py asserts HV_TOL cond(block).
    extremes      radius 2^500: xnorm within 10 eps of the radius (a square root of a product that rounds twice);
                  radius 2^-600: exact zeros and r = P b exactly (tau = 0).
    host loop     statuses, CG exits and n_free equal, CG steps within one; cost, cost_new and the control at 10 x MEASURED
                  below (a measured 0 is asserted as equality), the scheme of test_gpu_newton_1d.py.  The yardstick is the
                  loop composed here from Engine1D.hess_cg_trust, newton_trial(1), forward and cost with the verdicts of
                  tests/_trust_ref.judge (tests/_trust_ref.host_rounds): GD_1D.trust_refine's loop on a problem without a
                  configuration object.

That the tests can fail (two mutant libraries, built from copies of the sources and run on an MI355X against this file, the
2D one and the two test_gpu_trust_state files): without the zeroing of xx, xp and the pending cell before a call (the memset
in 1D, mode 1 of k_ncg_fin_tr in 2D) 43 of the 53 cases fail, all 14 of this file; with an absolute curvature threshold
(`!(c > 1e-20)` for `!(c > 0)`) in both scalar kernels 17 fail: the 16 scaling cases of both engines and one state case."""
import copy

import numpy as np
import pytest

from _cg_ref import CONVERGED, LIMIT, NEGCURV
from _trust_ref import BOUNDARY, host_rounds, off_block_members, steihaug
from test_gpu_hess_cg_1d import KEYS as CG_KEYS, _block, _cg, _mass, _negative_b3
from test_gpu_hessvec_1d import TOL as HV_TOL
from test_gpu_krylov_1d import V, _q0, _tile, driver, small                                   # noqa: F401 (fixtures)
from test_gpu_krylov_grid_1d import grid                                                       # noqa: F401 (fixture)
from test_gpu_newton_1d import _box_cut, _pgd
from test_gpu_second_order_1d import _problem
from test_gpu_trust_1d import ACCEPTED, IDLE, OUT_KEYS, REJECTED, TR_KEYS, _dnorm, _driven, _tr, _vectors
from test_gpu_trust_2d import _radius_for_exit_at

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
CLASS = 1.5e-11
# relative differences between the device rounds and the composed host loop (the MEASURE lines of the rounds off one block)
MEASURED = dict(cost=0.0, cost_new=0.0, control=0.0)
TOL = {k: 10 * v for k, v in MEASURED.items()}
assert max(TOL.values()) <= CLASS


class _Product:
    """v -> (P H P v) on the flat nodes by Engine1D.hessvec on a context of its own: the product of the restatement, usable
    where a helper expects a dense block (`blk @ v`)."""

    def __init__(self, pr, nodes, opt=None):
        self.pr, self.nodes, self.opt, self.eng = pr, nodes, opt or pr.opt, pr.context(1)

    def __matmul__(self, v):
        pr = self.pr
        h = np.zeros(pr.u.size)
        h[self.nodes] = v
        return self.eng.hessvec(h.reshape((1,) + pr.shape), pr.t, self.opt, **pr.kw())["hv"][0].ravel()[self.nodes]

    def close(self):
        self.eng.close()


def _ref_dev(ref, Df, radius):
    direct = float(np.sqrt(np.sum((1.0 if Df is None else Df) * ref["x"] ** 2)))
    return max(abs(direct - radius), abs(ref["xnorm"] - radius), abs(direct - ref["xnorm"])) / radius


# ---------------------------------------------------------------------------------------------------------------------
# C. boundary exits at steps 1 and 3 on the eight-chunk grid at batch 3
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
def test_boundary_exits_at_steps_one_and_three_on_the_eight_chunk_grid(grid, precond):
    pr, nb, k = grid, 3, 5
    b = _q0((nb,) + pr.shape, 48)
    mask = (np.abs(pr.u) > 1e-8) & (np.abs(pr.u) < 1.0 - 1e-8)      # uploaded, so that the restatement has the same nodes
    nodes = np.flatnonzero(mask.ravel())
    masks = _tile(mask, nb)
    Df = _mass(pr).ravel()[nodes] if precond else None
    ones = np.ones(len(nodes), dtype=bool)
    bf = [b[i].ravel()[nodes] for i in range(nb)]
    op = _Product(pr, nodes)
    radius = np.array([np.inf, _radius_for_exit_at(op, bf[1], 1, Df), _radius_for_exit_at(op, bf[2], 3, Df)])
    refs = [steihaug(op.__matmul__, ones, bf[i], k, radius[i], 1e-30, Df) for i in range(nb)]
    plain = refs[0] if not precond else steihaug(op.__matmul__, ones, bf[0], k, np.inf, 1e-30, None)
    op.close()
    assert (plain["curv"] > 0).all()
    cond_lb = float(plain["curv"].max() / plain["curv"].min())
    eng = pr.context(nb)
    want = _cg(pr, eng, k, nb=nb, rhs=b, cg_tol=1e-30, precond=precond, mask=masks)
    Vw = _vectors(eng)
    many = _tr(pr, eng, k, radius, nb=nb, rhs=b, cg_tol=1e-30, precond=precond, mask=masks)
    Vm = _vectors(eng)
    eng.close()
    print(f"MEASURE grid batch 3 precond {precond}: status {list(many['status'])} steps {list(many['steps'])} restatement "
          f"{[r['status'] for r in refs]} {[r['steps'] for r in refs]} radius {radius.tolist()} n_free {list(many['n_free'])} "
          f"cond >= {cond_lb:.3g}")
    assert [r["status"] for r in refs] == [LIMIT, BOUNDARY, BOUNDARY] and [r["steps"] for r in refs] == [5, 1, 3]
    assert list(many["status"]) == [LIMIT, BOUNDARY, BOUNDARY] and list(many["steps"]) == [5, 1, 3]
    assert (many["n_free"] == len(nodes)).all() and len(nodes) > 2 * 4096           # more than two chunks of free nodes
    # member 0, radius = +inf, is the hess_cg run
    for key in CG_KEYS:
        assert np.array_equal(many[key][0], want[key][0], equal_nan=True), key
    for w, a, c in zip("xrp", Vm, Vw):
        assert np.array_equal(a[0], c[0]), w
    # every member is a single context
    for i in range(nb):
        one = pr.context(1)
        got = _tr(pr, one, k, radius[i], nb=1, rhs=b[i][None], cg_tol=1e-30, precond=precond, mask=mask[None])
        for key in TR_KEYS:
            assert np.array_equal(got[key][0], many[key][i], equal_nan=True), (key, i)
        for w, vm in zip("xrp", Vm):
            assert np.array_equal(one.cg_vector(w)[0], vm[i]), (w, i)
        one.close()
    # the boundary and r = P b - P H P x
    hx = pr.hessvec(Vm[0])
    for i in (1, 2):
        X, Rr = Vm[0][i], Vm[1][i]
        ref_dev = _ref_dev(refs[i], Df, radius[i])
        dev = max(abs(_dnorm(pr, X, precond) - radius[i]), abs(many["xnorm"][i] - radius[i])) / radius[i]
        d_r = np.abs(Rr - np.where(mask, b[i] - hx[i], 0.0)).max() / np.linalg.norm(bf[i])
        print(f"MEASURE grid batch 3 precond {precond} member {i}: | ||x||_D - radius | / radius {dev / EPS:.2f} eps, restatement "
              f"{ref_dev / EPS:.2f} eps; r identity {d_r:.2e} (bound {HV_TOL[2][1] * cond_lb:.2e})")
        assert not X[~mask].any() and not Rr[~mask].any() and np.isfinite(X).all()
        assert dev <= 10 * max(ref_dev, EPS)
        assert d_r <= HV_TOL[2][1] * cond_lb


# ---------------------------------------------------------------------------------------------------------------------
# C. the rounds off one block: depths 1 and 2, two and three chunks
# ---------------------------------------------------------------------------------------------------------------------
def _resident(pr, name):
    """The problem of `small(name)` with what _pgd and _box_cut read: the start state of the march and a configuration."""
    q = copy.copy(pr)
    q.phi0 = _problem(pr.V, name)["phi0"][0]
    q.ocfg = pr.V.module("Vch_control_1D.config").OptimizationConfig()
    return q


def _host_rounds(q, opt, u0, n_rounds, radius0, radius_max, radius_min, k=50, cg_tol=1e-8):
    """The loop of GD_1D.trust_refine on the problem `q` (tests/_trust_ref.host_rounds over the calls of Engine1D)."""
    eng = q.context(1)
    pq, pt = q.phi_Q[None], q.phi_T[None]

    def full_cost(v):
        phi, _ = eng.forward(q.phi0[None], q.dts, u=v[None], store=True)
        return float(np.atleast_2d(eng.cost(phi.reshape((1,) + q.shape), v[None], pq, pt, q.x, q.t, opt))[0, 4])

    out = host_rounds(lambda u: eng.forward(q.phi0[None], q.dts, u=np.ascontiguousarray(u[None]), store=False),
                      lambda u, radius: eng.hess_cg_trust(k, radius, q.t, opt, cg_tol=cg_tol, u=np.ascontiguousarray(u[None]), phi_Q=pq,
                                                          phi_T=pt, dt=q.dts, x=q.x),
                      lambda: eng.newton_trial(1.0)["u"][0], full_cost, u0, n_rounds, radius0, radius_max, radius_min)
    eng.close()
    return out


@pytest.mark.parametrize("name", ["n1030", "n2051"])
def test_rounds_off_one_block(small, name):
    q = _resident(small(name), name)
    S1 = q.V.module("Vch_control_1D.second_order_conditions")
    opts, u0, radius0 = off_block_members(q, _box_cut, _dnorm)
    n_rounds = 3
    lim = dict(radius_max=1024.0 * float(radius0.max()), radius_min=1e-10 * float(radius0.min()))
    eng = _pgd(q, opts, u0)
    many = eng.pgd_trust(n_rounds, radius0, **lim)
    Um, Pm = eng.pgd_get("u"), eng.pgd_get("phi")
    eng.close()
    print(f"MEASURE rounds {name}: status {many['status'].tolist()} cg {many['cg_status'].tolist()} in {many['cg_steps'].tolist()} n_free "
          f"{many['n_free'].tolist()} radius {many['radius'].tolist()} ratio {many['ratio'].tolist()} clipped {many['clipped'].tolist()} "
          f"cost {many['cost'].tolist()} -> {many['cost_new'].tolist()}")
    rows, n = q.shape
    assert many["rounds"] == n_rounds and (many["status"] != IDLE).all()
    assert many["cg_status"][0, 0] == BOUNDARY and many["status"][0, 0] == ACCEPTED
    assert many["cg_status"][1, 0] == NEGCURV and many["cg_steps"][1, 0] >= 1
    assert many["status"][2, 0] == REJECTED and many["clipped"][2, 0] == rows * n and many["n_free"][2, 0] == (rows - 1) * n
    assert (many["n_free"][:2, 0] > 4096).all()                     # the free set spans more than one chunk
    worst = dict(cost=0.0, cost_new=0.0, control=0.0)
    rel = lambda a, b: abs(a - b) / abs(b)
    for i in range(3):
        # a context of its own
        one = _pgd(q, [opts[i]], u0[i][None])
        got = one.pgd_trust(n_rounds, radius0[i], **lim)
        U1, P1 = one.pgd_get("u"), one.pgd_get("phi")
        one.close()
        for key in OUT_KEYS:
            assert np.array_equal(got[key][0], many[key][i], equal_nan=True), (key, i)
        assert np.array_equal(U1, Um[i]) and np.array_equal(P1, Pm[i]), i
        # the host loop
        uh, host = _host_rounds(q, opts[i], u0[i], n_rounds, radius0[i], **lim)
        assert len(host) == n_rounds
        for r, h in enumerate(host):
            print(f"MEASURE rounds {name} member {i} round {r}: host {h}")
            assert (h["status"], h["cg_status"], h["n_free"]) == (many["status"][i, r], many["cg_status"][i, r], many["n_free"][i, r]), (i, r)
            assert abs(h["steps"] - many["cg_steps"][i, r]) <= 1, (i, r)
            for key in ("cost", "cost_new"):
                worst[key] = max(worst[key], rel(many[key][i, r], h[key]))
        worst["control"] = max(worst["control"], float(np.abs(Um[i] - uh).max() / np.abs(uh).max()))
        # an accepted round's control is clip(u + x) with the kink rule, from the step alone
        acc = np.flatnonzero(many["status"][i] == ACCEPTED)
        if len(acc):
            r = int(acc[0])                                             # the rounds before it moved nothing
            one = _pgd(q, [opts[i]], u0[i][None])
            R = one.RESIDENT
            S = one.hess_cg_trust(50, many["radius"][i, r], q.t, opts[i], cg_tol=1e-8, u=R, phi_Q=R, phi_T=R, dt=q.dts, x=q.x)
            X = one.cg_vector("x")[0]
            assert S["xnorm"][0] == many["xnorm"][i, r] and S["status"][0] == many["cg_status"][i, r]
            one.pgd_trust(r + 1, radius0[i], **lim)
            U1 = one.pgd_get("u")
            one.close()
            lo, hi = opts[i].u_min, opts[i].u_max
            t = np.clip(u0[i] + X, lo, hi)
            t[S1.free_set(u0[i], lo, hi) & (t * u0[i] < 0.0)] = 0.0
            assert np.array_equal(U1.view(np.int64), t.view(np.int64)), i
            assert not np.array_equal(t, u0[i])
    print(f"MEASURE rounds {name} against the host loop: {worst}")
    for key in worst:
        assert worst[key] <= TOL[key], (key, worst[key])


# ---------------------------------------------------------------------------------------------------------------------
# D. radii at the ends of the double range
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
def test_radii_at_the_ends_of_the_double_range(driver, precond):
    """radius^2 not finite (2^600): no boundary, the call is the radius = +inf call.  radius^2 finite (2^500): the direction of
    negative curvature is followed to the boundary.  radius^2 = 0 (2^-600): tau = 0, a zero step, on the negative-definite
    block (NEGCURV, the restatement's exit there) and on the positive-definite one (BOUNDARY)."""
    pr = driver
    mask = pr.mask.copy()
    mask[0] = False                                                  # the negative-definite block of test_gpu_trust_1d.py
    nodes = np.flatnonzero(mask.ravel())
    opt = pr.V.make_opt(pr.opt, b3=_negative_b3(pr))
    b = _q0(pr.shape, 26)
    radii = dict(inf=np.inf, big=2.0 ** 600, mid=2.0 ** 500, tiny=2.0 ** -600)
    eng = pr.context(1)
    out = {}
    for key, radius in radii.items():
        R = _tr(pr, eng, 5, radius, rhs=b, precond=precond, mask=mask, opt=opt)
        out[key] = (R, [v[0] for v in _vectors(eng)])
    Rp = _tr(pr, eng, 5, radii["tiny"], rhs=b, precond=precond, mask=pr.mask)
    Xp, Rrp, Pp = (v[0] for v in _vectors(eng))
    eng.close()
    refs = {key: _driven(pr, nodes, b, 5, radii[key], 0.0, precond, opt=opt) for key in ("big", "mid", "tiny")}
    refp = _driven(pr, pr.free, b, 5, radii["tiny"], 0.0, precond)
    for key, (R, _) in out.items():
        print(f"MEASURE extremes precond {precond} {key}: status {R['status'][0]} steps {R['steps'][0]} xnorm {R['xnorm'][0]:.17g} "
              f"pred {R['pred'][0]:.6e}")
    # 2^600 is the radius = +inf call
    Ri, Vi = out["inf"]
    Rb, Vb = out["big"]
    assert Ri["status"][0] == NEGCURV and Ri["steps"][0] == 0 and not Vi[0].any() and Ri["pred"][0] == 0.0 and Ri["xnorm"][0] == 0.0
    assert refs["big"]["status"] == NEGCURV and refs["big"]["steps"] == 0 and not refs["big"]["x"].any()
    for key in TR_KEYS:
        assert np.array_equal(Rb[key], Ri[key], equal_nan=True), key
    for w, a, c in zip("xrp", Vb, Vi):
        assert np.array_equal(a, c), w
    # 2^500 steps to the boundary
    Rm, (X, _, _) = out["mid"]
    dev = abs(Rm["xnorm"][0] - radii["mid"]) / radii["mid"]
    direct = abs(_dnorm(pr, X, precond) - radii["mid"]) / radii["mid"]
    print(f"MEASURE extremes precond {precond} 2^500: xnorm {dev / EPS:.2f} eps, ||x||_D from x {direct / EPS:.2f} eps off the radius; "
          f"restatement {abs(refs['mid']['xnorm'] - radii['mid']) / radii['mid'] / EPS:.2f} eps")
    assert refs["mid"]["status"] == NEGCURV and refs["mid"]["steps"] == 1
    assert Rm["status"][0] == NEGCURV and Rm["steps"][0] == 1 and np.isfinite(X).all() and np.isfinite(Rm["pred"][0]) and Rm["pred"][0] > 0
    assert dev <= 10 * EPS and direct <= (len(nodes) + 8) * EPS
    # 2^-600: a zero step
    for what, R, (X, Rr, Pd), ref, m, status in (("negative definite", out["tiny"][0], out["tiny"][1], refs["tiny"], mask, NEGCURV),
                                                   ("positive definite", Rp, (Xp, Rrp, Pp), refp, pr.mask, BOUNDARY)):
        assert ref["status"] == status and ref["steps"] == 1 and not ref["x"].any() and ref["pred"] == 0.0 and ref["resid"][0] == 1.0, what
        assert R["status"][0] == status and R["steps"][0] == 1, what
        assert not X.any() and np.array_equal(Rr, np.where(m, b, 0.0)), what
        assert np.isfinite(Pd).all() and Pd[m].any() and R["pred"][0] == 0.0 and R["xnorm"][0] == 0.0, what
        assert abs(R["resid"][0, 0] - 1.0) <= len(nodes) * EPS, what          # two sums of the same squares, in another order
        assert np.isfinite(R["curv"][0, 0]) and np.isfinite(R["rnorm0"][0]), what


# ---------------------------------------------------------------------------------------------------------------------
# E. scale equivariance: no absolute threshold in the scalar kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("kind", ["boundary", "interior"])
@pytest.mark.parametrize("name", ["driver", "n2051"])
def test_the_step_is_scale_equivariant_bit_for_bit(request, small, name, kind, precond):
    """rhs and radius times 2^+-40: x, r, p, rnorm0 and xnorm scale by it, pred by its square, steps, status, resid and curv
    stay, all exactly (the products are direct solves, linear in the bits; the restatement has the property on the CPU)."""
    pr = request.getfixturevalue("driver") if name == "driver" else small(name)
    blk = _block(pr)
    b = _q0(pr.shape, 47)
    bf = b.ravel()[pr.free]
    D = _mass(pr).ravel()[pr.free] if precond else np.ones(len(pr.free))
    if kind == "boundary":
        radius = _radius_for_exit_at(blk, bf, 3, D if precond else None)
    else:
        xs = np.linalg.solve(blk, bf)
        radius = 10.0 * float(np.sqrt(np.sum(D * xs * xs)))
    k = 4 * len(pr.free)
    eng = pr.context(1)
    runs = []
    for s in (1.0, 2.0 ** 40, 2.0 ** -40):
        R = _tr(pr, eng, k, s * radius, rhs=s * b, cg_tol=1e-8, precond=precond, mask=pr.mask)
        runs.append((s, R, _vectors(eng)))
    eng.close()
    _, R0, V0 = runs[0]
    print(f"MEASURE scale {name} {kind} precond {precond}: status {R0['status'][0]} steps {R0['steps'][0]} xnorm / radius "
          f"{R0['xnorm'][0] / radius:.6f}")
    if kind == "boundary":
        assert R0["status"][0] == BOUNDARY and R0["steps"][0] == 3
    else:
        assert R0["status"][0] == CONVERGED and R0["xnorm"][0] < radius and R0["steps"][0] >= 3
    for s, R, Vs in runs[1:]:
        for key in ("steps", "status", "n_free", "resid", "curv"):
            assert np.array_equal(R[key], R0[key], equal_nan=True), (key, s)
        for key in ("rnorm0", "xnorm"):
            assert np.array_equal(R[key], s * R0[key]), (key, s)
        assert np.array_equal(R["pred"], (s * s) * R0["pred"]), s
        for w, a, c in zip("xrp", Vs, V0):
            assert np.array_equal(a, s * c), (w, s)
