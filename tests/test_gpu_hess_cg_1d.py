"""vch1d_hess_cg / vch1d_cg_vector on the GPU: (preconditioned) conjugate gradients on the reduced Hessian P H P of the 1D
engine with x, r, p, the free set and the recurrence in device memory, against dense masked Hessians
assembled from Engine1D.hessvec on a second context, against np.linalg.solve of their blocks and against the NumPy
restatement of the iteration (tests/_cg_ref.py, pinned by test_cg_ref_cpu.py and test_cg_ref_1d_cpu.py) with the same
D = diag(wt'_k wx_i), wt'_0 := wt_1.  The problems are those of test_gpu_krylov_1d.py: `driver` (N = 32, 5 steps, 231 nodes,
172 free, mask built on the device) and the `small` cases n33_off / n1030 / n2051 (uploaded 12-node masks at cyclic-
reduction depths 0 / 1 / 2 with one, two and three streaming chunks).

Tolerances (none tuned against the code under test).
    solve        x and d against np.linalg.solve of the block: relative inf-norm error <= cond(block) 1.2e-8 at
                 cg_tol = 1e-8 (the residual bound times the condition number, with the 20 % margin of DESIGN.md 10g);
                 the true residual recomputed with hessvec <= 1.2e-8.
    restatement  the first four resid (absolute), curv (of the largest) and pred (relative), and the pred identities
                 pred = b.x - x.Hx / 2 and b.x = x.Hx (of sum |b||x|): HV_TOL[depth] of test_gpu_hessvec_1d.TOL times
                 cond(block).  b.x = x.Hx says that r is orthogonal to every earlier direction, which conjugate gradients
                 lose in floating point over tens of steps (measured at convergence, 65 and 57 steps: 6.3e-10 and 1.1e-10
                 on the device, 3.0e-10 and 7.1e-10 for the restatement on the dense block); the identities are asserted
                 at that tolerance after four steps, the pred identity at convergence too, and b.x = x.Hx at convergence
                 at what the stop rule guarantees, |x.r| <= 1.2e-8 ||x|| ||P b||.
    three nodes  x against the 3 x 3 solve: 10 n eps cond.
    Newton rhs   rnorm0 against the host-built norm: HV_TOL[0]'s gradient tolerance (1.5e-14) times the ratio of the
                 gradient's size to the right-hand side's on the free set (the two are subtracted).
    bits         exact.
    steps        within +-1 of the restatement on the dense block where cond(block) <= 100; elsewhere within +-1 of the
                 restatement driven by Engine1D.hessvec on a second context as its product (on an
                 ill-conditioned block the count follows the product's rounding)."""
import ctypes as C

import numpy as np
import pytest

from oracle import vch1d_oracle as o
from _cg_ref import CONVERGED, LIMIT, NEGCURV, cg
from test_gpu_forms import _env
from test_gpu_hessvec_1d import TOL as HV_TOL
from test_gpu_krylov_1d import Problem, _mask_of, _q0, _tile, driver, small      # noqa: F401 (fixtures)
from test_gpu_second_order_1d import V, _engine                                   # noqa: F401 (V: fixture)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SOLVE = 1.2e-8
KEYS = ("steps", "status", "n_free", "resid", "curv", "pred", "rnorm0")


def _tw(t):
    """Trapezoid weights of the nodes t."""
    d = np.diff(np.asarray(t, dtype=np.float64))
    w = np.zeros(len(d) + 1)
    w[:-1] += 0.5 * d
    w[1:] += 0.5 * d
    return w


def _weights(pr):
    """wt (x) wx of the cost, in the shape of a control (row 0 is zero)."""
    return _tw(pr.t)[:, None] * _tw(pr.x)[None, :]


def _mass(pr):
    """D of vch1d_hess_cg: wt' (x) wx with wt'_0 := wt_1."""
    wt = _tw(pr.t)
    wt[0] = wt[1]
    return wt[:, None] * _tw(pr.x)[None, :]


def _block(pr, nodes=None):
    """The symmetrised block on the flat nodes (default: the problem's free set) from the problem's dense matrix or block."""
    if nodes is None:
        nodes = pr.free
    if hasattr(pr, "Hm"):
        return pr.Hm[np.ix_(nodes, nodes)]
    assert np.array_equal(nodes, pr.free)
    return pr.A


def _cg(pr, eng, k, nb=0, **kw):
    args = pr.kw(nb)
    args.update(kw)
    return eng.hess_cg(k, pr.t, args.pop("opt", pr.opt), **args)


def _ref(pr, blk, nodes, b, k, cg_tol, precond):
    """The restatement on the block of the free nodes."""
    Df = _mass(pr).ravel()[nodes]
    return cg(lambda v: blk @ v, np.ones(len(nodes), dtype=bool), b.ravel()[nodes], k, cg_tol, Df if precond else None)


def _driven(pr, nodes, b, k, cg_tol, precond, opt=None):
    """The restatement on the free nodes with Engine1D.hessvec (a context of its own) as its product."""
    eng = pr.context(1)

    def apply(v):
        h = np.zeros(pr.u.size)
        h[nodes] = v
        return eng.hessvec(h.reshape((1,) + pr.shape), pr.t, opt or pr.opt, **pr.kw())["hv"][0].ravel()[nodes]

    Df = _mass(pr).ravel()[nodes]
    out = cg(apply, np.ones(len(nodes), dtype=bool), b.ravel()[nodes], k, cg_tol, Df if precond else None)
    eng.close()
    return out


def _check_steps(pr, blk, nodes, b, k, cg_tol, precond, m, ref, what):
    """The step count within one of the restatement: on the dense block where it is well conditioned, else driven by hessvec."""
    cond = np.linalg.cond(blk)
    if cond <= 100:
        want = ref["steps"]
    else:
        want = _driven(pr, nodes, b, k, cg_tol, precond)["steps"]
    print(f"MEASURE {what}: steps {m}, restatement on the block {ref['steps']}, cond {cond:.3g}, asserted against {want}")
    assert abs(m - want) <= 1


# ---------------------------------------------------------------------------------------------------------------------
# 1. the solve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
def test_driver_solve_with_the_free_set_built_on_the_device(driver, precond):
    pr = driver
    blk, n = _block(pr), len(pr.free)
    b = _q0(pr.shape, 21)
    bf = b.ravel()[pr.free]
    ev = np.linalg.eigvalsh(blk)
    cond = ev[-1] / ev[0]
    k = 4 * n
    eng = pr.context(1)
    R = _cg(pr, eng, k, rhs=b, cg_tol=1e-8, precond=precond)
    X, Rr = eng.cg_vector("x")[0], eng.cg_vector("r")[0]
    eng.close()
    m = int(R["steps"][0])
    want = np.linalg.solve(blk, bf)
    xf = X.ravel()[pr.free]
    err = np.abs(xf - want).max() / np.abs(want).max()
    hx = pr.hessvec(X[None])[0]
    true = np.linalg.norm(np.where(pr.mask, b - hx, 0.0)) / np.linalg.norm(bf)
    ref = _ref(pr, blk, pr.free, b, k, 1e-8, precond)
    print(f"MEASURE driver precond {precond}: steps {m} recurrence {R['resid'][0, m - 1]:.2e} true residual {true:.2e} cond {cond:.3g} "
          f"error {err:.2e} stats {R['stats']}")
    assert R["status"][0] == CONVERGED and R["n_free"][0] == n == 172
    assert all(np.isfinite(R[key][0]).all() for key in ("pred", "rnorm0")) and np.isfinite(X).all() and np.isfinite(Rr).all()
    assert R["resid"][0, m - 1] <= 1e-8 and np.isnan(R["resid"][0, m:]).all() and np.isnan(R["curv"][0, m:]).all()
    assert not X[~pr.mask].any() and not Rr[~pr.mask].any() and np.abs(X).max() > 0
    assert abs(R["rnorm0"][0] - np.linalg.norm(bf)) <= 4 * EPS * np.linalg.norm(bf)
    assert true <= SOLVE
    assert err <= cond * SOLVE
    assert R["stats"]["linear_solves"] == pr.M * (2 * m + 1) and R["stats"]["host_syncs"] == 2, R["stats"]
    _check_steps(pr, blk, pr.free, b, k, 1e-8, precond, m, ref, f"driver precond {precond}")


@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("name", ["n33_off", "n1030", "n2051"])
def test_depths_and_chunks_with_an_uploaded_mask(small, name, precond):
    pr = small(name)
    blk, n = pr.A, len(pr.free)
    b = _q0(pr.shape, 22)
    bf = b.ravel()[pr.free]
    cond = np.linalg.cond(blk)
    k = 4 * n
    eng = pr.context(1)
    R = _cg(pr, eng, k, rhs=b, cg_tol=1e-8, precond=precond, mask=pr.mask)
    X = eng.cg_vector("x")[0]
    eng.close()
    m = int(R["steps"][0])
    want = np.linalg.solve(blk, bf)
    err = np.abs(X.ravel()[pr.free] - want).max() / np.abs(want).max()
    ref = _ref(pr, blk, pr.free, b, k, 1e-8, precond)
    print(f"MEASURE {name} precond {precond}: steps {m} cond {cond:.3g} error {err:.2e}")
    assert R["status"][0] == CONVERGED and R["n_free"][0] == n == 12
    assert not X[~pr.mask].any() and np.isfinite(X).all()
    assert err <= cond * SOLVE
    assert R["stats"]["linear_solves"] == pr.M * (2 * m + 1), R["stats"]
    _check_steps(pr, blk, pr.free, b, k, 1e-8, precond, m, ref, f"{name} precond {precond}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the CPU restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("name", ["driver", "n33_off", "n1030", "n2051"])
def test_first_steps_agree_with_the_cpu_restatement(request, small, name, precond):
    pr = request.getfixturevalue("driver") if name == "driver" else small(name)
    depth = getattr(pr, "depth", 0)
    blk = _block(pr)
    b = _q0(pr.shape, 23)
    eng = pr.context(1)
    R = _cg(pr, eng, 4, rhs=b, cg_tol=1e-30, precond=precond, mask=pr.mask)
    eng.close()
    ref = _ref(pr, blk, pr.free, b, 4, 1e-30, precond)
    tol = HV_TOL[depth][1] * np.linalg.cond(blk)
    assert R["steps"][0] == ref["steps"] == 4 and R["status"][0] == ref["status"] == LIMIT
    d_res = np.abs(R["resid"][0] - ref["resid"]).max()
    d_curv = np.abs(R["curv"][0] - ref["curv"]).max() / np.abs(ref["curv"]).max()
    d_pred = abs(R["pred"][0] - ref["pred"]) / abs(ref["pred"])
    print(f"MEASURE cpu restatement {name} precond {precond}: first 4 resid {d_res:.2e} curv {d_curv:.2e} pred {d_pred:.2e} (bound {tol:.2e})")
    assert d_res <= tol and d_curv <= tol and d_pred <= tol


# ---------------------------------------------------------------------------------------------------------------------
# 3. three free nodes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
def test_three_free_nodes(driver, precond):
    pr = driver
    nodes = pr.free[[4, 77, 150]]
    mask, b = _mask_of(pr.shape, nodes), _q0(pr.shape, 24)
    eng = pr.context(1)
    R = _cg(pr, eng, 12, rhs=b, precond=precond, mask=mask)
    X = eng.cg_vector("x")[0]
    eng.close()
    blk = pr.Hm[np.ix_(nodes, nodes)]
    want = np.linalg.solve(blk, b.ravel()[nodes])
    err = np.abs(X.ravel()[nodes] - want).max() / np.abs(want).max()
    cond = np.linalg.cond(blk)
    print(f"MEASURE three nodes precond {precond}: steps {R['steps'][0]} error {err:.2e} cond {cond:.3g}")
    assert R["status"][0] == CONVERGED and R["n_free"][0] == 3 and R["steps"][0] == 3
    assert not X[~mask].any()
    assert err <= 10 * 3 * EPS * cond


# ---------------------------------------------------------------------------------------------------------------------
# 4. the Newton right-hand side
# ---------------------------------------------------------------------------------------------------------------------
def test_newton_right_hand_side_with_per_trajectory_kappa_b3_and_box(driver):
    pr, V = driver, driver.V
    W, S1 = _weights(pr), driver.S1
    opts = [V.make_opt(pr.opt, kappa_sparsity=ks, b3=b3, u_min=lo, u_max=hi)
            for ks, b3, lo, hi in ((1e-4, 1e-4, -1.0, 1.0), (3e-3, 2.5e-4, -0.8, 0.9))]
    eng = pr.context(2)
    R = _cg(pr, eng, 4 * 172, nb=2, opt=opts, cg_tol=1e-8)
    X, Rr = eng.cg_vector("x"), eng.cg_vector("r")
    R4 = _cg(pr, eng, 4, nb=2, opt=opts, cg_tol=1e-30)              # four steps of the same iteration, for the identities
    X4 = eng.cg_vector("x")
    eng.close()
    other = pr.context(2)
    G = other.exact_gradient(pr.t, opts, **pr.kw(2))
    hx = other.hessvec(X, pr.t, opts, **pr.kw(2))["hv"]
    hx4 = other.hessvec(X4, pr.t, opts, **pr.kw(2))["hv"]
    other.close()
    assert list(R4["steps"]) == [4, 4] and np.array_equal(R4["rnorm0"], R["rnorm0"]) and np.array_equal(R4["resid"], R["resid"][:, :4])
    assert R["stats"]["host_syncs"] == 2
    for i, op in enumerate(opts):
        mask = S1.free_set(pr.u, op.u_min, op.u_max)
        free = np.flatnonzero(mask.ravel())
        bb = np.where(mask, -(G[i] + op.kappa_sparsity * W * np.sign(pr.u)), 0.0)
        nb_, ng = np.linalg.norm(bb), np.linalg.norm(np.where(mask, G[i], 0.0))
        dev = abs(R["rnorm0"][i] - nb_) / nb_
        blk = pr.Hm[np.ix_(free, free)] + (op.b3 - pr.opt.b3) * np.diag(W.ravel()[free])
        cond = np.linalg.cond(blk)
        want = np.linalg.solve(blk, bb.ravel()[free])
        err = np.abs(X[i].ravel()[free] - want).max() / np.abs(want).max()
        # pred = b.x - x.Hx / 2 and b.x = x.Hx (x.r = 0: r is orthogonal to every earlier direction) hold for every CG
        # iterate in exact arithmetic.  After four steps they hold to the product's accuracy and are asserted at the hessvec
        # tolerance times cond.  A run of tens of steps loses the orthogonality to its early directions, as conjugate
        # gradients do in floating point (the restatement on the dense block is printed beside the device); there
        # |x.r| <= ||x|| ||r|| <= cg_tol ||x|| ||P b|| is what the stop rule guarantees, and that is asserted.
        tol = HV_TOL[0][1] * cond
        ident = {}
        for name, xx, hh, pred in (("4 steps", X4[i], hx4[i], R4["pred"][i]), ("converged", X[i], hx[i], R["pred"][i])):
            bx = float(np.sum(bb * xx))
            xhx = float(np.sum(xx * np.where(mask, hh, 0.0)))
            scale = float(np.sum(np.abs(bb) * np.abs(xx)))
            ident[name] = (abs(pred - (bx - 0.5 * xhx)) / scale, abs(bx - xhx) / scale, abs(bx - xhx), scale)
        ref = cg(lambda v: blk @ v, np.ones(len(free), dtype=bool), bb.ravel()[free], 4 * 172, 1e-8, _mass(pr).ravel()[free])
        xr = ref["x"]
        ref_dev = abs(bb.ravel()[free] @ xr - xr @ (blk @ xr)) / float(np.abs(bb.ravel()[free]) @ np.abs(xr))
        print(f"MEASURE newton rhs {i}: n_free {R['n_free'][i]} rnorm0 dev {dev:.2e} (kappa's share {abs(nb_ - ng) / ng:.1e}) steps {R['steps'][i]} "
              f"(restatement {ref['steps']}) error {err:.2e} cond {cond:.3g}; pred dev / b.x - x.Hx after 4 steps {ident['4 steps'][0]:.2e} / "
              f"{ident['4 steps'][1]:.2e} (bound {tol:.2e}), converged {ident['converged'][0]:.2e} / {ident['converged'][1]:.2e} "
              f"(the restatement's own b.x - x.Ax {ref_dev:.2e})")
        assert R["status"][i] == CONVERGED and R["n_free"][i] == len(free)
        assert mask[0].any() and np.abs(G[i][0][mask[0]]).min() > 0
        assert dev <= HV_TOL[0][0] * max(1.0, ng / nb_)
        assert err <= cond * SOLVE
        assert not X[i][~mask].any() and not Rr[i][~mask].any() and not X4[i][~mask].any()
        assert ident["4 steps"][0] <= tol and ident["4 steps"][1] <= tol
        assert ident["converged"][0] <= tol
        assert ident["converged"][2] <= SOLVE * np.linalg.norm(X[i]) * nb_


def test_newton_right_hand_side_on_row_zero(driver):
    """r before any step is P b: a b3 so negative that the first direction has negative curvature leaves it untouched.  On
    row 0 wt = 0, so the sign term has no weight there and r[0] = -P grad[0], which does not vanish: row 0 drives step 0."""
    pr, V = driver, driver.V
    op = V.make_opt(pr.opt, b3=_negative_b3(pr), kappa_sparsity=0.5)
    eng = pr.context(1)
    R = _cg(pr, eng, 1, opt=op)
    r, x = eng.cg_vector("r")[0], eng.cg_vector("x")[0]
    G = eng.exact_gradient(pr.t, op, **pr.kw())[0]
    eng.close()
    assert R["status"][0] == NEGCURV and R["steps"][0] == 0 and not x.any()
    bb = np.where(pr.mask, -(G + op.kappa_sparsity * _weights(pr) * np.sign(pr.u)), 0.0)
    scale = np.abs(G).max()
    dev0 = np.abs(r[0] + np.where(pr.mask[0], G[0], 0.0)).max() / scale
    dev = np.abs(r - bb).max() / scale
    share = np.abs(op.kappa_sparsity * _weights(pr)[1:]).max() / scale
    print(f"MEASURE newton rhs row 0: r[0] + P grad[0] {dev0:.2e}, r - P b {dev:.2e} of max |grad|; the sign term's share on rows >= 1 {share:.1e}")
    assert pr.mask[0].any() and np.abs(G[0][pr.mask[0]]).min() > 0 and share > 1e-3
    assert dev0 <= HV_TOL[0][0] and dev <= HV_TOL[0][0]
    assert R["stats"]["linear_solves"] == pr.M * 3


# ---------------------------------------------------------------------------------------------------------------------
# 5. the preconditioner on row 0, negative curvature: H(b3') = H(b3) + (b3' - b3) diag(wt (x) wx), row 0 unshifted
# ---------------------------------------------------------------------------------------------------------------------
def _negative_b3(pr):
    """A b3 so negative that every node of a row >= 1 has curvature below -3 lambda_max(block)."""
    W = _weights(pr).ravel()[pr.free]
    lam = np.linalg.eigvalsh(_block(pr))[-1]
    return pr.opt.b3 - 4.0 * lam / W[W > 0].min()


def test_preconditioner_on_row_zero(driver):
    pr, V = driver, driver.V
    assert pr.mask[0].any()                                          # free nodes on row 0, where wt = 0
    b, D = _q0(pr.shape, 25), _mass(pr)
    eng = pr.context(1)
    R = _cg(pr, eng, 1, rhs=b, precond=True, opt=V.make_opt(pr.opt, b3=_negative_b3(pr)))
    X, Pd = eng.cg_vector("x")[0], eng.cg_vector("p")[0]
    eng.close()
    want = np.where(pr.mask, b, 0.0) / D                            # D^-1 P b with wt'_0 = wt_1
    assert R["status"][0] == NEGCURV and R["steps"][0] == 0 and not X.any()
    assert np.isfinite(Pd).all() and np.isfinite(R["curv"][0, 0]) and np.isfinite(R["rnorm0"][0]) and R["pred"][0] == 0.0
    assert not Pd[~pr.mask].any() and np.abs(Pd[0]).max() > 0
    assert (np.abs(Pd - want) <= 4 * EPS * np.abs(want)).all()      # the product of two weights and a quotient
    assert R["stats"]["linear_solves"] == pr.M * 3                   # one product taken, no update


@pytest.mark.parametrize("precond", [False, True])
def test_negative_definite_exits_at_step_zero(driver, precond):
    pr, V = driver, driver.V
    mask = pr.mask.copy()
    mask[0] = False                                                  # row 0 is not shifted by b3: left out, the block is negative definite
    nodes = np.flatnonzero(mask.ravel())
    b3 = _negative_b3(pr)
    W, D = _weights(pr).ravel()[nodes], _mass(pr).ravel()[nodes]
    blk = pr.Hm[np.ix_(nodes, nodes)] + (b3 - pr.opt.b3) * np.diag(W)
    assert np.linalg.eigvalsh(blk)[-1] < 0
    b = _q0(pr.shape, 26)
    eng = pr.context(1)
    R = _cg(pr, eng, 5, rhs=b, precond=precond, mask=mask, opt=V.make_opt(pr.opt, b3=b3))
    X, Pd = eng.cg_vector("x")[0], eng.cg_vector("p")[0]
    eng.close()
    pf = Pd.ravel()[nodes]
    curv = (pf @ (blk @ pf)) / (pf @ ((D if precond else 1.0) * pf))
    dev = abs(R["curv"][0, 0] - curv) / abs(curv)
    print(f"MEASURE negative definite precond {precond}: curv {R['curv'][0, 0]:.6e} p.Ap / p.Dp {curv:.6e} dev {dev:.2e}")
    assert R["status"][0] == NEGCURV and R["steps"][0] == 0 and R["pred"][0] == 0.0 and not X.any()
    assert R["curv"][0, 0] < 0 and np.isnan(R["curv"][0, 1:]).all() and np.isnan(R["resid"][0]).all()
    assert dev <= HV_TOL[0][1] * np.linalg.cond(blk)


# ---------------------------------------------------------------------------------------------------------------------
# 6. a batch of three against three single contexts; a shared base against the tiled one
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_of_three_equals_three_single_contexts(driver):
    pr = driver
    masks = np.stack([_mask_of(pr.shape, pr.free[[4, 77, 150]]), _mask_of(pr.shape, pr.free[[0, 20, 40, 90, 120, 160, 171]]), pr.mask])
    b = _q0((3,) + pr.shape, 27)
    k = 14
    eng = pr.context(3)
    many = _cg(pr, eng, k, nb=3, rhs=b, precond=False, mask=masks, cg_tol=1e-8)
    Vm = [eng.cg_vector(w) for w in "xrp"]
    eng.close()
    print(f"MEASURE batch: n_free {list(many['n_free'])} steps {list(many['steps'])} status {list(many['status'])}")
    assert list(many["n_free"]) == [3, 7, 172]
    assert many["status"][0] == CONVERGED and many["steps"][0] == 3
    assert many["status"][1] == CONVERGED and 3 < many["steps"][1] < k            # seven nodes: rounding may need steps beyond seven
    assert many["status"][2] == LIMIT and many["steps"][2] == k                   # 172 nodes go on
    assert many["stats"]["host_syncs"] == 2
    for i in range(3):
        eng = pr.context(1)
        one = _cg(pr, eng, k, rhs=b[i], precond=False, mask=masks[i], cg_tol=1e-8)
        for key in KEYS:
            assert np.array_equal(one[key][0], many[key][i], equal_nan=True), (key, i)
        for w, vm in zip("xrp", Vm):
            assert np.array_equal(eng.cg_vector(w)[0], vm[i]), (w, i)
        eng.close()


def test_shared_base_equals_the_tiled_base(driver):
    pr, V = driver, driver.V
    opts = [V.make_opt(pr.opt, u_min=-1.0, u_max=1.0, kappa_sparsity=1e-4), V.make_opt(pr.opt, u_min=-0.7, u_max=0.9, kappa_sparsity=2e-3)]
    out = []
    for nb in (0, 2):
        eng = pr.context(2)
        R = _cg(pr, eng, 5, nb=nb, opt=opts, cg_tol=1e-30)
        out.append((R, [eng.cg_vector(w) for w in "xrp"]))
        eng.close()
    (Ra, Va), (Rb, Vb) = out
    assert Ra["n_free"][0] == 172 and Ra["n_free"][1] < 172 and list(Ra["steps"]) == [5, 5]
    for key in KEYS:
        assert np.array_equal(Ra[key], Rb[key], equal_nan=True), key
    for a, b in zip(Va, Vb):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the cached gradient sweep: bits, solve counts, looks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("newton", [False, True])
def test_cached_sweep_has_the_bits_of_the_repeated_one_and_the_counts(driver, newton):
    pr = driver
    k, B = 3, 2
    rhs = None if newton else _q0((2,) + pr.shape, 28)
    eng = pr.context(B)
    got = _cg(pr, eng, k, nb=B, rhs=rhs, cg_tol=1e-30)
    Xg = [eng.cg_vector(w) for w in "xrp"]
    longer = _cg(pr, eng, 6, nb=B, rhs=rhs, cg_tol=1e-30)
    eng.close()
    with _env(VCH_KRYLOV_NOCACHE=1):
        eng = pr.context(B)
    ref = _cg(pr, eng, k, nb=B, rhs=rhs, cg_tol=1e-30)
    Xr = [eng.cg_vector(w) for w in "xrp"]
    eng.close()
    for key in KEYS:
        assert np.array_equal(got[key], ref[key], equal_nan=True), key
    for a, b in zip(Xg, Xr):
        assert np.array_equal(a, b)
    assert list(got["steps"]) == [k, k] and list(got["status"]) == [LIMIT, LIMIT]
    assert got["stats"]["linear_solves"] == B * pr.M * (2 * k + 1), got["stats"]
    assert ref["stats"]["linear_solves"] == 3 * B * pr.M * k + (B * pr.M if newton else 0), ref["stats"]
    assert got["stats"]["host_syncs"] == longer["stats"]["host_syncs"] == ref["stats"]["host_syncs"] == 2      # no look between the steps
    assert longer["stats"]["launches"] > got["stats"]["launches"] and got["stats"]["seconds"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. state: what either Krylov call leaves for the other's fetch; about a PGD iterate
# ---------------------------------------------------------------------------------------------------------------------
def test_either_call_invalidates_what_the_other_left(driver):
    pr, V = driver, driver.V
    b = _q0(pr.shape, 29)
    eng = pr.context(1)
    with pytest.raises(V.VchError, match="-3"):          # nothing resident before any call
        eng.cg_vector("x")
    pr.lanczos(eng, b, 3)
    eng.krylov_vector(np.ones((1, 1)))
    with pytest.raises(V.VchError, match="-3"):          # a Lanczos basis is no x
        eng.cg_vector("x")
    R = _cg(pr, eng, 3, rhs=b, cg_tol=1e-30)
    X = eng.cg_vector("x")
    with pytest.raises(V.VchError, match="-3"):          # the Lanczos basis is gone
        eng.krylov_vector(np.ones((1, 1)))
    pr.lanczos(eng, b, 2, reorth=False)
    with pytest.raises(V.VchError, match="-3"):          # and so are x, r, p after a Lanczos run
        eng.cg_vector("x")
    again = _cg(pr, eng, 3, rhs=b, cg_tol=1e-30)
    assert np.array_equal(eng.cg_vector("x"), X)
    with pytest.raises(ValueError):
        eng.cg_vector("q")
    eng.close()
    for key in KEYS:
        assert np.array_equal(again[key], R[key], equal_nan=True), key


def test_pgd_iterate_free_set_from_the_resident_control_and_an_undisturbed_run(V):
    S1 = V.module("Vch_control_1D.second_order_conditions")
    N, T, dt = 32, 0.05, 0.01
    P = o.Params1D(N=N, T=T, dt_initial=dt)
    tg, dts = V.time_grid(T, dt)
    t = np.concatenate([[0.0], tg])
    x = np.linspace(0.0, 1.0, N + 1)
    phi0 = np.stack([0.2 * np.cos(np.pi * x + 0.4 * b) for b in range(2)])
    phi_T = np.stack([0.7 * np.sin(2 * np.pi * x), 0.5 * np.cos(2 * np.pi * x)])
    w = [dict(b1=0.3, b2=13.0, b3=0.0019, kappa_sparsity=9e-5, alpha_max=100.0),
         dict(b1=2.0, b2=4.0, b3=1e-3, kappa_sparsity=9e-5, alpha_max=100.0)]

    def start(opts):
        eng = _engine(V, P, 2)
        eng.pgd_init(phi0, phi_T, t, dts, opts)
        eng.pgd_iterate(2)
        return eng

    # the scale of the control under a wide box, then a box of its own per trajectory that pins part of the nodes
    probe = start([V.make_opt(u_min=-1e6, u_max=1e6, **w[0]), V.make_opt(u_min=-1e6, u_max=1e6, **w[1])])
    top = np.abs(probe.pgd_get("u")).reshape(2, -1).max(axis=1)
    probe.close()
    assert top.min() > 0
    opts = [V.make_opt(u_min=-0.5 * top[0], u_max=0.25 * top[0], **w[0]), V.make_opt(u_min=-0.1 * top[1], u_max=0.6 * top[1], **w[1])]
    plain = start(opts)
    want = plain.pgd_iterate(1)
    u_want = plain.pgd_get("u")
    plain.close()
    eng = start(opts)
    u, phi = eng.pgd_get("u"), eng.pgd_get("phi")
    R = eng.RESIDENT
    L = eng.hess_cg(3, t, opts, u=R, phi_Q=R, phi_T=R, dt=dts)
    nf = [int(S1.free_set(u[b], opts[b].u_min, opts[b].u_max).sum()) for b in range(2)]
    print(f"MEASURE pgd: n_free {list(L['n_free'])} of {u[0].size}, free_set() {nf}, steps {list(L['steps'])} status {list(L['status'])}")
    assert list(L["n_free"]) == nf and 0 < min(nf) and max(nf) < u[0].size
    X = eng.cg_vector("x")
    for b in range(2):
        assert not X[b][~S1.free_set(u[b], opts[b].u_min, opts[b].u_max)].any()
    assert np.array_equal(eng.pgd_get("u"), u) and np.array_equal(eng.pgd_get("phi"), phi)
    got = eng.pgd_iterate(1)
    for key in ("cost", "alpha", "trials", "change", "tracking_error", "terminal_error"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(eng.pgd_get("u"), u_want)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_any_launch_and_data_errors_name_the_trajectory(driver):
    pr, V = driver, driver.V
    lib = V.load()
    b = _q0((2,) + pr.shape, 30)
    eng = pr.context(2)
    first = _cg(pr, eng, 4, rhs=b, cg_tol=1e-30)
    X = eng.cg_vector("x")
    live = lib.vch_mem_live()
    t_bad = pr.t.copy()
    t_bad[3] = t_bad[2]                                  # rows 2 and 3 share a time: wt' stays positive, the step size does not
    t_flat = pr.t.copy()
    t_flat[2] = t_flat[1] = t_flat[0]                    # wt'_0 = wt_1 = 0
    for bad in (dict(k=0), dict(k=-3), dict(precond=2), dict(precond=-1), dict(cg_tol=np.nan), dict(cg_tol=np.inf), dict(u=None),
                dict(opt=[pr.opt, pr.opt, pr.opt])):
        args = dict(k=4, rhs=b, cg_tol=1e-30)
        args.update(bad)
        with pytest.raises(ValueError):
            _cg(pr, eng, args.pop("k"), **args)
        assert lib.vch_mem_live() == live, bad
        assert np.array_equal(eng.cg_vector("x"), X), bad                     # what was resident is as it was
    with pytest.raises(V.VchError, match="-3"):                               # RESIDENT before pgd_init
        _cg(pr, eng, 4, rhs=b, u=eng.RESIDENT)
    # through the C ABI itself: outputs and stats untouched, the message names the function
    D = C.POINTER(C.c_double)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(D)
    re_, cu, pd_, rn = np.full((2, 4), 7.0), np.full((2, 4), 7.0), np.full(2, 7.0), np.full(2, 7.0)
    st, ss, nf = np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int64)
    stats = V.module("_lib").Stats()
    stats.launches = 77
    last_error = V.module("_lib").last_error
    arr = (type(pr.opt) * 1)(pr.opt)
    rows = pr.shape[0]
    keep = dict(dts=np.ascontiguousarray(pr.dts, dtype=np.float64))

    def raw(u=pr.u, k=4, precond=1, rows=rows, n_base=1, re=re_, pd=pd_, cg_tol=0.0, t=pr.t, dt=keep["dts"]):
        t = np.ascontiguousarray(t, dtype=np.float64)
        return lib.vch1d_hess_cg(eng.ctx, dp(pr.phi), dp(u), n_base, rows, dp(dt), dp(t), dp(pr.x), dp(pr.phi_Q), dp(pr.phi_T),
                                 arr, 1, None, 0.0, dp(b), k, cg_tol, precond, None if re is None else re.ctypes.data_as(D),
                                 cu.ctypes.data_as(D), None if pd is None else pd.ctypes.data_as(D), rn.ctypes.data_as(D),
                                 st.ctypes.data_as(C.POINTER(C.c_int32)), ss.ctypes.data_as(C.POINTER(C.c_int32)),
                                 nf.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(stats))

    checks = [(dict(k=0), "k = 0"), (dict(precond=2), "precond"), (dict(cg_tol=float("nan")), "cg_tol"), (dict(re=None), "NULL resid_out"),
                     (dict(pd=None), "NULL resid_out"), (dict(u=None), "no node is free"), (dict(rows=2), "rows"), (dict(n_base=3), "n_base"),
                     (dict(t=t_flat, dt=keep["dts"]), "row 0"), (dict(t=t_bad, dt=None), "step 1")]
    for kw, what in checks:
        assert raw(**kw) == -1, kw
        assert what in last_error() and "vch1d_hess_cg" in last_error(), (what, last_error())
    for a in (re_, cu, pd_, rn, st, ss, nf):
        assert (a == 7).all()
    assert stats.launches == 77 and lib.vch_mem_live() == live and np.array_equal(eng.cg_vector("x"), X)
    assert raw(t=t_flat, precond=0) == 0                 # without the preconditioner the weights are not divided by
    assert not (re_ == 7).any() and stats.host_syncs == 2
    # data-dependent: an empty free set, a right-hand side that is not finite on the free set
    masks = np.stack([pr.mask, np.zeros_like(pr.mask)])
    with pytest.raises(ValueError, match="trajectory 1"):
        _cg(pr, eng, 4, nb=2, rhs=b, mask=masks)
    with pytest.raises(V.VchError, match="-3"):          # the failed call left nothing to fetch
        eng.cg_vector("x")
    with pytest.raises(ValueError, match="trajectory 0"):
        _cg(pr, eng, 4, rhs=b, opt=[V.make_opt(pr.opt, u_min=1.1, u_max=1.2), pr.opt])      # no node inside that box
    with pytest.raises(ValueError, match="trajectory 0"):
        _cg(pr, eng, 4, opt=[V.make_opt(pr.opt, u_min=1.1, u_max=1.2), pr.opt])             # nor for the Newton right-hand side
    bn = b.copy()
    bn[1].ravel()[pr.free[7]] = np.inf
    with pytest.raises(ValueError, match="trajectory 1"):
        _cg(pr, eng, 4, rhs=bn)
    with pytest.raises(V.VchError, match="-3"):
        eng.cg_vector("x")
    bo = b.copy()
    bo[1][~pr.mask] = np.nan                             # off the free set: not read
    bo[0][pr.mask] = 0.0                                 # a zero right-hand side: zero steps, converged, x = 0
    good = _cg(pr, eng, 4, rhs=bo, cg_tol=1e-30)
    X0 = eng.cg_vector("x")
    eng.close()
    assert good["steps"][0] == 0 and good["status"][0] == CONVERGED and good["rnorm0"][0] == 0.0 and not X0[0].any()
    assert good["steps"][1] == 4 and np.isfinite(good["resid"][1]).all() and np.isnan(good["resid"][0]).all()
    assert good["stats"]["linear_solves"] == pr.M * 1 + pr.M * (2 * 4 + 1)
    for key in ("resid", "curv", "pred", "steps"):
        assert np.array_equal(good[key][1], first[key][1], equal_nan=True), key


# ---------------------------------------------------------------------------------------------------------------------
# 10. refused allocations
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_allocations_and_the_balance(driver):
    pr, V = driver, driver.V
    lib = V.load()
    b = _q0(pr.shape, 31)
    base = lib.vch_mem_live()
    eng = pr.context(1)
    live0 = lib.vch_mem_live()
    want = _cg(pr, eng, 3, rhs=b, cg_tol=1e-30)
    m = lib.vch_mem_live() - live0
    pr.lanczos(eng, b, 2, reorth=False)
    again = _cg(pr, eng, 3, rhs=b, cg_tol=1e-30)
    assert lib.vch_mem_live() - live0 == m                # Lanczos without reorthogonalisation and CG share one allocation
    eng.close()
    assert lib.vch_mem_live() == base
    print("lazy requests of the first call:", m)
    assert m >= 6
    for key in KEYS:
        assert np.array_equal(again[key], want[key], equal_nan=True), key
    seen = False
    for i in range(m):
        eng = pr.context(1)
        live0 = lib.vch_mem_live()
        lib.vch_mem_refuse_after(i)
        try:
            with pytest.raises(V.VchError, match="-2|-4") as err:
                _cg(pr, eng, 3, rhs=b, cg_tol=1e-30)
        finally:
            lib.vch_mem_refuse_after(-1)
        assert lib.vch_mem_live() == live0, (i, lib.vch_mem_live() - live0)
        if "Krylov storage" in str(err.value):
            seen = True
            assert "-4" in str(err.value) and "bytes" in str(err.value) and "vch1d_hess_cg" in str(err.value)
        with pytest.raises(V.VchError, match="-3"):
            eng.cg_vector("x")
        got = _cg(pr, eng, 3, rhs=b, cg_tol=1e-30)        # the same call then succeeds
        assert lib.vch_mem_live() - live0 == m
        for key in KEYS:
            assert np.array_equal(got[key], want[key], equal_nan=True), key
        eng.close()
        assert lib.vch_mem_live() == base
    assert seen


# ---------------------------------------------------------------------------------------------------------------------
# 11. the drivers, on the driver's grid with b3 = 1 from the default start of run_main_simulation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refine(V, driver):
    """The driver problem's control about the default start of the 1D march (a base point of its own), b3 = 1."""
    F1 = V.module("Vch_control_1D.Forward_solver")
    K1 = V.module("Vch_control_1D.config")
    d = driver
    phi0 = F1.init_phi_random(d.P.N, F1.delta_sep, amp=0.01, seed=42, enforce_zero_mean=True)
    one = _engine(V, d.P, 1)
    phi = one.forward(phi0, d.dts, u=d.u)[0]
    one.close()
    ocfg = K1.OptimizationConfig(b3=1.0, u_min=-1.0, u_max=1.0)
    pr = Problem(V, d.P, d.t, d.dts, d.x, phi, d.u, V.make_opt(ocfg))
    pr.cfg, pr.S1, pr.ocfg, pr.K1, pr.phi0 = d.cfg, d.S1, ocfg, K1, phi0
    pr.mask = d.mask
    pr.free = d.free
    pr.A = pr.block(pr.free)
    return pr


def test_newton_step_driver_equals_the_dense_solve(refine):
    pr, V = refine, refine.V
    W = _weights(pr)
    N = pr.S1.reduced_newton_step(pr.cfg, pr.u, pr.x, pr.t, pr.ocfg, phi_Q_target=pr.phi_Q, phi_T_target=pr.phi_T, u_min=-1.0,
                                  u_max=1.0, k=4 * 172)
    by_weights = pr.S1.reduced_newton_step(pr.cfg, pr.u, pr.x, pr.t, b1=pr.ocfg.b1, b2=pr.ocfg.b2, b3=pr.ocfg.b3,
                                           kappa=pr.ocfg.kappa_sparsity, phi_Q_target=pr.phi_Q, phi_T_target=pr.phi_T, u_min=-1.0,
                                           u_max=1.0, k=4 * 172)
    eng = pr.context(1)
    G = eng.exact_gradient(pr.t, pr.opt, **pr.kw())[0]
    eng.close()
    bb = np.where(pr.mask, -(G + pr.ocfg.kappa_sparsity * W * np.sign(pr.u)), 0.0)
    want = np.linalg.solve(pr.A, bb.ravel()[pr.free])
    cond = np.linalg.cond(pr.A)
    err = np.abs(N["d"].ravel()[pr.free] - want).max() / np.abs(want).max()
    print(f"MEASURE newton step: steps {N['steps']} status {N['status']} cond {cond:.3g} error {err:.2e} pred {N['pred']:.6e}")
    assert set(N) == {"d", "steps", "status", "resid", "pred", "rnorm0", "curv_min", "n_free", "p"}
    assert N["status"] == "converged" and N["n_free"] == 172 and N["p"] is None and N["curv_min"] > 0
    assert N["d"].shape == pr.u.shape and not N["d"][~pr.mask].any()
    assert err <= cond * SOLVE
    assert np.array_equal(by_weights["d"], N["d"]) and by_weights["steps"] == N["steps"]
    with pytest.raises(ValueError):
        pr.S1.reduced_newton_step(pr.cfg, pr.u, pr.x, pr.t, b1=1.0)


def test_newton_refine(refine):
    pr, V = refine, refine.V
    G1 = V.module("Vch_control_1D.GD_1D")
    ocfg = pr.K1.OptimizationConfig(b3=1.0, u_min=-0.9, u_max=0.9)
    u0 = pr.u
    n_newton = 3
    u3, recs = G1.newton_refine(pr.cfg, ocfg, u0, pr.phi_Q, pr.phi_T, n_newton=n_newton)
    # the same rounds one by one, for the iterates between them and the predicted decrease of every round
    its, chain, preds = [u0], [], []
    for _ in range(len(recs)):
        preds.append(pr.S1.reduced_newton_step(pr.cfg, its[-1], pr.x, pr.t, ocfg, phi_Q_target=pr.phi_Q, phi_T_target=pr.phi_T,
                                               u_min=-0.9, u_max=0.9)["pred"])
        un, r1 = G1.newton_refine(pr.cfg, ocfg, its[-1], pr.phi_Q, pr.phi_T, n_newton=1)
        its.append(un)
        chain += r1
    assert np.array_equal(its[-1], u3) and chain == recs
    for i, r in enumerate(recs):
        print(f"MEASURE newton_refine round {i}: cost {r['cost']:.6f} -> {r['cost_new']:.6f} n_free {r['n_free']} rnorm0 {r['rnorm0']:.3e} "
              f"steps {r['steps']} status {r['status']} s {r['s']} pred {preds[i]:.3e}")
    assert 1 <= len(recs) <= n_newton and recs[0]["s"] is not None
    for r, pred in zip(recs, preds):
        if r["s"] is not None:
            assert r["cost_new"] <= r["cost"] - 1e-4 * r["s"] * pred
        else:
            assert r["cost_new"] == r["cost"]
    costs = [recs[0]["cost"]] + [r["cost_new"] for r in recs]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert all(r["n_free"] == int(pr.S1.free_set(v, -0.9, 0.9).sum()) for r, v in zip(recs, its))
    assert (np.abs(u3) <= 0.9).all()
    last = recs[-1]
    assert (len(recs) == n_newton or last["rnorm0"] == 0.0 or (last["status"] == "negcurv" and last["steps"] == 0)
            or last["s"] is None)
