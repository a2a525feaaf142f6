"""vch1d_pgd_newton / vch1d_newton_trial on the GPU: damped Newton rounds on the free set about the resident PGD iterate of the
1D engine, batched, with the step, the trials and the decisions on the device, against NumPy for the trial
kernel, against the host loop GD_1D.newton_refine, and a batch against single-trajectory contexts.

Problems (the fixtures of test_gpu_krylov_1d.py / test_gpu_hess_cg_1d.py; every context has max_steps = 8, so a trajectory's
stride in a history is 10 rows and not its own row count):
    driver   N = 32, 5 steps: 7 rows x 33 nodes = 231 nodes, one ragged streaming chunk
    n1030    N = 1030, 3 steps: 5 rows x 1031 nodes, two chunks of 4096 nodes, the last ragged, the boundary inside row 3
    refine   the driver's grid and control about the default start of the 1D march with b3 = 1: the problem of
             test_newton_refine (box +-0.9, three rounds)
    sweep    N = 48, 8 steps: the four members of test_gpu_sweep_1d.py through GD_1D.run_sweep

Tolerances.  The trial kernel: the control is bitwise NumPy's (every s is a power of two, so u + s x rounds once however
the multiply-add is compiled) and the counts are exact; the two sums are n terms of one sign added in another order,
asserted at n eps relative.  Against the host loop: status, s and n_free are equal round by round; the CG steps, cost,
cost_new and the final control are measured on an MI355X (the MEASURE lines of test 2), held in MEASURED and asserted at
10 x the measured value, which the assertion at import keeps at or below the class tolerance 1.5e-11 of the 2D file; a
measured 0 is asserted as equality.  The yardstick there is the host loop, never the device call itself.  Everything else
is bitwise: a batch member against a context of its own, a run continued after the rounds against a run started from their
iterate, a context the PGD stop rule ended against a fresh one started from its control."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_hess_cg_1d import _cg, refine                                      # noqa: F401 (fixture)
from test_gpu_krylov_1d import V, _q0, _tile, driver, small                        # noqa: F401 (fixtures)
from test_gpu_second_order_1d import _engine

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
CLASS = 1.5e-11
# measured on an MI355X (the MEASURE lines of test 2): the largest difference in CG steps and the relative differences of
# cost, cost_new and the final control between the device rounds and the host loop
MEASURED = dict(steps=0, cost=0.0, cost_new=0.0, control=0.0)
TOL = {k: 10 * v for k, v in MEASURED.items()}
assert max(TOL[k] for k in ("cost", "cost_new", "control")) <= CLASS
ACCEPTED, STATIONARY, NEGCURV, BREAKDOWN, STALLED, IDLE = range(6)
OUT_KEYS = ("cost", "cost_new", "s", "pred", "rnorm0", "halvings", "cg_steps", "cg_status", "status", "n_free", "pinned", "clipped")
PGD_KEYS = ("cost", "alpha", "trials", "change", "tracking_error", "terminal_error")


def _pgd(pr, opts, u0, alpha0=None, t=None):
    """A context of batch len(opts) with the problem of `pr` resident as a PGD problem from the controls u0."""
    nb = len(opts)
    eng = pr.context(nb)
    eng.pgd_init(_tile(pr.phi0, nb), _tile(pr.phi_T, nb), pr.t if t is None else t, pr.dts, list(opts), phi_Q=_tile(pr.phi_Q, nb), x=pr.x,
                 u0=np.ascontiguousarray(u0), alpha0=alpha0)
    return eng


def _same(a, b, keys=OUT_KEYS):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


# ---------------------------------------------------------------------------------------------------------------------
# 1. the trial kernel against NumPy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["driver", "n1030"])
def test_trial_kernel_against_numpy(request, name):
    pr = request.getfixturevalue("driver") if name == "driver" else request.getfixturevalue("small")(name)
    Vm = pr.V
    nb, s = 3, np.array([1.0, 0.5, 0.125])
    rows, n = pr.shape
    nodes = rows * n
    assert (name, rows, n) in (("driver", 7, 33), ("n1030", 5, 1031))
    mask = np.random.default_rng(51).random(pr.shape) < 0.5                  # about half the nodes, uploaded
    assert 0.4 * nodes < mask.sum() < 0.6 * nodes
    top = float(np.abs(pr.u).max())
    b = _q0(pr.shape, 41)
    eng = pr.context(nb)
    wide = [Vm.make_opt(u_min=-1e30, u_max=1e30)] * nb
    _cg(pr, eng, 2, nb=nb, rhs=_tile(b, nb), mask=_tile(mask, nb), opt=wide, cg_tol=1e-30)
    X1 = eng.cg_vector("x")[0]
    # a right-hand side whose two-step iterate is a few times the control's size: s x flips signs and leaves the boxes
    b = b * 2.0 ** np.round(np.log2(4.0 * top / np.median(np.abs(X1[mask]))))
    R = _cg(pr, eng, 2, nb=nb, rhs=_tile(b, nb), mask=_tile(mask, nb), opt=wide, cg_tol=1e-30)
    X0 = eng.cg_vector("x")
    assert (R["steps"] == 2).all() and (R["n_free"] == mask.sum()).all()
    # the boxes from the quantiles of u + s x: a tenth of the nodes beyond either bound
    boxes = []
    for i in range(nb):
        v = pr.u + s[i] * X0[i]
        lo, hi = float(np.quantile(v, 0.1)), float(np.quantile(v, 0.9))
        assert lo < 0.0 < hi
        boxes.append((lo, hi))
    opts = [Vm.make_opt(u_min=lo, u_max=hi) for lo, hi in boxes]
    _cg(pr, eng, 2, nb=nb, rhs=_tile(b, nb), mask=_tile(mask, nb), opt=opts, cg_tol=1e-30)
    X, Rr, Pp = eng.cg_vector("x"), eng.cg_vector("r"), eng.cg_vector("p")
    assert np.array_equal(X, X0) and not X[:, ~mask].any()                  # an uploaded mask: the box does not enter the solve
    T = eng.newton_trial(s)
    quiet = eng.newton_trial(s, want_u=False)
    after = eng.cg_vector("x"), eng.cg_vector("r"), eng.cg_vector("p")
    eng.close()
    assert quiet["u"] is None and np.array_equal(quiet["change"], T["change"]) and np.array_equal(quiet["pinned"], T["pinned"])
    for i, (lo, hi) in enumerate(boxes):
        v = pr.u + s[i] * X[i]
        t = np.clip(v, lo, hi)
        clipped = int((t != v).sum())
        pin = mask & (t * pr.u < 0.0)
        t[pin] = 0.0
        rest = ~mask & (pr.u >= lo) & (pr.u <= hi)
        # the expectation itself has all three kinds
        assert pin.sum() >= 1 and clipped >= 1 and rest.sum() >= 1, (i, int(pin.sum()), clipped, int(rest.sum()))
        d2, n2 = float(np.sum((t - pr.u) ** 2)), float(np.sum(pr.u ** 2))
        print(f"MEASURE trial {name} member {i}: s {s[i]} box {lo:.3g} {hi:.3g} pinned {int(pin.sum())} clipped {clipped} untouched "
              f"off the mask {int(rest.sum())} of {nodes}; sums dev {abs(T['change'][i, 0] / d2 - 1):.2e} "
              f"{abs(T['change'][i, 1] / n2 - 1):.2e} (bound {nodes * EPS:.2e})")
        assert np.array_equal(T["u"][i].view(np.int64), t.view(np.int64)), i
        assert np.array_equal(T["u"][i][rest].view(np.int64), pr.u[rest].view(np.int64))
        assert T["pinned"][i] == pin.sum() and T["clipped"][i] == clipped
        assert abs(T["change"][i, 0] - d2) <= nodes * EPS * d2 and abs(T["change"][i, 1] - n2) <= nodes * EPS * n2
    for got, want in zip(after, (X, Rr, Pp)):
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the host loop
# ---------------------------------------------------------------------------------------------------------------------
def _refine_case(pr):
    ocfg = pr.K1.OptimizationConfig(b3=1.0, u_min=-0.9, u_max=0.9)
    return ocfg, pr.V.make_opt(ocfg), pr.u


def test_rounds_against_the_host_loop(refine):
    pr, Vm = refine, refine.V
    G1 = Vm.module("Vch_control_1D.GD_1D")
    ocfg, box, u0 = _refine_case(pr)
    u3, recs = G1.newton_refine(pr.cfg, ocfg, u0, pr.phi_Q, pr.phi_T, n_newton=3)
    ud, rd = G1.newton_refine(pr.cfg, ocfg, u0, pr.phi_Q, pr.phi_T, n_newton=3, on_device=True)
    assert ud.shape == u3.shape and len(rd) == len(recs) == 3
    rel = lambda a, b: abs(a - b) / abs(b)
    dev = dict(steps=0, cost=0.0, cost_new=0.0)
    for r, (a, b) in enumerate(zip(rd, recs)):
        print(f"MEASURE round {r}: device cost {a['cost']:.17g} -> {a['cost_new']:.17g} s {a['s']} n_free {a['n_free']} cg {a['status']} "
              f"in {a['steps']} rnorm0 {a['rnorm0']:.6e}; host cost {b['cost']:.17g} -> {b['cost_new']:.17g} s {b['s']} n_free "
              f"{b['n_free']} cg {b['status']} in {b['steps']} rnorm0 {b['rnorm0']:.6e}; rel. dev {rel(a['cost'], b['cost']):.2e} "
              f"{rel(a['cost_new'], b['cost_new']):.2e}")
        assert set(a) == set(b)
        assert (a["status"], a["s"], a["n_free"]) == (b["status"], b["s"], b["n_free"]) and a["s"] is not None
        dev["steps"] = max(dev["steps"], abs(a["steps"] - b["steps"]))
        dev["cost"] = max(dev["cost"], rel(a["cost"], b["cost"]))
        dev["cost_new"] = max(dev["cost_new"], rel(a["cost_new"], b["cost_new"]))
    dev["control"] = float(np.abs(ud - u3).max() / np.abs(u3).max())
    print(f"MEASURE against the host loop: {dev}")
    for key in dev:
        assert dev[key] <= TOL[key], (key, dev[key])
    # the engine call itself: the records of the driver's device path
    eng = _pgd(pr, [box], u0[None])
    R = eng.pgd_newton(3)
    u_dev = eng.pgd_get("u")
    eng.close()
    assert R["rounds"] == 3 and R["status"][0].tolist() == [ACCEPTED] * 3 and np.array_equal(u_dev, ud)
    for r, a in enumerate(rd):
        assert a["cost"] == R["cost"][0, r] and a["cost_new"] == R["cost_new"][0, r] and a["rnorm0"] == R["rnorm0"][0, r]
        assert a["steps"] == R["cg_steps"][0, r] and a["n_free"] == R["n_free"][0, r] and a["s"] == R["s"][0, r]


# ---------------------------------------------------------------------------------------------------------------------
# 3. a batch of three against three single contexts
# ---------------------------------------------------------------------------------------------------------------------
HALF = 0.5
CUT = HALF - 2.0 ** -20
# measured on an MI355X (the MEASURE line of test 3) and pinned: the halvings the box-cut member needs, s = 2^-CUT_HALVINGS
CUT_HALVINGS = 5


def _box_cut(pr):
    """After _box_cut of test_gpu_newton_2d.py: b3 = 1 from u0 = 0.5 at every node of rows 1.., with the lower bound 2^-20
    below: the Newton step is about -u there, every trial is clipped to the bound and gains a few millionths of the
    decrease `pred` the model predicts for the full step, a sufficient decrease 1e-4 s pred only after several halvings.
    Row 0 is zero and so off the free set: with all of row 0 free the reduced Hessian is singular.  It
    lies outside the box, and every trial clips it to the bound whatever s is.  Row 0 has quadrature weight zero but drives
    step 0, so under tracking weights that move changes the cost by an amount that does not shrink with s (measured with
    the default b1, b2: the full step is accepted at once, 1.61390 -> 1.61340, with the whole gain from row 0).  The
    member therefore runs with b1 = b2 = 0: its cost is the control's alone, row 0 does not enter it, and what the
    halvings see is the clip at the bound, as in 2D."""
    u0 = np.full_like(pr.u, HALF)
    u0[0] = 0.0
    return pr.V.make_opt(pr.ocfg, b1=0.0, b2=0.0, b3=1.0, u_min=CUT, u_max=2.0), u0


def _three(pr):
    """Member 0: the case of test 2 (accepts a step in every round).  Member 1: u0 = 0 has an empty free set (STATIONARY
    at round 0, the control untouched).  Member 2: the box-cut start."""
    _, box, u = _refine_case(pr)
    cut, half = _box_cut(pr)
    opts = [box, pr.V.make_opt(pr.ocfg, kappa_sparsity=0.05, u_min=-0.5, u_max=0.5), cut]
    return opts, np.stack([u, np.zeros_like(u), half])


def test_batch_of_three_equals_three_single_contexts(refine):
    pr = refine
    opts, u0 = _three(pr)
    n_rounds = 3
    eng = _pgd(pr, opts, u0)
    many = eng.pgd_newton(n_rounds)
    Um, Pm = eng.pgd_get("u"), eng.pgd_get("phi")
    Xm = eng.cg_vector("x"), eng.cg_vector("r"), eng.cg_vector("p")
    eng.close()
    print(f"MEASURE batch: status {many['status'].tolist()} s {many['s'].tolist()} halvings {many['halvings'].tolist()} n_free "
          f"{many['n_free'].tolist()} pinned {many['pinned'].tolist()} clipped {many['clipped'].tolist()} cg {many['cg_status'].tolist()} "
          f"steps {many['cg_steps'].tolist()} cost {many['cost'].tolist()} cost_new {many['cost_new'].tolist()} pred {many['pred'].tolist()}")
    assert many["rounds"] == n_rounds
    assert many["status"][0].tolist() == [ACCEPTED] * 3 and np.isfinite(many["s"][0]).all()
    # the empty free set: STATIONARY, zero steps, converged, idle afterwards, and the resident vectors are zeros
    assert many["status"][1].tolist() == [STATIONARY, IDLE, IDLE] and many["n_free"][1, 0] == 0 and many["rnorm0"][1, 0] == 0.0
    assert many["pred"][1, 0] == 0.0 and many["cg_steps"][1, 0] == 0 and many["cg_status"][1, 0] == 1
    assert not Um[1].any() and np.isnan(many["cost"][1, 1:]).all() and np.isnan(many["s"][1]).all()
    assert not many["n_free"][1, 1:].any() and not many["halvings"][1].any()
    for vec in Xm:
        assert not vec[1].any()
    assert np.abs(Xm[0][0]).max() > 0
    # the box-cut member: the step is cut short
    rows, n = pr.shape
    assert many["status"][2, 0] == ACCEPTED and many["halvings"][2, 0] >= 1 and many["n_free"][2, 0] == (rows - 1) * n
    assert many["halvings"][2, 0] == CUT_HALVINGS and many["s"][2, 0] == 2.0 ** -CUT_HALVINGS
    assert many["clipped"][2, 0] == rows * n and (Um[2] == CUT).all() and many["cost_new"][2, 0] < many["cost"][2, 0]
    assert many["status"][2, 1:].tolist() == [STATIONARY, IDLE] and many["n_free"][2, 1] == 0
    assert many["cost"][2, 1] == many["cost_new"][2, 0] == many["cost_new"][2, 1]
    for i in range(3):
        one = _pgd(pr, [opts[i]], u0[i][None])
        got = one.pgd_newton(n_rounds)
        U1, P1 = one.pgd_get("u"), one.pgd_get("phi")
        X1 = one.cg_vector("x")
        one.close()
        assert got["rounds"] == (3, 1, 2)[i]              # alone, a trajectory that has ended ends the call
        for key in OUT_KEYS:
            assert np.array_equal(got[key][0], many[key][i], equal_nan=True), (key, i)
        assert np.array_equal(U1, Um[i]) and np.array_equal(P1, Pm[i]), i
        if i == 0:
            assert np.array_equal(X1[0], Xm[0][0])        # the last round's vectors
    # one halving short: STALLED, the control unmoved, the cost unchanged
    cut, half = opts[2], u0[2]
    eng = _pgd(pr, [cut], half[None])
    phi0 = eng.pgd_get("phi")
    R = eng.pgd_newton(2, max_halvings=CUT_HALVINGS - 1)
    assert R["rounds"] == 1 and R["status"][0].tolist() == [STALLED, IDLE] and R["halvings"][0, 0] == CUT_HALVINGS - 1
    assert R["cost_new"][0, 0] == R["cost"][0, 0] and np.isnan(R["s"][0, 0])
    assert np.array_equal(eng.pgd_get("u"), half) and np.array_equal(eng.pgd_get("phi"), phi0)
    R = eng.pgd_newton(1, max_halvings=CUT_HALVINGS)     # a new call starts afresh: nobody is idle
    assert R["status"][0, 0] == ACCEPTED and R["s"][0, 0] == many["s"][2, 0] and R["cost_new"][0, 0] == many["cost_new"][2, 0]
    assert R["cost_new"][0, 0] <= R["cost"][0, 0] - 1e-4 * R["s"][0, 0] * R["pred"][0, 0]
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. state afterwards
# ---------------------------------------------------------------------------------------------------------------------
def test_the_adjoint_of_the_replaced_iterate_is_invalid_and_the_solve_sees_the_new_free_set(refine):
    pr, Vm = refine, refine.V
    _, box, u0 = _refine_case(pr)
    resident = lambda e: e.hess_cg(3, pr.t, box, u=e.RESIDENT, phi_Q=e.RESIDENT, phi_T=e.RESIDENT, dt=pr.dts, x=pr.x)
    eng = _pgd(pr, [box], u0[None], alpha0=1e-3)         # a short first step: the iterate keeps a free set
    eng.pgd_iterate(1)
    eng.pgd_kkt(refresh=False)                           # the sweep of the iteration left r resident
    before = resident(eng)
    R = eng.pgd_newton(1)
    assert R["status"][0, 0] == ACCEPTED and R["n_free"][0, 0] == before["n_free"][0]
    with pytest.raises(Vm.VchError, match="-3"):         # r is the adjoint of an iterate that has been replaced
        eng.pgd_kkt(refresh=False)
    un = eng.pgd_get("u")
    assert np.abs(eng.cg_vector("x")).max() > 0          # the round's vectors are resident
    # hess_cg in its resident mode works about the new iterate: its free set is the new control's, which is another one
    after = resident(eng)
    n_new = int(pr.S1.free_set(un, -0.9, 0.9).sum())
    print(f"MEASURE state: n_free {before['n_free'][0]} -> {after['n_free'][0]}, pinned {R['pinned'][0, 0]} clipped {R['clipped'][0, 0]}")
    assert after["n_free"][0] == n_new and n_new != before["n_free"][0]
    assert np.isfinite(eng.exact_gradient(pr.t, box, u=eng.RESIDENT, phi_Q=eng.RESIDENT, phi_T=eng.RESIDENT, dt=pr.dts, x=pr.x)).all()
    assert eng.pgd_kkt(refresh=True)["total"][0] == pr.u.size
    eng.pgd_kkt(refresh=False)
    eng.close()


def test_init_then_rounds_then_an_iteration_equals_init_from_the_newton_iterate(refine):
    pr = refine
    _, box, u0 = _refine_case(pr)
    eng = _pgd(pr, [box], u0[None])
    R = eng.pgd_newton(2)
    assert R["status"][0].tolist() == [ACCEPTED, ACCEPTED]
    un, phin = eng.pgd_get("u"), eng.pgd_get("phi")
    got = eng.pgd_iterate(1)
    u_got, phi_got = eng.pgd_get("u"), eng.pgd_get("phi")
    eng.close()
    ref = _pgd(pr, [box], un[None])
    assert np.array_equal(ref.pgd_get("phi"), phin)
    want = ref.pgd_iterate(1)
    for key in PGD_KEYS:
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(ref.pgd_get("u"), u_got) and np.array_equal(ref.pgd_get("phi"), phi_got)
    ref.close()


def test_a_call_that_accepts_nothing_leaves_the_pgd_run_undisturbed(refine):
    """Member 0 is stationary (empty free set), member 1 is the box-cut start one halving short (STALLED): nothing moves,
    and the iteration that follows is that of a run without the call."""
    pr = refine
    opts, u0 = _three(pr)
    opts, u0 = opts[1:], u0[1:]
    plain = _pgd(pr, opts, u0)
    want = plain.pgd_iterate(1)
    u_want, phi_want = plain.pgd_get("u"), plain.pgd_get("phi")
    plain.close()
    eng = _pgd(pr, opts, u0)
    phi0 = eng.pgd_get("phi")
    R = eng.pgd_newton(2, max_halvings=CUT_HALVINGS - 1)
    assert R["rounds"] == 1 and R["status"][:, 0].tolist() == [STATIONARY, STALLED]
    assert np.isnan(R["s"]).all() and np.array_equal(R["cost"][:, 0], R["cost_new"][:, 0])
    assert np.array_equal(eng.pgd_get("u"), u0) and np.array_equal(eng.pgd_get("phi"), phi0)
    got = eng.pgd_iterate(1)
    for key in PGD_KEYS:
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(eng.pgd_get("u"), u_want) and np.array_equal(eng.pgd_get("phi"), phi_want)
    eng.pgd_kkt(refresh=False)                           # nothing moved: the iteration's adjoint is the resident one
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the stop quirk
# ---------------------------------------------------------------------------------------------------------------------
def test_a_trajectory_the_stop_rule_ended_is_brought_up_to_its_control(refine):
    """A warm start from the driver's control, inside its own box [-1, 1], with a tiny alpha_max: the relative change of
    every iteration stays below 1e-5 and the stop rule fires in the twelfth (k = 11), which takes the new control and keeps
    the previous state and cost."""
    pr, Vm = refine, refine.V
    box = Vm.make_opt(pr.ocfg, b3=1.0, u_min=-1.0, u_max=1.0, alpha_max=1e-6)
    eng = _pgd(pr, [box], pr.u[None])
    it = eng.pgd_iterate(12)
    u_stop, phi_stop = eng.pgd_get("u"), eng.pgd_get("phi")
    one = pr.context(1)
    fresh = one.forward(pr.phi0, pr.dts, u=u_stop)[0]
    print(f"MEASURE stop quirk: iterations {it['iters']} changes {it['change'][0].tolist()} state differs from the fresh march by "
          f"{np.abs(phi_stop - fresh).max():.3e}")
    assert it["iters"] == 12 and (it["change"][0] < 1e-5).all() and u_stop.any()
    assert eng.pgd_iterate(1)["iters"] == 0              # stopped: never iterated again
    assert not np.array_equal(phi_stop, fresh)           # the precondition: the resident state is the previous iterate's
    R = eng.pgd_newton(1)
    u_got, phi_got = eng.pgd_get("u"), eng.pgd_get("phi")
    again = eng.pgd_newton(1)                            # reconciled once: a second call marches nothing more
    eng.close()
    ref = _pgd(pr, [box], u_stop[None])
    assert np.array_equal(ref.pgd_get("phi"), fresh)
    want = ref.pgd_newton(1)
    _same(R, want)
    assert R["status"][0, 0] == ACCEPTED
    assert np.array_equal(u_got, ref.pgd_get("u")) and np.array_equal(phi_got, ref.pgd_get("phi"))
    _same(again, ref.pgd_newton(1))
    ref.close()
    assert np.array_equal(phi_got, one.forward(pr.phi0, pr.dts, u=u_got)[0])            # the fresh march of the new control
    one.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors and memory
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_anything_is_enqueued_or_allocated(refine):
    pr, Vm = refine, refine.V
    lib = Vm.load()
    last_error = Vm.module("_lib").last_error
    _, box, u0 = _refine_case(pr)
    fresh = pr.context(1)
    live = lib.vch_mem_live()
    with pytest.raises(Vm.VchError, match="-3"):
        fresh.pgd_newton(1)
    assert "vch1d_pgd_newton" in last_error()
    with pytest.raises(Vm.VchError, match="-3"):
        fresh.newton_trial(1.0)
    assert lib.vch_mem_live() == live
    fresh.close()
    eng = _pgd(pr, [box], u0[None])
    U, P = eng.pgd_get("u"), eng.pgd_get("phi")
    live = lib.vch_mem_live()

    def unchanged(what):
        assert lib.vch_mem_live() == live, what
        assert np.array_equal(eng.pgd_get("u"), U) and np.array_equal(eng.pgd_get("phi"), P), what

    for bad in (dict(n_rounds=0), dict(n_rounds=-2), dict(k=0), dict(max_halvings=-1), dict(precond=2), dict(precond=-1),
                dict(cg_tol=np.nan), dict(cg_tol=np.inf)):
        args = dict(n_rounds=2)
        args.update(bad)
        with pytest.raises(ValueError):
            eng.pgd_newton(**args)
        assert "vch1d_pgd_newton" in last_error()
        unchanged(bad)
    # NULL outputs, at the C boundary
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    d, i32, i64 = np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(6, dtype=np.int64)
    full = [dp(d), dp(d), dp(d), dp(d), dp(d), ip(i32), ip(i32), ip(i32), ip(i32), i64.ctypes.data_as(C.POINTER(C.c_int64))]
    for hole in range(len(full)):
        outs = list(full)
        outs[hole] = None
        assert lib.vch1d_pgd_newton(eng.ctx, 2, 5, 1e-8, 1, 0.0, 10, *outs, None) == -1, hole
        unchanged(hole)
    # the trial's seam: no resident vectors yet, then step lengths that are not finite or not positive
    with pytest.raises(Vm.VchError, match="-3"):
        eng.newton_trial(1.0)
    unchanged("trial")
    eng.close()
    # the preconditioner's time weights: rows 0, 1, 2 share a time, wt'_0 = wt_1 = 0
    t_flat = pr.t.copy()
    t_flat[2] = t_flat[1] = t_flat[0]
    eng = _pgd(pr, [box], u0[None], t=t_flat)
    U, P = eng.pgd_get("u"), eng.pgd_get("phi")
    live = lib.vch_mem_live()
    with pytest.raises(ValueError):
        eng.pgd_newton(1, precond=True)
    assert "row 0" in last_error() and "vch1d_pgd_newton" in last_error()
    unchanged("time weights")
    eng.close()
    # after a stateless solve: the seam's argument errors
    eng = pr.context(1)
    eng.hess_cg(2, pr.t, box, **pr.kw())
    X = eng.cg_vector("x")
    live = lib.vch_mem_live()
    for s in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            eng.newton_trial(s)
        assert lib.vch_mem_live() == live, s
    assert lib.vch1d_newton_trial(eng.ctx, None, None, dp(d), i64.ctypes.data_as(C.POINTER(C.c_int64))) == -1
    assert lib.vch_mem_live() == live and np.array_equal(eng.cg_vector("x"), X)
    T = eng.newton_trial(0.5)                            # no PGD problem was loaded: the trial scratch comes on first use
    assert lib.vch_mem_live() == live + 1
    t = np.clip(pr.u + 0.5 * X[0], -0.9, 0.9)
    t[pr.S1.free_set(pr.u, -0.9, 0.9) & (t * pr.u < 0.0)] = 0.0
    assert np.array_equal(T["u"][0], t)
    eng.close()


def test_refused_allocations_and_the_balance(refine):
    pr, Vm = refine, refine.V
    lib = Vm.load()
    _, box, u0 = _refine_case(pr)
    base = lib.vch_mem_live()
    eng = _pgd(pr, [box], u0[None])
    live0 = lib.vch_mem_live()
    want = eng.pgd_newton(1, k=3)
    m = lib.vch_mem_live() - live0
    u_want = eng.pgd_get("u")
    eng.newton_trial(0.5, want_u=False)
    eng.pgd_newton(1, k=3)
    eng.hess_cg(3, pr.t, box, u=eng.RESIDENT, phi_Q=eng.RESIDENT, phi_T=eng.RESIDENT, dt=pr.dts, x=pr.x)
    assert lib.vch_mem_live() - live0 == m               # the rounds run in the storage of hess_cg and the PGD buffers
    eng.close()
    assert lib.vch_mem_live() == base
    print("lazy requests of the first call:", m)
    assert m >= 6
    seen = False
    for i in range(m):
        eng = _pgd(pr, [box], u0[None])
        live0 = lib.vch_mem_live()
        lib.vch_mem_refuse_after(i)
        try:
            with pytest.raises(Vm.VchError, match="-2|-4") as err:
                eng.pgd_newton(1, k=3)
        finally:
            lib.vch_mem_refuse_after(-1)
        assert lib.vch_mem_live() == live0, (i, lib.vch_mem_live() - live0)
        if "Krylov storage" in str(err.value):
            seen = True
            assert "-4" in str(err.value) and "bytes" in str(err.value) and "vch1d_pgd_newton" in str(err.value)
        assert np.array_equal(eng.pgd_get("u"), u0)       # the context stays usable, the iterate is as it was
        got = eng.pgd_newton(1, k=3)                      # the same call then succeeds with the same bits
        assert lib.vch_mem_live() - live0 == m
        _same(got, want)
        assert np.array_equal(eng.pgd_get("u"), u_want)
        eng.close()
        assert lib.vch_mem_live() == base
    assert seen


# ---------------------------------------------------------------------------------------------------------------------
# 7. run_sweep(n_newton)
# ---------------------------------------------------------------------------------------------------------------------
def test_run_sweep_polishes_every_member(V):                # noqa: F811
    import test_gpu_sweep_1d as S
    K1 = V.module("Vch_control_1D.config")
    G1 = V.module("Vch_control_1D.GD_1D")
    F1 = V.module("Vch_control_1D.Forward_solver")
    cfg = K1.ForwardSolverConfig(N=S.N, T=S.M * S.DT, dt_initial=S.DT)
    members = [K1.OptimizationConfig(**S.MEMBERS[n]) for n in S.NAMES]
    kw = dict(n_iter=S.N_ITER, seed=42, amp=0.05, return_controls=True)
    plain = G1.run_sweep(cfg, members, **kw)
    zero = G1.run_sweep(cfg, members, n_newton=0, **kw)
    parent_keys = {"costs", "alphas", "trials", "changes", "tracking_error", "terminal_error", "iters", "seconds", "kkt", "phi_T", "t_hist",
                   "x", "u"}
    assert set(plain) == set(zero) == parent_keys
    for key in parent_keys - {"seconds", "kkt", "iters"}:
        assert np.array_equal(plain[key], zero[key]), key
    assert plain["iters"] == zero["iters"]
    for key in plain["kkt"]:
        assert np.array_equal(plain["kkt"][key], zero["kkt"][key]), key
    res = G1.run_sweep(cfg, members, n_newton=2, **kw)
    assert set(res) == parent_keys | {"newton", "costs_newton"}
    for key in ("costs", "alphas", "trials", "changes", "tracking_error", "terminal_error"):
        assert np.array_equal(res[key], plain[key]), key                 # the polish comes after the PGD iterations
    cn, N = res["costs_newton"], res["newton"]
    print(f"MEASURE sweep: costs_newton {cn.tolist()} status {N['status'].tolist()} s {N['s'].tolist()} n_free {N['n_free'].tolist()} "
          f"cg {N['cg_status'].tolist()} steps {N['cg_steps'].tolist()} halvings {N['halvings'].tolist()}")
    assert cn.shape == (len(members), 3) and np.isfinite(cn).all()
    assert np.array_equal(cn[:, 0], plain["costs"][:, -1])
    assert (np.diff(cn, axis=1) <= 0.0).all()
    moved = N["status"] == ACCEPTED
    assert np.array_equal(np.isfinite(N["s"]), moved)
    for b in range(len(members)):
        if not moved[b].any():
            assert np.array_equal(res["u"][b], plain["u"][b])
    # a direct pgd_newton on an identically prepared context
    B = len(members)
    tg, dts = V.time_grid(float(cfg.T), float(cfg.dt_initial))
    t_hist = np.concatenate([[0.0], tg])
    phi0 = F1.init_phi_random(S.N, F1.delta_sep, amp=0.05, seed=42, enforce_zero_mean=True)
    eng = V.Engine1D.from_config(cfg, batch=B, max_steps=len(dts))
    phi_T = G1.build_targets_1d(eng.x.copy(), t_hist, phi0, float(cfg.Lx), float(cfg.T), choice_t=1, choice_q=2)[0]
    eng.pgd_init(_tile(phi0, B), _tile(phi_T, B), t_hist, dts, [V.make_opt(o) for o in members], x=eng.x.copy())
    eng.pgd_iterate(S.N_ITER)
    direct = eng.pgd_newton(2)
    u_direct = eng.pgd_get("u")
    kkt = eng.pgd_kkt(refresh=True)
    eng.close()
    _same(N, direct)
    assert N["rounds"] == direct["rounds"] and np.array_equal(res["u"], u_direct)
    for key in kkt:
        assert np.array_equal(res["kkt"][key], kkt[key]), key
