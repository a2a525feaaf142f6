"""vch2d_pgd_newton / vch2d_newton_trial on the GPU: damped Newton rounds on the free set about the resident PGD iterate of the
2D engine, batched, with the step, the trials and the decisions on the device, against NumPy for the trial
kernel, against the host loop GD2_configured.newton_refine, and a batch against single-trajectory contexts.

Problems (the fixtures of test_gpu_krylov_2d.py):
    dense    12 x 9, M = 2 (390 nodes), GEMM-DCT, one tile: the case of test_newton_refine (b3 = 1, box +-0.9,
             u0 = u + 0.75) and its variants
    tiles    128 x 32, Ly 0.5, M = 2: plane 33 x 129, 3 x 3 tiles with ragged last rows and columns
    chunks   16 x 16 (FFT), 21 levels under VCH_KR_LCHUNK=4: six chunks of levels, the last ragged
    sweep    64 x 32, 4 steps: the four members of test_gpu_sweep.py through GD2_configured.run_sweep

Tolerances.  The trial kernel: the control is bitwise NumPy's (every s is a power of two, so u + s x rounds once however
the multiply-add is compiled) and the counts are exact; the two sums are n terms of one sign added in another order,
asserted at n eps relative.  Against the host loop: status, s and n_free are equal round by round and the CG steps within
one; cost, cost_new and the final control came out equal on an MI355X (the MEASURE lines of test 2: the device rounds run
the kernels of the host loop on the same operands), so equality is asserted: MEASURED below holds the differences, all 0.
Everything else is bitwise: a batch member against a context of its own, and a run continued after the rounds against a
run started from their iterate."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_forms import _env
from test_gpu_hessvec_2d import EPS, _engine
from test_gpu_krylov_2d import Problem, V, _mask_of, _q0, _tile, chunks, dense, tiles      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

CLASS = 1.5e-11
# measured on an MI355X (the MEASURE lines of test 2), relative differences between the device rounds and the host loop
MEASURED = dict(cost=0.0, cost_new=0.0, control=0.0)
TOL = {k: 10 * v for k, v in MEASURED.items()}
assert max(TOL.values()) <= CLASS
ACCEPTED, STATIONARY, NEGCURV, BREAKDOWN, STALLED, IDLE = range(6)
OUT_KEYS = ("cost", "cost_new", "s", "pred", "rnorm0", "halvings", "cg_steps", "cg_status", "status", "n_free", "pinned", "clipped")
PGD_KEYS = ("cost", "alpha", "attempts", "change", "tracking_error", "terminal_error")


def _pgd(pr, opts, u0, alpha0=None):
    """A context of batch len(opts) with the problem of `pr` resident as a PGD problem from the controls u0."""
    nb = len(opts)
    with _env(**pr.env):
        eng = _engine(pr.V, pr.P, nb, max_steps=pr.max_steps)
    eng.pgd_init(_tile(pr.phi0, nb), _tile(pr.phi_T, nb), pr.t, list(opts), phi_Q=_tile(pr.phi_Q, nb), ramp=False, x=pr.x, y=pr.y,
                 u0=np.ascontiguousarray(u0), alpha0=alpha0)
    return eng


CUT = 0.5 - 2.0 ** -20


def _box_cut(pr):
    """b3 = 1 from u0 = 0.5 at every node, all free, with the lower bound 2^-20 below: the Newton step is about -u at
    every node, every trial is clipped to the bound and gains about 4e-6 of the decrease `pred` the model predicts for
    the full step, a sufficient decrease 1e-4 s pred only from s = 1/32 on, the fifth halving.  The accepted trial has
    every node on the bound: the next free set is empty."""
    return pr.V.make_opt(pr.ocfg, b3=1.0, u_min=CUT, u_max=2.0), np.full_like(pr.u, 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the trial kernel against NumPy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiles", "chunks"])
def test_trial_kernel_against_numpy(request, name):
    pr = request.getfixturevalue(name)
    V = pr.V
    nb, s = 3, np.array([1.0, 0.5, 0.125])
    top = float(np.abs(pr.u).max())
    boxes = [(-0.6 * top, 0.8 * top), (-0.3 * top, 0.5 * top), (-0.9 * top, 0.2 * top)]
    opts = [V.make_opt(u_min=lo, u_max=hi) for lo, hi in boxes]
    # a right-hand side whose solution is 32 times the control's size on the free nodes: s x flips signs and leaves the boxes
    b = _q0(pr.shape, 41)
    want = np.linalg.solve(pr.A, b.ravel()[pr.free])
    b *= 32.0 * top / np.median(np.abs(want))
    n = len(pr.free)
    eng = pr.context(nb)
    R = eng.hess_cg(2 * n, rhs=_tile(b, nb), cg_tol=1e-8, mask=_tile(pr.mask, nb), opt=opts, **pr.kw(nb))
    X = eng.cg_vector("x")
    assert (R["n_free"] == n).all() and np.abs(X).max() > top
    T = eng.newton_trial(s)
    after = eng.cg_vector("x")
    eng.close()
    nodes = pr.u.size
    for i, (lo, hi) in enumerate(boxes):
        v = pr.u + s[i] * X[i]
        t = np.clip(v, lo, hi)
        clipped = int((t != v).sum())
        pin = pr.mask & (t * pr.u < 0.0)
        t[pin] = 0.0
        assert pin.sum() >= 1 and clipped >= 1, (i, int(pin.sum()), clipped)          # the expectation itself has both kinds
        d2, n2 = float(np.sum((t - pr.u) ** 2)), float(np.sum(pr.u ** 2))
        print(f"MEASURE trial {name} member {i}: s {s[i]} pinned {int(pin.sum())} clipped {clipped} of {nodes}; sums dev "
              f"{abs(T['change'][i, 0] / d2 - 1):.2e} {abs(T['change'][i, 1] / n2 - 1):.2e} (bound {nodes * EPS:.2e})")
        assert np.array_equal(T["u"][i].view(np.int64), t.view(np.int64)), i
        assert T["pinned"][i] == pin.sum() and T["clipped"][i] == clipped
        assert abs(T["change"][i, 0] - d2) <= nodes * EPS * d2 and abs(T["change"][i, 1] - n2) <= nodes * EPS * n2
    assert np.array_equal(after, X)


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the host driver
# ---------------------------------------------------------------------------------------------------------------------
def _refine_case(pr):
    K2 = pr.V.module("Vch_control_2D.config")
    ocfg = K2.OptimizationConfig(b3=1.0, u_min=-0.9, u_max=0.9)
    return ocfg, pr.V.make_opt(ocfg), pr.u + 0.75


def test_rounds_against_the_host_driver(dense):
    pr, V = dense, dense.V
    G2 = V.module("Vch_control_2D.GD2_configured")
    ocfg, box, u0 = _refine_case(pr)
    u3, recs = G2.newton_refine(pr.cfg, ocfg, u0, pr.phi_Q, pr.phi_T, n_newton=3)
    eng = _pgd(pr, [box], u0[None])
    R = eng.pgd_newton(3)
    u_dev = eng.pgd_get("u")
    eng.close()
    assert R["rounds"] == 3 and len(recs) == 3
    rel = lambda a, b: abs(a - b) / abs(b)
    dev = dict(cost=0.0, cost_new=0.0)
    for r, rec in enumerate(recs):
        print(f"MEASURE round {r}: device cost {R['cost'][0, r]:.17g} -> {R['cost_new'][0, r]:.17g} s {R['s'][0, r]} n_free "
              f"{R['n_free'][0, r]} cg {V.Engine2D.CG_STATUS[R['cg_status'][0, r]]} in {R['cg_steps'][0, r]} pinned "
              f"{R['pinned'][0, r]} clipped {R['clipped'][0, r]} halvings {R['halvings'][0, r]}; host cost {rec['cost']:.17g} -> "
              f"{rec['cost_new']:.17g} s {rec['s']} n_free {rec['n_free']} cg {rec['status']} in {rec['steps']}; rel. dev "
              f"{rel(R['cost'][0, r], rec['cost']):.2e} {rel(R['cost_new'][0, r], rec['cost_new']):.2e}")
        assert R["status"][0, r] == ACCEPTED and V.Engine2D.CG_STATUS[R["cg_status"][0, r]] == rec["status"]
        assert R["s"][0, r] == rec["s"] and R["n_free"][0, r] == rec["n_free"]
        assert abs(int(R["cg_steps"][0, r]) - rec["steps"]) <= 1
        dev["cost"] = max(dev["cost"], rel(R["cost"][0, r], rec["cost"]))
        dev["cost_new"] = max(dev["cost_new"], rel(R["cost_new"][0, r], rec["cost_new"]))
    dev["control"] = float(np.abs(u_dev - u3).max() / np.abs(u3).max())
    print(f"MEASURE against the host driver: {dev}")
    assert [int(R["n_free"][0, r]) for r in range(2)] == [273, 119]
    for key in dev:
        assert dev[key] <= TOL[key], key
    # the first round's recorded digits
    assert abs(R["cost"][0, 0] - 0.655718) <= 1e-6 and abs(R["cost_new"][0, 0] - 0.651414) <= 1e-6
    # the driver's device path: the same records
    ud, rd = G2.newton_refine(pr.cfg, ocfg, u0, pr.phi_Q, pr.phi_T, n_newton=3, on_device=True)
    assert np.array_equal(ud, u_dev) and ud.shape == u3.shape and len(rd) == 3
    for r, (a, b) in enumerate(zip(rd, recs)):
        assert set(a) == set(b)
        assert (a["status"], a["s"], a["n_free"]) == (b["status"], b["s"], b["n_free"]) and abs(a["steps"] - b["steps"]) <= 1
        assert a["cost"] == R["cost"][0, r] and a["cost_new"] == R["cost_new"][0, r] and a["rnorm0"] == R["rnorm0"][0, r]
        assert rel(a["rnorm0"], b["rnorm0"]) <= CLASS


# ---------------------------------------------------------------------------------------------------------------------
# 3. a batch of three against three single contexts
# ---------------------------------------------------------------------------------------------------------------------
def _three(pr):
    """Member 0: the case of test 2 under other weights; every round accepts the full step, and it sits out the halved
    trials of member 2.  Member 1: a sparsity parameter under which u0 = 0 has an empty free set (STATIONARY at round 0,
    the control untouched).  Member 2: the box-cut start (ACCEPTED at s = 1/32 after five halvings, then STATIONARY)."""
    V = pr.V
    cut, half = _box_cut(pr)
    opts = [V.make_opt(pr.ocfg, b1=2.0, b2=4.0, b3=1.0, u_min=-0.9, u_max=0.9),
            V.make_opt(pr.ocfg, kappa_sparsity=1e3, u_min=-0.5, u_max=0.5), cut]
    u0 = np.stack([pr.u + 0.75, np.zeros_like(pr.u), half])
    return opts, u0


def test_batch_of_three_equals_three_single_contexts(dense):
    pr = dense
    opts, u0 = _three(pr)
    n_rounds = 3
    eng = _pgd(pr, opts, u0)
    many = eng.pgd_newton(n_rounds)
    Um, Pm = eng.pgd_get("u"), eng.pgd_get("phi")
    eng.close()
    print(f"MEASURE batch: status {many['status'].tolist()} s {many['s'].tolist()} halvings {many['halvings'].tolist()} n_free "
          f"{many['n_free'].tolist()} pinned {many['pinned'].tolist()} clipped {many['clipped'].tolist()} cg {many['cg_status'].tolist()}")
    assert many["rounds"] == n_rounds
    assert many["status"][0].tolist() == [ACCEPTED] * 3 and many["s"][0].tolist() == [1.0] * 3 and not many["halvings"][0].any()
    assert many["status"][1].tolist() == [STATIONARY, IDLE, IDLE] and many["n_free"][1, 0] == 0 and many["rnorm0"][1, 0] == 0.0
    assert not Um[1].any() and np.isnan(many["cost"][1, 1:]).all() and np.isnan(many["s"][1]).all()
    assert many["status"][2].tolist() == [ACCEPTED, STATIONARY, IDLE] and many["n_free"][2].tolist() == [pr.u.size, 0, 0]
    assert many["s"][2, 0] == 1.0 / 32 and many["halvings"][2].tolist() == [5, 0, 0] and many["clipped"][2, 0] == pr.u.size
    assert (Um[2] == CUT).all() and many["cost_new"][2, 0] < many["cost"][2, 0]
    assert many["cost"][2, 1] == many["cost_new"][2, 0] == many["cost_new"][2, 1]
    for i in range(3):
        one = _pgd(pr, [opts[i]], u0[i][None])
        got = one.pgd_newton(n_rounds)
        U1, P1 = one.pgd_get("u"), one.pgd_get("phi")
        one.close()
        assert got["rounds"] == (3, 1, 2)[i]              # alone, a trajectory that has ended ends the call
        for key in OUT_KEYS:
            assert np.array_equal(got[key][0], many[key][i], equal_nan=True), (key, i)
        assert np.array_equal(U1, Um[i]) and np.array_equal(P1, Pm[i]), i


# ---------------------------------------------------------------------------------------------------------------------
# 4. state
# ---------------------------------------------------------------------------------------------------------------------
def test_a_call_that_accepts_nothing_leaves_the_pgd_run_undisturbed(dense):
    """Member 0 is stationary (empty free set), member 1 has b3 < 0 under which the Hessian is negative definite (NEGCURV
    at step 0), member 2 is the box-cut start, whose full step fails, under max_halvings = 0 (STALLED): nothing moves, and
    the iteration that follows is that of a run without the call."""
    pr, V = dense, dense.V
    cut, half = _box_cut(pr)
    opts = [V.make_opt(pr.ocfg, kappa_sparsity=1e3, u_min=-0.5, u_max=0.5), V.make_opt(pr.ocfg, b3=-1e-3, u_min=-2.0, u_max=2.0), cut]
    u0 = np.stack([np.zeros_like(pr.u), pr.u, half])
    plain = _pgd(pr, opts, u0)
    want = plain.pgd_iterate(1)
    u_want, phi_want = plain.pgd_get("u"), plain.pgd_get("phi")
    plain.close()
    eng = _pgd(pr, opts, u0)
    phi0 = eng.pgd_get("phi")
    R = eng.pgd_newton(2, max_halvings=0)
    assert R["rounds"] == 1 and R["status"][:, 0].tolist() == [STATIONARY, NEGCURV, STALLED] and R["cg_steps"][1, 0] == 0
    assert np.isnan(R["s"]).all() and np.array_equal(R["cost"][:, 0], R["cost_new"][:, 0])
    assert R["clipped"][:, 0].tolist() == [0, 0, pr.u.size] and R["halvings"][:, 0].tolist() == [0, 0, 0]
    assert np.array_equal(eng.pgd_get("u"), u0) and np.array_equal(eng.pgd_get("phi"), phi0)
    got = eng.pgd_iterate(1)
    for key in PGD_KEYS:
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(eng.pgd_get("u"), u_want) and np.array_equal(eng.pgd_get("phi"), phi_want)
    eng.close()


def test_halvings_stall_or_accept_at_the_bound(dense):
    """The box-cut start alone: three halvings are not enough, ten are (the fifth is accepted)."""
    pr = dense
    cut, half = _box_cut(pr)
    eng = _pgd(pr, [cut], half[None])
    R = eng.pgd_newton(2, max_halvings=3)
    assert R["rounds"] == 1 and R["status"][0].tolist() == [STALLED, IDLE] and R["halvings"][0, 0] == 3
    assert np.array_equal(eng.pgd_get("u"), half)
    R = eng.pgd_newton(2, max_halvings=10)             # a new call starts afresh: nobody is idle
    bound = R["cost"][0, 0] - 1e-4 * R["s"][0, 0] * R["pred"][0, 0]
    print(f"MEASURE box cut: cost {R['cost'][0, 0]:.17g} -> {R['cost_new'][0, 0]:.17g} at s {R['s'][0, 0]}, pred {R['pred'][0, 0]:.6e}, "
          f"gain / pred {(R['cost'][0, 0] - R['cost_new'][0, 0]) / R['pred'][0, 0]:.3e}")
    assert R["status"][0].tolist() == [ACCEPTED, STATIONARY] and R["s"][0, 0] == 1.0 / 32 and R["halvings"][0, 0] == 5
    assert R["cost_new"][0, 0] <= bound
    assert R["cost"][0, 0] - R["cost_new"][0, 0] < 1e-4 * (2.0 / 32) * R["pred"][0, 0]        # s = 1/16 would have failed
    eng.close()


def test_the_rounds_leave_the_state_of_an_init_from_their_iterate(dense):
    pr, V = dense, dense.V
    _, box, u0 = _refine_case(pr)
    eng = _pgd(pr, [box], u0[None])
    R = eng.pgd_newton(2)
    assert R["status"][0].tolist() == [ACCEPTED, ACCEPTED]
    un, phin = eng.pgd_get("u"), eng.pgd_get("phi")
    # the cost of the resident state is the last accepted trial's
    J = eng.cost(None, un[None], pr.phi_Q[None], pr.phi_T[None], pr.t, box, pr.x, pr.y)
    assert J[4] == R["cost_new"][0, 1]
    # the Newton-CG vectors of the last round are resident, the calls about the base point work about the new iterate
    assert np.abs(eng.cg_vector("x")).max() > 0
    g = eng.exact_gradient(opt=box)
    assert np.isfinite(g).all()
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


def test_the_adjoint_of_the_replaced_iterate_is_invalid(dense):
    pr, V = dense, dense.V
    _, box, u0 = _refine_case(pr)
    eng = _pgd(pr, [box], u0[None], alpha0=1e-3)         # a short first step: the iterate keeps a free set
    eng.pgd_iterate(1)
    eng.pgd_kkt(refresh=False)                           # the sweep of the iteration left r resident
    R = eng.pgd_newton(1)
    assert R["status"][0, 0] == ACCEPTED
    with pytest.raises(V.VchError, match="-3"):
        eng.pgd_kkt(refresh=False)
    k = eng.pgd_kkt(refresh=True)
    assert k["total"][0] == pr.u.size
    eng.pgd_kkt(refresh=False)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors come before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_any_launch(dense):
    pr, V = dense, dense.V
    _, box, u0 = _refine_case(pr)
    fresh = _engine(V, pr.P, 1, max_steps=pr.M)
    c0 = fresh.counters()
    with pytest.raises(V.VchError, match="-3"):
        fresh.pgd_newton(1)
    with pytest.raises(V.VchError, match="-3"):
        fresh.newton_trial(1.0)
    assert fresh.counters() == c0
    fresh.close()
    eng = _pgd(pr, [box], u0[None])
    c0 = eng.counters()
    for bad in (dict(n_rounds=0), dict(n_rounds=-2), dict(k=0), dict(max_halvings=-1), dict(precond=2), dict(precond=-1),
                dict(cg_tol=np.nan), dict(cg_tol=np.inf)):
        args = dict(n_rounds=2)
        args.update(bad)
        with pytest.raises(ValueError):
            eng.pgd_newton(**args)
        assert eng.counters() == c0, bad
    # NULL outputs, at the C boundary
    lib = V.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    d, i32, i64 = np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(6, dtype=np.int64)
    full = [dp(d), dp(d), dp(d), dp(d), dp(d), ip(i32), ip(i32), ip(i32), ip(i32), i64.ctypes.data_as(C.POINTER(C.c_int64))]
    for hole in range(len(full)):
        outs = list(full)
        outs[hole] = None
        assert lib.vch2d_pgd_newton(eng.ctx, 2, 5, 1e-8, 1, 0.0, 0.0, 10, *outs, None) == -1, hole
        assert eng.counters() == c0, hole
    # the trial's seam: no resident vectors yet, then step lengths that are not finite or not positive
    with pytest.raises(V.VchError, match="-3"):
        eng.newton_trial(1.0)
    assert eng.counters() == c0
    eng.hess_cg(2, opt=[box])
    c1 = eng.counters()
    for s in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            eng.newton_trial(s)
        assert eng.counters() == c1, s
    assert lib.vch2d_newton_trial(eng.ctx, None, None, dp(d), i64.ctypes.data_as(C.POINTER(C.c_int64))) == -1
    assert eng.counters() == c1
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. allocation balance
# ---------------------------------------------------------------------------------------------------------------------
def test_the_allocation_balance(dense):
    pr, V = dense, dense.V
    lib = V.load()
    _, box, u0 = _refine_case(pr)
    base = lib.vch_mem_live()
    eng = _pgd(pr, [box], u0[None])
    live0 = lib.vch_mem_live()
    eng.hess_cg(3, opt=[box])
    m = lib.vch_mem_live() - live0
    eng.pgd_newton(2, k=3)
    eng.newton_trial(0.5, want_u=False)
    assert lib.vch_mem_live() - live0 == m               # the rounds run in the storage of hess_cg and the PGD scratch
    eng.close()
    assert lib.vch_mem_live() == base
    eng = _pgd(pr, [box], u0[None])
    eng.pgd_newton(1, k=3)
    assert lib.vch_mem_live() - live0 == m
    eng.close()
    assert lib.vch_mem_live() == base


# ---------------------------------------------------------------------------------------------------------------------
# 7. run_sweep(n_newton)
# ---------------------------------------------------------------------------------------------------------------------
def test_run_sweep_polishes_every_member(V):
    import test_gpu_sweep as S
    K2 = V.module("Vch_control_2D.config")
    G2 = V.module("Vch_control_2D.GD2_configured")
    cfg = K2.ForwardSolverConfig(Nx=S.NX, Ny=S.NY, Lx=S.LX, Ly=S.LY, T=S.M * S.DT, dt_initial=S.DT, tau=S.TAU)
    members = [K2.OptimizationConfig(**S.MEMBERS[n]) for n in S.NAMES]
    plain = G2.run_sweep(cfg, members, n_iter=S.N_ITER, return_controls=True)
    zero = G2.run_sweep(cfg, members, n_iter=S.N_ITER, return_controls=True, n_newton=0)
    parent_keys = {"costs", "alphas", "attempts", "changes", "tracking_error", "terminal_error", "iters", "seconds", "kkt", "phi_T",
                   "t_hist", "x", "y", "u"}
    assert set(plain) == set(zero) == parent_keys
    for key in parent_keys - {"seconds", "kkt", "iters"}:
        assert np.array_equal(plain[key], zero[key]), key
    assert plain["iters"] == zero["iters"]
    for key in plain["kkt"]:
        assert np.array_equal(plain["kkt"][key], zero["kkt"][key]), key
    res = G2.run_sweep(cfg, members, n_iter=S.N_ITER, return_controls=True, n_newton=2)
    assert set(res) == parent_keys | {"newton", "costs_newton"}
    for key in ("costs", "alphas", "attempts", "changes", "tracking_error", "terminal_error"):
        assert np.array_equal(res[key], plain[key]), key                 # the polish comes after the PGD iterations
    cn, N = res["costs_newton"], res["newton"]
    print(f"MEASURE sweep: costs_newton {cn.tolist()} status {N['status'].tolist()} s {N['s'].tolist()} n_free {N['n_free'].tolist()}")
    assert cn.shape == (len(members), 3) and np.isfinite(cn).all()
    assert np.array_equal(cn[:, 0], plain["costs"][:, -1])
    assert (np.diff(cn, axis=1) <= 0.0).all()
    moved = N["status"] == ACCEPTED
    assert np.array_equal(np.isfinite(N["s"]), moved)
    for b in range(len(members)):
        if not moved[b].any():
            assert np.array_equal(res["u"][b], plain["u"][b])
