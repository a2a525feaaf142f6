"""vch1d_hessvec on the GPU: the exact gradient field G = d(J1+J2+J3)/du and the Hessian-vector product H h of the discrete
1D cost by transposed tangent sweeps (k1d_hessvec, one persistent workgroup per direction), against CPU linear algebra
(tests/_adjoint_ref_1d.py: the oracle's Newton matrix transposed and its high-precision banded solve, pinned against the
tangent reference by test_adjoint_cpu_1d.py) and against the existing entry point vch1d_second_order.  The engine marches,
its state history is pulled and fed to the CPU reference: the engine's cyclic reduction on J^T is compared with a direct
solve on the same history, not with itself.

Cases, directions, starts and controls are those of test_gpu_second_order_1d.py (n32, n33_off, n1030, n2051: depths 0, 0,
1, 2; batch 3 = a white-noise direction, a smooth one, h == 0).

Measured on the MI355X / asserted (10 x measured, rounded up), the largest deviation over everything this file compares
at that depth.  Fields: relative max-norm against the CPU reference.  Identities: relative to the sum of the absolute
values of the terms of the node sum.
                grad                  hv                    identities
    depth 0     1.44e-15 / 1.5e-14    6.97e-16 / 7.0e-15    2.14e-16 / 2.2e-15    (n32, n33_off, the weights, the PGD iterate, N = 24)
    depth 1     1.58e-13 / 1.6e-12    6.22e-14 / 6.3e-13    2.89e-14 / 2.9e-13    (n1030)
    depth 2     2.04e-12 / 2.1e-11    8.92e-13 / 9.0e-12    7.79e-14 / 7.8e-13    (n2051)
The growth with N is the reference's own: its solve variants differ by 1e-11 at N ~ 1000-2000.
Every asserted value is orders below the CPU floors FLOOR_D1 = 1e-5 (fields) and FLOOR_S = 1e-5 (identities) of
test_tangent_cpu_1d.py; the assertion at import keeps a loose tolerance from hiding a wrong kernel.

Dense Hessian (N = 24, M = 2, 100 unit directions about one base point): asymmetry, deviation from the CPU reference's
matrix (both relative to max|H|) and of the eigenvalues (relative to the largest), measured / asserted:
5.89e-17 / 5.9e-16 (the reference's own asymmetry: 3.93e-17), 1.57e-16 / 1.6e-15, 1.24e-15 / 1.3e-14.
Driver (driver_problem(), box [-1, 1]): the extreme Ritz values of reduced_hessian_extremes after n_free steps against
eigvalsh of the dense masked Hessian, relative to the largest eigenvalue.  DRIVER_RITZ is not a measured bound but the
round-off of the method: Lanczos with full reorthogonalisation over the whole free set gives T = Q^T A Q with Q orthonormal
to a few eps, so its eigenvalues are those of A to O(n eps ||A||); with n = 231 nodes, eps = 2.3e-16 and a factor 10 that
is 5.2e-13 of the largest eigenvalue (the matrix's own asymmetry, 6e-17 per entry, is below that).  Measured on the
MI355X: 2.09e-16, 172 of 231 nodes free, 162 steps to an invariant subspace."""
import contextlib
import ctypes as C
import io
import math

import numpy as np
import pytest

from oracle import vch1d_oracle as o
from _adjoint_ref_1d import adjoint_reference_1d, trapz_nodes
from _tangent_ref_1d import DRIVER, driver_problem
from test_gpu_second_order_1d import CASES, WEIGHTS, V, _call, _engine, runs  # noqa: F401  (V, runs: fixtures)
from test_tangent_cpu_1d import FLOOR_D1, FLOOR_S

pytestmark = pytest.mark.gpu

#        depth: grad, hv, identities
TOL = {0: (1.5e-14, 7.0e-15, 2.2e-15), 1: (1.6e-12, 6.3e-13, 2.9e-13), 2: (2.1e-11, 9.0e-12, 7.8e-13)}
DENSE_SYM, DENSE_REF, DENSE_EIG = 5.9e-16, 1.6e-15, 1.3e-14
DRIVER_RITZ = 5.2e-13        # 10 x 231 x 2.3e-16, see the docstring
for _t in TOL.values():
    assert _t[0] <= FLOOR_D1 and _t[1] <= FLOOR_D1 and _t[2] <= FLOOR_S
assert max(DENSE_SYM, DENSE_REF) <= FLOOR_D1 and max(DENSE_EIG, DRIVER_RITZ) <= FLOOR_S


def _hv(pr, eng=None, h="H", **kw):
    args = dict(phi_hist=pr["phi"], u=pr["U"], phi_Q=pr["phi_Q"], phi_T=pr["phi_T"], dt=pr["dts"])
    opt = kw.pop("opt", pr["opt"])
    args.update(kw)
    return (eng or pr["eng"]).hessvec(pr["H"] if isinstance(h, str) else h, pr["t"], opt, **args)


def _weights(opt):
    return opt.b1, opt.b2, opt.b3


@pytest.fixture(scope="module")
def hv(runs):
    """Per case: the engine's batch-3 answer, the same directions about trajectory 1's base point, and the CPU reference on
    the engine's own history (computed once, shared, never modified)."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        pr = runs(name)
        res = _hv(pr)
        base = dict(phi_hist=pr["phi"][1], u=pr["U"][1], phi_Q=pr["phi_Q"][1], phi_T=pr["phi_T"][1])
        shared = _hv(pr, shared_base=True, **base)
        ref = [adjoint_reference_1d(pr["P"], pr["phi"][b], pr["t"], pr["x"], pr["U"][b], pr["phi_Q"][b], pr["phi_T"][b],
                                    *_weights(pr["opt"]), h=pr["H"][b], dts=pr["dts"]) for b in range(3)]
        cache[name] = dict(pr=pr, res=res, shared=shared, base=base, ref=ref)
        return cache[name]

    return get


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _dev(a, b, want):
    """|sum(a b) - want| relative to sum |a b|."""
    return abs(float(np.sum(a * b)) - float(want)) / float(np.sum(np.abs(a * b)))


def _same(a, b):
    for k in ("grad", "hv", "gh", "hHh"):
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name", list(CASES))
def test_fields_against_the_cpu_reference(hv, name):
    m = hv(name)
    pr, res = m["pr"], m["res"]
    assert np.abs(pr["phi"]).max() < 1.0 - o.DELTA_SEP - 0.1          # the clip the scheme ignores is inactive
    wg = max(_rel(res["grad"][b], m["ref"][b][0]) for b in range(3))
    wh = max(_rel(res["hv"][b], m["ref"][b][1]) for b in range(2))
    print(f"MEASURE {name} depth {pr['depth']}: grad {wg:.2e} hv {wh:.2e}; stats {res['stats']}")
    tg, th, _ = TOL[pr["depth"]]
    assert wg < tg
    assert wh < th
    assert res["grad"][:, 0].any() and res["hv"][0, 0].any()         # row 0: quadrature weight 0, yet it drives step 0
    assert res["stats"]["launches"] == 1 and res["stats"]["seconds"] > 0
    assert res["stats"]["linear_solves"] == 3 * 3 * pr["M"]


@pytest.mark.parametrize("name", list(CASES))
def test_identities_against_second_order(hv, name):
    m = hv(name)
    pr, res, sh = m["pr"], m["res"], m["shared"]
    H = pr["H"]
    so1, so2 = _call(pr, order=1), pr["res"]
    devs = {}
    for b in (0, 1):
        devs[f"gh{b}"] = _dev(res["grad"][b], H[b], so1["s_state"][b] + so1["s_ctrl"][b])
        devs[f"hHh{b}"] = _dev(H[b], res["hv"][b], (so2["c_gn"][b] + so2["c_state"][b]) + so2["c_ctrl"][b])
        devs[f"dot_gh{b}"] = _dev(res["grad"][b], H[b], res["gh"][b])
        devs[f"dot_hHh{b}"] = _dev(H[b], res["hv"][b], res["hHh"][b])
    # symmetry needs one base point for both directions: trajectory 1's
    devs["sym"] = _dev(H[1], sh["hv"][0], np.sum(H[0] * sh["hv"][1]))
    print(f"MEASURE {name} depth {pr['depth']}: identities " + " ".join(f"{k} {v:.2e}" for k, v in devs.items()))
    assert max(devs.values()) < TOL[pr["depth"]][2], devs
    assert res["gh"][2] == 0.0 and res["hHh"][2] == 0.0
    assert np.array_equal(sh["grad"][0], res["grad"][1]) and np.array_equal(sh["hv"][1], res["hv"][1])


@pytest.mark.parametrize("name", list(CASES))
def test_exact_zero_rows_and_trajectories(V, hv, name):
    m = hv(name)
    pr, res = m["pr"], m["res"]
    assert not res["hv"][2].any() and res["grad"][2].any()          # h == 0: H h exactly zero, the gradient is not
    w = trapz_nodes(pr["t"])[-1] * trapz_nodes(pr["x"])
    assert trapz_nodes(pr["t"])[0] == 0.0
    for b in range(3):
        assert np.array_equal(res["grad"][b, -1], pr["opt"].b3 * w * pr["U"][b, -1]), b
        assert np.array_equal(res["hv"][b, -1], pr["opt"].b3 * w * pr["H"][b, -1]), b
    assert res["grad"][0, -1].any() and res["hv"][0, -1].any()
    zero = _hv(pr, opt=V.make_opt(b3=0.0))
    assert not zero["grad"][:, -1].any() and not zero["hv"][:, -1].any() and zero["grad"][0, 0].any()


@pytest.mark.parametrize("name", list(CASES))
def test_batch_of_three_equals_three_single_contexts(V, hv, name):
    m = hv(name)
    pr, res = m["pr"], m["res"]
    for b in range(3):
        eng = _engine(V, pr["P"], 1)
        phi, _ = eng.forward(pr["phi0"][b], pr["dts"], u=pr["U"][b])
        assert np.array_equal(phi, pr["phi"][b])
        r = eng.hessvec(pr["H"][b], pr["t"], pr["opt"], u=pr["U"][b], phi_Q=pr["phi_Q"][b], phi_T=pr["phi_T"][b], dt=pr["dts"])
        eng.close()
        for k in ("grad", "hv", "gh", "hHh"):
            assert np.array_equal(r[k][0], res[k][b]), (k, b)


@pytest.mark.parametrize("name", list(CASES))
def test_shared_base_equals_the_tiled_base(hv, name):
    m = hv(name)
    pr = m["pr"]
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (3,) + a.shape))
    many = _hv(pr, **{k: tile(v) for k, v in m["base"].items()})
    _same(m["shared"], many)
    assert not np.array_equal(m["shared"]["grad"][0], m["res"]["grad"][0])      # another base point than trajectory 0's own


@pytest.mark.parametrize("name", list(CASES))
def test_order_one_is_the_gradient_of_order_two(hv, name):
    m = hv(name)
    pr, res = m["pr"], m["res"]
    r1 = _hv(pr, order=1)
    assert np.array_equal(r1["grad"], res["grad"]) and np.array_equal(r1["gh"], res["gh"])
    assert r1["hv"] is None and np.isnan(r1["hHh"]).all()
    assert r1["stats"]["linear_solves"] == 3 * pr["M"] and r1["stats"]["launches"] == 1
    g = pr["eng"].exact_gradient(pr["t"], pr["opt"], phi_hist=pr["phi"], u=pr["U"], phi_Q=pr["phi_Q"], phi_T=pr["phi_T"],
                                 dt=pr["dts"])
    assert np.array_equal(g, res["grad"])
    no_h = _hv(pr, h=None, order=1)
    assert np.array_equal(no_h["grad"], res["grad"]) and np.isnan(no_h["gh"]).all()


def test_per_trajectory_weights_against_the_scalar_form(V, hv):
    m = hv("n33_off")
    pr = m["pr"]
    opts = [V.make_opt(b1=w[0], b2=w[1], b3=w[2]) for w in WEIGHTS]
    many = _hv(pr, opt=opts)
    worst = np.zeros(2)
    for b, w in enumerate(WEIGHTS):
        one = _hv(pr, opt=opts[b])
        for k in ("grad", "hv", "gh", "hHh"):
            assert np.array_equal(many[k][b], one[k][b]), (k, b)
        if b < 2:
            G, Hh = adjoint_reference_1d(pr["P"], pr["phi"][b], pr["t"], pr["x"], pr["U"][b], pr["phi_Q"][b], pr["phi_T"][b],
                                         *w, h=pr["H"][b], dts=pr["dts"])
            worst = np.maximum(worst, (_rel(many["grad"][b], G), _rel(many["hv"][b], Hh)))
    print(f"MEASURE weights depth 0: grad {worst[0]:.2e} hv {worst[1]:.2e}")
    assert worst[0] < TOL[0][0] and worst[1] < TOL[0][1]
    assert not np.array_equal(many["grad"][1], m["res"]["grad"][1])            # other weights than the defaults


def test_resident_history_after_forward(V, hv):
    m = hv("n1030")
    pr = m["pr"]
    eng = _engine(V, pr["P"], 3)
    phi, _ = eng.forward(pr["phi0"], pr["dts"], u=pr["U"])
    assert np.array_equal(phi, pr["phi"])
    res = _hv(pr, eng=eng, phi_hist=None)
    eng.close()
    _same(res, m["res"])


@pytest.fixture(scope="module")
def dense(V):
    """N = 24, M = 2: the full Hessian about one base point from rows * (N+1) unit directions in one batch, and the CPU
    reference's."""
    P = o.Params1D(N=24, T=0.02, dt_initial=0.01)
    tg, dts = V.time_grid(P.T, P.dt_initial)
    t = np.concatenate([[0.0], tg])
    rows, n = len(t), P.N + 1
    x = np.linspace(0.0, P.Lx, n)
    u = 9.0 * np.stack([np.cos(np.pi * x * (1 + k % 3)) * np.sin(1 + k) for k in range(rows)])
    one = _engine(V, P, 1)
    phi, _ = one.forward(0.2 * np.cos(np.pi * x), np.asarray(dts), u=u)
    one.close()
    phi_T, phi_Q = o.build_targets(x, t, phi[0], P.Lx, P.T)
    nd = rows * n
    E = np.eye(nd).reshape(nd, rows, n)
    eng = _engine(V, P, nd)
    opt = V.make_opt()
    res = eng.hessvec(E, t, opt, phi_hist=phi, u=u, phi_Q=phi_Q, phi_T=phi_T, dt=np.asarray(dts), shared_base=True)
    eng.close()
    Hm = res["hv"].reshape(nd, nd).T                                 # column j = H e_j
    ref = [adjoint_reference_1d(P, phi, t, x, u, phi_Q, phi_T, opt.b1, opt.b2, opt.b3, h=E[j], dts=dts) for j in range(nd)]
    Hr = np.stack([r[1].ravel() for r in ref], axis=1)
    return dict(Hm=Hm, Hr=Hr, grad=res["grad"], Gr=ref[0][0], rows=rows, n=n)


def test_dense_hessian_is_symmetric_and_the_references(dense):
    Hm, Hr = dense["Hm"], dense["Hr"]
    assert dense["rows"] == 4 and Hm.shape == (100, 100)
    scale = np.abs(Hr).max()
    sym, dev = np.abs(Hm - Hm.T).max() / scale, np.abs(Hm - Hr).max() / scale
    ev, er = np.linalg.eigvalsh(0.5 * (Hm + Hm.T)), np.linalg.eigvalsh(0.5 * (Hr + Hr.T))
    eig = np.abs(ev - er).max() / np.abs(er).max()
    print(f"MEASURE dense: asymmetry {sym:.2e} (reference's own {np.abs(Hr - Hr.T).max() / scale:.2e}) vs reference {dev:.2e} "
          f"eigenvalues {eig:.2e}; spectrum {er[0]:.3e} .. {er[-1]:.3e}")
    assert sym < DENSE_SYM
    assert dev < DENSE_REF
    assert eig < DENSE_EIG
    for b in (0, 57, 99):                                            # the gradient does not depend on the direction
        assert np.array_equal(dense["grad"][b], dense["grad"][0])
    print(f"MEASURE dense depth 0: grad {_rel(dense['grad'][0], dense['Gr']):.2e}")
    assert _rel(dense["grad"][0], dense["Gr"]) < TOL[0][0]


def test_driver_level_reduced_hessian_extremes(V):
    """reduced_hessian_extremes on driver_problem(): (a) with the box [-1, 1] the clipped control gives a proper free set,
    and after n_free Lanczos steps the smallest Ritz value is the smallest eigenvalue of the dense masked Hessian; (b) with
    a box the control stays inside and kappa above |r*|, every direction exact_second_order_condition draws is supported on
    the free set (kink nodes pinned), and no curvature it reports is below the smallest Ritz value."""
    S1 = V.module("Vch_control_1D.second_order_conditions")
    K1 = V.module("Vch_control_1D.config")
    D = DRIVER
    P, phi0, u_star, r_star = driver_problem()
    cfg = K1.ForwardSolverConfig(N=P.N, T=P.T, dt_initial=P.dt_initial)
    tg, dts = V.time_grid(P.T, P.dt_initial)
    t = np.concatenate([[0.0], tg])
    x = np.linspace(0.0, P.Lx, P.N + 1)
    O = o.OptParams1D()
    one = _engine(V, P, 1)
    phi_star = one.forward(phi0, np.asarray(dts), u=u_star)[0]
    one.close()
    assert np.abs(phi_star).max() < 1.0 - o.DELTA_SEP - 0.1
    phi_T, phi_Q = o.build_targets(x, t, phi_star[0], P.Lx, P.T)
    nd = u_star.size
    eng = _engine(V, P, nd)
    opt = V.make_opt(b1=O.b1, b2=O.b2, b3=O.b3, kappa_sparsity=0.0)
    E = np.eye(nd).reshape((nd,) + u_star.shape)
    Hm = eng.hessvec(E, t, opt, phi_hist=phi_star, u=u_star, phi_Q=phi_Q, phi_T=phi_T, x=x, shared_base=True)["hv"]
    eng.close()
    Hm = Hm.reshape(nd, nd).T
    Hm = 0.5 * (Hm + Hm.T)
    args = (cfg, u_star, phi_star, x, t, O.b1, O.b2, O.b3)
    # (a) the box of the driver problem
    mask = S1.free_set(u_star, D["u_min"], D["u_max"]).ravel()
    assert 0 < mask.sum() < nd and (np.abs(u_star) >= D["u_max"] - 1e-8).any() and (np.abs(u_star) <= 1e-8).any()
    ev = np.linalg.eigvalsh(Hm[np.ix_(mask, mask)])
    R = S1.reduced_hessian_extremes(*args, O.kappa_sparsity, phi_Q, phi_T, D["u_min"], D["u_max"], k=nd, seed=D["seed"])
    dev = max(abs(R["theta_min"] - ev[0]), abs(R["theta_max"] - ev[-1])) / abs(ev[-1])
    print(f"MEASURE driver: n_free {R['n_free']} of {nd}, steps {R['steps']}, theta_min {R['theta_min']:.6e} eigvalsh {ev[0]:.6e} "
          f"theta_max {R['theta_max']:.6e} eigvalsh {ev[-1]:.6e} rel.dev {dev:.2e}, residuals {R['res_min']:.1e} {R['res_max']:.1e}")
    assert R["n_free"] == mask.sum() and R["steps"] <= R["n_free"]
    assert dev < DRIVER_RITZ
    few = S1.reduced_hessian_extremes(*args, O.kappa_sparsity, phi_Q, phi_T, D["u_min"], D["u_max"], k=12, seed=D["seed"])
    assert few["steps"] == 12 and ev[0] <= few["theta_min"] + DRIVER_RITZ * abs(ev[-1]) and few["theta_max"] <= ev[-1] * (1 + DRIVER_RITZ)
    assert np.abs(ev - few["theta_max"]).min() <= few["res_max"] + DRIVER_RITZ * abs(ev[-1])   # an eigenvalue within the residual
    # (b) a box that is nowhere active, kappa above |r* + b3 u*|: the kink nodes are pinned, the others free
    wide, kap, nd_dirs = 2.0, 1.0, D["num_directions"]
    assert np.abs(r_star + O.b3 * u_star).max() < kap
    free = S1.free_set(u_star, -wide, wide)
    rng = np.random.default_rng(D["seed"])
    dirs = [S1._generate_direction(u_star, r_star, -wide, wide, kap, O.b3, rng) for _ in range(nd_dirs)]
    assert all(not h[~free].any() and abs(np.linalg.norm(h) - 1.0) < 1e-12 for h in dirs) and not free.all()
    with contextlib.redirect_stdout(io.StringIO()):
        exact = S1.exact_second_order_condition(cfg, u_star, r_star, phi_star, x, t, O.b1, O.b2, O.b3, kap, phi_Q, phi_T,
                                                -wide, wide, num_directions=nd_dirs, seed=D["seed"])
    Rw = S1.reduced_hessian_extremes(*args, kap, phi_Q, phi_T, -wide, wide, k=nd, seed=D["seed"])
    print(f"MEASURE driver wide box: theta_min {Rw['theta_min']:.6e} curvatures {exact}")
    assert Rw["n_free"] == free.sum()
    assert all(Rw["theta_min"] <= c for c in exact)
    assert abs(Rw["theta_min"] - np.linalg.eigvalsh(Hm[np.ix_(free.ravel(), free.ravel())])[0]) < DRIVER_RITZ * abs(ev[-1])


def test_resident_pgd_state_and_undisturbed_iterations(V):
    """After pgd_init + 2 iterations: RESIDENT control and targets equal passing pgd_get("u" / "phi" / "phi_Q") and phi_T
    explicitly, and two further iterations are bit for bit those of an uninterrupted 4-iteration run."""
    N, T, dt = 32, 0.05, 0.01
    P = o.Params1D(N=N, T=T, dt_initial=dt)
    tg, dts = V.time_grid(T, dt)
    t = np.concatenate([[0.0], tg])
    x = np.linspace(0.0, 1.0, N + 1)
    phi0 = np.stack([0.2 * np.cos(np.pi * x + 0.4 * b) for b in range(2)])
    phi_T = np.stack([0.7 * np.sin(2 * np.pi * x), 0.5 * np.cos(2 * np.pi * x)])
    opt = V.make_opt(b1=0.3, b2=13.0, b3=0.0019, kappa_sparsity=9e-5, alpha_max=100.0)
    noise = np.random.default_rng(5).standard_normal((2, len(t), N + 1))
    H = noise / np.abs(noise).max()

    def start():
        eng = _engine(V, P, 2)
        eng.pgd_init(phi0, phi_T, t, dts, opt)
        return eng, eng.pgd_iterate(2)

    plain, _ = start()
    want = plain.pgd_iterate(2)
    u_want = plain.pgd_get("u")
    plain.close()
    eng, _ = start()
    u, phi, phi_Q, r = eng.pgd_get("u"), eng.pgd_get("phi"), eng.pgd_get("phi_Q"), eng.pgd_get("r")
    assert np.abs(u).max() > 0
    R = eng.RESIDENT
    res = eng.hessvec(H, t, opt, u=R, phi_Q=R, phi_T=R, dt=dts)
    explicit = eng.hessvec(H, t, opt, phi_hist=phi, u=u, phi_Q=phi_Q, phi_T=phi_T, dt=dts)
    _same(res, explicit)
    worst = np.zeros(2)
    for k, a in (("u", u), ("phi", phi), ("r", r), ("phi_Q", phi_Q)):
        assert np.array_equal(eng.pgd_get(k), a), k
    for b in range(2):
        G, Hh = adjoint_reference_1d(P, phi[b], t, x, u[b], phi_Q[b], phi_T[b], opt.b1, opt.b2, opt.b3, h=H[b], dts=dts)
        worst = np.maximum(worst, (_rel(res["grad"][b], G), _rel(res["hv"][b], Hh)))
    print(f"MEASURE pgd depth 0: grad {worst[0]:.2e} hv {worst[1]:.2e}")
    assert worst[0] < TOL[0][0] and worst[1] < TOL[0][1]
    got = eng.pgd_iterate(2)
    for k in ("cost", "alpha", "trials", "change", "tracking_error", "terminal_error"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(eng.pgd_get("u"), u_want)
    eng.close()


def test_error_codes_come_before_any_launch(V, hv):
    m = hv("n32")
    pr = m["pr"]
    eng, H, t, opt = pr["eng"], pr["H"], pr["t"], pr["opt"]
    fresh = _engine(V, pr["P"], 3)
    with pytest.raises(V.VchError, match="-3"):                      # no resident history
        fresh.hessvec(H, t, opt)
    with pytest.raises(V.VchError, match="-3"):                      # RESIDENT before pgd_init
        _hv(pr, eng=fresh, u=fresh.RESIDENT)
    with pytest.raises(V.VchError, match="-3"):
        _hv(pr, eng=fresh, phi_T=fresh.RESIDENT)
    fresh.forward(pr["phi0"], pr["dts"][:-1], u=pr["U"][:, :-1])
    with pytest.raises(V.VchError, match="-3"):                      # a resident history with another number of rows
        fresh.hessvec(H, t, opt)
    fresh.close()
    bad_dt = pr["dts"].copy()
    bad_dt[1] = 0.0
    neg_dt = pr["dts"].copy()
    neg_dt[0] = -0.01
    inf_dt = pr["dts"].copy()
    inf_dt[0] = math.inf
    t_back = t.copy()
    t_back[3] = t_back[2]
    big = eng.max_steps + 3
    bad = [
        (dict(opt=[opt, opt]), "n_opts"),
        (dict(order=3), "order"),
        (dict(order=0), "order"),
        (dict(dt=bad_dt), "dt"),
        (dict(dt=neg_dt), "dt"),
        (dict(dt=inf_dt), "dt"),
        (dict(opt=V.make_opt(b1=math.nan)), "b1, b2, b3"),
        (dict(opt=[opt, opt, V.make_opt(b3=math.inf)]), "trajectory 2"),
        (dict(h=None, order=2), "NULL direction"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            _hv(pr, **kw)
    with pytest.raises(ValueError, match="dt"):                      # dt derived from a t_hist that does not advance
        eng.hessvec(H, t_back, opt, phi_hist=pr["phi"])
    # what the wrapper cannot express goes through the C ABI itself
    lib, D = eng.lib, C.POINTER(C.c_double)
    dp = lambda a: a.ctypes.data_as(D)
    shape = (3, pr["rows"], eng.n)
    grad, hvo, dots = np.full(shape, 7.0), np.full(shape, 7.0), np.full((3, 2), 7.0)
    stats = V.module("_lib").Stats()
    stats.launches = 77
    last_error = V.module("_lib").last_error
    arr = (type(opt) * 1)(opt)
    hbig, tbig = np.zeros((3, big, eng.n)), np.linspace(0.0, 1.0, big)

    def raw(phi=pr["phi"], n_base=3, h=H, rows=pr["rows"], tt=t, x=pr["x"], hv_=hvo, order=2, n_opts=1, pq=dp(pr["phi_Q"])):
        return lib.vch1d_hessvec(eng.ctx, dp(phi), dp(pr["U"]), n_base, None if h is None else dp(h), rows, dp(pr["dts"]),
                                 None if tt is None else dp(tt), None if x is None else dp(x), pq, dp(pr["phi_T"]), arr,
                                 n_opts, order, dp(grad), None if hv_ is None else dp(hv_), dp(dots), C.byref(stats))

    resident = C.cast(C.c_void_p(1), D)
    for kw, code, what in [(dict(rows=2), -1, "rows"), (dict(rows=big, h=hbig, tt=tbig), -1, "rows"),
                           (dict(n_base=2), -1, "n_base"), (dict(n_opts=2), -1, "n_opts"), (dict(order=5), -1, "order"),
                           (dict(h=None), -1, "NULL direction"), (dict(hv_=None), -1, "NULL hv_out"),
                           (dict(tt=None), -1, "NULL t_hist"), (dict(x=None), -1, "NULL x"),
                           (dict(pq=resident), -3, "before vch1d_pgd_init")]:
        assert raw(**kw) == code, kw.keys()
        assert what in last_error() and "vch1d_hessvec" in last_error(), (what, last_error())
    assert (grad == 7.0).all() and (hvo == 7.0).all() and (dots == 7.0).all() and stats.launches == 77
    # order 1 needs neither h nor hv_out
    assert raw(h=None, hv_=None, order=1) == 0 and stats.launches == 1 and stats.linear_solves == 3 * pr["M"]
    assert np.array_equal(grad, m["res"]["grad"]) and (hvo == 7.0).all() and np.isnan(dots).all()
    # ... and the context still answers, with the bits of the first call
    _same(_hv(pr), m["res"])
