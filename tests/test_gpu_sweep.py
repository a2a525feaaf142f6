"""Per-trajectory optimisation parameters, warm start and the on-device KKT statistic of the 2D PGD loop
(vch2d_pgd_init_v, vch2d_pgd_kkt, Engine2D.pgd_init(opt=[...], u0, alpha0), Engine2D.pgd_kkt, GD2_configured.run_sweep).

The PGD cases run on the FFT grid and parameter corner of tests/test_gpu_forms.py (64 x 32 intervals on 1.0 x 0.5,
tau 1e-3, dt 1e-2, M = 4; seed 42, amplitude 0.1; 3 iterations).  Four members start from the SAME phi0, so whatever
differs between them comes from their parameters.  oracle.vch2d_oracle.pgd on them (CPU):

    member   OptParams (others default)                          attempts   smallest rel. gap    exact zeros   nodes at a
                                                                            judged / incumbent   in u          bound
    default  -                                                   0,0,0      1.4e-3               24 %          0
    weights  b1 0.5, b2 40, kappa_sparsity 5e-3, alpha_max 20    0,0,0      1.4e-3               68 %          0.4 %
    box      u_min -0.05, u_max 0.02, alpha_max 5                0,0,0      4.4e-5               24 %          7 % / 15 %
    wide     alpha_max 4000, u_min -100, u_max 100, b3 1e-3      0,10,10    2.1e-3               25 %          0

(gaps over the optimistic steps and the backtracking trials alike).  test_sweep_inputs_qualify asserts the properties of
this table that the GPU tests lean on.

Mutants applied by hand to the kernels, and the tests of this file that failed under each:
  * row 0 of the parameter table for every trajectory in k_grad_prox: test_mixed_parameters_equal_single_runs,
    test_mixed_parameters_vs_oracle, test_kkt_counts_match_numpy, test_kkt_masks_padding (both grids);
  * the same in the adjoint source (k_adj_rhs): test_mixed_parameters_equal_single_runs,
    test_mixed_parameters_vs_oracle, test_kkt_counts_match_numpy;
  * the padding mask dropped in k_kkt_count (run on test_kkt_masks_padding only, whose contexts keep one spare history
    level so that the unmasked reads stay inside the allocation): test_kkt_masks_padding (both grids).
(test_warm_start_continues_the_run and test_run_sweep_mirror compare batch runs with batch runs and pass under the first two.)
"""
import ctypes as C

import numpy as np
import pytest

from conftest import relerr

gpu = pytest.mark.gpu
SOLVE = 1e-9
M, N_ITER = 4, 3
NX, NY, LX, LY = 64, 32, 1.0, 0.5
TAU, DT = 1e-3, 1e-2
MEMBERS = {
    "default": {},
    "weights": dict(b1=0.5, b2=40.0, kappa_sparsity=5e-3, alpha_max=20.0),
    "box": dict(u_min=-0.05, u_max=0.02, alpha_max=5.0),
    "wide": dict(alpha_max=4000.0, u_min=-100.0, u_max=100.0, b3=1e-3),
}
NAMES = tuple(MEMBERS)
OUT_KEYS = ("cost", "alpha", "attempts", "change")


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


@pytest.fixture(scope="module")
def O2():
    from oracle import vch2d_oracle
    return vch2d_oracle


def _params(O2):
    return O2.Params2D(Nx=NX, Ny=NY, Lx=LX, Ly=LY, T=M * DT, dt_initial=DT, tau=TAU)


def _opts(O2):
    return [O2.OptParams(**MEMBERS[n]) for n in NAMES]


_REFS = {}


def _refs(O2):
    """O2.pgd (3 iterations) per member, with every cost the loop evaluated."""
    if not _REFS:
        P = _params(O2)
        orig = O2.cost
        for n, O in zip(NAMES, _opts(O2)):
            costs = []

            def recording(*args, **kw):
                costs.append(orig(*args, **kw))
                return costs[-1]
            O2.cost = recording
            try:
                r = O2.pgd(P, O, n_iter=N_ITER)
            finally:
                O2.cost = orig
            _REFS[n] = (r, costs)
    return _REFS


def test_sweep_inputs_qualify(O2):
    """No member's line search sits on an accept / reject tie: every cost a candidate was judged by differs from its
    incumbent's by more than 1e-5 relative (a hundred times the 1e-7 the costs are compared to); `wide` backtracks;
    `weights` and `box` end with exact zeros and `box` with nodes at both bounds."""
    R = _refs(O2)
    for n, O in zip(NAMES, _opts(O2)):
        r, costs = R[n]
        assert len(r.costs) == N_ITER + 1 and costs[0] == r.costs[0]
        assert len(costs) == 1 + sum(1 + a for a in r.attempts), (n, len(costs), r.attempts)
        i, gap = 1, np.inf
        for k, att in enumerate(r.attempts):
            inc = r.costs[k]
            for cnd in costs[i:i + 1 + att]:                     # the optimistic step, then the backtracking trials
                gap = min(gap, abs(cnd - inc) / inc)
                assert abs(cnd - inc) > 1e-5 * inc, (n, k, cnd, inc)
            i += 1 + att
            assert costs[i - 1] == r.costs[k + 1]
        zeros = float(np.mean(r.u == 0.0))
        lo, hi = float(np.mean(r.u == O.u_min)), float(np.mean(r.u == O.u_max))
        print(f"{n}: attempts {r.attempts} smallest gap {gap:.1e} zeros {zeros:.2%} at bounds {lo:.2%} / {hi:.2%}")
        if n == "wide":
            assert max(r.attempts) > 0
        if n in ("weights", "box"):
            assert zeros > 0
        if n == "box":
            assert lo > 0 and hi > 0


def _problem(O2):
    P = _params(O2)
    t, _ = O2.time_grid(P.T, P.dt_initial)
    phi0 = O2.init_phi_random(NX, NY, 1e-2, amp=0.1, seed=42)
    x, y = np.linspace(0.0, LX, NX + 1), np.linspace(0.0, LY, NY + 1)
    phi_T, phi_Q = O2.build_targets(x, y, t, phi0, LX, LY, P.T)
    return P, t, phi0, phi_T, phi_Q, x, y


def _engine(V, batch, max_steps=M):
    return V.Engine2D(Nx=NX, Ny=NY, Lx=LX, Ly=LY, tau=TAU, batch=batch, max_steps=max_steps)


def _tile(a, B):
    return np.repeat(np.asarray(a)[None], B, axis=0)


def _init_batch(V, O2, e, **kw):
    P, t, phi0, phi_T, _, _, _ = _problem(O2)
    B = len(NAMES)
    return e.pgd_init(_tile(phi0, B), _tile(phi_T, B), t, [V.make_opt(o) for o in _opts(O2)], ramp=True, T=P.T, **kw)


_RUN = {}


def _batch_run(V, O2):
    """The four members as one batch: init, 3 iterations, u; then pgd_kkt(refresh=True) and u, r, phi pulled after it."""
    if not _RUN:
        e = _engine(V, len(NAMES))
        _RUN["J0"] = _init_batch(V, O2, e)
        _RUN["out"] = e.pgd_iterate(N_ITER)
        _RUN["u"] = e.pgd_get("u")
        _RUN["kkt"] = e.pgd_kkt(refresh=True)
        _RUN["u_after"], _RUN["r_after"], _RUN["phi_after"] = e.pgd_get("u"), e.pgd_get("r"), e.pgd_get("phi")
        e.close()
    return _RUN


@gpu
def test_mixed_parameters_equal_single_runs(V, O2):
    """A member of the mixed batch computes the bits of a batch-1 context run with its parameters through the single-opt
    vch2d_pgd_init: J0, costs, step lengths, attempts, changes, the control, the KKT counts and the stationarity."""
    R = _batch_run(V, O2)
    P, t, phi0, phi_T, _, _, _ = _problem(O2)
    for b, O in enumerate(_opts(O2)):
        e = _engine(V, 1)
        J0 = e.pgd_init(phi0, phi_T, t, V.make_opt(O), ramp=True, T=P.T)
        out = e.pgd_iterate(N_ITER)
        u = e.pgd_get("u")
        k = e.pgd_kkt(refresh=True)
        e.close()
        print(f"{NAMES[b]}: attempts {out['attempts'][0]} cost {out['cost'][0]} / {R['out']['cost'][b]} "
              f"counts {[int(k[n][0]) for n in ('n_zero', 'n_small', 'n_match')]} stationarity {k['stationarity'][0]!r}"
              f" / {R['kkt']['stationarity'][b]!r}")
        assert np.array_equal(J0[0], R["J0"][b]), (J0, R["J0"][b])
        for key in OUT_KEYS:
            assert np.array_equal(out[key][0], R["out"][key][b]), (NAMES[b], key, out[key][0], R["out"][key][b])
        assert np.array_equal(u, R["u"][b])
        for key in ("n_zero", "n_small", "n_match", "total"):
            assert int(k[key][0]) == int(R["kkt"][key][b]), (NAMES[b], key)
        assert k["stationarity"][0] == R["kkt"]["stationarity"][b]


@gpu
def test_mixed_parameters_vs_oracle(V, O2):
    """The mixed batch against O2.pgd per member, with the assertions of test_mixed_batch_pgd_vs_oracle."""
    R, refs = _batch_run(V, O2), _refs(O2)
    J0, out, u = R["J0"], R["out"], R["u"]
    for b, n in enumerate(NAMES):
        r = refs[n][0]
        print(f"pgd {n}: attempts {out['attempts'][b]} / {r.attempts} cost {out['cost'][b]} / {r.costs} "
              f"alpha {out['alpha'][b]} / {r.alphas} u {relerr(u[b], r.u):.1e} J0 {abs(J0[b, 4] / r.costs[0] - 1):.1e}")
    for b, n in enumerate(NAMES):
        r = refs[n][0]
        assert abs(J0[b, 4] / r.costs[0] - 1) < 1e-10
        assert list(out["attempts"][b]) == list(r.attempts), (out["attempts"][b], r.attempts)
        assert np.allclose(out["alpha"][b], r.alphas, rtol=1e-12, atol=0), (out["alpha"][b], r.alphas)
        assert np.allclose(out["cost"][b], r.costs[1:], rtol=1e-7, atol=0), (out["cost"][b], r.costs)
        assert relerr(u[b], r.u) < 1e-6


def _np_kkt(V, O2, u, r, O, tol=1e-6):
    S2 = V.module("Vch_control_2D.second_order_conditions_2d")
    counts = S2.sparsity_statistics(u, r, O.kappa_sparsity, tol)
    un = O2.prox_step(u, O2.gradient(r, u, O), 1.0, O)
    return counts, float(np.linalg.norm(un - u) / (np.linalg.norm(u) + 1e-9))


def _assert_kkt(V, O2, k, u, r, opts, tol=1e-6):
    for b, O in enumerate(opts):
        counts, stat = _np_kkt(V, O2, u[b], r[b], O, tol)
        got = tuple(int(k[n][b]) for n in ("n_zero", "n_small", "n_match", "total"))
        print(f"kkt {b}: counts {got} / {counts} stationarity {k['stationarity'][b]:.15e} / {stat:.15e}")
        assert got == counts, (b, got, counts)
        assert np.allclose(k["pct"][b], [100.0 * c / counts[3] for c in counts[:3]], rtol=1e-15, atol=0)
        assert abs(k["stationarity"][b] - stat) <= 1e-12 * stat, (b, k["stationarity"][b], stat)


@gpu
def test_kkt_counts_match_numpy(V, O2):
    """pgd_kkt(refresh=True) after the three iterations: the counts are exactly sparsity_statistics of the control and
    adjoint pulled after the call, the stationarity is NumPy's prox step with alpha = 1 on them, and the refreshed adjoint
    is that of the resident state under each member's own b1, b2.  refresh=False needs a sweep since the init, leaves the
    following iteration bit-identical; refresh=True leaves it identical up to the adjoint's solve tolerance."""
    R = _batch_run(V, O2)
    P, t, phi0, phi_T, phi_Q, _, _ = _problem(O2)
    opts = _opts(O2)
    B = len(opts)
    assert np.array_equal(R["u_after"], R["u"]) and np.all(R["kkt"]["total"] == (M + 1) * 65 * 33)
    _assert_kkt(V, O2, R["kkt"], R["u_after"], R["r_after"], opts)
    e1 = _engine(V, 1)
    for b, O in enumerate(opts):
        _, _, r1, _ = e1.backward(R["phi_after"][b], t, O.b1, O.b2, phi_Q=phi_Q, phi_T=phi_T)
        print(f"refreshed r {NAMES[b]}: {relerr(R['r_after'][b], r1):.1e}")
        assert relerr(R["r_after"][b], r1) < SOLVE
    e1.close()
    runs = {}
    for mode in ("plain", "resident", "refresh"):
        e = _engine(V, B)
        _init_batch(V, O2, e)
        if mode == "plain":
            with pytest.raises(V.VchError, match="engine error -3"):
                e.pgd_kkt(refresh=False)
        first = e.pgd_iterate(1)
        if mode != "plain":
            k = e.pgd_kkt(refresh=(mode == "refresh"))
            _assert_kkt(V, O2, k, e.pgd_get("u"), e.pgd_get("r"), opts)
        runs[mode] = (first, e.pgd_iterate(1), e.pgd_get("u"))
        e.close()
    for mode in ("resident", "refresh"):
        for key in OUT_KEYS:
            assert np.array_equal(runs[mode][0][key], runs["plain"][0][key])
    for key in OUT_KEYS:
        assert np.array_equal(runs["resident"][1][key], runs["plain"][1][key]), key
    assert np.array_equal(runs["resident"][2], runs["plain"][2])
    print(f"refresh between two calls: cost {runs['refresh'][1]['cost'][:, 0]} / {runs['plain'][1]['cost'][:, 0]}")
    assert np.array_equal(runs["refresh"][1]["attempts"], runs["plain"][1]["attempts"])
    assert np.array_equal(runs["refresh"][1]["alpha"], runs["plain"][1]["alpha"])
    assert np.allclose(runs["refresh"][1]["cost"], runs["plain"][1]["cost"], rtol=1e-7, atol=0)


@gpu
@pytest.mark.parametrize("Nx,Ny", [(70, 20), (20, 70)])
def test_kkt_masks_padding(V, O2, Nx, Ny):
    """The count kernel on the GEMM path with rows padded to the pitch and tiles that overhang both extents: a warm start
    from a control with exact zeros, values on either side of tol and saturated nodes on the last row, the last column and
    the tile seams of the engine's plane (Ny+1 rows of Nx+1 entries over the flat array) is counted exactly."""
    Mp, B, tol = 2, 3, 1e-6
    opts = [O2.OptParams(kappa_sparsity=ks, u_min=-0.05, u_max=0.02) for ks in (1e-4, 5e-3, 1.0)]
    P = O2.Params2D(Nx=Nx, Ny=Ny, Lx=1.0, Ly=1.0, T=Mp * DT, dt_initial=DT)
    t, _ = O2.time_grid(P.T, P.dt_initial)
    phi0 = O2.init_phi_random(Nx, Ny, 1e-2, amp=0.1, seed=42)
    x, y = np.linspace(0.0, 1.0, Nx + 1), np.linspace(0.0, 1.0, Ny + 1)
    phi_T, _ = O2.build_targets(x, y, t, phi0, 1.0, 1.0, P.T)
    nf, ns = Nx + 1, Ny + 1
    rng = np.random.default_rng(7)
    u0 = rng.uniform(-0.04, 0.015, (B, Mp + 1, ns, nf))             # the engine's view of the flat (Nx+1)(Ny+1) array
    marks = (0.0, 5e-7, -5e-7, 2e-6, -2e-6, -0.05, 0.02)
    rows = sorted({0, 15, 16, ns - 1} | ({31, 32, 63, 64} & set(range(ns))))
    cols = sorted({0, nf - 1} | ({63, 64} & set(range(nf))))
    for i, rr in enumerate(rows):
        for c in range(nf):
            u0[:, :, rr, c] = marks[(i + c) % len(marks)]
    for j, c in enumerate(cols):
        for rr in range(ns):
            u0[:, :, rr, c] = marks[(j + rr + 3) % len(marks)]
    u0 = u0.reshape(B, Mp + 1, Nx + 1, Ny + 1)
    # one spare history level: max_steps = Mp + 1
    e = V.Engine2D(Nx=Nx, Ny=Ny, batch=B, max_steps=Mp + 1)
    assert not e.uses_fft
    e.pgd_init(_tile(phi0, B), _tile(phi_T, B), t, [V.make_opt(o) for o in opts], ramp=True, T=P.T, u0=u0)
    k = e.pgd_kkt(refresh=True, tol=tol)
    u, r = e.pgd_get("u"), e.pgd_get("r")
    e.close()
    assert np.array_equal(u, u0)                                    # taken as given
    assert np.all(k["total"] == (Mp + 1) * (Nx + 1) * (Ny + 1))
    _assert_kkt(V, O2, k, u, r, opts, tol)
    assert 0 < k["n_zero"][0] < k["total"][0]
    assert k["n_small"][2] == k["total"][2] and np.abs(r[2]).max() <= 1.0


@gpu
def test_warm_start_continues_the_run(V, O2):
    """A context warm-started from the control after two iterations, with the step length the loop would use next, does
    the third iteration of the uninterrupted run; J0 under a start control is the oracle's cost of the march under it."""
    A = _batch_run(V, O2)
    opts = _opts(O2)
    B = len(opts)
    e = _engine(V, B)
    _init_batch(V, O2, e)
    mid = e.pgd_iterate(2)
    u2 = e.pgd_get("u")
    e.close()
    for key in OUT_KEYS:
        assert np.array_equal(mid[key], A["out"][key][:, :2])
    alpha0 = np.minimum(np.array([o.alpha_max for o in opts]), 1.2 * A["out"]["alpha"][:, 1])
    e = _engine(V, B)
    J0 = _init_batch(V, O2, e, u0=u2, alpha0=alpha0)
    out = e.pgd_iterate(1)
    u = e.pgd_get("u")
    e.close()
    P, t, phi0, phi_T, phi_Q, x, y = _problem(O2)
    for b, O in enumerate(opts):
        ph, _, _ = O2.forward(P, control=u2[b], phi0=phi0)
        Jo = O2.cost(ph, u2[b], phi_Q, phi_T, x, y, t, O)
        print(f"warm {NAMES[b]}: J0 {J0[b, 4]!r} / run A {A['out']['cost'][b, 1]!r} / oracle {Jo!r}; attempts "
              f"{out['attempts'][b, 0]} / {A['out']['attempts'][b, 2]} alpha {out['alpha'][b, 0]!r} / "
              f"{A['out']['alpha'][b, 2]!r} cost {out['cost'][b, 0]!r} / {A['out']['cost'][b, 2]!r} "
              f"u {relerr(u[b], A['u'][b]):.1e}")
    for b, O in enumerate(opts):
        ph, _, _ = O2.forward(P, control=u2[b], phi0=phi0)
        assert np.isclose(J0[b, 4], O2.cost(ph, u2[b], phi_Q, phi_T, x, y, t, O), rtol=1e-7, atol=0)
    assert np.allclose(J0[:, 4], A["out"]["cost"][:, 1], rtol=1e-7, atol=0)
    assert np.array_equal(out["attempts"][:, 0], A["out"]["attempts"][:, 2])
    assert np.array_equal(out["alpha"][:, 0], A["out"]["alpha"][:, 2])
    assert np.allclose(out["cost"][:, 0], A["out"]["cost"][:, 2], rtol=1e-7, atol=0)
    for b in range(B):
        assert relerr(u[b], A["u"][b]) < 1e-6


@gpu
def test_sweep_argument_errors(V, O2):
    """Bad parameter sets and calls out of order return an error code with a message, and launch nothing."""
    lib, _lib = V.load(), V.module("_lib")
    P, t, phi0, phi_T, _, x, y = _problem(O2)
    B = len(NAMES)
    e = _engine(V, B)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    p0, pT, J0 = _tile(phi0, B), _tile(phi_T, B), np.zeros((B, 5))
    cnt, stat = np.zeros((B, 4), dtype=np.int64), np.zeros(B)
    before = e.counters()

    def init(opts, n):
        arr = (_lib.OptParams * len(opts))(*[V.make_opt(o) for o in opts])
        return lib.vch2d_pgd_init_v(e.ctx, dp(p0), dp(pT), None, 1, P.T, dp(t), M, dp(x), dp(y), arr, n, None, None, dp(J0))

    assert lib.vch2d_pgd_kkt(e.ctx, 1, 1e-6, cnt.ctypes.data_as(C.POINTER(C.c_int64)), dp(stat)) == -3
    assert b"pgd_init" in lib.vch_last_error()
    good = _opts(O2)
    assert init(good[:2], 2) == -1 and b"n_opts" in lib.vch_last_error()
    for member, kw, word in ((2, dict(u_min=0.5, u_max=0.1), b"u_min"), (1, dict(alpha_max=0.0), b"alpha_max"),
                             (3, dict(b1=float("nan")), b"b1")):
        bad = list(good)
        bad[member] = O2.OptParams(**kw)
        assert init(bad, B) == -1
        msg = lib.vch_last_error()
        assert word in msg and f"trajectory {member}".encode() in msg, msg
    with pytest.raises(ValueError, match="trajectory 0"):
        e.pgd_init(p0, pT, t, [V.make_opt(O2.OptParams(kappa_sparsity=-1.0))] * B, ramp=True, T=P.T)
    with pytest.raises(V.VchError):
        e.pgd_kkt()
    assert e.counters() == before
    assert init([O2.OptParams(u_min=-np.inf, u_max=np.inf)], 1) == 0          # infinite bounds stay legal
    e.close()


@gpu
def test_run_sweep_mirror(V, O2):
    """GD2_configured.run_sweep on the four members: the batch of the tests above, through the mirror's configs."""
    G2, K2 = V.module("Vch_control_2D.GD2_configured"), V.module("Vch_control_2D.config")
    R = _batch_run(V, O2)
    cfg = K2.ForwardSolverConfig(Nx=NX, Ny=NY, Lx=LX, Ly=LY, T=M * DT, dt_initial=DT, tau=TAU)
    res = G2.run_sweep(cfg, [K2.OptimizationConfig(**MEMBERS[n]) for n in NAMES], n_iter=N_ITER, return_controls=True)
    assert "phi" not in res and res["iters"] == N_ITER
    assert np.array_equal(res["costs"][:, 0], R["J0"][:, 4]) and np.array_equal(res["costs"][:, 1:], R["out"]["cost"])
    for key, mine in (("alphas", "alpha"), ("attempts", "attempts"), ("changes", "change")):
        assert np.array_equal(res[key], R["out"][mine]), key
    assert np.array_equal(res["u"], R["u"])
    for key in ("n_zero", "n_small", "n_match", "total", "stationarity", "pct"):
        assert np.array_equal(res["kkt"][key], R["kkt"][key]), key
    assert "u" not in G2.run_sweep(cfg, [K2.OptimizationConfig(**MEMBERS["box"])], n_iter=1)
