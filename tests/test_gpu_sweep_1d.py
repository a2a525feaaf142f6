"""Per-trajectory optimisation parameters, warm start and the on-device KKT statistic of the 1D PGD loop
(vch1d_pgd_init_v, vch1d_pgd_kkt, Engine1D.pgd_init(opt=[...], u0, alpha0), Engine1D.pgd_kkt, GD_1D.run_sweep).

The PGD cases run on N = 48, T = 0.08, dt = 1e-2 (M = 8, rows = 10), init_phi_random(48, amp=0.05, seed=42), 3 iterations.
Four members start from the SAME phi0, so whatever differs between them comes from their parameters.
oracle.vch1d_oracle.pgd(..., initial_phi=...) on them (CPU; fields not named are the defaults of OptParams1D):

    member   parameters                                               trials  smallest rel. gap   exact  at u_min /  KKT counts at the
                                                                              judged / incumbent  zeros  u_max       refreshed r, tol 1e-6
    base     alpha_max 2                                              1,1,1   7.5e-4              20 %   0           98, 98, 490 / 490
    weights  b1 0.5, b2 40, kappa_sparsity 0.1, alpha_max 1           1,1,1   3.5e-4              43 %   0           210, 212, 488
    box      u_min -0.05, u_max 0.02, kappa_sparsity 0.03, alpha_max 2  1,1,1   4.9e-6              40 %   25 % / 28 % 195, 195, 490
    wide     alpha_max 2e5, u_min -100, u_max 100, b3 1e-3            1,5,1   3.3e-1              20 %   41 % / 39 % 98, 98, 490

`wide` exhausts the line search in iteration 2 (all five trials fail, the last is taken, G1:112-113; cost 1.071 -> 3.595).
Every |dJ| between accepted costs is >= 7.9e-6, so the plateau counter (1e-7) never moves, and the stop rule needs k > 10.
With tol = 2e-3 the counts are non-trivial: base 106, 98, 482 and box 196, 195, 489.  test_sweep_inputs_qualify asserts
the properties of this table that the GPU tests lean on.

Bit-for-bit claims rest on the 1D kernels: one trajectory is one workgroup with fixed reduction orders, the Newton and
adjoint solves are direct (cyclic reduction), and the table only changes where b1, b2, b3, kappa_sparsity, u_min, u_max
are read from.

Mutants applied by hand to the kernels, each built as a library of its own, and the tests of this file that failed under
each on an MI355X (the other tests passed):
  * row 0 of the parameter table for every trajectory in k1d_grad_prox: test_mixed_parameters_equal_single_runs,
    test_mixed_parameters_vs_oracle, test_kkt_counts_match_numpy (the tol = 2e-3 counts of the table),
    test_run_sweep_mirror (its one-member sweep against the batch);
  * the same in k1d_backward: test_mixed_parameters_equal_single_runs, test_mixed_parameters_vs_oracle,
    test_kkt_counts_match_numpy;
  * the same in k1d_kkt: test_mixed_parameters_equal_single_runs, test_kkt_counts_match_numpy, test_kkt_beyond_one_pass;
  * the strided tail of k1d_kkt dropped (each thread takes its first node only): test_kkt_beyond_one_pass
    (test_kkt_counts_match_numpy passes: its 490 nodes fit one pass of the T1 = 512 threads).
(test_warm_start_continues_the_run compares batch runs with batch runs and passes under the first two.)
"""
import ctypes as C

import numpy as np
import pytest

from conftest import golden, relerr

pytestmark = pytest.mark.gpu
N, M, DT, N_ITER = 48, 8, 1e-2, 3
ROWS = M + 2
MEMBERS = {
    "base": dict(alpha_max=2.0),
    "weights": dict(b1=0.5, b2=40.0, kappa_sparsity=0.1, alpha_max=1.0),
    "box": dict(u_min=-0.05, u_max=0.02, kappa_sparsity=0.03, alpha_max=2.0),
    "wide": dict(alpha_max=2.0e5, u_min=-100.0, u_max=100.0, b3=1e-3),
}
NAMES = tuple(MEMBERS)
OUT_KEYS = ("cost", "alpha", "trials", "change")
KKT_KEYS = ("n_zero", "n_small", "n_match", "total")
# the issue's table: counts at the refreshed adjoint
KKT_TABLE = {"base": (98, 98, 490), "weights": (210, 212, 488), "box": (195, 195, 490), "wide": (98, 98, 490)}
KKT_TABLE_2E3 = {"base": (106, 98, 482), "box": (196, 195, 489)}


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


@pytest.fixture(scope="module")
def O1():
    from oracle import vch1d_oracle
    return vch1d_oracle


def _params(O1, n=N, m=M):
    return O1.Params1D(N=n, T=m * DT, dt_initial=DT)


def _opts(O1):
    return [O1.OptParams1D(**MEMBERS[n]) for n in NAMES]


def _cargs(O):
    return (O.b1, O.b2, O.b3, O.kappa_sparsity)


_PROBLEM = {}


def _problem(O1, n=N, m=M):
    """P, t_hist (rows), dt (M), phi0, phi_T, phi_Q, x of the shared start."""
    if (n, m) not in _PROBLEM:
        P = _params(O1, n, m)
        phi0 = O1.init_phi_random(n, amp=0.05, seed=42)
        x = np.linspace(0.0, P.Lx, n + 1)
        t, dts, acc = [0.0, 0.0], [], 0.0
        while acc < P.T - 1e-10:                       # the accumulated-time rule of O1.forward
            d = min(P.dt_initial, P.T - acc)
            dts.append(d)
            acc += d
            t.append(min(acc, P.T))
        t, dts = np.array(t), np.array(dts)
        phi_T, phi_Q = O1.build_targets(x, t, phi0, P.Lx, P.T)
        _PROBLEM[(n, m)] = (P, t, dts, phi0, phi_T, phi_Q, x)
    return _PROBLEM[(n, m)]


_REFS = {}


def _refs(O1):
    """O1.pgd (3 iterations) per member with every cost the loop evaluated, and the adjoint of its final state."""
    if not _REFS:
        P, t, _, phi0, phi_T, phi_Q, x = _problem(O1)
        orig = O1.cost
        for n, O in zip(NAMES, _opts(O1)):
            costs = []

            def recording(*args, **kw):
                costs.append(orig(*args, **kw))
                return costs[-1]
            O1.cost = recording
            try:
                r = O1.pgd(P, O, n_iter=N_ITER, initial_phi=phi0)
            finally:
                O1.cost = orig
            assert np.array_equal(r.t_hist, t)
            _, _, r_fresh = O1.backward(r.phi, x, t, O.b1, O.b2, phi_Q, phi_T)
            _REFS[n] = (r, costs, r_fresh)
    return _REFS


def _np_counts(u, r, kappa, tol=1e-6):
    """The predicates of GD_1D.verify_sparsity_condition (G1:115-147) as counts."""
    z, s = np.abs(u) < tol, np.abs(r) <= kappa
    return int(z.sum()), int(s.sum()), int((z == s).sum()), int(u.size)


def test_sweep_inputs_qualify(O1):
    """No member's line search sits on an accept / reject tie: every cost a candidate was judged by differs from its
    incumbent's by more than 1e-6 relative (1000 x the 1e-9 the costs are held to); `wide` has a 5-trial iteration;
    `weights` and `box` end with exact zeros from the threshold and `box` with nodes at both bounds; no |dJ| comes near the
    plateau rule's 1e-7; the KKT counts of the table hold on the CPU."""
    R = _refs(O1)
    for n, O in zip(NAMES, _opts(O1)):
        r, costs, r_fresh = R[n]
        assert len(r.costs) == N_ITER + 1 and costs[0] == r.costs[0] and not r.converged
        i, gap = 1, np.inf
        for k, nt in enumerate(r.trials):
            inc = r.costs[k]
            ncand = 1 if costs[i] < inc else 1 + nt      # the optimistic step, then (after its failure) the nt trials
            for cnd in costs[i:i + ncand]:
                gap = min(gap, abs(cnd - inc) / inc)
                assert abs(cnd - inc) > 1e-6 * inc, (n, k, cnd, inc)
            i += ncand
            assert costs[i - 1] == r.costs[k + 1]
        assert i == len(costs)
        zeros = float(np.mean(r.u == 0.0))
        lo, hi = float(np.mean(r.u == O.u_min)), float(np.mean(r.u == O.u_max))
        dj = float(np.min(np.abs(np.diff(r.costs))))
        counts = _np_counts(r.u, r_fresh, O.kappa_sparsity)
        print(f"{n}: trials {r.trials} smallest gap {gap:.1e} zeros {zeros:.2%} at bounds {lo:.2%} / {hi:.2%} "
              f"min |dJ| {dj:.1e} kkt {counts}")
        assert dj > 1e-6
        assert counts == KKT_TABLE[n] + (ROWS * (N + 1),)
        if n in KKT_TABLE_2E3:
            assert _np_counts(r.u, r_fresh, O.kappa_sparsity, 2e-3)[:3] == KKT_TABLE_2E3[n]
        if n == "wide":
            assert list(r.trials) == [1, 5, 1] and r.costs[2] > r.costs[1]      # the exhausted search's last try is taken
        else:
            assert list(r.trials) == [1, 1, 1]
        if n in ("weights", "box"):
            assert zeros > 0.3
        if n == "box":
            assert lo > 0.2 and hi > 0.2


def _engine(V, batch, n=N, max_steps=M):
    return V.Engine1D(N=n, batch=batch, max_steps=max_steps)


def _tile(a, B):
    return np.repeat(np.asarray(a)[None], B, axis=0)


def _init_batch(V, O1, e, **kw):
    _, t, dts, phi0, phi_T, _, x = _problem(O1)
    B = len(NAMES)
    return e.pgd_init(_tile(phi0, B), _tile(phi_T, B), t, dts, [V.make_opt(o) for o in _opts(O1)], x=x, **kw)


_RUN = {}


def _batch_run(V, O1):
    """The four members as one batch: init, 3 iterations, u and the loop's r; then pgd_kkt(refresh=True) with both values
    of tol, and u, r, phi, phi_Q pulled after it."""
    if not _RUN:
        e = _engine(V, len(NAMES))
        _RUN["J0"] = _init_batch(V, O1, e)
        _RUN["out"] = e.pgd_iterate(N_ITER)
        _RUN["u"], _RUN["r"] = e.pgd_get("u"), e.pgd_get("r")
        _RUN["kkt"] = e.pgd_kkt(refresh=True)
        _RUN["kkt_2e3"] = e.pgd_kkt(refresh=True, tol=2e-3)
        _RUN["u_after"], _RUN["r_after"] = e.pgd_get("u"), e.pgd_get("r")
        _RUN["phi_after"], _RUN["phi_Q"] = e.pgd_get("phi"), e.pgd_get("phi_Q")
        e.close()
    return _RUN


def _assert_run_is_batch(R, J0, out, u, members=None):
    for b in (range(len(NAMES)) if members is None else members):
        assert np.array_equal(J0[b], R["J0"][b]), (NAMES[b], J0[b], R["J0"][b])
        for key in OUT_KEYS:
            assert np.array_equal(out[key][b], R["out"][key][b]), (NAMES[b], key, out[key][b], R["out"][key][b])
        assert np.array_equal(u[b], R["u"][b]), NAMES[b]


def test_mixed_parameters_equal_single_runs(V, O1):
    """A member of the mixed batch computes the bits of a batch-1 context run with its parameters through the single-opt
    vch1d_pgd_init: J0, costs, step lengths, trials, changes, the control, the KKT counts and the stationarity."""
    R = _batch_run(V, O1)
    _, t, dts, phi0, phi_T, _, x = _problem(O1)
    for b, O in enumerate(_opts(O1)):
        e = _engine(V, 1)
        J0 = e.pgd_init(phi0, phi_T, t, dts, V.make_opt(O), x=x)
        out = e.pgd_iterate(N_ITER)
        u = e.pgd_get("u")
        k = e.pgd_kkt(refresh=True)
        e.close()
        print(f"{NAMES[b]}: trials {out['trials'][0]} cost {out['cost'][0]} / {R['out']['cost'][b]} "
              f"counts {[int(k[n][0]) for n in KKT_KEYS]} stationarity {k['stationarity'][0]!r}"
              f" / {R['kkt']['stationarity'][b]!r}")
        assert np.array_equal(J0[0], R["J0"][b]), (J0, R["J0"][b])
        for key in OUT_KEYS:
            assert np.array_equal(out[key][0], R["out"][key][b]), (NAMES[b], key, out[key][0], R["out"][key][b])
        assert np.array_equal(u, R["u"][b])
        for key in KKT_KEYS:
            assert int(k[key][0]) == int(R["kkt"][key][b]), (NAMES[b], key)
        assert k["stationarity"][0] == R["kkt"]["stationarity"][b]


def test_init_v_with_one_set_is_init(V):
    """vch1d_pgd_init_v(n_opts = 1, u0 = NULL, alpha0 = NULL) and vch1d_pgd_init: identical bits over 3 iterations of the
    golden problem g1d_pgd_32_bt (two exhausted line searches)."""
    gp = golden("g1d_pgd_32_bt.npz")
    G1, F1 = V.module("Vch_control_1D.GD_1D"), V.module("Vch_control_1D.Forward_solver")
    lib, _lib = V.load(), V.module("_lib")
    n, T, dt = int(gp["N"]), float(gp["T"]), float(gp["dt"])
    tg, dts = V.time_grid(T, dt)
    t = np.concatenate([[0.0], tg])
    assert np.array_equal(t, gp["t_hist"])
    phi0 = F1.init_phi_random(n, F1.delta_sep, amp=0.01, seed=42, enforce_zero_mean=True)
    x = np.linspace(0.0, 1.0, n + 1)
    phi_T = G1.build_targets_1d(x, t, phi0, 1.0, T, choice_q=2)[0]
    opt = V.make_opt(V.module("Vch_control_1D.config").OptimizationConfig(alpha_max=float(gp["alpha_max"])))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    runs = []
    for entry in ("init", "init_v"):
        e = _engine(V, 1, n=n, max_steps=len(dts))
        if entry == "init":
            J0 = e.pgd_init(phi0, phi_T, t, dts, opt, x=x)
        else:
            J0 = np.zeros((1, 5))
            arr = (_lib.OptParams * 1)(opt)
            rc = lib.vch1d_pgd_init_v(e.ctx, dp(phi0), dp(phi_T), None, dp(x), dp(t), len(t), dp(dts), arr, 1, None, None, dp(J0))
            assert rc == 0, lib.vch_last_error()
            e._pgd_rows = len(t)
        out = e.pgd_iterate(N_ITER)
        runs.append((J0, out, e.pgd_get("u"), e.pgd_get("r"), e.pgd_get("phi")))
        e.close()
    a, b = runs
    print(f"init / init_v: trials {a[1]['trials'][0]} / {b[1]['trials'][0]} cost {a[1]['cost'][0]} / {b[1]['cost'][0]}")
    assert list(a[1]["trials"][0]) == list(gp["trials"][:N_ITER]) and max(a[1]["trials"][0]) == 5
    assert np.array_equal(a[0], b[0])
    for key in OUT_KEYS + ("tracking_error", "terminal_error"):
        assert np.array_equal(a[1][key], b[1][key]), key
    for k in (2, 3, 4):
        assert np.array_equal(a[k], b[k])


def test_mixed_parameters_vs_oracle(V, O1):
    """The mixed batch against O1.pgd per member, with the tolerances of test_pgd_resident_vs_reference_golden."""
    R, refs = _batch_run(V, O1), _refs(O1)
    J0, out, u, r = R["J0"], R["out"], R["u"], R["r"]
    for b, n in enumerate(NAMES):
        ref = refs[n][0]
        print(f"pgd {n}: trials {out['trials'][b]} / {ref.trials} cost {out['cost'][b]} / {ref.costs} alpha {out['alpha'][b]} "
              f"/ {ref.alphas} u {relerr(u[b], ref.u):.1e} r {relerr(r[b], ref.r):.1e} J0 {abs(J0[b, 4] / ref.costs[0] - 1):.1e}")
    for b, n in enumerate(NAMES):
        ref = refs[n][0]
        assert np.allclose(np.concatenate([J0[b, 4:5], out["cost"][b]]), ref.costs, rtol=1e-9, atol=0), (out["cost"][b], ref.costs)
        assert np.allclose(out["alpha"][b], ref.alphas, rtol=1e-14, atol=0), (out["alpha"][b], ref.alphas)
        assert list(out["trials"][b]) == list(ref.trials), (out["trials"][b], ref.trials)
        assert relerr(u[b], ref.u) < 1e-8 and relerr(r[b], ref.r) < 1e-8


def _assert_kkt(V, O1, k, u, r, opts, tol=1e-6):
    G1 = V.module("Vch_control_1D.GD_1D")
    for b, O in enumerate(opts):
        counts = _np_counts(u[b], r[b], O.kappa_sparsity, tol)
        un = O1.prox_project(O1.gradient_step(u[b], O1.gradient(r[b], u[b], O.b3), 1.0), 1.0, O.kappa_sparsity, O.u_min, O.u_max)
        stat = float(np.linalg.norm(un - u[b]) / (np.linalg.norm(u[b]) + 1e-9))
        got = tuple(int(k[n][b]) for n in KKT_KEYS)
        print(f"kkt {b} tol {tol:g}: counts {got} / {counts} stationarity {k['stationarity'][b]:.15e} / {stat:.15e}")
        assert got == counts, (b, got, counts)
        pct = G1.verify_sparsity_condition(u[b], r[b], O.kappa_sparsity, tol=tol, verbose=False)
        assert np.allclose(k["pct"][b], pct, rtol=1e-15, atol=0), (k["pct"][b], pct)
        assert abs(k["stationarity"][b] - stat) <= 1e-12 * stat, (b, k["stationarity"][b], stat)


def test_kkt_counts_match_numpy(V, O1):
    """pgd_kkt(refresh=True) after the three iterations, tol 1e-6 and 2e-3: the counts are exactly the predicates of
    verify_sparsity_condition on the control and adjoint pulled after the call, the stationarity is NumPy's prox step with
    alpha = 1 on them, and the refreshed adjoint is Engine1D.backward of the resident state under each member's own b1,
    b2 (the same kernel on the same inputs: equal bits).  refresh=False needs a sweep since the init.  A run interrupted
    by pgd_kkt continues bit for bit, with either value of refresh: the adjoint is a direct solve."""
    R = _batch_run(V, O1)
    _, t, _, _, phi_T, _, _ = _problem(O1)
    opts = _opts(O1)
    B = len(opts)
    assert np.array_equal(R["u_after"], R["u"]) and np.all(R["kkt"]["total"] == ROWS * (N + 1))
    _assert_kkt(V, O1, R["kkt"], R["u_after"], R["r_after"], opts)
    _assert_kkt(V, O1, R["kkt_2e3"], R["u_after"], R["r_after"], opts, tol=2e-3)
    for n, want in KKT_TABLE_2E3.items():                  # the second tolerance really moves the first predicate
        b = NAMES.index(n)
        assert tuple(int(R["kkt_2e3"][key][b]) for key in KKT_KEYS[:3]) == want
        assert int(R["kkt_2e3"]["n_zero"][b]) > int(R["kkt"]["n_zero"][b])
    e1 = _engine(V, 1)                                     # default physics: the 1D adjoint freezes its parameters there
    for b, O in enumerate(opts):
        _, _, r1 = e1.backward(R["phi_after"][b], t, O.b1, O.b2, phi_Q=R["phi_Q"][b], phi_T=phi_T)
        print(f"refreshed r {NAMES[b]}: {relerr(R['r_after'][b], r1):.1e}")
        assert np.array_equal(R["r_after"][b], r1), NAMES[b]
    e1.close()
    runs = {}
    for mode in ("plain", "resident", "refresh"):
        e = _engine(V, B)
        _init_batch(V, O1, e)
        if mode == "plain":
            with pytest.raises(V.VchError, match="engine error -3"):
                e.pgd_kkt(refresh=False)
        first = e.pgd_iterate(1)
        if mode != "plain":
            k = e.pgd_kkt(refresh=(mode == "refresh"))
            _assert_kkt(V, O1, k, e.pgd_get("u"), e.pgd_get("r"), opts)
        runs[mode] = (first, e.pgd_iterate(2), e.pgd_get("u"))
        e.close()
    for mode in ("resident", "refresh"):
        for i in (0, 1):
            for key in OUT_KEYS:
                assert np.array_equal(runs[mode][i][key], runs["plain"][i][key]), (mode, i, key)
        assert np.array_equal(runs[mode][2], runs["plain"][2]), mode
    assert np.array_equal(runs["plain"][2], R["u"])


def test_kkt_beyond_one_pass(V, O1):
    """N = 700: n = 701 nodes per row, more than the T1 = 512 threads of the workgroup and no multiple of 64, 4 rows.  A
    warm start with exact zeros, values on either side of tol and saturated nodes at the row ends, around thread 512 and
    over the whole first and last row is returned as given and counted exactly right after the init."""
    n_, Mp, B, tol = 700, 2, 3, 1e-6
    opts = [O1.OptParams1D(kappa_sparsity=ks, u_min=-0.05, u_max=0.02) for ks in (1e-4, 5e-3, 1.0)]
    _, t, dts, phi0, phi_T, _, x = _problem(O1, n_, Mp)
    rows = Mp + 2
    assert len(t) == rows
    rng = np.random.default_rng(7)
    u0 = rng.uniform(-0.04, 0.015, (B, rows, n_ + 1))
    marks = (0.0, 5e-7, -5e-7, 2e-6, -2e-6, -0.05, 0.02)
    for j, node in enumerate((0, 511, 512, 700)):
        for rr in range(rows):
            u0[:, rr, node] = marks[(j + rr) % len(marks)]
    for rr in (0, rows - 1):
        u0[:, rr, :] = np.array(marks)[(np.arange(n_ + 1) + rr) % len(marks)]
    e = _engine(V, B, n=n_, max_steps=Mp)
    e.pgd_init(_tile(phi0, B), _tile(phi_T, B), t, dts, [V.make_opt(o) for o in opts], x=x, u0=u0)
    k = e.pgd_kkt(refresh=True, tol=tol)
    u, r = e.pgd_get("u"), e.pgd_get("r")
    e.close()
    assert np.array_equal(u, u0)                                    # taken as given
    assert np.all(k["total"] == 4 * 701)
    _assert_kkt(V, O1, k, u, r, opts, tol)
    assert 0 < k["n_zero"][0] < k["total"][0]
    assert k["n_small"][2] == k["total"][2] and np.abs(r[2]).max() <= 1.0


def test_warm_start_continues_the_run(V, O1):
    """A context warm-started from the control after two iterations, with the step length the loop would use next, does
    the third iteration of the uninterrupted run; J0 under a start control is the oracle's cost of the march under it."""
    A = _batch_run(V, O1)
    opts = _opts(O1)
    B = len(opts)
    e = _engine(V, B)
    _init_batch(V, O1, e)
    mid = e.pgd_iterate(2)
    u2 = e.pgd_get("u")
    e.close()
    for key in OUT_KEYS:
        assert np.array_equal(mid[key], A["out"][key][:, :2])
    alpha0 = np.minimum(np.array([o.alpha_max for o in opts]), 1.2 * A["out"]["alpha"][:, 1])
    e = _engine(V, B)
    J0 = _init_batch(V, O1, e, u0=u2, alpha0=alpha0)
    out = e.pgd_iterate(1)
    u = e.pgd_get("u")
    e.close()
    P, t, _, phi0, phi_T, phi_Q, x = _problem(O1)
    Jo = []
    for b, O in enumerate(opts):
        ph, _, _ = O1.forward(P, control=u2[b], initial_phi=phi0)
        Jo.append(O1.cost(ph, u2[b], phi_Q, phi_T, x, t, *_cargs(O)))
        print(f"warm {NAMES[b]}: J0 {J0[b, 4]!r} / run A {A['out']['cost'][b, 1]!r} / oracle {Jo[b]!r}; trials "
              f"{out['trials'][b, 0]} / {A['out']['trials'][b, 2]} alpha {out['alpha'][b, 0]!r} / "
              f"{A['out']['alpha'][b, 2]!r} cost {out['cost'][b, 0]!r} / {A['out']['cost'][b, 2]!r} "
              f"u {relerr(u[b], A['u'][b]):.1e}")
    assert np.allclose(J0[:, 4], Jo, rtol=1e-9, atol=0)
    assert np.allclose(J0[:, 4], A["out"]["cost"][:, 1], rtol=1e-13, atol=0)
    assert np.array_equal(out["trials"][:, 0], A["out"]["trials"][:, 2])
    assert np.array_equal(out["alpha"][:, 0], A["out"]["alpha"][:, 2])
    assert np.allclose(out["cost"][:, 0], A["out"]["cost"][:, 2], rtol=1e-13, atol=0)
    for b in range(B):
        assert relerr(u[b], A["u"][b]) < 1e-12


def test_sweep_argument_errors(V, O1):
    """Bad parameter sets and calls out of order return an error code with a message that names the field and the
    trajectory; the context then takes a good init and runs the batch's bits."""
    lib, _lib = V.load(), V.module("_lib")
    _, t, dts, phi0, phi_T, _, x = _problem(O1)
    B = len(NAMES)
    e = _engine(V, B)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    p0, pT, J0 = _tile(phi0, B), _tile(phi_T, B), np.zeros((B, 5))
    cnt, stat = np.zeros((B, 4), dtype=np.int64), np.zeros(B)

    def init(opts, n, alpha0=None):
        arr = (_lib.OptParams * len(opts))(*[V.make_opt(o) for o in opts])
        return lib.vch1d_pgd_init_v(e.ctx, dp(p0), dp(pT), None, dp(x), dp(t), ROWS, dp(dts), arr, n, None,
                                    None if alpha0 is None else dp(alpha0), dp(J0))

    assert lib.vch1d_pgd_kkt(e.ctx, 1, 1e-6, cnt.ctypes.data_as(C.POINTER(C.c_int64)), dp(stat)) == -3
    assert b"pgd_init" in lib.vch_last_error()
    good = _opts(O1)
    assert init(good[:2], 2) == -1 and b"n_opts" in lib.vch_last_error()
    for member, kw, word in ((2, dict(u_min=0.5, u_max=0.1), b"u_min"), (1, dict(alpha_max=0.0), b"alpha_max"),
                             (3, dict(b1=float("nan")), b"b1"), (0, dict(kappa_sparsity=-1.0), b"kappa_sparsity")):
        bad = list(good)
        bad[member] = O1.OptParams1D(**kw)
        assert init(bad, B) == -1
        msg = lib.vch_last_error()
        assert word in msg and f"trajectory {member}".encode() in msg, msg
    a0 = np.array([1.0, 1.0, 0.0, 1.0])
    assert init(good, B, a0) == -1
    msg = lib.vch_last_error()
    assert b"alpha0" in msg and b"trajectory 2" in msg, msg
    with pytest.raises(ValueError, match="trajectory 0"):
        e.pgd_init(p0, pT, t, dts, [V.make_opt(O1.OptParams1D(kappa_sparsity=-1.0))] * B, x=x)
    with pytest.raises(V.VchError, match="engine error -3"):       # still no problem loaded
        e.pgd_kkt()
    assert init([O1.OptParams1D(u_min=-np.inf, u_max=np.inf)], 1) == 0          # infinite bounds stay legal
    R = _batch_run(V, O1)
    J0 = _init_batch(V, O1, e)
    out = e.pgd_iterate(N_ITER)
    _assert_run_is_batch(R, J0, out, e.pgd_get("u"))
    e.close()


def test_run_sweep_mirror(V, O1):
    """GD_1D.run_sweep on the four members: the batch of the tests above, through the mirror's configs."""
    G1, K1 = V.module("Vch_control_1D.GD_1D"), V.module("Vch_control_1D.config")
    R = _batch_run(V, O1)
    cfg = K1.ForwardSolverConfig(N=N, T=M * DT, dt_initial=DT)
    res = G1.run_sweep(cfg, [K1.OptimizationConfig(**MEMBERS[n]) for n in NAMES], n_iter=N_ITER, seed=42, amp=0.05,
                       return_controls=True)
    assert "phi" not in res and res["iters"] == N_ITER
    assert np.array_equal(res["costs"][:, 0], R["J0"][:, 4]) and np.array_equal(res["costs"][:, 1:], R["out"]["cost"])
    for key, mine in (("alphas", "alpha"), ("trials", "trials"), ("changes", "change")):
        assert np.array_equal(res[key], R["out"][mine]), key
    assert np.array_equal(res["u"], R["u"])
    for key in KKT_KEYS + ("stationarity", "pct"):
        assert np.array_equal(res["kkt"][key], R["kkt"][key]), key
    one = G1.run_sweep(cfg, [K1.OptimizationConfig(**MEMBERS["box"])], n_iter=1, initial_phi=_problem(O1)[3])
    assert "u" not in one and "phi" not in one
    assert np.array_equal(one["costs"][0], [R["J0"][2, 4], R["out"]["cost"][2, 0]])
