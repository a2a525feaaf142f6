"""Directional sparsity in the 1D engine on the GPU: the group prox of both modes against the NumPy
restatement (tests/_group_prox_ref.py), the cost, the resident loop against the function-seam loop, mixed batches, the
KKT statistic by groups, that the full-sparsity paths keep their bits, and the refused calls."""
import ctypes as C

import numpy as np
import pytest

import _group_prox_ref as G
from conftest import relerr

pytestmark = pytest.mark.gpu

BOXES = ((-1.0, 1.0), (-0.3, 2.0), (0.0, 1.0), (-1.0, 0.0), (-np.inf, np.inf))
# a partial wave, the wave edge, the workgroup edge (the rows kernel built for one and for two values per thread), a row of
# three values in the kernel built for four, and nine values with one in the last slot
SIZES = (24, 63, 64, 511, 512, 1500, 4096)
MAXROWS = 70


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


@pytest.fixture(scope="module")
def O1():
    from oracle import vch1d_oracle
    return vch1d_oracle


@pytest.fixture(scope="module")
def engines(V):
    made = {}

    def get(N):
        if N not in made:
            made[N] = V.Engine1D(N=N, batch=3, max_steps=MAXROWS)
        return made[N]
    yield get
    for e in made.values():
        e.close()


def _grids(rng, n, rows):
    x = np.cumsum(np.r_[0.0, rng.uniform(0.5, 1.5, n - 1)])
    x /= x[-1]
    t = np.r_[0.0, 0.0, np.cumsum(rng.uniform(0.5, 1.5, rows - 2))]       # t = 0 twice, as in a history
    return x, t / t[-1]


def _seam_case(rng, mode, n, rows, lo, hi, alpha, b3):
    """u, r (3, rows, n) whose gradient step v holds groups of every kind: amplitude 0.005 (||v|| < lam = 0.02: zero; on a
    one-sided box also a large group on the wrong side), 0.05 (closed form; one-signed where the box is one-sided) and 3
    (box-active where the box is finite).  ||clip(s v)|| <= 2 keeps rho / lam <= 100."""
    ng = rows if mode == "time" else n
    cls = (np.arange(3 * ng).reshape(3, ng) + rng.integers(3)) % 3
    amp = np.choose(cls, [0.005, 0.05, 3.0])
    amp = amp[:, :, None] if mode == "time" else amp[:, None, :]
    cl = cls[:, :, None] if mode == "time" else cls[:, None, :]
    z = rng.standard_normal((3, rows, n))
    one_sided = (lo == 0.0) or (hi == 0.0)
    sgn = 1.0 if lo == 0.0 else -1.0
    if one_sided:
        z = np.where(cl == 1, sgn * np.abs(z), z)
        wrong = (cl == 0) & (rng.random(cl.shape) < 0.5)
        z = np.where(wrong, -sgn * 400.0 * np.abs(z), z)
    v = amp * z
    r = rng.standard_normal((3, rows, n))
    u = (v + alpha * r) / (1.0 - alpha * b3)
    return u, r


@pytest.mark.parametrize("mode", ["time", "space"])
@pytest.mark.parametrize("N", SIZES)
def test_group_prox_seam_against_the_restatement(V, engines, mode, N):
    """s to 1e-12 absolute and u+ to 1e-12 max|v|.  The bound is derived, not measured: both roots make |h| a few ulps of
    rho = ||clip(s v)||, and |h'| >= min(rho, lam) at the root (h' <= -rho always), so s is off by at most
    ~1e-15 max(1, rho / lam); rho / lam <= 100 is kept in the inputs, which leaves a factor of ten.  With the infinite box
    u+ is s v to the bit (alpha a power of two and b3 = 0 make v exact)."""
    eng, n = engines(N), N + 1
    rng = np.random.default_rng(1000 + N + (mode == "space"))
    for rows in (3, 7) + ((MAXROWS,) if mode == "space" else ()):
        x, t = _grids(rng, n, rows)
        for lo, hi in BOXES:
            inf = np.isinf(hi)
            alpha, ks, b3 = 0.5, 0.04, (0.0 if inf else 0.1)
            u, r = _seam_case(rng, mode, n, rows, lo, hi, alpha, b3)
            opt = V.make_opt(b3=b3, kappa_sparsity=ks, u_min=lo, u_max=hi)
            up, s = eng.grad_prox(u, r, alpha, opt, sparsity=mode, x=x, t_hist=t, return_scale=True)
            kinds = set()
            for b in range(3):
                ur, sr, kr = G.prox(u[b], r[b], alpha, b3, ks, lo, hi, mode, x, t)
                v = u[b] - alpha * (r[b] + b3 * u[b])
                kinds |= set(kr)
                rho = G.group_norms(ur, x, t, mode)[np.array(kr) == "box"]       # the groups whose s is a computed root
                assert rho.size == 0 or rho.max() / (alpha * ks) <= 100.0
                assert np.max(np.abs(s[b] - sr)) <= 1e-12, (mode, N, rows, lo, hi, b)
                assert np.max(np.abs(up[b] - ur)) <= 1e-12 * np.max(np.abs(v)), (mode, N, rows, lo, hi, b)
                assert np.array_equal(s[b] == 0.0, np.array(kr) == "zero")
                if inf:
                    sv = s[b][:, None] * v if mode == "time" else s[b][None, :] * v
                    assert np.array_equal(up[b], sv)
            # an infinite box is never active: it has the two other kinds
            assert kinds == ({"zero", "closed"} if inf else {"zero", "closed", "box"}), (mode, N, rows, lo, hi, kinds)


def _problem(V, N=48, T=0.08, dt=1e-2):
    F1 = V.module("Vch_control_1D.Forward_solver")
    tg, dts = V.time_grid(T, dt)
    t_hist = np.concatenate([[0.0], tg])
    phi0 = np.stack([F1.init_phi_random(N, 1e-2, amp=a, seed=s) for s, a in zip((42, 43, 44), (0.01, 0.2, 0.05))])
    x = np.linspace(0.0, 1.0, N + 1)
    phi_T = np.repeat((0.7 * np.sin(2.0 * np.pi * x))[None], 3, axis=0)
    return phi0, phi_T, t_hist, dts, x


def _run(V, phi0, phi_T, t_hist, dts, opts, sparsity, n_iter=3, via=None):
    """pgd_init + pgd_iterate on a fresh context -> (J0, res, u, phi)."""
    B = phi0.shape[0]
    e = V.Engine1D(N=phi0.shape[1] - 1, batch=B, max_steps=len(dts))
    try:
        J0 = e.pgd_init(phi0, phi_T, t_hist, dts, opts, sparsity=sparsity) if via is None else via(e)
        res = e.pgd_iterate(n_iter)
        return J0, res, e.pgd_get("u").reshape(B, len(t_hist), -1), e.pgd_get("phi").reshape(B, len(t_hist), -1)
    finally:
        e.close()


def _same_bits(a, b):
    (Ja, ra, ua, pa), (Jb, rb, ub, pb) = a, b
    return (np.array_equal(Ja, Jb) and np.array_equal(ua, ub) and np.array_equal(pa, pb) and
            all(np.array_equal(ra[k], rb[k], equal_nan=True) for k in ("cost", "alpha", "trials", "change")))


def test_full_mode_keeps_its_bits(V, engines):
    rng = np.random.default_rng(5)
    eng, n, rows = engines(63), 64, 7
    lib, dp = eng.lib, lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    x, t = _grids(rng, n, rows)
    u, r, phi, pq = (rng.standard_normal((3, rows, n)) for _ in range(4))
    pt = rng.standard_normal((3, n))
    al = np.array([0.5, 0.3, 2.0])
    opt = V.make_opt(b3=0.1, kappa_sparsity=0.2, u_min=-0.5, u_max=0.7)
    a, b, s = eng.grad_prox(u, r, al, opt), np.empty_like(u), np.full((3, n), 7.0)
    assert lib.vch1d_grad_prox_g(eng.ctx, dp(u), dp(r), rows, None, None, dp(al), C.byref(opt), 0, dp(b), dp(s)) == 0
    assert np.array_equal(a, b) and np.all(s == 7.0)
    Ja, Jb = eng.cost(phi, u, pq, pt, x, t, opt), np.empty((3, 5))
    assert lib.vch1d_cost_g(eng.ctx, dp(phi), dp(u), dp(pq), dp(pt), rows, dp(x), dp(t), C.byref(opt), 0, dp(Jb)) == 0
    assert np.array_equal(Ja, Jb)
    phi0, phi_T, t_hist, dts, _ = _problem(V)
    opts = [V.make_opt(alpha_max=a) for a in (2.0e5, 100.0, 20.0)]
    assert _same_bits(_run(V, phi0, phi_T, t_hist, dts, opts, None), _run(V, phi0, phi_T, t_hist, dts, opts, "full"))
    assert _same_bits(_run(V, phi0, phi_T, t_hist, dts, opts, None), _run(V, phi0, phi_T, t_hist, dts, opts, ["full"] * 3))


@pytest.mark.parametrize("N", [48, 600])
def test_cost_of_both_modes(V, O1, N):
    rng = np.random.default_rng(N)
    n, rows = N + 1, 9
    e = V.Engine1D(N=N, batch=2, max_steps=rows)
    x, t = _grids(rng, n, rows)
    phi, u, pq = (rng.standard_normal((2, rows, n)) for _ in range(3))
    u[1, :, ::3] = 0.0
    u[1, 4] = 0.0
    pt = rng.standard_normal((2, n))
    w = (0.7, 3.0, 0.4, 0.25)
    opt = V.make_opt(b1=w[0], b2=w[1], b3=w[2], kappa_sparsity=w[3])
    for mode in ("time", "space"):
        J = e.cost(phi, u, pq, pt, x, t, opt, sparsity=mode)
        for b in range(2):
            assert abs(J[b, 3] / G.j4(u[b], x, t, w[3], mode) - 1.0) <= 1e-13
            assert abs(J[b, 4] / G.cost(O1, phi[b], u[b], pq[b], pt[b], x, t, *w, mode) - 1.0) <= 1e-13
            assert np.array_equal(J[b, :3], e.cost(phi, u, pq, pt, x, t, opt)[b, :3])
    e.close()


# kappa_sparsity and alpha_max were picked on the CPU, with the restatement's loop over the oracle: the adjoint's row norms at
# u = 0 run from 0.058 down to 0.028 (kappa_s = 0.045 cuts between rows 6 and 7), its column norms from 0 to 0.018 (0.012
# leaves 17 or 18 of 49 columns zero), and alpha_max = 2e5 makes the second iteration backtrack through all five trials.
RESIDENT = {"time": dict(kappa_sparsity=0.045, alpha_max=2.0e5), "space": dict(kappa_sparsity=0.012, alpha_max=2.0e5)}


@pytest.fixture(scope="module")
def resident(V):
    G1 = V.module("Vch_control_1D.GD_1D")
    K1 = V.module("Vch_control_1D.config")
    cfg = K1.ForwardSolverConfig(N=48, T=0.08, dt_initial=1e-2)
    phi0 = _problem(V)[0]
    out = {}
    for mode, kw in RESIDENT.items():
        opt = K1.OptimizationConfig(**kw)
        out[mode] = (cfg, opt, phi0, G1.run_optimization_resident(cfg, opt, n_iter=3, initial_phi=phi0, sparsity=mode))
    return out


@pytest.mark.parametrize("mode", ["time", "space"])
def test_resident_loop_matches_function_seam(V, O1, resident, mode):
    G1 = V.module("Vch_control_1D.GD_1D")
    cfg, opt, phi0, rb = resident[mode]
    assert rb["u"].shape == (3, 10, 49)
    for b in range(3):
        rs = G1.run_optimization(cfg, opt, n_iter=3, sparsity=mode, initial_phi=phi0[b])
        assert list(rs["trials"]) == list(rb["trials"][b])
        assert np.allclose(rs["costs"], rb["costs"][b], rtol=1e-12)
        assert relerr(rs["u"], rb["u"][b]) < 1e-10
        # some, not all groups are zero (row 0, the duplicated t = 0 row, is zero in any case: its adjoint is)
        gn = G.group_norms(rb["u"][b], rb["x"], rb["t_hist"], mode)[(1 if mode == "time" else 0):]
        assert 0 < np.count_nonzero(gn == 0.0) < gn.size, gn
    assert max(max(t) for t in rb["trials"]) > 1          # a line search ran
    # the restatement's own loop over the oracle, from the reference's seed
    P = O1.Params1D(N=48, T=0.08, dt_initial=1e-2)
    ref = G.pgd(O1, P, O1.OptParams1D(**RESIDENT[mode]), mode, 3, initial_phi=phi0[0])
    assert ref["trials"] == list(rb["trials"][0]) and np.allclose(ref["costs"], rb["costs"][0], rtol=1e-9)
    assert relerr(rb["u"][0], ref["u"]) < 1e-7


def test_mixed_batch_members_have_the_bits_of_their_single_runs(V):
    phi0, phi_T, t_hist, dts, _ = _problem(V)
    modes = ["full", "time", "space"]
    opts = [V.make_opt(kappa_sparsity=9e-5, alpha_max=2.0e5), V.make_opt(kappa_sparsity=0.045, alpha_max=100.0, u_min=-0.3, u_max=2.0),
            V.make_opt(kappa_sparsity=0.012, alpha_max=2.0e5, u_min=-1.0, u_max=0.5)]
    Jm, rm, um, pm = _run(V, phi0, phi_T, t_hist, dts, opts, modes)
    for b in range(3):
        one = _run(V, phi0[b:b + 1], phi_T[b:b + 1], t_hist, dts, [opts[b]], modes[b])
        part = (Jm[b:b + 1], {k: rm[k][b:b + 1] for k in ("cost", "alpha", "trials", "change")}, um[b:b + 1], pm[b:b + 1])
        assert _same_bits(part, one), modes[b]
    # and in another order, next to other neighbours
    order = [2, 0, 1]
    Jp, rp, up_, pp = _run(V, phi0[order], phi_T[order], t_hist, dts, [opts[i] for i in order], [modes[i] for i in order])
    assert np.array_equal(up_, um[order]) and np.array_equal(pp, pm[order]) and np.array_equal(rp["cost"], rm["cost"][order])


def test_kkt_counts_groups(V):
    phi0, phi_T, t_hist, dts, x = _problem(V)
    modes = ["time", "space", "full"]
    opts = [V.make_opt(kappa_sparsity=0.045, alpha_max=2.0e5), V.make_opt(kappa_sparsity=0.012, alpha_max=2.0e5), V.make_opt(alpha_max=100.0)]
    e = V.Engine1D(N=48, batch=3, max_steps=len(dts))
    e.pgd_init(phi0, phi_T, t_hist, dts, opts, sparsity=modes)
    e.pgd_iterate(3)
    k = e.pgd_kkt(refresh=True)
    u, r = e.pgd_get("u"), e.pgd_get("r")
    for b in (0, 1):
        o = opts[b]
        cnt, stat = G.kkt(u[b], r[b], x, t_hist, o.b3, o.kappa_sparsity, o.u_min, o.u_max, modes[b])
        got = [k["n_zero"][b], k["n_small"][b], k["n_match"][b], k["total"][b]]
        assert got == list(cnt), (modes[b], got, cnt)
        assert 0 < cnt[0] < cnt[3]
        assert abs(k["stationarity"][b] - stat) <= 1e-10 * max(stat, 1.0)
    # the full member next to them keeps the node counts of a batch of its own
    e1 = V.Engine1D(N=48, batch=1, max_steps=len(dts))
    e1.pgd_init(phi0[2], phi_T[2], t_hist, dts, [opts[2]])
    e1.pgd_iterate(3)
    k1 = e1.pgd_kkt(refresh=True)
    assert k["total"][2] == 10 * 49 and all(k[key][2] == k1[key][0] for key in ("n_zero", "n_small", "n_match", "total", "stationarity"))
    # the statistic leaves the loop alone
    again = e.pgd_iterate(1)
    e2 = V.Engine1D(N=48, batch=3, max_steps=len(dts))
    e2.pgd_init(phi0, phi_T, t_hist, dts, opts, sparsity=modes)
    e2.pgd_iterate(3)
    plain = e2.pgd_iterate(1)
    assert np.array_equal(again["cost"], plain["cost"]) and np.array_equal(e.pgd_get("u"), e2.pgd_get("u"))
    for q in (e, e1, e2):
        q.close()


def test_refused_calls_leave_the_problem_usable(V):
    phi0, phi_T, t_hist, dts, x = _problem(V)
    VchError = V.module("_lib").VchError
    opts = [V.make_opt(kappa_sparsity=0.045, alpha_max=100.0), V.make_opt(alpha_max=100.0), V.make_opt(kappa_sparsity=0.012, alpha_max=100.0)]
    modes = ["time", "full", "space"]
    plain = _run(V, phi0, phi_T, t_hist, dts, opts, modes, n_iter=2)
    e = V.Engine1D(N=48, batch=3, max_steps=len(dts))
    e.pgd_init(phi0, phi_T, t_hist, dts, opts, sparsity=modes)
    first = e.pgd_iterate(1)
    R = e.RESIDENT
    for call in (lambda: e.pgd_newton(2), lambda: e.pgd_trust(2, 1.0),
                 lambda: e.hess_cg(3, t_hist, opts, u=R, phi_Q=R, phi_T=R, dt=dts),
                 lambda: e.hess_cg_trust(3, 1.0, t_hist, opts, u=R, phi_Q=R, phi_T=R, dt=dts)):
        with pytest.raises(VchError, match="engine error -3"):
            call()
    # a mode outside 0..2 and a group mode whose box does not hold 0: VCH_ERR_ARG, nothing changed
    with pytest.raises(ValueError, match="sparsity"):
        bad = np.array([1, 3, 2], dtype=np.int32)
        arr = (type(opts[0]) * 3)(*opts)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        V.module("_lib").check(e.lib.vch1d_pgd_init_g(e.ctx, dp(phi0), dp(phi_T), None, dp(x), dp(t_hist), len(t_hist), dp(dts), arr, 3,
                                                      None, None, bad.ctypes.data_as(C.POINTER(C.c_int32)), 3, None))
    with pytest.raises(ValueError, match="box"):
        e.pgd_init(phi0, phi_T, t_hist, dts, [V.make_opt(u_min=0.1, u_max=1.0)] * 3, sparsity="time")
    with pytest.raises(ValueError, match="box"):
        e.grad_prox(np.zeros((3, 4, 49)), np.zeros((3, 4, 49)), 1.0, V.make_opt(u_min=-1.0, u_max=-0.1), sparsity="space",
                    t_hist=np.arange(4.0))
    second = e.pgd_iterate(1)
    for key in ("cost", "alpha", "trials", "change"):
        assert np.array_equal(first[key][:, 0], plain[1][key][:, 0], equal_nan=True)
        assert np.array_equal(second[key][:, 0], plain[1][key][:, 1], equal_nan=True)
    assert np.array_equal(e.pgd_get("u").reshape(plain[2].shape), plain[2])
    # an explicit right-hand side concerns the smooth part only and keeps working
    rhs = np.ones((3, len(t_hist), 49))
    out = e.hess_cg(2, t_hist, opts, rhs=rhs, u=R, phi_Q=R, phi_T=R, dt=dts, mask=np.ones((3, len(t_hist), 49), dtype=bool))
    assert np.all(out["steps"] >= 1)
    e.close()
