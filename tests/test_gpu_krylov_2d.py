"""vch2d_hess_lanczos / vch2d_krylov_vector on the GPU: Lanczos on the reduced Hessian P H P of the 2D engine with the basis, the
free set and the recurrence in device memory, against eigvalsh of dense masked Hessians assembled from
Engine2D.hessvec, against the Lanczos relation with Engine2D.hessvec on a second context, and against the NumPy restatement
of the iteration (tests/_lanczos_ref.py, pinned by test_lanczos_ref_cpu.py).

Problems:
    dense    12 x 9, M = 2 (390 nodes): the driver problem of test_gpu_hessvec_2d.py, GEMM-DCT, one tile; the box +-0.5 pins
             200 nodes, the free set (190) is built on the device; dense matrix from 13 hessvec calls of batch 30
    tiles    128 x 32, Ly 0.5, M = 2: 3 x 3 tiles; uploaded mask of 24 free nodes on tile corners, tile edges and interior
             nodes, on all three levels, the middle tile with none; 24 x 24 block from one hessvec call of batch 24
    chunks   16 x 16 (FFT), T = 0.2, dt = 0.01 (21 levels) under VCH_KR_LCHUNK=4: six chunks of levels, the last ragged; 12
             free nodes in the first, a middle and the last chunk; 12 x 12 block from one hessvec call of batch 12

Tolerances, all relative to the largest eigenvalue of the masked matrix.  Where the number of nodes n is known and the
bound 10 n eps is inside the project's 1.5e-11 class, that bound is asserted (dense: n = 390, 9.0e-13 = DRIVER_RITZ of
test_gpu_hessvec_2d.py); elsewhere 10 x the value measured on an MI355X:
    spectrum     dense, both extremes against eigvalsh: measured 6.05e-14 (bound 9.0e-13; the host path measures 4.4e-14)
                 tiles, all 24 Ritz values: measured 4.25e-14, asserted 4.25e-13
                 chunks, all 12 Ritz values: measured 1.51e-13, asserted 1.51e-12
    relation     max_j ||P H q_j - beta_{j-1} q_{j-1} - alpha_j q_j - beta_j q_{j+1}||_inf / lambda_max and ||Q^T Q - I||_max:
                 dense (k = 8) measured 2.61e-15 and 4.44e-16 (bound 9.0e-13)
                 tiles (k = 6) measured 4.05e-15 and 4.44e-16, asserted 4.05e-14 and 4.44e-15
    step 0       alpha_0 against sum q_0 . hv of Engine2D.hessvec(q_0): n eps sum|terms| asserted (4.7e-22 on dense, measured
                 8.3e-25; tiles: equal)
    CPU          first 4 alpha, beta against tests/_lanczos_ref.py on the dense matrix: measured 3.06e-14, asserted 3.06e-13
    stops        the three Ritz values of a free set of 3 nodes against eigvalsh of the 3 x 3 block: measured 2.72e-15
                 (bound 9.0e-13)
    reorth = 0   every Ritz value within its own residual estimate |beta_m s_m| + 10 n eps lambda_max of an eigenvalue
                 (k = 40 on dense: the worst value lies 4.7e-6 lambda_max INSIDE its estimate)
The measured values are in MEASURED below, beside the tolerances derived from them."""
import numpy as np
import pytest

from oracle import vch2d_oracle as o
from _lanczos_ref import lanczos, ritz
from test_gpu_forms import _env
from test_gpu_hessvec_2d import DN, DRIVER_RITZ, EPS, _engine, _problem

pytestmark = pytest.mark.gpu

CLASS = 1.5e-11
# measured on an MI355X (the MEASURE lines of this file), relative to lambda_max
MEASURED = dict(tiles_ritz=4.25e-14, chunks_ritz=1.51e-13, tiles_rel=4.05e-15, tiles_orth=4.44e-16, cpu=3.06e-14)
TOL = {k: 10 * v for k, v in MEASURED.items()}
assert max(TOL.values()) <= CLASS and DRIVER_RITZ <= CLASS


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


def _tile(a, nb):
    return np.ascontiguousarray(np.broadcast_to(a, (nb,) + np.shape(a)))


class Problem:
    """One base point (grid, march, control, targets) from which contexts of any batch are made."""

    def __init__(self, V, P, t, dts, x, y, phi0, u, opt, env=None, max_steps=None):
        self.V, self.P, self.t, self.dts, self.x, self.y, self.phi0, self.u, self.opt = V, P, t, dts, x, y, phi0, u, opt
        self.M, self.env = len(dts), env or {}
        self.max_steps = self.M if max_steps is None else max_steps      # of the contexts made here: the march may be shorter
        e = _engine(V, P, 1, max_steps=self.M)
        hist, _ = e.forward(phi0, dts, u=u)
        e.close()
        self.phi_T, self.phi_Q = o.build_targets(x, y, t, hist[0], P.Lx, P.Ly, P.T)
        self.shape = u.shape

    def context(self, nb):
        with _env(**self.env):
            eng = _engine(self.V, self.P, nb, max_steps=self.max_steps)
        eng.forward(_tile(self.phi0, nb), self.dts, u=_tile(self.u, nb), store=False)
        return eng

    def kw(self, nb):
        return dict(dt=self.dts, t_hist=self.t, phi_Q=_tile(self.phi_Q, nb), phi_T=_tile(self.phi_T, nb), x=self.x, y=self.y)

    def hessvec(self, H):
        """H h for the directions H (nb, M+1, ..) on a context of their own."""
        nb = len(H)
        eng = self.context(nb)
        r = eng.hessvec(np.ascontiguousarray(H), opt=self.opt, **self.kw(nb))
        eng.close()
        assert r["stats"]["unconverged_solves"] == 0
        return r["hv"]

    def block(self, nodes):
        """The symmetrised block of the Hessian on the flat node indices `nodes`: one hessvec call of batch len(nodes)."""
        E = np.zeros((len(nodes), self.u.size))
        E[np.arange(len(nodes)), nodes] = 1.0
        hv = self.hessvec(E.reshape((len(nodes),) + self.shape)).reshape(len(nodes), -1)
        A = hv[:, nodes]
        return 0.5 * (A + A.T)


def _q0(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape)


def _mask_of(shape, nodes):
    m = np.zeros(int(np.prod(shape)), dtype=bool)
    m[nodes] = True
    return m.reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------
# the three problems
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense(V):
    K2 = V.module("Vch_control_2D.config")
    F2 = V.module("Vch_control_2D.Forward2_solver")
    S2 = V.module("Vch_control_2D.second_order_conditions_2d")
    Nx, Ny, T, dt = DN["Nx"], DN["Ny"], DN["T"], DN["dt"]
    cfg = K2.ForwardSolverConfig.model_construct(Nx=Nx, Ny=Ny, T=T, dt_initial=dt)
    ocfg = K2.OptimizationConfig()
    P = o.Params2D(Nx=Nx, Ny=Ny, Lx=cfg.Lx, Ly=cfg.Ly, tau=cfg.tau, gamma=cfg.gamma, c1=cfg.c1, c2=cfg.c2, kappa=cfg.kappa,
                   T=T, dt_initial=dt)
    t, dts = V.time_grid(T, dt)
    x, y = np.linspace(0.0, cfg.Lx, Nx + 1), np.linspace(0.0, cfg.Ly, Ny + 1)
    xx, yy = np.meshgrid(x / cfg.Lx, y / cfg.Ly, indexing="ij")
    u_star = np.clip(np.stack([1.4 * np.cos(np.pi * xx * (1 + k % 3)) * np.cos(np.pi * yy) * np.sin(1 + k) for k in range(3)]),
                     DN["u_min"], DN["u_max"])
    phi0 = F2.init_phi_random(Nx, Ny, 1e-2, amp=0.1, seed=42)
    box = V.make_opt(ocfg, u_min=DN["u_min"], u_max=DN["u_max"])
    pr = Problem(V, P, t, dts, x, y, phi0, u_star, box)
    nd, nb = u_star.size, 30
    Hd = np.empty((nd, nd))
    eng = pr.context(nb)
    for k0 in range(0, nd, nb):
        E = np.zeros((nb, nd))
        E[np.arange(nb), k0 + np.arange(nb)] = 1.0
        r = eng.hessvec(E.reshape((nb,) + u_star.shape), opt=box, **pr.kw(nb))
        assert r["stats"]["unconverged_solves"] == 0
        Hd[:, k0:k0 + nb] = r["hv"].reshape(nb, nd).T
    eng.close()
    pr.Hm = 0.5 * (Hd + Hd.T)
    pr.mask = S2.free_set(u_star, DN["u_min"], DN["u_max"])
    pr.free = np.flatnonzero(pr.mask.ravel())
    assert len(pr.free) == 190 and nd == 390
    pr.ev = np.linalg.eigvalsh(pr.Hm[np.ix_(pr.free, pr.free)])
    pr.cfg, pr.ocfg, pr.S2 = cfg, ocfg, S2
    return pr


@pytest.fixture(scope="module")
def tiles(V):
    p = _problem("tiles")
    pr = Problem(V, p["P"], p["t"], p["dts"], p["x"], p["y"], p["phi0"][0], p["U"][0], V.make_opt())
    ns, nf = p["P"].Ny + 1, p["P"].Nx + 1                   # the engine's plane: ns rows of nf entries of the flat field
    assert (ns, nf) == (33, 129)
    nodes = []
    for ts in range(3):
        for tf in range(3):
            if (ts, tf) == (1, 1):
                continue                                     # the middle tile has no free node
            rows = [16 * ts, min(16 * ts + 15, ns - 1), min(16 * ts + 7, ns - 1)]
            cols = [64 * tf, min(64 * tf + 63, nf - 1), min(64 * tf + 31, nf - 1)]
            for lvl, (r, c) in enumerate([(rows[0], cols[0]), (rows[1], cols[2]), (rows[2], cols[2])]):
                nodes.append(lvl * ns * nf + r * nf + c)     # a tile corner, a tile edge, an interior node
    pr.free = np.array(sorted(set(nodes)))
    assert len(pr.free) == 24
    pr.mask = _mask_of(pr.shape, pr.free)
    pr.A = pr.block(pr.free)
    pr.ev = np.linalg.eigvalsh(pr.A)
    return pr


@pytest.fixture(scope="module")
def chunks(V):
    N, T, dt = 16, 0.2, 0.01
    P = o.Params2D(Nx=N, Ny=N, T=T, dt_initial=dt)
    t, dts = o.time_grid(T, dt)
    assert len(dts) == 20
    x = np.linspace(0.0, 1.0, N + 1)
    xx, yy = np.meshgrid(x, x, indexing="ij")
    u = np.stack([12.0 * np.cos(np.pi * xx * (1 + k % 3)) * np.cos(np.pi * yy) * np.sin(1 + k) for k in range(len(t))])
    phi0 = o.init_phi_random(N, N, o.DELTA_SEP, amp=0.1, seed=42)
    pr = Problem(V, P, t, dts, x, x, phi0, u, V.make_opt(), env=dict(VCH_KR_LCHUNK=4))
    lev = (N + 1) ** 2
    # chunks of four levels: 0-3, ..., 16-19 and the ragged last one {20}
    at = [(0, 5), (1, 77), (3, 288), (2, 140), (8, 0), (9, 16), (10, 150), (11, 201), (20, 3), (20, 144), (20, 271), (20, 288)]
    pr.free = np.array(sorted(l * lev + n for l, n in at))
    assert len(pr.free) == 12
    pr.mask = _mask_of(pr.shape, pr.free)
    pr.A = pr.block(pr.free)
    pr.ev = np.linalg.eigvalsh(pr.A)
    return pr


def _check_stats(st, rtol=1e-12):
    assert st["unconverged_solves"] == 0, st
    assert st["max_lin_relres"] <= rtol, st


# ---------------------------------------------------------------------------------------------------------------------
# 1. spectrum
# ---------------------------------------------------------------------------------------------------------------------
def test_dense_extremes_with_the_free_set_built_on_the_device(dense):
    pr = dense
    eng = pr.context(1)
    R = eng.hess_lanczos(_q0(pr.shape, 1), 190, opt=pr.opt, **pr.kw(1))
    eng.close()
    _check_stats(R["stats"])
    assert R["n_free"][0] == 190 and R["steps"][0] <= 190
    theta, _, _ = ritz(R["alpha"][0], R["beta"][0], R["steps"][0])
    dev = max(abs(theta[0] - pr.ev[0]), abs(theta[-1] - pr.ev[-1])) / pr.ev[-1]
    print(f"MEASURE dense: steps {R['steps'][0]} theta_min {theta[0]:.6e} eigvalsh {pr.ev[0]:.6e} theta_max {theta[-1]:.6e} "
          f"eigvalsh {pr.ev[-1]:.6e} rel.dev {dev:.2e}; stats {R['stats']}")
    assert dev < DRIVER_RITZ


@pytest.mark.parametrize("name", ["tiles", "chunks"])
def test_all_ritz_values_of_a_small_uploaded_free_set(request, name):
    pr = request.getfixturevalue(name)
    n = len(pr.free)
    eng = pr.context(1)
    R = eng.hess_lanczos(_q0(pr.shape, 2), n + 5, opt=pr.opt, mask=pr.mask, **pr.kw(1))
    # the basis: masked-off nodes exact zeros
    Q = np.stack([eng.krylov_vector(np.eye(1, j + 1, j))[0] for j in range(min(3, int(R["steps"][0])))])
    eng.close()
    _check_stats(R["stats"])
    assert R["n_free"][0] == n and R["steps"][0] == n
    assert not Q[:, ~pr.mask].any() and np.abs(Q).max() > 0
    theta, _, _ = ritz(R["alpha"][0], R["beta"][0], n)
    dev = np.abs(theta - pr.ev).max() / pr.ev[-1]
    print(f"MEASURE {name}: all {n} Ritz values against eigvalsh {dev:.2e}; spectrum {pr.ev[0]:.4e} .. {pr.ev[-1]:.4e}")
    assert dev < TOL[name + "_ritz"]


# ---------------------------------------------------------------------------------------------------------------------
# 2. Lanczos relation and basis; 4c. the step-0 identity
# ---------------------------------------------------------------------------------------------------------------------
def _relation(pr, k, mask_arg):
    eng = pr.context(1)
    R = eng.hess_lanczos(_q0(pr.shape, 3), k, opt=pr.opt, mask=mask_arg, **pr.kw(1))
    assert R["steps"][0] == k
    Q = np.stack([eng.krylov_vector(np.eye(1, j + 1, j))[0] for j in range(k + 1)])
    eng.close()
    HQ = pr.hessvec(Q[:k])                                           # Engine2D.hessvec on a second context
    a, b, lam = R["alpha"][0], R["beta"][0], pr.ev[-1]
    assert not Q[:, ~pr.mask].any()                                  # masked-off nodes of every q_j are exact zeros
    rel = 0.0
    for j in range(k):
        r = np.where(pr.mask, HQ[j], 0.0) - a[j] * Q[j] - b[j] * Q[j + 1] - (b[j - 1] * Q[j - 1] if j else 0.0)
        rel = max(rel, np.abs(r).max() / lam)
    Qf = Q.reshape(k + 1, -1)
    orth = np.abs(Qf @ Qf.T - np.eye(k + 1)).max()
    # step 0: alpha_0 is the device's sum of q_0 . hv (plus the second round's correction, round-off of it)
    t0 = Q[0] * HQ[0]
    ident = abs(a[0] - t0.sum()), Q[0].size * EPS * np.abs(t0).sum()
    return rel, orth, ident


def test_lanczos_relation_and_basis_dense(dense):
    rel, orth, ident = _relation(dense, 8, None)
    print(f"MEASURE dense k=8: relation {rel:.2e} orthogonality {orth:.2e} step-0 identity {ident[0]:.2e} (bound {ident[1]:.2e})")
    assert rel < DRIVER_RITZ and orth < DRIVER_RITZ
    assert ident[0] <= ident[1]


def test_lanczos_relation_and_basis_tiles(tiles):
    rel, orth, ident = _relation(tiles, 6, tiles.mask)
    print(f"MEASURE tiles k=6: relation {rel:.2e} orthogonality {orth:.2e} step-0 identity {ident[0]:.2e} (bound {ident[1]:.2e})")
    assert rel < TOL["tiles_rel"] and orth < TOL["tiles_orth"]
    assert ident[0] <= ident[1]


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the CPU restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_first_steps_agree_with_the_cpu_restatement(dense):
    pr = dense
    q0 = _q0(pr.shape, 4)
    eng = pr.context(1)
    R = eng.hess_lanczos(q0, 8, opt=pr.opt, **pr.kw(1))
    eng.close()
    ref = lanczos(lambda v: pr.Hm @ v, pr.mask, q0, 8)
    lam = pr.ev[-1]
    dev = max(np.abs(R["alpha"][0, :4] - ref["alpha"][:4]).max(), np.abs(R["beta"][0, :4] - ref["beta"][:4]).max()) / lam
    print(f"MEASURE cpu restatement: first 4 alpha, beta {dev:.2e} of lambda_max")
    assert dev < TOL["cpu"]


# ---------------------------------------------------------------------------------------------------------------------
# 4a, 7. a batch of three with different masks and boxes; the stops
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_of_three_equals_three_single_contexts_and_the_stops(dense):
    pr, V = dense, dense.V
    masks = np.stack([_mask_of(pr.shape, pr.free[[4, 77, 150]]), _mask_of(pr.shape, pr.free[[0, 20, 40, 90, 120, 160, 189]]),
                      pr.mask])
    opts = [V.make_opt(pr.ocfg, u_min=-0.5, u_max=0.5), V.make_opt(pr.ocfg, u_min=-0.3, u_max=0.4),
            V.make_opt(pr.ocfg, u_min=-2.0, u_max=2.0)]
    q0 = _q0((3,) + pr.shape, 5)
    k = 12
    eng = pr.context(3)
    many = eng.hess_lanczos(q0, k, opt=opts, mask=masks, **pr.kw(3))
    eng.close()
    _check_stats(many["stats"])
    assert list(many["n_free"]) == [3, 7, 190] and list(many["steps"]) == [3, 7, 12]
    for b in range(3):
        eng = pr.context(1)
        one = eng.hess_lanczos(q0[b], k, opt=opts[b], mask=masks[b], **pr.kw(1))
        eng.close()
        for key in ("alpha", "beta", "steps", "n_free"):
            assert np.array_equal(one[key][0], many[key][b], equal_nan=True), (key, b)
    # the stops: n_free = 3 with k = 12 takes three steps, the rest is NaN, and the three Ritz values are the block's
    a, bt = many["alpha"][0], many["beta"][0]
    assert np.isnan(a[3:]).all() and np.isnan(bt[3:]).all() and np.isfinite(a[:3]).all() and np.isfinite(bt[:3]).all()
    assert np.isnan(many["alpha"][1][7:]).all() and np.isfinite(many["alpha"][2]).all()
    nodes = pr.free[[4, 77, 150]]
    ev3 = np.linalg.eigvalsh(pr.Hm[np.ix_(nodes, nodes)])
    theta, _, _ = ritz(a, bt, 3)
    dev = np.abs(theta - ev3).max() / ev3[-1]
    print(f"MEASURE stops: three Ritz values of n_free = 3 against eigvalsh {dev:.2e}")
    assert dev < DRIVER_RITZ


# ---------------------------------------------------------------------------------------------------------------------
# 4b, 5. the cached gradient sweep: bits and solve counts
# ---------------------------------------------------------------------------------------------------------------------
def test_cached_sweep_has_the_bits_of_the_repeated_one_and_the_solve_counts(dense):
    pr = dense
    q0, k, B = _q0((2,) + pr.shape, 6), 5, 2
    eng = pr.context(B)
    got = eng.hess_lanczos(q0, k, opt=pr.opt, **pr.kw(B))
    eng.close()
    with _env(VCH_KRYLOV_NOCACHE=1):
        eng = pr.context(B)
    ref = eng.hess_lanczos(q0, k, opt=pr.opt, **pr.kw(B))
    eng.close()
    for key in ("alpha", "beta", "steps", "n_free"):
        assert np.array_equal(got[key], ref[key], equal_nan=True), key
    assert list(got["steps"]) == [k, k]
    _check_stats(got["stats"])
    _check_stats(ref["stats"])
    assert got["stats"]["linear_solves"] == B * pr.M * (2 * k + 1), got["stats"]
    assert ref["stats"]["linear_solves"] == 3 * B * pr.M * k, ref["stats"]


# ---------------------------------------------------------------------------------------------------------------------
# 6. without reorthogonalisation
# ---------------------------------------------------------------------------------------------------------------------
def test_three_term_recurrence(dense):
    pr, V = dense, dense.V
    eng = pr.context(1)
    R = eng.hess_lanczos(_q0(pr.shape, 7), 40, opt=pr.opt, reorth=False, **pr.kw(1))
    _check_stats(R["stats"])
    assert R["steps"][0] == 40
    with pytest.raises(V.VchError, match="-3"):          # q_0 is no longer held
        eng.krylov_vector(np.ones((1, 1)))
    eng.close()
    theta, S, res = ritz(R["alpha"][0], R["beta"][0], 40)
    slack = DRIVER_RITZ * pr.ev[-1]
    worst = max(np.abs(pr.ev - th).min() - rs for th, rs in zip(theta, res))
    print(f"MEASURE reorth=0 k=40: worst (distance to an eigenvalue - residual estimate) {worst / pr.ev[-1]:.2e} of lambda_max")
    for th, rs in zip(theta, res):
        assert np.abs(pr.ev - th).min() <= rs + slack, (th, rs)


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors and memory
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_any_launch_and_data_errors_name_the_trajectory(dense):
    pr, V = dense, dense.V
    q0 = _q0((2,) + pr.shape, 8)
    eng = pr.context(2)
    kw = pr.kw(2)
    c0 = eng.counters()
    for bad in (dict(k=0), dict(k=-3), dict(q0=None), dict(reorth=2), dict(reorth=-1)):
        args = dict(q0=q0, k=4, opt=pr.opt, **kw)
        args.update(bad)
        with pytest.raises(ValueError):
            eng.hess_lanczos(**args)
        assert eng.counters() == c0, bad
    # the row rule: a march under a control of fewer than M + 1 rows has no direction of M + 1 rows
    short = _engine(V, pr.P, 2, max_steps=pr.M)
    short.forward(_tile(pr.phi0, 2), pr.dts, u=_tile(pr.u[:2], 2), store=False)
    c1 = short.counters()
    with pytest.raises(ValueError, match="rows"):
        short.hess_lanczos(q0, 4, opt=pr.opt, **kw)
    assert short.counters() == c1
    short.close()
    # data-dependent: an empty free set, a start vector that vanishes on the free set
    masks = np.stack([pr.mask, np.zeros_like(pr.mask)])
    with pytest.raises(ValueError, match="trajectory 1"):
        eng.hess_lanczos(q0, 4, opt=pr.opt, mask=masks, **kw)
    with pytest.raises(ValueError, match="trajectory 0"):
        eng.hess_lanczos(q0, 4, opt=[V.make_opt(pr.ocfg, u_min=0.6, u_max=0.7), pr.opt], **kw)      # no node inside that box
    qz = q0.copy()
    qz[1][pr.mask] = 0.0
    with pytest.raises(ValueError, match="trajectory 1"):
        eng.hess_lanczos(qz, 4, opt=pr.opt, **kw)
    with pytest.raises(V.VchError, match="-3"):          # the failed calls left no basis
        eng.krylov_vector(np.ones((2, 1)))
    good = eng.hess_lanczos(q0, 4, opt=pr.opt, **kw)
    eng.close()
    fresh = pr.context(2)
    want = fresh.hess_lanczos(q0, 4, opt=pr.opt, **kw)
    with pytest.raises(ValueError):
        fresh.krylov_vector(np.ones((2, 6)))             # m above steps + 1
    fresh.close()
    for key in ("alpha", "beta", "steps", "n_free"):
        assert np.array_equal(good[key], want[key], equal_nan=True), key


def test_refused_allocations_and_the_balance(dense):
    pr, V = dense, dense.V
    lib = V.load()
    q0 = _q0(pr.shape, 9)
    base = lib.vch_mem_live()
    eng = pr.context(1)
    live0 = lib.vch_mem_live()
    want = eng.hess_lanczos(q0, 6, opt=pr.opt, **pr.kw(1))
    m = lib.vch_mem_live() - live0
    again = eng.hess_lanczos(q0, 6, opt=pr.opt, **pr.kw(1))
    assert lib.vch_mem_live() - live0 == m                # the second invocation allocates nothing
    bigger = eng.hess_lanczos(q0, 9, opt=pr.opt, **pr.kw(1))
    assert lib.vch_mem_live() - live0 == m                # a larger basis replaces the storage
    eng.close()
    assert lib.vch_mem_live() == base
    print("lazy requests of the first call:", m)
    assert m >= 4
    for key in ("alpha", "beta", "steps"):
        assert np.array_equal(again[key], want[key], equal_nan=True), key
    assert np.array_equal(bigger["alpha"][:, :6], want["alpha"]) and np.array_equal(bigger["beta"][:, :6], want["beta"])
    for i in range(m):
        eng = pr.context(1)
        live0 = lib.vch_mem_live()
        lib.vch_mem_refuse_after(i)
        try:
            with pytest.raises(V.VchError, match="-2|-4") as err:
                eng.hess_lanczos(q0, 6, opt=pr.opt, **pr.kw(1))
        finally:
            lib.vch_mem_refuse_after(-1)
        assert lib.vch_mem_live() == live0, (i, lib.vch_mem_live() - live0)
        if "Krylov storage" in str(err.value):
            assert "bytes" in str(err.value)
        got = eng.hess_lanczos(q0, 6, opt=pr.opt, **pr.kw(1))
        assert lib.vch_mem_live() - live0 == m
        for key in ("alpha", "beta", "steps", "n_free"):
            assert np.array_equal(got[key], want[key], equal_nan=True), (key, i)
        eng.close()
        assert lib.vch_mem_live() == base


# ---------------------------------------------------------------------------------------------------------------------
# 9. about a PGD iterate
# ---------------------------------------------------------------------------------------------------------------------
def test_pgd_iterate_free_set_from_the_resident_control_and_an_undisturbed_run(V):
    S2 = V.module("Vch_control_2D.second_order_conditions_2d")
    N, T, dt = 16, 0.05, 0.01
    P = o.Params2D(Nx=N, Ny=N, T=T, dt_initial=dt)
    t, dts = o.time_grid(T, dt)
    x = np.linspace(0.0, 1.0, N + 1)
    phi0 = np.stack([o.init_phi_random(N, N, o.DELTA_SEP, amp=0.1, seed=42 + b) for b in range(2)])
    phi_T = np.stack([o.build_targets(x, x, t, phi0[b], P.Lx, P.Ly, P.T)[0] for b in range(2)])

    def start(opts):
        eng = _engine(V, P, 2)
        eng.pgd_init(phi0, phi_T, t, opts, ramp=True, T=T)
        eng.pgd_iterate(2)
        return eng

    # the scale of the control under a wide box, then a box of its own per trajectory that pins part of the nodes
    probe = start([V.make_opt(), V.make_opt(b1=2.0, b2=4.0, b3=1e-3)])
    top = np.abs(probe.pgd_get("u")).reshape(2, -1).max(axis=1)
    probe.close()
    assert top.min() > 0
    opts = [V.make_opt(u_min=-0.5 * top[0], u_max=0.25 * top[0]), V.make_opt(b1=2.0, b2=4.0, b3=1e-3, u_min=-0.1 * top[1], u_max=0.6 * top[1])]
    plain = start(opts)
    want = plain.pgd_iterate(1)
    u_want = plain.pgd_get("u")
    plain.close()
    eng = start(opts)
    u, phi = eng.pgd_get("u"), eng.pgd_get("phi")
    R = eng.hess_lanczos(_q0(u.shape, 10), 5, opt=opts)
    _check_stats(R["stats"])
    nf = [int(S2.free_set(u[b], opts[b].u_min, opts[b].u_max).sum()) for b in range(2)]
    print(f"MEASURE pgd: n_free {list(R['n_free'])} of {u[0].size}, free_set() {nf}, steps {list(R['steps'])}")
    assert list(R["n_free"]) == nf and 0 < min(nf) and max(nf) < u[0].size
    assert np.array_equal(eng.pgd_get("u"), u) and np.array_equal(eng.pgd_get("phi"), phi)
    got = eng.pgd_iterate(1)
    for key in ("cost", "alpha", "attempts", "change", "tracking_error", "terminal_error"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(eng.pgd_get("u"), u_want)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. the driver
# ---------------------------------------------------------------------------------------------------------------------
def test_driver_on_device(dense):
    pr, S2 = dense, dense.S2
    kw = dict(x=pr.x, y=pr.y, t_hist=pr.t, opt_config=pr.ocfg, phi_Q_target=pr.phi_Q, phi_T_target=pr.phi_T, fwd_config=pr.cfg,
              u_min=DN["u_min"], u_max=DN["u_max"], k=390, seed=DN["seed"])
    host = S2.reduced_hessian_extremes_2d(pr.u, **kw)
    dev = S2.reduced_hessian_extremes_2d(pr.u, on_device=True, vector=True, **kw)
    assert set(dev) == set(host) | {"v_min"}
    assert dev["n_free"] == host["n_free"] == 190 and dev["steps"] <= dev["n_free"] and len(dev["ritz"]) == dev["steps"]
    lam = pr.ev[-1]
    for name, R in (("host", host), ("device", dev)):
        d = max(abs(R["theta_min"] - pr.ev[0]), abs(R["theta_max"] - pr.ev[-1])) / lam
        print(f"MEASURE driver {name}: steps {R['steps']} theta_min {R['theta_min']:.6e} theta_max {R['theta_max']:.6e} rel.dev {d:.2e} "
              f"residuals {R['res_min']:.1e} {R['res_max']:.1e}")
        assert d < DRIVER_RITZ
    v = dev["v_min"]
    assert v.shape == pr.u.shape and abs(np.linalg.norm(v) - 1.0) < 10 * EPS and not v[~pr.mask].any()
    eng = pr.context(1)
    so = eng.second_order(v[None], pr.dts, pr.t, pr.opt, phi_Q=pr.phi_Q[None], phi_T=pr.phi_T[None], x=pr.x, y=pr.y)
    eng.close()
    rq = float(so["c_gn"][0] + so["c_state"][0] + so["c_ctrl"][0])
    print(f"MEASURE driver: Rayleigh quotient of v_min {rq:.6e} theta_min {dev['theta_min']:.6e} res_min {dev['res_min']:.1e}")
    assert abs(rq - dev["theta_min"]) <= dev["res_min"] + DRIVER_RITZ * lam
    with pytest.raises(ValueError):
        S2.reduced_hessian_extremes_2d(pr.u, vector=True, **kw)
    with pytest.raises(ValueError):
        S2.reduced_hessian_extremes_2d(pr.u, on_device=True, vector=True, reorth=False, **kw)
