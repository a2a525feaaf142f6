"""Directional sparsity in the 2D engine on the GPU: the group prox of both modes against the NumPy
restatement (tests/_group_prox_ref_2d.py) on one tile, ragged tiles with a pad column, a column of tiles and 3 x 3 tiles;
that the full-sparsity paths keep their bits; the cost; the resident loop in a mixed batch; three iterations against the
restatement's loop over the oracle; the KKT statistic by groups; the refused calls.  Measured floors are in
profiles/dirsparse_2d_edges.txt."""
import ctypes as C

import numpy as np
import pytest

import _dirsparse_2d_cases as K
import _group_prox_ref_2d as G
from conftest import relerr

pytestmark = pytest.mark.gpu

BOXES, SHAPES, ROWS = K.BOXES, K.SHAPES, K.ROWS
MAXSTEPS = 32                        # rows <= 33


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


@pytest.fixture(scope="module")
def O2():
    from oracle import vch2d_oracle
    return vch2d_oracle


@pytest.fixture(scope="module")
def engines(V):
    made = {}

    def get(Nx, Ny, batch=K.BATCH, max_steps=MAXSTEPS):
        key = (Nx, Ny, batch, max_steps)
        if key not in made:
            made[key] = V.Engine2D(Nx=Nx, Ny=Ny, batch=batch, max_steps=max_steps)
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


# ---- 1. the prox seam ------------------------------------------------------------------------------------------------------
def _check_seam(V, eng, case, label):
    """One seam call against the restatement.  Tolerances: 1e-12 on s, 1e-12 max|v| on u+ (the 1D tests' own)."""
    mode, lo, hi, al, ks = case["mode"], case["lo"], case["hi"], case["alpha"], case["ks"]
    u, r, x, y, t = case["u"], case["r"], case["x"], case["y"], case["t"]
    m_c, m_b = K.decision_margins(case)
    assert m_c >= 1e-9 and m_b >= 1e-9, (label, m_c, m_b)
    opt = V.make_opt(b3=0.0, kappa_sparsity=ks, u_min=lo, u_max=hi)
    up, s = eng.grad_prox(u, r, al, opt, sparsity=mode, x=x, y=y, t_hist=t, return_scale=True)
    kinds, worst_s, worst_u = set(), 0.0, 0.0
    for b in range(u.shape[0]):
        ur, sr, kr = G.prox(u[b], r[b], al, 0.0, ks, lo, hi, mode, x, y, t)
        kr = np.array(kr)
        kinds |= set(kr)
        v = u[b] - al * r[b]
        worst_s = max(worst_s, float(np.max(np.abs(s[b] - sr))))
        worst_u = max(worst_u, float(np.max(np.abs(up[b] - ur)) / np.max(np.abs(v))))
        assert np.array_equal(s[b].ravel() == 0.0, kr == "zero"), label
        # a closed-form group is s v to the bit; a box-active one has an entry the box holds
        sv = (s[b][:, None, None] if mode == "time" else s[b][None]) * v
        same = np.all(G.groups(up[b], mode) == G.groups(sv, mode), axis=1)
        assert np.array_equal(same[kr != "zero"], (kr == "closed")[kr != "zero"]), label
        assert np.max(np.abs(s[b] - sr)) <= 1e-12, (label, b)
        assert np.max(np.abs(up[b] - ur)) <= 1e-12 * np.max(np.abs(v)), (label, b)
    print(f"{label}: margins c {m_c:.1e} box {m_b:.1e}  |s - s_ref| {worst_s:.2e}  |u+ - ref| / max|v| {worst_u:.2e}  {sorted(kinds)}")
    return kinds


@pytest.mark.parametrize("mode", ["time", "space"])
@pytest.mark.parametrize("shape", SHAPES)
def test_group_prox_seam_against_the_restatement(V, engines, mode, shape):
    Nx, Ny = shape
    eng = engines(Nx, Ny)
    for rows in ROWS:
        for lo, hi in BOXES:
            kinds = _check_seam(V, eng, K.seam_case(mode, Nx, Ny, rows, lo, hi), f"{mode} {shape} rows {rows} box ({lo}, {hi})")
            assert kinds == ({"zero", "closed"} if np.isinf(hi) else {"zero", "closed", "box"})


@pytest.mark.parametrize("mode", ["time", "space"])
def test_group_prox_seam_projection_when_lambda_is_zero(V, engines, mode):
    """kappa_s = 0: the prox is the projection, s = 1.0 and u+ = clip(v) to the bit."""
    Nx, Ny = 70, 20
    eng = engines(Nx, Ny)
    case = K.seam_case(mode, Nx, Ny, 17, -0.3, 2.0, ks=0.0)
    opt = V.make_opt(b3=0.0, kappa_sparsity=0.0, u_min=-0.3, u_max=2.0)
    up, s = eng.grad_prox(case["u"], case["r"], case["alpha"], opt, sparsity=mode, x=case["x"], y=case["y"], t_hist=case["t"],
                          return_scale=True)
    assert np.all(s == 1.0)
    assert np.array_equal(up, np.clip(case["u"] - case["alpha"] * case["r"], -0.3, 2.0))


@pytest.mark.parametrize("mode", ["time", "space"])
def test_group_prox_seam_at_rho_over_lambda_1e6(V, engines, mode):
    """lam = 1e-6 against box-active groups of norm ~1: the root sits 1e-6 below 1."""
    Nx, Ny = 70, 20
    kinds = _check_seam(V, engines(Nx, Ny), K.seam_case(mode, Nx, Ny, 17, -1.0, 1.0, ks=2e-6), f"{mode} rho/lam 1e6")
    assert "box" in kinds


@pytest.mark.parametrize("mode", ["time", "space"])
def test_group_prox_seam_with_a_weightless_line_of_nodes(V, engines, mode):
    """An x grid with one node three times: the nodes of that line have W = 0 and carry entries of 50.  In time mode they
    drop out of their level's norm.  In space mode the repeated x node weighs nothing in the prox: the pencil kernels read
    wt only, never W, so this case is an ordinary one there; a level of weight zero (a repeated t) is
    tests/test_gpu_dirsparse_edges_2d.py::test_seam_on_nodes_and_levels_of_zero_weight[zero_t-...]."""
    Nx, Ny = 70, 20
    case = K.seam_case(mode, Nx, Ny, 17, -1.0, 1.0, triple_x=True)
    assert np.count_nonzero(G.plane_w(case["x"], case["y"]) == 0.0) == Ny + 1
    kinds = _check_seam(V, engines(Nx, Ny), case, f"{mode} weightless line")
    assert "box" in kinds


# ---- 2. full mode keeps its bits ----------------------------------------------------------------------------------------------
def _small_problem(V, O2, N=16, steps=6, batch=2):
    P = O2.Params2D(Nx=N, Ny=N, T=steps * 1e-2, dt_initial=1e-2)
    t, dts = V.time_grid(P.T, 1e-2)
    phi0 = np.stack([O2.init_phi_random(N, N, 1e-2, amp=0.1, seed=42 + b) for b in range(batch)])
    x = np.linspace(0.0, 1.0, N + 1)
    phi_T = np.repeat(O2.build_targets(x, x, t, phi0[0], 1.0, 1.0, P.T)[0][None], batch, axis=0)
    return P, phi0, phi_T, np.asarray(t), x


def test_full_mode_keeps_its_bits(V, O2, engines):
    N, B = 16, 2
    P, phi0, phi_T, t, x = _small_problem(V, O2)
    eng, lib, chk = engines(N, N, B, 8), None, V.module("_lib").check
    lib = eng.lib
    rng = np.random.default_rng(5)
    rows = t.size
    u, r = 0.3 * rng.standard_normal((B, rows, N + 1, N + 1)), 0.1 * rng.standard_normal((B, rows, N + 1, N + 1))
    phi, pq = rng.uniform(-0.5, 0.5, u.shape), rng.uniform(-0.5, 0.5, u.shape)
    opt = V.make_opt(kappa_sparsity=0.02, u_min=-0.2, u_max=0.3)
    al = np.array([0.5, 1.7])
    old = eng.grad_prox(u, r, al, opt)
    new, scale = np.empty_like(u), np.full((B, rows), 7.0)
    chk(lib.vch2d_grad_prox_g(eng.ctx, _dp(u), _dp(r), rows, _dp(x), _dp(x), _dp(t), _dp(al), C.byref(opt), 0, _dp(new), _dp(scale)))
    assert np.array_equal(old, new) and np.all(scale == 7.0)
    Jo = eng.cost(phi, u, pq, phi_T, t, opt)
    Jn = np.empty((B, 5))
    chk(lib.vch2d_cost_g(eng.ctx, _dp(phi), _dp(u), _dp(pq), _dp(phi_T), rows - 1, _dp(x), _dp(x), _dp(t), C.byref(opt), 0, _dp(Jn)))
    assert np.array_equal(Jo, Jn)
    opts = [V.make_opt(O2.OptParams()), V.make_opt(O2.OptParams(kappa_sparsity=3e-4, u_min=-0.01, u_max=0.02))]
    runs = []
    for sparsity in (None, "full", ["full", "full"]):
        J0 = eng.pgd_init(phi0, phi_T, t, opts, T=P.T, alpha0=[20.0, 50.0], sparsity=sparsity)
        res = eng.pgd_iterate(3)
        runs.append((J0, res, eng.pgd_get("u"), eng.pgd_get("phi")))
    for J0, res, uu, ph in runs[1:]:
        assert np.array_equal(J0, runs[0][0]) and np.array_equal(uu, runs[0][2]) and np.array_equal(ph, runs[0][3])
        for key in ("cost", "alpha", "attempts", "change", "tracking_error", "terminal_error"):
            assert np.array_equal(res[key], runs[0][1][key]), key


# ---- 3. the cost --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["time", "space"])
@pytest.mark.parametrize("shape", [(16, 16), (70, 20)])
def test_cost_of_both_modes(V, O2, engines, mode, shape):
    """J1..J3 are the oracle's (1e-12) and J4 is j4 of the restatement to 1e-13 relative: a sum of up to 1491 positive
    terms in another order differs by a few ulps."""
    Nx, Ny = shape
    eng = engines(Nx, Ny)
    rng = np.random.default_rng(11)
    rows = 17
    x, y, t = K.grids(rng, Nx, Ny, rows)
    shp = (K.BATCH, rows, Nx + 1, Ny + 1)
    phi, pq, u = rng.uniform(-0.5, 0.5, shp), rng.uniform(-0.5, 0.5, shp), rng.standard_normal(shp)
    u[:, 3] = 0.0
    u[:, :, 5, :] = 0.0
    pt = rng.uniform(-0.5, 0.5, (K.BATCH, Nx + 1, Ny + 1))
    O = O2.OptParams(b1=3.0, b2=7.0, b3=0.2, kappa_sparsity=0.03)
    J = eng.cost(phi, u, pq, pt, t, V.make_opt(O), x=x, y=y, sparsity=mode)
    for b in range(K.BATCH):
        ref = O2.cost_parts(phi[b], u[b], pq[b], pt[b], x, y, t, O)
        j4 = G.j4(u[b], x, y, t, O.kappa_sparsity, mode)
        print(f"{mode} {shape} b {b}: J4 {J[b, 3]:.15e} ref {j4:.15e} rel {abs(J[b, 3] / j4 - 1):.1e}")
        assert np.allclose(J[b, :3], ref[:3], rtol=1e-12, atol=0.0)
        assert abs(J[b, 3] / j4 - 1.0) <= 1e-13
        assert J[b, 4] == J[b, 0] + J[b, 1] + J[b, 2] + J[b, 3]


# ---- 4. the resident loop in a mixed batch ------------------------------------------------------------------------------------
MODES, BOX = K.MODES, K.BOX
# Picked on the CPU with the restatement's loop over the oracle: under b3 = 2 trajectory 0's first trials 2, 1.6, 1.28, 1.024
# and 0.8192 ascend (the step overshoots the quadratic b3 / 2 int u^2) and 0.65536 descends; the others descend at once.
B3 = (2.0, 1e-4, 1e-4, 1e-4)
ALPHA0 = (2.0, 30.0, 8.0, 5.0)
ALPHA_MAX = (50.0, 100.0, 8.0, 2.0)                                     # trajectory 3's first step is its cap


def _opts(O2, ks):
    return [O2.OptParams(b3=B3[b], kappa_sparsity=ks[b], alpha_max=ALPHA_MAX[b], u_min=BOX[b][0], u_max=BOX[b][1]) for b in range(4)]


@pytest.fixture(scope="module")
def resident(V, O2, engines):
    """Everything one accepted step of the batch leaves behind, computed once: a first init gives the adjoint at u0, whose
    group norms place kappa_sparsity of the group-mode trajectories; the second init is the problem under test: KKT statistic
    at u0, one iteration, a KKT look that must not disturb the loop, one more iteration; the same in a run without the look;
    every member alone in a batch-1 context; the cost through the seam on a context of its own."""
    Nx, Ny = K.RES_SHAPE
    P, phi0, phi_T, t, x, y, u0 = K.resident_problem(O2)
    eng = engines(Nx, Ny, 4, K.STEPS)
    mk = lambda ks: [V.make_opt(o) for o in _opts(O2, ks)]
    eng.pgd_init(phi0, phi_T, t, mk([1e-3] * 4), T=P.T, u0=u0, alpha0=ALPHA0, sparsity=MODES)
    eng.pgd_kkt(refresh=True)
    r_first = eng.pgd_get("r")
    ks = [1e-4 if m == "full" else K.kappa_between(G.group_norms(r_first[b], x, y, t, m).ravel(), 0.5) for b, m in enumerate(MODES)]
    d = dict(P=P, x=x, y=y, t=t, phi0=phi0, phi_T=phi_T, u0=u0, ks=ks, opts=_opts(O2, ks), r_first=r_first)
    d["J0"] = eng.pgd_init(phi0, phi_T, t, mk(ks), T=P.T, u0=u0, alpha0=ALPHA0, sparsity=MODES)
    d["kkt"] = eng.pgd_kkt(refresh=True)
    d["r_kkt"] = eng.pgd_get("r")
    d["res"] = eng.pgd_iterate(1)
    d["r"], d["u"], d["phi"], d["phi_Q"] = (eng.pgd_get(k) for k in ("r", "u", "phi", "phi_Q"))
    d["kkt_norefresh"] = eng.pgd_kkt(refresh=False)
    d["res2"] = eng.pgd_iterate(1)
    d["u2"] = eng.pgd_get("u")
    eng.pgd_init(phi0, phi_T, t, mk(ks), T=P.T, u0=u0, alpha0=ALPHA0, sparsity=MODES)
    d["plain"] = (eng.pgd_iterate(2), eng.pgd_get("u"))
    e1 = engines(Nx, Ny, 1, K.STEPS)
    d["single"] = []
    for b in range(4):
        J1 = e1.pgd_init(phi0[b], phi_T[b], t, [mk(ks)[b]], T=P.T, u0=u0[b], alpha0=ALPHA0[b], sparsity=MODES[b])
        d["single"].append((J1, e1.pgd_iterate(1), e1.pgd_get("u"), e1.pgd_get("phi")))
    d["Jc"] = np.stack([eng.cost(d["phi"], d["u"], d["phi_Q"], phi_T, t, mk(ks)[b], x=x, y=y, sparsity=MODES[b])[b] for b in range(4)])
    return d


def test_resident_step_against_the_restatement(resident):
    """One accepted step of every group-mode trajectory from the warm start: u+ to 1e-12 max|v| of the restatement's prox of
    the pulled adjoint at the accepted step size, `change` to 1e-12 relative, J4 at u0 and of the accepted iterate to 1e-13
    and the loop's cost equal to the seam's to 1e-13 (the 1D file's tolerances).  Trajectory 0 backtracks."""
    d = resident
    x, y, t, u0, r, res = d["x"], d["y"], d["t"], d["u0"], d["r"], d["res"]
    # the adjoint at u0 each time; the loop's sweep stops at a relative residual of 1e-12, the refresh of pgd_kkt at 1e-15
    assert np.array_equal(d["r_first"], d["r_kkt"]) and relerr(d["r"], d["r_kkt"]) < 1e-8
    assert res["iters"] == 1
    att = [int(res["attempts"][b, 0]) for b in range(4)]
    assert att[0] >= 1 and att[1:] == [0, 0, 0], att
    for b, mode in enumerate(MODES):
        if mode == "full":
            continue
        o = d["opts"][b]
        assert res["cost"][b, 0] < d["J0"][b, 4] and att[b] < 10                 # a descent: alpha is the step u+ was made with
        al = min(ALPHA0[b], ALPHA_MAX[b])
        if att[b]:
            al *= 0.8
            for _ in range(att[b] - 1):
                al *= 0.8
        assert res["alpha"][b, 0] == al, (b, res["alpha"][b, 0], al)
        ur, sr, kinds = G.prox(u0[b], r[b], al, o.b3, o.kappa_sparsity, o.u_min, o.u_max, mode, x, y, t)
        v = u0[b] - al * (r[b] + o.b3 * u0[b])
        print(f"b {b} {mode}: attempts {att[b]} alpha {al:g} kinds { {k: kinds.count(k) for k in sorted(set(kinds))} } "
              f"u+ err {np.max(np.abs(d['u'][b] - ur)) / np.max(np.abs(v)):.2e}")
        assert np.max(np.abs(d["u"][b] - ur)) <= 1e-12 * np.max(np.abs(v)), b
        chg = np.linalg.norm(ur - u0[b]) / (np.linalg.norm(u0[b]) + 1e-9)
        assert abs(res["change"][b, 0] / chg - 1.0) <= 1e-12, (b, res["change"][b, 0], chg)
        assert abs(d["J0"][b, 3] / G.j4(u0[b], x, y, t, o.kappa_sparsity, mode) - 1.0) <= 1e-13, b
        assert abs(d["Jc"][b, 3] / G.j4(d["u"][b], x, y, t, o.kappa_sparsity, mode) - 1.0) <= 1e-13, b
        assert abs(res["cost"][b, 0] / d["Jc"][b, 4] - 1.0) <= 1e-13, b


def test_resident_members_keep_the_bits_of_a_batch_of_their_own(resident):
    d = resident
    for b in range(4):
        J1, r1, u1, p1 = d["single"][b]
        assert np.array_equal(d["J0"][b], J1[0]), b
        for key in ("cost", "alpha", "attempts", "change"):
            assert np.array_equal(d["res"][key][b], r1[key][0]), (b, key)
        assert np.array_equal(d["u"][b], u1) and np.array_equal(d["phi"][b], p1), b


def test_resident_kkt_by_groups(resident):
    """pgd_kkt(refresh=True) at u0: the four counts exactly and the stationarity to 1e-10 of the restatement on u0 and the
    pulled adjoint.  kappa_sparsity lies between two adjacent group norms of the adjoint and u0's groups are exactly zero or
    far above the tolerance 1e-6, so no decision is within 1e-9 of its threshold.  A look with refresh=False between two
    iterations leaves their bits alone."""
    d = resident
    x, y, t, u0, r, k = d["x"], d["y"], d["t"], d["u0"], d["r_kkt"], d["kkt"]
    for b, mode in enumerate(MODES):
        if mode == "full":
            assert k["total"][b] == u0[b].size
            continue
        o = d["opts"][b]
        gr, gu = G.group_norms(r[b], x, y, t, mode).ravel(), G.group_norms(u0[b], x, y, t, mode).ravel()
        assert np.min(np.abs(gr / o.kappa_sparsity - 1.0)) >= 1e-9 and np.min(np.abs(gu / 1e-6 - 1.0)) >= 1e-9
        cnt, stat = G.kkt(u0[b], r[b], x, y, t, o.b3, o.kappa_sparsity, o.u_min, o.u_max, mode)
        got = [k["n_zero"][b], k["n_small"][b], k["n_match"][b], k["total"][b]]
        print(f"b {b} {mode}: counts {got} stationarity {k['stationarity'][b]:.6e} (restatement {stat:.6e})")
        assert got == list(cnt), (mode, got, cnt)
        assert cnt[3] == (t.size if mode == "time" else u0[b][0].size) and 0 < cnt[0] < cnt[3] and 0 < cnt[1] < cnt[3]
        assert abs(k["stationarity"][b] - stat) <= 1e-10 * max(stat, 1.0), (b, k["stationarity"][b], stat)
    plain, u_plain = d["plain"]
    for key in ("cost", "alpha", "attempts", "change"):
        assert np.array_equal(np.c_[d["res"][key], d["res2"][key]], plain[key]), key
    assert np.array_equal(d["u2"], u_plain)
    assert d["kkt_norefresh"]["total"][0] == u0[0][0].size and d["kkt_norefresh"]["total"][2] == t.size


# ---- 5. three iterations against the oracle loop ---------------------------------------------------------------------------------
LOOP_BOX = {"time": (-0.001, 0.002), "space": (-0.004, 0.006)}
# Engine and oracle agree on the adjoint of this problem to R_AGREE (max |r_engine - r_oracle| of the loop's sweep at u = 0,
# measured: profiles/dirsparse_2d_edges.txt); u+ = prox(u - alpha r) carries alpha times that, three steps with alpha <= 10
# carry at most 30 times that, and the margin is 10.  Measured: 1.03e-12 (max|r| = 2.97e-2), and |u - u_ref| = 3.8e-14 (time),
# 7.4e-12 (space) after the three iterations.
R_AGREE = 1.1e-12
U_TOL = 10.0 * 30.0 * R_AGREE


@pytest.mark.parametrize("mode", ["time", "space"])
def test_three_iterations_against_the_oracle_loop(V, O2, engines, mode):
    N = 16
    P, phi0, phi_T, t, x = _small_problem(V, O2, batch=1)
    eng = engines(N, N, 1, 6)
    # the adjoint at u = 0 as the loop takes it (its sweep stops at a relative residual of 1e-12; it does not depend on the mode)
    eng.pgd_init(phi0, phi_T, t, V.make_opt(O2.OptParams()), T=P.T)
    eng.pgd_iterate(1)
    r0 = eng.pgd_get("r")
    phi_o = O2.forward(P, control=None, phi0=phi0[0])[0]
    pT, pQ = O2.build_targets(x, x, t, phi0[0], 1.0, 1.0, P.T, 1, 1)
    r_o = O2.backward(phi_o, x, x, t, P, 5.0, 10.0, pQ, pT)[2]
    agree = float(np.max(np.abs(r0 - r_o)))
    ks = K.kappa_between(G.group_norms(r_o, x, x, t, mode).ravel(), 0.5)
    lo, hi = LOOP_BOX[mode]
    O = O2.OptParams(kappa_sparsity=ks, u_min=lo, u_max=hi, alpha_max=10.0)
    ref = G.pgd(O2, P, O, mode, 3, phi0=phi0[0], alpha0=8.0)
    assert max(ref["alphas"]) <= 10.0
    J0 = eng.pgd_init(phi0, phi_T, t, [V.make_opt(O)], T=P.T, alpha0=8.0, sparsity=mode)
    res = eng.pgd_iterate(3)
    u = eng.pgd_get("u")
    err = float(np.max(np.abs(u - ref["u"])))
    print(f"{mode}: adjoint agreement {agree:.2e} (max|r| {np.max(np.abs(r_o)):.2e})  |u - u_ref| {err:.2e} (tolerance {U_TOL:.1e}, "
          f"max|u| {np.max(np.abs(ref['u'])):.2e})  attempts {list(res['attempts'][0])} / {ref['attempts']}  costs {list(res['cost'][0])}")
    assert list(res["attempts"][0]) == ref["attempts"]
    assert np.allclose(np.r_[J0[0, 4], res["cost"][0]], ref["costs"], rtol=1e-9, atol=0.0)
    assert np.allclose(res["alpha"][0], ref["alphas"], rtol=1e-15, atol=0.0)
    assert err <= U_TOL
    assert np.allclose(res["change"][0][1:], ref["change"][1:], rtol=1e-6, atol=0.0)


# ---- 7. the refusals -------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_problem_usable(V, O2, engines):
    N, B = 16, 2
    P, phi0, phi_T, t, x = _small_problem(V, O2)
    lib_mod = V.module("_lib")
    VchError = lib_mod.VchError
    opts = [V.make_opt(O2.OptParams(kappa_sparsity=2e-3, u_min=-0.004, u_max=0.006, alpha_max=10.0)),
            V.make_opt(O2.OptParams(kappa_sparsity=1e-2, u_min=-0.001, u_max=0.002, alpha_max=10.0))]
    modes = ["space", "time"]
    eng = engines(N, N, B, 8)
    eng.pgd_init(phi0, phi_T, t, opts, T=P.T, sparsity=modes)
    plain = eng.pgd_iterate(2)
    u_plain = eng.pgd_get("u")
    eng.pgd_init(phi0, phi_T, t, opts, T=P.T, sparsity=modes)
    first = eng.pgd_iterate(1)
    for call in (lambda: eng.pgd_newton(2), lambda: eng.pgd_trust(2, 1.0), lambda: eng.hess_cg(3),
                 lambda: eng.hess_cg_trust(3, 1.0), lambda: eng.newton_trial(1.0)):
        with pytest.raises(VchError, match="engine error -3"):
            call()
    # VCH_ERR_ARG: NULL sparsity, n_sparsity not 1 or B, a mode outside 0..2, a group mode whose box does not hold 0
    arr = (type(opts[0]) * B)(*opts)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    init_g = lambda sp, n: lib_mod.check(eng.lib.vch2d_pgd_init_g(eng.ctx, _dp(phi0), _dp(phi_T), None, 1, P.T, _dp(t), t.size - 1,
                                                                  _dp(x), _dp(x), arr, B, None, None, sp, n, None))
    good = np.array([2, 1, 0], dtype=np.int32)
    with pytest.raises(ValueError, match="sparsity"):
        init_g(None, B)
    with pytest.raises(ValueError, match="n_sparsity"):
        init_g(i32(good), 3)
    with pytest.raises(ValueError, match="sparsity 3"):
        init_g(i32(np.array([1, 3], dtype=np.int32)), B)
    with pytest.raises(ValueError, match="box"):
        eng.pgd_init(phi0, phi_T, t, [V.make_opt(u_min=0.1, u_max=1.0)] * B, T=P.T, sparsity="time")
    with pytest.raises(ValueError, match="box"):
        eng.grad_prox(np.zeros((B, 4, N + 1, N + 1)), np.zeros((B, 4, N + 1, N + 1)), 1.0, V.make_opt(u_min=-1.0, u_max=-0.1),
                      sparsity="space", t_hist=np.arange(4.0))
    second = eng.pgd_iterate(1)
    for key in ("cost", "alpha", "attempts", "change"):
        assert np.array_equal(first[key][:, 0], plain[key][:, 0]), key
        assert np.array_equal(second[key][:, 0], plain[key][:, 1]), key
    assert np.array_equal(eng.pgd_get("u"), u_plain)
    # the smooth part's calls keep working in a group mode
    h = np.ones((B, t.size, N + 1, N + 1))
    so = eng.second_order(h)
    hv = eng.hessvec(h)
    assert np.all(np.isfinite(so["curvature"])) and isinstance(hv, dict)
    out = eng.hess_cg(2, rhs=h, mask=np.ones(h.shape, dtype=bool))
    assert np.all(out["steps"] >= 1)
    # after a plain init the Newton rounds run again
    eng.pgd_init(phi0, phi_T, t, [V.make_opt(O2.OptParams()), V.make_opt(O2.OptParams())], T=P.T)
    eng.pgd_iterate(1)
    R = eng.pgd_newton(1)
    assert R["rounds"] == 1 and np.all(np.isfinite(R["cost"][:, 0]))
