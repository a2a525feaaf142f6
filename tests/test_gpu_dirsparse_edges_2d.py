"""Directional sparsity in the 2D engine where tests/test_gpu_dirsparse_2d.py does not look.

A. The prox seam at its three decisions (alive or zero, closed form or iteration, the end of the iteration) with the 1D edge
   tests' builders on planes and pencils: |c / lam - 1| and the vote margin down to 1e-9, rho / lam up to 1e9, lam = 0,
   weightless lines of x or y nodes (time) and weightless levels (space), a step per trajectory; grids (16, 16), (70, 20),
   (130, 40) with 3, 16, 17 and 33 levels.  The inputs are tests/_dirsparse_2d_edge_cases.py; that they keep MARGIN from
   every threshold is checked without a GPU in tests/test_dirsparse_edges_2d_cpu.py.
B. The resident loop past what has run: 17 levels in a context built for 41 with full runs at both ends of the batch and a
   time member that backtracks (B1); 33 levels on a column of tiles (B2); members whose groups are all dead, through the
   "return last try" exit, the plateau boost and the stop rule while the others go on (B3).
C. cost(..., u=None) of the group modes.
D. Call order: seam calls with other grids before a group-mode init, a plain init after it.
Measured floors, counts and run times are in profiles/dirsparse_2d_edges.txt."""
import numpy as np
import pytest

import _dirsparse_2d_cases as K
import _dirsparse_2d_edge_cases as X
import _group_prox_ref_2d as G

pytestmark = pytest.mark.gpu

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

    def get(Nx, Ny, batch=X.BATCH, max_steps=MAXSTEPS):
        key = (Nx, Ny, batch, max_steps)
        if key not in made:
            made[key] = V.Engine2D(Nx=Nx, Ny=Ny, batch=batch, max_steps=max_steps)
        return made[key]
    yield get
    for e in made.values():
        e.close()


# ---- A. the prox seam at its decisions ------------------------------------------------------------------------------------
FLOORS = {}                          # regime -> [the restatement's |s_double - s_long double|, |s_gpu - s_ref|], the largest seen
SEAM = pytest.mark.parametrize("mode,shape", [(m, s) for m in X.MODES for s in X.SHAPES], ids=lambda v: str(v).replace(" ", ""))


def _seam(V, eng, regime, param, mode, shape):
    """Every row count and box of one (regime, mode, shape) through grad_prox against the restatement, with the assertions of
    the 1D _seam: s == 0 exactly where the restatement says zero and s > 0 elsewhere; closed-form groups have the bits of
    s v and box-active ones an entry the box holds (the kinds are the restatement's); s to 1e-12 absolute, u+ to 1e-12
    max|v|.  In the edge regime a box-active group whose root lies 64 ulps or more below the closed form s0 must have moved
    at least half of that way: at a vote margin of 1e-9 the two differ by less than the 1e-12 asked of s (7e-14 on the
    planes of (130, 40)), so a wrong vote would pass everything else.  The long-double restatement gives the recorded floor.
    -> the kinds seen."""
    seen, n_far = set(), 0
    fl = FLOORS.setdefault(regime if param is None else f"{regime} {param:g}", [0.0, 0.0])
    for rows, lo, hi, case in X.all_cases(regime, param, mode, shape):
        opt = V.make_opt(b3=0.0, kappa_sparsity=case["ks"], u_min=lo, u_max=hi)
        up, s = eng.grad_prox(case["u"], case["r"], case["alpha"], opt, sparsity=mode, x=case["x"], y=case["y"], t_hist=case["t"],
                              return_scale=True)
        for b in range(X.BATCH):
            tag = (regime, param, mode, shape, rows, lo, hi, b)
            va = X.formed_v(case, b)
            alive, vote = X.margins(case, b)
            assert np.min(np.abs(alive)) >= X.MARGIN and (vote.size == 0 or np.min(np.abs(vote)) >= X.MARGIN), tag
            ur, sr, kr = X.restate(case, b)
            kr = np.array(kr)
            assert np.array_equal(kr != "zero", alive > 0.0), tag
            if vote.size:
                assert np.array_equal(kr[kr != "zero"] == "box", vote > 0.0), tag
            seen |= set(kr)
            sl = X.restate(case, b, dtype=X.LD)[1]
            fl[0] = max(fl[0], float(np.max(np.abs(sr - sl))))
            fl[1] = max(fl[1], float(np.max(np.abs(s[b] - sr))))
            sg = s[b].ravel()
            assert np.array_equal(sg == 0.0, kr == "zero") and np.all(sg >= 0.0), tag
            sv = (s[b][:, None, None] if mode == "time" else s[b][None]) * va
            same = np.all(G.groups(up[b], mode) == G.groups(sv, mode), axis=1)
            assert np.array_equal(same[kr != "zero"], (kr == "closed")[kr != "zero"]), tag
            assert not G.groups(up[b], mode)[kr == "zero"].any(), tag
            assert np.max(np.abs(s[b] - sr)) <= 1e-12, tag
            assert np.max(np.abs(up[b] - ur)) <= 1e-12 * max(np.max(np.abs(va)), 1e-300), tag
            if regime == "edge":                  # a box-active group has left the closed form: at least half way to the root
                s0 = X.closed_form_ld(case, b)
                far = (kr == "box") & (s0 - sl.ravel() >= X.MOVED)
                assert np.all((s0 - sg)[far] >= 0.5 * (s0 - sl.ravel())[far]), tag
                n_far += int(far.sum())
            if regime == "lam0":
                assert sg[0] == 0.0 and np.all(sg[1:] == 1.0), tag
                assert np.array_equal(up[b], np.clip(va, lo, hi)), tag
    assert n_far >= 8 or regime != "edge"
    print(f"EDGE2D seam {regime} {param} {mode} {shape}: restatement's floor {fl[0]:.2e}, gpu {fl[1]:.2e} (largest so far), "
          f"kinds {sorted(str(k) for k in seen)}")
    return seen


@SEAM
def test_seam_barely_alive_and_barely_dead(V, engines, mode, shape):
    """c / lam - 1 = +-1e-9, +-1e-6, +-1e-3 on every box, the sums in the kernels' own orders (tile partials folded by one
    thread; sixteen wavefront partials through LDS)."""
    assert _seam(V, engines(*shape), "alive", None, mode, shape) == X.KINDS["alive"]


@SEAM
def test_seam_barely_closed_and_barely_box(V, engines, mode, shape):
    """max|s0 v| at (1 -+ 1e-9) and (1 -+ 1e-6) of a bound, the four finite boxes."""
    assert _seam(V, engines(*shape), "edge", None, mode, shape) == X.KINDS["edge"]


@SEAM
@pytest.mark.parametrize("ratio", X.RATIOS)
def test_seam_at_large_rho_over_lam(V, engines, mode, shape, ratio):
    """lam = alpha 0.5 / ratio against groups of amplitude 3 (box-active) and 0.05 (closed form, s0 = 1 - O(1 / ratio))."""
    assert X.KINDS["ratio"] <= _seam(V, engines(*shape), "ratio", ratio, mode, shape)


@SEAM
def test_seam_at_lam_zero_is_the_projection(V, engines, mode, shape):
    """kappa_s = 0: s == 1.0 on every group but the all-zero one, u+ == clip(v) bit for bit."""
    _seam(V, engines(*shape), "lam0", None, mode, shape)


@pytest.mark.parametrize("shape", X.SHAPES, ids=str)
@pytest.mark.parametrize("regime", ["zero_x", "zero_y", "zero_t"])
def test_seam_on_nodes_and_levels_of_zero_weight(V, engines, regime, shape):
    """Time: an x node three times, and on its own a y node three times (a line of nodes with W = 0); space: t[0] == t[1] and
    an interior level three times (wt has exact zeros, which the pencil kernels read).  Entries of 50 stand on the weightless
    nodes or levels: a group whose weighted rest is below lam vanishes, entry of 50 included; in the others that entry is
    scaled and clipped like the rest."""
    mode = "space" if regime == "zero_t" else "time"
    assert _seam(V, engines(*shape), regime, None, mode, shape) == X.KINDS[regime]


# ---- B. the resident loop ----------------------------------------------------------------------------------------------------
OUT_KEYS = ("cost", "alpha", "attempts", "change")


def _opts(O2, spec, ks):
    return [O2.OptParams(b3=spec["b3"][b], kappa_sparsity=ks[b], alpha_max=spec["alpha_max"][b], u_min=spec["box"][b][0],
                         u_max=spec["box"][b][1]) for b in range(len(spec["modes"]))]


def _resident(V, O2, engines, spec):
    """Everything one accepted step of the batch leaves behind, computed once: a first init gives the adjoint at u0, whose
    group norms place kappa_sparsity of the group members; the second init is the problem under test: KKT statistic at u0,
    one iteration; the cost of the accepted iterate through the seam; every member alone in a batch-1 context of exact
    size."""
    (Nx, Ny), modes = spec["shape"], spec["modes"]
    B = len(modes)
    P, phi0, phi_T, t, x, y, u0 = K.resident_problem(O2, Nx, Ny, spec["steps"], B)
    eng = engines(Nx, Ny, B, spec["max_steps"])
    mk = lambda ks: [V.make_opt(o) for o in _opts(O2, spec, ks)]
    a0 = spec["alpha0"]
    eng.pgd_init(phi0, phi_T, t, mk([1e-3] * B), T=P.T, u0=u0, alpha0=a0, sparsity=modes)
    eng.pgd_kkt(refresh=True)
    r_first = eng.pgd_get("r")
    ks = [1e-4 if m == "full" else K.kappa_between(G.group_norms(r_first[b], x, y, t, m).ravel(), 0.5) for b, m in enumerate(modes)]
    d = dict(spec=spec, x=x, y=y, t=t, u0=u0, ks=ks, opts=_opts(O2, spec, ks), r_first=r_first)
    d["J0"] = eng.pgd_init(phi0, phi_T, t, mk(ks), T=P.T, u0=u0, alpha0=a0, sparsity=modes)
    d["kkt"] = eng.pgd_kkt(refresh=True)
    d["r_kkt"] = eng.pgd_get("r")
    # a second look with the zero threshold between two adjacent pencil norms of the space member's u0: at the default 1e-6
    # the pencils of u0 are exactly zero or far above it, and n_zero cannot see which levels the kernel's norm of u covers
    sp = modes.index("space")
    d["tol"] = K.kappa_between(G.group_norms(u0[sp], x, y, t, "space").ravel(), 0.5)
    d["kkt_tol"] = eng.pgd_kkt(refresh=False, tol=d["tol"])
    d["res"] = eng.pgd_iterate(1)
    d["r"], d["u"], d["phi"], phi_Q = (eng.pgd_get(k) for k in ("r", "u", "phi", "phi_Q"))
    d["Jc"] = np.stack([eng.cost(d["phi"], d["u"], phi_Q, phi_T, t, mk(ks)[b], x=x, y=y, sparsity=modes[b])[b] for b in range(B)])
    e1 = engines(Nx, Ny, 1, spec["steps"])
    d["single"] = []
    for b in range(B):
        J1 = e1.pgd_init(phi0[b], phi_T[b], t, [mk(ks)[b]], T=P.T, u0=u0[b], alpha0=a0[b], sparsity=modes[b])
        d["single"].append((J1, e1.pgd_iterate(1), e1.pgd_get("u"), e1.pgd_get("phi")))
    return d


@pytest.fixture(scope="module")
def b1(V, O2, engines):
    return _resident(V, O2, engines, X.B1)


@pytest.fixture(scope="module")
def b2(V, O2, engines):
    return _resident(V, O2, engines, X.B2)


def _step_against_the_restatement(d, name):
    spec, x, y, t, u0, r, res = d["spec"], d["x"], d["y"], d["t"], d["u0"], d["r"], d["res"]
    modes = spec["modes"]
    assert np.array_equal(d["r_first"], d["r_kkt"]) and res["iters"] == 1
    att = [int(a) for a in res["attempts"][:, 0]]
    print(f"EDGE2D {name} attempts {att} alpha {[float(a) for a in res['alpha'][:, 0]]}")
    for b, mode in enumerate(modes):
        al = min(spec["alpha0"][b], spec["alpha_max"][b])
        for _ in range(att[b]):
            al *= 0.8
        if b == spec["overshoot"]:
            assert att[b] >= 1, att                                              # the overshoot under b3 = 2 backtracks
        if mode == "full":
            continue
        o = d["opts"][b]
        assert res["cost"][b, 0] < d["J0"][b, 4] and att[b] < 10                 # a descent: alpha is the step u+ was made with
        assert res["alpha"][b, 0] == al, (b, res["alpha"][b, 0], al)
        ur, sr, kinds = G.prox(u0[b], r[b], al, o.b3, o.kappa_sparsity, o.u_min, o.u_max, mode, x, y, t)
        v = u0[b] - al * (r[b] + o.b3 * u0[b])
        print(f"EDGE2D {name} b {b} {mode}: attempts {att[b]} alpha {al:g} kinds { {k: kinds.count(k) for k in sorted(set(kinds))} } "
              f"u+ err {np.max(np.abs(d['u'][b] - ur)) / np.max(np.abs(v)):.2e}")
        assert np.max(np.abs(d["u"][b] - ur)) <= 1e-12 * np.max(np.abs(v)), b
        chg = np.linalg.norm(ur - u0[b]) / (np.linalg.norm(u0[b]) + 1e-9)
        assert abs(res["change"][b, 0] / chg - 1.0) <= 1e-12, (b, res["change"][b, 0], chg)
        assert abs(d["J0"][b, 3] / G.j4(u0[b], x, y, t, o.kappa_sparsity, mode) - 1.0) <= 1e-13, b
        assert abs(d["Jc"][b, 3] / G.j4(d["u"][b], x, y, t, o.kappa_sparsity, mode) - 1.0) <= 1e-13, b
        assert abs(res["cost"][b, 0] / d["Jc"][b, 4] - 1.0) <= 1e-13, b


def _members_keep_their_bits(d):
    for b in range(len(d["spec"]["modes"])):
        J1, r1, u1, p1 = d["single"][b]
        assert np.array_equal(d["J0"][b], J1[0]), b
        for key in OUT_KEYS:
            assert np.array_equal(d["res"][key][b], r1[key][0]), (b, key)
        assert np.array_equal(d["u"][b], u1) and np.array_equal(d["phi"][b], p1), b


def _kkt_by_groups(d, name):
    x, y, t, u0, r, k = d["x"], d["y"], d["t"], d["u0"], d["r_kkt"], d["kkt"]
    k2, tol = d["kkt_tol"], d["tol"]
    for b, mode in enumerate(d["spec"]["modes"]):
        if mode != "full":                        # the look at the threshold `tol`: counts alone (the stationarity does not read it)
            gu = G.group_norms(u0[b], x, y, t, mode).ravel()
            assert np.min(np.abs(gu[gu > 0.0] / tol - 1.0)) >= 1e-9
            cnt = G.kkt(u0[b], r[b], x, y, t, d["opts"][b].b3, d["opts"][b].kappa_sparsity, d["opts"][b].u_min, d["opts"][b].u_max, mode, tol=tol)[0]
            got = [k2["n_zero"][b], k2["n_small"][b], k2["n_match"][b], k2["total"][b]]
            print(f"EDGE2D {name} kkt at tol {tol:.3e} b {b} {mode}: counts {[int(g) for g in got]}")
            assert got == list(cnt), (mode, got, cnt)
            assert mode != "space" or k["n_zero"][b] + 100 < cnt[0] < cnt[3] - 100
            assert k2["stationarity"][b] == k["stationarity"][b]
        if mode == "full":
            assert k["total"][b] == u0[b].size
            continue
        o = d["opts"][b]
        gr, gu = G.group_norms(r[b], x, y, t, mode).ravel(), G.group_norms(u0[b], x, y, t, mode).ravel()
        assert np.min(np.abs(gr / o.kappa_sparsity - 1.0)) >= 1e-9 and np.min(np.abs(gu / 1e-6 - 1.0)) >= 1e-9
        cnt, stat = G.kkt(u0[b], r[b], x, y, t, o.b3, o.kappa_sparsity, o.u_min, o.u_max, mode)
        got = [k["n_zero"][b], k["n_small"][b], k["n_match"][b], k["total"][b]]
        print(f"EDGE2D {name} kkt b {b} {mode}: counts {[int(g) for g in got]} stationarity {k['stationarity'][b]:.6e} (restatement {stat:.6e})")
        assert got == list(cnt), (mode, got, cnt)
        assert cnt[3] == (t.size if mode == "time" else u0[b][0].size) and 0 < cnt[0] < cnt[3] and 0 < cnt[1] < cnt[3]
        assert abs(k["stationarity"][b] - stat) <= 1e-10 * max(stat, 1.0), (b, k["stationarity"][b], stat)


def test_b1_step_against_the_restatement(b1):
    """(130, 40), 17 levels in a context built for 41 (hist_stride and the row count of the calls differ), batch [full, full,
    time, space, time, full]: the time member with b3 = 2, alpha0 = 2 backtracks (attempts >= 1, alpha = alpha0 0.8^attempts);
    one accepted step of every group member against the restatement on the pulled adjoint: u+ to 1e-12 max|v|, change to
    1e-12 relative, J4 before and after and the loop's cost against the seam's to 1e-13."""
    _step_against_the_restatement(b1, "B1")


def test_b1_members_keep_the_bits_of_a_batch_of_their_own(b1):
    """Every member, the three full ones (k_grad_prox launched on the run [0, 2) and on the run [5, 6) with pointer offsets)
    included, against a batch-1 context with max_steps = 16: J0, cost, alpha, attempts, change, u and phi bit for bit."""
    _members_keep_their_bits(b1)


def test_b1_kkt_by_groups_at_the_warm_start(b1):
    """pgd_kkt(refresh=True) at u0: the four counts exactly, stationarity to 1e-10 max(stat, 1); the space member's counts
    take a second trip of k_gp_kkt_space's level loop (17 levels, 16 wavefronts).  Level 16 alone decides nothing at the
    default tol = 1e-6 (u0's pencils are exactly zero or far above it, and the adjoint vanishes at the last level), so a
    second look takes tol between two adjacent pencil norms of u0: n_zero then depends on every level of the norm."""
    _kkt_by_groups(b1, "B1")


def test_b2_step_against_the_restatement(b2):
    """(20, 70), 33 levels (a third trip of the pencil loops), batch [time, space, full] in a context of exact size."""
    _step_against_the_restatement(b2, "B2")


def test_b2_members_keep_the_bits_of_a_batch_of_their_own(b2):
    _members_keep_their_bits(b2)


def test_b2_kkt_by_groups_at_the_warm_start(b2):
    _kkt_by_groups(b2, "B2")


@pytest.fixture(scope="module")
def b3(V, O2, engines):
    """(16, 16), 4 levels, [time, space, full, time] from u = 0, 24 iterations in one call.  Members 0 and 1 carry kappa_s ten
    times the largest group norm of the adjoint at u = 0: v = -alpha r has ||v_g|| = alpha ||r_g|| < alpha kappa_s = lam
    whatever the step, so every group is dead at every trial."""
    spec = X.B3
    (Nx, Ny), modes = spec["shape"], spec["modes"]
    P, phi0, phi_T, t, x, y = X.cold_problem(O2, Nx, Ny, spec["steps"], 4)
    eng = engines(Nx, Ny, 4, spec["max_steps"])
    opts = lambda ks: [O2.OptParams(kappa_sparsity=ks[b], alpha_max=spec["alpha_max"][b], u_min=spec["box"][b][0],
                                    u_max=spec["box"][b][1]) for b in range(4)]
    mk = lambda ks: [V.make_opt(o) for o in opts(ks)]
    eng.pgd_init(phi0, phi_T, t, mk([1e-3] * 4), T=P.T, sparsity=modes)
    eng.pgd_kkt(refresh=True)
    r0 = eng.pgd_get("r")
    norms = [None if m == "full" else G.group_norms(r0[b], x, y, t, m).ravel() for b, m in enumerate(modes)]
    ks = [10.0 * float(norms[0].max()), 10.0 * float(norms[1].max()), 3e-4, K.kappa_between(norms[3], 0.5)]
    d = dict(spec=spec, ks=ks, t=t, nodes=(Nx + 1) * (Ny + 1))
    d["J0"] = eng.pgd_init(phi0, phi_T, t, mk(ks), T=P.T, sparsity=modes)
    d["res"] = eng.pgd_iterate(spec["iters"])
    d["u"], d["phi"] = eng.pgd_get("u"), eng.pgd_get("phi")
    d["kkt"] = eng.pgd_kkt(refresh=True)
    e1 = engines(Nx, Ny, 1, spec["max_steps"])
    d["single"] = {}
    for b in (2, 3):
        J1 = e1.pgd_init(phi0[b], phi_T[b], t, [mk(ks)[b]], T=P.T, sparsity=modes[b])
        d["single"][b] = (J1, e1.pgd_iterate(spec["iters"]), e1.pgd_get("u"), e1.pgd_get("phi"))
    return d


@pytest.mark.parametrize("b", [0, 1])
def test_b3_dead_members_return_the_last_try_and_stop(b3, b):
    """A member all of whose groups are dead: u stays exactly 0, the cost keeps the bits of J0, no trial descends, so every
    iteration takes the "return last try" exit (attempts == 10, change == 0.0) and alpha follows a replay of vch_pgd.h's 2D
    rule (reduced once more, growth 1.2, plateau boost 1.5 after five equal costs); it stops in the first iteration with
    k > 20 while members 2 and 3 go on; after it the five doubles are NaN and attempts 0.  KKT at the end state: every
    group is zero, small and in agreement, stationarity exactly 0."""
    spec, res = b3["spec"], b3["res"]
    alphas, stop = X.replay_dead(spec["alpha_max"][b], spec["iters"])
    n = stop + 1
    print(f"EDGE2D B3 b {b} {spec['modes'][b]}: kappa_s {b3['ks'][b]:.3e} stops in iteration {stop} (0-based), alpha {res['alpha'][b, 0]:.6e} .. "
          f"{res['alpha'][b, stop]:.6e}")
    assert res["iters"] == spec["iters"] and stop == 21
    assert not b3["u"][b].any()
    assert np.all(res["cost"][b, :n] == b3["J0"][b, 4]) and np.all(res["attempts"][b, :n] == 10) and np.all(res["change"][b, :n] == 0.0)
    assert np.array_equal(res["alpha"][b, :n], np.array(alphas)), (res["alpha"][b, :n], alphas)
    for key in ("cost", "alpha", "change", "tracking_error", "terminal_error"):
        assert np.isnan(res[key][b, n:]).all() and not np.isnan(res[key][b, :n]).any(), (key, res[key][b])
    assert np.all(res["attempts"][b, n:] == 0)
    k = b3["kkt"]
    ng = b3["t"].size if spec["modes"][b] == "time" else b3["nodes"]
    assert [k["n_zero"][b], k["n_small"][b], k["n_match"][b], k["total"][b]] == [ng] * 4
    assert k["stationarity"][b] == 0.0


@pytest.mark.parametrize("b", [2, 3])
def test_b3_live_members_run_on_with_the_bits_of_their_own_batch(b3, b):
    """Members 2 (full) and 3 (time) run all 24 iterations while members 0 and 1 stop, with the bits of their batch-1 runs."""
    res = b3["res"]
    J1, r1, u1, p1 = b3["single"][b]
    assert np.array_equal(b3["J0"][b], J1[0])
    for key in OUT_KEYS + ("tracking_error", "terminal_error"):
        assert not np.isnan(res[key][b]).any(), key
        assert np.array_equal(res[key][b], r1[key][0]), key
    assert np.array_equal(b3["u"][b], u1) and np.array_equal(b3["phi"][b], p1)
    assert np.all(res["change"][b] > 1e-5)                                   # the stop rule had nothing to act on here


# ---- C. the cost without a control ---------------------------------------------------------------------------------------------
def test_cost_without_a_control(V, engines):
    """cost(..., u=None, sparsity=mode) at (130, 40), 22 levels: J3 = J4 = 0 and J1, J2 have the bits of the full mode, with
    the pencil partials of an earlier call with a control still lying in the host buffer."""
    Nx, Ny, rows = 130, 40, 22
    eng = engines(Nx, Ny)
    rng = np.random.default_rng(11)
    x, y, t = K.grids(rng, Nx, Ny, rows)
    shp = (X.BATCH, rows, Nx + 1, Ny + 1)
    phi, pq = rng.standard_normal((2,) + shp)
    pt = rng.standard_normal((X.BATCH, Nx + 1, Ny + 1))
    opt = V.make_opt(b1=0.7, b2=3.0, b3=0.4, kappa_sparsity=0.25)
    full = eng.cost(phi, None, pq, pt, t, opt, x=x, y=y)
    assert np.all(full[:, 2:4] == 0.0) and np.all(full[:, :2] > 0.0)
    for mode in X.MODES:
        with_u = eng.cost(phi, rng.standard_normal(shp), pq, pt, t, opt, x=x, y=y, sparsity=mode)
        assert np.all(with_u[:, 2:4] > 0.0)
        J = eng.cost(phi, None, pq, pt, t, opt, x=x, y=y, sparsity=mode)
        assert np.all(J[:, 2:4] == 0.0) and np.array_equal(J, full), mode


# ---- D. call order ---------------------------------------------------------------------------------------------------------------
def test_init_after_seam_calls_with_other_grids(V, O2):
    """A "space" seam call with another t_hist and row count and a "time" seam call with other x, y overwrite gp_wt and
    W_cost; pgd_init(..., sparsity=[...]) restores both: two iterations have the bits of a fresh context's.  A plain
    pgd_init on the same context then has the bits of a context that never saw a group mode."""
    Nx, Ny = K.RES_SHAPE
    P, phi0, phi_T, t, x, y, u0 = K.resident_problem(O2, batch=2)
    modes, box = ["time", "space"], [(-0.05, 0.08), (-0.3, 2.0)]
    mk = lambda: [V.make_opt(O2.OptParams(kappa_sparsity=2e-3, alpha_max=8.0, u_min=lo, u_max=hi)) for lo, hi in box]

    def group_run(e):
        J0 = e.pgd_init(phi0, phi_T, t, mk(), T=P.T, u0=u0, alpha0=[8.0, 5.0], sparsity=modes)
        return J0, e.pgd_iterate(2), e.pgd_kkt(refresh=True), e.pgd_get("u"), e.pgd_get("phi")

    def plain_run(e):
        J0 = e.pgd_init(phi0, phi_T, t, mk(), T=P.T, u0=u0, alpha0=[8.0, 5.0])
        return J0, e.pgd_iterate(2), e.pgd_kkt(refresh=True), e.pgd_get("u"), e.pgd_get("phi")

    def same(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
        for key in OUT_KEYS + ("tracking_error", "terminal_error"):
            assert np.array_equal(a[1][key], b[1][key]), key
        for key in ("n_zero", "n_small", "n_match", "total", "stationarity"):
            assert np.array_equal(a[2][key], b[2][key]), key

    made = [V.Engine2D(Nx=Nx, Ny=Ny, batch=2, max_steps=12) for _ in range(3)]
    try:
        used, fresh, never = made
        for mode in ("space", "time"):
            c = X.edge_case("alive", mode, Nx, Ny, 11, -0.3, 2.0)
            up, s = used.grad_prox(c["u"], c["r"], c["alpha"], V.make_opt(b3=0.0, kappa_sparsity=c["ks"], u_min=-0.3, u_max=2.0),
                                   sparsity=mode, x=c["x"], y=c["y"], t_hist=c["t"], return_scale=True)
            assert np.any(s == 0.0) and np.any(s > 0.0)
        same(group_run(used), group_run(fresh))
        same(plain_run(used), plain_run(never))
    finally:
        for e in made:
            e.close()
