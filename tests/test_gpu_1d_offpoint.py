"""GPU tests of the 1D engine away from the default physics (Lx != 1, c2 != 1, other tau, gamma, c1, kappa), inside
decision margins.

Every other 1D test of the nonlinear path runs at Lx = 1 and the default tau, gamma, c1, c2, kappa, where a factor Lx
dropped from the mass shift, c2 used where c1 belongs or the run-time tau reaching the frozen adjoint are invisible.
Here the engine runs at OFF and OFF2 (tests/_offpoint_1d.py) against the CPU oracle and against the reference's own
vectors at these points (tests/golden/g1d_off_33.npz, g1d_off2_33.npz; the oracle is pinned to them by
test_oracle_golden_1d_off.py).  The Newton and line-search paths are compared step for step only on inputs that
test_offpoint_1d_windows.py holds inside their decision window on the CPU; the knife-edge trajectory (a node on the clip
value, decisions taken at distance 0.0) gets path-independent assertions only.

Tolerances (none taken from the engine's output): OPS 1e-12 and SOLVE 1e-9 of test_gpu_1d.py; free energy 1e-13 relative
(test_gpu_mirror.py); fields of a march max(1e-9, 20 eps cond_J), cond_J the Skeel condition of the first step's matrix
(test_gpu_1d_levels.py; cond_J <= 1.2e4 here, so 1e-9 everywhere); the adjoint sweep max(1e-9, 20 eps max_k cond_k).

Measured on the MI355X / asserted:
  a. OFF2 N = 33     lap 2.2e-16, Rphi 1.2e-17, Rmu 1.4e-16 / 1e-12;  jacobian_solve 3.9e-14, adjoint_solve 5.3e-13,
                     terminal 6.6e-15 / 1e-9;  free energy 7e-18 plain, 1.4e-17 with w, 1.2e-16 with eps / 1e-13
  b. march           fields vs oracle 5.6e-16 (OFF 33), 7.0e-16 (OFF 64), 7.1e-16 (OFF2 33), 8.1e-16 (OFF2 64) / 1e-9; vs
                     the reference's histories 6.3e-16, 7.5e-16 / 1e-9;  mass drift <= 7e-17 / 1e-12;  counts equal
  c. capped Newton   phi_new, mu_new 4.9e-15, 2.3e-15, 2.1e-14, 1.6e-14 / 1e-9;  one-step march 2.0e-15, 7.0e-16,
                     8.4e-15, 5.7e-16 / 1e-9 (default 33, OFF 33, OFF 64, OFF2 33);  norms 6, 7, 6, 5 as the oracle
  d. knife edge      trajectories 0, 2: 4.7e-16, 4.6e-16 / 1e-9;  trajectory 1: 3 of 5 loops converged (the oracle: 3),
                     max|phi| 0.99, mass drift 1.4e-17 / 1e-12
  d2. clipped start  fields vs oracle 6.7e-16 (N 33), 1.3e-15 (N 64) / 1e-9;  mass drift 5.6e-17 / 1e-12;  OFF: row 2 exact /
                     1e-14, mass drift 5.6e-17 / 1e-12.  With the shift divided by 1: fields 4.0e-4, mass drift 2.7e-4
  e. adjoint, OFF2   N = 33: p 6.7e-12, r 6.1e-12, the reference's sweep 5.9e-12 / 1e-9;  N = 64: p 4.5e-11, r 7.8e-11 /
                     1.3e-8 (20 eps cond, cond 2.9e6);  q = -L p: 0.29 eps / 4 eps;  cost 2.3e-16 / 1e-12;  prox 1.4e-16 /
                     1e-14;  OFF2 and default engines bit-identical
  f. PGD             alpha 0 / 1e-12;  costs 4.3e-15, 3.2e-14, 3.4e-14, 1.7e-13 / 1e-9;  u 1.1e-11, 7.4e-11, 2.0e-11,
                     1.6e-10 / 1e-8;  phi <= 6.0e-13, r <= 3.5e-11 / 1e-8;  phi_Q 8.0e-17 / 1e-15 (OFF 33, OFF 48, OFF2 33,
                     OFF2 48);  zero pattern equal at every node (no node within 1e-6 of the prox threshold, the
                     nearest 5.7e-6 away) / compared share >= 0.95
The window margins of every input are in test_offpoint_1d_windows.py.

Mutation check (scratch builds, not committed): with the mass shift of k1d_forward divided by 1.0 instead of P.Lx only
d2 fails (every other march has a round-off shift); with P.c1 for P.c2 in newton1's cphi b, c, d, d2 and f fail -- as do
the tests at the default point, where c1 = 0.75 and c2 = 1 differ as well.
"""
import functools

import numpy as np
import pytest

import _offpoint_1d as X
from conftest import golden, relerr
from oracle import vch1d_oracle as O1

pytestmark = pytest.mark.gpu
OPS, SOLVE = 1e-12, 1e-9
EPS = X.EPS
M = X.M


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


def _engine(V, P, batch=1, **kw):
    return V.Engine1D(P.N, P.Lx, P.tau, P.gamma, P.c1, P.c2, P.kappa, batch=batch, max_steps=8, **kw)


def _dts(t):
    d = np.diff(t)[1:]
    assert d.size == M and abs(d[-1] - 5e-3) < 1e-15              # five steps, the last one ragged
    return d


def _counts(st):
    return st["newton_iters"], st["linear_solves"], st["armijo_trials"], st["linear_iters"]     # linear_iters: failed_ls


def _ref_counts(sts):
    return tuple(sum(s[k] for s in sts) for k in ("newton_its", "solves", "armijo_trials", "failed_ls"))


def _mass_drift(P, ph):
    w = (P.Lx / P.N) * O1.trapz_weights(P.N + 1)
    m = ph @ w
    return float(np.max(np.abs(m - m[..., :1])))


# ---------------------------------------------------------------------------------------
# a. element-wise kernels and stand-alone solves at OFF2
# ---------------------------------------------------------------------------------------
def test_operators_solves_energy_off2(V):
    """apply_laplacian, residuals, jacobian_solve, adjoint_solve (step and terminal form) and free_energy (plain, with
    w_hist, with eps) at OFF2, N = 33, against the reference's vectors and the oracle."""
    g = golden("g1d_off2_33.npz")
    P = X.params("off2", 33)
    n, h, dt = P.N + 1, P.Lx / P.N, 1e-2
    e = _engine(V, P)
    m = {}
    m["lap"] = max(relerr(e.apply_laplacian(g["v"]), g["Lv"]), relerr(e.apply_laplacian(g["v"]), O1.lap(g["v"], h)))
    Rp, Rm = e.residuals(g["phi_new"], g["phi_old"], g["mu_new"], g["mu_old"], g["w_new"], g["w_old"], dt)
    m["Rphi"], m["Rmu"] = relerr(Rp, g["Rphi"]), relerr(Rm, g["Rmu"])
    m["Rphi_o"] = relerr(Rp, O1.residual_phi(g["phi_new"], g["phi_old"], g["mu_new"], g["mu_old"], g["w_new"], g["w_old"],
                                             dt, P, h))
    d = g["dvec"]
    dphi, dmu = e.jacobian_solve(g["phi_new"], dt, d[:n], d[n:])
    m["jac"] = max(relerr(dphi, g["Jsol"][:n]), relerr(dmu, g["Jsol"][n:]))
    hp = O1.hp_solve(O1.newton_rows(g["phi_new"], dt, P, h), np.stack([d[:n], d[n:]], 1).ravel())
    m["jac_hp"] = max(relerr(dphi, hp[0::2]), relerr(dmu, hp[1::2]))
    pa, pt = e.adjoint_solve(g["phi_new"], dt, g["v"]), e.adjoint_solve(None, 0.0, g["v"])
    m["adj"] = max(relerr(pa, g["Asol"]), relerr(pa, O1.hp_solve(O1.adjoint_rows(g["phi_new"], dt, h), g["v"])))
    m["adjT"] = max(relerr(pt, g["ATsol"]), relerr(pt, O1.hp_solve(O1.adjoint_rows(None, 0.0, h, n=n), g["v"])))
    E = {"E": e.free_energy(g["phi_u"]), "E_w": e.free_energy(g["phi_u"], w_hist=g["w_hist"]),
         "E_sep_eps": e.free_energy(g["phi_sep_u"], eps=0.5 * O1.DELTA_SEP)}
    Eo = {"E": [O1.free_energy(p, P.kappa, P.c1, P.c2, h) for p in g["phi_u"]],
          "E_w": [O1.free_energy(p, P.kappa, P.c1, P.c2, h, w=w) for p, w in zip(g["phi_u"], g["w_hist"])],
          "E_sep_eps": [O1.free_energy(p, P.kappa, P.c1, P.c2, h, eps=0.5 * O1.DELTA_SEP) for p in g["phi_sep_u"]]}
    for k in E:
        m[k] = max(float(np.max(np.abs(E[k] - r) / np.maximum(1.0, np.abs(r)))) for r in (g[k], np.array(Eo[k])))
    e.close()
    print("\nops off2: " + " ".join(f"{k} {v:.2e}" for k, v in m.items()))
    assert max(m["lap"], m["Rphi"], m["Rmu"], m["Rphi_o"]) < OPS, m
    assert max(m["jac"], m["jac_hp"], m["adj"], m["adjT"]) < SOLVE, m
    assert max(m["E"], m["E_w"], m["E_sep_eps"]) <= 1e-13, m


# ---------------------------------------------------------------------------------------
# b. the march inside the window
# ---------------------------------------------------------------------------------------
GOLD_ROWS = {("smooth", 12.0): ("phi_nat", "phi_u", "phi_ushort"), ("sep", 12.0): ("phi_sep_nat", "phi_sep_u", None)}


@pytest.mark.parametrize("N", X.MARCH_NS)
@pytest.mark.parametrize("point", ["off", "off2"])
def test_march_inside_the_window_vs_oracle(V, point, N):
    """B = 3 (X.BATCH[point]), five steps with a ragged last one, without control, with control and with the control cut to
    M rows (hold-last branch): summed Newton / solve / Armijo counts equal the oracle's and no line-search failure on
    either side; fields to max(1e-9, 20 eps cond_J) against O1.forward(solver="banded") and, at N = 33, the reference's
    own histories; the control moves the state by > 100 x that; mass (weights h trapz, h = Lx / N: a shift divided by 1
    instead of Lx shows here) conserved to 1e-12; trajectory 1 bit for bit its own B = 1 run."""
    cases = [X.march_case(*c, N) for c in X.BATCH[point]]
    P = cases[0]["P"]
    g = golden(f"g1d_{point}_33.npz") if N == 33 else None
    tol = max(X.march_tol(c) for c in cases)
    dts = _dts(cases[0]["t"])
    phi0, U = np.stack([c["phi0"] for c in cases]), np.stack([c["ctl"] for c in cases])
    e3, e1 = _engine(V, P, 3), _engine(V, P, 1)
    worst = dict(oracle=0.0, gold=0.0, drift=0.0)
    for j, (tag, u) in enumerate((("nat", None), ("u", U), ("short", U[:, :M]))):
        ph, st = e3.forward(phi0, dts, u=u)
        sts = [c[tag][1] for c in cases]
        assert all(X.in_march_window(s)[0] for s in sts)
        assert _counts(st) == _ref_counts(sts) and st["linear_iters"] == 0, (tag, st, _ref_counts(sts))
        for b, c in enumerate(cases):
            worst["oracle"] = max(worst["oracle"], relerr(ph[b], c[tag][0]))
            key = GOLD_ROWS.get(X.BATCH[point][b][1:], (None,) * 3)[j]
            if g is not None and key is not None:
                worst["gold"] = max(worst["gold"], relerr(ph[b], g[key]))
        worst["drift"] = max(worst["drift"], _mass_drift(P, ph))
        if tag != "nat":
            assert min(relerr(ph[b], cases[b]["nat"][0]) for b in range(3)) > 100 * tol, tag
        ph1, st1 = e1.forward(phi0[1], dts, u=None if u is None else u[1])
        assert np.array_equal(ph1, ph[1]), tag
    e3.close()
    e1.close()
    print(f"\nmarch {point} N={N}: relerr oracle {worst['oracle']:.2e} fixture {worst['gold']:.2e} tol {tol:.2e} "
          f"mass drift {worst['drift']:.2e}")
    assert worst["oracle"] < tol and worst["gold"] < tol and worst["drift"] <= 1e-12, worst


# ---------------------------------------------------------------------------------------
# c. single Newton calls whose first step is cut by the ceiling
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("point,N,seed", X.CAPPED)
def test_newton_capped_first_step_vs_oracle(V, point, N, seed):
    """newton_raphson on the capped-step window: as many norms as the oracle, equal to rtol 1e-6 except the last
    (test_newton_vs_golden), phi_new and mu_new to SOLVE; at N = 33 off the default point also the reference's own call.
    vch1d_newton_raphson returns no counts, so the same call is run once more as a one-step march -- w = 0 and
    mu = mu_init(phi, 0) are the march's start, and the control u_0 = u_1 = (gamma/dt + 1/2) w_new makes the filter
    return w_new to an ulp -- whose linear_solves, armijo_trials and newton_iters must equal the oracle's."""
    c = X.capped_case(point, N, seed)
    P, st = c["P"], c["st"]
    e = _engine(V, P)
    pn, mn, hist = e.newton_raphson(c["phi"], c["mu"], c["w_old"], c["w_new"], c["dt"])
    assert len(hist) == len(c["hist"]), (hist, c["hist"])
    assert np.allclose(hist[:-1], c["hist"][:-1], rtol=1e-6, atol=0)
    err = max(relerr(pn, c["phi_new"]), relerr(mn, c["mu_new"]))
    if point != "default" and N == 33:
        g = golden(f"g1d_{point}_33.npz")
        assert int(g["nr_seed"]) == seed and len(hist) == len(g["nr_hist"])
        assert np.allclose(hist[:-1], g["nr_hist"][:-1], rtol=1e-6, atol=0)
        err = max(err, relerr(pn, g["nr_phi_new"]), relerr(mn, g["nr_mu_new"]))
    u = np.tile((P.gamma / c["dt"] + 0.5) * c["w_new"], (2, 1))
    assert relerr(O1.w_filter(c["w_old"], c["dt"], P.gamma, u[0], u[1]), c["w_new"]) < 4 * EPS
    ph, fs = e.forward(c["phi"], np.array([c["dt"]]), u=u)
    e.close()
    assert (fs["linear_solves"], fs["armijo_trials"], fs["newton_iters"], fs["linear_iters"]) == \
        (st["solves"], st["armijo_trials"], st["newton_its"], 0), (fs, st)
    stepped = np.clip(c["phi_new"], -1 + O1.DELTA_SEP, 1 - O1.DELTA_SEP)
    w = (P.Lx / N) * O1.trapz_weights(N + 1)
    stepped = stepped - (w @ stepped - w @ c["phi"]) / P.Lx
    err_step = relerr(ph[2], stepped)
    print(f"\nnewton capped {point} N={N} seed {seed}: norms {len(hist)} relerr {err:.2e} one-step march {err_step:.2e}")
    assert err < SOLVE and err_step < SOLVE


# ---------------------------------------------------------------------------------------
# d. a batch with a knife-edge trajectory: properties only
# ---------------------------------------------------------------------------------------
def test_knife_edge_batch_properties(V):
    """OFF2, N = 33, B = 3: smooth / amp 12, sep / amp 200 (knife edge: the oracle leaves two of its five loops through
    maxit and the line-search failure, decided at distance 0.0 from the thresholds), sep / amp 12.  Each trajectory is
    bit for bit its own B = 1 run and the batch's counters are the sums of the singles'; trajectories 0 and 2 match the
    oracle as in b; trajectory 1 is finite, inside (-1, 1), conserves mass to 1e-12, and not every one of its loops
    converged: per loop the norms recorded exceed the solves by one exactly when it converged, so
    newton_iters - linear_solves < M.  Nothing is asserted about which exit it took, or in which step."""
    cases = [X.march_case(*c, 33) for c in X.KNIFE_BATCH]
    P = cases[0]["P"]
    assert not X.in_march_window(cases[1]["u"][1])[0]
    dts = _dts(cases[0]["t"])
    phi0, U = np.stack([c["phi0"] for c in cases]), np.stack([c["ctl"] for c in cases])
    e3, e1 = _engine(V, P, 3), _engine(V, P, 1)
    ph, st = e3.forward(phi0, dts, u=U)
    singles = [e1.forward(phi0[b], dts, u=U[b]) for b in range(3)]
    e3.close()
    e1.close()
    for b in range(3):
        assert np.array_equal(singles[b][0], ph[b]), b
    assert _counts(st) == tuple(sum(_counts(s[1])[k] for s in singles) for k in range(4)), (st, singles)
    errs = []
    for b in (0, 2):
        ref, rs = cases[b]["u"]
        assert _counts(singles[b][1]) == _ref_counts([rs]), (b, singles[b][1], rs)
        errs.append(relerr(ph[b], ref))
        assert errs[-1] < X.march_tol(cases[b]), (b, errs)
    s1 = singles[1][1]
    drift = _mass_drift(P, ph[1])
    conv = s1["newton_iters"] - s1["linear_solves"]
    print(f"\nknife edge: relerr b0 {errs[0]:.2e} b2 {errs[1]:.2e}; b1 converged loops {conv} of {M} (oracle "
          f"{sum(k[0] == 'conv' for k in cases[1]['u'][1]['exits'])}), failed_ls {s1['linear_iters']}, "
          f"max|phi| {np.abs(ph[1]).max():.6f}, mass drift {drift:.2e}")
    assert np.isfinite(ph[1]).all() and np.abs(ph[1]).max() < 1.0 and drift <= 1e-12
    assert conv < M, s1


# ---------------------------------------------------------------------------------------
# d2. a start beyond the clip: the only march in which the mass shift is not round-off
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", X.MARCH_NS)
def test_clipped_start_mass_shift_vs_oracle(V, N):
    """In every converged step the mass defect before the shift is round-off (the mu equation is linear, one full Newton
    step removes it), so (mass - mass_0) / Lx and (mass - mass_0) / 1 cannot be told apart there.  X.CLIPPED starts with
    >= 10 nodes beyond 1 - delta_sep: the first loop finds no admissible trial point in 12 halvings (decided >= 3.6e-3
    from the threshold, not by round-off), returns the old state, the clip bites and the shift is 1.2e-3.  OFF2, B = 3:
    counts (one line-search failure per trajectory, no Armijo trial in that loop) and fields against the oracle as in
    b, mass to 1e-12.  At N = 33 also OFF (Lx = 1.3), properties only because its later loops end near the tolerance:
    row 2 is the clipped start minus the oracle's shift, to 1e-14 (two n-term mass sums: n eps = 7.5e-15), and mass
    holds to 1e-12 on every row."""
    cases = [X.march_case(*c, N) for c in X.CLIPPED]
    P = cases[0]["P"]
    tol = max(X.march_tol(c) for c in cases)
    dts = _dts(cases[0]["t"])
    phi0, U = np.stack([c["phi0"] for c in cases]), np.stack([c["ctl"] for c in cases])
    e3 = _engine(V, P, 3)
    worst = dict(oracle=0.0, drift=0.0)
    for tag, u in (("nat", None), ("u", U)):
        ph, st = e3.forward(phi0, dts, u=u)
        sts = [c[tag][1] for c in cases]
        assert all(X.in_clipped_window(s)[0] for s in sts)
        assert _counts(st) == _ref_counts(sts) and st["linear_iters"] == 3, (tag, st, _ref_counts(sts))
        worst["oracle"] = max([worst["oracle"]] + [relerr(ph[b], c[tag][0]) for b, c in enumerate(cases)])
        worst["drift"] = max(worst["drift"], _mass_drift(P, ph))
        assert all(abs(X.first_shift(c, tag)) > 1e-4 for c in cases)
    e3.close()
    msg = f"\nclipped start off2 N={N}: relerr oracle {worst['oracle']:.2e} tol {tol:.2e} mass drift {worst['drift']:.2e}"
    if N == 33:
        c = X.march_case(*X.CLIPPED_PROP, 33)
        e = _engine(V, c["P"])
        ph, st = e.forward(c["phi0"], dts, u=c["ctl"])
        e.close()
        row2 = np.clip(c["phi0"], -1 + O1.DELTA_SEP, 1 - O1.DELTA_SEP) - X.first_shift(c)
        e2, dr = relerr(ph[2], row2), _mass_drift(c["P"], ph)
        msg += f"; off: row 2 {e2:.2e} mass drift {dr:.2e} failed_ls {st['linear_iters']}"
        assert np.isfinite(ph).all() and e2 < 1e-14 and dr <= 1e-12 and st["linear_iters"] >= 1
    print(msg)
    assert worst["oracle"] < tol and worst["drift"] <= 1e-12, worst


# ---------------------------------------------------------------------------------------
# e. adjoint sweep and cost at Lx != 1
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _adjoint_ref(N, targets):
    """The oracle's banded sweep on its own controlled OFF2 history and the Skeel condition of every level's system."""
    c = X.march_case("off2", "smooth", 12.0, N)
    P, x, t = c["P"], c["x"], c["t"]
    h = P.Lx / N
    ph = golden("g1d_off2_33.npz")["phi_u"] if N == 33 else c["u"][0]
    o = X.PGD_OPT
    if targets:
        phi_T, phi_Q = O1.build_targets(x, t, c["phi0"], P.Lx, P.T, 1, 1)
        b1, b2 = o["b1"], o["b2"]
    else:
        phi_T, phi_Q, b1, b2 = None, None, 1.3, 0.7
    p, q, r = O1.backward(ph, x, t, b1, b2, phi_Q, phi_T, solver="banded")
    conds = []
    for k in range(M, 0, -1):
        dt = t[k + 1] - t[k]
        src = 0.5 * dt * b1 * ((ph[k] + ph[k + 1]) - (0.0 if phi_Q is None else phi_Q[k] + phi_Q[k + 1]))
        rhs = O1._rows_matvec(O1.adjoint_rhs_rows(ph[k + 1], dt, h), p[k + 1]) + src
        conds.append(O1.cond_estimate(O1.adjoint_rows(ph[k], dt, h), p[k], rhs))
    return dict(P=P, x=x, t=t, ph=ph, phi_T=phi_T, phi_Q=phi_Q, b1=b1, b2=b2, p=p, q=q, r=r,
                tol=max(1e-9, 20 * EPS * max(conds)))


@pytest.mark.parametrize("N", X.MARCH_NS)
def test_adjoint_sweep_and_cost_off_unit_length(V, N):
    """backward on the controlled OFF2 history (N = 33: the reference's own; N = 64: the oracle's), x = linspace(0, Lx,
    N + 1), with build_targets' targets and without: an engine created with OFF2 and one with the defaults plus Lx = 0.7
    give bit-identical p, q, r (the adjoint is frozen at the default tau, gamma, c1, c2 except for h); p, r against
    O1.backward(solver="banded") to max(1e-9, 20 eps max_k cond_k), q = -L p to 4 eps componentwise, and at N = 33 all
    three against the reference's sweep.  The five cost components against O1.cost_parts to 1e-12 relative, grad_prox
    to 1e-14."""
    P = X.params("off2", N)
    n, h = N + 1, P.Lx / N
    e, ed = _engine(V, P), V.Engine1D(N=N, Lx=P.Lx, max_steps=8)
    g = golden("g1d_off2_33.npz") if N == 33 else None
    Lrows = O1._lap_rows(n, h)
    m = {}
    for targets in (True, False):
        a = _adjoint_ref(N, targets)
        p, q, r = e.backward(a["ph"], a["t"], a["b1"], a["b2"], a["phi_Q"], a["phi_T"])
        pd, qd, rd = ed.backward(a["ph"], a["t"], a["b1"], a["b2"], a["phi_Q"], a["phi_T"])
        assert np.array_equal(r, rd) and np.array_equal(p, pd) and np.array_equal(q, qd)
        assert not p[0].any() and not r[0].any()                          # B1:110
        ep, er = relerr(p, a["p"]), relerr(r, a["r"])
        wq = max(O1.backward_error(Lrows, p[k], -q[k]) for k in range(M + 2))
        m[targets] = (ep, er, a["tol"], wq / EPS)
        assert ep < a["tol"] and er < a["tol"] and wq <= 4 * EPS, (targets, m)
        if g is not None:
            keys = ("p", "q", "r") if targets else ("p_none", "q_none", "r_none")
            if targets:
                assert relerr(a["phi_Q"], g["phi_Q"]) < 1e-15 and relerr(a["phi_T"], g["phi_T"]) < 1e-15
            eg = max(relerr(v, g[k]) for v, k in zip((p, q, r), keys))
            m[targets] += (eg,)
            assert eg < a["tol"], (targets, eg)
    # cost and prox: x carries Lx (trapezoid in x), t the ragged step
    a = _adjoint_ref(N, True)
    o = X.PGD_OPT
    opt = V.make_opt(O1.OptParams1D(**o))
    uc = X.control(P, 12.0) / 20.0
    J = e.cost(a["ph"], uc, a["phi_Q"], a["phi_T"], a["x"], a["t"], opt)
    parts = O1.cost_parts(a["ph"], uc, a["phi_Q"], a["phi_T"], a["x"], a["t"], o["b1"], o["b2"], o["b3"], o["kappa_sparsity"])
    ref5 = np.concatenate([parts, [parts.sum()]])
    ec = float(np.max(np.abs(J / ref5 - 1)))
    assert np.all(ref5 > 0) and ec < 1e-12, (J, ref5)
    un = e.grad_prox(uc, a["r"], 7.0, opt)
    px = O1.prox_project(O1.gradient_step(uc, O1.gradient(a["r"], uc, o["b3"]), 7.0), 7.0, o["kappa_sparsity"], o["u_min"],
                         o["u_max"])
    eu = relerr(un, px)
    assert (px == 0).any() and (px == o["u_min"]).any() and (px == o["u_max"]).any() and eu < 1e-14
    if g is not None:
        assert np.array_equal(uc, g["u_cost"]) and abs(J[4] / float(g["J"]) - 1) < 1e-12
        assert relerr(e.grad_prox(g["u_cost"], g["r"], float(g["prox_alpha"]), opt), g["prox"]) < 1e-14
    e.close()
    ed.close()
    print(f"\nadjoint off2 N={N}: " + "; ".join(
        f"targets={k}: p {v[0]:.2e} r {v[1]:.2e} tol {v[2]:.2e} q omega/eps {v[3]:.2g}" +
        (f" fixture {v[4]:.2e}" if len(v) > 4 else "") for k, v in m.items()) + f"; cost {ec:.2e} prox {eu:.2e}")


# ---------------------------------------------------------------------------------------
# f. the device-resident PGD loop
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", X.PGD_NS)
@pytest.mark.parametrize("point", X.PGD_POINTS)
def test_pgd_resident_inside_the_window_vs_oracle(V, point, N):
    """pgd_init with phi_Q = None (the device ramp; T = 0.045, so t / T differs from t) and four iterations against
    O1.pgd(solver="banded", initial_phi=...): trials [1, 5, 1, 5] (the accepted optimistic step and the search that
    returns its last try), alpha to 1e-12, J0 and costs to 1e-9, u, phi, r to 1e-8, the device phi_Q against
    build_targets to 1e-15; the zero pattern of u equals the oracle's wherever the prox argument is >= 1e-6 away from
    the threshold (>= 95 % of the nodes).  With b1, b2, b3, the sparsity weight and the box all off their defaults and
    about half of u zero and 0.4 of it on the box."""
    c = X.pgd_case(point, N)
    P, Op, ref = c["P"], c["Op"], c["res"]
    t = ref.t_hist
    e = _engine(V, P)
    J0 = e.pgd_init(c["phi0"], ref.phi_T, t, _dts(t), V.make_opt(Op))
    out = e.pgd_iterate(X.PGD_ITERS)
    u, phi, r, phi_Q = (e.pgd_get(k) for k in ("u", "phi", "r", "phi_Q"))
    e.close()
    assert list(out["trials"][0]) == list(ref.trials) == [1, 5, 1, 5], (out["trials"], ref.trials)
    ea = float(np.max(np.abs(out["alpha"][0] / np.array(ref.alphas) - 1)))
    ec = max(abs(J0[0, 4] / ref.costs[0] - 1), float(np.max(np.abs(out["cost"][0] / np.array(ref.costs[1:]) - 1))))
    eu, ep, er, eq = relerr(u, ref.u), relerr(phi, ref.phi), relerr(r, ref.r), relerr(phi_Q, ref.phi_Q)
    keep = c["band"] >= X.BAND
    print(f"\npgd {point} N={N}: alpha {ea:.2e} cost {ec:.2e} u {eu:.2e} phi {ep:.2e} r {er:.2e} phi_Q {eq:.2e} "
          f"pattern compared on {keep.mean():.4f}, zero {np.mean(u == 0):.3f}")
    assert ea < 1e-12 and ec < 1e-9 and max(eu, ep, er) < 1e-8 and eq < 1e-15
    assert keep.mean() >= 0.95 and np.array_equal((u == 0)[keep], (ref.u == 0)[keep])


def test_pgd_resident_batch_is_its_singles(V):
    """One B = 3 run at OFF2, N = 33, with three phase shifts of phi0, is bit for bit its three B = 1 runs."""
    cs = [X.pgd_case("off2", 33, s) for s in X.PGD_SHIFTS]
    P, Op = cs[0]["P"], cs[0]["Op"]
    t = cs[0]["res"].t_hist
    phi0, phi_T = np.stack([c["phi0"] for c in cs]), np.stack([c["res"].phi_T for c in cs])

    def run(eng, p0, pT):
        J0 = eng.pgd_init(p0, pT, t, _dts(t), V.make_opt(Op))
        out = eng.pgd_iterate(X.PGD_ITERS)
        return J0, out, [eng.pgd_get(k) for k in ("u", "phi", "r")]

    e3, e1 = _engine(V, P, 3), _engine(V, P, 1)
    J3, o3, f3 = run(e3, phi0, phi_T)
    for b in range(3):
        J1, o1, f1 = run(e1, phi0[b], phi_T[b])
        assert np.array_equal(J1[0], J3[b])
        for k in ("cost", "alpha", "trials"):
            assert np.array_equal(o1[k][0], o3[k][b]), (b, k)
        assert list(o1["trials"][0]) == list(cs[b]["res"].trials)
        for a1, a3 in zip(f1, f3):
            assert np.array_equal(a1, a3[b]), b
    e3.close()
    e1.close()
