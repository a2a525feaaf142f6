"""Directional sparsity in the 1D engine where tests/test_gpu_dirsparse_1d.py does not look.

A. The resident loop off the one-block shape: N = 130, 512, 1500, 4096 (rows kernel built for 1, 2, 4 and 9 values per
   thread; 3, 9, 24 and 65 workgroups of the column kernel per trajectory, the last one ragged), 22 rows (more than the
   column kernel's 16 waves), a batch of four with a space trajectory behind a full and a time one, a warm start u0 with
   whole rows and columns at zero and parts outside the box, a step alpha0 per trajectory.  One accepted step is compared
   with the NumPy restatement (tests/_group_prox_ref.py) applied to the pulled adjoint: u+, the change the stop rule acts
   on, J4 before and after, the KKT counts and stationarity; at N = 130 three iterations against the restatement's loop
   over the oracle.
B. The prox seam at its three decisions (alive or zero, closed form or iteration, the end of the iteration), at lam = 0,
   at rho / lam up to 1e9, on nodes of zero weight and with a step per trajectory.
C. cost(..., u=None) of the group modes.
"""
import numpy as np
import pytest

import _group_prox_ref as G
from _group_edge_cases import MARGIN, _margins, build_alive, build_edge, build_lam0, build_mixed, build_zero_weight
from conftest import relerr

pytestmark = pytest.mark.gpu

BATCH, MAXROWS = 4, 33


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
            made[N] = V.Engine1D(N=N, batch=BATCH, max_steps=MAXROWS)
        return made[N]
    yield get
    for e in made.values():
        e.close()


# ---- A. the resident loop ----------------------------------------------------------------------------------------------
STEPS, DT = 20, 1e-2
MODES = ["space", "full", "time", "space"]
BOX = [(-0.3, 2.0), (-1.0, 1.0), (-0.05, 0.08), (-0.35, 0.0)]           # the last one is one-sided
PHI_AMP = (0.01, 0.2, 0.05, 0.1)
# Picked on the CPU with the restatement's loop over the oracle at N = 130 and 512 (see test_resident_matches_the_oracle_loop):
# the march under u0 converges, every first trial below descends except trajectory 0's, which backtracks (1.9 and 1.52
# ascend, 1.216 descends; the cost turns between 1.25 and 1.5625 at both sizes), and each accepted step has groups of all
# three kinds.
# The steps stay moderate on purpose: engine and oracle agree on the adjoint to 1e-9 relative (their Newton solves stop at
# different residuals), u+ = prox(u - alpha r) carries alpha times that difference, and with max|r| = 0.076 against controls of
# size 0.08 .. 0.4 three steps of alpha <= 10 keep it below 1e-8, a tenth of the 1e-7 the comparison with the oracle's loop allows
# (a first choice of alpha0 = 1000 for the time trajectory, under the box (-0.25, 0.4), put 1.05e-7 there after three steps).
ALPHA0 = (1.9, 30.0, 8.0, 5.0)
ALPHA_MAX = (50.0, 100.0, 8.0, 2.0)                                     # trajectory 3's first step is its cap
RES_SIZES = (130, 512, 1500, 4096)


def resident_problem(O1, N):
    """phi0, phi_T (4, n), t_hist, dts, x and the warm start u0 (4, 22, n): a few Fourier modes in x and t of amplitude up to
    0.6 (outside every box of BOX but the full member's), rows 5, 6 and 13 and the columns with 0.2 <= x <= 0.3 or index
    = 3 mod 7 exactly zero."""
    n = N + 1
    x = np.linspace(0.0, 1.0, n)
    t, ts, dts = 0.0, [0.0, 0.0], []                # the reference's accumulated-time rule, as the oracle's march takes it
    while t < STEPS * DT - 1e-10:
        dts.append(min(DT, STEPS * DT - t))
        t += dts[-1]
        ts.append(min(t, STEPS * DT))
    t_hist, dts = np.array(ts), np.array(dts)
    assert t_hist.size == STEPS + 2
    phi0 = np.stack([O1.init_phi_random(N, 1e-2, amp=a, seed=40 + b) for b, a in enumerate(PHI_AMP)])
    phi_T = np.repeat((0.7 * np.sin(2.0 * np.pi * x))[None], BATCH, axis=0)
    tt = (t_hist / t_hist[-1])[:, None]
    u0 = np.stack([0.35 * np.sin(2 * np.pi * x + b)[None] * np.cos(np.pi * tt) +
                   0.2 * np.sin(6 * np.pi * x - b)[None] * np.sin(3 * np.pi * tt + 0.4) +
                   0.08 * np.cos(10 * np.pi * x)[None] * np.cos(5 * np.pi * tt + b) for b in range(BATCH)])
    u0[:, [5, 6, 13], :] = 0.0
    u0[:, :, (x >= 0.2) & (x <= 0.3)] = 0.0
    u0[:, :, 3::7] = 0.0
    return phi0, phi_T, t_hist, dts, x, u0


def kappa_between(norms, q):
    """A threshold between two adjacent sorted group norms near the quantile q, in the middle of the widest relative gap
    of the five pairs around it: no group norm is closer to it than half that gap."""
    s = np.sort(norms[norms > 0.0])
    k = int(q * s.size)
    j = max(range(max(k - 2, 0), min(k + 3, s.size - 1)), key=lambda i: s[i + 1] / s[i])
    return float(0.5 * (s[j] + s[j + 1]))


def _opts(O1, ks):
    return [O1.OptParams1D(kappa_sparsity=ks[b], alpha_max=ALPHA_MAX[b], u_min=BOX[b][0], u_max=BOX[b][1]) for b in range(BATCH)]


@pytest.fixture(scope="module")
def resident(V, O1, engines):
    """N -> everything one accepted step of the batch leaves behind, computed once: a first init gives the adjoint at u0, whose
    group norms place kappa_sparsity of the group-mode trajectories (the adjoint at u0 does not depend on it); the second
    init is the problem under test: KKT statistic at u0, one iteration, the full member run alone, and at N = 130 two
    more iterations."""
    done = {}

    def get(N):
        if N in done:
            return done[N]
        eng = engines(N)
        phi0, phi_T, t_hist, dts, x, u0 = resident_problem(O1, N)
        mk = lambda ks: [V.make_opt(o) for o in _opts(O1, ks)]
        eng.pgd_init(phi0, phi_T, t_hist, dts, mk([1e-3] * BATCH), u0=u0, alpha0=ALPHA0, sparsity=MODES)
        eng.pgd_kkt(refresh=True)
        r_first = eng.pgd_get("r")
        ks = [O1.OptParams1D().kappa_sparsity if m == "full" else kappa_between(G.group_norms(r_first[b], x, t_hist, m), 0.5)
              for b, m in enumerate(MODES)]
        d = dict(N=N, x=x, t_hist=t_hist, dts=dts, phi0=phi0, phi_T=phi_T, u0=u0, ks=ks, opts=_opts(O1, ks), r_first=r_first)
        d["J0"] = eng.pgd_init(phi0, phi_T, t_hist, dts, mk(ks), u0=u0, alpha0=ALPHA0, sparsity=MODES)
        d["kkt"] = eng.pgd_kkt(refresh=True)
        d["r_kkt"] = eng.pgd_get("r")
        d["res"] = eng.pgd_iterate(1)
        d["r"], d["u"], d["phi"], phi_Q = (eng.pgd_get(k) for k in ("r", "u", "phi", "phi_Q"))
        if N == 130:
            d["res2"] = eng.pgd_iterate(2)
            d["u3"] = eng.pgd_get("u")
        # the cost of the accepted iterate through the function seam, each trajectory with its own parameters and mode (this
        # overwrites the resident control and state, so it comes last)
        d["Jc"] = np.stack([eng.cost(d["phi"], d["u"], phi_Q, phi_T, x, t_hist, mk(ks)[b], sparsity=MODES[b])[b] for b in range(BATCH)])
        e1 = V.Engine1D(N=N, batch=1, max_steps=STEPS)
        try:
            J1 = e1.pgd_init(phi0[1], phi_T[1], t_hist, dts, [mk(ks)[1]], u0=u0[1], alpha0=ALPHA0[1])
            d["single"] = (J1, e1.pgd_iterate(1), e1.pgd_get("u"), e1.pgd_get("phi"))
        finally:
            e1.close()
        done[N] = d
        return d
    return get


def _alpha_used(b, trials):
    a = min(ALPHA0[b], ALPHA_MAX[b])
    for _ in range(trials - 1):
        a *= 0.8
    return a


@pytest.mark.parametrize("N", RES_SIZES)
def test_resident_step_against_the_restatement(resident, N):
    """One accepted step of every group-mode trajectory from the warm start: u+ to 1e-12 max|v| of the restatement's prox of
    the pulled adjoint at the accepted step size, `change` to 1e-12 relative of ||u+ - u0||_F / (||u0||_F + 1e-9), J4 at u0,
    J4 of the accepted iterate and the loop's cost to 1e-13 relative.  Trajectory 0 backtracks (its first trials ascend),
    the others accept at once; every group-mode trajectory's accepted step has zero, closed-form and box-active groups."""
    d = resident(N)
    x, t, u0, r, res = d["x"], d["t_hist"], d["u0"], d["r"], d["res"]
    assert np.array_equal(d["r_first"], d["r_kkt"]) and np.array_equal(d["r"], d["r_kkt"])     # the adjoint at u0 each time
    assert res["iters"] == 1
    trials = [int(res["trials"][b, 0]) for b in range(BATCH)]
    assert trials[0] > 1 and trials[2] == 1 and trials[3] == 1, trials
    for b, mode in enumerate(MODES):
        if mode == "full":
            continue
        o = d["opts"][b]
        assert res["cost"][b, 0] < d["J0"][b, 4] and trials[b] < 5               # a descent: alpha is the step u+ was made with
        al = _alpha_used(b, trials[b])
        assert res["alpha"][b, 0] == al, (b, res["alpha"][b, 0], al)
        ur, sr, kinds = G.prox(u0[b], r[b], al, o.b3, o.kappa_sparsity, o.u_min, o.u_max, mode, x, t)
        v = u0[b] - al * (r[b] + o.b3 * u0[b])
        print(f"N {N} b {b} {mode}: trials {trials[b]} alpha {al:g} kinds { {k: kinds.count(k) for k in sorted(set(kinds))} } "
              f"u+ err {np.max(np.abs(d['u'][b] - ur)) / np.max(np.abs(v)):.2e}")
        assert set(kinds) == {"zero", "closed", "box"}, (N, b, set(kinds))
        assert np.max(np.abs(d["u"][b] - ur)) <= 1e-12 * np.max(np.abs(v)), (N, b)
        chg = np.linalg.norm(ur - u0[b]) / (np.linalg.norm(u0[b]) + 1e-9)
        assert abs(res["change"][b, 0] / chg - 1.0) <= 1e-12, (N, b, res["change"][b, 0], chg)
        assert abs(d["J0"][b, 3] / G.j4(u0[b], x, t, o.kappa_sparsity, mode) - 1.0) <= 1e-13, (N, b)
        assert abs(d["Jc"][b, 3] / G.j4(d["u"][b], x, t, o.kappa_sparsity, mode) - 1.0) <= 1e-13, (N, b)
        assert abs(res["cost"][b, 0] / d["Jc"][b, 4] - 1.0) <= 1e-13, (N, b)


@pytest.mark.parametrize("N", RES_SIZES)
def test_resident_full_member_keeps_the_bits_of_its_own_batch(resident, N):
    d = resident(N)
    J1, r1, u1, p1 = d["single"]
    assert np.array_equal(d["J0"][1], J1[0])
    for key in ("cost", "alpha", "trials", "change"):
        assert np.array_equal(d["res"][key][1], r1[key][0]), key
    assert np.array_equal(d["u"][1], u1) and np.array_equal(d["phi"][1], p1)


@pytest.mark.parametrize("N", RES_SIZES)
def test_resident_kkt_by_groups_at_the_warm_start(resident, N):
    """pgd_kkt(refresh=True) at u0: the four counts exactly and the stationarity to 1e-10 max(stat, 1) of the restatement on
    u0 and the pulled adjoint.  kappa_sparsity lies between two adjacent group norms of the adjoint and u0's groups are
    exactly zero or far above the tolerance 1e-6, so no decision is within 1e-9 of its threshold; no group is left out."""
    d = resident(N)
    x, t, u0, r, k = d["x"], d["t_hist"], d["u0"], d["r_kkt"], d["kkt"]
    n = N + 1
    for b, mode in enumerate(MODES):
        if mode == "full":
            assert k["total"][b] == t.size * n
            continue
        o = d["opts"][b]
        gr, gu = G.group_norms(r[b], x, t, mode), G.group_norms(u0[b], x, t, mode)
        assert np.min(np.abs(gr / o.kappa_sparsity - 1.0)) >= 1e-9 and np.min(np.abs(gu / 1e-6 - 1.0)) >= 1e-9
        cnt, stat = G.kkt(u0[b], r[b], x, t, o.b3, o.kappa_sparsity, o.u_min, o.u_max, mode)
        got = [k["n_zero"][b], k["n_small"][b], k["n_match"][b], k["total"][b]]
        print(f"N {N} b {b} {mode}: counts {got} stationarity {k['stationarity'][b]:.6e} (restatement {stat:.6e})")
        assert got == list(cnt), (N, mode, got, cnt)
        assert cnt[3] == (t.size if mode == "time" else n) and 0 < cnt[0] < cnt[3] and 0 < cnt[1] < cnt[3]
        assert abs(k["stationarity"][b] - stat) <= 1e-10 * max(stat, 1.0), (N, b, k["stationarity"][b], stat)


@pytest.mark.parametrize("b", [0, 2, 3])
def test_resident_matches_the_oracle_loop(resident, O1, b):
    """Three iterations at N = 130 against the restatement's loop over the oracle from the same u0 and alpha0: the trials,
    the costs to 1e-9, u to 1e-7 and the change to 1e-6 relative (the tolerances of the u = 0 resident test)."""
    d = resident(130)
    P = O1.Params1D(N=130, T=STEPS * DT, dt_initial=DT)
    ref = G.pgd(O1, P, d["opts"][b], MODES[b], 3, initial_phi=d["phi0"][b], u0=d["u0"][b], alpha0=ALPHA0[b])
    assert np.array_equal(ref["t_hist"], d["t_hist"])
    got = {k: np.r_[d["res"][k][b], d["res2"][k][b]] for k in ("cost", "trials", "change")}
    print(f"b {b}: trials {list(got['trials'])} / {ref['trials']}  costs {list(got['cost'])}  change {list(got['change'])}")
    assert list(got["trials"]) == ref["trials"]
    assert np.allclose(np.r_[d["J0"][b, 4], got["cost"]], ref["costs"], rtol=1e-9, atol=0.0)
    assert relerr(d["u3"][b], ref["u"]) < 1e-7
    assert np.allclose(got["change"], ref["change"], rtol=1e-6, atol=0.0)


# ---- B. the prox seam at its decisions ------------------------------------------------------------------------------------
LD = np.longdouble
BOXES = ((-1.0, 1.0), (-0.3, 2.0), (0.0, 1.0), (-1.0, 0.0), (-np.inf, np.inf))
SEAM_SIZES = (24, 64, 512)
SEAM_ROWS = (3, 16, 17, 33)                        # below, at and past the column kernel's 16 waves, and past twice that
ALPHAS = np.array([0.5, 0.25, 1.0, 2.0])           # a step per trajectory; powers of two: with b3 = 0, v = u - alpha r is one rounding
KS = 0.04


def _grids(rng, n, rows, repeat_x=False):
    x = np.cumsum(np.r_[0.0, rng.uniform(0.5, 1.5, n - 1)])
    if repeat_x:                                    # a node three times: one weight exactly zero between two halved ones
        j = n // 2
        x[j + 1:] -= x[j + 1] - x[j]
        x[j + 2:] -= x[j + 2] - x[j]
        assert x[j] == x[j + 1] == x[j + 2] and G.trapz_w(x)[j + 1] == 0.0
    x /= x[-1]
    t = np.r_[0.0, 0.0, np.cumsum(rng.uniform(0.5, 1.5, rows - 2))]       # t = 0 twice, as in a history: wt[0] = 0
    return x, t / t[-1]


FLOORS = {}                                         # regime -> [the restatement's |s_double - s_long double|, |s_gpu - s_ref|], the largest seen


def _seam(V, eng, regime, build, mode, N, ks, b3=0.0, repeat_x=False, boxes=BOXES, seed=0):
    """Runs `build` through grad_prox at every row count and box and checks against the restatement: the kind of every group
    (s == 0 exactly where it says zero, s > 0 elsewhere; the inputs keep MARGIN from both decisions, measured in long
    double on the v the kernel forms), s to 1e-12 absolute, u+ to 1e-12 max|v|, and with b3 = 0 the bits of s v on the
    closed-form groups.  -> the kinds seen."""
    n = N + 1
    rng = np.random.default_rng(7000 + 10 * N + (mode == "space") + seed)
    seen = set()
    fl = FLOORS.setdefault(regime, [0.0, 0.0])
    for rows in SEAM_ROWS:
        x, t = _grids(rng, n, rows, repeat_x)
        w = G.trapz_w(x) if mode == "time" else G.trapz_w(t)
        ng, m = (rows, n) if mode == "time" else (n, rows)
        for lo, hi in boxes:
            vg = np.stack([build(rng, ng, m, w, ALPHAS[b] * ks, lo, hi) for b in range(BATCH)])
            v = vg if mode == "time" else np.ascontiguousarray(vg.transpose(0, 2, 1))
            r = rng.standard_normal(v.shape) * np.sqrt(np.mean(v * v, axis=(1, 2)))[:, None, None]
            dead = ~vg.any(axis=2)                  # an all-zero group stays one: r = 0 there
            r = np.where(dead[:, :, None] if mode == "time" else dead[:, None, :], 0.0, r)
            al = ALPHAS[:, None, None]
            u = (v + al * r) / (1.0 - al * b3)
            opt = V.make_opt(b3=b3, kappa_sparsity=ks, u_min=lo, u_max=hi)
            up, s = eng.grad_prox(u, r, ALPHAS, opt, sparsity=mode, x=x, t_hist=t, return_scale=True)
            for b in range(BATCH):
                tag = (regime, mode, N, rows, lo, hi, b)
                va = u[b] - ALPHAS[b] * (r[b] + b3 * u[b])              # the v both sides form
                alive, vote = _margins(va if mode == "time" else va.T, w, ALPHAS[b] * ks, lo, hi)
                assert np.min(np.abs(alive)) >= MARGIN and (vote.size == 0 or np.min(np.abs(vote)) >= MARGIN), tag
                ur, sr, kr = G.prox(u[b], r[b], ALPHAS[b], b3, ks, lo, hi, mode, x, t)
                sl, kl = G.prox(u[b], r[b], ALPHAS[b], b3, ks, lo, hi, mode, x, t, dtype=LD)[1:]
                kr = np.array(kr)
                assert list(kr) == kl and np.array_equal(kr != "zero", alive > 0.0), tag
                if vote.size:
                    assert np.array_equal(kr[kr != "zero"] == "box", vote > 0.0), tag
                seen |= set(kr)
                fl[0] = max(fl[0], float(np.max(np.abs(sr - sl))))
                fl[1] = max(fl[1], float(np.max(np.abs(s[b] - sr))))
                assert np.array_equal(s[b] == 0.0, kr == "zero"), tag
                assert np.max(np.abs(s[b] - sr)) <= 1e-12, tag
                assert np.max(np.abs(up[b] - ur)) <= 1e-12 * max(np.max(np.abs(va)), 1e-300), tag
                if b3 == 0.0:
                    sv = s[b][:, None] * va if mode == "time" else s[b][None, :] * va
                    closed = kr == "closed"
                    pick = (lambda a: a[closed]) if mode == "time" else (lambda a: a[:, closed])
                    assert np.array_equal(pick(up[b]), pick(sv)), tag
    print(f"{regime} {mode} N {N}: restatement's floor {fl[0]:.2e}, gpu {fl[1]:.2e} (largest so far), kinds {sorted(str(k) for k in seen)}")
    return seen


SEAM = pytest.mark.parametrize("mode,N", [(m, N) for m in ("time", "space") for N in SEAM_SIZES])


@SEAM
def test_seam_barely_alive_and_barely_dead(V, engines, mode, N):
    """c / lam - 1 = +-1e-9, +-1e-6, +-1e-3 on every box; measured (MI355X, largest over the cases): the restatement's own
    floor |s_double - s_long double| 3.2e-16, |s_gpu - s_ref| 4.4e-16."""
    seen = _seam(V, engines(N), "alive", build_alive, mode, N, KS)
    assert seen == {"zero", "closed", "box"}


@SEAM
def test_seam_barely_closed_and_barely_box(V, engines, mode, N):
    """max|s0 v| at (1 -+ 1e-9) and (1 -+ 1e-6) of a bound, the four finite boxes; measured: floor 2.4e-16, gpu 2.8e-16."""
    seen = _seam(V, engines(N), "edge", build_edge, mode, N, KS, boxes=BOXES[:4])
    assert seen == {"closed", "box"}


@SEAM
@pytest.mark.parametrize("ratio", [1e3, 1e6, 1e9])
def test_seam_at_large_rho_over_lam(V, engines, mode, N, ratio):
    """lam = alpha 0.5 / ratio against groups of amplitude 3 (rho ~ the bound: rho / lam ~ ratio, the box active) and 0.05
    (closed form, s0 = 1 - O(1 / ratio)).  h' <= -rho at the root, so the root is as well conditioned as at
    rho / lam = 1 and the 1e-12 of the project holds unchanged; measured at each ratio: floor 1.1e-16, gpu 1.1e-16.  b3 = 0 here like
    everywhere at the seam: with b3 = 0.1 the kernel's v (two fused roundings) and NumPy's (three) differ by an ulp of u, a
    column of two weighted entries where u and alpha r cancel then has ||v|| off by 4e-13 relative, and s0 = 1 - lam / ||v||
    moved by 5.7e-14 at ratio 1e3 (measured on the MI355X, reproduced on the CPU by forming v the kernel's way): a
    statement about the inputs, not about the prox."""
    seen = _seam(V, engines(N), f"ratio {ratio:g}", build_mixed, mode, N, 0.5 / ratio, seed=int(np.log10(ratio)))
    assert {"closed", "box"} <= seen              # and "zero": a group of three with nothing inside a one-sided box's cone


@SEAM
def test_seam_at_lam_zero_is_the_projection(V, engines, mode, N):
    """kappa_sparsity = 0: s == 1.0 exactly on every group with a weighted entry inside the cone, s == 0 and u+ = 0 on the
    all-zero group, u+ == clip(v) bit for bit in both group modes and the full-mode grad_prox within 1e-15 max|v| of it (it
    forms v with other roundings)."""
    eng, n = engines(N), N + 1
    rng = np.random.default_rng(8000 + N + (mode == "space"))
    for rows in SEAM_ROWS:
        x, t = _grids(rng, n, rows)
        w = G.trapz_w(x) if mode == "time" else G.trapz_w(t)
        ng, m = (rows, n) if mode == "time" else (n, rows)
        for lo, hi in BOXES:
            vg = np.stack([build_lam0(rng, ng, m, w, 0.0, lo, hi) for b in range(BATCH)])
            v = vg if mode == "time" else np.ascontiguousarray(vg.transpose(0, 2, 1))
            r = np.where(v == 0.0, 0.0, rng.standard_normal(v.shape))
            u = v + ALPHAS[:, None, None] * r
            opt = V.make_opt(b3=0.0, kappa_sparsity=0.0, u_min=lo, u_max=hi)
            up, s = eng.grad_prox(u, r, ALPHAS, opt, sparsity=mode, x=x, t_hist=t, return_scale=True)
            full = eng.grad_prox(u, r, ALPHAS, opt)
            va = u - ALPHAS[:, None, None] * r
            assert np.all(s[:, 0] == 0.0) and np.all(s[:, 1:] == 1.0), (mode, N, rows, lo, hi)
            assert np.array_equal(up, np.clip(va, lo, hi)), (mode, N, rows, lo, hi)
            assert not (up[:, 0] if mode == "time" else up[:, :, 0]).any()
            assert np.max(np.abs(full - up)) <= 1e-15 * np.max(np.abs(va)), (mode, N, rows, lo, hi)


@SEAM
def test_seam_on_nodes_of_zero_weight(V, engines, mode, N):
    """Space: wt[0] = 0 (t = 0 twice) and every column's row 0 holds +-50; time: an x grid with a node three times (one
    weight zero, two halved) and +-50 on those nodes.  A group whose weighted rest is below lam vanishes, entry of 50
    included; in the others that entry is scaled and clipped like the rest.  Measured: floor 2.8e-16, gpu 3.6e-16."""
    seen = _seam(V, engines(N), "zero weight", build_zero_weight, mode, N, KS, repeat_x=True)
    assert seen == {"zero", "closed", "box"}


# ---- C. -----------------------------------------------------------------------------------------------------------------
def test_cost_without_a_control(V, engines):
    """cost(..., u=None, sparsity=mode): J3 = J4 = 0 and J1, J2 have the bits of the full mode; N = 130, so that the column
    norms (not launched without a control) would take three workgroups."""
    eng, n, rows = engines(130), 131, 22
    rng = np.random.default_rng(11)
    x, t = _grids(rng, n, rows)
    phi, pq = rng.standard_normal((2, BATCH, rows, n))
    pt = rng.standard_normal((BATCH, n))
    opt = V.make_opt(b1=0.7, b2=3.0, b3=0.4, kappa_sparsity=0.25)
    full = eng.cost(phi, None, pq, pt, x, t, opt)
    assert np.all(full[:, 2:4] == 0.0) and np.all(full[:, :2] > 0.0)
    for mode in ("time", "space"):
        # a control first, so that stale column norms are there to be picked up
        eng.cost(phi, rng.standard_normal((BATCH, rows, n)), pq, pt, x, t, opt, sparsity=mode)
        J = eng.cost(phi, None, pq, pt, x, t, opt, sparsity=mode)
        assert np.all(J[:, 2:4] == 0.0) and np.array_equal(J, full), mode
