"""GPU tests of the 1D engine at every cyclic-reduction depth, against the CPU oracle run live.

vch1d_create picks the number of implicit cyclic-reduction (CR) levels `lvl` so that the nr = N // 2^lvl + 1 block
rows of the explicit levels fit the NR_MAX = 1025 rows kept in LDS: lvl 0 for N <= 1024, 1 for 1025 <= N <= 2049,
2 for 2050 <= N <= 4096.  At depth >= 1 the rows of the explicit levels are built in registers (RowAt<SYS, LVL>) and the
implicit levels are back-substituted through global memory; when N is not a multiple of 2^lvl, nodes past the last
explicit row are solved by that loop alone.  The size matrix NS holds every depth, every residue of N mod 2^lvl and the
full-LDS case nr = NR_MAX at each depth (test_size_matrix_covers_every_depth).

Measures (oracle/vch1d_oracle.py):
  * omega = backward_error(rows, x, b): componentwise (Oettli-Prager) backward error, residual in long double.  It does
    not depend on the condition of the system, so one bound OMEGA holds every solve at every N.  OMEGA is set from the
    depth-0 sizes, where the engine matches the reference's goldens, and depths 1 and 2 are held to it.
  * cond = cond_estimate(rows, x, b): Skeel condition, ||x_hat - x|| / ||x|| <= omega cond.  Used only to size
    forward-error tolerances against hp_solve (banded LU + two steps of long double iterative refinement).

Lx = 1 throughout (config 2's spacing at N = 4096).
"""
import functools

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NR_MAX = 1025                       # csrc/vch_kernels1d.h
OMEGA = 8 * EPS                     # backward-error bound of every engine solve: depth 0 measures <= 3.4 eps
M, DT = 8, 1e-3
NS = [2, 3, 24, 511, 512, 513, 1023, 1024, 1025, 1026, 1500, 2047, 2048, 2049, 2050, 2051, 3001, 4093, 4094, 4095,
      4096]
MARCH_NS = [1024, 1025, 2048, 2051, 4095, 4096]
SEEDS = (1000, 1001, 1002)
MARGIN = 20.0                       # every Newton loop's last residual norm <= 1e-6 / MARGIN (test_gpu_plans.py)


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


@pytest.fixture(scope="module")
def O1():
    from oracle import vch1d_oracle
    return vch1d_oracle


def _depth(N):
    """vch1d_create's choice of implicit levels."""
    lvl = 0
    while N // (1 << lvl) + 1 > NR_MAX:
        lvl += 1
    return lvl


def test_size_matrix_covers_every_depth():
    """Every depth 0, 1, 2; at every depth every residue of N mod 2^lvl and the full LDS case nr = NR_MAX; the
    march matrix holds a multiple and a ragged N at every depth."""
    for d in (0, 1, 2):
        at = [N for N in NS if _depth(N) == d]
        assert {N % (1 << d) for N in at} == set(range(1 << d)), (d, at)
        assert any(N // (1 << d) + 1 == NR_MAX for N in at), (d, at)
        ma = [N for N in MARCH_NS if _depth(N) == d]
        assert {N % (1 << d) == 0 for N in ma} == ({True} if d == 0 else {True, False}), (d, ma)
    assert _depth(4096) == 2 and _depth(2049) == 1 and _depth(1024) == 0


def _phis(N):
    """Three states: smooth, uniform random in (-0.9, 0.9), near-separated with |phi| up to 0.98 (the Newton diagonal
    D = tau/dt + 2 c1 / (1 - phi^2) then spans 1.5 ... 38 + tau/dt)."""
    x = np.linspace(0.0, 1.0, N + 1)
    rng = np.random.default_rng(N)
    sep = 0.98 * np.tanh((x - 0.37) / 0.02) * np.tanh((0.81 - x) / 0.03)
    return np.stack([0.6 * np.cos(3 * np.pi * x) + 0.2 * np.sin(7 * np.pi * x), rng.uniform(-0.9, 0.9, N + 1),
                     np.clip(sep, -0.98, 0.98)])


def _rhs(m, seed):
    """Random, smooth cosine, unit spike at the first and at the last entry."""
    rng = np.random.default_rng(seed)
    spike0, spike1 = np.zeros(m), np.zeros(m)
    spike0[0] = spike1[-1] = 1.0
    return [rng.standard_normal(m), np.cos(2 * np.pi * np.arange(m) / m), spike0, spike1]


def _interleave(a, b):
    out = np.empty(2 * a.size)
    out[0::2], out[1::2] = a, b
    return out


class _Solves:
    """Collects omega (engine, LAPACK banded LU) per system and checks the forward error against hp_solve."""

    def __init__(self, O1, N):
        self.O1, self.N = O1, N
        self.w, self.w_lu, self.fwd = {}, {}, {}

    def check(self, name, rows, x, b):
        from scipy.linalg import solve_banded
        O1 = self.O1
        k = (len(rows) - 1) // 2
        w = O1.backward_error(rows, x, b)
        w_lu = O1.backward_error(rows, solve_banded((k, k), O1._rows_to_banded(rows), b), b)
        x_hp = O1.hp_solve(rows, b)
        tol = max(1e-13, 20 * EPS * O1.cond_estimate(rows, x_hp, b))
        fe = relerr(x, x_hp)
        self.w[name] = max(self.w.get(name, 0.0), w)
        self.w_lu[name] = max(self.w_lu.get(name, 0.0), w_lu)
        self.fwd[name] = max(self.fwd.get(name, 0.0), fe / tol)
        assert fe <= tol, (name, self.N, fe, tol)


# ---------------------------------------------------------------------------------------
# A. stand-alone solves at every N
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_solves_every_depth_vs_hp_reference(V, O1, N):
    """jacobian_solve, adjoint_solve(phi, dt) and adjoint_solve(None, 0) of a B = 3 batch (three states), dt 1e-3 and
    5e-2, four right-hand sides: omega <= OMEGA, forward error against hp_solve <= 20 eps cond (floor 1e-13), and
    trajectory 1 bit for bit its own B = 1 solve."""
    n, h = N + 1, 1.0 / N
    P = O1.Params1D(N=N)
    phi = _phis(N)
    e3, e1 = V.Engine1D(N=N, batch=3), V.Engine1D(N=N, batch=1)
    S = _Solves(O1, N)
    rn, ra = _rhs(2 * n, 7 * N), _rhs(n, 7 * N + 1)
    for j in range(4):
        r0, r1 = rn[j][0::2].copy(), rn[j][1::2].copy()
        if j >= 2:                                   # spikes at node 0 / node n-1 in both equations
            r0[:] = r1[:] = 0.0
            r0[-(j - 2)] = r1[-(j - 2)] = 1.0
        R0, R1, RA = np.stack([r0] * 3), np.stack([r1] * 3), np.stack([ra[j]] * 3)
        for dt in (1e-3, 5e-2):
            dphi, dmu = e3.jacobian_solve(phi, dt, R0, R1)
            p = e3.adjoint_solve(phi, dt, RA)
            for b in range(3):
                S.check("newton", O1.newton_rows(phi[b], dt, P, h), _interleave(dphi[b], dmu[b]), _interleave(r0, r1))
                S.check("adjoint", O1.adjoint_rows(phi[b], dt, h), p[b], ra[j])
            d1, m1 = e1.jacobian_solve(phi[1], dt, r0, r1)
            assert np.array_equal(d1, dphi[1]) and np.array_equal(m1, dmu[1]), (N, dt, j)
            assert np.array_equal(e1.adjoint_solve(phi[1], dt, ra[j]), p[1]), (N, dt, j)
        pt = e3.adjoint_solve(None, 0.0, RA)
        for b in range(3):
            S.check("terminal", O1.adjoint_rows(None, 0.0, h, n=n), pt[b], ra[j])
        assert np.array_equal(e1.adjoint_solve(None, 0.0, ra[j]), pt[1])
    e3.close()
    e1.close()
    print("\nomega/eps N=%d depth=%d " % (N, _depth(N)) +
          " ".join(f"{k}: engine {S.w[k] / EPS:.3g} LU {S.w_lu[k] / EPS:.3g} fwd/tol {S.fwd[k]:.2g}" for k in S.w))
    for k, w in S.w.items():
        assert w <= OMEGA, (k, N, w / EPS)


# ---------------------------------------------------------------------------------------
# B. march, C. adjoint sweep
# ---------------------------------------------------------------------------------------
def _ic(N, seed, amp=0.5, K=12):
    """Band-limited random state: the first K cosines with coefficients falling as 1/k, scaled to max |phi| = amp.
    (White noise at h = 1/4096 puts Newton on its round-off floor, where the counts are decided by round-off.)"""
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 1.0, N + 1)
    c = rng.standard_normal(K) / np.arange(1, K + 1)
    f = np.cos(np.pi * np.outer(np.arange(1, K + 1), x)).T @ c
    return amp * f / np.max(np.abs(f))


def _controls(N, rows):
    """Ramped controls, |u| <= 1, a shape per trajectory; trajectory 2's switches sign half way."""
    x = np.linspace(0.0, 1.0, N + 1)
    ramp = np.linspace(0.0, 1.0, rows)[:, None]
    sign = np.where(np.arange(rows) < rows // 2, 1.0, -1.0)[:, None]
    return np.stack([ramp * np.cos(np.pi * x)[None], -0.8 * ramp * np.sin(2 * np.pi * x)[None],
                     sign * ramp * np.cos(3 * np.pi * x)[None]])


def _margin_ok(st):
    """The input window of the count comparisons: every Newton loop ends >= MARGIN below the tolerance, none through
    the line-search-failure return."""
    worst = 1e-6 / max(st["last_norms"])
    assert worst >= MARGIN and st["failed_ls"] == 0, (worst, st["failed_ls"])
    return worst


@functools.lru_cache(maxsize=None)
def _march_case(N):
    from oracle import vch1d_oracle as O1
    P = O1.Params1D(N=N, T=M * DT, dt_initial=DT)
    phi0 = np.stack([_ic(N, s) for s in SEEDS])
    u = _controls(N, M + 2)
    out = dict(P=P, phi0=phi0, ctl=u)
    for tag, uu in (("nat", None), ("u", u)):
        hs, st = [], {}
        for b in range(3):
            ph, x, t = O1.forward(P, control=None if uu is None else uu[b], initial_phi=phi0[b], solver="banded",
                                  stats=st)
            hs.append(ph)
        out[tag] = (np.stack(hs), st)
    out["x"], out["t"] = x, t
    # the step matrix's Skeel condition (x = 1, b = 0), worst over the initial states
    out["cond_J"] = max(O1.cond_estimate(O1.newton_rows(phi0[b], DT, P, 1.0 / N), np.ones(2 * N + 2),
                                         np.zeros(2 * N + 2)) for b in range(3))
    tg = [O1.build_targets(x, t, phi0[b], 1.0, M * DT, 1, 1) for b in range(3)]
    out["phi_T"], out["phi_Q"] = np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])
    return out


def _counts(st):
    return st["newton_iters"], st["linear_solves"], st["armijo_trials"], st["linear_iters"]


@pytest.mark.parametrize("N", MARCH_NS)
def test_march_every_depth_vs_oracle(V, O1, N):
    """M = 8 steps of dt = 1e-3, B = 3, band-limited initial states, without control and with ramped controls, against
    O1.forward(solver="banded"): the summed Newton / solve / Armijo counts equal, no line-search failure on either
    side, fields to max(1e-9, 20 eps cond(J)).  Every Newton correction is a solve with backward error <= OMEGA on
    the engine's side and a few eps on the oracle's (banded LU), so the corrections, and with the counts equal the
    iterates, differ by <= (OMEGA + eps) cond(J) relative, cond(J) the Skeel condition of the step matrix; the last
    correction of each step is >= 20x below the tolerance, and the march is dissipative, so the differences do not
    grow over the 8 steps.  At depths 1 and 2 trajectory 1 is bit for bit its own B = 1 run."""
    c = _march_case(N)
    tol = max(1e-9, 20 * EPS * c["cond_J"])
    e = V.Engine1D(N=N, batch=3, max_steps=M)
    dts = np.diff(c["t"])[1:]
    assert dts.size == M
    for tag, u in (("nat", None), ("u", c["ctl"])):
        ref, st_ref = c[tag]
        margin = _margin_ok(st_ref)
        ph, st = e.forward(c["phi0"], dts, u=u)
        cnt_ref = (st_ref["newton_its"], st_ref["solves"], st_ref["armijo_trials"], st_ref["failed_ls"])
        assert _counts(st) == cnt_ref, (tag, st, cnt_ref)
        errs = [relerr(ph[b], ref[b]) for b in range(3)]
        print(f"\nmarch N={N} {tag}: margin {margin:.0f} relerr {max(errs):.2e} tol {tol:.2e}")
        assert max(errs) < tol, (tag, errs, tol)
        if tag == "u":                               # the control moves the state measurably
            assert min(relerr(ref[b], c["nat"][0][b]) for b in range(3)) > 100 * tol
    e.close()
    if _depth(N) >= 1:
        e1 = V.Engine1D(N=N, batch=1, max_steps=M)
        ph1, _ = e1.forward(c["phi0"][1], dts, u=c["ctl"][1])
        assert np.array_equal(ph1, ph[1])
        e1.close()


@pytest.mark.parametrize("N", MARCH_NS)
def test_adjoint_sweep_every_depth_vs_oracle(V, O1, N):
    """The adjoint sweep on the oracle's controlled histories (B = 3, targets from build_targets, and without targets):
    every level's p_k has omega <= OMEGA in the oracle's step equation adjoint_rows(phi_k, dt) p_k =
    B(phi_k+1) p_k+1 + src, the right-hand side formed from the engine's own p_k+1 in long double; the terminal level
    likewise in (I - tau L) p_M = b2 (phi_M - phi_T); q = -L p to 4 eps (componentwise); row 0 of p and r is zero
    (B1:110).  p and r against the oracle's banded sweep: each level's solve is within OMEGA cond_k of its exact
    solution (cond_k its Skeel condition), so p and its filtered Laplacian r get max(1e-9, 20 eps max_k cond_k).
    At depths 1 and 2 trajectory 1's sweep is bit for bit its own B = 1 sweep."""
    c = _march_case(N)
    n, h = N + 1, 1.0 / N
    ref, _ = c["u"]
    t = c["t"]
    opt = O1.OptParams1D()
    e = V.Engine1D(N=N, batch=3, max_steps=M)
    Lrows = O1._lap_rows(n, h)
    for targets in (True, False):
        pq, pt = (c["phi_Q"], c["phi_T"]) if targets else (None, None)
        b1, b2 = (opt.b1, opt.b2) if targets else (1.3, 0.7)
        p, q, r = e.backward(ref, t, b1, b2, pq, pt)
        for b in range(3):
            phQ = np.zeros_like(ref[b]) if pq is None else pq[b]
            phT = np.zeros(n) if pt is None else pt[b]
            last = M + 1
            term = b2 * (np.asarray(ref[b][last], np.longdouble) - np.asarray(phT, np.longdouble))
            ws = [O1.backward_error(O1.adjoint_rows(None, 0.0, h, n=n), p[b][last], term)]
            conds = []
            for k in range(last - 1, 0, -1):
                dt = t[k + 1] - t[k]
                Bp, Bs = O1._residual_ld(O1.adjoint_rhs_rows(ref[b][k + 1], dt, h), p[b][k + 1], np.zeros(n))
                f0 = np.asarray(ref[b][k], np.longdouble) - np.asarray(phQ[k], np.longdouble)
                f1 = np.asarray(ref[b][k + 1], np.longdouble) - np.asarray(phQ[k + 1], np.longdouble)
                src = np.longdouble(0.5 * dt * b1) * (f0 + f1)
                rhs = src - Bp
                A = O1.adjoint_rows(ref[b][k], dt, h)
                ws.append(O1.backward_error(A, p[b][k], rhs, f=Bs + np.abs(src)))
                conds.append(O1.cond_estimate(A, p[b][k], rhs.astype(np.float64)))
            assert max(ws) <= OMEGA, (N, targets, b, [w / EPS for w in ws])
            assert max(O1.backward_error(Lrows, p[b][k], -q[b][k]) for k in range(last + 1)) <= 4 * EPS
            assert not p[b][0].any() and not r[b][0].any()
            pr, qr, rr = O1.backward(ref[b], c["x"], t, b1, b2, pq[b] if targets else None,
                                     pt[b] if targets else None, solver="banded")
            tol = max(1e-9, 20 * EPS * max(conds))
            print(f"\nadjoint N={N} targets={targets} b={b}: omega/eps {max(ws) / EPS:.3g} relerr p {relerr(p[b], pr):.2e} "
                  f"r {relerr(r[b], rr):.2e} tol {tol:.2e}")
            assert relerr(p[b], pr) < tol and relerr(r[b], rr) < tol, (relerr(p[b], pr), relerr(r[b], rr), tol)
        if targets and _depth(N) >= 1:
            e1 = V.Engine1D(N=N, batch=1, max_steps=M)
            _, _, r1 = e1.backward(ref[1], t, b1, b2, pq[1], pt[1])
            e1.close()
            assert np.array_equal(r1, r[1])
    e.close()


# ---------------------------------------------------------------------------------------
# D. device-resident PGD at depth 2 with a ragged tail
# ---------------------------------------------------------------------------------------
def test_pgd_resident_depth2_ragged_vs_oracle(V, O1):
    """N = 4095 (depth 2, three nodes past the last explicit row), T = 8e-3, B = 3, the initial states of B: pgd_init and
    three iterations against O1.pgd(solver="banded", initial_phi=...) per trajectory.  alpha_max = 300 makes the line
    searches differ: in the second iteration trajectory 2 backtracks while 0 and 1 have accepted, so k1d_forward's
    skip path runs at depth 2 with live and skipped workgroups.  Every march of the oracle's loops keeps the Newton
    margin.  Trials equal, alpha to 1e-12, costs to 1e-9.  The final control: the prox step and the clip are
    1-Lipschitz, so an iteration moves the control difference by at most alpha |dr| + alpha b3 |du|, alpha <= 300,
    b3 = 0.0019; r is round-off limited at N = 4095 (section C: two backward-stable sweeps differ by ~1e-5 relative),
    so u gets 8 alpha_max max|dr| over its size, dr the last sweep's measured difference."""
    N, T = 4095, M * DT
    P = O1.Params1D(N=N, T=T, dt_initial=DT)
    Op = O1.OptParams1D(alpha_max=300.0)
    phi0 = np.stack([_ic(N, s) for s in SEEDS])
    st = {}
    refs = [O1.pgd(P, Op, n_iter=3, solver="banded", initial_phi=phi0[b], stats=st) for b in range(3)]
    margin = _margin_ok(st)
    assert any(len({r.trials[k] for r in refs}) > 1 for k in range(3)), [r.trials for r in refs]
    t = refs[0].t_hist
    e = V.Engine1D(N=N, batch=3, max_steps=M)
    J0 = e.pgd_init(phi0, np.stack([r.phi_T for r in refs]), t, np.diff(t)[1:], V.make_opt(Op))
    out = e.pgd_iterate(3)
    u, r_eng = e.pgd_get("u"), e.pgd_get("r")
    e.close()
    for b, r in enumerate(refs):
        assert abs(J0[b, 4] / r.costs[0] - 1) < 1e-9, b
        assert list(out["trials"][b]) == list(r.trials), (b, out["trials"][b], r.trials)
        assert np.allclose(out["alpha"][b], r.alphas, rtol=1e-12, atol=0), (b, out["alpha"][b], r.alphas)
        assert np.allclose(out["cost"][b], r.costs[1:], rtol=1e-9, atol=0), (b, out["cost"][b], r.costs)
        tol_u = max(1e-12, 8 * Op.alpha_max * np.max(np.abs(r_eng[b] - r.r)) / np.max(np.abs(r.u)))
        print(f"\npgd b={b}: margin {margin:.0f} trials {r.trials} relerr u {relerr(u[b], r.u):.2e} tol {tol_u:.2e}")
        assert relerr(r_eng[b], r.r) < 1e-4 and relerr(u[b], r.u) < tol_u, (b, relerr(r_eng[b], r.r), relerr(u[b], r.u))
