"""GPU tests of the 2D MARCH (the path the benchmark times: fused evaluation kernels, reduction-free sweeps, inline dmu,
starting guesses, folded end of step) on every DCT plan of the engine, on rectangular grids and on batches across
GUESS_BMAX, against the CPU oracle run live and against a 512^2 oracle golden (tests/golden/make_golden_plans.py).

Plans (csrc/vch_engine2d.hip, with_plan): an axis of N intervals is transformed by an FFT of length L = 2N on power-of-two
grids -- compile-time lengths 512 (LOGL 9), 1024 (LOGL 10) and 2048 (LOGL 11, a 2048-point image), a run-time length
otherwise (L < 512 in a 1024-point image, L = 4096 in a 4096-point image) -- and by the MFMA GEMM with 64 x 64 tiles on
every other grid.  The grid matrix below puts every plan on each axis with the other axis on a different plan and
hx != hy, so a swapped fast / slow axis quantity in a march kernel changes the result.

A subtly wrong sweep, tail or guess still converges, only with more Newton iterations: the tests pin the Newton, solve
and Armijo counts as well as the fields.  Lengths Lx, Ly are chosen so that the last residual norm of every Newton loop
sits at least 20x below the 1e-6 tolerance (the count is then decided by the arithmetic, not by round-off).

Tolerances as in test_gpu_2d.py: OPS 1e-12, SOLVE 1e-9, MARCH 1e-8.
"""
import contextlib
import os

import numpy as np
import pytest

from conftest import golden, relerr

pytestmark = pytest.mark.gpu

OPS, SOLVE, MARCH = 1e-12, 1e-9, 1e-8
M, DT = 4, 1e-3


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


@pytest.fixture(scope="module")
def O2():
    from oracle import vch2d_oracle
    return vch2d_oracle


@contextlib.contextmanager
def _env(**kv):
    """Set engine switches for the contexts created inside the block, then restore the environment."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _plan(n):
    """The DCT plan of an axis of n intervals, as with_plan picks it."""
    if not (n >= 16 and n & (n - 1) == 0):
        return "gemm"
    logl = (2 * n).bit_length() - 1
    return {9: "L512", 10: "L1024", 11: "L2048"}.get(logl, "L4096" if logl == 12 else "runtime")


#        Nx    Ny    Lx    Ly
GRIDS = [(512, 16, 2.0, 0.25), (16, 512, 0.25, 2.0),
         (256, 32, 1.0, 0.5), (32, 256, 0.3, 1.0),
         (1024, 16, 4.0, 0.25), (16, 1024, 0.25, 4.0),
         (2048, 16, 8.0, 0.25), (16, 2048, 0.25, 8.0),
         (64, 64, 1.0, 0.5),                                  # equal node counts, hx != hy: same plan, different spacing
         (100, 70, 1.3, 0.9), (129, 65, 1.0, 0.5)]            # GEMM: 2 x 2 tiles with tails; 3 x 2 tiles, 2-node tails
FFT_GRIDS = [g for g in GRIDS if _plan(g[0]) != "gemm"]
gid = lambda g: f"{g[0]}x{g[1]}"


def test_grid_matrix_covers_every_plan():
    """Every FFT plan appears on the fast axis (x, Nx) and on the slow axis (y, Ny) with the other axis on another plan."""
    want = {"runtime", "L512", "L1024", "L2048", "L4096"}
    fast = {_plan(g[0]) for g in FFT_GRIDS if _plan(g[0]) != _plan(g[1])}
    slow = {_plan(g[1]) for g in FFT_GRIDS if _plan(g[0]) != _plan(g[1])}
    assert fast == want and slow == want, (fast, slow)
    assert "gemm" in {_plan(g[0]) for g in GRIDS}


def _controls(x, y, Lx, Ly, B, rows, seed=0):
    """A control per trajectory (shape and amplitude of its own, |u| up to ~3 like the line search's), ramped in time."""
    out = []
    for b in range(B):
        k = (b + seed) % 4 + 1
        shape = np.sin(k * np.pi * x / Lx)[:, None] * np.cos((5 - k) * np.pi * y / Ly)[None, :]
        a = (3.0, -2.0, 1.5, -2.5)[(b + seed) % 4] * (1.0 + 0.05 * b)
        out.append(a * np.linspace(0.0, 1.0, rows)[:, None, None] * shape[None])
    return np.stack(out)


def _counts(st):
    return st["newton_iters"], st["linear_solves"], st["armijo_trials"]


def _oracle_march(O2, P, phi0, u):
    """Oracle forward per trajectory; returns histories and the counts summed over the batch."""
    hs, tot = [], {}
    for b in range(phi0.shape[0]):
        st = {}
        h, _, _ = O2.forward(P, control=None if u is None else u[b], phi0=phi0[b], stats=st)
        hs.append(h)
        for k in ("newton_its", "solves", "armijo_trials"):
            tot[k] = tot.get(k, 0) + st[k]
    return np.stack(hs), (tot["newton_its"], tot["solves"], tot["armijo_trials"])


class _Case:
    """Inputs of a grid of the matrix, B = 2 (seeds 42 and 43, controls of their own), and the oracle's answers."""

    def __init__(self, V, O2, g):
        self.Nx, self.Ny, self.Lx, self.Ly = g
        self.P = O2.Params2D(Nx=self.Nx, Ny=self.Ny, Lx=self.Lx, Ly=self.Ly, T=M * DT, dt_initial=DT)
        self.t, self.dts = V.time_grid(M * DT, DT)
        assert len(self.dts) == M
        self.x, self.y = np.linspace(0, self.Lx, self.Nx + 1), np.linspace(0, self.Ly, self.Ny + 1)
        self.phi0 = np.stack([O2.init_phi_random(self.Nx, self.Ny, 1e-2, amp=0.1, seed=s) for s in (42, 43)])
        self.u = _controls(self.x, self.y, self.Lx, self.Ly, 2, M + 1)
        self.ref_nat, self.cnt_nat = _oracle_march(O2, self.P, self.phi0, None)
        self.ref_u, self.cnt_u = _oracle_march(O2, self.P, self.phi0, self.u)
        tg = [O2.build_targets(self.x, self.y, self.t, self.phi0[b], self.Lx, self.Ly, M * DT, 1, 1) for b in range(2)]
        self.phi_T, self.phi_Q = np.stack([a for a, _ in tg]), np.stack([b for _, b in tg])
        self.opt = O2.OptParams()
        self.adj = [O2.backward(self.ref_u[b], self.x, self.y, self.t, self.P, self.opt.b1, self.opt.b2, self.phi_Q[b],
                                self.phi_T[b]) for b in range(2)]

    def engine(self, V, B=2):
        return V.Engine2D(Nx=self.Nx, Ny=self.Ny, Lx=self.Lx, Ly=self.Ly, batch=B, max_steps=M)


def _check_adjoint(O2, c, b, p, q, r):
    """Adjoint sweep of trajectory b against the oracle's.

    Every level p_n must solve the oracle's step equation A(phi_n) p_n = B(phi_n+1) p_n+1 + src to 1e-11 relative residual
    (this pins the operator: a wrong spacing, diagonal or step is an O(1) residual) and q = -L p must agree to SOLVE.  The
    smooth part of p itself, and with it the filter state r, is round-off limited: A = I - tau L + dt/2 L^2 - dt/2 D L has
    eigenvalue 1 on the constant mode and ~1 on the first cosines of a long axis, but up to cond = 1 + tau lam + dt/2 lam^2,
    lam = 4/hx^2 + 4/hy^2 (4e7 on the 3.9e-3-spaced axes here), so a solve whose residual is at round-off relative to
    the right-hand side fixes those modes only to about eps cond.  Two direct solves differ at that level too: on
    16 x 1024 the oracle's SuperLU solution of one step has a true relative residual of 4e-9 for a smooth right-hand
    side.  p gets 20 eps cond (at least SOLVE), r the MARCH class."""
    hx, hy = c.Lx / c.Nx, c.Ly / c.Ny
    pr, qr, rr = c.adj[b]
    ph, pq = c.ref_u[b], c.phi_Q[b]
    term = c.opt.b2 * (ph[M] - c.phi_T[b])                      # (I - tau L) p_M = b2 (phi_M - phi_T)
    assert np.linalg.norm(p[M] - c.P.tau * O2.lap(p[M], hx, hy) - term) < 1e-11 * np.linalg.norm(term)
    for n in range(M):
        dt = c.t[n + 1] - c.t[n]
        rhs = O2.adjoint_B_apply(ph[n + 1], p[n + 1], dt, c.P, hx, hy) + 0.5 * dt * c.opt.b1 * (ph[n] - pq[n] + ph[n + 1] - pq[n + 1])
        res = O2.adjoint_A_apply(ph[n], p[n], dt, c.P, hx, hy) - rhs
        assert np.linalg.norm(res) < 1e-11 * np.linalg.norm(rhs), (b, n, np.linalg.norm(res) / np.linalg.norm(rhs))
    assert relerr(q, qr) < SOLVE, (b, relerr(q, qr))
    lam = 4.0 / hx ** 2 + 4.0 / hy ** 2
    tol_p = max(SOLVE, 20 * np.finfo(float).eps * (1.0 + c.P.tau * lam + 0.5 * DT * lam ** 2))
    assert relerr(p, pr) < tol_p, (b, relerr(p, pr), tol_p)
    assert relerr(r, rr) < MARCH, (b, relerr(r, rr))


_CASES = {}


def _case(V, O2, g):
    if g not in _CASES:
        _CASES[g] = _Case(V, O2, g)
    return _CASES[g]


# ---------------------------------------------------------------------------------------
# A. grid matrix vs the oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GRIDS, ids=gid)
def test_march_adjoint_cost_prox_vs_oracle(V, O2, g):
    """Forward march (no control / per-trajectory controls), adjoint sweep, cost and gradient-prox step of a B = 2 batch
    against the oracle: march fields to SOLVE, the summed Newton / solve / Armijo counts exactly, the adjoint as in
    _check_adjoint, cost to 1e-12 and the prox step to 1e-14."""
    c = _case(V, O2, g)
    e = c.engine(V)
    assert e.uses_fft == (_plan(c.Nx) != "gemm")
    ph, st = e.forward(c.phi0, c.dts)
    for b in range(2):
        assert relerr(ph[b], c.ref_nat[b]) < SOLVE, (b, relerr(ph[b], c.ref_nat[b]), st)
    assert _counts(st) == c.cnt_nat, (st, c.cnt_nat)
    ph_u, st = e.forward(c.phi0, c.dts, u=c.u)
    for b in range(2):
        assert relerr(ph_u[b], c.ref_u[b]) < SOLVE, (b, relerr(ph_u[b], c.ref_u[b]), st)
        # the control moves the state measurably: a march that dropped it would fail the comparison above
        assert np.max(np.abs(c.ref_u[b] - c.ref_nat[b])) > 1e3 * SOLVE * np.max(np.abs(c.ref_u[b]))
    assert _counts(st) == c.cnt_u, (st, c.cnt_u)
    # adjoint sweep on the oracle's controlled history
    p, q, r, st = e.backward(c.ref_u, c.t, c.opt.b1, c.opt.b2, c.phi_Q, c.phi_T)
    for b in range(2):
        _check_adjoint(O2, c, b, p[b], q[b], r[b])
    # cost of the engine's controlled history (both sides see the same input)
    J = e.cost(ph_u, c.u, c.phi_Q, c.phi_T, c.t, c.opt)
    for b in range(2):
        Jr = O2.cost(ph_u[b], c.u[b], c.phi_Q[b], c.phi_T[b], c.x, c.y, c.t, c.opt)
        assert abs(J[b, 4] / Jr - 1) < 1e-12, (b, J[b, 4], Jr)
    # gradient step + soft threshold + box clip, a step length per trajectory
    rr = np.stack([c.adj[b][2] for b in range(2)])
    alpha = np.array([0.5, 50.0])
    un = e.grad_prox(c.u, rr, alpha, c.opt)
    for b in range(2):
        ref = O2.prox_step(c.u[b], O2.gradient(rr[b], c.u[b], c.opt), alpha[b], c.opt)
        assert relerr(un[b], ref) < 1e-14
    e.close()


@pytest.mark.parametrize("g", GRIDS, ids=gid)
def test_batch_member_equals_single_run(V, O2, g):
    """Trajectory 1 of the B = 2 march and sweep is bit for bit its own B = 1 run."""
    c = _case(V, O2, g)
    e2 = c.engine(V)
    ph2, _ = e2.forward(c.phi0, c.dts, u=c.u)
    _, _, r2, _ = e2.backward(None, c.t, c.opt.b1, c.opt.b2, c.phi_Q, c.phi_T, want=("r",))
    e2.close()
    e1 = c.engine(V, B=1)
    ph1, _ = e1.forward(c.phi0[1], c.dts, u=c.u[1])
    _, _, r1, _ = e1.backward(None, c.t, c.opt.b1, c.opt.b2, c.phi_Q[1], c.phi_T[1], want=("r",))
    e1.close()
    assert np.array_equal(ph2[1], ph1), float(np.max(np.abs(ph2[1] - ph1)))
    assert np.array_equal(r2[1], r1), float(np.max(np.abs(r2[1] - r1)))


@pytest.mark.parametrize("g", FFT_GRIDS, ids=gid)
def test_engine_variants_agree(V, O2, g):
    """The fast path against its own switches on every FFT plan: separate evaluation kernels (VCH_FUSED=0) give the same
    arithmetic, bit for bit; CG-form solves (VCH_CHEB=0) and solves started from zero (VCH_GUESS=0) give the same counts
    and fields equal to the solves' tolerance."""
    c = _case(V, O2, g)

    def march(**env):
        with _env(**env):
            e = c.engine(V)
            out = e.forward(c.phi0, c.dts, u=c.u)
            e.close()
        return out
    ph, st = march()
    key = lambda s: _counts(s) + (s["linear_iters"],)
    ph0, st0 = march(VCH_FUSED=0)
    assert np.array_equal(ph, ph0), float(np.max(np.abs(ph - ph0)))
    assert key(st) == key(st0), (st, st0)
    for sw in ("VCH_CHEB", "VCH_GUESS"):
        phs, sts = march(**{sw: 0})
        assert _counts(sts) == _counts(st), (sw, st, sts)
        assert np.max(np.abs(ph - phs)) < 1e-10, (sw, float(np.max(np.abs(ph - phs))))


# The loop's by-products against the oracle's loop.  The oracle solves to other tolerances than the engine, so these are
# measured, not derived: 10x the worst gap seen on the MI355X over the cases of the two tests below (change 3.06e-8 at
# 512 x 16, errors 7.33e-15 in the batch of 33 at 16 x 16; profiles/pgd_byproducts.txt), which is far inside what the same
# tests give the quantities they derive from (the errors from the cost, 1e-7; the change from u, 1e-6).  The errors are
# ratios near 1 that two short iterations barely move, hence the small figure; it is below what a reordered sum may cost
# (nodes x 2^-52), so a change of the reduction order means measuring again.  The derived comparison is
# tests/test_gpu_pgd_byproducts.py.
ERR_TOL, CHANGE_TOL = 7.4e-14, 3.1e-7


def _byproduct_gaps(out, b, r):
    """The largest relative gaps of trajectory b's change / tracking_error / terminal_error to those of the oracle's loop r."""
    return tuple(float(np.max(np.abs(out[k][b] / np.asarray(ref) - 1.0)))
                 for k, ref in (("change", r.changes), ("tracking_error", r.tracking), ("terminal_error", r.terminal)))


@pytest.mark.parametrize("g", [(512, 16, 2.0, 0.25), (16, 512, 0.25, 2.0), (100, 70, 1.3, 0.9)], ids=gid)
def test_pgd_two_iterations_vs_oracle(V, O2, g):
    """Two device-resident PGD iterations (adjoint sweep, prox, optimistic march, line search) per orientation of the
    1024-point plan and on the GEMM path, B = 2, against O2.pgd: equal attempts and step lengths, costs to 1e-7, the
    relative control change to CHANGE_TOL and the tracking / terminal errors to ERR_TOL."""
    Nx, Ny, Lx, Ly = g
    P = O2.Params2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, T=M * DT, dt_initial=DT)
    Op = O2.OptParams()
    t, _ = V.time_grid(M * DT, DT)
    seeds = (42, 43)
    refs = [O2.pgd(P, Op, n_iter=2, seed=s) for s in seeds]
    phi0 = np.stack([O2.init_phi_random(Nx, Ny, 1e-2, amp=0.1, seed=s) for s in seeds])
    e = V.Engine2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, batch=2, max_steps=M)
    J0 = e.pgd_init(phi0, np.stack([r.phi_T for r in refs]), t, V.make_opt(Op), ramp=True, T=M * DT)
    out = e.pgd_iterate(2)
    u = e.pgd_get("u")
    e.close()
    for b, r in enumerate(refs):
        assert abs(J0[b, 4] / r.costs[0] - 1) < 1e-10
        assert list(out["attempts"][b]) == list(r.attempts), (out["attempts"][b], r.attempts)
        assert np.allclose(out["alpha"][b], r.alphas, rtol=1e-12, atol=0), (out["alpha"][b], r.alphas)
        assert np.allclose(out["cost"][b], r.costs[1:], rtol=1e-7, atol=0), (out["cost"][b], r.costs)
        assert relerr(u[b], r.u) < 1e-6
        gc, gq, gt = _byproduct_gaps(out, b, r)
        print(f"MEASURE oracle two_iterations {gid(g)} b {b}: change {gc:.2e} tracking {gq:.2e} terminal {gt:.2e}")
        assert gc < CHANGE_TOL and gq < ERR_TOL and gt < ERR_TOL, (b, gc, gq, gt)


def test_column_pass_width_variants(V, O2):
    """VCH_COLS_C = 2048 / 4096 (4 / 8 columns per workgroup of the 1024-point column pass) on the slow axis of 16 x 512.
    Equal to the default to 1e-13, not bit for bit: at C = 1024 the plan hands the first transform's last pass to the
    spectral multiplier and the second transform in registers (FftRegOk), at C = 2048 / 4096 the multiplied image goes
    through LDS (ScaleEmit).  The operations are the same, but only in the register path may the compiler contract the
    multiplier into the next pass's butterflies.  The counts must be equal."""
    c = _case(V, O2, (16, 512, 0.25, 2.0))
    rng = np.random.default_rng(4)
    v = rng.standard_normal((2, c.Nx + 1, c.Ny + 1))

    def run(**env):
        with _env(**env):
            e = c.engine(V)
            z = e.spectral_solve(7.0, 0.9, 3e-3, v)
            ph, st = e.forward(c.phi0, c.dts, u=c.u)
            e.close()
        return z, ph, st
    z, ph, st = run()
    for w in (2048, 4096):
        zw, phw, stw = run(VCH_COLS_C=w)
        assert relerr(zw, z) < 1e-13, (w, relerr(zw, z))
        assert _counts(stw) == _counts(st), (w, st, stw)
        assert np.max(np.abs(phw - ph)) < 1e-13, (w, float(np.max(np.abs(phw - ph))))


# ---------------------------------------------------------------------------------------
# B. the benched plan at its own size: 512^2 oracle golden
# ---------------------------------------------------------------------------------------
def test_march_512_vs_oracle_golden(V, O2):
    """512^2 (1024-point plans on both axes), 4 steps under a |u| ~ 3 control, B = 2 with trajectory 0 on the golden's
    inputs: every level (::8), full rows and columns at the tile edges (64-node tiles), workgroup boundaries and the last
    node, per-level norms and masses, and the per-step Newton / solve / Armijo counts; the adjoint sweep's r likewise, to MARCH (round-off limited, _check_adjoint)."""
    g = golden("g2d_march_512.npz")
    N, LINES = int(g["Nx"]), g["lines"]
    t, dts = V.time_grid(float(g["T"]), float(g["dt"]))
    assert np.array_equal(t, g["t_hist"]) and len(dts) == M
    phi0 = np.stack([O2.init_phi_random(N, N, 1e-2, amp=float(g["amp"]), seed=s) for s in (int(g["seed"]), 7)])
    x = np.linspace(0, 1, N + 1)
    shape = np.sin(2 * np.pi * x)[:, None] * np.cos(np.pi * x)[None, :]
    ramp = np.linspace(0, 1, M + 1)[:, None, None]
    u = np.stack([float(g["amp_u"]) * ramp * shape[None], -2.0 * ramp * shape.T[None]])
    opt = O2.OptParams()
    phi_T, phi_Q = O2.build_targets(x, x, t, phi0[0], 1.0, 1.0, float(g["T"]), 1, 1)
    e = V.Engine2D(Nx=N, Ny=N, batch=2, max_steps=M)
    ph, st2 = e.forward(phi0, dts, u=u)
    p0 = ph[0]
    _, _, r, _ = e.backward(None, t, opt.b1, opt.b2, np.stack([phi_Q, phi_Q]), np.stack([phi_T, phi_T]), want=("r",))
    r0 = r[0]
    del ph, r
    e.close()
    wts = np.outer(O2.trapz_weights(N + 1), O2.trapz_weights(N + 1)) / (N * N)
    assert relerr(p0[:, ::8, ::8], g["phi_sub"]) < SOLVE
    assert relerr(r0[:, ::8, ::8], g["r_sub"]) < MARCH          # round-off limited by the adjoint step operator, see _check_adjoint
    for k in (1, M):
        assert relerr(p0[k][LINES, :], g[f"phi_rows_{k}"]) < SOLVE and relerr(p0[k][:, LINES], g[f"phi_cols_{k}"]) < SOLVE, k
    for k in (0, M - 1):
        assert relerr(r0[k][LINES, :], g[f"r_rows_{k}"]) < MARCH and relerr(r0[k][:, LINES], g[f"r_cols_{k}"]) < MARCH, k
    assert np.allclose(np.linalg.norm(p0.reshape(M + 1, -1), axis=1), g["phi_norm"], rtol=1e-9, atol=0)
    assert np.allclose(np.sum(wts * p0, axis=(1, 2)), g["phi_mass"], rtol=0, atol=1e-14)       # conserved, ~1e-17
    assert np.allclose(np.linalg.norm(r0.reshape(M + 1, -1), axis=1), g["r_norm"], rtol=MARCH, atol=0)
    # r is a sum of q = -L p levels, whose trapezoid mass vanishes: zero to round-off on both sides
    rmax = np.abs(g["r_sub"]).max()
    assert np.abs(g["r_mass"]).max() < 1e-13 * rmax and np.abs(np.sum(wts * r0, axis=(1, 2))).max() < 1e-13 * rmax
    # per-step counts of trajectory 0: cumulative counts of single-trajectory marches of 1 .. M steps (a march's first k
    # steps do not depend on how many follow), and its single run is bit for bit the batch member
    e1 = V.Engine2D(Nx=N, Ny=N, batch=1, max_steps=M)
    cum = []
    for k in range(1, M + 1):
        phk, st = e1.forward(phi0[0], dts[:k], u=u[0])
        cum.append(_counts(st))
    e1.close()
    assert np.array_equal(phk, p0)
    steps = np.diff(np.array([(0, 0, 0)] + cum), axis=0)
    assert np.array_equal(steps, g["step_counts"]), (steps, g["step_counts"])


# ---------------------------------------------------------------------------------------
# C. batches across GUESS_BMAX
# ---------------------------------------------------------------------------------------
SMALL = [(16, 16, 1.0, 1.0), (32, 16, 1.0, 0.6)]


def _batch_inputs(O2, g, B, rows, seed0):
    Nx, Ny, Lx, Ly = g
    x, y = np.linspace(0, Lx, Nx + 1), np.linspace(0, Ly, Ny + 1)
    phi0 = np.stack([O2.init_phi_random(Nx, Ny, 1e-2, amp=0.1, seed=seed0 + b) for b in range(B)])
    return phi0, _controls(x, y, Lx, Ly, B, rows)


@pytest.mark.parametrize("g", SMALL, ids=gid)
def test_batch_32_members_equal_single_runs(V, O2, g, capfd):
    """B = GUESS_BMAX = 32, the last batch with a guess policy and coefficient row per trajectory: trajectories 0 and 31
    (whose guess orders differ: own start amplitude, a control that switches sign half way) are bit for bit their B = 1
    marches."""
    Nx, Ny, Lx, Ly = g
    Ms = 24
    _, dts = V.time_grid(Ms * DT, DT)
    phi0, u = _batch_inputs(O2, g, 32, Ms + 1, 100)
    phi0[31] = O2.init_phi_random(Nx, Ny, 1e-2, amp=0.6, seed=5)
    u[31] *= np.where(np.arange(Ms + 1) < Ms // 2, 1.0, -1.0)[:, None, None] * 5.0
    e = V.Engine2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, batch=32, max_steps=Ms)
    ph, st = e.forward(phi0, dts, u=u)
    e.close()
    orders = {}
    for b in (0, 31):
        capfd.readouterr()
        with _env(VCH_DEBUG_GUESS=1):
            e1 = V.Engine2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, batch=1, max_steps=Ms)
            ph1, _ = e1.forward(phi0[b], dts, u=u[b])
            e1.close()
        orders[b] = [ln.split("(run")[0] for ln in capfd.readouterr().err.splitlines() if ln.startswith("guess order")]
        assert np.array_equal(ph[b], ph1), (b, float(np.max(np.abs(ph[b] - ph1))))
    assert orders[0] and orders[0] != orders[31], orders          # the two rows of the coefficient table really differ


@pytest.mark.parametrize("B", [33, 40])
@pytest.mark.parametrize("g", SMALL, ids=gid)
def test_batch_beyond_guess_bmax_vs_oracle(V, O2, g, B):
    """Batches above GUESS_BMAX share one guess policy (fed by the worst trajectory) and coefficient row 0: every
    trajectory's march and adjoint sweep still match the oracle to SOLVE, with the summed counts equal."""
    Nx, Ny, Lx, Ly = g
    P = O2.Params2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, T=M * DT, dt_initial=DT)
    t, dts = V.time_grid(M * DT, DT)
    phi0, u = _batch_inputs(O2, g, B, M + 1, 200 + B)
    ref, cnt = _oracle_march(O2, P, phi0, u)
    e = V.Engine2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, batch=B, max_steps=M)
    ph, st = e.forward(phi0, dts, u=u)
    assert _counts(st) == cnt, (st, cnt)
    for b in range(B):
        assert relerr(ph[b], ref[b]) < SOLVE, (b, relerr(ph[b], ref[b]))
    x, y = e.x, e.y
    opt = O2.OptParams()
    tg = [O2.build_targets(x, y, t, phi0[b], Lx, Ly, M * DT, 1, 1) for b in range(B)]
    phi_T, phi_Q = np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])
    p, q, r, _ = e.backward(ref, t, opt.b1, opt.b2, phi_Q, phi_T)
    e.close()
    for b in range(B):
        pr, qr, rr = O2.backward(ref[b], x, y, t, P, opt.b1, opt.b2, phi_Q[b], phi_T[b])
        assert relerr(p[b], pr) < SOLVE and relerr(q[b], qr) < SOLVE and relerr(r[b], rr) < SOLVE, b


@pytest.mark.parametrize("g", SMALL, ids=gid)
def test_pgd_batch_33_vs_oracle(V, O2, g):
    """Two PGD iterations of a 33-trajectory batch (distinct seeds) against O2.pgd per trajectory, the relative control
    change and the tracking / terminal errors included (CHANGE_TOL, ERR_TOL)."""
    Nx, Ny, Lx, Ly = g
    B = 33
    P = O2.Params2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, T=M * DT, dt_initial=DT)
    Op = O2.OptParams()
    t, _ = V.time_grid(M * DT, DT)
    seeds = [300 + b for b in range(B)]
    refs = [O2.pgd(P, Op, n_iter=2, seed=s) for s in seeds]
    phi0 = np.stack([O2.init_phi_random(Nx, Ny, 1e-2, amp=0.1, seed=s) for s in seeds])
    e = V.Engine2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, batch=B, max_steps=M)
    J0 = e.pgd_init(phi0, np.stack([r.phi_T for r in refs]), t, V.make_opt(Op), ramp=True, T=M * DT)
    out = e.pgd_iterate(2)
    e.close()
    for b, r in enumerate(refs):
        assert abs(J0[b, 4] / r.costs[0] - 1) < 1e-10, b
        assert list(out["attempts"][b]) == list(r.attempts), (b, out["attempts"][b], r.attempts)
        assert np.allclose(out["alpha"][b], r.alphas, rtol=1e-12, atol=0), (b, out["alpha"][b], r.alphas)
        assert np.allclose(out["cost"][b], r.costs[1:], rtol=1e-7, atol=0), (b, out["cost"][b], r.costs)
        gc, gq, gt = _byproduct_gaps(out, b, r)
        print(f"MEASURE oracle batch_33 {gid(g)} b {b}: change {gc:.2e} tracking {gq:.2e} terminal {gt:.2e}")
        assert gc < CHANGE_TOL and gq < ERR_TOL and gt < ERR_TOL, (b, gc, gq, gt)
