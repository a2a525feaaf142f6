"""The Krylov calls of the 2D engine (hess_lanczos / krylov_vector, hess_cg / cg_vector / newton_trial, pgd_newton; DESIGN.md
10e, 10g, 10i) with tiles, chunks of levels and batch above one AT THE SAME TIME, and with max_steps above the march.  The
kernels k_kr_*, k_ncg_*, k_nt_trial and k_nt_fin index their partials [B][chunks][tiles] through KR_COORDS;
test_gpu_krylov_2d.py has tiles (9, one chunk, batch 1), chunks (one tile, six, batch 1) and dense (one tile, one chunk,
batch 3), each with max_steps == M, where kr_layout (sized by max_steps) and the launches (sized by M + 1) agree.

Problem `grid`: 128 x 32, Ly 0.5 (plane 33 x 129 = 3 x 3 tiles), steps 1e-2 (0.4 + 1.2 default_rng(5).random(9)) (M = 9, 10
levels, the largest step 3.5 times the smallest), VCH_KR_LCHUNK=4: chunks of levels {0-3, 4-7, 8-9}, the last ragged; every
context has max_steps = M + 7, so kr_layout counts 5 chunks where the calls launch 3.  test_grid_march_meets_the_band_premise
(no GPU) shows with the oracle that the march converges and stays in the interior band of the mass fix.

Free set: 27 uploaded nodes, one per (tile, chunk) pair, on tile corners, tile edges and interior nodes in rotation, on
levels 0, 2, 3, 4, 5, 7, 8, 9; the 27 x 27 block A from one hessvec call of batch 27.  Masks of a batch of three: all 27
nodes, the 18 of chunks 0 and 2, the 9 of tile column 0.

Tolerances, relative to the largest eigenvalue of the member's block.  10 n eps with n = 42570 nodes is 9.8e-11, outside the
project's 1.5e-11 class, so the Ritz values, the Lanczos relation and the basis take 10 x the deviation from the CPU reference
(eigvalsh of the block, Engine2D.hessvec on a second context, the identity matrix) measured on an MI355X, as
test_gpu_krylov_2d.py does for `tiles`; all inside the 1.5e-11 class.  CG: the rule of
test_gpu_hess_cg_2d.test_solve_with_an_uploaded_right_hand_side (true residual <= 1.2e-8, x within cond 1.2e-8 of
np.linalg.solve, steps within one of the restatement on the block at the linear solves' rtol 1e-14 and at the default).
newton_trial as test_gpu_newton_2d.test_trial_kernel_against_numpy: control bitwise, counts exact, sums at n eps.  A member
of a batch against a context of its own: bitwise.

Measured on an MI355X at the default rtol = 1e-12 (free sets of 27 / 18 / 9 nodes):
    Ritz values   all of every member against eigvalsh of its block: 3.51e-14 / 2.91e-14 / 3.50e-14, asserted 3.51e-13
                  (spectra 7.0e-12 .. 4.0e-10, 7.0e-12 .. 4.0e-10, 5.6e-11 .. 2.0e-10)
    relation      k = 6 on member 0: 1.84e-14, orthogonality 4.44e-16, asserted 1.84e-13 and 4.44e-15; step-0 identity 2.6e-26
                  (bound n eps sum|terms| = 1.2e-21)
    CG            steps without / with the preconditioner 21, 14, 8 / 13, 10, 8, the restatement's at rtol 1e-14 and at the
                  default; true residual at most 4.78e-9, error against np.linalg.solve at most 3.58e-9 (cond 56.8, 56.8, 3.56)
    trial         pinned 11 / 8 / 4, clipped 3625 / 11807 / 10831 of 42570 nodes; sums 2.2e-16 relative (bound 9.8e-12)
    rounds        members 0 and 2 accept s = 1 twice (free sets 28479 -> 14073 and 42570 -> 1120), member 1 STATIONARY, IDLE

That the tests can fail (the mutants of test_gpu_hessvec_matrix.py's docstring): with k_hv_emit's alpha, beta taken from the
neighbouring step the Ritz values miss by 1.8e-3, the relation by 2.5e-4 and the CG solution's true residual is 4.4e-2; kp
with c2 = 1 and the cut partial sums pass here (default c2, 9 tiles).  The partial layout itself is guarded by the bitwise
comparisons with single contexts (one chunk count, one batch) and by the dense references."""
import types

import numpy as np
import pytest

from oracle import vch2d_oracle as o
from _cg_ref import CONVERGED, cg
from _lanczos_ref import ritz
from test_gpu_hess_cg_2d import SOLVE, STEPS_RTOL, _mass
from test_gpu_hessvec_2d import EPS
from test_gpu_hessvec_matrix import ragged_steps
from test_gpu_krylov_2d import CLASS, Problem, V, _check_stats, _mask_of, _q0, _relation      # noqa: F401 (fixture)
from test_gpu_newton_2d import ACCEPTED, IDLE, OUT_KEYS, STATIONARY, _pgd, _three
from test_gpu_second_order_matrix import cos_controls

gpu = pytest.mark.gpu

NX, NY, LX, LY, M, BASE, LCHUNK, SPARE = 128, 32, 1.0, 0.5, 9, 1e-2, 4, 7
# measured on an MI355X (the MEASURE lines of this file), relative to lambda_max of the member's block
MEASURED = dict(ritz=3.51e-14, rel=1.84e-14, orth=4.44e-16)
TOL = {k: 10 * v for k, v in MEASURED.items()}
assert max(TOL.values()) <= CLASS


def _inputs():
    dts = ragged_steps(BASE, M)
    t = np.concatenate([[0.0], np.cumsum(dts)])
    P = o.Params2D(Nx=NX, Ny=NY, Lx=LX, Ly=LY, T=float(t[-1]), dt_initial=float(dts.max()))
    x, y = np.linspace(0.0, LX, NX + 1), np.linspace(0.0, LY, NY + 1)
    xx, yy = np.meshgrid(x / LX, y / LY, indexing="ij")
    return P, t, dts, x, y, o.init_phi_random(NX, NY, o.DELTA_SEP, amp=0.1, seed=42), cos_controls(xx, yy, M, 20.0, 1)[0]


def test_grid_march_meets_the_band_premise():
    """With the oracle alone: every Newton call converges in under 20 iterations and |phi_n| + |s| stays inside the interior
    band of the mass fix for n >= 1 (the clip inactive, every node shifted, the shifts at work)."""
    P, t, dts, x, y, phi0, u = _inputs()
    assert len(dts) == M and dts.max() / dts.min() > 3.0
    st = {}
    phi, _, th = o.forward(P, control=u, phi0=phi0, stats=st, dts=dts)
    s = np.array(st["mass_shifts"])
    top = float(np.abs(phi[1:]).max())
    print(f"grid: max|phi[1:]| {top:.3f}, |shifts| {np.abs(s).min():.2e} .. {np.abs(s).max():.2e}, Newton norms recorded "
          f"{[c[0] for c in st['step_counts']]}")
    assert np.array_equal(th, t) and phi.shape[0] == M + 1
    assert all(c[0] < 20 for c in st["step_counts"]) and all(st["mass_shift_interior"])
    assert top < 0.985 - np.abs(s).max() and np.abs(s).min() > 1e-7


def _free_nodes():
    """(flat nodes, their tile column, their chunk): one node per (tile, chunk) pair."""
    ns, nf = NY + 1, NX + 1                                  # the engine's plane: ns rows of nf entries of the flat field
    assert (ns, nf) == (33, 129)
    levels = [(0, 3, 2), (4, 7, 5), (8, 9, 9)]               # per chunk, by tile in rotation
    nodes, tcol, chunk = [], [], []
    for ts in range(3):
        for tf in range(3):
            i = 3 * ts + tf
            rows = [16 * ts, min(16 * ts + 15, ns - 1), min(16 * ts + 7, ns - 1)]
            cols = [64 * tf, min(64 * tf + 31, nf - 1), min(64 * tf + 31, nf - 1)]
            for ch in range(3):
                kind = (i + ch) % 3                           # a tile corner, a tile edge, an interior node
                lvl = levels[ch][i % 3]
                assert ch * LCHUNK <= lvl < min((ch + 1) * LCHUNK, M + 1)
                nodes.append(lvl * ns * nf + rows[kind] * nf + cols[kind])
                tcol.append(tf)
                chunk.append(ch)
    order = np.argsort(nodes)
    nodes, tcol, chunk = np.array(nodes)[order], np.array(tcol)[order], np.array(chunk)[order]
    assert len(set(nodes.tolist())) == 27
    return nodes, tcol, chunk


@pytest.fixture(scope="module")
def grid(V):
    P, t, dts, x, y, phi0, u = _inputs()
    pr = Problem(V, P, t, dts, x, y, phi0, u, V.make_opt(), env=dict(VCH_KR_LCHUNK=LCHUNK), max_steps=M + SPARE)
    assert -(-(pr.max_steps + 1) // LCHUNK) == 5 and -(-(M + 1) // LCHUNK) == 3
    pr.free, tcol, chunk = _free_nodes()
    pr.mask = _mask_of(pr.shape, pr.free)
    pr.A = pr.block(pr.free)
    pr.ev = np.linalg.eigvalsh(pr.A)
    pr.sub = [np.arange(27), np.flatnonzero(chunk != 1), np.flatnonzero(tcol == 0)]      # members' nodes, as indices into free
    assert [len(s) for s in pr.sub] == [27, 18, 9]
    pr.masks = np.stack([_mask_of(pr.shape, pr.free[s]) for s in pr.sub])
    top = float(np.abs(u).max())
    pr.boxes = [(-0.6 * top, 0.8 * top), (-0.3 * top, 0.5 * top), (-0.9 * top, 0.2 * top)]
    pr.opts = [V.make_opt(u_min=lo, u_max=hi) for lo, hi in pr.boxes]
    return pr


# ---------------------------------------------------------------------------------------------------------------------
# 1. Lanczos
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_lanczos_batch_of_three_masks(grid):
    pr = grid
    q0, k = _q0((3,) + pr.shape, 2), 32
    eng = pr.context(3)
    many = eng.hess_lanczos(q0, k, opt=pr.opts, mask=pr.masks, **pr.kw(3))
    Q = np.stack([eng.krylov_vector(np.tile(np.eye(1, j + 1, j), (3, 1))) for j in range(3)])      # q_0, q_1, q_2 of every member
    eng.close()
    _check_stats(many["stats"])
    assert list(many["n_free"]) == [27, 18, 9] and list(many["steps"]) == [27, 18, 9]
    assert Q.shape[2] == M + 1                                        # the march's levels; those up to max_steps are not returned
    worst = 0.0
    for b, sub in enumerate(pr.sub):
        n = len(sub)
        a, bt = many["alpha"][b], many["beta"][b]
        assert np.isfinite(a[:n]).all() and np.isfinite(bt[:n]).all() and np.isnan(a[n:]).all() and np.isnan(bt[n:]).all()
        assert not Q[:, b][:, ~pr.masks[b]].any() and np.abs(Q[:, b]).max() > 0          # masked-off nodes: exact zeros
        ev = np.linalg.eigvalsh(pr.A[np.ix_(sub, sub)])
        theta, _, _ = ritz(a, bt, n)
        dev = np.abs(theta - ev).max() / ev[-1]
        worst = max(worst, dev)
        print(f"MEASURE grid member {b}: all {n} Ritz values against eigvalsh {dev:.2e}; spectrum {ev[0]:.4e} .. {ev[-1]:.4e}")
        one_eng = pr.context(1)
        one = one_eng.hess_lanczos(q0[b], k, opt=pr.opts[b], mask=pr.masks[b], **pr.kw(1))
        one_eng.close()
        for key in ("alpha", "beta", "steps", "n_free"):
            assert np.array_equal(one[key][0], many[key][b], equal_nan=True), (key, b)
    print(f"MEASURE grid: Ritz values, worst member {worst:.2e}")
    assert worst < TOL["ritz"]


@gpu
def test_lanczos_relation_and_basis(grid):
    rel, orth, ident = _relation(grid, 6, grid.mask)
    print(f"MEASURE grid k=6: relation {rel:.2e} orthogonality {orth:.2e} step-0 identity {ident[0]:.2e} (bound {ident[1]:.2e})")
    assert rel < TOL["rel"] and orth < TOL["orth"]
    assert ident[0] <= ident[1]


# ---------------------------------------------------------------------------------------------------------------------
# 2. Newton-CG and the trial
# ---------------------------------------------------------------------------------------------------------------------
CG_KEYS = ("steps", "status", "n_free", "resid", "curv", "pred", "rnorm0")


@gpu
@pytest.mark.parametrize("precond", [False, True])
def test_cg_batch_of_three_masks(grid, precond):
    pr = grid
    b = _q0((3,) + pr.shape, 21)
    Df = _mass(pr).ravel()[pr.free]
    k = 2 * 27
    for rtol in (0.0, STEPS_RTOL):
        eng = pr.context(3)
        R = eng.hess_cg(k, rhs=b, cg_tol=1e-8, precond=precond, mask=pr.masks, opt=pr.opts, rtol=rtol, **pr.kw(3))
        X, Pd = eng.cg_vector("x"), eng.cg_vector("p")
        eng.close()
        _check_stats(R["stats"], rtol or 1e-12)
        assert list(R["n_free"]) == [27, 18, 9] and X.shape[1] == M + 1
        for i, sub in enumerate(pr.sub):
            nodes, blk = pr.free[sub], pr.A[np.ix_(sub, sub)]
            bf = b[i].ravel()[nodes]
            ref = cg(lambda v: blk @ v, np.ones(len(sub), dtype=bool), bf, k, 1e-8, Df[sub] if precond else None)
            ev = np.linalg.eigvalsh(blk)
            cond = ev[-1] / ev[0]
            want = np.linalg.solve(blk, bf)
            m = int(R["steps"][i])
            xf = X[i].ravel()[nodes]
            true = np.linalg.norm(bf - blk @ xf) / np.linalg.norm(bf)
            err = np.abs(xf - want).max() / np.abs(want).max()
            print(f"MEASURE grid cg member {i} precond {precond} rtol {rtol:g}: steps {m} (restatement {ref['steps']}) recurrence "
                  f"{R['resid'][i, m - 1]:.2e} true residual {true:.2e} cond {cond:.3g} error {err:.2e} rnorm0 dev "
                  f"{abs(R['rnorm0'][i] - ref['rnorm0']) / ref['rnorm0']:.1e}")
            assert R["status"][i] == CONVERGED
            assert not X[i][~pr.masks[i]].any() and np.abs(X[i]).max() > 0
            assert R["resid"][i, m - 1] <= 1e-8 and np.isnan(R["resid"][i, m:]).all() and np.isnan(R["curv"][i, m:]).all()
            assert true <= SOLVE
            assert err <= cond * SOLVE
            assert abs(m - ref["steps"]) <= 1
            if rtol == 0.0:
                one_eng = pr.context(1)
                one = one_eng.hess_cg(k, rhs=b[i], cg_tol=1e-8, precond=precond, mask=pr.masks[i], opt=pr.opts[i], **pr.kw(1))
                X1, P1 = one_eng.cg_vector("x")[0], one_eng.cg_vector("p")[0]
                one_eng.close()
                assert one["stats"]["linear_solves"] == pr.M * (2 * m + 1), one["stats"]
                for key in CG_KEYS:
                    assert np.array_equal(one[key][0], R[key][i], equal_nan=True), (key, i)
                assert np.array_equal(X1, X[i]) and np.array_equal(P1, Pd[i]), i


@gpu
def test_trial_kernel_against_numpy(grid):
    pr = grid
    s = np.array([1.0, 0.5, 0.125])
    top = float(np.abs(pr.u).max())
    # a right-hand side whose solution is 32 times the control's size on the free nodes: s x flips signs and leaves the boxes
    b = _q0(pr.shape, 41)
    want = np.linalg.solve(pr.A, b.ravel()[pr.free])
    b *= 32.0 * top / np.median(np.abs(want))
    eng = pr.context(3)
    R = eng.hess_cg(2 * 27, rhs=np.stack([b] * 3), cg_tol=1e-8, mask=pr.masks, opt=pr.opts, **pr.kw(3))
    X = eng.cg_vector("x")
    assert list(R["n_free"]) == [27, 18, 9] and np.abs(X).reshape(3, -1).max(axis=1).min() > top
    T = eng.newton_trial(s)
    after = eng.cg_vector("x")
    eng.close()
    nodes = pr.u.size
    for i, (lo, hi) in enumerate(pr.boxes):
        v = pr.u + s[i] * X[i]
        t = np.clip(v, lo, hi)
        clipped = int((t != v).sum())
        pin = pr.masks[i] & (t * pr.u < 0.0)
        t[pin] = 0.0
        assert pin.sum() >= 1 and clipped >= 1, (i, int(pin.sum()), clipped)          # the expectation itself has both kinds
        d2, n2 = float(np.sum((t - pr.u) ** 2)), float(np.sum(pr.u ** 2))
        print(f"MEASURE grid trial member {i}: s {s[i]} pinned {int(pin.sum())} clipped {clipped} of {nodes}; sums dev "
              f"{abs(T['change'][i, 0] / d2 - 1):.2e} {abs(T['change'][i, 1] / n2 - 1):.2e} (bound {nodes * EPS:.2e})")
        assert np.array_equal(T["u"][i].view(np.int64), t.view(np.int64)), i
        assert T["pinned"][i] == pin.sum() and T["clipped"][i] == clipped
        assert abs(T["change"][i, 0] - d2) <= nodes * EPS * d2 and abs(T["change"][i, 1] - n2) <= nodes * EPS * n2
    assert np.array_equal(after, X)


# ---------------------------------------------------------------------------------------------------------------------
# 3. Newton rounds
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_newton_rounds_batch_of_three(grid):
    """Member 0 of test_gpu_newton_2d._three (about this grid's control scaled into the box of that test), its member 1 (an
    empty free set) and the box-cut start; the free sets are built on the device and cover every tile and chunk."""
    pr, V = grid, grid.V
    K2 = V.module("Vch_control_2D.config")
    uc = np.clip(pr.u * (1.4 / np.abs(pr.u).max()), -0.5, 0.5)
    opts, u0 = _three(types.SimpleNamespace(V=V, ocfg=K2.OptimizationConfig(), u=uc))
    n_rounds, kw = 2, dict(k=8)
    eng = _pgd(pr, opts, u0)
    many = eng.pgd_newton(n_rounds, **kw)
    Um, Pm = eng.pgd_get("u"), eng.pgd_get("phi")
    eng.close()
    print(f"MEASURE grid rounds: status {many['status'].tolist()} s {many['s'].tolist()} halvings {many['halvings'].tolist()} n_free "
          f"{many['n_free'].tolist()} cg {many['cg_status'].tolist()} in {many['cg_steps'].tolist()} cost {many['cost'].tolist()} -> "
          f"{many['cost_new'].tolist()}")
    assert many["status"][1].tolist() == [STATIONARY, IDLE] and many["n_free"][1, 0] == 0 and not Um[1].any()
    assert many["n_free"][2, 0] == pr.u.size
    for r in range(n_rounds):                               # the box-cut start: monotone in cost
        if many["status"][2, r] == ACCEPTED:
            assert many["cost_new"][2, r] < many["cost"][2, r]
        elif np.isfinite(many["cost"][2, r]):
            assert many["cost_new"][2, r] == many["cost"][2, r]
    for i in range(3):
        one = _pgd(pr, [opts[i]], u0[i][None])
        got = one.pgd_newton(n_rounds, **kw)
        U1, P1 = one.pgd_get("u"), one.pgd_get("phi")
        one.close()
        for key in OUT_KEYS:
            assert np.array_equal(got[key][0], many[key][i], equal_nan=True), (key, i)
        assert np.array_equal(U1, Um[i]) and np.array_equal(P1, Pm[i]), i
