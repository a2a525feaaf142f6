"""The Krylov calls of the 1D engine (hess_lanczos / krylov_vector, hess_cg / cg_vector / newton_trial, pgd_newton; DESIGN.md
10f, 10h, 10j) on many streaming chunks, batch above one and max_steps above the march AT THE SAME TIME.  The streaming
kernels run on the grid (chunks of KR1_CHUNK = 4096 nodes of a trajectory's history, B); k1d_kr_fin, k1d_ncg_fin and
k1d_nt_fin add a trajectory's partials with kr1_sum (or its copies), whose loop strides over the chunks by KR1_T = 256
threads: chunks 256 and above are read by its second pass alone.  test_gpu_krylov_1d.py, test_gpu_hess_cg_1d.py and
test_gpu_newton_1d.py have at most 3 chunks and max_steps 8 >= M.

Problem `many_chunks`: N = 4096, M = 255 uniform steps of 1e-3, so 257 rows x 4097 nodes = 258 chunks; chunk 256 holds
nodes of row M (coupled to the march) and of the last row, chunk 257 last-row nodes only.  Batch 3, max_steps = M + 7,
uploaded masks: member 0 has 12 nodes (chunks 0, 1, 40, 128, 200, 255, 256, 257; one interior and one end node of the last
row, whose entries are b3 wt wx alone: two equal ones would end Lanczos early), member 1 eight of them (chunk 256
included), member 2 five (none beyond chunk 255).  The 12 x 12 block A comes from one hessvec call of batch 12 about the
shared base; test_chunk_arithmetic (no GPU) pins the chunk of every node, test_gpu_hessvec_levels_1d.py the march's premise.

Problem `grid`: N = 2050 (depth 2, residue 2), T = 0.115, dt = 0.01: 12 steps, the last of 0.005; 14 rows x 2051 nodes =
8 chunks, the last of 42 nodes; max_steps = M + 7.  Two pgd_newton rounds on the three members of test_gpu_newton_1d._three
(accepting, empty free set, box cut), the start of the host loop (init_phi_random, amp 0.01, seed 42).

Tolerances.  Ritz values: 10 x the deviation from eigvalsh of the member's block measured on an MI355X (MEASURED), kept by
the assertion at import at or below the hv tolerance of depth 2 in test_gpu_hessvec_1d.TOL: Lanczos on a 12-node block
cannot legitimately be further from hessvec's block than hessvec is from the truth.  The Lanczos relation and the basis:
10 n eps lambda_max with n = 257 x 4097 nodes (derived, not measured).  CG: SOLVE of test_gpu_hess_cg_1d.py (true residual
on the block, the error against np.linalg.solve within cond SOLVE) and its step rule against tests/_cg_ref.cg.  The trial:
the control bitwise NumPy's, the counts exact, the sums at n eps.  Rounds: member 0 against GD_1D.newton_refine under
test_gpu_newton_1d.TOL with status, s and n_free equal.  A member of a batch against a context of its own: bitwise.

Measured on an MI355X:
    Ritz values   all of every member against eigvalsh of its block: 7.42e-16 / 1.70e-15 / 1.61e-15, asserted 1.8e-14
                  (spectra 4.3e-14 .. 2.6e-11, 5.0e-14 .. 2.5e-11, 7.1e-13 .. 2.6e-11)
    relation      k = 6 on member 0: 2.16e-16, orthogonality 2.22e-16 (bound 2.3e-9)
    CG            steps without / with D 10, 7, 5 / 7, 5, 5, the restatement's on the block; true residual at most 2.2e-9,
                  error against np.linalg.solve at most 4.2e-11 (cond 606, 496, 36.9)
    trial         pinned 8 / 4 / 3, clipped 392819 / 612321 / 528498 of 1052929 nodes; sums 6.7e-16 relative at most
    rounds        member 0 accepts s = 1 twice (free sets 21276 and 9605, 50 and 3 CG steps), member 1 STATIONARY, IDLE, the
                  box-cut member accepts s = 1/32 after 5 halvings, then STATIONARY; member 0 equals the host loop bitwise

That the tests can fail (the mutants of test_gpu_hessvec_levels_1d.py's docstring): with kr1_sum and its two copies cut to
the first KR1_T partials the four many_chunks tests fail (Ritz values 32, relation 2.6e-2, CG at its limit of 48 steps with
a true residual of 6.9e-4, the trial's pinned count 6 for 8) and the grid rounds pass (8 chunks); with cr_solve<2> wrong at
node n - 2 the Lanczos and CG tests fail (N = 4096 is even: Ritz values 7.9e-1) while the trial and the rounds, which compare
the device with itself and with a host loop that drives the same solve, pass; the back-update mutant passes here (uniform
steps, and the Krylov kernels' own sweeps are not k1d_hessvec)."""
import numpy as np
import pytest

from oracle import vch1d_oracle as o
from _cg_ref import CONVERGED
from _lanczos_ref import ritz
from test_gpu_hess_cg_1d import KEYS as CG_KEYS, SOLVE, _cg, _check_steps, _ref
from test_gpu_hessvec_1d import TOL as HV_TOL
from test_gpu_krylov_1d import Problem, _mask_of, _q0, _tile
from test_gpu_newton_1d import ACCEPTED, IDLE, OUT_KEYS, STATIONARY, TOL as NEWTON_TOL, _pgd, _refine_case, _three
from test_gpu_second_order_1d import V, _engine  # noqa: F401  (V: fixture)

gpu = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KR1_T, KR1_CHUNK = 256, 4096                       # csrc/vch_kernels1d.h
SPARE = 7
NC, MC, DTC = 4096, 255, 1e-3                      # many_chunks
NG, TG, DTG = 2050, 0.115, 0.01                    # grid
# (row, node) of member 0; members 1 and 2 take the nodes of SUB1 and SUB2
AT = [(0, 0), (0, NC // 3), (1, 5), (40, 2000), (128, 1), (200, 3000), (254, NC), (255, 100), (255, 4000), (255, NC),
      (256, 3900), (256, NC)]
SUB1 = [(0, 0), (1, 5), (128, 1), (200, 3000), (254, NC), (255, 100), (255, 4000), (256, NC)]
SUB2 = [(0, NC // 3), (40, 2000), (128, 1), (200, 3000), (255, 100)]

# measured on an MI355X (the MEASURE lines of this file): all Ritz values of every member against eigvalsh of its block,
# relative to lambda_max of the block (members 7.42e-16, 1.70e-15, 1.61e-15); asserted at 10 x that, rounded up
MEASURED = dict(ritz=1.70e-15)
TOL = dict(ritz=1.8e-14)
assert 10 * MEASURED["ritz"] <= TOL["ritz"] <= HV_TOL[2][1]


def many_chunks_inputs():
    """(P, t_hist, dts, x, phi0, u): N = 4096, 255 steps of 1e-3; the start 0.2 cos(pi x), the driver's control of
    amplitude 1.4 clipped to [-1, 1]."""
    dts = np.full(MC, DTC)
    t = np.concatenate([[0.0, 0.0], np.cumsum(dts)])
    P = o.Params1D(N=NC, T=float(t[-1]), dt_initial=DTC)
    x = np.linspace(0.0, P.Lx, NC + 1)
    rows = MC + 2
    u = np.clip(np.stack([1.4 * np.cos(np.pi * x * (1 + k % 3)) * np.sin(1 + k) for k in range(rows)]), -1.0, 1.0)
    return P, t, dts, x, 0.2 * np.cos(np.pi * x), u


def _chunks(rows, n):
    return -(-rows * n // KR1_CHUNK)                # kr1_chunks of vch_engine1d.hip


def _flat(at, n):
    return np.array([r * n + i for r, i in at])


def test_chunk_arithmetic():
    """258 chunks at N = 4096 and M = 255, two of them beyond the first pass of kr1_sum; every node of the members where the
    module docstring puts it.  The grid problem: 12 steps, 8 chunks, the last of 42 nodes."""
    n, rows = NC + 1, MC + 2
    assert (rows, n) == (257, 4097) and _chunks(rows, n) == 258 > 256 == KR1_T
    f = _flat(AT, n)
    assert len(set(f.tolist())) == 12 and f.max() < rows * n
    chunk = f // KR1_CHUNK
    assert chunk.tolist() == [0, 0, 1, 40, 128, 200, 255, 255, 256, 256, 257, 257]
    rows_of = f // n
    assert rows_of[chunk == 256].tolist() == [MC, MC] and (rows_of[chunk == 257] == MC + 1).all()
    assert 256 * KR1_CHUNK // n == MC and (256 * KR1_CHUNK) % n > 0 and 257 * KR1_CHUNK // n == MC + 1
    assert sum(1 for r, i in AT if r == MC + 1) == 2 and {i for r, i in AT if r == MC + 1} == {3900, NC}
    assert set(SUB1) < set(AT) and set(SUB2) < set(AT) and len(SUB1) == 8 and len(SUB2) == 5
    assert 256 in _flat(SUB1, n) // KR1_CHUNK and (_flat(SUB2, n) // KR1_CHUNK).max() == 255
    from oracle.vch2d_oracle import time_grid
    _, dts = time_grid(TG, DTG)
    rows, n = len(dts) + 2, NG + 1
    assert len(dts) == 12 and dts[-1] < dts[0] and _chunks(rows, n) == 8 and rows * n - 7 * KR1_CHUNK == 42
    assert NG // 4 + 1 <= 1025 < NG // 2 + 1 and NG % 4 == 2           # depth 2, residue 2


# ---------------------------------------------------------------------------------------------------------------------
# many_chunks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(V):
    P, t, dts, x, phi0, u = many_chunks_inputs()
    one = _engine(V, P, 1, max_steps=MC + SPARE)
    phi = one.forward(phi0, dts, u=u)[0]
    one.close()
    assert np.abs(phi).max() < 1.0 - o.DELTA_SEP - 0.1
    pr = Problem(V, P, t, dts, x, phi, u, V.make_opt(), max_steps=MC + SPARE)
    n = P.N + 1
    pr.free = np.sort(_flat(AT, n))
    pr.mask = _mask_of(pr.shape, pr.free)
    pr.A = pr.block(pr.free)
    pr.ev = np.linalg.eigvalsh(pr.A)
    pos = {f: j for j, f in enumerate(pr.free.tolist())}
    pr.sub = [np.arange(12), np.array(sorted(pos[f] for f in _flat(SUB1, n))), np.array(sorted(pos[f] for f in _flat(SUB2, n)))]
    pr.masks = np.stack([_mask_of(pr.shape, pr.free[s]) for s in pr.sub])
    pr.boxes = [(-0.6, 0.8), (-0.3, 0.5), (-0.9, 0.2)]
    pr.opts = [V.make_opt(u_min=lo, u_max=hi) for lo, hi in pr.boxes]
    return pr


@gpu
def test_lanczos_batch_of_three_masks(many):
    pr = many
    q0, k = _q0((3,) + pr.shape, 2), 17
    eng = pr.context(3)
    R = eng.hess_lanczos(q0, k, pr.t, pr.opts, mask=pr.masks, **pr.kw(3))
    eng.close()
    assert list(R["n_free"]) == [12, 8, 5] and list(R["steps"]) == [12, 8, 5]
    worst = 0.0
    for b, sub in enumerate(pr.sub):
        m = len(sub)
        a, bt = R["alpha"][b], R["beta"][b]
        assert np.isfinite(a[:m]).all() and np.isfinite(bt[:m]).all() and np.isnan(a[m:]).all() and np.isnan(bt[m:]).all()
        ev = np.linalg.eigvalsh(pr.A[np.ix_(sub, sub)])
        assert np.diff(ev).min() > 0.0
        theta, _, _ = ritz(a, bt, m)
        dev = np.abs(theta - ev).max() / ev[-1]
        worst = max(worst, dev)
        print(f"MEASURE many_chunks member {b}: all {m} Ritz values against eigvalsh {dev:.2e}; spectrum {ev[0]:.4e} .. {ev[-1]:.4e}")
        one_eng = pr.context(1)
        one = one_eng.hess_lanczos(q0[b], k, pr.t, pr.opts[b], mask=pr.masks[b], **pr.kw())
        one_eng.close()
        for key in ("alpha", "beta", "steps", "n_free"):
            assert np.array_equal(one[key][0], R[key][b], equal_nan=True), (key, b)
    print(f"MEASURE many_chunks: Ritz values, worst member {worst:.2e}")
    assert worst < TOL["ritz"]


@gpu
def test_lanczos_relation_and_basis(many):
    pr, k = many, 6
    eng = pr.context(1)
    R = pr.lanczos(eng, _q0(pr.shape, 3), k, mask=pr.mask)
    assert R["steps"][0] == k
    Q = np.stack([eng.krylov_vector(np.eye(1, j + 1, j))[0] for j in range(k + 1)])
    eng.close()
    assert Q.shape[1] == MC + 2                      # the march's rows; those up to max_steps are not returned
    HQ = pr.hessvec(Q[:k])
    a, b, lam = R["alpha"][0], R["beta"][0], pr.ev[-1]
    assert not Q[:, ~pr.mask].any()
    rel = 0.0
    for j in range(k):
        r = np.where(pr.mask, HQ[j], 0.0) - a[j] * Q[j] - b[j] * Q[j + 1] - (b[j - 1] * Q[j - 1] if j else 0.0)
        rel = max(rel, np.abs(r).max() / lam)
    Qf = Q.reshape(k + 1, -1)
    orth = np.abs(Qf @ Qf.T - np.eye(k + 1)).max()
    bound = 10 * Qf.shape[1] * EPS
    print(f"MEASURE many_chunks k=6: relation {rel:.2e} orthogonality {orth:.2e} (bound {bound:.2e})")
    assert rel < bound and orth < bound


@gpu
@pytest.mark.parametrize("precond", [False, True])
def test_cg_batch_of_three_masks(many, precond):
    pr = many
    b = _q0((3,) + pr.shape, 21)
    k = 4 * 12
    eng = pr.context(3)
    R = _cg(pr, eng, k, nb=3, rhs=b, cg_tol=1e-8, precond=precond, mask=pr.masks, opt=pr.opts)
    X, Pd = eng.cg_vector("x"), eng.cg_vector("p")
    eng.close()
    assert list(R["n_free"]) == [12, 8, 5] and X.shape[1] == MC + 2
    for i, sub in enumerate(pr.sub):
        nodes, blk = pr.free[sub], pr.A[np.ix_(sub, sub)]
        bf = b[i].ravel()[nodes]
        cond = np.linalg.cond(blk)
        want = np.linalg.solve(blk, bf)
        m = int(R["steps"][i])
        xf = X[i].ravel()[nodes]
        true = np.linalg.norm(bf - blk @ xf) / np.linalg.norm(bf)
        err = np.abs(xf - want).max() / np.abs(want).max()
        print(f"MEASURE many_chunks cg member {i} precond {precond}: steps {m} true residual {true:.2e} cond {cond:.3g} error {err:.2e}")
        assert R["status"][i] == CONVERGED
        assert not X[i][~pr.masks[i]].any() and np.abs(X[i]).max() > 0
        assert true <= SOLVE
        assert err <= cond * SOLVE
        _check_steps(pr, blk, nodes, b[i], k, 1e-8, precond, m, _ref(pr, blk, nodes, b[i], k, 1e-8, precond),
                     f"many_chunks member {i} precond {precond}")
        one_eng = pr.context(1)
        one = _cg(pr, one_eng, k, rhs=b[i], cg_tol=1e-8, precond=precond, mask=pr.masks[i], opt=pr.opts[i])
        X1, P1 = one_eng.cg_vector("x")[0], one_eng.cg_vector("p")[0]
        one_eng.close()
        for key in CG_KEYS:
            assert np.array_equal(one[key][0], R[key][i], equal_nan=True), (key, i)
        assert np.array_equal(X1, X[i]) and np.array_equal(P1, Pd[i]), i


@gpu
def test_trial_kernel_against_numpy(many):
    pr = many
    s = np.array([1.0, 0.5, 0.125])
    # a right-hand side whose solution is 32 times the control's size on the free nodes: s x flips signs and leaves the boxes
    b = _q0(pr.shape, 41)
    want = np.linalg.solve(pr.A, b.ravel()[pr.free])
    b *= 32.0 / np.median(np.abs(want))
    eng = pr.context(3)
    R = _cg(pr, eng, 4 * 12, nb=3, rhs=_tile(b, 3), cg_tol=1e-8, mask=pr.masks, opt=pr.opts)
    X = eng.cg_vector("x")
    assert list(R["n_free"]) == [12, 8, 5]
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
        print(f"MEASURE many_chunks trial member {i}: s {s[i]} pinned {int(pin.sum())} clipped {clipped} of {nodes}; sums dev "
              f"{abs(T['change'][i, 0] / d2 - 1):.2e} {abs(T['change'][i, 1] / n2 - 1):.2e} (bound {nodes * EPS:.2e})")
        assert np.array_equal(T["u"][i].view(np.int64), t.view(np.int64)), i
        assert T["pinned"][i] == pin.sum() and T["clipped"][i] == clipped
        assert abs(T["change"][i, 0] - d2) <= nodes * EPS * d2 and abs(T["change"][i, 1] - n2) <= nodes * EPS * n2
    assert np.array_equal(after, X)


# ---------------------------------------------------------------------------------------------------------------------
# grid: Newton rounds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid(V):
    F1 = V.module("Vch_control_1D.Forward_solver")
    K1 = V.module("Vch_control_1D.config")
    tg, dts = V.time_grid(TG, DTG)
    t = np.concatenate([[0.0], tg])
    P = o.Params1D(N=NG, T=TG, dt_initial=DTG)
    x = np.linspace(0.0, P.Lx, NG + 1)
    u = np.clip(np.stack([1.4 * np.cos(np.pi * x * (1 + k % 3)) * np.sin(1 + k) for k in range(len(t))]), -1.0, 1.0)
    phi0 = F1.init_phi_random(NG, F1.delta_sep, amp=0.01, seed=42, enforce_zero_mean=True)
    M = len(dts)
    one = _engine(V, P, 1, max_steps=M + SPARE)
    phi = one.forward(phi0, np.asarray(dts), u=u)[0]
    one.close()
    ocfg = K1.OptimizationConfig(b3=1.0, u_min=-1.0, u_max=1.0)
    pr = Problem(V, P, t, dts, x, phi, u, V.make_opt(ocfg), max_steps=M + SPARE)
    pr.cfg, pr.ocfg, pr.K1, pr.phi0 = K1.ForwardSolverConfig(N=NG, T=TG, dt_initial=DTG), ocfg, K1, phi0
    return pr


@gpu
def test_newton_rounds_batch_of_three(grid):
    pr, Vm = grid, grid.V
    G1 = Vm.module("Vch_control_1D.GD_1D")
    opts, u0 = _three(pr)
    n_rounds = 2
    eng = _pgd(pr, opts, u0)
    many = eng.pgd_newton(n_rounds)
    Um, Pm = eng.pgd_get("u"), eng.pgd_get("phi")
    eng.close()
    print(f"MEASURE grid rounds: status {many['status'].tolist()} s {many['s'].tolist()} halvings {many['halvings'].tolist()} n_free "
          f"{many['n_free'].tolist()} cg {many['cg_status'].tolist()} in {many['cg_steps'].tolist()} cost {many['cost'].tolist()} -> "
          f"{many['cost_new'].tolist()}")
    assert many["status"][1].tolist() == [STATIONARY, IDLE] and many["n_free"][1, 0] == 0 and not Um[1].any()
    rows, n = pr.shape
    assert many["n_free"][2, 0] == (rows - 1) * n and many["halvings"][2, 0] >= 1
    for r in range(n_rounds):                               # the box-cut start: monotone in cost
        if many["status"][2, r] == ACCEPTED:
            assert many["cost_new"][2, r] < many["cost"][2, r]
    for i in range(3):
        one = _pgd(pr, [opts[i]], u0[i][None])
        got = one.pgd_newton(n_rounds)
        U1, P1 = one.pgd_get("u"), one.pgd_get("phi")
        one.close()
        for key in OUT_KEYS:
            assert np.array_equal(got[key][0], many[key][i], equal_nan=True), (key, i)
        assert np.array_equal(U1, Um[i]) and np.array_equal(P1, Pm[i]), i
    # member 0 against the host loop, with its own start state and targets
    ocfg, _, u = _refine_case(pr)
    uh, recs = G1.newton_refine(pr.cfg, ocfg, u, pr.phi_Q, pr.phi_T, n_newton=n_rounds)
    rel = lambda a, b: abs(a - b) / abs(b)
    dev = dict(steps=0, cost=0.0, cost_new=0.0)
    assert len(recs) == n_rounds
    for r, h in enumerate(recs):
        s = many["s"][0, r]
        print(f"MEASURE grid round {r}: device cost {many['cost'][0, r]:.17g} -> {many['cost_new'][0, r]:.17g} s {s} n_free "
              f"{many['n_free'][0, r]} cg {Vm.Engine1D.CG_STATUS[many['cg_status'][0, r]]} in {many['cg_steps'][0, r]}; host cost "
              f"{h['cost']:.17g} -> {h['cost_new']:.17g} s {h['s']} n_free {h['n_free']} cg {h['status']} in {h['steps']}")
        assert (None if np.isnan(s) else float(s)) == h["s"] and many["n_free"][0, r] == h["n_free"]
        assert Vm.Engine1D.CG_STATUS[many["cg_status"][0, r]] == h["status"]
        assert (many["status"][0, r] == ACCEPTED) == (h["s"] is not None)
        dev["steps"] = max(dev["steps"], abs(int(many["cg_steps"][0, r]) - h["steps"]))
        dev["cost"] = max(dev["cost"], rel(many["cost"][0, r], h["cost"]))
        dev["cost_new"] = max(dev["cost_new"], rel(many["cost_new"][0, r], h["cost_new"]))
    dev["control"] = float(np.abs(Um[0] - uh).max() / np.abs(uh).max())
    print(f"MEASURE grid against the host loop: {dev}")
    for key in dev:
        assert dev[key] <= NEWTON_TOL[key], (key, dev[key])
