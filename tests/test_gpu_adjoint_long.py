"""GPU tests of the 2D adjoint sweep's host logic (backward_pass / backward_core, csrc/vch_engine2d.hip) on sweeps of
M = 50 levels: the look schedule past its settle phase, guesses of order > 1 over a ring, the weight fallback on ragged
time grids, the restart of the ring behind a zero-length step, and the repeat pass (a solve ran out of its enqueued
sweeps: the whole batch is swept again on the safe schedule and the members whose first pass stood are put back).

Inputs (tests/_adjoint_sched.py): given histories on 32 x 16 (run-time FFT plan, guesses on) and 20 x 14 (GEMM), smooth
levels (D = f'' constant to 1 %) and separated levels (D from -0.5 to 36), default physics, b1 = 5, b2 = 10, both targets.
The oracle (scipy's direct solves) runs live, once per input.

Every sweep is checked by _check_sweep, test_gpu_plans._check_adjoint generalised to any time grid and to a given
history: step and terminal equations to max(1e-11, 10 x the oracle's own residual in the same equation), q to SOLVE,
p to max(SOLVE, 20 eps cond), r to MARCH, zero-length levels bitwise the level above, no output all zero.
Tolerances of test_gpu_plans.py: OPS 1e-12, SOLVE 1e-9, MARCH 1e-8.  Bitwise claims carry no tolerance.

Measured on an MI355X (the MEASURE lines of the tests, run with -s), each next to the bound derived for it:
  sweeps of one solve from zero, dt = 1e-3   smooth level 3, separated level 8 on both grids (8 and 10 at dt = 1e-2 against
                                             4); premise 8 >= 2 x 3 + 2.  No look inside either (8 < CG_CHUNK = 24)
  step residuals, uniform / ragged steps     engine 0.9e-14 .. 9e-14, oracle 1.2e-14 .. 1.5e-13: bound 1e-11
  step residuals, alternating steps          engine 9.3e-13, oracle 6.1e-12 (level 2: 8.9e-13 against 3.4e-11 = 10 x oracle)
  rel.err to the oracle                      p <= 5.5e-12 (1e-9), q <= 2.7e-13 (1e-9), r <= 1.4e-11 (1e-8)
  A, looks                                   fft 22 = 20 of look_levels + 2 closing reads (bound 20 + ceil(8 / 24) + 2 = 23);
                                             guesses off 10 (bound 8 + 1 + 2); gemm 10 (bound 11).  Sweeps of B = 2:
                                             250 with guesses, 303 without (0.83; bound 0.85 as in test_gpu_r2.py)
  D, looks                                   72 on fft and 60 on gemm (first pass + M = 50 of the repeat), 22 / 10 without
  E                                          the ramp member alone is repeated (72 / 60 looks; smooth and separated members
                                             22 / 10), so the B = 3 batch repeats too; unconverged_solves 0 in all four runs
                                             after the repeat

What the module found when it was written, all three fixed with it:
  * gemm grids: k_fin_cg_beta did not record step_lin_max, so the host enqueued the minimum of 2 sweeps per solve where 3
    were needed and every sweep of more than one level was repeated (case A: 60 looks and 506 sweeps, now 10 and 302).
  * case E failed on the fft grid: the ramp member converged in the batch (22 looks, its mates' longer solves paid for its
    sweeps) and was repeated alone (72 looks), p differing by 9.3e-13.  Sweep caps are now per trajectory (lin_cap).
  * the stale redo_iters of case D.
On the alternating grid of case B the sweep is repeated as well (72 looks): behind a long step the solves lengthen by
more than one sweep inside a look window.  The results stand (the repeat pass is the designed answer); it costs time only.
"""
import math

import numpy as np
import pytest

import _adjoint_sched as S
from conftest import relerr
from test_gpu_forms import _env

pytestmark = pytest.mark.gpu

OPS, SOLVE, MARCH = 1e-12, 1e-9, 1e-8
M, DT = S.M, S.DT
GRID_IDS = sorted(S.GRIDS)


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


@pytest.fixture(scope="module")
def O2():
    from oracle import vch2d_oracle
    return vch2d_oracle


def _engine(V, grid, B):
    Nx, Ny, Lx, Ly = S.GRIDS[grid]
    return V.Engine2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, batch=B, max_steps=M)


def _sweep(V, grid, t, hists, want=("p", "q", "r"), env=None, engine=None):
    """One sweep of the histories `hists` (a list: the batch) under the targets of the grid, on a fresh context unless
    one is given.  Returns (p, q, r, stats) with a leading batch axis on the fields."""
    B = len(hists)
    pq, pt = S.targets(grid)
    e = engine if engine is not None else _engine(V, grid, B)
    try:
        with _env(**(env or {})):
            out = e.backward(np.stack(hists), t, S.B1, S.B2, np.stack([pq] * B), np.stack([pt] * B), want=want)
    finally:
        if engine is None:
            e.close()
    p, q, r, st = out
    lead = lambda a: None if a is None else (a[None] if B == 1 else a)
    return lead(p), lead(q), lead(r), st


def _check_sweep(O2, grid, t, hist, p, q, r, tag):
    """One trajectory's sweep against the oracle's (see the module docstring)."""
    pr, qr, rr = S.oracle_sweep(O2, grid, t, hist)
    Nx, Ny, Lx, Ly = S.GRIDS[grid]
    hx, hy = Lx / Nx, Ly / Ny
    res = S.step_residuals(O2, grid, t, hist, p)
    ref = S.step_residuals(O2, grid, t, hist, pr)
    solved = ~np.isnan(ref)
    bound = np.maximum(1e-11, 10.0 * ref)
    worst = int(np.nanargmax(res / bound))
    print(f"MEASURE {tag}: step residual, engine {np.nanmax(res):.2e} oracle {np.nanmax(ref):.2e}; worst against its bound "
          f"at level {worst}: {res[worst]:.2e} / {bound[worst]:.2e}; rel.err p {relerr(p, pr):.2e} q {relerr(q, qr):.2e} "
          f"r {relerr(r, rr):.2e}")
    assert np.all(res[solved] < bound[solved]), (tag, worst, res[worst], bound[worst])
    zero = np.flatnonzero(~solved)
    assert list(zero) == [n for n in range(M) if t[n + 1] - t[n] <= S.DT_ZERO]
    for n in zero:
        for a in (p, q, r):
            assert np.array_equal(a[n], a[n + 1]), (tag, n)
    assert relerr(q, qr) < SOLVE, (tag, relerr(q, qr))
    lam = 4.0 / hx ** 2 + 4.0 / hy ** 2
    tol_p = max(SOLVE, 20 * np.finfo(float).eps * (1.0 + 0.05 * lam + 0.5 * float(np.max(np.diff(t))) * lam ** 2))
    assert relerr(p, pr) < tol_p, (tag, relerr(p, pr), tol_p)
    assert relerr(r, rr) < MARCH, (tag, relerr(r, rr))
    for a in (p, q, r):
        assert np.all(np.isfinite(a)) and np.any(a != 0.0), tag


def _same(a, b):
    return all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------ premise
_SWEEPS = {}


def _level_sweeps(V, grid):
    """Sweeps of a single solve A(phi_n) x = rhs from x = 0 (Engine2D.adjoint_solve) on a smooth and on a separated
    level, dt = DT, and the looks inside the separated one (the call's host_syncs less its two own reads)."""
    if grid not in _SWEEPS:
        rhs = S.B2 * (S.smooth_level(grid, M) - S.targets(grid)[1])
        e = _engine(V, grid, 1)
        _, st_s = e.adjoint_solve(S.smooth_level(grid, 20), DT, rhs)
        _, st_h = e.adjoint_solve(S.sep_level(grid, 20), DT, rhs)
        e.close()
        assert st_s["unconverged_solves"] == 0 and st_h["unconverged_solves"] == 0, (st_s, st_h)
        _SWEEPS[grid] = (st_s["linear_iters"], st_h["linear_iters"], st_h["host_syncs"] - 2)
        print(f"MEASURE {grid}: sweeps of one solve at dt = {DT:g}: smooth level {_SWEEPS[grid][0]}, separated level "
              f"{_SWEEPS[grid][1]} (looks inside it: {_SWEEPS[grid][2]})")
    return _SWEEPS[grid]


@pytest.mark.parametrize("grid", GRID_IDS)
def test_premise_separated_levels_solve_longer(V, grid):
    """What cases D and E lean on: a separated level needs at least twice the sweeps of a smooth one plus 2, so a
    schedule taken from smooth solves (longest + 1 or + 2) cannot finish a separated one."""
    k_smooth, k_sep, _ = _level_sweeps(V, grid)
    assert k_smooth >= 1 and k_sep >= 2 * k_smooth + 2, (k_smooth, k_sep)


# ------------------------------------------------------------------------------------------------ A. long sweep, uniform steps
def _first_solve_looks(V, grid):
    """Looks inside the first solve of a sweep, which runs on the rigorous budget with a look every CG_CHUNK sweeps
    until every trajectory has converged: at most ceil(k / CG_CHUNK) for a solve of k sweeps.  k is bounded by the
    measured count of the hardest kind of level started from zero (the sweep's first solve starts from p_M)."""
    return math.ceil(_level_sweeps(V, grid)[1] / S.CG_CHUNK)


@pytest.mark.parametrize("grid", GRID_IDS)
def test_long_sweep_uniform(V, O2, grid):
    """A.  B = 2, two smooth histories, 50 uniform levels: against the oracle, every solve converged, and no more looks
    than the schedule's (look_levels) + those inside the first solve + the two reads that close a sweep (backward_core
    reads the records, vch2d_backward reads them before it copies out).  On the FFT grid the guesses pay at 50 levels:
    fewer sweeps than under VCH_ADJ_GUESS_OFF=1."""
    t = S.t_uniform()
    hs = [S.hist_smooth(grid, 0), S.hist_smooth(grid, 1)]
    p, q, r, st = _sweep(V, grid, t, hs)
    for b in range(2):
        _check_sweep(O2, grid, t, hs[b], p[b], q[b], r[b], f"A {grid} b={b}")
    looks = len(S.look_levels(M, S.uses_guess(grid))) + _first_solve_looks(V, grid) + 2
    print(f"MEASURE A {grid}: host_syncs {st['host_syncs']} (bound {looks}), linear_iters {st['linear_iters']}, "
          f"unconverged {st['unconverged_solves']}")
    assert st["unconverged_solves"] == 0, st
    assert st["host_syncs"] <= looks, (st, looks)
    if S.uses_guess(grid):
        p0, q0, r0, st0 = _sweep(V, grid, t, hs, env={"VCH_ADJ_GUESS_OFF": 1})
        print(f"MEASURE A {grid}: linear_iters without guesses {st0['linear_iters']}, host_syncs {st0['host_syncs']}")
        assert st["linear_iters"] < 0.85 * st0["linear_iters"], (st, st0)
        assert st0["host_syncs"] <= len(S.look_levels(M, False)) + _first_solve_looks(V, grid) + 2, st0
        for b in range(2):
            _check_sweep(O2, grid, t, hs[b], p0[b], q0[b], r0[b], f"A {grid} b={b} guesses off")


# ------------------------------------------------------------------------------------------------ B. ragged steps
@pytest.mark.parametrize("steps", ["ragged", "alternating"])
def test_ragged_steps(V, O2, steps):
    """B.  FFT grid, a smooth and a separated history.  ragged: steps dt (0.5 + U(0,1)).  alternating: steps s, s, L, L
    with L = 50 s, where the order-2 weights reach 101 > 64 and the order must drop (checked here with the formula of
    backward_pass; plain alternation s, L would give the guesses a uniform grid, tests/test_adjoint_sched_cpu.py)."""
    t = S.t_ragged() if steps == "ragged" else S.t_alternating()
    assert bool(S.orders_lowered(t)) == (steps == "alternating")
    hs = [S.hist_smooth("fft", 0), S.hist_sep("fft")]
    p, q, r, st = _sweep(V, "fft", t, hs)
    print(f"MEASURE B {steps}: host_syncs {st['host_syncs']}, linear_iters {st['linear_iters']}, unconverged "
          f"{st['unconverged_solves']}, max_lin_relres {st['max_lin_relres']:.2e}")
    for b in range(2):
        _check_sweep(O2, "fft", t, hs[b], p[b], q[b], r[b], f"B {steps} b={b}")
    assert st["unconverged_solves"] == 0, st


# ------------------------------------------------------------------------------------------------ C. zero-length steps
@pytest.mark.parametrize("place", ["settle", "after_look", "two", "step0", "last"])
@pytest.mark.parametrize("grid", GRID_IDS)
def test_zero_length_steps(V, O2, grid, place):
    """C.  Zero-length steps inside the settle phase, directly after a look of the steady phase, two in a row, at step 0
    and at the last step (the first solve of the sweep then comes one level later): against the oracle, the copied
    levels bitwise the level above.  Behind a copied level the ring of the guesses starts again."""
    t = S.t_zero(S.zero_places(grid)[place])
    hs = [S.hist_smooth(grid, 0), S.hist_sep(grid)]
    p, q, r, st = _sweep(V, grid, t, hs)
    print(f"MEASURE C {grid} {place}: host_syncs {st['host_syncs']}, linear_iters {st['linear_iters']}, unconverged "
          f"{st['unconverged_solves']}")
    for b in range(2):
        _check_sweep(O2, grid, t, hs[b], p[b], q[b], r[b], f"C {grid} {place} b={b}")
    # r only: the copy branch with the p and q outputs NULL
    _, _, r1, _ = _sweep(V, grid, t, hs, want=("r",))
    assert np.array_equal(r1, r)


# ------------------------------------------------------------------------------------------------ D. the repeat pass
def _jump_refs(V, O2, grid, place):
    """Case D's inputs and single runs: the jump history alone on the safe schedule, the smooth ones alone by default."""
    key = ("D", grid, place)
    if key not in _SWEEPS:
        t = S.t_uniform()
        hard = S.hist_jump(grid, S.jump_levels(grid)[place])
        easy = [S.hist_smooth(grid, 0), S.hist_smooth(grid, 1)]
        safe = _sweep(V, grid, t, [hard], env={"VCH_ADJ_SAFE": 1})
        singles = [_sweep(V, grid, t, [h]) for h in easy]
        for s in singles:
            assert s[3]["unconverged_solves"] == 0 and s[3]["host_syncs"] < M, s[3]      # no repeat in the smooth runs
        _check_sweep(O2, grid, t, hard, safe[0][0], safe[1][0], safe[2][0], f"D {grid} {place} safe single")
        _SWEEPS[key] = (t, hard, easy, safe, singles)
    return _SWEEPS[key]


@pytest.mark.parametrize("place", ["after_look", "before_look", "last_solve"])
@pytest.mark.parametrize("grid", GRID_IDS)
def test_repeat_pass(V, O2, grid, place):
    """D.  Trajectory 0 turns from smooth to separated one level after a look / ADJ_LOOK - 1 levels after a look / at
    level 0 only (the last solve of the sweep, which no later solve counts: the lin_active branch of backward_core);
    trajectory 1 is smooth.  The schedule taken from the smooth solves cannot finish the separated ones
    (test_premise_separated_levels_solve_longer), so the sweep is repeated: host_syncs >= M.  Trajectory 0 is then
    bitwise its B = 1 sweep on the safe schedule, and trajectory 1, saved and put back, bitwise its B = 1 default sweep.
    The same with the r output only (p and q NULL: one block per kept member in the save buffer) and with B = 1 (nothing
    kept)."""
    t, hard, easy, safe, singles = _jump_refs(V, O2, grid, place)
    p, q, r, st = _sweep(V, grid, t, [hard, easy[0]])
    print(f"MEASURE D {grid} {place}: n0 = {S.jump_levels(grid)[place]}, host_syncs {st['host_syncs']}, linear_iters "
          f"{st['linear_iters']}, unconverged (repeat pass) {st['unconverged_solves']}; smooth single: host_syncs "
          f"{singles[0][3]['host_syncs']}")
    assert st["host_syncs"] >= M, st                                   # the premise: the repeat happened
    _check_sweep(O2, grid, t, hard, p[0], q[0], r[0], f"D {grid} {place} b=0")
    _check_sweep(O2, grid, t, easy[0], p[1], q[1], r[1], f"D {grid} {place} b=1")
    assert _same((p[0], q[0], r[0]), (safe[0][0], safe[1][0], safe[2][0]))
    assert _same((p[1], q[1], r[1]), (singles[0][0][0], singles[0][1][0], singles[0][2][0]))
    pn, qn, r_only, st_r = _sweep(V, grid, t, [hard, easy[0]], want=("r",))
    assert pn is None and qn is None and st_r["host_syncs"] >= M
    assert np.array_equal(r_only, r)
    p1, q1, r1, st1 = _sweep(V, grid, t, [hard])
    assert st1["host_syncs"] >= M, st1
    assert _same((p1[0], q1[0], r1[0]), (safe[0][0], safe[1][0], safe[2][0]))


@pytest.mark.parametrize("grid", GRID_IDS)
def test_repeat_pass_hard_member_in_the_middle(V, O2, grid):
    """D, B = 3 with the hard member between two smooth ones: each member bitwise its own single run."""
    t, hard, easy, safe, singles = _jump_refs(V, O2, grid, "after_look")
    p, q, r, st = _sweep(V, grid, t, [easy[0], hard, easy[1]])
    assert st["host_syncs"] >= M, st
    assert _same((p[1], q[1], r[1]), (safe[0][0], safe[1][0], safe[2][0]))
    for b, s in ((0, singles[0]), (2, singles[1])):
        assert _same((p[b], q[b], r[b]), (s[0][0], s[1][0], s[2][0])), b
    _check_sweep(O2, grid, t, easy[1], p[2], q[2], r[2], f"D {grid} B=3 b=2")


@pytest.mark.parametrize("grid", GRID_IDS)
def test_context_after_a_repeat_pass(V, O2, grid):
    """D, afterwards on the same context: the sweeps of the repeated pass's first pass belong to that call only.  A
    forward march and a sweep under VCH_ADJ_SAFE=1 report the linear_iters of the same call on a fresh context; a
    default sweep of smooth histories gives the bits and the host_syncs of a fresh context; the save buffer is gone
    (vch_mem_live as in test_gpu_mem_owner.py: the repeat leaves no block behind, close() returns to the base)."""
    lib = V.load()
    t, hard, easy, safe, singles = _jump_refs(V, O2, grid, "after_look")
    phi0, dts = S.march_input(grid)
    phi0 = np.stack([phi0, -phi0])
    base = lib.vch_mem_live()
    fresh = _engine(V, grid, 2)
    _, st_f = fresh.forward(phi0, dts)
    live_f = lib.vch_mem_live()
    fresh_smooth = _sweep(V, grid, t, easy, engine=fresh)
    live_swept = lib.vch_mem_live() - live_f                           # the lazy families of a sweep
    fresh_safe = _sweep(V, grid, t, [hard, easy[0]], env={"VCH_ADJ_SAFE": 1}, engine=fresh)
    assert lib.vch_mem_live() - live_f == live_swept
    fresh.close()
    assert lib.vch_mem_live() == base

    e = _engine(V, grid, 2)
    e.forward(phi0, dts)
    rep = _sweep(V, grid, t, [hard, easy[0]], engine=e)
    assert rep[3]["host_syncs"] >= M, rep[3]
    assert lib.vch_mem_live() - live_f == live_swept, "the save buffer of the repeat pass is still allocated"
    _, st_f1 = e.forward(phi0, dts)
    print(f"MEASURE D {grid} afterwards: forward linear_iters {st_f1['linear_iters']} (fresh {st_f['linear_iters']}); "
          f"repeated sweep linear_iters {rep[3]['linear_iters']}, safe sweep {fresh_safe[3]['linear_iters']}")
    assert st_f1["linear_iters"] == st_f["linear_iters"], (st_f1, st_f)
    again_safe = _sweep(V, grid, t, [hard, easy[0]], env={"VCH_ADJ_SAFE": 1}, engine=e)
    assert again_safe[3]["linear_iters"] == fresh_safe[3]["linear_iters"], (again_safe[3], fresh_safe[3])
    assert _same(again_safe[:3], fresh_safe[:3])
    again = _sweep(V, grid, t, easy, engine=e)
    assert _same(again[:3], fresh_smooth[:3])
    assert again[3]["host_syncs"] == fresh_smooth[3]["host_syncs"] and again[3]["linear_iters"] == fresh_smooth[3]["linear_iters"]
    assert lib.vch_mem_live() - live_f == live_swept
    e.close()
    assert lib.vch_mem_live() == base


# ------------------------------------------------------------------------------------------------ E. unequal members on a ramp
@pytest.mark.parametrize("grid", GRID_IDS)
def test_unequal_members_equal_single_runs(V, O2, grid):
    """E.  B = 3: a smooth history, one that ramps from smooth to separated over the levels 30 .. 14 (its solves lengthen
    inside a look window), one separated throughout.  The sweeps enqueued per level come from the longest solve of the
    BATCH; include/vch.h promises that a member of a batch of <= 32 is bitwise its single run all the same.  Each member
    against its B = 1 run, bitwise, in p, q, r, and in unconverged_solves (the batch's count is the sum of the
    singles'); every run against the oracle."""
    t = S.t_uniform()
    hs = [S.hist_smooth(grid, 0), S.hist_ramp(grid), S.hist_sep(grid)]
    names = ("smooth", "ramp", "separated")
    p, q, r, st = _sweep(V, grid, t, hs)
    print(f"MEASURE E {grid} batch: unconverged {st['unconverged_solves']}, host_syncs {st['host_syncs']}, linear_iters "
          f"{st['linear_iters']}")
    singles = []
    for b, h in enumerate(hs):
        s = _sweep(V, grid, t, [h])
        singles.append(s)
        print(f"MEASURE E {grid} single {names[b]}: unconverged {s[3]['unconverged_solves']}, host_syncs "
              f"{s[3]['host_syncs']}, linear_iters {s[3]['linear_iters']}, max_lin_relres {s[3]['max_lin_relres']:.2e}")
    for b, h in enumerate(hs):
        _check_sweep(O2, grid, t, h, p[b], q[b], r[b], f"E {grid} batch {names[b]}")
        s = singles[b]
        _check_sweep(O2, grid, t, h, s[0][0], s[1][0], s[2][0], f"E {grid} single {names[b]}")
    for b in range(3):
        s = singles[b]
        diff = max(float(np.max(np.abs(u[b] - v[0]))) for u, v in zip((p, q, r), s[:3]))
        assert _same((p[b], q[b], r[b]), (s[0][0], s[1][0], s[2][0])), (names[b], diff)
    assert st["unconverged_solves"] == sum(s[3]["unconverged_solves"] for s in singles), (st, [s[3] for s in singles])


# ------------------------------------------------------------------------------------------------ F. shared policy
def test_batch_beyond_guess_bmax(V, O2):
    """F.  B = 33 on the FFT grid: one guess order for the batch, fed by the worst member.  The smooth histories of case A
    cycled, amplitudes scaled by 1 + 0.01 b; members 0, 16 and 32 against the oracle, every solve converged.  (Bitwise
    equality with single runs is not promised above GUESS_BMAX = 32.)"""
    t = S.t_uniform()
    hs = [(1.0 + 0.01 * b) * S.hist_smooth("fft", b % 2) for b in range(S.GUESS_BMAX + 1)]
    p, q, r, st = _sweep(V, "fft", t, hs)
    print(f"MEASURE F: host_syncs {st['host_syncs']}, linear_iters {st['linear_iters']}, unconverged "
          f"{st['unconverged_solves']}")
    for b in (0, 16, 32):
        _check_sweep(O2, "fft", t, hs[b], p[b], q[b], r[b], f"F b={b}")
    assert st["unconverged_solves"] == 0, st
