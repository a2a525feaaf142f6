"""Qualification of the inputs of test_gpu_1d_offpoint.py, on the CPU oracle alone (not marked gpu).

The GPU tests compare the engine's path through the Newton loop and the PGD line search with the oracle's step for step.
That is only a fair demand where no decision of the path sits on its threshold: once a node reaches the clip value
1 - delta_sep the admissibility test max|phi_t| < 0.99 is taken at distance 0.0 and two correct implementations
legitimately leave through different exits.  Every input (tests/_offpoint_1d.py) must therefore lie in its window here;
a platform change that moves one out fails in this file and not on the GPU.  The windows are conditions, not measurements.

March window: every loop exits "conv", failed_ls == 0, the last residual norm >= MARGIN = 20 x below the tolerance,
min_margin >= 1e-6 (1000 x the 1e-9 field tolerance).  Measured with solver="banded" (oracle.newton_step's margin: the
continuous min(1, 0.9 amax) is not counted), N = 33 / 64, the controlled march (the uncontrolled one is further inside):
    point  start   amp   residual margin    min_margin         max|phi|
    OFF    smooth  12    84060 / 63007      0.805 / 0.805      0.200
    OFF2   smooth  12    18600 / 13982      0.697 / 0.697      0.300
    OFF2   sep     12    228 / 168          9.20e-3 / 9.20e-3  0.985  (the unclipped Newton diagonal near 1)
Clipped-start window (OFF2, start 0.9999 tanh tanh with >= 10 nodes beyond the clip value): the first loop leaves through
the line-search failure after one solve and 12 halvings without an admissible trial point, every later loop converges
>= 20 x below the tolerance, min_margin >= 1e-6; the first step's uniform shift must exceed 1e-4.  N = 33 / 64:
    amp 12   residual margin 264 / 200    min_margin 4.89e-3 / 4.86e-3    shift 1.244e-3 / 1.287e-3
    amp -5   residual margin 230 / 235    min_margin 2.3e-3 / 2.3e-3
    amp 7    residual margin 750 / 539    min_margin 4.51e-3 / 4.48e-3
(amp -9: residual margin 1.0 at N = 33, outside; OFF, amp 12: residual margin 1 - 7, outside: properties only.)
Capped-step window: one Newton call whose first step is cut by alpha = 0.9 amax < 1 and which then converges without a
halving, min_margin >= 1e-6:
    point    N   seed  norms  capped  min_margin
    default  33  2     6      1       1.07e-2
    OFF      33  2     7      1       3.43e-2
    OFF      64  0     6      1       9.32e-2
    OFF2     33  3     5      1       6.30e-4
PGD window (N = 33, 48; three phase shifts of phi0): trials [1, 5, 1, 5] everywhere, smallest relative cost gap 1.75e-3
(OFF) / 7.63e-3 (OFF2) against 1e-6, residual margin >= 703 against 20, min_margin >= 0.67, 53-57 % of u exactly zero and
38-41 % on the box.  The zero pattern of the last control is decided by |u_prev / alpha - (r + b3 u_prev)| <= kappa with
the alpha the control was made with (alphas_used: the last search runs out, so alphas[-1] is 0.8 x that); this rule
reproduces the oracle's own u == 0 at every node, and the smallest distance from kappa = 2e-3 is 9.3e-6, 5.7e-6, 7.7e-5,
2.8e-5 (OFF 33, OFF 48, OFF2 33, OFF2 48 at the shift 0.3 the GPU test compares patterns at), over all shifts 5.2e-7
(one node of 343 inside the 1e-6 band at OFF 48, shift 0.9: share outside 0.9971 against 0.95, 1.0 everywhere else).
Knife edge (OFF2, sep, amp 200, N = 33): exits conv, conv, conv, maxit, failed_ls, min_margin 0.0: outside the window, so
the GPU test asserts path-independent properties only."""
import numpy as np
import pytest

import _offpoint_1d as X
from oracle import vch1d_oracle as O1


@pytest.mark.parametrize("N", X.MARCH_NS)
@pytest.mark.parametrize("point,kind,amp", X.MARCH)
def test_march_inputs_inside_the_window(point, kind, amp, N):
    c = X.march_case(point, kind, amp, N)
    for tag in ("nat", "u", "short"):
        ph, st = c[tag]
        ok, res, mm = X.in_march_window(st)
        print(f"\n{point} {kind} amp {amp} N={N} {tag}: residual margin {res:.0f} min_margin {mm:.3g} "
              f"max|phi| {np.abs(ph).max():.4f}")
        assert [e[0] for e in st["exits"]] == ["conv"] * X.M and st["failed_ls"] == 0
        assert res >= X.MARGIN and mm >= X.MIN_MARGIN and ok
        assert sum(e[1] for e in st["exits"]) == st["newton_its"] == st["solves"] + X.M
    tol = X.march_tol(c)
    assert np.abs(c["u"][0] - c["nat"][0]).max() / np.abs(c["nat"][0]).max() > 100 * tol
    assert not np.array_equal(c["short"][0], c["u"][0])                    # the hold-last branch changes the last step
    if kind == "sep":                                                      # the Newton diagonal near 1, never on the clip
        assert 0.975 < np.abs(c["u"][0]).max() < 1 - O1.DELTA_SEP - 1e-3


def test_knife_edge_is_outside_the_window():
    point, kind, amp = X.KNIFE
    ph, st = X.march_case(point, kind, amp, 33)["u"]
    kinds = [e[0] for e in st["exits"]]
    assert len(kinds) == X.M and sum(k == "conv" for k in kinds) < X.M
    assert not X.in_march_window(st)[0] and st["min_margin"] < X.MIN_MARGIN
    assert np.isfinite(ph).all() and np.abs(ph).max() < 1.0


@pytest.mark.parametrize("N", X.MARCH_NS)
@pytest.mark.parametrize("point,kind,amp", X.CLIPPED)
def test_clipped_start_inputs_inside_the_window(point, kind, amp, N):
    c = X.march_case(point, kind, amp, N)
    for tag in ("nat", "u"):
        ok, res, mm = X.in_clipped_window(c[tag][1])
        sh = X.first_shift(c, tag)
        print(f"\nclipped start {point} amp {amp} N={N} {tag}: residual margin {res:.0f} min_margin {mm:.3g} "
              f"first shift {sh:.3e}")
        assert ok and res >= X.MARGIN and mm >= X.MIN_MARGIN
        assert abs(sh) > 1e-4                      # 1e8 x the 1e-12 mass bound: a wrong divisor of the shift cannot hide
    assert (np.abs(c["phi0"]) > 1 - O1.DELTA_SEP).sum() >= 10


def test_clipped_start_off_is_properties_only():
    """At OFF the loops after the first end within 20 x of the tolerance: no path comparison, but the first step -- the
    old state clipped and shifted -- is decided inside margins."""
    point, kind, amp = X.CLIPPED_PROP
    c = X.march_case(point, kind, amp, 33)
    st = c["u"][1]
    assert st["exits"][0] == ("failed_ls", 1, 12, 0) and st["min_margin"] >= X.MIN_MARGIN
    assert not X.in_clipped_window(st)[0] and abs(X.first_shift(c)) > 1e-4


@pytest.mark.parametrize("point,N,seed", X.CAPPED)
def test_capped_step_inputs_inside_the_window(point, N, seed):
    c = X.capped_case(point, N, seed)
    st = c["st"]
    (kind, its, halvings, capped), = st["exits"]
    print(f"\ncapped {point} N={N} seed {seed}: norms {its} capped {capped} min_margin {st['min_margin']:.3g}")
    assert kind == "conv" and its == len(c["hist"]) and capped >= 1 and st["min_margin"] >= X.MIN_MARGIN
    assert halvings == 0
    # the ceiling cut the FIRST step: alpha = 0.9 amax < 1 for the Newton correction at the start
    P, phi, h = c["P"], c["phi"], c["P"].Lx / N
    R = np.concatenate([O1.residual_phi(phi, phi, c["mu"], c["mu"], c["w_new"], c["w_old"], c["dt"], P, h),
                        O1.residual_mu(phi, phi, c["mu"], c["mu"], c["dt"], h)])
    dphi = O1._solve_newton_banded(phi, c["dt"], P, h, R)[:N + 1]
    lim = np.where(dphi > 0, 1 - O1.DELTA_SEP, -1 + O1.DELTA_SEP)
    amax = np.min((lim - phi)[dphi != 0] / dphi[dphi != 0])
    assert 0.1 < 0.9 * amax < 1.0, amax


@pytest.mark.parametrize("N", X.PGD_NS)
@pytest.mark.parametrize("point", X.PGD_POINTS)
def test_pgd_inputs_inside_the_window(point, N):
    for shift in X.PGD_SHIFTS:
        c = X.pgd_case(point, N, shift)
        res, st, Op = c["res"], c["st"], c["Op"]
        resm = O1.NEWTON_TOL / max(st["last_norms"])
        share = float((c["band"] >= X.BAND).mean())
        zero = float((res.u == 0).mean())
        box = float(((res.u == Op.u_min) | (res.u == Op.u_max)).mean())
        print(f"\npgd {point} N={N} shift {shift}: trials {res.trials} cost gap {st['min_cost_gap']:.3g} residual margin "
              f"{resm:.0f} min_margin {st['min_margin']:.3g} zero {zero:.3f} box {box:.3f} outside band {share:.4f}")
        assert list(res.trials) == [1, 5, 1, 5]          # the accepted optimistic step; backtracking returning its last try
        assert st["min_cost_gap"] >= X.COST_GAP and resm >= X.MARGIN and st["min_margin"] >= X.MIN_MARGIN
        assert all(e[0] == "conv" for e in st["exits"]) and st["failed_ls"] == 0
        assert np.array_equal(c["zero_predicted"], res.u == 0)     # the band is measured round the real threshold
        print(f"smallest distance from the prox threshold {c['band'].min():.3g} (kappa {Op.kappa_sparsity:g})")
        assert share >= 0.95 and 0.3 < zero < 0.7 and box > 0.2
