"""The long-double restatement of the PGD loops' by-products (tests/_pgd_byproducts_ref.py) against the two oracles, on
the CPU: it reproduces the relative control change and the tracking / terminal errors that O2.pgd and O1.pgd record, from
the iterates the loops accepted, on a rectangular grid with a ragged last time step; and it agrees with error_metrics on
random histories over a ragged time grid, RMS fallback and zero terminal target included.
"""
import numpy as np
import pytest

import _pgd_byproducts_ref as R
from oracle import vch1d_oracle as O1
from oracle import vch2d_oracle as O2

TOL = 1e-13
DT = 1e-2


def _record(mod, run):
    """run() with mod.cost and mod.error_metrics recording their (phi, u) / phi arguments.  The last cost the loop evaluated
    before it calls error_metrics is that of the candidate it accepted (optimistic, first descent or last try)."""
    cost, metrics = mod.cost, mod.error_metrics
    last, accepted = [], []

    def rec_cost(phi, u, *a, **kw):
        last[:] = [phi, u]
        return cost(phi, u, *a, **kw)

    def rec_metrics(phi, *a, **kw):
        assert phi is last[0]
        accepted.append((last[0], last[1]))
        return metrics(phi, *a, **kw)
    mod.cost, mod.error_metrics = rec_cost, rec_metrics
    try:
        res = run()
    finally:
        mod.cost, mod.error_metrics = cost, metrics
    return res, accepted


def _close(a, b):
    return abs(a - b) <= TOL * abs(b)


@pytest.mark.parametrize("alpha_max", [50.0, 4e4])
def test_restatement_reproduces_the_2d_loop(alpha_max):
    """12 x 9, Lx = 1.3, Ly = 0.9, T = 3.5 dt (four steps, the last one half): three iterations, with the default first step
    and with one that makes the loop backtrack."""
    P = O2.Params2D(Nx=12, Ny=9, Lx=1.3, Ly=0.9, T=3.5 * DT, dt_initial=DT)
    res, acc = _record(O2, lambda: O2.pgd(P, O2.OptParams(alpha_max=alpha_max), n_iter=3))
    assert len(acc) == 3 and res.t_hist.size == 5 and abs(res.t_hist[-1] - res.t_hist[-2] - 0.5 * DT) < 1e-15
    if alpha_max > 50.0:
        assert max(res.attempts) > 0, res.attempts
    u_old = np.zeros_like(acc[0][1])
    for k, (phi, u) in enumerate(acc):
        trk, trm = R.errors_2d(phi, res.phi_Q, res.phi_T, res.x, res.y, res.t_hist)
        assert _close(R.change(u, u_old), res.changes[k]), (k, R.change(u, u_old), res.changes[k])
        assert _close(trk, res.tracking[k]) and _close(trm, res.terminal[k]), (k, trk, res.tracking[k], trm, res.terminal[k])
        u_old = u
    assert np.array_equal(u_old, res.u)


@pytest.mark.parametrize("alpha_max", [100.0, 2e5])
def test_restatement_reproduces_the_1d_loop(alpha_max):
    """N = 24, Lx = 1.3, T = 3.5 dt: three iterations."""
    P = O1.Params1D(N=24, Lx=1.3, T=3.5 * DT, dt_initial=DT)
    res, acc = _record(O1, lambda: O1.pgd(P, O1.OptParams1D(alpha_max=alpha_max), n_iter=3))
    assert len(acc) == 3 and res.t_hist.size == 6 and res.t_hist[0] == res.t_hist[1] == 0.0
    if alpha_max > 100.0:
        assert max(res.trials) > 1, res.trials
    u_old = np.zeros_like(acc[0][1])
    for k, (phi, u) in enumerate(acc):
        trk, trm = R.errors_1d(phi, res.phi_Q, res.phi_T, res.x, res.t_hist)
        assert _close(R.change(u, u_old), res.changes[k]), (k, R.change(u, u_old), res.changes[k])
        assert _close(trk, res.tracking[k]) and _close(trm, res.terminal[k]), (k, trk, res.tracking[k], trm, res.terminal[k])
        u_old = u
    assert np.array_equal(u_old, res.u)


def _ragged(rng, n, length):
    g = np.r_[0.0, np.cumsum(rng.uniform(0.3, 1.7, n - 1))]
    return g * (length / g[-1])


@pytest.mark.parametrize("case", ["plain", "fallback", "zero_terminal"])
def test_error_metrics_on_a_ragged_time_grid(case):
    """Random histories on non-uniform x, y and t: the restatement against O2.error_metrics and O1.error_metrics, with a
    target history of size 1e-12 (the RMS fallback decides the tracking denominator) and with phi_T = 0 (the terminal
    denominator is the bare 1e-12)."""
    rng = np.random.default_rng(5)
    x, y, t = _ragged(rng, 13, 1.3), _ragged(rng, 10, 0.9), _ragged(rng, 7, 0.055)
    phi, pq = rng.standard_normal((2, 7, 13, 10))
    pt = rng.standard_normal((13, 10))
    if case == "fallback":
        pq *= 1e-12
    if case == "zero_terminal":
        pt[:] = 0.0
    p2 = R.errors_2d_parts(phi, pq, pt, x, y, t)
    assert p2["fallback"] == (case == "fallback")
    ref = O2.error_metrics(phi, pq, pt, x, y, t)
    assert _close(p2["track"], ref[0]) and _close(p2["term"], ref[1]), (p2, ref)
    assert (p2["track"], p2["term"]) == R.errors_2d(phi, pq, pt, x, y, t)
    if case == "zero_terminal":
        assert p2["den_T"] == 0.0 and p2["term"] > 1e11
    t1 = np.r_[0.0, t]                                                  # the 1D history's duplicated t = 0 row
    p1 = R.errors_1d_parts(np.concatenate([phi[:1, :, 0], phi[:, :, 0]]), np.concatenate([pq[:1, :, 0], pq[:, :, 0]]), pt[:, 0], x, t1)
    ref1 = O1.error_metrics(np.concatenate([phi[:1, :, 0], phi[:, :, 0]]), np.concatenate([pq[:1, :, 0], pq[:, :, 0]]), pt[:, 0], x, t1)
    assert p1["fallback"] == (case == "fallback")
    assert _close(p1["track"], ref1[0]) and _close(p1["term"], ref1[1]), (p1, ref1)


def test_change_and_gap_at_zero():
    u = np.zeros((3, 4))
    assert R.change(u, u) == 0.0
    v = np.full((3, 4), 2.0)
    assert R.change(v, u) == pytest.approx(np.sqrt(12.0) * 2.0 / 1e-9, rel=1e-15)
    assert R.gap(0.0, 0.0) == 0.0 and R.gap(1e-300, 0.0) == float("inf") and R.gap(0.0, 1.0) == float("inf")
    assert R.gap(1.5, 1.0) == 0.5
