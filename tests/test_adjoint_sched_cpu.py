"""tests/_adjoint_sched.py pinned without a GPU: the look schedule against cases worked by hand from backward_pass
(csrc/vch_engine2d.hip), the guess weights against the closed form, and every synthetic input of
tests/test_gpu_adjoint_long.py against the oracle alone (inside the clips, a finite sweep, bitwise copies at the
zero-length steps)."""
import numpy as np
import pytest

import _adjoint_sched as S
from oracle import vch2d_oracle as O2


def test_look_levels_hand_worked():
    """M = 50.  Guesses on: the first solve (49), the look right after it (48), then every level while M-1-n < 16, i.e.
    down to 34; steps_since_look is 1 after 34 and reaches 8 at level 26; then 18, 10, 2.  Guesses off: 49, 48, then
    steps_since_look is 1 after 48 and reaches 8 at level 40; then 32, 24, 16, 8, 0."""
    assert S.look_levels(50, True) == list(range(49, 33, -1)) + [26, 18, 10, 2]
    assert S.look_levels(50, False) == [49, 48, 40, 32, 24, 16, 8, 0]
    assert S.steady_looks(50, True) == [26, 18, 10, 2] and S.steady_looks(50, False) == [40, 32, 24, 16, 8, 0]
    # M = 64 (tests/test_gpu_r2.py): 16 + 6 looks, inside that test's M // 8 + 16 with the two closing reads
    assert len(S.look_levels(64, True)) == 22
    # short sweeps: every level is looked at (what the M <= 8 tests of the suite run)
    assert S.look_levels(8, True) == list(range(7, -1, -1)) and S.look_levels(2, False) == [1, 0]
    assert S.look_levels(1, True) == [0]


def test_look_levels_zero_steps():
    """A copied level has no look and does not count as a step since the last look."""
    # the last step is copied: the first solve is level 48, the look after it 47; the settle phase still ends at 34
    t = S.t_zero((49,))
    assert S.look_levels(50, True, t) == list(range(48, 33, -1)) + [26, 18, 10, 2]
    assert S.look_levels(50, False, t) == [48, 47, 39, 31, 23, 15, 7]
    # level 25 copied: the window after the look at 26 is one level longer
    t = S.t_zero((25,))
    assert S.look_levels(50, True, t) == list(range(49, 33, -1)) + [26, 17, 9, 1]
    # a copied level inside the settle phase is skipped only
    t = S.t_zero((40,))
    assert S.look_levels(50, True, t) == [n for n in range(49, 33, -1) if n != 40] + [26, 18, 10, 2]
    # the places of case C lie where their names say
    for g in S.GRIDS:
        guess = S.uses_guess(g)
        z = S.zero_places(g)
        assert S.M - 1 - z["settle"][0] < S.ADJ_SETTLE
        assert z["after_look"][0] + 1 in S.steady_looks(S.M, guess)
        assert z["two"][0] - z["two"][1] == 1 and z["step0"] == (0,) and z["last"] == (S.M - 1,)
    assert S.uses_guess("fft") and not S.uses_guess("gemm")


def test_jump_levels():
    for g in S.GRIDS:
        looks = S.look_levels(S.M, S.uses_guess(g))
        j = S.jump_levels(g)
        assert j["after_look"] + 1 in looks and j["before_look"] + S.ADJ_LOOK - 1 in looks and j["last_solve"] == 1
        assert j["before_look"] - 1 in looks      # the first separated level is the next look's: the look precedes its solve
        h = S.hist_jump(g, j["after_look"])
        n0 = j["after_look"]
        assert np.array_equal(h[n0], S.smooth_level(g, n0)) and np.array_equal(h[n0 - 1], S.sep_level(g, n0 - 1))


def test_guess_weights():
    """Uniform grid: order 1 is p_{n+2}, order 2 is 2 p_{n+2} - p_{n+4}, order 4 the cubic (4, -6, 4, -1).  The
    alternating grid crosses sum |w| > 64 at order 2 (1 + 2 L/s = 101 where the window's two pairs are L, L and s, s),
    the ragged one and plain alternation do not."""
    t = S.t_uniform()
    for mu, want in ((1, [1.0]), (2, [2.0, -1.0]), (4, [4.0, -6.0, 4.0, -1.0])):
        w, mag = S.guess_weights(t, 10, mu)
        assert np.allclose(w, want, rtol=1e-12) and abs(mag - np.sum(np.abs(want))) < 1e-10
    assert not S.orders_lowered(t) and not S.orders_lowered(S.t_ragged())
    ta = S.t_alternating()
    steps = np.diff(ta)
    assert abs(steps.max() / steps.min() - 50.0) < 1e-9
    low = S.orders_lowered(ta)
    assert len(low) >= 10, low
    assert abs(max(S.guess_weights(ta, n, 2)[1] for n in low) - 101.0) < 1e-6
    plain = np.concatenate([[0.0], np.cumsum(np.where(np.arange(S.M) % 2 == 0, 1e-4, 5e-3))])
    assert not S.orders_lowered(plain)


_INPUTS = S.inputs()


@pytest.mark.parametrize("name", sorted(_INPUTS))
def test_input_qualifies(name):
    g, t, h = _INPUTS[name]
    Nx, Ny = S.GRIDS[g][:2]
    assert h.shape == (S.M + 1, Nx + 1, Ny + 1) and t.shape == (S.M + 1,) and np.all(np.diff(t) >= 0.0)
    assert np.max(np.abs(h)) <= S.PHI_MAX, np.max(np.abs(h))
    p, q, r = S.oracle_sweep(O2, g, t, h)
    assert all(np.all(np.isfinite(a)) for a in (p, q, r))
    assert all(np.any(a[:S.M] != 0.0) for a in (p, q, r))
    zero = [n for n in range(S.M) if t[n + 1] - t[n] <= S.DT_ZERO]
    assert ("-zero-" in name) == bool(zero)
    for n in zero:
        assert all(np.array_equal(a[n], a[n + 1]) for a in (p, q, r)), n
    # the oracle's own p in its own equations: the reference error that the GPU module's bound starts from
    res = S.step_residuals(O2, g, t, h, p)
    assert np.all(np.isnan(res[zero])) and np.nanmax(res) < 1e-9, np.nanmax(res)
    D = O2.fpp(h, 0.75, 1.0)
    if "sep" in name:
        assert D.min() < -0.45 and D.max() > 30.0, (D.min(), D.max())
    if "smooth" in name:
        assert D.max() - D.min() < 0.02, (D.min(), D.max())
