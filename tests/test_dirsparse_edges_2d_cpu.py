"""CPU-only conditions on the inputs of tests/test_gpu_dirsparse_edges_2d.py (tests/_dirsparse_2d_edge_cases.py, DESIGN.md
10n), checked on the NumPy restatement alone: every case keeps both decisions of the prox MARGIN = 5e-10 (relative) from
their thresholds, measured in long double on the v both sides form; the restatement names the same kind for every group in
double and in long double; every regime yields the kinds it is built for.  A seed that does not meet these is changed, not
excused.  Also the replay of the line-search rule for a trajectory whose groups are all dead.  No compute calls."""
import numpy as np
import pytest

import _dirsparse_2d_edge_cases as X

CASES = [(regime, param, mode, shape) for mode in X.MODES for regime, param in X.regimes(mode) for shape in X.SHAPES]
WORST = {}


@pytest.mark.parametrize("regime,param,mode,shape", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_edge_cases_keep_their_margins_and_their_kinds(regime, param, mode, shape):
    seen = set()
    m_alive = m_vote = np.inf
    gap, n_near = 0.0, 0
    for rows, lo, hi, case in X.all_cases(regime, param, mode, shape):
        for b in range(X.BATCH):
            tag = (regime, param, mode, shape, rows, lo, hi, b)
            alive, vote = X.margins(case, b)
            m_alive = min(m_alive, float(np.min(np.abs(alive))))
            m_vote = min(m_vote, float(np.min(np.abs(vote), initial=np.inf)))
            assert np.min(np.abs(alive)) >= X.MARGIN and (vote.size == 0 or np.min(np.abs(vote)) >= X.MARGIN), tag
            _, sr, kr = X.restate(case, b)
            _, sl, kl = X.restate(case, b, dtype=X.LD)
            kr = np.array(kr)
            assert list(kr) == kl, tag
            assert np.array_equal(kr != "zero", alive > 0.0), tag
            if vote.size:
                assert np.array_equal(kr[kr != "zero"] == "box", vote > 0.0), tag
            gap = max(gap, float(np.max(np.abs(sr - sl))))
            if regime == "edge":                  # the barely box-active groups sit far enough from s0 for the GPU test to tell
                near = np.zeros(kr.size, dtype=bool)
                near[kr != "zero"] = np.abs(vote) < 2e-9
                near &= kr == "box"
                moved = (X.closed_form_ld(case, b) - sl.ravel())[near]
                assert np.all(moved >= X.MOVED), tag
                n_near += int(near.sum())
            seen |= set(kr)
            if regime == "lam0":                  # group 0 is all zero; every other one is alive
                assert kr[0] == "zero" and np.all(kr[1:] != "zero"), tag
    print(f"{regime} {param} {mode} {shape}: min |c / lam - 1| {m_alive:.3e}  min vote margin {m_vote:.3e}  "
          f"|s_double - s_long double| {gap:.2e}  kinds {sorted(seen)}")
    assert n_near >= 8 or regime != "edge"
    if regime == "ratio":
        assert X.KINDS[regime] <= seen, seen
    elif regime in X.KINDS:
        assert seen == X.KINDS[regime], seen
    assert gap <= 1e-13                           # the restatement's own rounding is far below the 1e-12 the GPU test asks for


def test_zero_weight_grids_have_exact_zeros():
    rng = np.random.default_rng(1)
    for rows in X.ROWS:
        x, y, t = X.grids(rng, 70, 20, rows, "zero_t")
        wt = X.G1.trapz_w(t)
        assert t[0] == t[1] and wt[0] == 0.0 and np.all(np.diff(t) >= 0.0)
        assert (np.count_nonzero(wt == 0.0) == 2) == (rows >= 6)
    for regime, n in (("zero_x", 21), ("zero_y", 71)):
        x, y, t = X.grids(rng, 70, 20, 17, regime)
        assert np.count_nonzero(X.G.plane_w(x, y) == 0.0) == n


def test_replay_of_a_dead_trajectory():
    """Eleven failed rounds per iteration: alpha_k = 0.8^11 alpha_prev; growth 1.2, the boost 1.5 at k = 5, 10, 15, 20 (five
    equal costs in a row each time), the stop at the first k > 20."""
    al, stop = X.replay_dead(0.5, 24)
    assert stop == 21 and len(al) == 22
    assert al[0] == pytest.approx(0.5 * 0.8 ** 11, rel=1e-14)
    for k in range(1, 22):
        g = 1.5 if (k - 1) in (5, 10, 15, 20) else 1.2
        assert al[k] == pytest.approx(al[k - 1] * g * 0.8 ** 11, rel=1e-14), k
    assert X.replay_dead(0.5, 10)[1] is None
