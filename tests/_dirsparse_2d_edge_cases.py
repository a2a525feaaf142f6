"""Inputs of the 2D directional-sparsity edge tests, shared by the GPU test and by the CPU test that checks,
without a GPU, that every case keeps its decisions MARGIN from their thresholds: the builders of tests/_group_edge_cases.py
(the 1D edge tests' own) applied to the levels (planes under the product weights W_ij = wx_i wy_j) or the pencils (under
wt) of a (rows, Nx+1, Ny+1) control.  The seed is a function of the arguments; grids are non-uniform; b3 = 0 and the steps
are powers of two, so v = u - alpha r is one rounding on both sides."""
import zlib

import numpy as np

import _dirsparse_2d_cases as K
import _group_edge_cases as E
import _group_prox_ref as G1
import _group_prox_ref_2d as G

LD = np.longdouble
MARGIN = E.MARGIN
BOXES = K.BOXES
# tiles are 64 x 16: one tile; ragged 2 x 2 tiles with a pad column; 3 x 3 tiles
SHAPES = ((16, 16), (70, 20), (130, 40))
# below, at, past and past twice the sixteen wavefronts of a pencil workgroup
ROWS = (3, 16, 17, 33)
BATCH = 2
ALPHAS = np.array([0.5, 2.0])         # a step per trajectory
KS = 0.04
RATIOS = (1e3, 1e6, 1e9)
MODES = ("time", "space")

BUILD = {"alive": E.build_alive, "edge": E.build_edge, "ratio": E.build_mixed, "lam0": E.build_lam0, "zero_x": E.build_zero_weight,
         "zero_y": E.build_zero_weight, "zero_t": E.build_zero_weight}
# the kinds a regime must yield over the rows and boxes of one (mode, shape); ratio: at least these
KINDS = {"alive": {"zero", "closed", "box"}, "edge": {"closed", "box"}, "ratio": {"closed", "box"},
         "zero_x": {"zero", "closed", "box"}, "zero_y": {"zero", "closed", "box"}, "zero_t": {"zero", "closed", "box"}}


def regimes(mode):
    """The (regime, param) pairs of a mode: a weightless line of x or of y nodes in "time", weightless levels in "space"."""
    zero = [("zero_x", None), ("zero_y", None)] if mode == "time" else [("zero_t", None)]
    return [("alive", None), ("edge", None)] + [("ratio", q) for q in RATIOS] + [("lam0", None)] + zero


def boxes_of(regime):
    return BOXES[:4] if regime == "edge" else BOXES


def _triple(a):
    """An interior node three times: one weight exactly zero between two halved ones."""
    j = a.size // 2
    a[j + 1:] -= a[j + 1] - a[j]
    a[j + 2:] -= a[j + 2] - a[j]
    assert a[j] == a[j + 1] == a[j + 2]


def grids(rng, Nx, Ny, rows, regime):
    """Non-uniform x, y, t scaled to [0, 1].  zero_x / zero_y: a node of x / y three times.  zero_t: t[0] == t[1] (as in a
    1D history) and, from six levels on, an interior level three times: wt has exact zeros."""
    mk = lambda n: np.cumsum(np.r_[0.0, rng.uniform(0.5, 1.5, n - 1)])
    x, y, t = mk(Nx + 1), mk(Ny + 1), mk(rows)
    if regime == "zero_x":
        _triple(x)
    if regime == "zero_y":
        _triple(y)
    if regime == "zero_t":
        t[1:] -= t[1]
        if rows >= 6:
            _triple(t)
    x, y, t = x / x[-1], y / y[-1], t / t[-1]
    if regime == "zero_x":
        assert np.count_nonzero(G.plane_w(x, y) == 0.0) == Ny + 1
    if regime == "zero_y":
        assert np.count_nonzero(G.plane_w(x, y) == 0.0) == Nx + 1
    if regime == "zero_t":
        assert np.count_nonzero(G1.trapz_w(t) == 0.0) == (2 if rows >= 6 else 1)
    return x, y, t


def edge_case(regime, mode, Nx, Ny, rows, lo, hi, param=None):
    """u, r (BATCH, rows, Nx+1, Ny+1), the steps alpha (BATCH,), kappa_s and the grids of one seam call."""
    key = f"edges/{regime}/{param}/{mode}/{Nx}/{Ny}/{rows}/{lo}/{hi}"
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    x, y, t = grids(rng, Nx, Ny, rows, regime)
    ks = {"ratio": 0.5 / (param or 1.0), "lam0": 0.0}.get(regime, KS)
    w = G.weights(mode, x, y, t)
    shp = (rows, Nx + 1, Ny + 1)
    ng, m = (rows, shp[1] * shp[2]) if mode == "time" else (shp[1] * shp[2], rows)
    vg = [BUILD[regime](rng, ng, m, w, ALPHAS[b] * ks, lo, hi) for b in range(BATCH)]
    v = np.stack([G.ungroup(g, shp, mode) for g in vg])
    if regime == "lam0":
        r = np.where(v == 0.0, 0.0, rng.standard_normal(v.shape))
    else:
        r = rng.standard_normal(v.shape) * np.sqrt(np.mean(v * v, axis=(1, 2, 3)))[:, None, None, None]
        dead = np.stack([G.ungroup(np.broadcast_to(~g.any(axis=1)[:, None], g.shape), shp, mode) for g in vg])
        r = np.where(dead, 0.0, r)                   # an all-zero group stays one
    u = v + ALPHAS[:, None, None, None] * r
    return dict(regime=regime, mode=mode, u=u, r=r, alpha=ALPHAS.copy(), ks=ks, lo=lo, hi=hi, x=x, y=y, t=t, w=w)


def formed_v(case, b):
    """The v both sides form: one rounding of u - alpha r (alpha a power of two, b3 = 0)."""
    return case["u"][b] - case["alpha"][b] * case["r"][b]


def margins(case, b):
    """_margins of trajectory b in long double: c / lam - 1 of every group, and the vote margin of the live ones."""
    return E._margins(G.groups(formed_v(case, b), case["mode"]), case["w"], case["alpha"][b] * case["ks"], case["lo"], case["hi"])


def restate(case, b, dtype=np.float64):
    """(u+, s, kinds) of the restatement for trajectory b; s is (rows,) or (Nx+1, Ny+1)."""
    c = case
    return G.prox(c["u"][b], c["r"][b], c["alpha"][b], 0.0, c["ks"], c["lo"], c["hi"], c["mode"], c["x"], c["y"], c["t"], dtype=dtype)


MOVED = 64 * 2.0 ** -53              # 64 ulps of a number below 1


def closed_form_ld(case, b):
    """s0 = 1 - lam / ||v|| of every group in long double (flat, in group order): what a kernel that votes "closed form"
    returns to a few ulps.  Where the restatement says box-active, the root lies below s0 by delta = s0 - s, about
    (lam / ||v||) x (the clipped entries' share of ||s0 v||^2) x the vote margin: 7e-14 and more at a margin of 1e-9 on
    these grids, below the 1e-12 asked of s but far above its rounding (4e-16).  A wrong vote at the edge is visible only
    against this."""
    vg = G.groups(formed_v(case, b), case["mode"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1.0 - LD(case["alpha"][b] * case["ks"]) / E._ldnorm(vg, case["w"])


def all_cases(regime, param, mode, shape):
    Nx, Ny = shape
    for rows in ROWS:
        for lo, hi in boxes_of(regime):
            yield rows, lo, hi, edge_case(regime, mode, Nx, Ny, rows, lo, hi, param)


# ---- the resident loops (problems: K.resident_problem; kappa_s of a group member: K.kappa_between) ---------------------------
# B1: (130, 40), 17 levels in a context built for 41; a full run of two at index 0, a run of one at the end
B1 = dict(shape=(130, 40), steps=16, max_steps=40, modes=["full", "full", "time", "space", "time", "full"],
          box=[(-1.0, 1.0), (-0.5, 0.7), (-0.3, 2.0), (-0.35, 0.0), (-0.05, 0.08), (-0.2, 0.2)],
          b3=(1e-4, 1e-4, 2.0, 1e-4, 1e-4, 1e-4), alpha0=(30.0, 12.0, 2.0, 5.0, 8.0, 20.0),
          alpha_max=(100.0, 100.0, 50.0, 2.0, 8.0, 40.0), overshoot=2)
# B2: (20, 70) (1 x 5 tiles), 33 levels: a third trip of the pencil loops; the full run at the end.  The time member's box
# was picked on the CPU with the restatement's loop over the oracle: u0 reaches 0.63, and under the boxes (-0.05, 0.08) and
# (-0.3, 0.4) the forced projection alone raises this member's cost, so that none of the eleven trials descends; under
# (-0.4, 0.5) the first trial descends (0.645176 -> 0.645098) with 9 box-active, 23 closed-form levels and a zero one.
B2 = dict(shape=(20, 70), steps=32, max_steps=32, modes=["time", "space", "full"],
          box=[(-0.4, 0.5), (-0.3, 2.0), (-1.0, 1.0)], b3=(1e-4, 1e-4, 1e-4), alpha0=(8.0, 5.0, 30.0),
          alpha_max=(50.0, 50.0, 100.0), overshoot=None)
# B3: (16, 16), 4 levels, from u = 0: members 0 and 1 have every group dead.  Members 2 and 3 keep moving: under the box
# (-1, 1) and steps of at most 1 their control grows by the same amount per iteration (max|u| = 0.70 and 0.006 after 24
# iterations of the restatement's loop over the oracle), so the change falls like 1 / k, 0.043 at k = 23, and the stop rule
# (change < 1e-5) has nothing to act on.
B3 = dict(shape=(16, 16), steps=3, max_steps=3, modes=["time", "space", "full", "time"], iters=24,
          box=[(-0.3, 2.0), (-0.35, 0.0), (-1.0, 1.0), (-1.0, 1.0)], alpha_max=(0.5, 2.0, 1.0, 1.0))


def cold_problem(O2, Nx, Ny, steps, batch):
    """K.resident_problem without its warm start (whose zero levels 2 and 5 need six levels): P, phi0, phi_T, t_hist, x, y."""
    P = O2.Params2D(Nx=Nx, Ny=Ny, T=steps * K.DT, dt_initial=K.DT)
    t_hist = np.asarray(O2.time_grid(P.T, K.DT)[0], dtype=np.float64)
    assert t_hist.size == steps + 1
    x, y = np.linspace(0.0, P.Lx, Nx + 1), np.linspace(0.0, P.Ly, Ny + 1)
    phi0 = np.stack([O2.init_phi_random(Nx, Ny, 1e-2, amp=K.PHI_AMP[b % 4], seed=40 + b) for b in range(batch)])
    phi_T = np.repeat(O2.build_targets(x, y, t_hist, phi0[0], P.Lx, P.Ly, P.T, 1, 1)[0][None], batch, axis=0)
    return P, phi0, phi_T, t_hist, x, y


def replay_dead(alpha_max, n_iter, alpha0=None):
    """vch_pgd.h's 2D rule for a trajectory none of whose trials ever descends and whose cost and control never move (every
    group dead): per iteration the eleven rounds (one optimistic, ten backtracking) all fail, the last try is returned with
    alpha reduced once more (0.8^11 alpha_prev, the products taken one at a time as the state machine takes them),
    attempts = 10, change = 0; alpha_prev grows by 1.2, or by 1.5 once five equal costs in a row have been seen (the count
    then restarts), capped at alpha_max; the stop needs change < 1e-5 and k > 20.  -> (alphas, the index of the stop
    iteration or None)."""
    prev = alpha_max if alpha0 is None else min(alpha0, alpha_max)
    alphas, plateau, stop = [], 0, None
    for k in range(n_iter):
        a = prev
        for _ in range(10):
            a *= 0.8
        a_k = a * 0.8
        alphas.append(a_k)
        plateau = plateau + 1 if k > 0 else 0
        boost = plateau >= 5
        prev = min(alpha_max, a_k * (1.5 if boost else 1.2))
        if boost:
            plateau = 0
        if k > 20:
            stop = k
            break
    return alphas, stop
