"""Inputs of the 1D off-default tests, shared by test_offpoint_1d_windows.py (CPU: every input lies inside its decision
window, asserted on the oracle alone) and test_gpu_1d_offpoint.py (the engine against the oracle on exactly these inputs).
Every oracle run is computed once (lru_cache) and never modified.

Two parameter points away from Lx = 1, c2 = 1 and the other defaults (oracle.Params1D):
    OFF   Lx 1.3, c2 0.5, gamma 3.0, kappa 1e-3, c1 0.9, tau 0.01     (the point of test_gpu_second_order_1d.py)
    OFF2  Lx 0.7, c2 1.4, gamma 0.5, kappa 4e-4, c1 0.6, tau 0.2
T = 0.045 with dt = 0.01: M = 5 steps, the last one ragged (5e-3).  xs = x / Lx."""
import functools

import numpy as np

from oracle import vch1d_oracle as O1

EPS = np.finfo(np.float64).eps
OFF = dict(Lx=1.3, c2=0.5, gamma=3.0, kappa=1e-3, c1=0.9, tau=0.01)
OFF2 = dict(Lx=0.7, c2=1.4, gamma=0.5, kappa=4e-4, c1=0.6, tau=0.2)
POINTS = {"default": {}, "off": OFF, "off2": OFF2}
T, DT, M = 0.045, 0.01, 5
MARGIN = 20.0                 # last residual norm of every Newton loop <= NEWTON_TOL / MARGIN (test_gpu_1d_levels.py)
MIN_MARGIN = 1e-6             # smallest decision margin of a path comparison: 1000 x the 1e-9 field tolerance
COST_GAP = 1e-6               # smallest relative cost gap of a PGD acceptance test

# march window: (point, start, control amplitude).  The first three are the cases the window was laid out for; the other
# amplitudes fill the B = 3 batches (BATCH: one engine has one parameter point) and must qualify like them.
MARCH = [("off", "smooth", 12.0), ("off2", "smooth", 12.0), ("off2", "sep", 12.0),
         ("off", "smooth", -9.0), ("off", "smooth", 7.0), ("off2", "smooth", -9.0)]
BATCH = {"off": [("off", "smooth", 12.0), ("off", "smooth", -9.0), ("off", "smooth", 7.0)],
         "off2": [("off2", "smooth", 12.0), ("off2", "sep", 12.0), ("off2", "smooth", -9.0)]}
MARCH_NS = (33, 64)
KNIFE = ("off2", "sep", 200.0)                      # N = 33: outside the window, properties only
KNIFE_BATCH = [("off2", "smooth", 12.0), KNIFE, ("off2", "sep", 12.0)]
# clipped-start window: a start with nodes beyond the clip value.  The first loop cannot find an admissible trial point
# (the Newton diagonal 2 c1 / (1 - phi^2) pins those nodes) and leaves through the line-search failure with the old
# state, so the post-step clip bites and the uniform mass shift is ~1e-3 instead of round-off: the only place where its
# divisor Lx shows.  Every later loop converges inside the march window.
# (Amplitude -9 leaves the window at N = 33 -- a later loop ends 1.0 x below the tolerance -- so -5 it is.)
CLIPPED = [("off2", "over", 12.0), ("off2", "over", -5.0), ("off2", "over", 7.0)]
CLIPPED_PROP = ("off", "over", 12.0)                # Lx > 1, N = 33: later loops end near the tolerance; properties only
# capped-step window: (point, N, seed)
CAPPED = [("default", 33, 2), ("off", 33, 2), ("off", 64, 0), ("off2", 33, 3)]
# PGD window
PGD_POINTS, PGD_NS, PGD_ITERS = ("off", "off2"), (33, 48), 4
PGD_OPT = dict(alpha_max=2e3, b1=1.5, b2=4.0, b3=3e-2, kappa_sparsity=2e-3, u_min=-0.4, u_max=0.25)
PGD_SHIFTS = (0.3, 0.9, 1.7)                        # phase of the second cosine of phi0, one per trajectory of the batch
BAND = 1e-6                                         # |r + b3 u| this close to the prox threshold: pattern not compared


def params(point, N):
    return O1.Params1D(N=N, T=T, dt_initial=DT, **POINTS[point])


def grid(P):
    x = np.linspace(0.0, P.Lx, P.N + 1)
    return x, x / P.Lx


def control(P, amp, rows=M + 2):
    xs = grid(P)[1]
    return amp * np.stack([np.cos(np.pi * xs * (1 + k % 3)) * np.sin(1 + k) for k in range(rows)])


def start(P, kind):
    xs = grid(P)[1]
    if kind == "smooth":
        return 0.2 * np.cos(np.pi * xs)
    if kind == "over":
        return 0.9999 * np.tanh((xs - 0.37) / 0.05) * np.tanh((0.81 - xs) / 0.06)
    return np.clip(0.985 * np.tanh((xs - 0.37) / 0.05) * np.tanh((0.81 - xs) / 0.06), -0.99, 0.99)


@functools.lru_cache(maxsize=None)
def march_case(point, kind, amp, N):
    """The oracle's banded march from `kind` without control ("nat"), with control(amp) ("u") and with the control cut to
    M rows, the hold-last branch F1:351-353 ("short"): (history, stats) each; cond_J the Skeel condition of the first
    step's matrix (x = 1, b = 0, as in test_gpu_1d_levels.py)."""
    P = params(point, N)
    phi0, u = start(P, kind), control(P, amp)
    out = dict(P=P, phi0=phi0, ctl=u)
    for tag, uu in (("nat", None), ("u", u), ("short", u[:M])):
        st = {}
        ph, x, t = O1.forward(P, control=uu, initial_phi=phi0, solver="banded", stats=st)
        out[tag] = (ph, st)
    out["x"], out["t"] = x, t
    out["cond_J"] = O1.cond_estimate(O1.newton_rows(phi0, DT, P, P.Lx / N), np.ones(2 * N + 2), np.zeros(2 * N + 2))
    return out


def march_tol(c):
    return max(1e-9, 20 * EPS * c["cond_J"])


def in_march_window(st, loops=M):
    """The conditions of the march window; returns (residual margin, min_margin)."""
    res = O1.NEWTON_TOL / max(st["last_norms"])
    ok = (len(st["exits"]) == loops and all(e[0] == "conv" for e in st["exits"]) and st["failed_ls"] == 0
          and res >= MARGIN and st["min_margin"] >= MIN_MARGIN)
    return ok, res, st["min_margin"]


def in_clipped_window(st):
    """First loop: line-search failure after one solve and 12 halvings, no admissible trial; the others as in the march
    window.  Returns (ok, residual margin of the later loops, min_margin)."""
    res = O1.NEWTON_TOL / max(st["last_norms"][1:])
    ok = (len(st["exits"]) == M and st["exits"][0] == ("failed_ls", 1, 12, 0) and st["failed_ls"] == 1
          and all(e[0] == "conv" for e in st["exits"][1:]) and res >= MARGIN and st["min_margin"] >= MIN_MARGIN)
    return ok, res, st["min_margin"]


def first_shift(c, tag="u"):
    """The uniform shift of the first step of a clipped-start march, read off the oracle's history: the loop returned
    the old state, so row 2 = clip(row 1) - shift."""
    ph = c[tag][0]
    d = np.clip(ph[1], -1 + O1.DELTA_SEP, 1 - O1.DELTA_SEP) - ph[2]
    assert np.ptp(d) < 4 * EPS
    return float(d.mean())


@functools.lru_cache(maxsize=None)
def capped_case(point, N, seed):
    """One Newton call whose first step is cut by the ceiling alpha = 0.9 amax < 1."""
    P = params(point, N)
    h = P.Lx / N
    xs = grid(P)[1]
    phi = np.clip(0.9 * np.random.default_rng(seed).standard_normal(N + 1), -0.97, 0.97)
    w_old, w_new = np.zeros(N + 1), 5.0 * np.cos(2 * np.pi * xs)
    mu = O1.mu_init(phi, 0.0, P, h)
    st = {}
    pn, mn, hist = O1.newton_step(phi, mu, w_old, w_new, 1e-2, P, h, solver="banded", return_history=True, stats=st)
    return dict(P=P, phi=phi, mu=mu, w_old=w_old, w_new=w_new, dt=1e-2, phi_new=pn, mu_new=mn, hist=np.array(hist), st=st)


def pgd_phi0(P, shift=0.3):
    xs = grid(P)[1]
    return 0.2 * np.cos(np.pi * xs) + 0.05 * np.cos(3 * np.pi * xs + shift)


@functools.lru_cache(maxsize=None)
def pgd_case(point, N, shift=0.3):
    P = params(point, N)
    Op = O1.OptParams1D(**PGD_OPT)
    phi0 = pgd_phi0(P, shift)
    st = {}
    res = O1.pgd(P, Op, n_iter=PGD_ITERS, solver="banded", initial_phi=phi0, stats=st)
    u_prev = O1.pgd(P, Op, n_iter=PGD_ITERS - 1, solver="banded", initial_phi=phi0).u
    # the alpha the last control was made with: the last search ran out, so alphas[-1] is one factor 0.8 smaller
    arg, band = prox_band(u_prev, res.r, Op, res.alphas_used[-1])
    return dict(P=P, Op=Op, phi0=phi0, res=res, st=st, band=band, zero_predicted=arg <= Op.kappa_sparsity)


def prox_band(u_prev, r, Op, alpha):
    """The last prox step is u = clip(soft(u_prev - alpha (r + b3 u_prev), alpha kappa)): a node of u is zero exactly
    where arg = |u_prev / alpha - (r + b3 u_prev)| <= kappa (for u_prev = 0: |r + b3 u| <= kappa).  Returns (arg, |arg -
    kappa|); the zero pattern is decided by round-off where the distance is ~0."""
    arg = np.abs(u_prev / alpha - O1.gradient(r, u_prev, Op.b3))
    return arg, np.abs(arg - Op.kappa_sparsity)
