"""The 2D adjoint sweep's launch schedule, restated from backward_pass (csrc/vch_engine2d.hip) for the tests, and the
synthetic inputs of tests/test_gpu_adjoint_long.py.  Nothing here needs a GPU; tests/test_adjoint_sched_cpu.py pins
the schedule by hand-worked cases and checks, with the oracle alone, that every input qualifies.

Schedule.  The sweep runs n = M-1 .. 0.  A level with dt <= 1e-14 is copied: no solve, no look, and the counter of steps
since the last look stands still.  Otherwise the host looks at the device state before the solve of level n when
  * it is the first solve of the sweep, or the one right after it (the first solve runs on the rigorous budget, with
    looks of its own every CG_CHUNK sweeps, and tells nothing about the schedule), or
  * steps_since_look >= 1 while guesses are on and M-1-n < ADJ_SETTLE (the orders of the guesses are being raised), or
  * steps_since_look >= ADJ_LOOK.
Guesses are on where both axes are powers of two (the stencil-free sweep) and neither VCH_ADJ_GUESS_OFF nor the safe
schedule is set; the GEMM grids have no settle phase.

Inputs.  Histories are given, not marched: Engine2D.backward and the oracle's backward take any history and time grid.
Fields are functions of the normalised coordinates xi = x/Lx, eta = y/Ly, so both grids see the same shapes.
  smooth level     a_n cos(pi k_n xi) cos(pi l_n eta + phase), a_n ~ 0.05: D = f''(phi) is constant to 1 %
  separated level  0.98 s_n tanh((xi - 0.37 - 1e-3 n)/0.05) tanh((0.81 - xi)/0.06) cos(pi eta), 0.98 <= s_n <= 1:
                   D spans -0.5 .. 36
Amplitudes, wavenumbers and the interface drift with the level n, so a level taken from the wrong row shows.
"""
import numpy as np

ADJ_LOOK, ADJ_SETTLE, CG_CHUNK = 8, 16, 24      # csrc/vch_engine2d.hip
GUESS_ORD, GUESS_BMAX = 8, 32                   # csrc/vch_kernels2d.h
MAG_MAX = 64.0                                  # backward_pass: sum |w| above this lowers the order
DT_ZERO = 1e-14                                 # B2:214: a step this short copies the level above

M = 50
DT = 1e-3
B1, B2 = 5.0, 10.0
#              Nx  Ny  Lx   Ly
GRIDS = {"fft": (32, 16, 1.0, 0.6),             # run-time FFT plan on both axes, guesses on, hx != hy
         "gemm": (20, 14, 1.3, 0.9)}            # MFMA GEMM transforms, no guesses
PHI_MAX = 1.0 - 1e-2 - 5e-3                     # 1 - DELTA_SEP - 5e-3: inside every clip of the engine and the oracle


def uses_guess(grid):
    Nx, Ny = GRIDS[grid][:2]
    return all(n >= 16 and n & (n - 1) == 0 for n in (Nx, Ny))


# ------------------------------------------------------------------------------------------------ schedule
def look_levels(M, guess, t_hist=None):
    """The levels n before whose solve backward_pass (safe = false) looks at the device state, in sweep order."""
    looks, since, first, again = [], 0, True, True
    for n in range(M - 1, -1, -1):
        if t_hist is not None and t_hist[n + 1] - t_hist[n] <= DT_ZERO:
            continue
        if again or since >= (1 if guess and M - 1 - n < ADJ_SETTLE else ADJ_LOOK):
            looks.append(n)
            since = 0
            again = False
        since += 1
        if first:
            first, again = False, True
    return looks


def steady_looks(M, guess, t_hist=None):
    """The looks of the steady phase (every ADJ_LOOK-th level)."""
    return [n for n in look_levels(M, guess, t_hist) if M - 1 - n >= (ADJ_SETTLE if guess else 2)]


def guess_weights(t_hist, n, mu):
    """Weights of the polynomial through the levels n+2k, k = 1..mu, evaluated at t_n (backward_pass), and sum |w|."""
    w = []
    for j in range(1, mu + 1):
        v = 1.0
        for k in range(1, mu + 1):
            if k != j:
                v *= (t_hist[n] - t_hist[n + 2 * k]) / (t_hist[n + 2 * j] - t_hist[n + 2 * k])
        w.append(v)
    return w, float(np.sum(np.abs(w)))


def orders_lowered(t_hist, mu=2):
    """Levels at which a guess of order mu has its levels in range and weights above MAG_MAX (the order must drop)."""
    Mh = len(t_hist) - 1
    return [n for n in range(Mh - 2 * mu, -1, -1) if guess_weights(t_hist, n, mu)[1] > MAG_MAX]


# ------------------------------------------------------------------------------------------------ time grids
def t_uniform(dt=DT):
    return np.concatenate([[0.0], np.cumsum(np.full(M, dt))])


def t_ragged(dt=DT, seed=11):
    rng = np.random.default_rng(seed)
    return np.concatenate([[0.0], np.cumsum(dt * (0.5 + rng.random(M)))])


def t_alternating(dt=DT, factor=50.0):
    """Steps s, s, L, L, s, s, .. with L = factor s = 5 dt.  The guesses take every second level, so plain alternation
    s, L, s, L gives them the uniform spacing s + L; in pairs the spacings are 2s and 2L, and the order-2 weights reach
    1 + 2 L/s = 101 > 64."""
    big = 5.0 * dt
    steps = np.where((np.arange(M) // 2) % 2 == 0, big / factor, big)
    return np.concatenate([[0.0], np.cumsum(steps)])


def t_zero(steps, dt=DT):
    """Uniform steps with the steps n in `steps` (t[n+1] - t[n]) of length zero."""
    d = np.full(M, dt)
    d[list(steps)] = 0.0
    return np.concatenate([[0.0], np.cumsum(d)])


def zero_places(grid):
    """Where case C puts zero-length steps: name -> steps."""
    s = steady_looks(M, uses_guess(grid))[1]
    return {"settle": (M - 10,), "after_look": (s - 1,), "two": (21, 20), "step0": (0,), "last": (M - 1,)}


# ------------------------------------------------------------------------------------------------ fields
def _coords(grid):
    Nx, Ny = GRIDS[grid][:2]
    return np.meshgrid(np.linspace(0.0, 1.0, Nx + 1), np.linspace(0.0, 1.0, Ny + 1), indexing="ij")


def smooth_level(grid, n, k=0):
    xi, eta = _coords(grid)
    a = 0.05 * (1.0 + 0.2 * np.sin(0.37 * n + 1.3 * k))
    return a * np.cos(np.pi * (1.0 + k + 0.5 * n / M) * xi) * np.cos(np.pi * (2.0 - 0.5 * n / M) * eta + 0.4 * k)


def sep_level(grid, n):
    xi, eta = _coords(grid)
    s = 1.0 - 0.01 * (1.0 + np.sin(0.4 * n))
    return 0.98 * s * np.tanh((xi - 0.37 - 1e-3 * n) / 0.05) * np.tanh((0.81 - xi) / 0.06) * np.cos(np.pi * eta)


def _hist(grid, w, k=0):
    """Levels (1 - w_n) smooth + w_n separated."""
    return np.stack([(1.0 - w[n]) * smooth_level(grid, n, k) + w[n] * sep_level(grid, n) for n in range(M + 1)])


def hist_smooth(grid, k=0):
    return _hist(grid, np.zeros(M + 1), k)


def hist_sep(grid):
    return _hist(grid, np.ones(M + 1))


def hist_jump(grid, n0):
    """Smooth at the levels n >= n0, separated below."""
    return _hist(grid, (np.arange(M + 1) < n0).astype(float))


RAMP = (30, 14)      # smooth from level 30 up, separated from level 14 down: 16 levels of the steady phase


def hist_ramp(grid, span=RAMP):
    hi, lo = span
    return _hist(grid, np.clip((hi - np.arange(M + 1)) / float(hi - lo), 0.0, 1.0))


def jump_levels(grid):
    """Case D: name -> n0.  L is a look of the steady phase with a full window of smooth levels before it."""
    L = steady_looks(M, uses_guess(grid))[1]
    return {"after_look": L - 1, "before_look": L - (ADJ_LOOK - 1), "last_solve": 1}


def targets(grid):
    """phi_Q (M + 1 levels) and phi_T, smooth and of order one against the smooth levels."""
    xi, eta = _coords(grid)
    pq = np.stack([0.3 * (1.0 - 0.5 * n / M) * np.cos(np.pi * xi) * np.cos(np.pi * eta) for n in range(M + 1)])
    return pq, 0.4 * np.cos(2.0 * np.pi * xi) * np.cos(np.pi * eta)


def march_input(grid):
    """A short forward march for case D's look at the counters: start field and steps."""
    return smooth_level(grid, 0) * 2.0, np.full(4, DT)


# ------------------------------------------------------------------------------------------------ the inputs by name
def inputs(dt=DT):
    """Every (grid, time grid, history) that the GPU module sweeps: name -> (grid, t_hist, history)."""
    out = {}
    for g in GRIDS:
        tu = t_uniform(dt)
        for k in (0, 1):
            out[f"{g}-uniform-smooth{k}"] = (g, tu, hist_smooth(g, k))
        out[f"{g}-uniform-sep"] = (g, tu, hist_sep(g))
        out[f"{g}-uniform-ramp"] = (g, tu, hist_ramp(g))
        for name, n0 in jump_levels(g).items():
            out[f"{g}-uniform-jump-{name}"] = (g, tu, hist_jump(g, n0))
        for name, steps in zero_places(g).items():
            tz = t_zero(steps, dt)
            out[f"{g}-zero-{name}-smooth0"] = (g, tz, hist_smooth(g, 0))
            out[f"{g}-zero-{name}-sep"] = (g, tz, hist_sep(g))
    for name, t in (("ragged", t_ragged(dt)), ("alternating", t_alternating(dt))):
        out[f"fft-{name}-smooth0"] = ("fft", t, hist_smooth("fft", 0))
        out[f"fft-{name}-sep"] = ("fft", t, hist_sep("fft"))
    for b in (0, 16, 32):
        out[f"fft-uniform-scaled{b}"] = ("fft", t_uniform(dt), (1.0 + 0.01 * b) * hist_smooth("fft", b % 2))
    return out


# ------------------------------------------------------------------------------------------------ oracle
def params(O2, grid, t_hist):
    Nx, Ny, Lx, Ly = GRIDS[grid]
    return O2.Params2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, T=float(t_hist[-1]), dt_initial=float(np.max(np.diff(t_hist))))


_ORACLE = {}


def oracle_sweep(O2, grid, t_hist, hist):
    """The oracle's (p, q, r) of a history under targets(grid), computed once per input and never modified."""
    key = (grid, t_hist.tobytes(), hist.tobytes())
    if key not in _ORACLE:
        Nx, Ny, Lx, Ly = GRIDS[grid]
        pq, pt = targets(grid)
        out = O2.backward(hist, np.linspace(0, Lx, Nx + 1), np.linspace(0, Ly, Ny + 1), t_hist, params(O2, grid, t_hist),
                          B1, B2, pq, pt)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def step_residuals(O2, grid, t_hist, hist, p):
    """Relative residuals of p in the terminal equation (I - tau L) p_M = b2 (phi_M - phi_T) [entry M] and in the step
    equations A(phi_n) p_n = B(phi_n+1) p_n+1 + src [entry n; NaN at a zero-length step]."""
    Nx, Ny, Lx, Ly = GRIDS[grid]
    hx, hy = Lx / Nx, Ly / Ny
    P = params(O2, grid, t_hist)
    pq, pt = targets(grid)
    res = np.full(M + 1, np.nan)
    term = B2 * (hist[M] - pt)
    res[M] = np.linalg.norm(p[M] - P.tau * O2.lap(p[M], hx, hy) - term) / np.linalg.norm(term)
    for n in range(M):
        dt = t_hist[n + 1] - t_hist[n]
        if dt <= DT_ZERO:
            continue
        rhs = O2.adjoint_B_apply(hist[n + 1], p[n + 1], dt, P, hx, hy) + 0.5 * dt * B1 * (hist[n] - pq[n] + hist[n + 1] - pq[n + 1])
        res[n] = np.linalg.norm(O2.adjoint_A_apply(hist[n], p[n], dt, P, hx, hy) - rhs) / np.linalg.norm(rhs)
    return res
