"""Inputs of the 2D directional-sparsity seam tests, shared by the GPU test and by the CPU test that checks,
without a GPU, that the seeds keep every decision of the prox away from its threshold."""
import zlib

import numpy as np

import _group_prox_ref_2d as G

BOXES = ((-1.0, 1.0), (-0.3, 2.0), (0.0, 1.0), (-1.0, 0.0), (-np.inf, np.inf))
# tiles are 64 x 16, the pitch is ceil(nf / 8) * 8: one tile; 2 x 2 ragged tiles with a pad column and more nodes than a
# workgroup has threads; 1 x 5 tiles; 3 x 3 tiles
SHAPES = ((16, 16), (70, 20), (20, 70), (130, 40))
# below the 16 wavefronts of a pencil workgroup, ragged against them, several times their count
ROWS = (3, 17, 33)
BATCH = 2
ALPHA, KS = 0.5, 0.04                 # lam = 0.02; alpha a power of two and b3 = 0: v = u - alpha r is one rounding


def grids(rng, Nx, Ny, rows, triple_x=False):
    """Non-uniform x, y, t on [0, 1]; triple_x: one interior node of x three times (a line of nodes of weight zero)."""
    mk = lambda n: np.cumsum(np.r_[0.0, rng.uniform(0.5, 1.5, n - 1)])
    x, y, t = mk(Nx + 1), mk(Ny + 1), mk(rows)
    if triple_x:
        k = (Nx + 1) // 2
        x[k - 1] = x[k + 1] = x[k]
    return x / x[-1], y / y[-1], t / t[-1]


def seam_case(mode, Nx, Ny, rows, lo, hi, ks=KS, big=3.0, triple_x=False, tag=""):
    """u, r (BATCH, rows, Nx+1, Ny+1) whose gradient step v = u - alpha r holds groups of every kind, as the 1D _seam_case
    builds them: amplitude 0.005 (||v|| < lam = 0.02: zero; on a one-sided box also a large part on the wrong side), 0.05
    (closed form; one-signed where the box is one-sided) and `big` (box-active where the box is finite).  The seed is a
    function of the arguments."""
    key = f"{mode}/{Nx}/{Ny}/{rows}/{lo}/{hi}/{ks}/{big}/{triple_x}/{tag}"
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    x, y, t = grids(rng, Nx, Ny, rows, triple_x)
    shp = (BATCH, rows, Nx + 1, Ny + 1)
    ng = rows if mode == "time" else (Nx + 1) * (Ny + 1)
    cls = (np.arange(BATCH * ng).reshape(BATCH, ng) + rng.integers(3)) % 3
    cl = cls[:, :, None, None] if mode == "time" else cls.reshape(BATCH, 1, Nx + 1, Ny + 1)
    amp = np.choose(cl, [0.005, 0.05, big])
    z = rng.standard_normal(shp)
    if lo == 0.0 or hi == 0.0:
        sgn = 1.0 if lo == 0.0 else -1.0
        z = np.where(cl == 1, sgn * np.abs(z), z)
        wrong = (cl == 0) & (rng.random(shp) < 0.5)
        z = np.where(wrong, -sgn * 400.0 * np.abs(z), z)
    v = amp * z
    if triple_x:
        v[:, :, (Nx + 1) // 2, :] = 50.0          # entries on the nodes of weight zero
    r = rng.standard_normal(shp)
    return dict(mode=mode, u=v + ALPHA * r, r=r, alpha=ALPHA, ks=ks, lo=lo, hi=hi, x=x, y=y, t=t)


def decision_margins(case):
    """In long double, on the v the kernel forms (one rounding): the smallest |c / lam - 1| over all groups and the smallest
    |max|s0 v| / bound - 1| over the live groups and the finite non-zero bounds (a bound of 0 decides by a sign, exactly)."""
    L = np.longdouble
    mode, lo, hi = case["mode"], case["lo"], case["hi"]
    lam = L(case["alpha"]) * L(case["ks"])
    w = G.weights(mode, case["x"], case["y"], case["t"]).astype(L)
    m_c = m_b = np.inf
    for b in range(case["u"].shape[0]):
        v = G.groups(case["u"][b] - case["alpha"] * case["r"][b], mode).astype(L)
        cone = v.copy()
        if hi == 0.0:
            cone[cone > 0] = 0
        if lo == 0.0:
            cone[cone < 0] = 0
        c = np.sqrt(np.sum(w * cone * cone, axis=1))
        nv = np.sqrt(np.sum(w * v * v, axis=1))
        if lam > 0:
            m_c = min(m_c, float(np.min(np.abs(c / lam - 1))))
        live = c > lam
        s0 = 1 - lam / nv[live]
        if np.isfinite(hi) and hi != 0.0:
            m_b = min(m_b, float(np.min(np.abs(s0 * np.max(v[live], axis=1) / L(hi) - 1), initial=np.inf)))
        if np.isfinite(lo) and lo != 0.0:
            m_b = min(m_b, float(np.min(np.abs(s0 * np.min(v[live], axis=1) / L(lo) - 1), initial=np.inf)))
    return m_c, m_b


# ---- the resident loop ---------------------------------------------------------------------------------------------------
RES_SHAPE, STEPS, DT = (70, 20), 6, 1e-2
MODES = ["space", "full", "time", "space"]
BOX = [(-0.3, 2.0), (-1.0, 1.0), (-0.05, 0.08), (-0.35, 0.0)]           # the last one is one-sided
PHI_AMP = (0.01, 0.2, 0.05, 0.1)


def resident_problem(O2, Nx=RES_SHAPE[0], Ny=RES_SHAPE[1], steps=STEPS, batch=4):
    """P, phi0, phi_T (batch, Nx+1, Ny+1), t_hist and the warm start u0 (batch, steps+1, Nx+1, Ny+1): a few Fourier modes in
    x, y and t of amplitude up to 0.6 (outside every box of BOX but the full member's), levels 2 and 5, the pencils with
    0.2 <= x <= 0.3 and those of index = 3 mod 7 along y exactly zero."""
    P = O2.Params2D(Nx=Nx, Ny=Ny, T=steps * DT, dt_initial=DT)
    t_hist, _ = O2.time_grid(P.T, DT)
    t_hist = np.asarray(t_hist, dtype=np.float64)
    assert t_hist.size == steps + 1
    x, y = np.linspace(0.0, P.Lx, Nx + 1), np.linspace(0.0, P.Ly, Ny + 1)
    phi0 = np.stack([O2.init_phi_random(Nx, Ny, 1e-2, amp=PHI_AMP[b % 4], seed=40 + b) for b in range(batch)])
    phi_T = np.repeat(O2.build_targets(x, y, t_hist, phi0[0], P.Lx, P.Ly, P.T, 1, 1)[0][None], batch, axis=0)
    tt = (t_hist / t_hist[-1])[:, None, None]
    X, Y = x[None, :, None], y[None, None, :]
    u0 = np.stack([0.35 * np.sin(2 * np.pi * X + b) * np.cos(np.pi * Y) * np.cos(np.pi * tt) +
                   0.2 * np.sin(6 * np.pi * X - b) * np.sin(3 * np.pi * tt + 0.4) * np.cos(2 * np.pi * Y) +
                   0.08 * np.cos(10 * np.pi * X) * np.cos(5 * np.pi * tt + b) * np.ones_like(Y) for b in range(batch)])
    u0[:, [2, 5]] = 0.0
    u0[:, :, (x >= 0.2) & (x <= 0.3), :] = 0.0
    u0[:, :, :, 3::7] = 0.0
    return P, phi0, phi_T, t_hist, x, y, u0


def kappa_between(norms, q):
    """A threshold between two adjacent sorted group norms near the quantile q, in the middle of the widest relative gap
    of the five pairs around it: no group norm is closer to it than half that gap."""
    s = np.sort(norms[norms > 0.0])
    k = int(q * s.size)
    j = max(range(max(k - 2, 0), min(k + 3, s.size - 1)), key=lambda i: s[i + 1] / s[i])
    return float(0.5 * (s[j] + s[j + 1]))
