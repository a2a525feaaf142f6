"""vch1d_second_order / vch1d_hessvec at every cyclic-reduction depth and on long, ragged marches: the transposed solve cr_solve<2>
(row0<2>, with its mirrored weights at i = 1 and i = n - 2) and the tangent solves cr_solve<0> of k1d_tangent and k1d_hessvec
over every N of test_gpu_1d_levels.NS (every depth, every residue of N mod 2^lvl, the full-LDS row count nr = 1025 at each
depth), against the CPU references of tests/_adjoint_ref_1d.py and tests/_tangent_ref_1d.py on the engine's own history.

Size matrix: every N of NS at two points, the defaults and OFF of test_gpu_second_order_1d.py (Lx 1.3), M = 2 steps of
1.0e-2 and 3.5e-3, batch 2 (a white-noise direction, a smooth one), starts and controls of _problem.
Ragged cases: steps base (0.4 + 1.2 default_rng(5).random(M)), base 1e-2 (the largest 3.5 times the smallest), batch 3
(white noise, smooth, a second white noise), per-trajectory WEIGHTS, max_steps = M + 7:
    r2049_off   N = 2049, OFF, M = 12     depth 1, residue 1, full LDS
    r4096       N = 4096, defaults, M = 12   depth 2, full LDS
    r33_long    N = 33, OFF, M = 24       depth 0

Every case checks: hessvec's grad and hv against adjoint_reference_1d; second_order's dphi and d2phi against
tangent_reference_1d; identity 1 (sum G h = slope) and 2 (sum h Hh = curvature) against second_order on the same context;
the pair identity sum h0 H h1 = sum h1 H h0 of one shared base point (trajectory 1's), which a wrong transpose breaks;
the device's gh and hHh within n eps sum|terms| of the host's sums (n the number of terms: derived, not measured).

Tolerances: the depth's TOL of test_gpu_hessvec_1d.py (grad, hv, identities) and test_gpu_second_order_1d.py (dphi,
d2phi).  A case that misses one gets OWN[case] = 10 x its deviation measured on an MI355X; the assertion at import keeps
OWN at or below the CPU floors FLOOR_D1, FLOOR_D2 and FLOOR_S.  test_cases_meet_their_premises (no GPU) shows with
o.forward(dts=..., solver="banded") that every Newton call of the ragged cases converges, that max|phi[1:]| stays below
1 - DELTA_SEP - 0.1 and that the four identities of test_adjoint_cpu_1d.py hold for the references at these sizes;
test_many_chunk_march_meets_its_premise shows the same for the march of test_gpu_krylov_grid_1d.many_chunks (N = 4096,
M = 255).  The identities are asserted at CPU_ID = 10 x measured with a floor of one EPS = 2.2e-16 (the convention of
test_adjoint_cpu_1d.py, where a measured 0 must not give a bound of 0); the floor, not 10 x measured, sets 8 of the 16
bounds (see CPU_MEASURED).

Measured on an MI355X (MEASURED below): worst grad / hv / dphi / d2phi / identities
    depth 0, N <= 33 and r33_long   1.8e-15 / 1.3e-15 / 7.4e-16 / 2.5e-15 / 2.7e-16
    depth 0, N = 511 ... 1024       4.6e-13 / 2.9e-13 / 1.8e-13 / 7.2e-13 / 4.2e-14
    depth 1 and r2049_off           2.8e-12 / 9.9e-13 / 7.4e-13 / 2.8e-12 / 8.0e-14
    depth 2 and r4096               1.4e-11 / 8.6e-12 / 6.8e-12 / 2.3e-11 / 1.8e-13
The depth's TOL was measured at one N (N <= 33 at depth 0), and the distance between two backward-stable solves grows with
N: 19 of the 45 cases miss a quantity's TOL and carry OWN for it, with the reference's own spread beside it (REF_SPREAD;
the ratios are stated there).  The pair identity is at most
9.6e-15 everywhere.  CPU, the references' identities on the oracle's march: CPU_MEASURED.

That the tests can fail: mutants of the engine that change arithmetic, never an address, built beside the tree and never
committed; every test not named passes under each:
  1. kr1_sum (and its copies in k1d_ncg_fin and k1d_nt_fin) reading only the first KR1_T partials: nothing here fails (no
     streaming kernel runs in these calls), nor in test_gpu_krylov_1d.py, test_gpu_hess_cg_1d.py, test_gpu_newton_1d.py or
     the grid rounds; the many_chunks tests of test_gpu_krylov_grid_1d.py fail.
  2. k1d_hessvec's back-update with al, kd and 1/dt of dts[min(k + 1, M - 1)]: fails r2049_off (grad 1.7e-1, hv 1.1e-1,
     identities 3.3e-3), r4096 (1.7e-1, 1.1e-1, 2.8e-3), r33_long (6.8e-1, 4.3e-1, 5.2e-2), and in test_gpu_hessvec_1d.py
     n33_off, whose last step is ragged (grad 3.9e-1), and its per-trajectory weights test; passes the uniform n32, n1030,
     n2051 and the whole size matrix: at M = 2 the step after step 0 is the last one, so the mutant reads the right step.
  3. cr_solve's implicit levels without the upper neighbour of node n - 2 when SYS == 2: fails the size matrix at N = 1026,
     1500, 2048, 2050, 4094 and 4096 at both points (grad 3.7e-1 ... 3.9e-1, hv 4e-2 ... 2.5e-1) and r4096 (grad 2.5e-1):
     the even N at depth >= 1, where n - 2 is odd and so solved on the last implicit level (sp = 1; at odd N it is an
     explicit row or has no upper neighbour at its level).  Also n1030 of test_gpu_hessvec_1d.py (grad 3.0e-1) and the
     many_chunks Lanczos and CG tests (N = 4096; Ritz values 7.9e-1).  Passes depth 0, the odd N, r2049_off and r33_long."""
import numpy as np
import pytest

from oracle import vch1d_oracle as o
from _adjoint_ref_1d import adjoint_reference_1d
from _tangent_ref_1d import tangent_reference_1d, tangent_scalars_1d
from test_gpu_1d_levels import NS, _depth
from test_gpu_hessvec_1d import TOL as HV_TOL
from test_gpu_second_order_1d import OFF, TOL as SO_TOL, WEIGHTS, V, _engine  # noqa: F401  (V: fixture)
from test_tangent_cpu_1d import FLOOR_D1, FLOOR_D2, FLOOR_S

gpu = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
STEPS = (1.0e-2, 3.5e-3)
POINTS = {"def": {}, "off": OFF}
MATRIX = [f"{N}_{p}" for N in NS for p in POINTS]
RAGGED = {
    #             N     parameters  M
    "r2049_off": (2049, OFF, 12),
    "r4096":     (4096, {}, 12),
    "r33_long":  (33, OFF, 24),
}
BASE, SPARE = 1e-2, 7

# measured on an MI355X (the MEASURE lines of this file): worst deviation (grad, hv, dphi, d2phi, identities) per case
MEASURED = {
    "2_def": (2.39e-16, 9.47e-17, 1.87e-16, 2.46e-16, 2.04e-16), "2_off": (5.44e-16, 1.51e-16, 4.78e-16, 5.73e-16, 2.74e-16),
    "3_def": (3.39e-16, 5.89e-17, 1.48e-16, 4.05e-16, 2.53e-16), "3_off": (3.84e-16, 2.29e-16, 2.12e-16, 7.04e-16, 1.80e-16),
    "24_def": (1.06e-15, 2.83e-16, 3.26e-16, 1.05e-15, 1.94e-16), "24_off": (1.78e-15, 9.17e-16, 7.41e-16, 2.53e-15, 1.13e-16),
    "511_def": (9.68e-14, 6.22e-15, 3.35e-14, 1.17e-13, 1.03e-14), "511_off": (4.54e-14, 7.27e-14, 3.30e-14, 5.26e-14, 6.36e-15),
    "512_def": (8.21e-14, 5.47e-15, 2.08e-14, 1.00e-13, 2.44e-15), "512_off": (5.85e-14, 1.24e-13, 6.81e-14, 1.01e-13, 1.01e-15),
    "513_def": (5.46e-14, 8.13e-15, 3.23e-14, 1.40e-13, 1.85e-15), "513_off": (3.56e-14, 5.28e-14, 3.04e-14, 5.72e-14, 3.05e-15),
    "1023_def": (2.49e-13, 1.09e-14, 9.61e-14, 2.74e-13, 4.16e-14), "1023_off": (1.58e-13, 2.90e-13, 1.56e-13, 5.55e-13, 2.14e-14),
    "1024_def": (4.56e-13, 4.32e-14, 1.81e-13, 7.21e-13, 6.55e-15), "1024_off": (1.69e-13, 2.19e-13, 1.80e-13, 3.89e-13, 2.22e-14),
    "1025_def": (2.40e-13, 1.68e-14, 8.77e-14, 3.24e-13, 2.68e-14), "1025_off": (1.15e-13, 2.02e-13, 1.58e-13, 4.37e-13, 2.73e-14),
    "1026_def": (3.50e-13, 3.59e-14, 1.73e-13, 6.56e-13, 3.93e-14), "1026_off": (1.02e-13, 3.34e-13, 1.66e-13, 6.94e-13, 4.55e-14),
    "1500_def": (4.80e-13, 3.80e-14, 2.53e-13, 4.51e-13, 2.27e-14), "1500_off": (1.89e-13, 3.08e-13, 1.77e-13, 4.76e-13, 2.34e-14),
    "2047_def": (2.76e-12, 2.58e-13, 6.32e-13, 2.76e-12, 3.69e-14), "2047_off": (4.33e-13, 4.68e-13, 4.03e-13, 8.57e-13, 3.55e-14),
    "2048_def": (1.91e-12, 1.07e-13, 3.88e-13, 8.76e-13, 1.61e-14), "2048_off": (4.04e-13, 9.89e-13, 7.39e-13, 1.97e-12, 7.96e-14),
    "2049_def": (2.79e-12, 1.45e-13, 4.41e-13, 1.88e-12, 1.13e-14), "2049_off": (6.42e-13, 9.75e-13, 4.96e-13, 1.10e-12, 4.29e-14),
    "2050_def": (1.80e-12, 9.31e-14, 4.31e-13, 1.05e-12, 3.10e-15), "2050_off": (5.36e-13, 4.43e-13, 3.08e-13, 1.02e-12, 4.61e-14),
    "2051_def": (2.10e-12, 6.27e-14, 3.19e-13, 1.26e-12, 2.77e-14), "2051_off": (3.67e-13, 3.93e-13, 3.27e-13, 9.56e-13, 4.66e-14),
    "3001_def": (3.67e-12, 2.32e-13, 7.27e-13, 3.61e-12, 1.34e-13), "3001_off": (7.08e-13, 9.69e-13, 9.19e-13, 2.89e-12, 7.76e-14),
    "4093_def": (4.79e-12, 5.19e-13, 2.87e-12, 5.16e-12, 6.04e-15), "4093_off": (2.69e-12, 8.61e-12, 4.64e-12, 2.33e-11, 1.17e-13),
    "4094_def": (1.37e-11, 1.05e-12, 5.65e-12, 1.92e-11, 1.55e-13), "4094_off": (2.68e-12, 6.26e-12, 4.16e-12, 9.18e-12, 1.08e-13),
    "4095_def": (8.47e-12, 7.05e-13, 3.46e-12, 1.41e-11, 7.32e-14), "4095_off": (2.65e-12, 4.46e-12, 3.81e-12, 1.06e-11, 1.78e-13),
    "4096_def": (5.95e-12, 4.08e-13, 1.51e-12, 9.89e-12, 9.65e-14), "4096_off": (4.34e-12, 8.27e-12, 6.76e-12, 1.99e-11, 4.75e-14),
    "r2049_off": (2.71e-13, 3.50e-14, 2.30e-13, 6.16e-13, 9.20e-16), "r4096": (1.84e-12, 5.55e-13, 1.08e-12, 8.80e-12, 2.09e-15),
    "r33_long": (9.82e-16, 1.30e-15, 7.32e-16, 1.19e-15, 1.88e-16),
}
# Own bounds of the cases that miss the depth's TOL, for the quantities they miss (g grad, hv, d1 dphi, d2 d2phi, id the
# identities): 10 x MEASURED, rounded up.  The depth-0 TOL was measured at N <= 33 and the depth-1 and depth-2 TOL at one N
# each; the distance between two backward-stable solves grows with the conditioning of the step matrices, so with N.
# REF_SPREAD: the reference's own spread at that N, hp_solve against plain banded LU on the oracle's history of the same case
# (trajectories 0 and 1; grad, hv, dphi, d2phi), computed on the CPU.  MEASURED over REF_SPREAD, for the own-bound
# quantities: grad 1.2 ... 10 (2048_def 10.1, 2049_def 8.6, 2047_def 7.2); hv 0.04 ... 0.3, but 3.7 at 1024_def; dphi and
# d2phi 0.002 ... 0.1, but 15 at 4094_def dphi (5.65e-12 against 3.66e-13).
OWN = {
    "511_def": dict(g=9.8e-13, d1=3.4e-13, d2=1.2e-12, id=1.1e-13),
    "511_off": dict(g=4.6e-13, hv=7.4e-13, d1=3.4e-13, d2=5.3e-13, id=6.4e-14),
    "512_def": dict(g=8.3e-13, d1=2.1e-13, d2=1.1e-12, id=2.5e-14),
    "512_off": dict(g=5.9e-13, hv=1.3e-12, d1=6.9e-13, d2=1.1e-12),
    "513_def": dict(g=5.5e-13, hv=8.2e-14, d1=3.3e-13, d2=1.5e-12),
    "513_off": dict(g=3.6e-13, hv=5.4e-13, d1=3.1e-13, d2=5.8e-13, id=3.1e-14),
    "1023_def": dict(g=2.6e-12, hv=1.1e-13, d1=9.7e-13, d2=2.8e-12, id=4.2e-13),
    "1023_off": dict(g=1.6e-12, hv=3.0e-12, d1=1.6e-12, d2=5.6e-12, id=2.2e-13),
    "1024_def": dict(g=4.6e-12, hv=4.4e-13, d1=1.9e-12, d2=7.3e-12, id=6.6e-14),
    "1024_off": dict(g=1.7e-12, hv=2.3e-12, d1=1.9e-12, d2=4.0e-12, id=2.3e-13),
    "2047_def": dict(g=2.8e-11, d2=2.8e-11),
    "2048_def": dict(g=2.0e-11),
    "2048_off": dict(hv=1.0e-11, d1=7.5e-12),
    "2049_def": dict(g=2.9e-11),
    "2049_off": dict(hv=9.8e-12),
    "4093_off": dict(d1=4.7e-11),
    "4094_def": dict(d1=5.7e-11),
    "4094_off": dict(d1=4.2e-11),
    "4096_off": dict(d1=6.8e-11),
}
REF_SPREAD = {
    "511_def": (2.53e-14, 6.13e-14, 1.47e-11, 2.60e-11), "511_off": (2.72e-14, 5.92e-13, 5.52e-12, 1.24e-11),
    "512_def": (3.49e-14, 1.15e-14, 2.34e-12, 6.09e-12), "512_off": (2.53e-14, 7.35e-13, 4.56e-12, 1.57e-11),
    "513_def": (3.75e-14, 6.62e-14, 1.57e-11, 2.61e-11), "513_off": (2.89e-14, 1.87e-13, 2.90e-12, 2.38e-12),
    "1023_def": (6.10e-14, 5.64e-14, 1.79e-11, 2.71e-11), "1023_off": (7.34e-14, 2.56e-12, 2.27e-11, 3.82e-11),
    "1024_def": (1.18e-13, 1.17e-14, 3.71e-12, 7.77e-12), "1024_off": (3.44e-14, 3.45e-12, 2.75e-11, 3.72e-11),
    "2047_def": (3.81e-13, 1.21e-12, 2.48e-10, 6.89e-10), "2048_def": (1.90e-13, 4.58e-14, 9.18e-12, 3.38e-11),
    "2048_off": (1.36e-13, 2.17e-11, 2.14e-10, 4.31e-10), "2049_def": (3.25e-13, 1.18e-12, 2.44e-10, 6.73e-10),
    "2049_off": (1.55e-13, 5.20e-12, 8.72e-11, 1.75e-10), "4093_off": (8.00e-13, 1.42e-10, 8.73e-10, 1.77e-09),
    "4094_def": (1.23e-12, 4.80e-15, 3.66e-13, 1.16e-12), "4094_off": (1.06e-12, 1.70e-11, 1.05e-10, 2.20e-10),
    "4096_off": (4.16e-13, 1.29e-10, 7.92e-10, 1.63e-09),
}
_FLOOR = dict(g=FLOOR_D1, hv=FLOOR_D1, d1=FLOOR_D1, d2=FLOOR_D2, id=FLOOR_S)
for _name, _o in OWN.items():
    assert _name in REF_SPREAD and all(v <= _FLOOR[k] for k, v in _o.items()), _name

# the reference's own identities on the oracle's march (test_cases_meet_their_premises, test_many_chunk_march_meets_its_premise),
# measured on the CPU: gh, hHh, polar, sym.  Asserted at 10 x measured with a floor of one EPS, the convention of
# test_adjoint_cpu_1d.py and a departure from a plain 10 x: a measured 0 leaves no room at all, and one rounding of the sum
# itself is the least a relative deviation can be held to.  The floor sets the bound in 8 of the 16 values (those below
# 2.2e-17: r2049_off gh, hHh, polar; r4096 sym; r33_long polar; many_chunks gh, polar, sym).
CPU_MEASURED = {"r2049_off": (3.22e-18, 0.0, 1.99e-17, 2.55e-17), "r4096": (1.17e-16, 1.22e-16, 8.37e-17, 1.47e-17),
                "r33_long": (3.12e-17, 4.42e-17, 5.90e-18, 4.13e-17), "many_chunks": (1.36e-17, 1.46e-16, 4.43e-18, 1.17e-19)}
CPU_ID = {k: tuple(max(10 * v, EPS) for v in vs) for k, vs in CPU_MEASURED.items()}


def ragged_steps(M):
    return BASE * (0.4 + 1.2 * np.random.default_rng(5).random(M))


def problem(N, par, dts, B):
    """The inputs of _problem of test_gpu_second_order_1d.py on the steps dts: starts 0.2 cos(pi x / Lx + 0.4 b), controls of
    amplitudes 12, -9, 7, directions white noise, smooth (and a second white noise for B = 3)."""
    dts = np.asarray(dts, dtype=np.float64)
    M = len(dts)
    t = np.concatenate([[0.0, 0.0], np.cumsum(dts)])
    P = o.Params1D(N=N, T=float(t[-1]), dt_initial=float(dts.max()), **par)
    rows = M + 2
    x = np.linspace(0.0, P.Lx, N + 1)
    xs = x / P.Lx
    ctrl = lambda amp, s: amp * np.stack([np.cos(np.pi * xs * (1 + (k + s) % 3)) * np.sin(1 + k + s) for k in range(rows)])
    U = np.stack([ctrl(12.0, 0), ctrl(-9.0, 1), ctrl(7.0, 2)])[:B]
    noise = np.random.default_rng(3).standard_normal((rows, N + 1))
    smooth = np.stack([np.cos(2 * np.pi * xs) * np.cos(0.3 * k) for k in range(rows)])
    other = np.random.default_rng(4).standard_normal((rows, N + 1))
    H = np.stack([noise / np.abs(noise).max(), smooth, other / np.abs(other).max()])[:B]
    phi0 = np.stack([0.2 * np.cos(np.pi * xs + 0.4 * b) for b in range(B)])
    return dict(P=P, N=N, t=t, dts=dts, M=M, rows=rows, x=x, U=U, H=H, phi0=phi0, B=B, depth=_depth(N))


_CASES = {}


def case(name):
    if name not in _CASES:
        if name in RAGGED:
            N, par, M = RAGGED[name]
            pr = problem(N, par, ragged_steps(M), 3)
            pr.update(W=list(WEIGHTS), max_steps=M + SPARE)
        else:
            N, p = name.split("_")
            pr = problem(int(N), POINTS[p], STEPS, 2)
            pr.update(W=None, max_steps=len(STEPS))
        pr["name"] = name
        _CASES[name] = pr
    return _CASES[name]


def _dev(a, b, want):
    """|sum(a b) - want| relative to sum |a b|."""
    return abs(float(np.sum(a * b)) - float(want)) / float(np.sum(np.abs(a * b)))


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_matrix_and_cases_cover_every_depth():
    """The matrix is test_gpu_1d_levels.NS at both points; the ragged cases sit where the issue puts them."""
    assert len(MATRIX) == 2 * len(NS) and {_depth(N) for N in NS} == {0, 1, 2}
    assert (_depth(2049), 2049 % 2, 2049 // 2 + 1) == (1, 1, 1025)
    assert (_depth(4096), 4096 % 4, 4096 // 4 + 1) == (2, 0, 1025)
    assert _depth(33) == 0
    for name, (_, _, M) in RAGGED.items():
        d = ragged_steps(M)
        assert len(d) == M and d.max() / d.min() > 3.0, name


# ---------------------------------------------------------------------------------------
# CPU: the ragged cases and the many-chunk march meet their premises
# ---------------------------------------------------------------------------------------
def _oracle_march(pr, b, stats):
    phi, x, t = o.forward(pr["P"], control=pr["U"][b], initial_phi=pr["phi0"][b], solver="banded", stats=stats, dts=pr["dts"])
    assert np.array_equal(t, pr["t"]) and phi.shape == pr["U"][b].shape
    return phi


@pytest.mark.parametrize("name", list(RAGGED))
def test_cases_meet_their_premises(name):
    pr = case(name)
    P = pr["P"]
    st = {}
    phis = [_oracle_march(pr, b, st) for b in range(pr["B"])]
    assert len(st["exits"]) == pr["B"] * pr["M"] and all(e[0] == "conv" for e in st["exits"]) and st["failed_ls"] == 0
    top = max(float(np.abs(p[1:]).max()) for p in phis)
    print(f"{name}: max|phi[1:]| {top:.3f}, Newton iterations per call up to {max(e[1] for e in st['exits'])}")
    assert top < 1.0 - o.DELTA_SEP - 0.1
    _check_reference_identities(name, P, phis[0], pr["U"][0], pr["t"], pr["x"], pr["dts"])


def _check_reference_identities(name, P, phi, u, t, x, dts):
    """The four identities of test_adjoint_cpu_1d.py on the oracle's march phi, with its seeded targets and directions and
    the weights WEIGHTS[0], asserted at CPU_ID[name]."""
    w = WEIGHTS[0]
    rng = np.random.default_rng(11)
    phi_Q, phi_T = rng.standard_normal(phi.shape), rng.standard_normal(phi.shape[1])
    h, g = rng.standard_normal(phi.shape), rng.standard_normal(phi.shape)
    ref = lambda d: adjoint_reference_1d(P, phi, t, x, u, phi_Q, phi_T, *w, h=d, dts=dts)

    def curvature(d):
        d1, d2 = tangent_reference_1d(P, phi, t, d, dts=dts)
        return tangent_scalars_1d(phi, d1, d2, u, d, phi_Q, phi_T, x, t, *w)

    (G, Hh), (_, Hg) = ref(h), ref(g)
    S = curvature(h)
    polar = (curvature(g + h)["curvature"] - curvature(g - h)["curvature"]) / 4.0
    devs = (_dev(G, h, S["slope"]), _dev(h, Hh, S["curvature"]), _dev(g, Hh, polar), _dev(g, Hh, float(np.sum(h * Hg))))
    print(f"MEASURE cpu {name}: gh {devs[0]:.2e} hHh {devs[1]:.2e} polar {devs[2]:.2e} sym {devs[3]:.2e}")
    for d, bnd, what in zip(devs, CPU_ID[name], ("gh", "hHh", "polar", "sym")):
        assert d < bnd, (what, d, bnd)


def test_many_chunk_march_meets_its_premise():
    """The march of test_gpu_krylov_grid_1d.many_chunks (N = 4096, 255 uniform steps of 1e-3) with the oracle alone: every
    Newton call converges, max|phi[1:]| < 1 - DELTA_SEP - 0.1, and the four identities of the references hold on it."""
    from test_gpu_krylov_grid_1d import many_chunks_inputs
    P, t, dts, x, phi0, u = many_chunks_inputs()
    st = {}
    phi, _, th = o.forward(P, control=u, initial_phi=phi0, solver="banded", stats=st, dts=dts)
    assert np.array_equal(th, t) and phi.shape == u.shape
    top = float(np.abs(phi[1:]).max())
    print(f"many_chunks: max|phi[1:]| {top:.3f}, Newton iterations per call up to {max(e[1] for e in st['exits'])}")
    assert len(st["exits"]) == len(dts) and all(e[0] == "conv" for e in st["exits"]) and st["failed_ls"] == 0
    assert top < 1.0 - o.DELTA_SEP - 0.1
    _check_reference_identities("many_chunks", P, phi, u, t, x, dts)


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
def _run(V, pr):
    """March, hessvec, second_order and the shared-base pair on one context; the references on the engine's history."""
    P, B = pr["P"], pr["B"]
    eng = _engine(V, P, B, max_steps=pr["max_steps"])
    try:
        phi, _ = eng.forward(pr["phi0"], pr["dts"], u=pr["U"])
        phi = phi.reshape((B, pr["rows"], P.N + 1))
        tg = [o.build_targets(pr["x"], pr["t"], phi[b][0], P.Lx, P.T) for b in range(B)]
        phi_T, phi_Q = np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])
        opts = [V.make_opt(b1=w[0], b2=w[1], b3=w[2]) for w in pr["W"]] if pr["W"] else V.make_opt()
        kw = dict(phi_hist=phi, u=pr["U"], phi_Q=phi_Q, phi_T=phi_T, dt=pr["dts"])
        res = eng.hessvec(pr["H"], pr["t"], opts, **kw)
        so = eng.second_order(pr["H"], pr["t"], opts, histories=True, **kw)
        one = opts[1] if isinstance(opts, list) else opts
        shared = eng.hessvec(pr["H"], pr["t"], one, phi_hist=phi[1], u=pr["U"][1], phi_Q=phi_Q[1], phi_T=phi_T[1], dt=pr["dts"],
                             shared_base=True)
    finally:
        eng.close()
    W = pr["W"] or [(one.b1, one.b2, one.b3)] * B
    return dict(phi=phi, phi_T=phi_T, phi_Q=phi_Q, res=res, so=so, shared=shared, W=W)


def _check(V, name):
    pr = case(name)
    r = _run(V, pr)
    res, so, sh, H, phi = r["res"], r["so"], r["shared"], pr["H"], r["phi"]
    d = pr["depth"]
    assert np.abs(phi).max() < 1.0 - o.DELTA_SEP - 0.1                # the clip the tangent schemes ignore is inactive
    assert res["stats"]["linear_solves"] == 3 * pr["B"] * pr["M"]
    worst = dict(g=0.0, hv=0.0, d1=0.0, d2=0.0, id=0.0)
    nterms = H[0].size
    for b in range(pr["B"]):
        G, Hh = adjoint_reference_1d(pr["P"], phi[b], pr["t"], pr["x"], pr["U"][b], r["phi_Q"][b], r["phi_T"][b], *r["W"][b],
                                     h=H[b], dts=pr["dts"])
        d1, d2 = tangent_reference_1d(pr["P"], phi[b], pr["t"], H[b], dts=pr["dts"])
        worst["g"] = max(worst["g"], _rel(res["grad"][b], G))
        worst["hv"] = max(worst["hv"], _rel(res["hv"][b], Hh))
        worst["d1"] = max(worst["d1"], _rel(so["dphi"][b], d1))
        worst["d2"] = max(worst["d2"], _rel(so["d2phi"][b], d2))
        e1 = _dev(res["grad"][b], H[b], so["s_state"][b] + so["s_ctrl"][b])
        e2 = _dev(H[b], res["hv"][b], (so["c_gn"][b] + so["c_state"][b]) + so["c_ctrl"][b])
        worst["id"] = max(worst["id"], e1, e2)
        # the device's dots: its own sums of the n products, in another order than the host's
        t0, t1 = res["grad"][b] * H[b], H[b] * res["hv"][b]
        assert abs(res["gh"][b] - t0.sum()) <= nterms * EPS * np.abs(t0).sum(), (name, b)
        assert abs(res["hHh"][b] - t1.sum()) <= nterms * EPS * np.abs(t1).sum(), (name, b)
    pair = _dev(H[1], sh["hv"][0], np.sum(H[0] * sh["hv"][1]))
    worst["id"] = max(worst["id"], pair)
    print(f"MEASURE {name} depth {d}: grad {worst['g']:.2e} hv {worst['hv']:.2e} dphi {worst['d1']:.2e} d2phi {worst['d2']:.2e} "
          f"identities {worst['id']:.2e} (pair {pair:.2e}); max|phi| {np.abs(phi).max():.3f}")
    tol = dict(g=HV_TOL[d][0], hv=HV_TOL[d][1], d1=SO_TOL[d][0], d2=SO_TOL[d][1], id=HV_TOL[d][2])
    tol.update(OWN.get(name, {}))
    assert worst["g"] < tol["g"]
    assert worst["hv"] < tol["hv"]
    assert worst["d1"] < tol["d1"]
    assert worst["d2"] < tol["d2"]
    assert worst["id"] < tol["id"]


@gpu
@pytest.mark.parametrize("name", MATRIX)
def test_size_matrix(V, name):
    _check(V, name)


@gpu
@pytest.mark.parametrize("name", list(RAGGED))
def test_ragged_steps(V, name):
    _check(V, name)
