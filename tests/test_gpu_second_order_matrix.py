"""vch2d_second_order away from one tile and one parameter point: a matrix of grids, physical parameters, batches and
contract edges for the tangent march, against the CPU reference of tests/_tangent_ref.py (the oracle's assembled Newton
matrix, one sparse factorisation per step, the march's mass fix linearised about the shifts the engine recorded).

Every case: the engine marches, its history and mass_shifts() are pulled, the reference runs on that history, fields and
the six scalars are compared as test_gpu_second_order.py does, and the call's statistics must show every solve converged
(unconverged_solves == 0, max_lin_relres <= rtol, linear_solves == 2 B M).

Cases (plane: nf = Nx + 1 on the fast axis in 64-wide tiles, ns = Ny + 1 on the slow axis in 16-high tiles):
  tiles_fft      128 x 32 (Lx 1, Ly 0.5): 129 x 33 nodes = 3 x 3 tiles, an interior tile on both axes; FFT path
  tiles_gemm     130 x 36 (Lx 1.3, Ly 0.9): 3 x 3 tiles, GEMM-DCT path
  tiles_fft under VCH_FORCE_GEMM_DCT=1: the same inputs through the other transform
  offA_14x11, offB_14x11   the rectangular off-default points of test_tangent_cpu.py (M = 4, dt = 0.02)
  offA_sq        16 x 16 with Lx 1.3, Ly 0.9 (square grid, hx != hy)
  offA_gemm      50 x 36 (Lx 1.3, Ly 0.9), offB_fft  64 x 32 (Lx 1, Ly 0.5): the grids of test_gpu_forms.py
                 offA: c2 0.5, gamma 3, kappa 1e-3, c1 0.9, tau 0.01 (tau / dt = 0.5); offB: c2 1.5, tau 0.2 (tau / dt = 10)
  wide           64 x 32, c1 0.45, tau 1e-3, dt 1e-2, M = 4, a tanh front at +-0.95: Dmax / Dmin = 16 .. 18 at the levels
                 the tangent solves use (above the engine's threshold 4: they take the right-scaled form), clip inactive
  batch33, batch40   16 x 16, M = 3: every trajectory its own control, direction and weights, each against the reference
  many_tiles     64 x 512 (Lx 0.5, Ly 2): 2 x 33 = 66 tiles (k_tan_fin's strided loop); the six scalars recomputed on the CPU
                 from the engine's own dphi, d2phi, and trajectory 0 against the reference
test_cases_meet_their_premises (no GPU) shows with the oracle alone that every case converges, keeps every node in the
interior band of the mass fix and the clip inactive, and that `wide` has its wide diagonal.

Tolerances, engine against reference: TOL_D1 / TOL_D2 / TOL_S of test_gpu_second_order.py (1.2e-11 / 1.4e-11 / 1.5e-11).
A case that does not meet them takes OWN[case] = 10 x its measured deviation (the factor that file argues for a CG that
stops on a relative residual), never above the SOLVE class 1e-9 of test_gpu_forms.py.

Measured on an MI355X at the default rtol = 1e-12, largest relative deviation over the trajectories compared (dphi / d2phi /
scalars; sweeps per solve from the call's vch_stats):
    tiles_fft    1.4e-13 / 1.3e-13 / 2.5e-14   5.0     (under VCH_FORCE_GEMM_DCT=1: 1.2e-13 / 1.4e-13 / 2.9e-14; the two runs
                                                       differ by 1.1e-14 / 1.8e-14 / 1.4e-14)
    tiles_gemm   1.4e-12 / 1.5e-12 / 5.5e-13   5.3
    offA_14x11   6.0e-13 / 5.8e-13 / 3.3e-13           offB_14x11   4.2e-13 / 1.4e-12 / 1.0e-12
    offA_sq      9.7e-13 / 1.0e-12 / 9.9e-13           offA_gemm    1.1e-12 / 3.4e-12 / 2.9e-13
    offB_fft     6.3e-14 / 5.9e-14 / 1.6e-13           many_tiles   3.4e-13 / 3.9e-13 / 1.2e-13 (reduction chain alone: 3.2e-13)
    wide         7.5e-12 / 7.7e-12 / 3.1e-12   24.6    (right-scaled CG by the march's rule, 0 unconverged, worst final residual
                                                       9.1e-13; as plain CG, which these solves were before this matrix
                                                       existed: 1.75e-11 / 2.71e-11 / 1.16e-11 and 50.6 sweeps per solve,
                                                       outside the common bounds)
    batch33, batch40   7.1e-13 / 1.5e-12 / 1.69e-11: the fields meet the common bounds; s_state of trajectory 22 (3.6e-7, a
                 white-noise direction) is a cancelling sum, 3 to 300 times below the other trajectories', and its relative
                 deviation inherits that (every other scalar of the batch: below 4e-12): own bound 1.7e-10 for the scalars
    edge (14 x 11, Ly 0.8), rtol 1e-6: 6.7e-7 .. 1.7e-6 / 1.6e-6 .. 4.2e-6 / 4.9e-6, 48 iterations against 96
    mass_shifts() against the oracle's shifts on the 14 x 11 golden march: 3.2e-10 relative"""
import numpy as np
import pytest

from oracle import vch2d_oracle as o
from _tangent_ref import KEYS, tangent_reference, tangent_scalars
from test_gpu_forms import MARCH, SOLVE, _controls, _env
from test_gpu_second_order import TOL_D1, TOL_D2, TOL_S

gpu = pytest.mark.gpu
ALL_KEYS = KEYS + ("slope", "curvature")
OFF_A = dict(c2=0.5, gamma=3.0, kappa=1e-3, c1=0.9, tau=0.01)
OFF_B = dict(c2=1.5, gamma=3.0, kappa=1e-3, c1=0.9, tau=0.2)
WIDE = dict(c1=0.45, tau=1e-3)

CASES = {
    #              grid (Nx, Ny, Lx, Ly)        parameters  M  dt    B   control  uses_fft
    "tiles_fft":  ((128, 32, 1.0, 0.5),         {},         3, 1e-2, 2,  "forms", True),
    "tiles_gemm": ((130, 36, 1.3, 0.9),         {},         3, 1e-2, 2,  "forms", False),
    "offA_14x11": ((14, 11, 1.3, 0.9),          OFF_A,      4, 2e-2, 2,  "cos20", False),
    "offB_14x11": ((14, 11, 1.3, 0.9),          OFF_B,      4, 2e-2, 2,  "cos10", False),
    "offA_sq":    ((16, 16, 1.3, 0.9),          OFF_A,      4, 2e-2, 2,  "cos20", True),
    "offA_gemm":  ((50, 36, 1.3, 0.9),          OFF_A,      4, 2e-2, 2,  "forms", False),
    "offB_fft":   ((64, 32, 1.0, 0.5),          OFF_B,      4, 2e-2, 2,  "forms", True),
    "wide":       ((64, 32, 1.0, 0.5),          WIDE,       4, 1e-2, 2,  "wide", True),
    "batch33":    ((16, 16, 1.0, 1.0),          {},         3, 1e-2, 33, "cos20", True),
    "batch40":    ((16, 16, 1.0, 1.0),          {},         3, 1e-2, 40, "cos20", True),
    "many_tiles": ((64, 512, 0.5, 2.0),         {},         2, 1e-2, 2,  "forms", True),
}
# own bounds (dphi, d2phi, scalars) = 10 x measured, for the cases that do not meet TOL_D1 / TOL_D2 / TOL_S
OWN = {"batch33": (TOL_D1, TOL_D2, 1.7e-10), "batch40": (TOL_D1, TOL_D2, 1.7e-10)}
assert all(max(v) <= SOLVE for v in OWN.values())


def _tol(name):
    return OWN.get(name, (TOL_D1, TOL_D2, TOL_S))


def cos_controls(xx, yy, M, a, B):
    """The "cos<a>" controls: M + 1 rows per trajectory, amplitude a (1 - 0.02 b) (-1)^b, the modes shifted by b."""
    cos = lambda amp, s: amp * np.stack([np.cos(np.pi * xx * (1 + (k + s) % 3)) * np.cos(np.pi * yy) * np.sin(1 + k + s)
                                         for k in range(M + 1)])
    return np.stack([cos(a * (1.0 - 0.02 * b) * (-1.0) ** b, b) for b in range(B)])


def directions(xx, yy, M, B):
    """(B, M + 1, ..) directions.  Even trajectories: white noise (it must cross tile edges), odd: smooth, with phases and
    a ramp that keep it from being orthogonal to the controls (a scalar that vanishes by symmetry has no relative deviation)."""
    rng = np.random.default_rng(11)
    H = []
    for b in range(B):
        if b % 2 == 0:
            n = rng.standard_normal((M + 1,) + xx.shape)
            H.append(n / np.abs(n).max())
        else:
            H.append(np.stack([np.exp(xx + 0.5 * yy - 1.5) * np.cos(2 * np.pi * xx * (1 + b % 3) + 0.3) * np.cos(np.pi * yy + 0.2)
                               * np.cos(0.3 * k + b) for k in range(M + 1)]))
    return np.stack(H)


def _problem(name):
    (Nx, Ny, Lx, Ly), par, M, dt, B, ctrl, fft = CASES[name]
    P = o.Params2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, T=M * dt, dt_initial=dt, **par)
    t, dts = o.time_grid(M * dt, dt)
    assert len(dts) == M <= 4
    x, y = np.linspace(0.0, Lx, Nx + 1), np.linspace(0.0, Ly, Ny + 1)
    xx, yy = np.meshgrid(x / Lx, y / Ly, indexing="ij")
    if ctrl == "forms":
        U = _controls(x, y, Lx, Ly, B, M + 1)
    elif ctrl == "wide":            # both trajectories march the one qualified input; their directions differ
        U = np.repeat(_controls(x, y, Lx, Ly, 1, M + 1), B, axis=0)
    else:
        U = cos_controls(xx, yy, M, float(ctrl[3:]), B)
    if ctrl == "wide":
        front = 0.95 * np.tanh((x[:, None] - 0.5 + 0.1 * np.cos(2 * np.pi * y[None, :] / Ly)) / 0.04)
        p0 = np.clip(front + 0.15 * o.init_phi_random(Nx, Ny, o.DELTA_SEP, amp=0.1, seed=42), -0.98, 0.98)
        phi0 = np.stack([p0] * B)
    else:
        phi0 = np.stack([o.init_phi_random(Nx, Ny, o.DELTA_SEP, amp=0.1, seed=42 + b % 7) for b in range(B)])
    W = [(5.0, 10.0, 1e-4)] * B if B <= 2 else [(1.0 + 0.3 * b, 10.0 - 0.2 * b, 1e-4 * (1 + b)) for b in range(B)]
    return dict(name=name, P=P, t=t, dts=dts, M=M, B=B, x=x, y=y, U=U, H=directions(xx, yy, M, B), phi0=phi0, W=W, fft=fft)


_PROBLEMS = {}


def problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = _problem(name)
    return _PROBLEMS[name]


def _diag_ratio(P, phi_star, dt):
    D = o.jac_diag(phi_star, dt, P)
    return float(D.max() / D.min())


# ---------------------------------------------------------------------------------------
# CPU: every case meets its premises
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cases_meet_their_premises(name):
    """With the oracle alone: every Newton call of the march converges, |phi_n| + |s| stays inside the interior band of the
    mass fix for n >= 1 (so the clip is inactive and every node is shifted), and the wide-diagonal case has Dmax / Dmin > 4
    at every level the tangent solves use.  Batches and the 66-tile grid: trajectories 0 and B - 1 (the others differ in
    the control's sign and scale only)."""
    pr = problem(name)
    P, orig, hists = pr["P"], o.newton_step, []

    def recording(*a, **kw):
        kw["return_history"] = True
        ph, mu, h = orig(*a, **kw)
        hists.append(list(h))
        return ph, mu

    o.newton_step = recording
    try:
        for b in sorted({0, pr["B"] - 1} if name != "many_tiles" else {0}):
            st = {}
            phi, _, _ = o.forward(P, control=pr["U"][b], phi0=pr["phi0"][b], stats=st)
            s = np.array(st["mass_shifts"])
            assert all(st["mass_shift_interior"]) or not s.any()
            top = np.abs(phi[1:]).max()
            print(f"{name} b={b}: max|phi| per level {[round(float(np.abs(p).max()), 3) for p in phi]}, shifts {s}, Newton "
                  f"norms recorded {[len(h) for h in hists]}")
            assert top < 0.985 - np.abs(s).max()
            assert np.abs(phi[0]).max() <= 0.98
            if name == "wide":
                ratios = [_diag_ratio(P, phi[n + 1] + s[n], pr["dts"][n]) for n in range(pr["M"])]
                print(f"wide: Dmax/Dmin {ratios}")
                assert min(ratios) > 4.0
    finally:
        o.newton_step = orig
    assert hists and all(h[-1] < o.NEWTON_TOL for h in hists)
    assert all(len(h) < 20 for h in hists)


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


def _engine(V, P, batch, max_steps=4):
    return V.Engine2D(P.Nx, P.Ny, P.Lx, P.Ly, P.tau, P.gamma, P.c1, P.c2, P.kappa, batch=batch, max_steps=max_steps)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _run(V, pr, env=None, **kw):
    """March, pull history and shifts, make the call.  Returns the problem extended by the engine's answers."""
    P, B = pr["P"], pr["B"]
    with _env(**(env or {})):
        eng = _engine(V, P, B)
    try:
        phi, _ = eng.forward(pr["phi0"], pr["dts"], u=pr["U"])
        phi = phi.reshape((B,) + phi.shape[-3:])
        shifts = eng.mass_shifts()
        tg = [o.build_targets(pr["x"], pr["y"], pr["t"], phi[b][0], P.Lx, P.Ly, P.T) for b in range(B)]
        phi_T, phi_Q = np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])
        opts = [V.make_opt(b1=w[0], b2=w[1], b3=w[2]) for w in pr["W"]]
        res = eng.second_order(pr["H"], pr["dts"], pr["t"], opts, phi_Q=phi_Q, phi_T=phi_T, histories=True, **kw)
        uses_fft = eng.uses_fft
    finally:
        eng.close()
    return dict(pr, phi=phi, shifts=shifts, phi_T=phi_T, phi_Q=phi_Q, res=res, uses_fft=uses_fft)


def _check_stats(r, rtol=1e-12):
    st = r["res"]["stats"]
    print(f"{r['name']}: stats {st}; sweeps per solve {st['linear_iters'] / max(1, st['linear_solves']):.2f}")
    assert st["unconverged_solves"] == 0
    assert st["max_lin_relres"] <= rtol
    assert st["linear_solves"] == 2 * r["B"] * r["M"]


def _scalars(r, b, d1, d2, h=None):
    """The reference scalars of trajectory b for the fields d1, d2, and the scale each deviation is taken relative to:
    the scalar's own magnitude, as in test_gpu_second_order.py."""
    S = tangent_scalars(r["phi"][b], d1, d2, r["U"][b], r["H"][b] if h is None else h, r["phi_Q"][b], r["phi_T"][b], r["x"],
                        r["y"], r["t"], *r["W"][b])
    return S, {k: abs(v) for k, v in S.items()}


def _reference(r, b):
    d1, d2 = tangent_reference(r["P"], r["phi"][b], r["t"], r["H"][b], r["shifts"][b])
    return (d1, d2) + _scalars(r, b, d1, d2)


def _deviations(r, b, ref=None):
    d1, d2, S, scale = ref or _reference(r, b)
    res = r["res"]
    e1, e2 = _rel(res["dphi"][b], d1), _rel(res["d2phi"][b], d2)
    dev = {k: abs(float(res[k][b]) - S[k]) / scale[k] for k in ALL_KEYS}
    es = max(dev.values())
    print(f"{r['name']} b={b}: rel.dev dphi {e1:.2e} d2phi {e2:.2e} scalars {es:.2e} (" +
          " ".join(f"{k} {float(res[k][b]):.3e} {v:.1e}" for k, v in dev.items()) + ")")
    return e1, e2, es


def _check_against_reference(r, bs):
    assert np.abs(r["phi"][:, 1:]).max() < 0.985 - np.abs(r["shifts"]).max()      # the premise, on the engine's own history
    worst = np.zeros(3)
    for b in bs:
        worst = np.maximum(worst, _deviations(r, b))
        assert r["res"]["n_h"][b] > 0 and r["res"]["c_gn"][b] > 0
    print(f"{r['name']}: largest relative deviation dphi {worst[0]:.2e} d2phi {worst[1]:.2e} scalars {worst[2]:.2e}")
    t1, t2, ts = _tol(r["name"])
    assert worst[0] < t1
    assert worst[1] < t2
    assert worst[2] < ts
    assert not r["res"]["dphi"][:, 0].any() and not r["res"]["d2phi"][:, 0].any()


@pytest.fixture(scope="module")
def tiles_default(V):
    return _run(V, problem("tiles_fft"))


@gpu
@pytest.mark.parametrize("name", ["tiles_fft", "tiles_gemm", "offA_14x11", "offB_14x11", "offA_sq", "offA_gemm", "offB_fft"])
def test_tiles_and_off_default_points(V, tiles_default, name):
    r = tiles_default if name == "tiles_fft" else _run(V, problem(name))
    assert r["uses_fft"] == r["fft"]
    if r["P"].Nx != r["P"].Ny:
        assert np.abs(r["shifts"]).min() > 1e-7          # the fix is at work on every step of a rectangular grid
    _check_stats(r)
    _check_against_reference(r, range(r["B"]))


@gpu
def test_wide_diagonal(V):
    """The tangent solves where the march switches to the right-scaled form, and they with it: Dmax / Dmin > 4 on the
    engine's history."""
    r = _run(V, problem("wide"))
    ratios = [_diag_ratio(r["P"], r["phi"][b][n + 1] + r["shifts"][b][n], r["dts"][n]) for b in range(2) for n in range(r["M"])]
    print(f"wide: Dmax/Dmin on the engine's history {[round(v, 1) for v in ratios]}; max|phi| per level "
          f"{[round(float(np.abs(r['phi'][0][n]).max()), 3) for n in range(r['M'] + 1)]}")
    assert min(ratios) > 4.0
    assert np.abs(r["phi"][:, 1:]).max() < 0.985
    _check_stats(r)
    _check_against_reference(r, range(2))


@gpu
@pytest.mark.parametrize("name", ["batch33", "batch40"])
def test_batches_above_32(V, name):
    r = _run(V, problem(name))
    _check_stats(r)
    assert len({tuple(w) for w in r["W"]}) == r["B"]
    _check_against_reference(r, range(r["B"]))           # 0, 16, 32, B - 1 among them


@gpu
def test_more_than_64_tiles(V):
    r = _run(V, problem("many_tiles"))
    _check_stats(r)
    res = r["res"]
    for b in range(2):
        # the reduction chain alone: the scalars from the engine's own fields, no linear solve in the way
        S, scale = _scalars(r, b, res["dphi"][b], res["d2phi"][b])
        dev = {k: abs(float(res[k][b]) - S[k]) / scale[k] for k in ALL_KEYS}
        print(f"many_tiles b={b}: scalars from the engine's own fields, rel.dev " + " ".join(f"{k} {v:.2e}" for k, v in dev.items()))
        assert max(dev.values()) < TOL_S, dev
    _check_against_reference(r, [0])


@gpu
def test_gemm_dct_variant_of_the_tiles_case(V, tiles_default):
    r = _run(V, problem("tiles_fft"), env=dict(VCH_FORCE_GEMM_DCT=1))
    assert tiles_default["uses_fft"] and not r["uses_fft"]
    _check_stats(r)
    _check_against_reference(r, range(2))
    a, d = r["res"], tiles_default["res"]
    e1, e2 = _rel(a["dphi"], d["dphi"]), _rel(a["d2phi"], d["d2phi"])
    es = max(float(np.abs(a[k] - d[k])[b] / _reference(r, b)[3][k]) for k in ALL_KEYS for b in range(2))
    print(f"GEMM-DCT against the default run: dphi {e1:.2e} d2phi {e2:.2e} scalars {es:.2e}")
    assert e1 < 2 * TOL_D1 and e2 < 2 * TOL_D2 and es < 2 * TOL_S        # both within the tolerance of one reference


# ---------------------------------------------------------------------------------------
# contract edges (14 x 11, Ly 0.8: the grid of the golden march; the mass fix shifts every step)
# ---------------------------------------------------------------------------------------
def _edge_problem():
    Nx, Ny, Lx, Ly, M, dt, B = 14, 11, 1.0, 0.8, 4, 1e-2, 2
    P = o.Params2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, T=M * dt, dt_initial=dt)
    t, dts = o.time_grid(M * dt, dt)
    x, y = np.linspace(0.0, Lx, Nx + 1), np.linspace(0.0, Ly, Ny + 1)
    U = 10.0 * _controls(x, y, Lx, Ly, B, M + 1)
    n = np.random.default_rng(21).standard_normal((B, M + 1, Nx + 1, Ny + 1))
    phi0 = np.stack([o.init_phi_random(Nx, Ny, o.DELTA_SEP, amp=0.1, seed=42 + b) for b in range(B)])
    return dict(name="edge", P=P, t=t, dts=dts, M=M, B=B, x=x, y=y, U=U, H=n / np.abs(n).max(), phi0=phi0,
                W=[(5.0, 10.0, 1e-4), (1.5, 2.0, 3e-2)], fft=False)


@gpu
@pytest.mark.parametrize("rows", [3, None])
def test_short_control_and_no_control(V, rows):
    """The control the march ran under has fewer rows than M + 1 (it counts as zero from there on), or there is none."""
    pr = _edge_problem()
    P, B, M = pr["P"], pr["B"], pr["M"]
    eng = _engine(V, P, B)
    u = None if rows is None else pr["U"][:, :rows]
    phi, _ = eng.forward(pr["phi0"], pr["dts"], u=u)
    r = dict(pr, phi=phi, shifts=eng.mass_shifts(), U=np.zeros_like(pr["U"]) if rows is None else pr["U"][:, :rows])
    tg = [o.build_targets(pr["x"], pr["y"], pr["t"], phi[b][0], P.Lx, P.Ly, P.T) for b in range(B)]
    r["phi_T"], r["phi_Q"] = np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])
    opts = [V.make_opt(b1=w[0], b2=w[1], b3=w[2]) for w in pr["W"]]
    r["res"] = eng.second_order(pr["H"], pr["dts"], pr["t"], opts, phi_Q=r["phi_Q"], phi_T=r["phi_T"], histories=True)
    eng.close()
    _check_stats(r)
    for b in range(B):
        d1, d2, S, scale = _reference(r, b)
        if rows is None:
            assert r["res"]["s_ctrl"][b] == 0.0 == S["s_ctrl"]
            scale = dict(scale, s_ctrl=1.0)          # compared exactly above; keeps the relative comparison below defined
        e1, e2, es = _deviations(r, b, (d1, d2, S, scale))
        assert e1 < TOL_D1 and e2 < TOL_D2 and es < TOL_S
        if rows is not None:
            assert r["res"]["s_ctrl"][b] != 0.0


@pytest.fixture(scope="module")
def edge(V):
    """One context on the edge problem: march, a jacobian_solve, then the default call -- the state the tests below continue
    from, each leaving it as it found it."""
    pr = _edge_problem()
    eng = _engine(V, pr["P"], pr["B"])
    phi, _ = eng.forward(pr["phi0"], pr["dts"], u=pr["U"])
    rp = np.random.default_rng(5).standard_normal(phi[:, 1].shape)
    rm = np.random.default_rng(6).standard_normal(phi[:, 1].shape)
    js = eng.jacobian_solve(phi[:, 2], pr["dts"][0], rp, rm)
    phi2, st_f = eng.forward(pr["phi0"], pr["dts"], u=pr["U"])
    assert np.array_equal(phi2, phi)
    r = dict(pr, phi=phi, shifts=eng.mass_shifts())
    tg = [o.build_targets(pr["x"], pr["y"], pr["t"], phi[b][0], pr["P"].Lx, pr["P"].Ly, pr["P"].T) for b in range(pr["B"])]
    r["phi_T"], r["phi_Q"] = np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])
    r["opts"] = [V.make_opt(b1=w[0], b2=w[1], b3=w[2]) for w in pr["W"]]
    r["res"] = eng.second_order(pr["H"], pr["dts"], pr["t"], r["opts"], phi_Q=r["phi_Q"], phi_T=r["phi_T"], histories=True)
    r.update(eng=eng, js=js, js_in=(rp, rm), st_f=st_f)
    yield r
    eng.close()


@gpu
def test_direction_of_one_row(edge):
    """h_rows = 1: the row drives no step (F2:545-548), dphi == 0 exactly; it still counts in the integrals of h."""
    e = edge
    res = e["eng"].second_order(e["H"][:, :1], e["dts"], e["t"], e["opts"], phi_Q=e["phi_Q"], phi_T=e["phi_T"], histories=True)
    assert not res["dphi"].any() and not res["d2phi"].any()
    assert (res["n_h"] > 0).all() and (res["c_ctrl"] > 0).all()
    for k in ("s_state", "c_gn", "c_state"):
        assert not res[k].any(), k
    for b in range(e["B"]):
        z = np.zeros_like(e["phi"][b])
        S, _ = _scalars(e, b, z, z, h=e["H"][b, :1])
        assert res["s_ctrl"][b] == 0.0 == S["s_ctrl"]        # the ramped control's row 0 is zero
        for k in ("c_ctrl", "n_h"):
            assert abs(float(res[k][b]) / S[k] - 1.0) < TOL_S, k


@gpu
def test_looser_rtol_is_honoured_and_the_tolerance_comes_back(edge):
    """rtol = 1e-6: fewer iterations, a deviation between the default tolerance and 100 rtol, residuals at or below rtol.
    Afterwards, and after a call that fails its argument checks, forward and jacobian_solve return the bits they returned
    before: the context's own linear tolerance is back."""
    e, eng = edge, edge["eng"]
    _check_stats(e)
    for b in range(e["B"]):
        e1, e2, es = _deviations(e, b)
        assert e1 < TOL_D1 and e2 < TOL_D2 and es < TOL_S
    rtol = 1e-6
    loose = eng.second_order(e["H"], e["dts"], e["t"], e["opts"], phi_Q=e["phi_Q"], phi_T=e["phi_T"], histories=True, rtol=rtol)
    with pytest.raises(ValueError):
        eng.second_order(e["H"], e["dts"], e["t"], e["opts"], phi_Q=e["phi_Q"], phi_T=e["phi_T"], rtol=rtol, order=3)
    st = loose["stats"]
    print(f"rtol 1e-6: stats {st}; default {e['res']['stats']}")
    assert st["linear_iters"] < e["res"]["stats"]["linear_iters"]
    assert st["unconverged_solves"] == 0 and st["max_lin_relres"] <= rtol
    assert st["linear_solves"] == 2 * e["B"] * e["M"]
    for b in range(e["B"]):
        e1, e2, es = _deviations(dict(e, res=loose, name="edge rtol 1e-6"), b)
        assert TOL_D1 < e1 < 100 * rtol and TOL_D2 < e2 < 100 * rtol
        assert es < 100 * rtol
    phi, st_f = eng.forward(e["phi0"], e["dts"], u=e["U"])
    assert np.array_equal(phi, e["phi"])
    for k in ("newton_iters", "linear_solves", "linear_iters", "armijo_trials", "max_lin_relres", "max_lin_absres"):
        assert st_f[k] == e["st_f"][k], k
    js = eng.jacobian_solve(e["phi"][:, 2], e["dts"][0], *e["js_in"])
    assert np.array_equal(js[0], e["js"][0]) and np.array_equal(js[1], e["js"][1])
    assert js[2]["linear_iters"] == e["js"][2]["linear_iters"]
    again = eng.second_order(e["H"], e["dts"], e["t"], e["opts"], phi_Q=e["phi_Q"], phi_T=e["phi_T"], histories=True)
    for k in KEYS:
        assert np.array_equal(again[k], e["res"][k]), k
    assert np.array_equal(again["dphi"], e["res"]["dphi"]) and np.array_equal(again["d2phi"], e["res"]["d2phi"])


@gpu
def test_backward_and_cost_after_the_call_are_undisturbed(V, edge):
    """forward -> second_order -> backward + cost on the resident history: the bits of a context that never made the call."""
    e = edge
    b1, b2 = 5.0, 10.0
    opt = V.make_opt(b1=b1, b2=b2, b3=1e-4)

    def tail(eng):
        p, q, r, _ = eng.backward(None, e["t"], b1, b2, phi_Q=e["phi_Q"], phi_T=e["phi_T"])
        return p, q, r, eng.cost(None, e["U"], e["phi_Q"], e["phi_T"], e["t"], opt)

    plain = _engine(V, e["P"], e["B"])
    plain.forward(e["phi0"], e["dts"], u=e["U"])
    want = tail(plain)
    plain.close()
    eng = _engine(V, e["P"], e["B"])
    eng.forward(e["phi0"], e["dts"], u=e["U"])
    res = eng.second_order(e["H"], e["dts"], e["t"], e["opts"], phi_Q=e["phi_Q"], phi_T=e["phi_T"])
    got = tail(eng)
    shifts = eng.mass_shifts()
    eng.close()
    for a, w in zip(got, want):
        assert np.array_equal(a, w)
    for k in KEYS:
        assert np.array_equal(res[k], e["res"][k]), k
    assert np.array_equal(shifts, e["shifts"])            # the record outlives backward and cost on the resident history


@gpu
def test_mass_shifts_against_the_oracle(V):
    """The record of the 14 x 11 golden march against the oracle's own shifts; (near) zero on a square grid; no record
    without a march."""
    from conftest import golden
    g = golden("g2d_forward_14x11.npz")
    P = o.Params2D(Nx=int(g["Nx"]), Ny=int(g["Ny"]), Lx=float(g["Lx"]), Ly=float(g["Ly"]), T=float(g["T"]), dt_initial=float(g["dt"]))
    t, dts = o.time_grid(P.T, P.dt_initial)
    eng = _engine(V, P, 1, max_steps=len(dts))
    with pytest.raises(V.VchError, match="-3"):
        eng.mass_shifts()
    for u in (None, g["u"]):
        st = {}
        ref, _, _ = o.forward(P, control=u, phi0=g["phi_nat"][0], stats=st)
        want = np.array(st["mass_shifts"])
        assert all(st["mass_shift_interior"]) and np.abs(want).min() > 1e-6
        phi, _ = eng.forward(g["phi_nat"][0], dts, u=u)
        got = eng.mass_shifts()
        assert got.shape == (1, len(dts))
        dev = np.abs(got[0] - want).max() / np.abs(want).max()
        print(f"14 x 11 golden march, control {u is not None}: shifts {got[0]}, rel.dev from the oracle's {dev:.2e}; fields "
              f"{_rel(phi, ref):.2e}")
        assert dev < MARCH
    # forward with the history kept on the device only: the same record
    eng.forward(g["phi_nat"][0], dts, u=g["u"], store=False)
    assert np.array_equal(eng.mass_shifts(), got)
    eng.close()
    sq = o.Params2D(Nx=16, Ny=16, T=0.04, dt_initial=0.01)
    eng = _engine(V, sq, 2)
    eng.forward(np.stack([o.init_phi_random(16, 16, o.DELTA_SEP, amp=0.1, seed=42 + b) for b in range(2)]),
                o.time_grid(0.04, 0.01)[1])
    s = eng.mass_shifts()
    eng.close()
    print(f"16 x 16: shifts {s}")
    assert s.shape == (2, 4) and np.abs(s).max() < 1e-15


@gpu
def test_pgd_shift_record_follows_the_accepted_history(V):
    """After PGD iterations on a rectangular grid (rejected line-search trials among them) the record is that of the
    resident iterate: a fresh march under the iterate's control reproduces its history and its shifts within the MARCH class,
    and the record is no longer the one pgd_init's march under the zero control left."""
    Nx, Ny, T, dt = 14, 11, 0.04, 0.01
    P = o.Params2D(Nx=Nx, Ny=Ny, Lx=1.0, Ly=0.8, T=T, dt_initial=dt)
    t, dts = o.time_grid(T, dt)
    x, y = np.linspace(0.0, P.Lx, Nx + 1), np.linspace(0.0, P.Ly, Ny + 1)
    phi0 = np.stack([o.init_phi_random(Nx, Ny, o.DELTA_SEP, amp=0.1, seed=42 + b) for b in range(2)])
    phi_T = np.stack([o.build_targets(x, y, t, phi0[b], P.Lx, P.Ly, T)[0] for b in range(2)])
    # alpha_max far too long a step: the optimistic step is rejected and the line search backtracks
    opts = [V.make_opt(alpha_max=4e4), V.make_opt(b1=2.0, b2=4.0, b3=1e-3, alpha_max=50.0)]
    eng = _engine(V, P, 2)
    eng.pgd_init(phi0, phi_T, t, opts, ramp=True, T=T)
    out = eng.pgd_iterate(3)
    print(f"attempts {out['attempts']}")
    assert out["attempts"].max() >= 1
    u, phi, s = eng.pgd_get("u"), eng.pgd_get("phi"), eng.mass_shifts()
    eng.close()
    fresh = _engine(V, P, 2)
    fresh.forward(phi0, dts)
    first = fresh.mass_shifts()
    ph, _ = fresh.forward(phi0, dts, u=u)
    want = fresh.mass_shifts()
    fresh.close()
    dev = [float(np.abs(s[b] - want[b]).max() / np.abs(want[b]).max()) for b in range(2)]
    moved = [float(np.abs(s[b] - first[b]).max() / np.abs(first[b]).max()) for b in range(2)]
    print(f"fields {_rel(ph, phi):.2e}; shifts against a fresh march {dev}, against the zero-control march {moved}")
    assert _rel(ph, phi) < MARCH and max(dev) < MARCH
    assert min(moved) > 1e3 * MARCH and np.abs(s).min() > 1e-7
