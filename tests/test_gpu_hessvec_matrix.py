"""vch2d_hessvec away from one tile and one parameter point: the transposed sweep (k_hv_init, k_hv_keep, k_hv_rhs<0/1>,
k_hv_emit, k_hv_dots, k_hv_dots_fin) over the cases of the tangent march's matrix
(test_gpu_second_order_matrix.py: its problem(), CASES and _diag_ratio, whose premises that file shows on the CPU) and over
three cases of its own with non-uniform time steps, against the plain-transpose CPU reference of tests/_adjoint_ref.py.

Every case: the engine marches, its history and mass_shifts() are pulled, hessvec (order 2) and second_order run on the same
context with the case's per-trajectory weights W, and the reference runs on the engine's own history.  Checked: grad and hv
against the reference (max-norm of the difference over the max-norm of the reference), identities 1 (sum G h = slope), 2
(sum h Hh = curvature; both against second_order) and 4 (sum g Hh = sum h Hg, the other direction of the pair on the same
base point) as test_gpu_hessvec_2d._check_case measures them, `dots` within n eps sum|terms| of the host's sums,
unconverged_solves == 0, max_lin_relres <= rtol, linear_solves == 3 B M, uses_fft, and on a rectangular grid
|shifts|.min() > 1e-7.

Cases of the tangent matrix (tiles_fft is the `tiles` case of test_gpu_hessvec_2d.py and is left out):
  tiles_gemm, offA_14x11, offB_14x11, offA_sq, offA_gemm, offB_fft     3 x 3 tiles through the GEMM-DCT; c2, gamma, kappa, c1,
                 tau off their defaults (k_hv_emit's tau/dt + 2 c2, kappa/2, alpha, beta; k_hv_rhs's c1, tau)
  wide           Dmax / Dmin = 16 .. 18: the transposed solves between their two diagonal scalings under the right-scaled
                 CG form the march's rule picks; the ratio is asserted on the engine's history
  batch33, batch40   above the 32 per-trajectory records of the solve chain; trajectories 0, 1, 16, 31, 32, B - 1 against the
                 reference; members 0, 31, 32 of batch33 bitwise equal to single-trajectory contexts in grad, hv, dots
  many_tiles     64 x 512, 66 tiles: the strided loop of post_sums in k_hv_rhs, k_hv_keep, k_hv_dots_fin; trajectory 0
                 against the reference, both trajectories in the identities and the dots
Cases of this file (steps dts = base (0.4 + 1.2 default_rng(5).random(M)): the largest 3.5 times the smallest, so ys = -2/dt,
ym/dt, kp, alpha, beta and the trapezoid weight wt[lvl] differ from level to level; phi0 = init_phi_random(amp 0.1, seed 42);
batch 2, a white-noise and a smooth direction, weights (5, 10, 1e-4)):
  ragged_offA    14 x 11, Lx 1.3, Ly 0.9, OFF_A, base 2e-2, M = 12, control cos20
  ragged_offB    32 x 16, Lx 1, Ly 0.5, OFF_B, base 2e-2, M = 12, control cos10
  long16         16 x 16, default parameters, base 1e-2, M = 24, control cos20.  A call takes one row count for the whole
                 batch, so the direction of 5 rows (< M + 1, the row rule) is a second call on the same context with the
                 first 5 rows of both directions: hv against the reference, identity 2 against second_order, identity 1
                 through the direction padded with zero rows to M + 1 (a direction in its own right)
test_cases_meet_their_premises (no GPU) shows for these three with o.forward(dts=...) alone that every Newton call converges
in under 20 iterations, max|phi[1:]| < 0.985 - max|s|, the shifts are non-zero on the two rectangles and the reference's
identities 1 and 2 (against tests/_tangent_ref.py) hold below the bounds of test_adjoint_cpu.py.

Tolerances: TOL_G / TOL_HV / TOL_ID of test_gpu_hessvec_2d.py (5.4e-12 / 1.1e-11 / 6.1e-13).  A case that misses one takes
OWN[case] = 10 x its deviation from the CPU reference measured on an MI355X (the factor test_gpu_second_order.py argues for a
CG that stops on a relative residual), never above the SOLVE class 1e-9 of test_gpu_forms.py.  Bitwise claims are bitwise;
the dots bound n eps sum|terms| is derived, not measured.

Measured on an MI355X at the default rtol = 1e-12, worst over the trajectories compared (grad / hv / identities; sweeps per
solve from the call's vch_stats); every case meets the common bounds, so OWN is empty:
    tiles_gemm   4.60e-13 / 9.57e-13 / 5.91e-15   5.3      offA_14x11   1.81e-13 / 1.02e-12 / 5.25e-14   4.9
    offB_14x11   1.54e-13 / 4.40e-13 / 1.86e-14   5.5      offA_sq      5.81e-14 / 4.24e-13 / 3.48e-14   4.6
    offA_gemm    1.12e-13 / 3.26e-13 / 4.84e-15   3.8      offB_fft     4.14e-14 / 5.10e-14 / 4.46e-16   4.0
    wide         3.50e-12 / 7.38e-12 / 1.86e-13   24.2     (Dmax / Dmin 16.3 .. 17.9 on the engine's history, worst final
                                                           residual 9.85e-13: the right-scaled form, inside the common bounds)
    batch33, batch40   3.55e-13 / 1.65e-13 / 2.72e-14   6.0
    many_tiles   2.52e-13 / 2.74e-14 / 1.56e-15   4.0
    ragged_offA  2.00e-14 / 4.07e-13 / 2.99e-14   5.1      ragged_offB  1.05e-13 / 5.69e-13 / 2.58e-14   4.6
    long16       2.97e-13 / 4.03e-12 / 1.44e-13   7.3      (5 rows: hv 3.85e-12, identities 9.92e-14)

That the tests can fail: mutants of the engine that change arithmetic or which in-bounds value is read, never an address,
built beside the tree and never committed; grad / hv / identities under each, every case not named is unchanged to the digits
above and passes, as do test_gpu_hessvec_2d.test_fields_identities_and_dots and (mutants 1 - 3) this file's other cases:
  1. k_hv_emit's kp = tau/dt + 2 * 1.0 in place of 2 c2.  Fails offA_14x11 5.1e-1 / 5.1e-1 / 1.8e-1, offB_14x11 8.4e-2 /
     8.2e-2 / 4.1e-2, offA_sq 3.9e-1 / 5.2e-1 / 2.0e-1, offA_gemm 3.8e-1 / 5.1e-1 / 9.8e-2, offB_fft 8.7e-2 / 8.3e-2 / 4.2e-2,
     ragged_offA 2.7 / 2.6 / 2.2e-1, ragged_offB 3.1e-1 / 3.1e-1 / 6.8e-2; passes every case at the default c2, the four
     cases of test_gpu_hessvec_2d.py and the whole of test_gpu_krylov_grid_2d.py among them.
  2. post_sums summing the first 64 tiles only.  In post_sums itself (the march's mass fix reads it too), in k_hv_rhs alone and
     in k_hv_keep alone: many_tiles fails, the call refused with VCH_ERR_STATE by the engine's own check of the fix's set
     (the classified weight no longer equals the recorded W_int).  In k_hv_dots_fin alone: many_tiles fails its dots bound,
     6.5e-10 against n eps sum|terms| = 2.1e-15.  Up to 64 tiles each of the four is the engine itself: nothing else in this
     file or in test_gpu_hessvec_2d.py's cases fails (run under the first and under all three sites at once), nor in
     test_gpu_fix_band.py (run under the latter).
  3. k_hv_emit's alpha, beta from dt[min(k + 1, M - 1)].  Fails ragged_offA 3.4e-1 / 3.6e-1 / 3.6e-2, ragged_offB 1.9e-1 /
     2.0e-1 / 3.3e-2, long16 2.5e-1 / 2.4e-1 / 3.8e-2 (and fft16 of test_gpu_hessvec_2d.py, whose last step is ragged, 7.1e-2;
     test_gpu_krylov_grid_2d.py: Ritz values 1.8e-3, relation 2.5e-4, CG true residual 4.4e-2); passes every uniform case."""
import numpy as np
import pytest

from oracle import vch2d_oracle as o
from _adjoint_ref import adjoint_reference
from _tangent_ref import tangent_reference, tangent_scalars
from test_adjoint_cpu import BOUND
from test_gpu_forms import SOLVE
from test_gpu_hessvec_2d import EPS, TOL_G, TOL_HV, TOL_ID, _check_stats, _engine, _ident, _pad, _rel
from test_gpu_second_order_matrix import CASES, OFF_A, OFF_B, _diag_ratio, cos_controls, directions, problem

gpu = pytest.mark.gpu

RAGGED = {
    #               grid (Nx, Ny, Lx, Ly)   parameters  M   base  control  uses_fft
    "ragged_offA": ((14, 11, 1.3, 0.9),     OFF_A,      12, 2e-2, 20.0,    False),
    "ragged_offB": ((32, 16, 1.0, 0.5),     OFF_B,      12, 2e-2, 10.0,    True),
    "long16":      ((16, 16, 1.0, 1.0),     {},         24, 1e-2, 20.0,    True),
}
SHORT_ROWS = 5

# measured on an MI355X (the MEASURE lines of this file): worst deviation (grad, hv, identities) per case
MEASURED = {
    "tiles_gemm": (4.60e-13, 9.57e-13, 5.91e-15), "offA_14x11": (1.81e-13, 1.02e-12, 5.25e-14),
    "offB_14x11": (1.54e-13, 4.40e-13, 1.86e-14), "offA_sq": (5.81e-14, 4.24e-13, 3.48e-14),
    "offA_gemm": (1.12e-13, 3.26e-13, 4.84e-15), "offB_fft": (4.14e-14, 5.10e-14, 4.46e-16),
    "wide": (3.50e-12, 7.38e-12, 1.86e-13), "batch33": (3.55e-13, 1.65e-13, 2.72e-14), "batch40": (3.55e-13, 1.65e-13, 2.72e-14),
    "many_tiles": (2.52e-13, 2.74e-14, 1.56e-15), "ragged_offA": (2.00e-14, 4.07e-13, 2.99e-14),
    "ragged_offB": (1.05e-13, 5.69e-13, 2.58e-14), "long16": (2.97e-13, 4.03e-12, 1.44e-13),
}
# own bounds (grad, hv, identities) = 10 x measured, for the cases that do not meet TOL_G / TOL_HV / TOL_ID
OWN = {}
assert all(max(v) <= SOLVE for v in OWN.values())


def _tol(name):
    return OWN.get(name, (TOL_G, TOL_HV, TOL_ID))


def ragged_steps(base, M):
    return base * (0.4 + 1.2 * np.random.default_rng(5).random(M))


_RAGGED = {}


def ragged_problem(name):
    if name not in _RAGGED:
        (Nx, Ny, Lx, Ly), par, M, base, amp, fft = RAGGED[name]
        dts = ragged_steps(base, M)
        t = np.concatenate([[0.0], np.cumsum(dts)])
        P = o.Params2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, T=float(t[-1]), dt_initial=float(dts.max()), **par)
        x, y = np.linspace(0.0, Lx, Nx + 1), np.linspace(0.0, Ly, Ny + 1)
        xx, yy = np.meshgrid(x / Lx, y / Ly, indexing="ij")
        phi0 = np.stack([o.init_phi_random(Nx, Ny, o.DELTA_SEP, amp=0.1, seed=42)] * 2)
        _RAGGED[name] = dict(name=name, P=P, t=t, dts=dts, M=M, B=2, x=x, y=y, U=cos_controls(xx, yy, M, amp, 2),
                             H=directions(xx, yy, M, 2), phi0=phi0, W=[(5.0, 10.0, 1e-4)] * 2, fft=fft)
    return _RAGGED[name]


def _case(name):
    return ragged_problem(name) if name in RAGGED else problem(name)


# ---------------------------------------------------------------------------------------
# CPU: the three cases of this file meet their premises
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RAGGED))
def test_cases_meet_their_premises(name):
    pr = ragged_problem(name)
    P, orig, hists = pr["P"], o.newton_step, []
    assert pr["dts"].max() / pr["dts"].min() > 3.0 and len(pr["dts"]) == pr["M"]

    def recording(*a, **kw):
        kw["return_history"] = True
        ph, mu, h = orig(*a, **kw)
        hists.append(list(h))
        return ph, mu

    o.newton_step = recording
    try:
        marches = []
        for b in range(2):
            st = {}
            phi, _, t = o.forward(P, control=pr["U"][b], phi0=pr["phi0"][b], stats=st, dts=pr["dts"])
            marches.append((phi, np.array(st["mass_shifts"])))
            assert np.array_equal(t, pr["t"]) and phi.shape[0] == pr["M"] + 1
    finally:
        o.newton_step = orig
    assert len(hists) == 2 * pr["M"] and all(h[-1] < o.NEWTON_TOL for h in hists)
    assert all(len(h) < 20 for h in hists)
    for b, (phi, s) in enumerate(marches):
        top = float(np.abs(phi[1:]).max())
        print(f"{name} b={b}: max|phi[1:]| {top:.3f}, |shifts| {np.abs(s).min():.2e} .. {np.abs(s).max():.2e}, Newton norms "
              f"recorded at most {max(len(h) for h in hists)}")
        assert top < 0.985 - np.abs(s).max()
        if P.Nx != P.Ny:
            assert np.abs(s).min() > 1e-7
        if name == "long16":
            ratios = [_diag_ratio(P, phi[n + 1] + s[n], pr["dts"][n]) for n in range(pr["M"])]
            print(f"long16 b={b}: Dmax/Dmin {min(ratios):.2f} .. {max(ratios):.2f}")
            assert max(ratios) < 4.0
        phi_T, phi_Q = o.build_targets(pr["x"], pr["y"], pr["t"], phi[0], P.Lx, P.Ly, P.T)
        w, h = pr["W"][b], pr["H"][b]
        G, Hh = adjoint_reference(P, phi, pr["t"], s, pr["U"][b], phi_Q, phi_T, pr["x"], pr["y"], *w, h=h)
        d1, d2 = tangent_reference(P, phi, pr["t"], h, s)
        S = tangent_scalars(phi, d1, d2, pr["U"][b], h, phi_Q, phi_T, pr["x"], pr["y"], pr["t"], *w)
        e1, e2 = _ident(G * h, [S["s_state"], S["s_ctrl"]]), _ident(h * Hh, [S["c_gn"], S["c_state"], S["c_ctrl"]])
        print(f"{name} b={b}: the reference's identity 1 {e1:.2e}, 2 {e2:.2e}")
        assert e1 < BOUND[1]
        assert e2 < BOUND[2]


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


def _march(V, pr, bs=None):
    """A context of the trajectories bs (all by default) after its march, with targets, weights and the keyword arguments
    of the calls about it."""
    bs = list(range(pr["B"])) if bs is None else list(bs)
    P = pr["P"]
    eng = _engine(V, P, len(bs), max_steps=pr["M"])
    phi, _ = eng.forward(pr["phi0"][bs], pr["dts"], u=pr["U"][bs])
    phi = phi.reshape((len(bs),) + phi.shape[-3:])
    tg = [o.build_targets(pr["x"], pr["y"], pr["t"], phi[i][0], P.Lx, P.Ly, P.T) for i in range(len(bs))]
    kw = dict(phi_Q=np.stack([q for _, q in tg]), phi_T=np.stack([a for a, _ in tg]), x=pr["x"], y=pr["y"])
    opts = [V.make_opt(b1=pr["W"][b][0], b2=pr["W"][b][1], b3=pr["W"][b][2]) for b in bs]
    return eng, phi, kw, opts


def _run(V, name):
    """March, hessvec and second_order on one context.  The context stays open (eng) for the calls a test adds."""
    pr = _case(name)
    eng, phi, kw, opts = _march(V, pr)
    shifts = eng.mass_shifts()
    res = eng.hessvec(pr["H"], pr["dts"], pr["t"], opts, **kw)
    so = eng.second_order(pr["H"], pr["dts"], pr["t"], opts, **kw)
    return dict(pr, eng=eng, phi=phi, shifts=shifts, kw=kw, opts=opts, res=res, so=so, uses_fft=eng.uses_fft)


def _reference(r, b, h=None):
    return adjoint_reference(r["P"], r["phi"][b], r["t"], r["shifts"][b], r["U"][b], r["kw"]["phi_Q"][b], r["kw"]["phi_T"][b],
                             r["x"], r["y"], *r["W"][b], h=r["H"][b] if h is None else h)


def _dots_against_host_sums(name, res, H, bs):
    """dots are the device's sums of the n products the host sums here in another order: n eps sum|terms| apart at most."""
    rows, n = H.shape[1], H[0].size
    for b in bs:
        t0, t1 = res["grad"][b][:rows] * H[b], H[b] * res["hv"][b]
        d0, d1 = abs(res["dots"][b, 0] - t0.sum()), abs(res["dots"][b, 1] - t1.sum())
        assert d0 <= n * EPS * np.abs(t0).sum(), (name, b)
        assert d1 <= n * EPS * np.abs(t1).sum(), (name, b)
    assert np.array_equal(res["slope"], res["dots"][:, 0]) and np.array_equal(res["curvature"], res["dots"][:, 1])


def _check(r, ref_bs, id_bs=None):
    """Everything the module docstring lists for one case: trajectories ref_bs against the reference, id_bs (default: the
    same) in the identities and the dots."""
    name, eng, res, so, H, M, B = r["name"], r["eng"], r["res"], r["so"], r["H"], r["M"], r["B"]
    id_bs = list(ref_bs) if id_bs is None else list(id_bs)
    assert r["uses_fft"] == r["fft"]
    assert np.abs(r["phi"][:, 1:]).max() < 0.985 - np.abs(r["shifts"]).max()        # the premise, on the engine's own history
    if r["P"].Nx != r["P"].Ny:
        assert np.abs(r["shifts"]).min() > 1e-7                                      # the fix is at work on every step
    _check_stats(res["stats"], B, M, 2)
    assert res["grad"].shape == (B, M + 1) + eng.shape and res["hv"].shape == H.shape
    worst = dict(g=0.0, hv=0.0, id=0.0)
    for b in ref_bs:
        G, Hh = _reference(r, b)
        eg, eh = _rel(res["grad"][b], G), _rel(res["hv"][b], Hh)
        print(f"MEASURE {name} b={b}: grad {eg:.2e} hv {eh:.2e}")
        worst["g"], worst["hv"] = max(worst["g"], eg), max(worst["hv"], eh)
    # identity 4: the other direction of the pair on the same base point
    perm = np.arange(B) ^ 1
    perm[perm >= B] = B - 1
    Hg = H[perm]
    rg = eng.hessvec(Hg, r["dts"], r["t"], r["opts"], **r["kw"])
    _check_stats(rg["stats"], B, M, 2)
    assert np.array_equal(rg["grad"], res["grad"])
    for b in id_bs:
        e1 = _ident(res["grad"][b] * H[b], [so["s_state"][b], so["s_ctrl"][b]])
        e2 = _ident(H[b] * res["hv"][b], [so["c_gn"][b], so["c_state"][b], so["c_ctrl"][b]])
        a, c = Hg[b] * res["hv"][b], H[b] * rg["hv"][b]
        e4 = abs(float(a.sum()) - float(c.sum())) / (float(np.abs(a).sum()) + float(np.abs(c).sum()))
        print(f"MEASURE {name} b={b}: identity 1 {e1:.2e} 2 {e2:.2e} 4 {e4:.2e}")
        worst["id"] = max(worst["id"], e1, e2, e4)
    _dots_against_host_sums(name, res, H, id_bs)
    st = res["stats"]
    print(f"MEASURE {name}: grad {worst['g']:.2e} hv {worst['hv']:.2e} identities {worst['id']:.2e}; max_lin_relres "
          f"{st['max_lin_relres']:.2e}, sweeps per solve {st['linear_iters'] / max(1, st['linear_solves']):.1f}")
    tg, th, ti = _tol(name)
    assert worst["g"] < tg
    assert worst["hv"] < th
    assert worst["id"] < ti


def _closing(r):
    r["eng"].close()


@gpu
@pytest.mark.parametrize("name", ["tiles_gemm", "offA_14x11", "offB_14x11", "offA_sq", "offA_gemm", "offB_fft"])
def test_tiles_and_off_default_points(V, name):
    r = _run(V, name)
    try:
        _check(r, range(r["B"]))
    finally:
        _closing(r)


@gpu
def test_wide_diagonal(V):
    """The transposed solves under the right-scaled form: Dmax / Dmin > 4 on the engine's history."""
    r = _run(V, "wide")
    try:
        ratios = [_diag_ratio(r["P"], r["phi"][b][n + 1] + r["shifts"][b][n], r["dts"][n]) for b in range(2) for n in range(r["M"])]
        print(f"MEASURE wide: Dmax/Dmin on the engine's history {[round(v, 1) for v in ratios]}")
        assert min(ratios) > 4.0
        _check(r, range(2))
    finally:
        _closing(r)


@gpu
@pytest.mark.parametrize("name", ["batch33", "batch40"])
def test_batches_above_32(V, name):
    r = _run(V, name)
    try:
        B = r["B"]
        assert len({tuple(w) for w in r["W"]}) == B
        _check(r, sorted({0, 1, 16, 31, 32, B - 1}))
        if name == "batch33":
            # the promise of vch2d_create: a member of a batch has the bits of a context of its own
            for b in (0, 31, 32):
                eng, phi, kw, opts = _march(V, r, [b])
                try:
                    assert np.array_equal(phi[0], r["phi"][b])
                    one = eng.hessvec(r["H"][b], r["dts"], r["t"], opts, **kw)
                finally:
                    eng.close()
                for k in ("grad", "hv", "dots"):
                    assert np.array_equal(one[k][0], r["res"][k][b]), (k, b)
    finally:
        _closing(r)


@gpu
def test_more_than_64_tiles(V):
    r = _run(V, "many_tiles")
    try:
        assert (-(-(r["P"].Nx + 1) // 64)) * (-(-(r["P"].Ny + 1) // 16)) > 64
        _check(r, [0], id_bs=range(2))
    finally:
        _closing(r)


@gpu
@pytest.mark.parametrize("name", list(RAGGED))
def test_ragged_steps(V, name):
    r = _run(V, name)
    try:
        assert r["dts"].max() / r["dts"].min() > 3.0
        _check(r, range(2))
        if name == "long16":
            ratios = [_diag_ratio(r["P"], r["phi"][b][n + 1] + r["shifts"][b][n], r["dts"][n]) for b in range(2)
                      for n in range(r["M"])]
            assert max(ratios) < 4.0                 # the plain form: the right-scaled one is `wide`'s
            _check_short_direction(r)
    finally:
        _closing(r)


def _check_short_direction(r):
    """The row rule: a direction of SHORT_ROWS rows < M + 1 drives no step from its last row on."""
    eng, M, name = r["eng"], r["M"], r["name"] + f" {SHORT_ROWS} rows"
    Hs = np.ascontiguousarray(r["H"][:, :SHORT_ROWS])
    args = (r["dts"], r["t"], r["opts"])
    res = eng.hessvec(Hs, *args, **r["kw"])
    so = eng.second_order(Hs, *args, **r["kw"])
    _check_stats(res["stats"], 2, M, 2)
    assert res["hv"].shape == Hs.shape and np.array_equal(res["grad"], r["res"]["grad"])
    Hp = _pad(Hs, M + 1)
    r1 = eng.hessvec(Hp, *args, order=1, **r["kw"])
    s1 = eng.second_order(Hp, *args, order=1, **r["kw"])
    eh = eid = 0.0
    for b in range(2):
        _, Hh = _reference(r, b, h=Hs[b])
        assert not np.array_equal(_reference(r, b, h=Hp[b])[1][:SHORT_ROWS], Hh)        # the padded direction is another one
        e = _rel(res["hv"][b], Hh)
        e2 = _ident(Hs[b] * res["hv"][b], [so["c_gn"][b], so["c_state"][b], so["c_ctrl"][b]])
        e1 = _ident(r1["grad"][b] * Hp[b], [s1["s_state"][b], s1["s_ctrl"][b]])
        print(f"MEASURE {name} b={b}: hv {e:.2e} identity 2 {e2:.2e} identity 1 (padded direction) {e1:.2e}")
        eh, eid = max(eh, e), max(eid, e1, e2)
    _dots_against_host_sums(name, res, Hs, range(2))
    _, th, ti = _tol(r["name"])
    assert eh < th
    assert eid < ti
