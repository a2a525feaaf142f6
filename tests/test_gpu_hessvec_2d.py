"""vch2d_hessvec on the GPU: the exact gradient field G = d(J1+J2+J3)/du and the Hessian-vector product H h of the 2D
engine (transposed sweep of the tangent march) against CPU linear algebra (tests/_adjoint_ref.py, the
plain-transpose form with sparse direct solves, pinned to the tangent reference by test_adjoint_cpu.py) and against
vch2d_second_order on the same context.  The engine marches, its state history and mass_shifts() are pulled and fed to the
CPU reference, as test_gpu_second_order.py does.

Cases, batch 3 each (white-noise direction, smooth direction, h == 0; every trajectory its own control):
    fft16      16 x 16, T = 0.045, dt = 0.01: stencil-free FFT path, ragged last step
    gemm14x11  14 x 11: GEMM-DCT path, the weights wq of the stored plane differ from the mass fix's (shifts non-zero)
    fft32x16   32 x 16, a direction of 3 rows < M + 1: rectangular FFT and the row rule
    tiles      128 x 32 (Lx 1, Ly 0.5), M = 2: 3 x 3 tiles, an interior tile on both axes, halos across tile edges
    fft16 under VCH_FORCE_GEMM_DCT=1

Error measures.  Fields: max-norm of the difference over the max-norm of the reference, per trajectory.  Identities
(1: sum G h = slope, 2: sum h Hh = curvature, 4: sum g Hh = sum h Hg; slope and curvature from Engine2D.second_order on the
same context): the difference over the sum of the absolute values of all terms of both sides.  Identity 1 needs
h_rows == g_rows (the row rule), so fft32x16 checks it with the direction padded by zero rows to M + 1, a direction in its
own right.  `dots` (reduced on the device) against the host's sums of the returned fields: both are sums of the same n
products in another order, so they differ by at most n eps sum|terms| (n = nodes of the direction, eps = 2.3e-16); that
bound is asserted, not a measured one.

Measured on an MI355X at the default rtol = 1e-12, worst over all cases, weights and the PGD iterate:
    grad 5.4e-13 (tiles)   hv 1.03e-12 (PGD iterate)   identities 6.1e-14 (identity 1 at the PGD iterate)
    (per case, grad / hv / identities: fft16 3.4e-13 / 5.3e-13 / 3.8e-14, gemm14x11 2.8e-13 / 6.1e-13 / 8.4e-15, fft32x16
     2.5e-13 / 5.0e-13 / 4.4e-15, tiles 5.4e-13 / 5.6e-14 / 2.0e-16, fft16 through the GEMM-DCT 3.4e-13 / 5.2e-13 / 3.8e-14,
     per-trajectory weights 1.7e-14 / 4.9e-14, PGD iterate 2.5e-13 / 1.03e-12 / 6.1e-14; the solves' own worst final
     relative residual 6.3e-13)
    dense Hessian 12 x 9, M = 2 (390 unit directions): asymmetry 7.5e-15, against the reference's matrix 8.3e-15
    (both relative to the largest entry), eigenvalues against the reference's 2.3e-14 of the largest
Asserted: 10 x measured per class: 5.4e-12, 1.1e-11, 6.1e-13; 7.5e-14, 8.4e-14, 2.3e-13 -- all below the 1.5e-11 class of
test_gpu_second_order.py.  Every call must report unconverged_solves == 0 and max_lin_relres <= rtol.
Driver: with k >= n_free both extreme Ritz values of reduced_hessian_extremes_2d equal eigvalsh of the dense masked Hessian
to 10 n eps of the largest eigenvalue (n = 390; the rule of the 1D test): DRIVER_RITZ = 9.0e-13; measured 4.4e-14
(190 free nodes of 390).  theta_min of a box that is nowhere active is not above the curvature of any direction the exact
condition samples there (1.157e-9 against 5.9e-9 .. 6.3e-9)."""
import contextlib
import io
import math

import numpy as np
import pytest

from oracle import vch2d_oracle as o
from _adjoint_ref import adjoint_reference
from test_gpu_forms import _env
from test_gpu_second_order import WEIGHTS

pytestmark = pytest.mark.gpu

EPS = 2.3e-16
TOL_G, TOL_HV, TOL_ID = 5.4e-12, 1.1e-11, 6.1e-13
DENSE_SYM, DENSE_REF, DENSE_EIG = 7.5e-14, 8.4e-14, 2.3e-13
DRIVER_RITZ = 10 * 390 * EPS
assert max(TOL_G, TOL_HV, TOL_ID, DENSE_SYM, DENSE_REF, DENSE_EIG, DRIVER_RITZ) <= 1.5e-11

CASES = {
    #            Nx   Ny  Lx   Ly   T      dt    rows of h (None: M + 1)   uses_fft
    "fft16":     (16, 16, 1.0, 1.0, 0.045, 0.01, None, True),
    "gemm14x11": (14, 11, 1.0, 1.0, 0.04, 0.01, None, False),
    "fft32x16":  (32, 16, 1.0, 1.0, 0.04, 0.01, 3, True),
    "tiles":     (128, 32, 1.0, 0.5, 0.02, 0.01, None, True),
}


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


def _engine(V, P, batch, max_steps=8):
    return V.Engine2D(P.Nx, P.Ny, P.Lx, P.Ly, P.tau, P.gamma, P.c1, P.c2, P.kappa, batch=batch, max_steps=max_steps)


def _problem(name):
    Nx, Ny, Lx, Ly, T, dt, rows, fft = CASES[name]
    P = o.Params2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, T=T, dt_initial=dt)
    t, dts = o.time_grid(T, dt)
    M = len(dts)
    x, y = np.linspace(0.0, Lx, Nx + 1), np.linspace(0.0, Ly, Ny + 1)
    xx, yy = np.meshgrid(x / Lx, y / Ly, indexing="ij")
    ctrl = lambda amp, s: amp * np.stack([np.cos(np.pi * xx * (1 + (k + s) % 3)) * np.cos(np.pi * yy) * np.sin(1 + k + s)
                                          for k in range(M + 1)])
    U = np.stack([ctrl(20.0, 0), ctrl(-12.0, 1), ctrl(8.0, 2)])
    rows = M + 1 if rows is None else rows
    noise = np.random.default_rng(3).standard_normal((rows, Nx + 1, Ny + 1))
    smooth = np.stack([np.cos(2 * np.pi * xx) * np.cos(np.pi * yy) * np.cos(0.3 * k) for k in range(rows)])
    H = np.stack([noise / np.abs(noise).max(), smooth, np.zeros_like(smooth)])
    phi0 = np.stack([o.init_phi_random(Nx, Ny, o.DELTA_SEP, amp=0.1, seed=42 + b) for b in range(3)])
    return dict(name=name, P=P, t=t, dts=dts, M=M, x=x, y=y, U=U, H=H, phi0=phi0, fft=fft)


def _check_stats(st, B, M, order, rtol=1e-12):
    assert st["unconverged_solves"] == 0, st
    assert st["max_lin_relres"] <= rtol, st
    assert st["linear_solves"] == (3 if order == 2 else 1) * B * M, st


def _run(V, name, env=None):
    """The batch-3 march, hessvec and second_order on the same context, and the CPU reference on the engine's own history."""
    pr = _problem(name)
    P = pr["P"]
    with _env(**(env or {})):
        eng = _engine(V, P, 3)
    phi, _ = eng.forward(pr["phi0"], pr["dts"], u=pr["U"])
    shifts = eng.mass_shifts()
    tg = [o.build_targets(pr["x"], pr["y"], pr["t"], phi[b][0], P.Lx, P.Ly, P.T) for b in range(3)]
    phi_T, phi_Q = np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])
    opt = V.make_opt()
    kw = dict(phi_Q=phi_Q, phi_T=phi_T, x=pr["x"], y=pr["y"])
    res = eng.hessvec(pr["H"], pr["dts"], pr["t"], opt, **kw)
    so = eng.second_order(pr["H"], pr["dts"], pr["t"], opt, **kw)
    w = (opt.b1, opt.b2, opt.b3)
    ref = [adjoint_reference(P, phi[b], pr["t"], shifts[b], pr["U"][b], phi_Q[b], phi_T[b], pr["x"], pr["y"], *w, h=pr["H"][b])
           for b in range(3)]
    pr.update(eng=eng, phi=phi, shifts=shifts, phi_T=phi_T, phi_Q=phi_Q, res=res, so=so, ref=ref, opt=opt, kw=kw, w=w)
    return pr


@pytest.fixture(scope="module")
def runs(V):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(V, name)
        return cache[name]

    yield get
    for pr in cache.values():
        pr["eng"].close()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _ident(terms, parts):
    """|sum terms - sum parts| over the sum of the absolute values of all terms of both sides."""
    parts = np.atleast_1d(np.asarray(parts, dtype=float))
    return abs(float(np.sum(terms)) - float(np.sum(parts))) / (float(np.sum(np.abs(terms))) + float(np.sum(np.abs(parts))))


def _pad(h, rows):
    out = np.zeros(h.shape[:1] + (rows,) + h.shape[2:])
    out[:, :h.shape[1]] = h
    return out


def _check_case(V, pr):
    name, eng, res, so, H, M = pr["name"], pr["eng"], pr["res"], pr["so"], pr["H"], pr["M"]
    rows = H.shape[1]
    assert eng.uses_fft == (pr["fft"] and not pr.get("forced"))
    assert np.abs(pr["phi"]).max() < 1.0 - o.DELTA_SEP - 0.1          # the clip the scheme ignores is inactive
    if pr["P"].Nx != pr["P"].Ny:
        assert np.abs(pr["shifts"][:2]).min() > 1e-7                  # rectangular grid: the mass fix shifts every step
    _check_stats(res["stats"], 3, M, 2)
    assert res["grad"].shape == (3, M + 1) + eng.shape and res["hv"].shape == H.shape
    worst = dict(g=0.0, hv=0.0, id=0.0)
    for b in range(3):
        G, Hh = pr["ref"][b]
        worst["g"] = max(worst["g"], _rel(res["grad"][b], G))
        if b < 2:
            worst["hv"] = max(worst["hv"], _rel(res["hv"][b], Hh))
    # h == 0: hv exactly zero
    assert not res["hv"][2].any() and res["dots"][2, 1] == 0.0 and res["dots"][2, 0] == 0.0
    # identity 2 against second_order, identity 1 where the rows agree (else with the padded direction, below)
    for b in range(2):
        e2 = _ident(H[b] * res["hv"][b], [so["c_gn"][b], so["c_state"][b], so["c_ctrl"][b]])
        worst["id"] = max(worst["id"], e2)
        print(f"MEASURE {name} b={b}: identity 2 {e2:.2e}")
        if rows == M + 1:
            e1 = _ident(res["grad"][b] * H[b], [so["s_state"][b], so["s_ctrl"][b]])
            worst["id"] = max(worst["id"], e1)
            print(f"MEASURE {name} b={b}: identity 1 {e1:.2e}")
    if rows != M + 1:
        Hp = _pad(H, M + 1)
        r1 = eng.hessvec(Hp, pr["dts"], pr["t"], pr["opt"], order=1, **pr["kw"])
        s1 = eng.second_order(Hp, pr["dts"], pr["t"], pr["opt"], order=1, **pr["kw"])
        for b in range(2):
            e1 = _ident(r1["grad"][b] * Hp[b], [s1["s_state"][b], s1["s_ctrl"][b]])
            worst["id"] = max(worst["id"], e1)
            print(f"MEASURE {name} b={b}: identity 1 (padded direction) {e1:.2e}")
    # identity 4: the other direction of the pair on the same base point
    Hg = H[[1, 0, 2]]
    rg = eng.hessvec(Hg, pr["dts"], pr["t"], pr["opt"], **pr["kw"])
    _check_stats(rg["stats"], 3, M, 2)
    assert np.array_equal(rg["grad"], res["grad"])
    for b in range(2):
        a, c = Hg[b] * res["hv"][b], H[b] * rg["hv"][b]
        e4 = abs(float(a.sum()) - float(c.sum())) / (float(np.abs(a).sum()) + float(np.abs(c).sum()))
        worst["id"] = max(worst["id"], e4)
        print(f"MEASURE {name} b={b}: identity 4 {e4:.2e}")
    # dots against the host's sums of the returned fields (n eps sum|terms|: another order of the same sum)
    n = H[0].size
    for b in range(3):
        t0, t1 = res["grad"][b][:rows] * H[b], H[b] * res["hv"][b]
        assert abs(res["dots"][b, 0] - t0.sum()) <= n * EPS * np.abs(t0).sum()
        assert abs(res["dots"][b, 1] - t1.sum()) <= n * EPS * np.abs(t1).sum()
    assert np.array_equal(res["slope"], res["dots"][:, 0]) and np.array_equal(res["curvature"], res["dots"][:, 1])
    print(f"MEASURE {name}: grad {worst['g']:.2e} hv {worst['hv']:.2e} identities {worst['id']:.2e}; "
          f"max_lin_relres {res['stats']['max_lin_relres']:.2e}; stats {res['stats']}")
    assert worst["g"] < TOL_G
    assert worst["hv"] < TOL_HV
    assert worst["id"] < TOL_ID


@pytest.mark.parametrize("name", list(CASES))
def test_fields_identities_and_dots(V, runs, name):
    _check_case(V, runs(name))


def test_gemm_dct_variant_of_the_square_case(V, runs):
    pr = _run(V, "fft16", env=dict(VCH_FORCE_GEMM_DCT=1))
    pr["forced"] = True
    try:
        assert runs("fft16")["eng"].uses_fft and not pr["eng"].uses_fft
        _check_case(V, pr)
    finally:
        pr["eng"].close()


@pytest.mark.parametrize("name", list(CASES))
def test_order_one_gradient_is_order_twos(runs, name):
    pr = runs(name)
    r1 = pr["eng"].hessvec(pr["H"], pr["dts"], pr["t"], pr["opt"], order=1, **pr["kw"])
    assert np.array_equal(r1["grad"], pr["res"]["grad"]) and r1["hv"] is None
    assert np.array_equal(r1["dots"][:, 0], pr["res"]["dots"][:, 0]) and np.isnan(r1["dots"][:, 1]).all()
    _check_stats(r1["stats"], 3, pr["M"], 1)
    g = pr["eng"].exact_gradient(pr["dts"], pr["t"], pr["opt"], **pr["kw"])
    assert np.array_equal(g, pr["res"]["grad"])


@pytest.mark.parametrize("name", list(CASES))
def test_batch_of_three_equals_three_single_contexts(V, runs, name):
    pr = runs(name)
    for b in range(3):
        eng = _engine(V, pr["P"], 1)
        phi, _ = eng.forward(pr["phi0"][b], pr["dts"], u=pr["U"][b])
        assert np.array_equal(phi, pr["phi"][b])
        r = eng.hessvec(pr["H"][b], pr["dts"], pr["t"], pr["opt"], phi_Q=pr["phi_Q"][b], phi_T=pr["phi_T"][b], x=pr["x"],
                        y=pr["y"])
        eng.close()
        assert np.array_equal(r["grad"][0], pr["res"]["grad"][b]), b
        assert np.array_equal(r["hv"][0], pr["res"]["hv"][b]), b
        assert np.array_equal(r["dots"][0], pr["res"]["dots"][b]), b


def test_per_trajectory_weights_against_the_scalar_form(V, runs):
    pr = runs("gemm14x11")
    eng = pr["eng"]
    opts = [V.make_opt(b1=w[0], b2=w[1], b3=w[2]) for w in WEIGHTS]
    many = eng.hessvec(pr["H"], pr["dts"], pr["t"], opts, **pr["kw"])
    _check_stats(many["stats"], 3, pr["M"], 2)
    for b, w in enumerate(WEIGHTS):
        one = eng.hessvec(pr["H"], pr["dts"], pr["t"], opts[b], **pr["kw"])
        for k in ("grad", "hv", "dots"):
            assert np.array_equal(many[k][b], one[k][b]), (k, b)
        G, Hh = adjoint_reference(pr["P"], pr["phi"][b], pr["t"], pr["shifts"][b], pr["U"][b], pr["phi_Q"][b], pr["phi_T"][b],
                                  pr["x"], pr["y"], *w, h=pr["H"][b])
        eg = _rel(many["grad"][b], G)
        print(f"MEASURE weights {w} b={b}: grad {eg:.2e}")
        assert eg < TOL_G
        if b < 2:
            eh = _rel(many["hv"][b], Hh)
            print(f"MEASURE weights {w} b={b}: hv {eh:.2e}")
            assert eh < TOL_HV


def test_pgd_iterate_is_not_disturbed_and_the_iterate_is_the_base_point(V):
    N, T, dt = 16, 0.05, 0.01
    P = o.Params2D(Nx=N, Ny=N, T=T, dt_initial=dt)
    t, dts = o.time_grid(T, dt)
    x = np.linspace(0.0, 1.0, N + 1)
    phi0 = np.stack([o.init_phi_random(N, N, o.DELTA_SEP, amp=0.1, seed=42 + b) for b in range(2)])
    phi_T = np.stack([o.build_targets(x, x, t, phi0[b], P.Lx, P.Ly, P.T)[0] for b in range(2)])
    opts = [V.make_opt(), V.make_opt(b1=2.0, b2=4.0, b3=1e-3)]
    noise = np.random.default_rng(5).standard_normal((2, len(t), N + 1, N + 1))
    H = noise / np.abs(noise).max()

    def start():
        eng = _engine(V, P, 2)
        eng.pgd_init(phi0, phi_T, t, opts, ramp=True, T=T)
        eng.pgd_iterate(2)
        return eng

    plain = start()
    want = plain.pgd_iterate(1)
    u_want = plain.pgd_get("u")
    plain.close()
    eng = start()
    u, phi, phi_Q = eng.pgd_get("u"), eng.pgd_get("phi"), eng.pgd_get("phi_Q")
    res = eng.hessvec(H, opt=opts)
    so = eng.second_order(H, opt=opts)
    _check_stats(res["stats"], 2, len(dts), 2)
    shifts = eng.mass_shifts()
    assert np.array_equal(eng.pgd_get("u"), u) and np.array_equal(eng.pgd_get("phi"), phi)
    assert np.abs(u).max() > 0 and res["grad"].shape == u.shape
    for b in range(2):
        G, Hh = adjoint_reference(P, phi[b], t, shifts[b], u[b], phi_Q[b], phi_T[b], x, x, opts[b].b1, opts[b].b2, opts[b].b3,
                                  h=H[b])
        eg, eh = _rel(res["grad"][b], G), _rel(res["hv"][b], Hh)
        e1 = _ident(res["grad"][b] * H[b], [so["s_state"][b], so["s_ctrl"][b]])
        e2 = _ident(H[b] * res["hv"][b], [so["c_gn"][b], so["c_state"][b], so["c_ctrl"][b]])
        print(f"MEASURE pgd b={b}: grad {eg:.2e} hv {eh:.2e} identity 1 {e1:.2e} identity 2 {e2:.2e}")
        assert eg < TOL_G and eh < TOL_HV and max(e1, e2) < TOL_ID
    got = eng.pgd_iterate(1)
    for k in ("cost", "alpha", "attempts", "change", "tracking_error", "terminal_error"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(eng.pgd_get("u"), u_want)
    with pytest.raises(ValueError):          # the resident problem has its own targets
        eng.hessvec(H, opt=opts, phi_T=phi_T)
    with pytest.raises(ValueError):          # ... and its control has M + 1 rows
        eng.hessvec(H, opt=opts, g_rows=len(dts))
    eng.close()


def test_error_codes_come_before_any_launch(V, runs):
    pr = runs("fft16")
    fresh = _engine(V, pr["P"], 3)
    c0 = fresh.counters()
    with pytest.raises(V.VchError, match="-3"):
        fresh.hessvec(pr["H"], pr["dts"], pr["t"], pr["opt"])
    assert fresh.counters() == c0
    fresh.close()
    eng, H, dts, t, opt, M = pr["eng"], pr["H"], pr["dts"], pr["t"], pr["opt"], pr["M"]
    c0 = eng.counters()
    bad = [
        dict(h=H, dt=dts[:-1], t_hist=t[:-1], opt=opt),                                   # M != M_res
        dict(h=H, dt=dts, t_hist=t, opt=[opt, opt]),                                      # n_opts neither 1 nor B
        dict(h=H, dt=dts, t_hist=t, opt=opt, order=3),
        dict(h=H, dt=dts, t_hist=t, opt=opt, order=0),
        dict(h=np.zeros((3, eng.max_steps + 2) + eng.shape), dt=dts, t_hist=t, opt=opt),   # h_rows > max_steps + 1
        dict(h=H, dt=dts, t_hist=t, opt=V.make_opt(b1=math.nan)),
        dict(h=H, dt=dts, t_hist=t, opt=[opt, opt, V.make_opt(b3=math.inf)]),
        dict(h=H, dt=dts, t_hist=t, opt=opt, g_rows=M),                                   # the march's control has M + 1 rows
        dict(h=H, dt=dts, t_hist=t, opt=opt, g_rows=0),
        dict(h=None, dt=dts, t_hist=t, opt=opt, order=2),                                 # NULL h at order 2
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.hessvec(**kw)
        assert eng.counters() == c0, kw.keys()
    # NULL hv_out at order 2, and the outputs of a refused call stay untouched (the raw entry point)
    _lib = V.module("_lib")
    dp = lambda a: a.ctypes.data_as(_lib._D)
    Hc = np.ascontiguousarray(H)
    grad, hv, dots = (np.full((3, M + 1) + eng.shape, 7.0), np.full(H.shape, 7.0), np.full((3, 2), 7.0))
    xs, ys = np.ascontiguousarray(pr["x"]), np.ascontiguousarray(pr["y"])
    dtc, tc = np.ascontiguousarray(dts, dtype=np.float64), np.ascontiguousarray(t, dtype=np.float64)
    arr = (_lib.OptParams * 1)(opt)
    call = lambda g_rows, hvp: eng.lib.vch2d_hessvec(eng.ctx, dp(Hc), H.shape[1], g_rows, dp(dtc), M, dp(tc), dp(xs), dp(ys),
                                                     None, None, arr, 1, 2, 0.0, dp(grad), hvp, dp(dots), None)
    assert call(M + 1, None) == -1 and call(M, dp(hv)) == -1
    assert (grad == 7.0).all() and (hv == 7.0).all() and (dots == 7.0).all() and eng.counters() == c0
    # ... and the context still answers, with the bits of the first call
    again = eng.hessvec(H, dts, t, opt, **pr["kw"])
    for k in ("grad", "hv", "dots"):
        assert np.array_equal(again[k], pr["res"][k]), k
    launches, looks = eng.counters()
    assert launches - c0[0] == again["stats"]["launches"] and looks - c0[1] == again["stats"]["host_syncs"]
    # after a forward without a control any g_rows in 1..M+1 is the zero control of that many rows
    eng0 = _engine(V, pr["P"], 3)
    eng0.forward(pr["phi0"], dts)
    full = eng0.hessvec(None, dts, t, opt, order=1, **pr["kw"])
    part = eng0.hessvec(None, dts, t, opt, order=1, g_rows=3, **pr["kw"])
    assert full["grad"].shape[1] == M + 1 and part["grad"].shape[1] == 3 and np.isnan(part["dots"]).all()
    assert np.array_equal(part["grad"][:, :2], full["grad"][:, :2]) and not np.array_equal(part["grad"][:, 2], full["grad"][:, 2])
    with pytest.raises(ValueError):
        eng0.hessvec(None, dts, t, opt, order=1, g_rows=M + 2, **pr["kw"])
    eng0.close()


# ---------------------------------------------------------------------------------------------------------------------
# dense Hessian and the driver, 12 x 9, M = 2: 3 x 13 x 10 = 390 unit directions
# ---------------------------------------------------------------------------------------------------------------------
DN = dict(Nx=12, Ny=9, T=0.02, dt=0.01, u_min=-0.5, u_max=0.5, seed=11)


@pytest.fixture(scope="module")
def dense(V):
    """The dense Hessian about the driver problem's base point from 13 calls of batch 30, and the reference's matrix."""
    K2 = V.module("Vch_control_2D.config")
    F2 = V.module("Vch_control_2D.Forward2_solver")
    Nx, Ny, T, dt = DN["Nx"], DN["Ny"], DN["T"], DN["dt"]
    # the mirror's config validates Nx, Ny > 10 (the reference's rule); the engine and the driver do not need it
    cfg = K2.ForwardSolverConfig.model_construct(Nx=Nx, Ny=Ny, T=T, dt_initial=dt)
    opt = K2.OptimizationConfig()
    P = o.Params2D(Nx=Nx, Ny=Ny, Lx=cfg.Lx, Ly=cfg.Ly, tau=cfg.tau, gamma=cfg.gamma, c1=cfg.c1, c2=cfg.c2, kappa=cfg.kappa,
                   T=T, dt_initial=dt)
    t, dts = V.time_grid(T, dt)
    M = len(dts)
    assert M == 2
    x, y = np.linspace(0.0, cfg.Lx, Nx + 1), np.linspace(0.0, cfg.Ly, Ny + 1)
    xx, yy = np.meshgrid(x / cfg.Lx, y / cfg.Ly, indexing="ij")
    u_star = np.clip(np.stack([1.4 * np.cos(np.pi * xx * (1 + k % 3)) * np.cos(np.pi * yy) * np.sin(1 + k) for k in range(M + 1)]),
                     DN["u_min"], DN["u_max"])
    phi0 = F2.init_phi_random(Nx, Ny, 1e-2, amp=0.1, seed=42)
    nd, nb = u_star.size, 30
    assert nd == 390 and nd % nb == 0
    eng = V.Engine2D(Nx, Ny, cfg.Lx, cfg.Ly, cfg.tau, cfg.gamma, cfg.c1, cfg.c2, cfg.kappa, batch=nb, max_steps=M)
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (nb,) + a.shape))
    phi, _ = eng.forward(tile(phi0), dts, u=tile(u_star))
    shifts = eng.mass_shifts()
    phi_T, phi_Q = o.build_targets(x, y, t, phi[0][0], cfg.Lx, cfg.Ly, T)
    mo = V.make_opt(opt)
    Hd = np.empty((nd, nd))
    for k0 in range(0, nd, nb):
        E = np.zeros((nb, nd))
        E[np.arange(nb), k0 + np.arange(nb)] = 1.0
        r = eng.hessvec(E.reshape((nb,) + u_star.shape), dts, t, mo, phi_Q=tile(phi_Q), phi_T=tile(phi_T), x=x, y=y)
        _check_stats(r["stats"], nb, M, 2)
        Hd[:, k0:k0 + nb] = r["hv"].reshape(nb, nd).T
    eng.close()
    cache = {}
    Hr = np.empty((nd, nd))
    for j in range(nd):
        e = np.zeros(nd)
        e[j] = 1.0
        Hr[:, j] = adjoint_reference(P, phi[0], t, shifts[0], u_star, phi_Q, phi_T, x, y, mo.b1, mo.b2, mo.b3,
                                     h=e.reshape(u_star.shape), cache=cache)[1].ravel()
    return dict(cfg=cfg, opt=opt, P=P, t=t, dts=dts, x=x, y=y, u_star=u_star, phi_T=phi_T, phi_Q=phi_Q, Hd=Hd, Hr=Hr, nd=nd)


def test_dense_hessian_symmetry_reference_and_spectrum(dense):
    Hd, Hr = dense["Hd"], dense["Hr"]
    top = np.abs(Hr).max()
    sym = np.abs(Hd - Hd.T).max() / top
    dev = np.abs(Hd - Hr).max() / top
    ev, er = np.linalg.eigvalsh(0.5 * (Hd + Hd.T)), np.linalg.eigvalsh(0.5 * (Hr + Hr.T))
    eig = np.abs(ev - er).max() / np.abs(er).max()
    print(f"MEASURE dense: asymmetry {sym:.2e} (reference's own {np.abs(Hr - Hr.T).max() / top:.2e}) against the reference {dev:.2e} "
          f"eigenvalues {eig:.2e}; spectrum {er[0]:.4e} .. {er[-1]:.4e}")
    assert sym < DENSE_SYM
    assert dev < DENSE_REF
    assert eig < DENSE_EIG


def test_driver_extremes_of_the_reduced_hessian(V, dense):
    S2 = V.module("Vch_control_2D.second_order_conditions_2d")
    D, nd = dense, dense["nd"]
    u_star, Hm = D["u_star"], 0.5 * (D["Hd"] + D["Hd"].T)
    kw = dict(x=D["x"], y=D["y"], t_hist=D["t"], opt_config=D["opt"], phi_Q_target=D["phi_Q"], phi_T_target=D["phi_T"],
              fwd_config=D["cfg"])
    mask = S2.free_set(u_star, DN["u_min"], DN["u_max"]).ravel()
    assert 0 < mask.sum() < nd and (np.abs(u_star) >= DN["u_max"] - 1e-8).any()         # the box pins part of the nodes
    ev = np.linalg.eigvalsh(Hm[np.ix_(mask, mask)])
    R = S2.reduced_hessian_extremes_2d(u_star, u_min=DN["u_min"], u_max=DN["u_max"], k=nd, seed=DN["seed"], **kw)
    dev = max(abs(R["theta_min"] - ev[0]), abs(R["theta_max"] - ev[-1])) / abs(ev[-1])
    print(f"MEASURE driver: n_free {R['n_free']} of {nd}, steps {R['steps']}, theta_min {R['theta_min']:.6e} eigvalsh {ev[0]:.6e} "
          f"theta_max {R['theta_max']:.6e} eigvalsh {ev[-1]:.6e} rel.dev {dev:.2e}, residuals {R['res_min']:.1e} {R['res_max']:.1e}")
    assert R["n_free"] == mask.sum() and R["steps"] <= R["n_free"]
    assert dev < DRIVER_RITZ
    # a box that is nowhere active, a control off the kink: every node is free and the sampled directions of the exact
    # condition are free-set directions
    wide, shift = 5.0, 0.75
    u_b = u_star + shift
    assert S2.free_set(u_b, -wide, wide).all()
    r_star = np.zeros_like(u_b)
    phi_b, _, _ = V.module("Vch_control_2D.Forward2_solver").run_main_simulation(D["cfg"], store_history=True, control_input=u_b,
                                                                                verbose=False)
    with contextlib.redirect_stdout(io.StringIO()):
        exact = S2.exact_second_order_condition_2d(u_b, r_star, phi_b, u_min=-wide, u_max=wide, num_directions=4,
                                                   seed=DN["seed"], **kw)
    Rw = S2.reduced_hessian_extremes_2d(u_b, u_min=-wide, u_max=wide, k=nd, seed=DN["seed"], **kw)
    print(f"MEASURE driver wide box: theta_min {Rw['theta_min']:.6e} theta_max {Rw['theta_max']:.6e} curvatures {exact}")
    assert Rw["n_free"] == nd and Rw["steps"] <= nd
    assert all(Rw["theta_min"] <= c for c in exact)
