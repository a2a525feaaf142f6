"""vch2d_second_order and vch2d_hessvec about states OUTSIDE the interior band of the march's mass fix (tests/_fix_band.py):
plateaus in [0.985, 0.99) that the fix skips, fronts inside the band that it shifts.  There phi* = phi_{n+1} + s_n on the
fix's set and phi_{n+1} on the skipped nodes, the linearised fix divides by the weight W_int the march recorded, and a
history from which the set cannot be told (the classified weight differs from W_int, either way) is refused.

The engine marches; its state history and mass_shifts() are pulled and fed to the CPU references (tests/_tangent_ref.py,
tests/_adjoint_ref.py, pinned on these inputs against central differences by test_tangent_cpu.py / test_adjoint_cpu.py).  The
fix's sets come from the ORACLE's march of the same input: the engine's history agrees with the oracle's to MARCH = 1e-8 (asserted)
and no node of a qualified input lies within 1e-6 of the threshold, nor a skipped one within 10 |s_n|, so both marches take
the same decisions.

Batch 3 per grid (32 x 16 FFT; 128 x 32 FFT, 3 x 3 tiles; 50 x 36 GEMM-DCT), mixed:
    0  band trajectory, white-noise direction      1  all-interior trajectory (init_phi_random(amp=0.1)), smooth direction
    2  band trajectory, h == 0
Error measures as in test_gpu_second_order.py (fields: max-norm over the reference's max-norm; scalars: relative) and
test_gpu_hessvec_2d.py (identities over the sum of |terms|; `dots` under n eps sum|terms|).  Every call must report
unconverged_solves == 0 and max_lin_relres <= rtol = 1e-12.

Solve form: Dmax / Dmin of the Newton diagonal is 6.2 .. 7.5 on the band inputs (plateau 2 c1 / (1 - phi^2) = 30 against
0.8 on the front -- a ratio of 40 -- plus tau / dt = 5 on both), above the engine's threshold 4: on the FFT grids these
solves run right-scaled (asserted on the CPU by test_tangent_cpu.py::test_band_diagonals_exceed_the_right_scaling_threshold).

Measured on an MI355X at rtol = 1e-12 (worst over trajectories 0 and 1; the engine's march against the oracle's: 4.5e-14 ..
3.0e-12, under MARCH):
    case                     dphi     d2phi    scalars  grad     hv       identities
    32x16                    1.8e-12  2.7e-12  6.2e-13  4.3e-13  4.0e-12  4.0e-14
    128x32                   9.8e-12  4.2e-12  3.9e-12  3.0e-12  5.5e-12  1.9e-13
    50x36 (GEMM-DCT)         1.35e-11 4.08e-11 4.77e-11 1.46e-11 2.03e-11 4.6e-13
    32x16 through GEMM-DCT   3.3e-12  1.32e-11 2.2e-12  8.21e-12 1.67e-11 6.2e-14
    all-node form (32x16)    3.5e-12  1.04e-11 1.39e-10 2.2e-13  4.0e-13  2.1e-14
    dense Hessian 12x9 band  asymmetry 3.18e-13, against the reference's matrix 5.71e-13 (relative to the largest entry)
Asserted: the project's classes TOL_D1 / TOL_D2 / TOL_S = 1.2e-11 / 1.4e-11 / 1.5e-11, TOL_G / TOL_HV / TOL_ID = 5.4e-12 /
1.1e-11 / 6.1e-13 wherever a case keeps them.  The entries that miss take 10 x their measured deviation, capped at SOLVE =
1e-9 (OVER below): all five field and scalar classes of 50x36, the stiffest solves on the path without the right-scaled
form; grad and hv of the forced GEMM-DCT run; the dense Hessian's two figures (3.2e-12, 5.8e-12); and the scalars of the
all-node form, where c_state = -1.8e-11 is what is left of cancelling integrals (its 1.39e-10 is 2.5e-21 absolute; 10 x
would pass SOLVE, so SOLVE it is).  Nothing is taken from the engine's own output.

Mutants (scratch builds, each fails the named tests):
    1. fix_phi_star returning phi1 + s at every node (the scheme as it was): dphi 3.6e-5 .. 1.4e-4, grad 6.3e-5 .. 4.6e-4,
       dense Hessian 2.9e-3 -- fails test_second_order_outside_the_band and test_hessvec_outside_the_band on all three grids,
       test_gemm_dct_variant_of_the_fft_grid and test_dense_hessian_about_a_band_state.
    2. TanFix dividing by the classified sum (sums[1]) with TanFix::unrecoverable returning false: passes every qualified case
       (the classified weight IS the recorded one there) and fails
       test_unrecoverable_interior_set_is_refused_and_the_context_lives_on (no error on the ambiguous input).
    3. k_hv_rhs taking the mean off the classified interior nodes only instead of (wts / wq) x mean off every node (the
       untransposed form): fails test_hessvec_outside_the_band on all three grids, the GEMM-DCT variant, the dense Hessian
       (asymmetry 0.66) and test_all_node_form_of_the_fix."""
import numpy as np
import pytest

from oracle import vch2d_oracle as o
import _fix_band as fb
from _adjoint_ref import adjoint_reference
from _tangent_ref import KEYS, march_with_fix, tangent_reference, tangent_scalars
from test_gpu_forms import _env
from test_gpu_hessvec_2d import DENSE_REF, DENSE_SYM, EPS, TOL_G, TOL_HV, TOL_ID, _check_stats, _ident, _rel
from test_gpu_second_order import TOL_D1, TOL_D2, TOL_S

pytestmark = pytest.mark.gpu

MARCH, SOLVE, RTOL = 1e-8, 1e-9, 1e-12
GRIDS = ("32x16", "128x32", "50x36")
FFT = {"32x16": True, "128x32": True, "50x36": False}
assert max(TOL_D1, TOL_D2, TOL_S, TOL_G, TOL_HV, TOL_ID) <= SOLVE
# The project's classes, and per case the entries that miss them: 10 x the measured deviation from the CPU reference (module
# docstring), never above SOLVE -- the rule of test_gpu_second_order_matrix.py.
CLASSES = dict(d1=TOL_D1, d2=TOL_D2, s=TOL_S, g=TOL_G, hv=TOL_HV, id=TOL_ID)
OVER = {
    "50x36": dict(d1=1.4e-10, d2=4.1e-10, s=4.8e-10, g=1.5e-10, hv=2.1e-10),
    "32x16 gemm": dict(g=8.3e-11, hv=1.7e-10),
    "fallback": dict(s=SOLVE),
}
DENSE_SYM_BAND, DENSE_REF_BAND = 3.2e-12, 5.8e-12
assert DENSE_SYM < DENSE_SYM_BAND <= SOLVE and DENSE_REF < DENSE_REF_BAND <= SOLVE


def _tol(case):
    t = dict(CLASSES)
    t.update(OVER.get(case, {}))
    assert all(CLASSES[k] <= v <= SOLVE for k, v in t.items())
    return t


def _assert_within(worst, case):
    t = _tol(case)
    for k, v in worst.items():
        assert v < t[k], (case, k, v, t[k])


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


def _engine(V, P, batch, max_steps=4):
    return V.Engine2D(P.Nx, P.Ny, P.Lx, P.Ly, P.tau, P.gamma, P.c1, P.c2, P.kappa, batch=batch, max_steps=max_steps)


_PROBLEMS = {}


def _problem(name):
    """The mixed batch of a grid and the oracle's marches of its trajectories (computed once)."""
    if name in _PROBLEMS:
        return _PROBLEMS[name]
    band = fb.build(name)
    P = band["P"]
    t, dts = o.time_grid(P.T, P.dt_initial)
    phi0 = np.stack([band["phi0"], o.init_phi_random(P.Nx, P.Ny, o.DELTA_SEP, amp=0.1, seed=43), band["phi0"]])
    U = np.stack([band["u"], -0.6 * band["u"], band["u"]])
    H = np.stack([band["dirs"]["noise"], band["dirs"]["smooth"], np.zeros_like(band["u"])])
    phi1, _, _, s1, fix1 = march_with_fix(P, control=U[1], phi0=phi0[1])
    # trajectory 1: every node inside the band before and after the fix, and the fix at work
    assert fix1["masks"].all() and np.abs(fix1["phi_c"]).max() < fb.THR - 10.0 * np.abs(s1).max() and np.abs(s1).min() > 1e-7
    assert fb.is_qualified(fb.qualify(band))
    pr = dict(name=name, P=P, t=t, dts=dts, M=len(dts), x=band["x"], y=band["y"], phi0=phi0, U=U, H=H,
              oracle_phi=[band["phi"], phi1, band["phi"]], masks=[band["masks"], fix1["masks"], band["masks"]])
    _PROBLEMS[name] = pr
    return pr


def _march(V, pr, batch_index=None, env=None):
    """A context with the batch (or one trajectory of it) marched; the engine's history checked against the oracle's."""
    sel = slice(None) if batch_index is None else batch_index
    with _env(**(env or {})):
        eng = _engine(V, pr["P"], 3 if batch_index is None else 1)
    phi, st = eng.forward(pr["phi0"][sel], pr["dts"], u=pr["U"][sel])
    return eng, phi, eng.mass_shifts()


def _run(V, name, env=None):
    pr = dict(_problem(name))
    P = pr["P"]
    eng, phi, shifts = _march(V, pr, env=env)
    for b in range(3):
        dev = np.abs(phi[b] - pr["oracle_phi"][b]).max()
        print(f"MEASURE {name} b={b}: march against the oracle {dev:.2e}")
        assert dev < MARCH
    tg = [o.build_targets(pr["x"], pr["y"], pr["t"], phi[b][0], P.Lx, P.Ly, P.T) for b in range(3)]
    phi_T, phi_Q = np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])
    opt = V.make_opt()
    kw = dict(phi_Q=phi_Q, phi_T=phi_T, x=pr["x"], y=pr["y"])
    pr.update(eng=eng, phi=phi, shifts=shifts, phi_T=phi_T, phi_Q=phi_Q, opt=opt, kw=kw, w=(opt.b1, opt.b2, opt.b3))
    pr["so2"] = eng.second_order(pr["H"], pr["dts"], pr["t"], opt, histories=True, **kw)
    pr["so1"] = eng.second_order(pr["H"], pr["dts"], pr["t"], opt, order=1, histories=True, **kw)
    pr["res"] = eng.hessvec(pr["H"], pr["dts"], pr["t"], opt, **kw)
    pr["tan"] = [tangent_reference(P, phi[b], pr["t"], pr["H"][b], shifts[b], masks=pr["masks"][b]) for b in range(3)]
    pr["adj"] = [adjoint_reference(P, phi[b], pr["t"], shifts[b], pr["U"][b], phi_Q[b], phi_T[b], pr["x"], pr["y"], *pr["w"],
                                   h=pr["H"][b], masks=pr["masks"][b]) for b in range(3)]
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


def _solves_ok(st):
    assert st["unconverged_solves"] == 0, st
    assert st["max_lin_relres"] <= RTOL, st


def _check_second_order(pr):
    name, M = pr["name"], pr["M"]
    so2, so1 = pr["so2"], pr["so1"]
    _solves_ok(so2["stats"])
    _solves_ok(so1["stats"])
    assert pr["eng"].uses_fft == (FFT[name] and not pr.get("forced"))
    assert np.abs(pr["shifts"]).min() > 1e-7                       # the fix is at work on every step of every trajectory
    worst = dict(d1=0.0, d2=0.0, s=0.0)
    for b in (0, 1):
        d1, d2 = pr["tan"][b]
        e1, e2, e1o = _rel(so2["dphi"][b], d1), _rel(so2["d2phi"][b], d2), _rel(so1["dphi"][b], d1)
        print(f"MEASURE {name} b={b}: dphi {e1:.2e} (order 1: {e1o:.2e}) d2phi {e2:.2e}")
        worst["d1"], worst["d2"] = max(worst["d1"], e1, e1o), max(worst["d2"], e2)
        S = tangent_scalars(pr["phi"][b], d1, d2, pr["U"][b], pr["H"][b], pr["phi_Q"][b], pr["phi_T"][b], pr["x"], pr["y"],
                            pr["t"], *pr["w"])
        for k in KEYS + ("slope", "curvature"):
            dev = abs(float(so2[k][b]) / S[k] - 1.0)
            print(f"MEASURE {name} b={b} {k}: engine {float(so2[k][b]):.12e} reference {S[k]:.12e} rel.dev {dev:.2e}")
            worst["s"] = max(worst["s"], dev)
            if k not in ("c_state", "curvature"):
                dev1 = abs(float(so1[k][b]) / S[k] - 1.0)
                worst["s"] = max(worst["s"], dev1)
        assert np.isnan(so1["c_state"][b])
    print(f"MEASURE {name}: second_order worst dphi {worst['d1']:.2e} d2phi {worst['d2']:.2e} scalars {worst['s']:.2e}")
    # h == 0 about a band trajectory: exact zeros
    assert not so2["dphi"][2].any() and not so2["d2phi"][2].any()
    for k in KEYS:
        assert so2[k][2] == 0.0, k
    return worst


def _check_hessvec(pr):
    name, eng, res, so, H, M = pr["name"], pr["eng"], pr["res"], pr["so2"], pr["H"], pr["M"]
    _check_stats(res["stats"], 3, M, 2, RTOL)
    worst = dict(g=0.0, hv=0.0, id=0.0)
    for b in range(3):
        G, Hh = pr["adj"][b]
        eg = _rel(res["grad"][b], G)
        worst["g"] = max(worst["g"], eg)
        print(f"MEASURE {name} b={b}: grad {eg:.2e}")
        if b < 2:
            eh = _rel(res["hv"][b], Hh)
            worst["hv"] = max(worst["hv"], eh)
            print(f"MEASURE {name} b={b}: hv {eh:.2e}")
    assert not res["hv"][2].any() and res["dots"][2, 1] == 0.0 and res["dots"][2, 0] == 0.0
    for b in range(2):
        e1 = _ident(res["grad"][b] * H[b], [so["s_state"][b], so["s_ctrl"][b]])
        e2 = _ident(H[b] * res["hv"][b], [so["c_gn"][b], so["c_state"][b], so["c_ctrl"][b]])
        print(f"MEASURE {name} b={b}: identity 1 {e1:.2e} identity 2 {e2:.2e}")
        worst["id"] = max(worst["id"], e1, e2)
    # identity 4: the directions of the two trajectories exchanged, about the same base points
    Hg = H[[1, 0, 2]]
    rg = eng.hessvec(Hg, pr["dts"], pr["t"], pr["opt"], **pr["kw"])
    _check_stats(rg["stats"], 3, M, 2, RTOL)
    assert np.array_equal(rg["grad"], res["grad"])
    for b in range(2):
        a, c = Hg[b] * res["hv"][b], H[b] * rg["hv"][b]
        e4 = abs(float(a.sum()) - float(c.sum())) / (float(np.abs(a).sum()) + float(np.abs(c).sum()))
        print(f"MEASURE {name} b={b}: identity 4 {e4:.2e}")
        worst["id"] = max(worst["id"], e4)
    n = H[0].size
    for b in range(3):
        t0, t1 = res["grad"][b] * H[b], H[b] * res["hv"][b]
        assert abs(res["dots"][b, 0] - t0.sum()) <= n * EPS * np.abs(t0).sum()
        assert abs(res["dots"][b, 1] - t1.sum()) <= n * EPS * np.abs(t1).sum()
    print(f"MEASURE {name}: hessvec worst grad {worst['g']:.2e} hv {worst['hv']:.2e} identities {worst['id']:.2e}; "
          f"max_lin_relres {res['stats']['max_lin_relres']:.2e}")
    return worst


@pytest.mark.parametrize("name", GRIDS)
def test_second_order_outside_the_band(runs, name):
    _assert_within(_check_second_order(runs(name)), name)


@pytest.mark.parametrize("name", GRIDS)
def test_hessvec_outside_the_band(runs, name):
    _assert_within(_check_hessvec(runs(name)), name)
    g = runs(name)["eng"].exact_gradient(runs(name)["dts"], runs(name)["t"], runs(name)["opt"], **runs(name)["kw"])
    assert np.array_equal(g, runs(name)["res"]["grad"])


@pytest.mark.parametrize("name", GRIDS)
def test_band_trajectory_is_bit_for_bit_its_own_single_run(V, runs, name):
    pr = runs(name)
    for b in (0, 1):
        eng, phi, shifts = _march(V, pr, batch_index=b)
        assert np.array_equal(phi, pr["phi"][b]) and np.array_equal(shifts[0], pr["shifts"][b])
        kw = dict(phi_Q=pr["phi_Q"][b], phi_T=pr["phi_T"][b], x=pr["x"], y=pr["y"])
        so = eng.second_order(pr["H"][b], pr["dts"], pr["t"], pr["opt"], histories=True, **kw)
        r = eng.hessvec(pr["H"][b], pr["dts"], pr["t"], pr["opt"], **kw)
        eng.close()
        _solves_ok(so["stats"])
        _check_stats(r["stats"], 1, pr["M"], 2, RTOL)
        for k in KEYS:
            assert np.array_equal(so[k][0], pr["so2"][k][b]), (k, b)
        assert np.array_equal(so["dphi"][0], pr["so2"]["dphi"][b]) and np.array_equal(so["d2phi"][0], pr["so2"]["d2phi"][b])
        for k in ("grad", "hv", "dots"):
            assert np.array_equal(r[k][0], pr["res"][k][b]), (k, b)


def test_gemm_dct_variant_of_the_fft_grid(V, runs):
    pr = _run(V, "32x16", env=dict(VCH_FORCE_GEMM_DCT=1))
    pr["forced"] = True
    try:
        assert runs("32x16")["eng"].uses_fft and not pr["eng"].uses_fft
        w = _check_second_order(pr)
        v = _check_hessvec(pr)
        print(f"MEASURE 32x16 through the GEMM-DCT: {w} {v}")
        _assert_within(w, "32x16 gemm")
        _assert_within(v, "32x16 gemm")
    finally:
        pr["eng"].close()


def test_dense_hessian_about_a_band_state(V):
    """12 x 9, M = 2: the 390 x 390 Hessian from 13 calls of batch 30 is symmetric and the reference's matrix."""
    m = fb.build("12x9")
    P, u, t = m["P"], m["u"], m["t"]
    dts = np.diff(t)
    nd, nb = u.size, 30
    assert nd == 390 and fb.is_qualified(fb.qualify(m))
    eng = _engine(V, P, nb, max_steps=2)
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (nb,) + a.shape))
    phi, _ = eng.forward(tile(m["phi0"]), dts, u=tile(u))
    shifts = eng.mass_shifts()
    assert np.abs(phi[0] - m["phi"]).max() < MARCH
    phi_T, phi_Q = o.build_targets(m["x"], m["y"], t, phi[0][0], P.Lx, P.Ly, P.T)
    mo = V.make_opt()
    Hd = np.empty((nd, nd))
    for k0 in range(0, nd, nb):
        E = np.zeros((nb, nd))
        E[np.arange(nb), k0 + np.arange(nb)] = 1.0
        r = eng.hessvec(E.reshape((nb,) + u.shape), dts, t, mo, phi_Q=tile(phi_Q), phi_T=tile(phi_T), x=m["x"], y=m["y"])
        _check_stats(r["stats"], nb, 2, 2, RTOL)
        Hd[:, k0:k0 + nb] = r["hv"].reshape(nb, nd).T
    eng.close()
    cache, Hr = {}, np.empty((nd, nd))
    for j in range(nd):
        e = np.zeros(nd)
        e[j] = 1.0
        Hr[:, j] = adjoint_reference(P, phi[0], t, shifts[0], u, phi_Q, phi_T, m["x"], m["y"], mo.b1, mo.b2, mo.b3,
                                     h=e.reshape(u.shape), cache=cache, masks=m["masks"])[1].ravel()
    top = np.abs(Hr).max()
    sym, dev = np.abs(Hd - Hd.T).max() / top, np.abs(Hd - Hr).max() / top
    print(f"MEASURE dense 12x9 band: asymmetry {sym:.2e} (reference's own {np.abs(Hr - Hr.T).max() / top:.2e}) "
          f"against the reference {dev:.2e}")
    assert sym < DENSE_SYM_BAND
    assert dev < DENSE_REF_BAND


def test_all_node_form_of_the_fix(V):
    """fb.FALLBACK: the march's fix ran in the all-node form at every step (no interior node; the record's weight is 0)."""
    m = fb.build(fb.FALLBACK)
    P, t = m["P"], m["t"]
    dts = np.diff(t)
    assert not m["fix"]["interior"].any()
    eng = _engine(V, P, 1)
    phi, _ = eng.forward(m["phi0"], dts, u=m["u"])
    shifts = eng.mass_shifts()[0]
    assert np.abs(phi - m["phi"]).max() < MARCH
    assert np.abs(shifts).min() > 1e-7 and np.abs(shifts / m["shifts"] - 1.0).max() < 1e-3
    phi_T, phi_Q = o.build_targets(m["x"], m["y"], t, phi[0], P.Lx, P.Ly, P.T)
    opt = V.make_opt()
    kw = dict(phi_Q=phi_Q, phi_T=phi_T, x=m["x"], y=m["y"])
    w = (opt.b1, opt.b2, opt.b3)
    worst = {}
    for dirname, h in m["dirs"].items():
        so = eng.second_order(h, dts, t, opt, histories=True, **kw)
        res = eng.hessvec(h, dts, t, opt, **kw)
        _solves_ok(so["stats"])
        _check_stats(res["stats"], 1, len(dts), 2, RTOL)
        d1, d2 = tangent_reference(P, phi, t, h, shifts, masks=m["masks"])
        G, Hh = adjoint_reference(P, phi, t, shifts, m["u"], phi_Q, phi_T, m["x"], m["y"], *w, h=h, masks=m["masks"])
        S = tangent_scalars(phi, d1, d2, m["u"], h, phi_Q, phi_T, m["x"], m["y"], t, *w)
        e = dict(d1=_rel(so["dphi"][0], d1), d2=_rel(so["d2phi"][0], d2), g=_rel(res["grad"][0], G), hv=_rel(res["hv"][0], Hh),
                 s=max(abs(float(so[k][0]) / S[k] - 1.0) for k in KEYS),
                 id=max(_ident(res["grad"][0] * h, [so["s_state"][0], so["s_ctrl"][0]]),
                        _ident(h * res["hv"][0], [so["c_gn"][0], so["c_state"][0], so["c_ctrl"][0]])))
        print(f"MEASURE fallback {dirname}: {e}; scalars "
              + ", ".join(f"{k} {abs(float(so[k][0]) / S[k] - 1.0):.2e} ({S[k]:.3e})" for k in KEYS))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in e.items()}
    eng.close()
    _assert_within(worst, "fallback")


def test_unrecoverable_interior_set_is_refused_and_the_context_lives_on(V):
    """The ambiguous input: at step 1 five skipped nodes pass |phi_{n+1} + s_n| < THR (step 0 has none), 1.2e-5 inside the
    threshold, so the engine sees them as the CPU does.  second_order and hessvec (both orders) return the error naming
    trajectory and step; a batch of two qualified trajectories on the same context is then answered bit for bit like on a
    fresh one -- so a qualified input with its non-round-off shifts is not refused -- and the memory balances after close."""
    amb, good = fb.build(fb.AMBIGUOUS), fb.build("32x16")
    P, t = good["P"], good["t"]
    dts = np.diff(t)
    # the CPU's prediction: the first step whose re-derived set is larger than the march's own
    extra = [int(np.sum((np.abs(amb["phi"][k + 1] + s) < fb.THR) & ~amb["masks"][k])) for k, s in enumerate(amb["shifts"])]
    step = next(k for k, n in enumerate(extra) if n)
    # every decision up to the predicted step, the march's (on phi_c) and the sweeps' (on phi_{n+1} + s_n), stands 100 x MARCH
    # off the threshold: the engine's W_int and classified sets of steps 0 .. step are the oracle's
    margin = min(min(np.abs(np.abs(amb["fix"]["phi_c"][k]) - fb.THR).min(),
                     np.abs(np.abs(amb["phi"][k + 1] + amb["shifts"][k]) - fb.THR).min()) for k in range(step + 1))
    print(f"MEASURE refusal: extra nodes per step {extra}, predicted step {step}, decision margin {margin:.2e}")
    assert step == 1 and extra[0] == 0 and margin > 100 * MARCH
    lib = V.module("_lib").load()
    live0 = lib.vch_mem_live()
    H = np.stack([good["dirs"]["noise"], good["dirs"]["smooth"]])
    kw = dict(x=good["x"], y=good["y"])
    opt = V.make_opt()

    def answers(eng):
        phi, _ = eng.forward(np.stack([good["phi0"], good["phi0"]]), dts, u=np.stack([good["u"], -good["u"]]))
        so = eng.second_order(H, dts, t, opt, histories=True, **kw)
        res = eng.hessvec(H, dts, t, opt, **kw)
        _solves_ok(so["stats"])
        _check_stats(res["stats"], 2, len(dts), 2, RTOL)
        return [phi, so["dphi"], so["d2phi"], res["grad"], res["hv"], res["dots"]] + [so[k] for k in KEYS]

    fresh = _engine(V, P, 2)
    want = answers(fresh)
    fresh.close()
    eng = _engine(V, P, 2)
    phi, _ = eng.forward(np.stack([good["phi0"], amb["phi0"]]), dts, u=np.stack([good["u"], amb["u"]]))
    assert np.abs(phi[1] - amb["phi"]).max() < MARCH and np.abs(phi[0] - good["phi"]).max() < MARCH
    msg = f"trajectory 1, step {step}: interior set of the mass fix not recoverable"
    with pytest.raises(V.VchError, match=msg):
        eng.second_order(H, dts, t, opt, **kw)
    with pytest.raises(V.VchError, match=msg):
        eng.second_order(H, dts, t, opt, order=1, **kw)
    with pytest.raises(V.VchError, match=msg):
        eng.hessvec(H, dts, t, opt, **kw)
    with pytest.raises(V.VchError, match=msg):
        eng.exact_gradient(dts, t, opt, **kw)
    got = answers(eng)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    eng.close()
    assert lib.vch_mem_live() == live0
