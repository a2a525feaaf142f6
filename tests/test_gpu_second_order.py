"""vch2d_second_order on the GPU: the tangent marches and the six scalars of J'(u)h and J''(u)[h,h] against CPU linear
algebra (tests/_tangent_ref.py: the oracle's assembled Newton matrix and a sparse direct solve, pinned against central
differences of the nonlinear march by test_tangent_cpu.py).  The engine marches, its state history and the shifts of its
mass fix (mass_shifts()) are pulled and fed to the CPU reference, so the engine's linear solves are compared with direct
ones on the same history, not with themselves.

Cases: 16 x 16 with 5 steps and a ragged last one (T = 0.045, dt = 0.01; stencil-free FFT path), 14 x 11 (GEMM-DCT path;
the rectangular grid exercises the Laplacian's Kronecker-order quirk), 32 x 16 (rectangular FFT, a direction of 3 rows
< M + 1).  Batch 3 each: a white-noise direction, a smooth one, h == 0; the controls differ per trajectory.

Tolerances of engine vs reference: the largest relative deviation at the default rtol = 1e-12 over everything this file
compares with the reference (the three cases, the per-trajectory weights, the PGD iterate), max-norm for the fields, per
scalar for the six scalars and their two sums:
    measured   dphi 1.11e-12   d2phi 1.40e-12   scalars 1.41e-12
               (per case, dphi / d2phi / scalars: 16 x 16 5.0e-13 / 9.9e-13 / 1.4e-12, 14 x 11 5.3e-13 / 8.4e-13 / 7.1e-13,
                32 x 16 6.3e-13 / 1.4e-12 / 7.0e-13, PGD iterate 1.1e-12 / 7.5e-13 / 9.5e-13; the solves' own worst final
                relative residual 7.7e-13)
    asserted   1.2e-11, 1.4e-11, 1.5e-11: 10 x measured (the factor covers a CG that stops on a relative residual and the
               round-off of the DCT), five to seven orders below the CPU floors 1e-5 (dphi, scalars) and 3e-4 (d2phi) of
               test_tangent_cpu.py, which nothing here may exceed."""
import math

import numpy as np
import pytest

from oracle import vch2d_oracle as o
from _tangent_ref import KEYS, tangent_reference, tangent_scalars

pytestmark = pytest.mark.gpu

TOL_D1, TOL_D2, TOL_S = 1.2e-11, 1.4e-11, 1.5e-11
assert TOL_D1 <= 1e-5 and TOL_D2 <= 3e-4 and TOL_S <= 1e-5

CASES = {
    #           Nx  Ny  T      dt    rows of h (None: M + 1)   uses_fft
    "fft16":    (16, 16, 0.045, 0.01, None, True),
    "gemm14x11": (14, 11, 0.04, 0.01, None, False),
    "fft32x16": (32, 16, 0.04, 0.01, 3, True),
}
WEIGHTS = [(5.0, 10.0, 1e-4), (1.5, 0.0, 3e-2), (0.0, 7.0, 1.0)]


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


def _engine(V, P, batch, max_steps=8):
    return V.Engine2D(P.Nx, P.Ny, P.Lx, P.Ly, P.tau, P.gamma, P.c1, P.c2, P.kappa, batch=batch, max_steps=max_steps)


def _problem(name):
    Nx, Ny, T, dt, rows, fft = CASES[name]
    P = o.Params2D(Nx=Nx, Ny=Ny, T=T, dt_initial=dt)
    t, dts = o.time_grid(T, dt)
    M = len(dts)
    x, y = np.linspace(0.0, P.Lx, Nx + 1), np.linspace(0.0, P.Ly, Ny + 1)
    xx, yy = np.meshgrid(x, y, indexing="ij")
    ctrl = lambda amp, s: amp * np.stack([np.cos(np.pi * xx * (1 + (k + s) % 3)) * np.cos(np.pi * yy) * np.sin(1 + k + s)
                                          for k in range(M + 1)])
    U = np.stack([ctrl(20.0, 0), ctrl(-12.0, 1), ctrl(8.0, 2)])
    rows = M + 1 if rows is None else rows
    noise = np.random.default_rng(3).standard_normal((rows, Nx + 1, Ny + 1))
    smooth = np.stack([np.cos(2 * np.pi * xx) * np.cos(np.pi * yy) * np.cos(0.3 * k) for k in range(rows)])
    H = np.stack([noise / np.abs(noise).max(), smooth, np.zeros_like(smooth)])
    phi0 = np.stack([o.init_phi_random(Nx, Ny, o.DELTA_SEP, amp=0.1, seed=42 + b) for b in range(3)])
    return dict(P=P, t=t, dts=dts, M=M, x=x, y=y, U=U, H=H, phi0=phi0, fft=fft)


@pytest.fixture(scope="module")
def runs(V):
    """Per case: the batch-3 march, the engine's answer with histories, and the CPU reference on the engine's own history
    (computed once, shared, never modified)."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        pr = _problem(name)
        P = pr["P"]
        eng = _engine(V, P, 3)
        assert eng.uses_fft == pr["fft"]
        phi, _ = eng.forward(pr["phi0"], pr["dts"], u=pr["U"])
        shifts = eng.mass_shifts()              # what the march's mass fix subtracted: the reference linearises it
        tg = [o.build_targets(pr["x"], pr["y"], pr["t"], phi[b][0], P.Lx, P.Ly, P.T) for b in range(3)]
        phi_T, phi_Q = np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])
        opt = V.make_opt()
        res = eng.second_order(pr["H"], pr["dts"], pr["t"], opt, phi_Q=phi_Q, phi_T=phi_T, histories=True)
        ref = []
        for b in range(3):
            d1, d2 = tangent_reference(P, phi[b], pr["t"], pr["H"][b], shifts[b])
            ref.append((d1, d2))
        pr.update(eng=eng, phi=phi, shifts=shifts, phi_T=phi_T, phi_Q=phi_Q, res=res, ref=ref, opt=opt)
        cache[name] = pr
        return pr

    yield get
    for pr in cache.values():
        pr["eng"].close()


def _ref_scalars(pr, b, w):
    d1, d2 = pr["ref"][b]
    return tangent_scalars(pr["phi"][b], d1, d2, pr["U"][b], pr["H"][b], pr["phi_Q"][b], pr["phi_T"][b], pr["x"], pr["y"],
                           pr["t"], *w)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", list(CASES))
def test_fields_and_scalars_against_cpu_linear_algebra(runs, name):
    pr = runs(name)
    res = pr["res"]
    assert np.abs(pr["phi"]).max() < 1.0 - o.DELTA_SEP - 0.1          # the clip the tangent scheme ignores is inactive
    if pr["P"].Nx != pr["P"].Ny:
        assert np.abs(pr["shifts"][:2]).min() > 1e-7                  # rectangular grid: the mass fix shifts every step
    worst = dict(d1=0.0, d2=0.0, s=0.0)
    for b in (0, 1):
        d1, d2 = pr["ref"][b]
        worst["d1"] = max(worst["d1"], _rel(res["dphi"][b], d1))
        worst["d2"] = max(worst["d2"], _rel(res["d2phi"][b], d2))
        S = _ref_scalars(pr, b, (pr["opt"].b1, pr["opt"].b2, pr["opt"].b3))
        for k in KEYS + ("slope", "curvature"):
            dev = abs(float(res[k][b]) / S[k] - 1.0)
            print(f"{name} b={b} {k}: engine {float(res[k][b]):.12e} reference {S[k]:.12e} rel.dev {dev:.2e}")
            worst["s"] = max(worst["s"], dev)
        assert res["n_h"][b] > 0 and res["c_gn"][b] > 0
    print(f"{name}: largest relative deviation dphi {worst['d1']:.2e} d2phi {worst['d2']:.2e} scalars {worst['s']:.2e}; "
          f"stats {res['stats']}")
    assert worst["d1"] < TOL_D1
    assert worst["d2"] < TOL_D2
    assert worst["s"] < TOL_S
    # h == 0: exact zeros, whatever the control and the state
    assert not res["dphi"][2].any() and not res["d2phi"][2].any()
    for k in KEYS + ("slope", "curvature"):
        assert res[k][2] == 0.0, k
    # level 0 of every tangent field is zero
    assert not res["dphi"][:, 0].any() and not res["d2phi"][:, 0].any()


@pytest.mark.parametrize("name", list(CASES))
def test_order_one_is_the_first_march_of_order_two(runs, name):
    pr = runs(name)
    r1 = pr["eng"].second_order(pr["H"], pr["dts"], pr["t"], pr["opt"], phi_Q=pr["phi_Q"], phi_T=pr["phi_T"], order=1,
                                histories=True)
    for k in ("s_state", "s_ctrl", "c_gn", "c_ctrl", "n_h", "slope"):
        assert np.array_equal(r1[k], pr["res"][k]), k
    assert np.isnan(r1["c_state"]).all() and np.isnan(r1["curvature"]).all()
    assert np.array_equal(r1["dphi"], pr["res"]["dphi"]) and not r1["d2phi"].any()
    assert r1["stats"]["linear_solves"] * 2 == pr["res"]["stats"]["linear_solves"] == 2 * 3 * pr["M"]


@pytest.mark.parametrize("name", list(CASES))
def test_batch_of_three_equals_three_single_contexts(V, runs, name):
    pr = runs(name)
    for b in range(3):
        eng = _engine(V, pr["P"], 1)
        phi, _ = eng.forward(pr["phi0"][b], pr["dts"], u=pr["U"][b])
        assert np.array_equal(phi, pr["phi"][b])
        r = eng.second_order(pr["H"][b], pr["dts"], pr["t"], pr["opt"], phi_Q=pr["phi_Q"][b], phi_T=pr["phi_T"][b],
                             histories=True)
        eng.close()
        for k in KEYS:
            assert r[k][0] == pr["res"][k][b], (k, b)
        assert np.array_equal(r["dphi"][0], pr["res"]["dphi"][b]) and np.array_equal(r["d2phi"][0], pr["res"]["d2phi"][b])


def test_per_trajectory_weights_against_the_scalar_form(V, runs):
    pr = runs("gemm14x11")
    eng = pr["eng"]
    opts = [V.make_opt(b1=w[0], b2=w[1], b3=w[2]) for w in WEIGHTS]
    many = eng.second_order(pr["H"], pr["dts"], pr["t"], opts, phi_Q=pr["phi_Q"], phi_T=pr["phi_T"])
    for b, w in enumerate(WEIGHTS):
        one = eng.second_order(pr["H"], pr["dts"], pr["t"], opts[b], phi_Q=pr["phi_Q"], phi_T=pr["phi_T"])
        for k in KEYS:
            assert many[k][b] == one[k][b], (k, b)
        if b < 2:
            S = _ref_scalars(pr, b, w)
            for k in KEYS:
                if S[k] != 0.0:
                    dev = abs(float(many[k][b]) / S[k] - 1.0)
                    print(f"weights {w} b={b} {k}: rel.dev {dev:.2e}")
                    assert dev < TOL_S, (k, b)
                else:
                    assert many[k][b] == 0.0, (k, b)
    assert many["n_h"][0] == pr["res"]["n_h"][0]


def test_pgd_iterate_is_not_disturbed_and_the_iterate_is_the_base_point(V):
    """After pgd_init + 2 iterations the call works about the current iterate (pgd_get('u' / 'phi')) with the problem's grid
    and targets, and a further iteration returns the bits of a run that never made the call."""
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
    res = eng.second_order(H, opt=opts, histories=True)
    shifts = eng.mass_shifts()
    assert np.array_equal(eng.pgd_get("u"), u) and np.array_equal(eng.pgd_get("phi"), phi)
    assert np.abs(u).max() > 0
    for b in range(2):
        d1, d2 = tangent_reference(P, phi[b], t, H[b], shifts[b])
        e1, e2 = _rel(res["dphi"][b], d1), _rel(res["d2phi"][b], d2)
        S = tangent_scalars(phi[b], d1, d2, u[b], H[b], phi_Q[b], phi_T[b], x, x, t, opts[b].b1, opts[b].b2, opts[b].b3)
        devs = {k: abs(float(res[k][b]) / S[k] - 1.0) for k in KEYS + ("slope", "curvature")}
        print(f"pgd b={b}: dphi {e1:.2e} d2phi {e2:.2e} scalars " + " ".join(f"{k} {v:.2e}" for k, v in devs.items()))
        assert e1 < TOL_D1 and e2 < TOL_D2
        assert max(devs.values()) < TOL_S, devs
    got = eng.pgd_iterate(1)
    for k in ("cost", "alpha", "attempts", "change", "tracking_error", "terminal_error"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(eng.pgd_get("u"), u_want)
    with pytest.raises(ValueError):          # the resident problem has its own targets
        eng.second_order(H, opt=opts, phi_T=phi_T)
    eng.close()


def test_error_codes_come_before_any_launch(V, runs):
    pr = runs("fft16")
    fresh = _engine(V, pr["P"], 3)
    c0 = fresh.counters()
    with pytest.raises(V.VchError, match="-3"):
        fresh.second_order(pr["H"], pr["dts"], pr["t"], pr["opt"])
    assert fresh.counters() == c0
    fresh.close()
    eng, H, dts, t, opt = pr["eng"], pr["H"], pr["dts"], pr["t"], pr["opt"]
    c0 = eng.counters()
    bad = [
        dict(h=H, dt=dts[:-1], t_hist=t[:-1], opt=opt),                                   # M != M_res
        dict(h=H, dt=dts, t_hist=t, opt=[opt, opt]),                                      # n_opts neither 1 nor B
        dict(h=H, dt=dts, t_hist=t, opt=opt, order=3),
        dict(h=H, dt=dts, t_hist=t, opt=opt, order=0),
        dict(h=np.zeros((3, eng.max_steps + 2) + eng.shape), dt=dts, t_hist=t, opt=opt),   # h_rows > max_steps + 1
        dict(h=H, dt=dts, t_hist=t, opt=V.make_opt(b1=math.nan)),
        dict(h=H, dt=dts, t_hist=t, opt=[opt, opt, V.make_opt(b3=math.inf)]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.second_order(**kw)
        assert eng.counters() == c0, kw.keys()
    # ... and the context still answers, with the bits of the first call
    again = eng.second_order(H, dts, t, opt, phi_Q=pr["phi_Q"], phi_T=pr["phi_T"])
    for k in KEYS:
        assert np.array_equal(again[k], pr["res"][k], equal_nan=True), k
    launches, looks = eng.counters()
    assert launches - c0[0] == again["stats"]["launches"] and looks - c0[1] == again["stats"]["host_syncs"]


def test_driver_level_exact_condition(V, capsys):
    """exact_second_order_condition_2d: the curvature of Engine2D.second_order for the finite-difference function's own
    seeded draws, and the finite-difference function's output for that seed is what it was before."""
    S2 = V.module("Vch_control_2D.second_order_conditions_2d")
    K2 = V.module("Vch_control_2D.config")
    F2 = V.module("Vch_control_2D.Forward2_solver")
    N, T, dt = 16, 0.05, 0.01
    cfg = K2.ForwardSolverConfig(Nx=N, Ny=N, T=T, dt_initial=dt)
    opt = K2.OptimizationConfig()
    t, dts = V.time_grid(T, dt)
    assert len(dts) == 5
    x = np.linspace(0.0, 1.0, N + 1)
    xx, yy = np.meshgrid(x, x, indexing="ij")
    u_star = np.clip(np.stack([1.4 * np.cos(np.pi * xx * (1 + k % 3)) * np.cos(np.pi * yy) * np.sin(1 + k) for k in range(6)]),
                     opt.u_min, opt.u_max)
    r_star = 1e-3 * np.stack([np.sin(np.pi * xx) * np.cos(2 * np.pi * yy) * (1 + k) for k in range(6)])
    phi_star, _, _ = F2.run_main_simulation(cfg, store_history=True, control_input=u_star, verbose=False)
    phi_T, phi_Q = o.build_targets(x, x, t, phi_star[0], 1.0, 1.0, T)
    kw = dict(u_star=u_star, r_star=r_star, phi_star=phi_star, x=x, y=x, t_hist=t, opt_config=opt, phi_Q_target=phi_Q,
              phi_T_target=phi_T, u_min=opt.u_min, u_max=opt.u_max, num_directions=3, seed=7, fwd_config=cfg)
    before = S2.approximate_second_order_condition_2d(**kw)
    exact = S2.exact_second_order_condition_2d(**kw)
    printed = capsys.readouterr().out
    after = S2.approximate_second_order_condition_2d(**kw)
    assert before == after and len(before) == 3
    assert len(exact) == 3 and all(math.isfinite(v) for v in exact)
    assert printed.count("exact slope") == 3 and printed.count("adjoint sum(g·h)") == 3
    rng = np.random.default_rng(7)
    dirs = np.stack([S2._generate_direction(u_star, r_star, opt.u_min, opt.u_max, rng) for _ in range(3)])
    assert (np.abs(u_star) >= opt.u_max - 1e-8).any()            # some nodes sit on the box: the cone is not the whole space
    eng = V.Engine2D(N, N, cfg.Lx, cfg.Ly, cfg.tau, cfg.gamma, cfg.c1, cfg.c2, cfg.kappa, batch=3, max_steps=5)
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (3,) + a.shape))
    eng.forward(tile(F2.init_phi_random(N, N, 1e-2, amp=0.1, seed=42)), dts, u=tile(u_star), store=False)
    res = eng.second_order(dirs, dts, t, V.make_opt(opt), phi_Q=tile(phi_Q), phi_T=tile(phi_T), x=x, y=x)
    eng.close()
    assert list(res["curvature"]) == exact
