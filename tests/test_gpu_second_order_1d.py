"""vch1d_second_order on the GPU: the tangent march of one persistent workgroup per direction and the six scalars of
J'(u)h and J''(u)[h,h] against CPU linear algebra (tests/_tangent_ref_1d.py: the oracle's Newton matrix and its
high-precision banded solve, pinned against central differences of the nonlinear march by test_tangent_cpu_1d.py).  The
engine marches, its state history is pulled and fed to the CPU reference, so the engine's cyclic reduction is compared
with a direct solve on the same history, not with itself.

Cases (the smallest shapes at which the kernel can go wrong), batch 3 each: a white-noise direction, a smooth one, h == 0;
the starts 0.2 cos(pi x / Lx + 0.4 b) and the controls (amplitudes 12, -9, 7) differ per trajectory:
    n32      N = 32, defaults, T = 0.05, dt = 0.01 (5 steps): fewer nodes than threads, cyclic-reduction depth 0
    n33_off  N = 33, Lx 1.3, c2 0.5, gamma 3, kappa 1e-3, c1 0.9, tau 0.01, T = 0.045, dt = 0.01: odd N, ragged last step
    n1030    N = 1030, T = 0.03 (3 steps): depth 1
    n2051    N = 2051, T = 0.03 (3 steps): depth 2, odd residue

Tolerances of engine vs reference: the largest relative deviation over everything this file compares with the reference at
that depth, max-norm for the fields, per scalar for the six scalars and their two sums:
                dphi                  d2phi                 scalars
    depth 0     6.18e-16 / 6.2e-15    1.26e-15 / 1.3e-14    9.33e-15 / 9.4e-14    (n32, n33_off, the weights, the PGD iterate)
    depth 1     6.64e-14 / 6.7e-13    2.35e-13 / 2.4e-12    1.22e-12 / 1.3e-11    (n1030)
    depth 2     4.05e-13 / 4.1e-12    3.45e-12 / 3.5e-11    1.34e-11 / 1.4e-10    (n2051)
measured on the MI355X / asserted (10 x measured, rounded up).  The growth with N is the reference's own: its solve variants
differ by 1e-11 at N ~ 1000-2000, and the worst scalar is c_state, a sum that cancels to 1e-3 of its terms.
Every asserted value is orders below the CPU floors 1e-5 (dphi, scalars) and 3e-4 (d2phi) of test_tangent_cpu_1d.py.

Driver level: the curvature of exact_second_order_condition against the central second difference of Engine1D.forward +
Engine1D.cost at eps = 3e-2 is held to DRIVER_TOL = 5.9e-6 of test_tangent_cpu_1d.py, 10 x the 5.82e-7 the same setup shows
on the CPU oracle (measured on the MI355X: 8.95e-7)."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import vch1d_oracle as o
from _tangent_ref_1d import DRIVER, KEYS, driver_problem, tangent_reference_1d, tangent_scalars_1d
from test_tangent_cpu_1d import DRIVER_TOL, FLOOR_D1, FLOOR_D2, FLOOR_S

pytestmark = pytest.mark.gpu

#        depth: dphi, d2phi, scalars
TOL = {0: (6.2e-15, 1.3e-14, 9.4e-14), 1: (6.7e-13, 2.4e-12, 1.3e-11), 2: (4.1e-12, 3.5e-11, 1.4e-10)}
for _t in TOL.values():
    assert _t[0] <= FLOOR_D1 and _t[1] <= FLOOR_D2 and _t[2] <= FLOOR_S

OFF = dict(Lx=1.3, c2=0.5, gamma=3.0, kappa=1e-3, c1=0.9, tau=0.01)
CASES = {
    #          Params1D fields                                     depth
    "n32":     (dict(N=32, T=0.05, dt_initial=0.01), 0),
    "n33_off": (dict(N=33, T=0.045, dt_initial=0.01, **OFF), 0),
    "n1030":   (dict(N=1030, T=0.03, dt_initial=0.01), 1),
    "n2051":   (dict(N=2051, T=0.03, dt_initial=0.01), 2),
}
WEIGHTS = [(5.0, 10.0, 1e-4), (1.5, 0.0, 3e-2), (0.0, 7.0, 1.0)]
ALL = KEYS + ("slope", "curvature")


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


def _engine(V, P, batch, max_steps=8):
    return V.Engine1D(P.N, P.Lx, P.tau, P.gamma, P.c1, P.c2, P.kappa, batch=batch, max_steps=max_steps)


def _problem(V, name):
    kw, depth = CASES[name]
    P = o.Params1D(**kw)
    tg, dts = V.time_grid(P.T, P.dt_initial)
    t = np.concatenate([[0.0], tg])
    rows = len(t)
    x = np.linspace(0.0, P.Lx, P.N + 1)
    xs = x / P.Lx
    ctrl = lambda amp, s: amp * np.stack([np.cos(np.pi * xs * (1 + (k + s) % 3)) * np.sin(1 + k + s) for k in range(rows)])
    U = np.stack([ctrl(12.0, 0), ctrl(-9.0, 1), ctrl(7.0, 2)])
    noise = np.random.default_rng(3).standard_normal((rows, P.N + 1))
    smooth = np.stack([np.cos(2 * np.pi * xs) * np.cos(0.3 * k) for k in range(rows)])
    H = np.stack([noise / np.abs(noise).max(), smooth, np.zeros_like(smooth)])
    phi0 = np.stack([0.2 * np.cos(np.pi * xs + 0.4 * b) for b in range(3)])
    return dict(P=P, t=t, dts=np.asarray(dts), M=len(dts), rows=rows, x=x, U=U, H=H, phi0=phi0, depth=depth)


@pytest.fixture(scope="module")
def runs(V):
    """Per case: the batch-3 march, the engine's answer with histories, and the CPU reference on the engine's own history
    (computed once, shared, never modified)."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        pr = _problem(V, name)
        P = pr["P"]
        eng = _engine(V, P, 3)
        phi, _ = eng.forward(pr["phi0"], pr["dts"], u=pr["U"])
        tg = [o.build_targets(pr["x"], pr["t"], phi[b][0], P.Lx, P.T) for b in range(3)]
        phi_T, phi_Q = np.stack([a for a, _ in tg]), np.stack([q for _, q in tg])
        opt = V.make_opt()
        res = eng.second_order(pr["H"], pr["t"], opt, phi_hist=phi, u=pr["U"], phi_Q=phi_Q, phi_T=phi_T, dt=pr["dts"],
                               histories=True)
        ref = [tangent_reference_1d(P, phi[b], pr["t"], pr["H"][b], dts=pr["dts"]) for b in range(2)]
        pr.update(eng=eng, phi=phi, phi_T=phi_T, phi_Q=phi_Q, res=res, ref=ref, opt=opt)
        cache[name] = pr
        return pr

    yield get
    for pr in cache.values():
        pr["eng"].close()


def _call(pr, eng=None, **kw):
    args = dict(phi_hist=pr["phi"], u=pr["U"], phi_Q=pr["phi_Q"], phi_T=pr["phi_T"], dt=pr["dts"])
    opt = kw.pop("opt", pr["opt"])
    args.update(kw)
    return (eng or pr["eng"]).second_order(pr["H"], pr["t"], opt, **args)


def _ref_scalars(pr, b, w):
    d1, d2 = pr["ref"][b]
    return tangent_scalars_1d(pr["phi"][b], d1, d2, pr["U"][b], pr["H"][b], pr["phi_Q"][b], pr["phi_T"][b], pr["x"], pr["t"], *w)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _same(a, b, keys=KEYS, fields=True):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    if fields:
        assert np.array_equal(a["dphi"], b["dphi"]) and np.array_equal(a["d2phi"], b["d2phi"])


@pytest.mark.parametrize("name", list(CASES))
def test_fields_and_scalars_against_cpu_linear_algebra(runs, name):
    pr = runs(name)
    res = pr["res"]
    assert np.abs(pr["phi"]).max() < 1.0 - o.DELTA_SEP - 0.1          # the clip the tangent scheme ignores is inactive
    worst = dict(d1=0.0, d2=0.0, s=0.0)
    for b in (0, 1):
        d1, d2 = pr["ref"][b]
        worst["d1"] = max(worst["d1"], _rel(res["dphi"][b], d1))
        worst["d2"] = max(worst["d2"], _rel(res["d2phi"][b], d2))
        S = _ref_scalars(pr, b, (pr["opt"].b1, pr["opt"].b2, pr["opt"].b3))
        for k in ALL:
            dev = abs(float(res[k][b]) / S[k] - 1.0)
            print(f"{name} b={b} {k}: engine {float(res[k][b]):.12e} reference {S[k]:.12e} rel.dev {dev:.2e}")
            worst["s"] = max(worst["s"], dev)
        assert res["n_h"][b] > 0 and res["c_gn"][b] > 0
    print(f"{name}: largest relative deviation dphi {worst['d1']:.2e} d2phi {worst['d2']:.2e} scalars {worst['s']:.2e}; "
          f"max|phi| {np.abs(pr['phi']).max():.3f}; stats {res['stats']}")
    t1, t2, ts = TOL[pr["depth"]]
    assert worst["d1"] < t1
    assert worst["d2"] < t2
    assert worst["s"] < ts
    # h == 0: exact zeros, whatever the control and the state
    assert not res["dphi"][2].any() and not res["d2phi"][2].any()
    for k in ALL:
        assert res[k][2] == 0.0, k
    # rows 0 and 1 (t = 0 twice) of every tangent field are zero
    assert not res["dphi"][:, :2].any() and not res["d2phi"][:, :2].any()
    assert res["dphi"][0, 2].any() and res["d2phi"][0, 2].any()
    assert res["stats"]["launches"] == 1 and res["stats"]["seconds"] > 0


@pytest.mark.parametrize("name", list(CASES))
def test_order_one_is_the_first_march_of_order_two(runs, name):
    pr = runs(name)
    r1 = _call(pr, order=1, histories=True)
    _same(r1, pr["res"], keys=("s_state", "s_ctrl", "c_gn", "c_ctrl", "n_h", "slope"), fields=False)
    assert np.isnan(r1["c_state"]).all() and np.isnan(r1["curvature"]).all()
    assert np.array_equal(r1["dphi"], pr["res"]["dphi"]) and not r1["d2phi"].any()
    assert r1["stats"]["linear_solves"] == 3 * pr["M"] and pr["res"]["stats"]["linear_solves"] == 2 * 3 * pr["M"]


@pytest.mark.parametrize("name", list(CASES))
def test_batch_of_three_equals_three_single_contexts(V, runs, name):
    pr = runs(name)
    for b in range(3):
        eng = _engine(V, pr["P"], 1)
        phi, _ = eng.forward(pr["phi0"][b], pr["dts"], u=pr["U"][b])
        assert np.array_equal(phi, pr["phi"][b])
        r = eng.second_order(pr["H"][b], pr["t"], pr["opt"], u=pr["U"][b], phi_Q=pr["phi_Q"][b], phi_T=pr["phi_T"][b],
                             dt=pr["dts"], histories=True)
        eng.close()
        for k in KEYS:
            assert r[k][0] == pr["res"][k][b], (k, b)
        assert np.array_equal(r["dphi"][0], pr["res"]["dphi"][b]) and np.array_equal(r["d2phi"][0], pr["res"]["d2phi"][b])


@pytest.mark.parametrize("name", list(CASES))
def test_shared_base_equals_the_tiled_base(runs, name):
    pr = runs(name)
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (3,) + a.shape))
    base = dict(phi_hist=pr["phi"][1], u=pr["U"][1], phi_Q=pr["phi_Q"][1], phi_T=pr["phi_T"][1])
    one = _call(pr, histories=True, shared_base=True, **base)
    many = _call(pr, histories=True, **{k: tile(v) for k, v in base.items()})
    _same(one, many)
    assert one["s_state"][0] != pr["res"]["s_state"][0]              # another base point than trajectory 0's own
    assert one["s_state"][1] == pr["res"]["s_state"][1]


def test_per_trajectory_weights_against_the_scalar_form(V, runs):
    pr = runs("n33_off")
    opts = [V.make_opt(b1=w[0], b2=w[1], b3=w[2]) for w in WEIGHTS]
    many = _call(pr, opt=opts)
    for b, w in enumerate(WEIGHTS):
        one = _call(pr, opt=opts[b])
        for k in KEYS:
            assert many[k][b] == one[k][b], (k, b)
        if b < 2:
            S = _ref_scalars(pr, b, w)
            for k in KEYS:
                if S[k] != 0.0:
                    dev = abs(float(many[k][b]) / S[k] - 1.0)
                    print(f"weights {w} b={b} {k}: rel.dev {dev:.2e}")
                    assert dev < TOL[0][2], (k, b)
                else:
                    assert many[k][b] == 0.0, (k, b)
    assert many["n_h"][0] == pr["res"]["n_h"][0]


def test_resident_history_after_forward(V, runs):
    pr = runs("n1030")
    eng = _engine(V, pr["P"], 3)
    phi, _ = eng.forward(pr["phi0"], pr["dts"], u=pr["U"])
    assert np.array_equal(phi, pr["phi"])
    res = _call(pr, eng=eng, phi_hist=None, histories=True)
    eng.close()
    _same(res, pr["res"])


def test_resident_pgd_state_and_undisturbed_iterations(V):
    """After pgd_init + 2 iterations: RESIDENT control and targets equal passing pgd_get("u" / "phi" / "phi_Q") and phi_T
    explicitly, and two further iterations are bit for bit those of an uninterrupted 4-iteration run."""
    N, T, dt = 32, 0.05, 0.01
    P = o.Params1D(N=N, T=T, dt_initial=dt)
    tg, dts = V.time_grid(T, dt)
    t = np.concatenate([[0.0], tg])
    x = np.linspace(0.0, 1.0, N + 1)
    phi0 = np.stack([0.2 * np.cos(np.pi * x + 0.4 * b) for b in range(2)])
    phi_T = np.stack([0.7 * np.sin(2 * np.pi * x), 0.5 * np.cos(2 * np.pi * x)])
    opt = V.make_opt(b1=0.3, b2=13.0, b3=0.0019, kappa_sparsity=9e-5, alpha_max=100.0)
    noise = np.random.default_rng(5).standard_normal((2, len(t), N + 1))
    H = noise / np.abs(noise).max()

    def start():
        eng = _engine(V, P, 2)
        eng.pgd_init(phi0, phi_T, t, dts, opt)
        return eng, eng.pgd_iterate(2)

    plain, _ = start()
    want = plain.pgd_iterate(2)
    u_want = plain.pgd_get("u")
    plain.close()
    eng, _ = start()
    u, phi, phi_Q = eng.pgd_get("u"), eng.pgd_get("phi"), eng.pgd_get("phi_Q")
    assert np.abs(u).max() > 0
    R = eng.RESIDENT
    res = eng.second_order(H, t, opt, u=R, phi_Q=R, phi_T=R, dt=dts, histories=True)
    explicit = eng.second_order(H, t, opt, phi_hist=phi, u=u, phi_Q=phi_Q, phi_T=phi_T, dt=dts, histories=True)
    _same(res, explicit)
    assert np.array_equal(eng.pgd_get("u"), u) and np.array_equal(eng.pgd_get("phi"), phi)
    for b in range(2):
        d1, d2 = tangent_reference_1d(P, phi[b], t, H[b], dts=dts)
        S = tangent_scalars_1d(phi[b], d1, d2, u[b], H[b], phi_Q[b], phi_T[b], x, t, opt.b1, opt.b2, opt.b3)
        devs = {k: abs(float(res[k][b]) / S[k] - 1.0) for k in ALL}
        print(f"pgd b={b}: dphi {_rel(res['dphi'][b], d1):.2e} d2phi {_rel(res['d2phi'][b], d2):.2e} scalars "
              + " ".join(f"{k} {v:.2e}" for k, v in devs.items()))
        assert _rel(res["dphi"][b], d1) < TOL[0][0] and _rel(res["d2phi"][b], d2) < TOL[0][1]
        assert max(devs.values()) < TOL[0][2], devs
    got = eng.pgd_iterate(2)
    for k in ("cost", "alpha", "trials", "change", "tracking_error", "terminal_error"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(eng.pgd_get("u"), u_want)
    eng.close()


def test_error_codes_come_before_any_launch(V, runs):
    pr = runs("n32")
    eng, H, t, opt = pr["eng"], pr["H"], pr["t"], pr["opt"]
    fresh = _engine(V, pr["P"], 3)
    with pytest.raises(V.VchError, match="-3"):                      # no resident history
        fresh.second_order(H, t, opt)
    with pytest.raises(V.VchError, match="-3"):                      # RESIDENT before pgd_init
        _call(pr, eng=fresh, u=fresh.RESIDENT)
    with pytest.raises(V.VchError, match="-3"):
        _call(pr, eng=fresh, phi_T=fresh.RESIDENT)
    fresh.forward(pr["phi0"], pr["dts"][:-1], u=pr["U"][:, :-1])
    with pytest.raises(V.VchError, match="-3"):                      # a resident history with another number of rows
        fresh.second_order(H, t, opt)
    fresh.close()
    bad_dt = pr["dts"].copy()
    bad_dt[1] = 0.0
    inf_dt = pr["dts"].copy()
    inf_dt[0] = math.inf
    t_back = t.copy()
    t_back[3] = t_back[2]
    big = eng.max_steps + 3
    bad = [
        (dict(opt=[opt, opt]), "n_opts"),
        (dict(order=3), "order"),
        (dict(order=0), "order"),
        (dict(dt=bad_dt), "dt"),
        (dict(dt=inf_dt), "dt"),
        (dict(opt=V.make_opt(b1=math.nan)), "b1, b2, b3"),
        (dict(opt=[opt, opt, V.make_opt(b3=math.inf)]), "trajectory 2"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            _call(pr, **kw)
    with pytest.raises(ValueError, match="dt"):                      # dt derived from a t_hist that does not advance
        eng.second_order(H, t_back, opt, phi_hist=pr["phi"])
    # what the wrapper cannot express goes through the C ABI itself
    lib, D = eng.lib, C.POINTER(C.c_double)
    dp = lambda a: a.ctypes.data_as(D)
    out = np.full((3, 6), 7.0)
    last_error = V.module("_lib").last_error
    arr = (type(opt) * 1)(opt)
    hbig, tbig = np.zeros((3, big, eng.n)), np.linspace(0.0, 1.0, big)

    def raw(phi=pr["phi"], n_base=3, h=H, rows=pr["rows"], tt=t, x=pr["x"], o_=out):
        return lib.vch1d_second_order(eng.ctx, dp(phi), None, n_base, None if h is None else dp(h), rows, None,
                                      None if tt is None else dp(tt), None if x is None else dp(x), None, None, arr, 1, 2,
                                      None if o_ is None else dp(o_), None, None, None)

    for kw, what in [(dict(rows=2), "rows"), (dict(rows=big, h=hbig, tt=tbig), "rows"), (dict(n_base=2), "n_base"),
                     (dict(h=None), "NULL direction"), (dict(tt=None), "NULL t_hist"), (dict(x=None), "NULL x"),
                     (dict(o_=None), "NULL out")]:
        assert raw(**kw) == -1, kw.keys()
        assert what in last_error(), (what, last_error())
    assert (out == 7.0).all()
    # ... and the context still answers, with the bits of the first call
    _same(_call(pr, histories=True), pr["res"])


def test_driver_level_exact_condition(V, capsys):
    """exact_second_order_condition: one entry per direction, the directions of approximate_second_order_condition for the
    same seed, and the curvature of the central second difference of forward + cost to the oracle's own discrepancy."""
    S1 = V.module("Vch_control_1D.second_order_conditions")
    K1 = V.module("Vch_control_1D.config")
    D = DRIVER
    P, phi0, u_star, r_star = driver_problem()
    cfg = K1.ForwardSolverConfig(N=P.N, T=P.T, dt_initial=P.dt_initial)
    tg, dts = V.time_grid(P.T, P.dt_initial)
    t = np.concatenate([[0.0], tg])
    x = np.linspace(0.0, P.Lx, P.N + 1)
    O = o.OptParams1D()
    nd = D["num_directions"]
    eng = _engine(V, P, nd)
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (nd,) + a.shape))
    phi_star = eng.forward(tile(phi0), dts, u=tile(u_star))[0][0]
    assert np.abs(phi_star).max() < 1.0 - o.DELTA_SEP - 0.1
    phi_T, phi_Q = o.build_targets(x, t, phi_star[0], P.Lx, P.T)
    exact = S1.exact_second_order_condition(cfg, u_star, r_star, phi_star, x, t, O.b1, O.b2, O.b3, O.kappa_sparsity, phi_Q,
                                            phi_T, D["u_min"], D["u_max"], num_directions=nd, seed=D["seed"])
    printed = capsys.readouterr().out
    assert len(exact) == nd and all(math.isfinite(v) and v > 0 for v in exact)
    assert printed.count("exact slope") == nd and printed.count("adjoint sum(g·h)") == nd
    # the first nd draws of the generator, as approximate_second_order_condition makes them
    rng = np.random.default_rng(D["seed"])
    dirs = np.stack([S1._generate_direction(u_star, r_star, D["u_min"], D["u_max"], O.kappa_sparsity, O.b3, rng)
                     for _ in range(nd)])
    assert (np.abs(u_star) >= D["u_max"] - 1e-8).any()              # some nodes sit on the box: the cone is not the whole space
    opt = V.make_opt(b1=O.b1, b2=O.b2, b3=O.b3, kappa_sparsity=0.0)
    res = eng.second_order(dirs, t, opt, phi_hist=phi_star, u=u_star, phi_Q=phi_Q, phi_T=phi_T, x=x, shared_base=True)
    assert list(res["curvature"]) == exact

    def J(U):
        ph = eng.forward(tile(phi0), dts, u=U)[0]
        return eng.cost(ph, U, tile(phi_Q), tile(phi_T), x, t, opt)[:, :3].sum(axis=1)

    e = D["eps"]
    fd = (J(u_star + e * dirs) - 2.0 * J(tile(u_star)) + J(u_star - e * dirs)) / e ** 2
    eng.close()
    dev = np.abs(fd / np.array(exact) - 1.0)
    print("driver: exact", exact, "central difference", list(fd), "rel.dev", list(dev))
    assert dev.max() < DRIVER_TOL
