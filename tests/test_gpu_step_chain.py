"""The shortened chain of a forward time step on the default path, each part against the launches it replaces:

  VCH_MASS_EARLY   the step's k_mass is enqueued in front of the host's look, gated on the Newton loop having ended, and
                   repeated behind the continuation loop of a step that did not fit its schedule;
  VCH_FIN_PUBLISH  the k_fin_residual<1> in front of a look copies its trajectory's record to mapped host memory and
                   stores the look's number to the trajectory's own sequence slot (no k_publish_state launch);
  VCH_CEIL_CELL    the step ceiling of a reduction-free solve is folded into one 64-bit cell per trajectory by the
                   solve's last row kernel (atomic minimum on an order-preserving key), the trial kernel and the
                   k_fin_residual<1> behind it arm the trial themselves (no k_fin_ceiling launch).

A trajectory's arithmetic does not change, so everything is compared bit for bit (`=0` restores the replaced form)."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("VCH_MASS_EARLY", "VCH_FIN_PUBLISH", "VCH_CEIL_CELL")
ALL_OFF = {s: "0" for s in SWITCHES}
COUNTS = ("newton_iters", "linear_solves", "armijo_trials", "linear_iters", "host_syncs")


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


@pytest.fixture(scope="module")
def O2():
    from oracle import vch2d_oracle
    return vch2d_oracle


class _env:
    """Environment for the engines created inside the block (the switches are read when an engine is created)."""

    def __init__(self, env):
        self.env = {k: str(v) for k, v in env.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _marches(V, env, phi0, dts, u=None, n=2, **engine_kw):
    """n marches on one engine: a stale ceiling cell or sequence slot shows in the second."""
    with _env(env):
        e = V.Engine2D(batch=phi0.shape[0], max_steps=len(dts), **engine_kw)
        try:
            return [e.forward(phi0, dts, u=u) for _ in range(n)]
        finally:
            e.close()


def _counts(st):
    return tuple(st[k] for k in COUNTS)


@pytest.fixture(scope="module")
def uneven(V, O2):
    """128 x 64 (rectangular, partial edge tiles, pitch != width), 30 steps, three trajectories with uneven starts under
    a control; the default engine's two marches, computed once."""
    Nx, Ny, M = 128, 64, 30
    _, dts = V.time_grid(M * 1e-3, 1e-3)
    phi0 = np.stack([O2.init_phi_random(Nx, Ny, 1e-2, amp=a, seed=42 + i) for i, a in enumerate((0.1, 0.6, 0.05))])
    shape = np.sin(2 * np.pi * np.linspace(0, 1, Nx + 1))[:, None] * np.cos(np.pi * np.linspace(0, 1, Ny + 1))[None, :]
    u = np.stack([a * np.linspace(0, 1, M + 1)[:, None, None] * shape[None] for a in (3.0, -2.0, 0.5)])
    kw = dict(Nx=Nx, Ny=Ny)
    return dict(phi0=phi0, dts=dts, u=u, kw=kw, M=M, ref=_marches(V, {}, phi0, dts, u, **kw))


@pytest.mark.parametrize("off", [("VCH_MASS_EARLY",), ("VCH_FIN_PUBLISH",), ("VCH_CEIL_CELL",), SWITCHES])
def test_each_part_against_the_form_it_replaces(V, uneven, off):
    (ph, st), (ph_b, st_b) = uneven["ref"]
    # (an engine's second march starts from the schedule its first one ended with: sweeps re-run by a slot that was too
    # short, and with them the launches, differ between the two -- in every form alike)
    assert np.array_equal(ph, ph_b) and _counts(st)[:3] == _counts(st_b)[:3], (st, st_b)
    out = _marches(V, {s: "0" for s in off}, uneven["phi0"], uneven["dts"], uneven["u"], **uneven["kw"])
    for (ph1, st1), (ph0, st0) in zip(uneven["ref"], out):
        assert np.array_equal(ph1, ph0), float(np.max(np.abs(ph1 - ph0)))
        assert _counts(st1) == _counts(st0), (st1, st0)
    st0 = out[0][1]
    print("launches: default", st["launches"], "with", off, "off", st0["launches"], "| solves", st["linear_solves"])
    # Launch counts.  The cells save one k_fin_ceiling launch per enqueued reduction-free sequence (the trajectories of a
    # batch share it, and a slot is enqueued whether or not a trajectory uses it, so the statistics do not give the exact
    # number).  The early k_mass is repeated once per step that did not fit its schedule: at most one per extra look, and
    # fewer than the sequences saved (every such step enqueues sequences of its own).  The publishing launch is not in
    # the count in either form.
    unfit_max = st["host_syncs"] - uneven["M"]
    if "VCH_CEIL_CELL" in off:
        assert st0["launches"] > st["launches"], (st, st0)
    elif "VCH_MASS_EARLY" in off:
        assert 0 <= st["launches"] - st0["launches"] <= unfit_max, (st, st0)
    else:
        assert st0["launches"] == st["launches"], (st, st0)


def test_step_that_does_not_fit_the_schedule(V, uneven):
    """VCH_CHEB_MARGIN=0 leaves the schedule no slack, so steps whose plans grow are finished by the continuation loop (one
    look per Armijo trial): the early k_mass skips the unfinished trajectories and is repeated behind the loop, the looks of
    the loop are published by its own k_fin_residual launches.  Against the replaced launches and against a look after
    every phase (VCH_NO_SPEC=1)."""
    M, tight = uneven["M"], {"VCH_CHEB_MARGIN": "0"}
    run = lambda env: _marches(V, env, uneven["phi0"], uneven["dts"], uneven["u"], **uneven["kw"])
    (ph, st), (ph_b, st_b) = run(tight)
    print("looks", st["host_syncs"], "steps", M)
    assert st["host_syncs"] > M + 1, st                   # the continuation loop really runs
    assert np.array_equal(ph, ph_b) and _counts(st)[:3] == _counts(st_b)[:3]
    for (ph0, st0), ref in zip(run({**tight, **ALL_OFF}), ((ph, st), (ph_b, st_b))):
        assert np.array_equal(ref[0], ph0) and _counts(ref[1]) == _counts(st0), (ref[1], st0)
    for ph1, st1 in run({"VCH_NO_SPEC": "1"}):      # (no slot is ever too short there: Newton / solve / trial counts only)
        assert np.array_equal(ph, ph1) and _counts(st)[:3] == _counts(st1)[:3], (st, st1)
    assert np.array_equal(ph, uneven["ref"][0][0])        # (the margin changes nothing either)


def test_frozen_trajectories_and_the_line_search(V, O2):
    """Three PGD iterations whose line searches end after different numbers of trials: the accepted trajectories sit the
    remaining trial marches out (frozen), where every tail of k_fin_residual still has to run for them."""
    N, T, dt = 32, 0.1, 1e-2
    t, dts = V.time_grid(T, dt)
    xs = np.linspace(0, 1, N + 1)
    base = np.sin(2 * np.pi * xs)[:, None] * np.cos(np.pi * xs)[None, :]
    phi_T = np.stack([a * base for a in (0.7, 0.3, 0.02)])
    phi0 = np.stack([O2.init_phi_random(N, N, 1e-2, amp=0.1, seed=7 + i) for i in range(3)])
    opt = V.make_opt(alpha_max=4.0e4)

    def run(env):
        with _env(env):
            e = V.Engine2D(Nx=N, Ny=N, batch=3, max_steps=len(dts))
            try:
                e.pgd_init(phi0, phi_T, t, opt, ramp=True, T=T)
                r = e.pgd_iterate(3)
                return r, e.pgd_get("u"), e.pgd_get("phi")
            finally:
                e.close()
    r, u, ph = run({})
    print("attempts", np.asarray(r["attempts"]).tolist())
    assert len({tuple(a) for a in np.asarray(r["attempts"]).tolist()}) > 1, r["attempts"]     # the searches really differ
    r0, u0, ph0 = run(ALL_OFF)
    for k in ("cost", "alpha", "attempts"):
        assert np.array_equal(r[k], r0[k]), (k, r[k], r0[k])
    assert np.array_equal(u, u0) and np.array_equal(ph, ph0)


def _first_ceiling_ratio(O2, phi0, dt, **phys):
    """min over the nodes of (+-(1 - delta) - phi) / dphi (F2:381-387) for the first Newton iteration of the first step
    from phi0 (w = 0), with the oracle's operators and a direct solve."""
    from scipy.sparse.linalg import spsolve
    Nx, Ny = phi0.shape[0] - 1, phi0.shape[1] - 1
    P = O2.Params2D(Nx=Nx, Ny=Ny, T=dt, dt_initial=dt, **phys)
    hx, hy = P.Lx / Nx, P.Ly / Ny
    w = np.zeros_like(phi0)
    mu = O2.mu_init(phi0, w, P, hx, hy)
    R = np.concatenate([O2.residual_phi(phi0, phi0, mu, mu, w, w, dt, P, hx, hy).ravel(),
                        O2.residual_mu(phi0, phi0, mu, mu, dt, hx, hy).ravel()])
    d = spsolve(O2.jac_matrix(phi0, dt, P, O2.lap_matrix(Nx, Ny, hx, hy)).tocsc(), -R)[:phi0.size]
    pf, lim = phi0.ravel(), 1.0 - O2.DELTA_SEP
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, (lim - pf) / d, np.where(d < 0, (-lim - pf) / d, np.inf))
    return float(np.min(r))


@pytest.mark.parametrize("case", ["binds", "negative"])
def test_ceiling_that_binds_and_one_that_is_negative(V, O2, case):
    """32^2, 3 steps from a start near the band, every solve in the reduction-free form (VCH_CHEB_MAX lifts the cap on the
    plan's length, which such a start exceeds).  `binds`: a smooth start of amplitude 0.97 under a shallow potential
    (c1 = 0.3) that drives phi outwards -- the first Newton step may go 0.96 of its length, so alpha = 0.9 x that < 1
    (oracle, checked here).  `negative`: the clipped-noise start of the stress goldens (amp = 1.0) with two nodes moved
    outside the band: ratios <= 0 from the first iteration on (alpha falls back to 1).  The ceiling from the cell must be the
    one k_fin_ceiling reduces from the per-workgroup minima: counts and every stored level bit for bit."""
    N, M, c1 = 32, 3, 0.3
    xs = np.linspace(0, 1, N + 1)
    if case == "binds":
        dt = 5e-3
        phi0 = 0.97 * np.cos(np.pi * xs)[:, None] * np.cos(2 * np.pi * xs)[None, :]
        ratio = _first_ceiling_ratio(O2, phi0, dt, c1=c1)
        assert 0.5 < ratio < 1.05, ratio                  # alpha = 0.9 x ratio: in (0.45, 0.945)
    else:
        dt = 1e-3
        phi0 = O2.init_phi_random(N, N, 1e-2, amp=1.0, seed=42)
        phi0[np.unravel_index(np.argmax(phi0), phi0.shape)] = 0.995
        phi0[np.unravel_index(np.argmin(phi0), phi0.shape)] = -0.995
        ratio = _first_ceiling_ratio(O2, phi0, dt, c1=c1)
        assert ratio <= 0.0, ratio
    phi0 = phi0[None]
    dts = np.full(M, dt)
    cheb = {"VCH_CHEB_MAX": "200"}
    (ph, st), (ph_b, st_b) = _marches(V, cheb, phi0, dts, Nx=N, Ny=N, c1=c1)
    (ph0, st0), (ph0b, st0b) = _marches(V, {**cheb, "VCH_CEIL_CELL": "0"}, phi0, dts, Nx=N, Ny=N, c1=c1)
    print(case, "ratio", ratio, st, st0)
    assert st0["launches"] > st["launches"], (st, st0)    # reduction-free solves did run
    if case == "binds":
        # a Newton step shorter than 1 costs at least one iteration more than the three or four of a free step
        assert st["newton_iters"] > 4 * M, st
    assert _counts(st) == _counts(st0) and _counts(st_b) == _counts(st0b), (st, st0, st_b, st0b)
    assert _counts(st)[:3] == _counts(st_b)[:3], (st, st_b)
    assert np.array_equal(ph, ph0) and np.array_equal(ph, ph_b) and np.array_equal(ph, ph0b)
    assert np.all(np.isfinite(ph)) and np.max(np.abs(ph[1:])) <= 1.0 - O2.DELTA_SEP       # (level 0 is the start itself)


def test_two_contexts_at_once(V, O2):
    """Two engines of batch 2 marching concurrently from two threads: each equals its own solo run (a context polls its
    own per-trajectory sequence slots and folds into its own cells)."""
    N, M = 64, 20
    _, dts = V.time_grid(M * 1e-3, 1e-3)
    starts = [np.stack([O2.init_phi_random(N, N, 1e-2, amp=a, seed=s) for a, s in pair])
              for pair in (((0.1, 3), (0.5, 4)), ((0.3, 5), (0.05, 6)))]
    solo = [_marches(V, {}, p, dts, n=1, Nx=N, Ny=N)[0] for p in starts]
    engines = [V.Engine2D(Nx=N, Ny=N, batch=2, max_steps=M) for _ in starts]
    out, errs = [None, None], []
    go = threading.Barrier(2)

    def work(i):
        try:
            go.wait()
            out[i] = [engines[i].forward(starts[i], dts) for _ in range(2)]
        except Exception as exc:      # noqa: BLE001 (reported by the assertion below)
            errs.append(exc)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for e in engines:
        e.close()
    assert not errs, errs
    for i in range(2):
        for k, (ph, st) in enumerate(out[i]):
            assert np.array_equal(ph, solo[i][0]) and _counts(st)[:3] == _counts(solo[i][1])[:3], (i, st, solo[i][1])
            assert k > 0 or _counts(st) == _counts(solo[i][1]), (i, st, solo[i][1])
