"""The transform kernels with a phase's global operands requested together (the default: k_dct_cols' column data and
multiplier entries, every pass's twiddles ahead of the barriers, the operands of k_cheb_rows' update for a batch of a thread's
nodes) against the forms they replace (k_dct_cols_plain, k_dct_rows_plain, k_cheb_rows_plain: VCH_ROWS_BATCH=0).

No expression, operand order or summation order differs, so everything is compared bit for bit.  The changed code exists for
256 / 512 / 1024 intervals on an axis (FFT lengths 512 / 1024 / 2048); 16 intervals on the other axis are 17 rows or columns:
a partial last row group and an odd last column pair.  64 x 32 runs the run-time-length paths of the shared scaffold.  The
switch is read when an engine is created."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAIN = {"VCH_ROWS_BATCH": "0"}
COUNTS = ("newton_iters", "linear_solves", "armijo_trials", "linear_iters", "host_syncs")
GRIDS = [(256, 16), (16, 256), (512, 16), (16, 512), (1024, 16), (16, 1024), (64, 32)]
M = 12
AMPS = (0.1, 0.6, 0.05)


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
    """Environment for the engines created inside the block."""

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


_cases = {}


def _case(V, O2, Nx, Ny):
    """Three trajectories with uneven starts under a control, M steps (built once per grid)."""
    if (Nx, Ny) not in _cases:
        t, dts = V.time_grid(M * 1e-3, 1e-3)
        phi0 = np.stack([O2.init_phi_random(Nx, Ny, 1e-2, amp=a, seed=42 + i) for i, a in enumerate(AMPS)])
        shape = np.sin(2 * np.pi * np.linspace(0, 1, Nx + 1))[:, None] * np.cos(np.pi * np.linspace(0, 1, Ny + 1))[None, :]
        u = np.stack([a * np.linspace(0, 1, M + 1)[:, None, None] * shape[None] for a in (3.0, -2.0, 0.5)])
        phi_T = np.stack([a * 0.7 * shape for a in (1.0, 0.4, 0.03)])
        _cases[(Nx, Ny)] = dict(t=t, dts=dts, phi0=phi0, u=u, phi_T=phi_T)
    return _cases[(Nx, Ny)]


def _marches(V, env, c, Nx, Ny, n=2, adjoint=False):
    """n marches on one engine (the second starts from the schedule and the guess tables the first one left), then
    optionally the adjoint sweep on the resident history: [(phi, stats, mass_shifts)], (p, q, r) or None."""
    with _env(env):
        e = V.Engine2D(Nx=Nx, Ny=Ny, batch=c["phi0"].shape[0], max_steps=len(c["dts"]))
        try:
            out = []
            for _ in range(n):
                ph, st = e.forward(c["phi0"], c["dts"], u=c["u"])
                out.append((ph, st, e.mass_shifts()))
            adj = None
            if adjoint:
                p, q, r, _ = e.backward(None, c["t"], 5.0, 10.0, None, c["phi_T"])
                adj = (p, q, r)
            return out, adj
        finally:
            e.close()


def _same(a, b):
    """Two marches: histories, shifts of the mass fix, the five counters and the launches."""
    (ph1, st1, s1), (ph0, st0, s0) = a, b
    assert np.array_equal(ph1, ph0), float(np.max(np.abs(ph1 - ph0)))
    assert np.array_equal(s1, s0), (s1, s0)
    assert tuple(st1[k] for k in COUNTS) == tuple(st0[k] for k in COUNTS), (st1, st0)
    assert st1["launches"] == st0["launches"], (st1, st0)


SETTINGS = {
    "default": {},
    "lin_eta_0": {"VCH_LIN_ETA": "0"},            # long plans: sweeps j >= 2 read y_prev, plans beyond cheb_max take the CG form
    "cheb_0": {"VCH_CHEB": "0"},                  # k_cg_rows_fwd, k_dct_rows<3 / 4>
    "continuation": {"VCH_CHEB_MARGIN": "0", "VCH_NO_SPEC": "1"},
}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("Nx,Ny", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_forward_march(V, O2, Nx, Ny, setting):
    """Two marches on one engine in either form, under the settings that reach the other forms of the solve."""
    other = SETTINGS[setting]
    c = _case(V, O2, Nx, Ny)
    new, _ = _marches(V, other, c, Nx, Ny)
    old, _ = _marches(V, {**other, **PLAIN}, c, Nx, Ny)
    st = new[0][1]
    print(setting, (Nx, Ny), "stats", {k: st[k] for k in COUNTS + ("launches",)})
    if setting == "lin_eta_0":
        assert st["linear_iters"] > st["linear_solves"], st    # some solve ran at least two sweeps
    if setting == "continuation":
        assert st["host_syncs"] > M + 1, st                   # the continuation loop really runs
    for a, b in zip(new, old):
        _same(a, b)


@pytest.mark.parametrize("Nx,Ny", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_adjoint_sweep(V, O2, Nx, Ny):
    """Engine2D.backward on a marched history (k_adj_rows_fwd, k_dct_rows<0 / 4 / 5>, k_dct_cols): p, q and r."""
    c = _case(V, O2, Nx, Ny)
    _, new = _marches(V, {}, c, Nx, Ny, n=1, adjoint=True)
    _, old = _marches(V, PLAIN, c, Nx, Ny, n=1, adjoint=True)
    for name, a, b in zip("pqr", new, old):
        assert np.abs(a).max() > 0, name
        assert np.array_equal(a, b), (name, float(np.max(np.abs(a - b))))


@pytest.mark.parametrize("Nx,Ny", [(512, 16), (16, 512)], ids=["512x16", "16x512"])
def test_pgd_iterations(V, O2, Nx, Ny):
    """Two PGD iterations with three trajectories: the forms agree, and trajectory 0 of the batch equals its run alone."""
    c = _case(V, O2, Nx, Ny)
    opt = V.make_opt()

    def run(env, nb):
        with _env(env):
            e = V.Engine2D(Nx=Nx, Ny=Ny, batch=nb, max_steps=M)
            try:
                e.pgd_init(c["phi0"][:nb], c["phi_T"][:nb], c["t"], opt, ramp=True, T=float(c["t"][-1]))
                r = e.pgd_iterate(2)
                u, ph = e.pgd_get("u"), e.pgd_get("phi")
                return r, u.reshape((nb,) + u.shape[-3:]), ph.reshape((nb,) + ph.shape[-3:])
            finally:
                e.close()
    r, u, ph = run({}, 3)
    r0, u0, ph0 = run(PLAIN, 3)
    r1, u1, ph1 = run({}, 1)
    print("cost", np.asarray(r["cost"]).tolist(), "attempts", np.asarray(r["attempts"]).tolist())
    for k in ("cost", "alpha", "attempts", "change"):
        assert np.array_equal(r[k], r0[k]), (k, r[k], r0[k])
        assert np.array_equal(r[k][0], r1[k][0]), (k, r[k], r1[k])
    assert np.array_equal(u, u0) and np.array_equal(ph, ph0)
    assert np.array_equal(u[0], u1[0]) and np.array_equal(ph[0], ph1[0])
