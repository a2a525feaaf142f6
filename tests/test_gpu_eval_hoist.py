"""The evaluation kernels with their loads hoisted (k_eval, the default) against the form they replace (k_eval_plain,
VCH_EVAL_HOIST=0):

  step start   k_mass's partials, raw phi, mu of the old level, w and the u pair are requested before the first barrier;
  guess tail   the increment planes are read into registers from the last halo-1 pass on, D on halo 1 is taken where phi is
               still at hand (the separate jac_diag pass and its barriers are gone).

No expression, operand order or summation order differs, so everything is compared bit for bit.  The switch is read when
an engine is created."""
import os

import numpy as np
import pytest

from conftest import golden, relerr

pytestmark = pytest.mark.gpu

PLAIN = {"VCH_EVAL_HOIST": "0"}
COUNTS = ("newton_iters", "linear_solves", "armijo_trials", "linear_iters", "host_syncs")
MARCH = 1e-8          # test_gpu_2d.py's bound for marched fields against a golden file


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


def _marches(V, env, phi0, dts, u=None, n=2, **engine_kw):
    """n marches on one engine (the second starts from the schedule and the guess tables the first one left):
    [(phi, stats, mass_shifts)]."""
    with _env(env):
        e = V.Engine2D(batch=phi0.shape[0], max_steps=len(dts), **engine_kw)
        try:
            out = []
            for _ in range(n):
                ph, st = e.forward(phi0, dts, u=u)
                out.append((ph, st, e.mass_shifts()))
            return out
        finally:
            e.close()


def _same(a, b):
    """Two marches: histories, shifts of the mass fix, the five counters and the launches."""
    (ph1, st1, s1), (ph0, st0, s0) = a, b
    assert np.array_equal(ph1, ph0), float(np.max(np.abs(ph1 - ph0)))
    assert np.array_equal(s1, s0), (s1, s0)
    assert tuple(st1[k] for k in COUNTS) == tuple(st0[k] for k in COUNTS), (st1, st0)
    assert st1["launches"] == st0["launches"], (st1, st0)


@pytest.fixture(scope="module")
def uneven(V, O2):
    """128 x 64, 30 steps, three trajectories with uneven starts under a control: 129 x 65 nodes, so a one-column and a
    one-row edge tile, pitch != width and a mass fix that is not the identity.  30 steps take the orders of the guesses up
    to their maximum."""
    Nx, Ny, M = 128, 64, 30
    _, dts = V.time_grid(M * 1e-3, 1e-3)
    phi0 = np.stack([O2.init_phi_random(Nx, Ny, 1e-2, amp=a, seed=42 + i) for i, a in enumerate((0.1, 0.6, 0.05))])
    shape = np.sin(2 * np.pi * np.linspace(0, 1, Nx + 1))[:, None] * np.cos(np.pi * np.linspace(0, 1, Ny + 1))[None, :]
    u = np.stack([a * np.linspace(0, 1, M + 1)[:, None, None] * shape[None] for a in (3.0, -2.0, 0.5)])
    return dict(phi0=phi0, dts=dts, u=u, kw=dict(Nx=Nx, Ny=Ny), M=M)


@pytest.mark.parametrize("other", [{}, {"VCH_POST_FOLD": "0"}, {"VCH_NO_SPEC": "1"}, {"VCH_CHEB_MARGIN": "0"}],
                         ids=["default", "post_fold_0", "no_spec", "cheb_margin_0"])
def test_march_with_sliver_tiles(V, uneven, other):
    """Two marches on one engine in either form.  VCH_POST_FOLD=0: nothing is pending at a step start (the other arm of the
    hoisted prologue); VCH_NO_SPEC=1: a look after every phase; VCH_CHEB_MARGIN=0: the continuation loop runs."""
    run = lambda env: _marches(V, {**other, **env}, uneven["phi0"], uneven["dts"], uneven["u"], **uneven["kw"])
    new, old = run({}), run(PLAIN)
    st = new[0][1]
    print(other, "stats", st, "shifts of trajectory 0, first steps", new[0][2][0][:3])
    if "VCH_CHEB_MARGIN" in other:
        assert st["host_syncs"] > uneven["M"] + 1, st         # the continuation loop really runs
    assert np.abs(new[0][2]).max() > 0                        # the mass fix is not the identity here
    for a, b in zip(new, old):
        _same(a, b)


@pytest.mark.parametrize("env", [{}, PLAIN], ids=["hoist", "plain"])
def test_batch_equals_single_on_a_square_grid(V, O2, env):
    """64 x 64 (every tile full but the one-node slivers of the 65th row and column), 20 steps, no control: trajectory 0 of
    a batch of 3 equals its run alone, in both forms, and the forms equal each other."""
    N, M = 64, 20
    _, dts = V.time_grid(M * 1e-3, 1e-3)
    phi0 = np.stack([O2.init_phi_random(N, N, 1e-2, amp=a, seed=11 + i) for i, a in enumerate((0.1, 0.5, 0.02))])
    (ph1, st1, s1), = _marches(V, env, phi0[:1], dts, n=1, Nx=N, Ny=N)
    (ph3, st3, s3), = _marches(V, env, phi0, dts, n=1, Nx=N, Ny=N)
    ph3 = ph3.reshape((3,) + ph3.shape[-3:])
    ph1 = ph1.reshape((1,) + ph1.shape[-3:])
    assert np.array_equal(ph3[0], ph1[0]), float(np.max(np.abs(ph3[0] - ph1[0])))
    assert np.array_equal(s3[0], s1[0])
    if env:
        (ph3d, st3d, s3d), = _marches(V, {}, phi0, dts, n=1, Nx=N, Ny=N)
        _same((ph3d, st3d, s3d), (ph3.reshape(ph3d.shape), st3, s3))


def test_pgd_loop_with_backtracking(V, O2):
    """16 x 16 with the settings of g2d_pgd_16_bt.npz (an overshooting first step: backtracking, so frozen trajectories
    and partial batches), 3 iterations, batch 3 whose trajectory 0 is the golden run."""
    g = golden("g2d_pgd_16_bt.npz")
    N, M, n_iter = int(g["N"]), len(g["t_hist"]) - 1, int(g["n_iter"])
    assert n_iter == 3
    opt = V.make_opt(alpha_max=float(g["alpha_max"]), b3=float(g["b3"]))
    phi0 = np.stack([O2.init_phi_random(N, N, 1e-2, amp=0.1, seed=42 + i) for i in range(3)])
    phi_T = np.stack([a * g["phi_T"] for a in (1.0, 0.4, 0.03)])

    def run(env):
        with _env(env):
            e = V.Engine2D(Nx=N, Ny=N, batch=3, max_steps=M)
            try:
                e.pgd_init(phi0, phi_T, g["t_hist"], opt, ramp=True, T=float(g["T"]))
                r = e.pgd_iterate(n_iter)
                return r, e.pgd_get("u"), e.pgd_get("phi")
            finally:
                e.close()
    r, u, ph = run({})
    r0, u0, ph0 = run(PLAIN)
    print("attempts", np.asarray(r["attempts"]).tolist())
    for k in ("cost", "alpha", "attempts", "change"):
        assert np.array_equal(r[k], r0[k]), (k, r[k], r0[k])
    assert np.array_equal(u, u0) and np.array_equal(ph, ph0)
    # the default form against the golden file, with test_gpu_2d.py::test_pgd_vs_golden's bounds
    assert np.allclose(r["cost"][0], g["costs"][1:], rtol=1e-8), (r["cost"], g["costs"])
    assert np.allclose(r["alpha"][0], g["alphas"], rtol=1e-13), (r["alpha"], g["alphas"])
    assert list(r["attempts"][0]) == list(g["attempts"])
    assert np.allclose(r["change"][0], g["changes"], rtol=1e-6)
    assert relerr(u[0], g["u_final"]) < MARCH
    assert relerr(ph[0], g["phi_final"]) < MARCH
