"""The kernels that request their global operands together (the default) against the forms they replace (the _plain kernels,
VCH_LOADS_BATCH=0):

  adjoint sweep   k_adj_finish: the tile and r, q_old of a thread's own nodes in one round;
                  k_adj_guess: x and every plane with a coefficient, for all of a thread's nodes, before the first use;
  forward march   k_fin_residual: the record, the partials (FIN_PU = 5 per lane in flight, a rolled tail beyond 64 * FIN_PU
                  tiles), the two sums of a reduction-free solve and the ceiling cell, all in front of the first barrier;
  everywhere      load_tile with a compile-time trip count (every kernel but the _plain ones, k_adj_rhs and k_adj_op; it has
                  no switch, so the march and the sweep against the oracle and the golden files are its test).

No expression, operand order or summation order differs, so everything is compared bit for bit.  The switch is read when an
engine is created."""
import os

import numpy as np
import pytest

from conftest import golden, relerr

pytestmark = pytest.mark.gpu

PLAIN = {"VCH_LOADS_BATCH": "0"}
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


def _run(V, env, c, n=2, adjoint=False, nb=None):
    """n marches on one engine (the second starts from the schedule and the guess tables the first one left), then
    optionally the adjoint sweep on the resident history with both targets set:
    [(phi, stats, mass_shifts)], (p, q, r, stats) or None.  nb: the first nb trajectories of the case only."""
    nb = c["phi0"].shape[0] if nb is None else nb
    with _env(env):
        e = V.Engine2D(batch=nb, max_steps=len(c["dts"]), **c["kw"])
        try:
            out = []
            for _ in range(n):
                ph, st = e.forward(c["phi0"][:nb], c["dts"], u=None if c["u"] is None else c["u"][:nb])
                out.append((ph, st, e.mass_shifts()))
            adj = None
            if adjoint:
                adj = e.backward(None, c["t"], 5.0, 10.0, c["phi_Q"][:nb], c["phi_T"][:nb])
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


def _same_adjoint(a, b):
    """Two sweeps: p, q, r, the five counters and the launches."""
    for name, x, y in zip("pqr", a[:3], b[:3]):
        assert np.abs(x).max() > 0, name
        assert np.array_equal(x, y), (name, float(np.max(np.abs(x - y))))
    keys = COUNTS + ("launches", "unconverged_solves", "max_lin_relres", "max_lin_absres")
    assert tuple(a[3][k] for k in keys) == tuple(b[3][k] for k in keys), (a[3], b[3])


def _case(V, O2, Nx, Ny, M, amps, uamps=None, seed=42):
    t, dts = V.time_grid(M * 1e-3, 1e-3)
    phi0 = np.stack([O2.init_phi_random(Nx, Ny, 1e-2, amp=a, seed=seed + i) for i, a in enumerate(amps)])
    shape = np.sin(2 * np.pi * np.linspace(0, 1, Nx + 1))[:, None] * np.cos(np.pi * np.linspace(0, 1, Ny + 1))[None, :]
    u = None if uamps is None else np.stack([a * np.linspace(0, 1, M + 1)[:, None, None] * shape[None] for a in uamps])
    phi_T = np.stack([a * 0.7 * shape for a in (1.0, 0.4, 0.03)[:len(amps)]])
    phi_Q = np.stack([a * np.linspace(0, 1, M + 1)[:, None, None] * shape[None] for a in (0.5, -0.3, 0.02)[:len(amps)]])
    return dict(t=t, dts=dts, phi0=phi0, u=u, phi_T=phi_T, phi_Q=phi_Q, kw=dict(Nx=Nx, Ny=Ny), M=M)


# ------------------------------------------------------------------------------------------------------------------
# A. marches and the adjoint sweep on the grid with sliver tiles
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def uneven(V, O2):
    """128 x 64, 30 steps, three trajectories with uneven starts under a control: 129 x 65 nodes, so a one-column and a
    one-row edge tile, pitch != width, a mass fix that is not the identity and 15 tiles (fewer than one wavefront's lanes).
    30 levels take the orders of the guesses, the adjoint sweep's included, up to their maximum."""
    return _case(V, O2, 128, 64, 30, (0.1, 0.6, 0.05), (3.0, -2.0, 0.5))


@pytest.mark.parametrize("other", [{}, {"VCH_NO_SPEC": "1"}, {"VCH_CHEB": "0"}, {"VCH_CEIL_CELL": "0"}, {"VCH_FUSED": "0"}],
                         ids=["default", "no_spec", "cheb_0", "ceil_cell_0", "fused_0"])
def test_march_with_sliver_tiles(V, uneven, other):
    """Two marches on one engine in either form.  VCH_NO_SPEC=1: a look after every phase (k_publish_state);
    VCH_CHEB=0: the CG form (cg_sums3, k_cg_finish, k_fin_residual behind a CG solve); VCH_CEIL_CELL=0: k_fin_ceiling closes the reduction-free solves (the
    arm of k_fin_residual<1> without a cell); VCH_FUSED=0: the unfused kernels and k_fin_residual<0>."""
    new, _ = _run(V, other, uneven)
    old, _ = _run(V, {**other, **PLAIN}, uneven)
    st = new[0][1]
    print(other, "stats", st, "shifts of trajectory 0, first steps", new[0][2][0][:3])
    assert np.abs(new[0][2]).max() > 0                        # the mass fix is not the identity here
    for a, b in zip(new, old):
        _same(a, b)


_sweeps = {}


def _sweep(V, uneven, other, plain):
    key = (tuple(sorted(other.items())), plain)
    if key not in _sweeps:
        _sweeps[key] = _run(V, {**other, **(PLAIN if plain else {})}, uneven, n=1, adjoint=True)[1]
    return _sweeps[key]


@pytest.mark.parametrize("other", [{}, {"VCH_ADJ_GUESS_OFF": "1"}, {"VCH_ADJ_SAFE": "1"}], ids=["default", "guess_off", "safe"])
def test_adjoint_sweep_with_sliver_tiles(V, uneven, other):
    """Engine2D.backward on the marched history with phi_Q and phi_T set, in either form: r, p, q and the stats."""
    new, old = _sweep(V, uneven, other, False), _sweep(V, uneven, other, True)
    print(other, "stats", new[3])
    _same_adjoint(new, old)


def test_adjoint_sweep_used_a_guess(V, uneven):
    """The default sweep really extrapolated (a guess of order > 1 is what saves iterations): with VCH_ADJ_GUESS_OFF=1 the
    solves need more of them."""
    on, off = _sweep(V, uneven, {}, False), _sweep(V, uneven, {"VCH_ADJ_GUESS_OFF": "1"}, False)
    print("linear iterations with the guess", on[3]["linear_iters"], "without", off[3]["linear_iters"])
    assert off[3]["linear_iters"] > on[3]["linear_iters"], (on[3], off[3])


# ------------------------------------------------------------------------------------------------------------------
# B. tile counts
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nx,Ny,M", [(256, 256, 4), (256, 1024, 3), (14, 11, 6)], ids=["85_tiles", "325_tiles", "gemm_14x11"])
def test_tile_counts(V, O2, Nx, Ny, M):
    """One march, batch 2, whose second trajectory starts almost flat and ends its Newton loops early.  256 x 256: 5 x 17 = 85
    tiles, more than one round of the 64 lanes and fewer than 64 * FIN_PU; 256 x 1024: 257 x 1025 nodes in 5 x 65 = 325 tiles,
    the smallest grid of the FFT path beyond 64 * FIN_PU = 320, so the rolled tail of fin_reduce runs; 14 x 11: the GEMM path
    (k_schur_p, the k_fin_cg_* kernels)."""
    c = _case(V, O2, Nx, Ny, M, (0.5, 0.01))
    new, _ = _run(V, {}, c, n=1)
    old, _ = _run(V, PLAIN, c, n=1)
    print((Nx, Ny), "stats", new[0][1])
    _same(new[0], old[0])


# ------------------------------------------------------------------------------------------------------------------
# C. the PGD loop with backtracking
# ------------------------------------------------------------------------------------------------------------------
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


# ------------------------------------------------------------------------------------------------------------------
# D. batch independence
# ------------------------------------------------------------------------------------------------------------------
def test_batch_equals_single(V, O2):
    """64 x 64, 20 steps and the adjoint sweep, in the new form: trajectory 0 of a batch of 3 equals its run alone."""
    c = _case(V, O2, 64, 64, 20, (0.1, 0.5, 0.02), seed=11)
    (m3,), a3 = _run(V, {}, c, n=1, adjoint=True)
    (m1,), a1 = _run(V, {}, c, n=1, adjoint=True, nb=1)
    ph3 = m3[0].reshape((3,) + m3[0].shape[-3:])
    ph1 = m1[0].reshape((1,) + m1[0].shape[-3:])
    assert np.array_equal(ph3[0], ph1[0]), float(np.max(np.abs(ph3[0] - ph1[0])))
    assert np.array_equal(m3[2][0], m1[2][0])
    for name, x3, x1 in zip("pqr", a3[:3], a1[:3]):
        x3 = x3.reshape((3,) + x3.shape[-3:])
        x1 = x1.reshape((1,) + x1.shape[-3:])
        assert np.abs(x1).max() > 0, name
        assert np.array_equal(x3[0], x1[0]), (name, float(np.max(np.abs(x3[0] - x1[0]))))
