#!/usr/bin/env python3
"""Golden vectors of the 1D reference away from its default parameters: g1d_off_33.npz and g1d_off2_33.npz.

TEST INFRASTRUCTURE, same rules as make_golden.py: runs only where the reference checkout is mounted read-only, imports
the reference's modules (never copies them), calls them on the inputs of tests/_offpoint_1d.py and stores inputs and
outputs as .npz data.  One fixture per parameter point (OFF, OFF2 of tests/_offpoint_1d.py) at N = 33, T = 0.045,
dt = 0.01 (five steps, the last one ragged), a few tens of kB each:

    operators        Lv, mu0, Rphi, Rmu, J^-1 d, fpp, A^-1 v, (I - tau L)^-1 v on seeded vectors (as g1d_ops_24.npz)
    march            the reference's history from the smooth start without control, with the amplitude-12 control, and with
                     the control cut to M rows (hold-last branch F1:351-353); from the near-separated start without and
                     with control
    adjoint, cost    p, q, r of run_backward on the controlled history with build_targets_1d's targets and without
                     targets; calculate_cost, calculate_gradient and the prox step
    free energy      F1.free_energy of every row of the controlled history: plain, with a w history, with eps given
    Newton           one newton_raphson call of the capped-step window: norm history and result

Usage:  python tests/golden/make_golden_1d_off.py
"""
import contextlib
import importlib
import io
import os
import sys
import tempfile

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF1D = "/root/reference/src/1D/Vch_control_1D"
DELTA_SEP = 1e-2


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def save(name, **arrs):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrs)
    print(f"  wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB")


def gen(point, tag, newton_seed):
    import _offpoint_1d as X
    with quiet():
        F1, B1, C1, K1, G1 = (importlib.import_module(n) for n in
                              ("Forward_solver", "backward_solver", "cost_and_function", "config", "GD_1D"))
    N = 33
    P = X.params(point, N)
    # model_construct: K1's validator wants c2 > c1, which OFF (c2 0.5, c1 0.9) breaks on purpose -- the solver functions
    # take any values, and a slip between c1 and c2 shows only where they are far apart in this order too
    cfg = K1.ForwardSolverConfig.model_construct(N=N, Lx=P.Lx, T=P.T, dt_initial=P.dt_initial, tau=P.tau, gamma=P.gamma,
                                                 c1=P.c1, c2=P.c2, kappa=P.kappa)
    h = P.Lx / N
    n = N + 1
    out = dict(N=N, Lx=P.Lx, T=P.T, dt=P.dt_initial, tau=P.tau, gamma=P.gamma, c1=P.c1, c2=P.c2, kappa=P.kappa)

    # ---- operators on seeded vectors, two nodes beyond the clips ------------------------------------------------------
    rng = np.random.default_rng(4321 + len(tag))
    L = F1.laplacian_matrix_neumann(N, h)
    v = rng.standard_normal(n)
    phi_new, phi_old = rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n)
    phi_new[3] = 0.9991
    phi_old[5] = -0.9999999995
    mu_new, mu_old, w_new, w_old = (rng.standard_normal(n) for _ in range(4))
    dvec = rng.standard_normal(2 * n)
    dt = 1e-2
    J = F1.assemble_jacobian(phi_new, dt, P.tau, P.c1, L, P.kappa)
    I = np.eye(n)
    A = I - B1.tau * L + 0.5 * dt * (L @ L) - 0.5 * dt * (np.diag(B1.fpp_log(phi_new)) @ L)          # B1:101
    out.update(v=v, phi_new=phi_new, phi_old=phi_old, mu_new=mu_new, mu_old=mu_old, w_new=w_new, w_old=w_old, dvec=dvec,
               Lv=F1.apply_laplacian(L, v), mu0=F1.initialize_mu(phi_old, w_new, P.c1, P.c2, L, P.kappa),
               Rphi=F1.solve_phi_residual(phi_new, phi_old, mu_new, mu_old, w_new, w_old, dt, P.tau, P.c1, P.c2, L, P.kappa),
               Rmu=F1.solve_mu_residual(phi_new, phi_old, mu_new, mu_old, dt, L),
               Jsol=np.linalg.solve(J, dvec), fpp=B1.fpp_log(phi_old), Asol=np.linalg.solve(A, v),
               ATsol=np.linalg.solve(I - B1.tau * L, v),
               w_filt=F1.solve_w(w_old, dt, P.gamma, w_new, v))

    # ---- marches ------------------------------------------------------------------------------------------------------
    u = X.control(P, 12.0)

    def run(kind, ctl):
        with quiet():
            ph, x, t = F1.run_main_simulation(cfg, store_history=True, control_input=ctl, verbose=False,
                                              initial_phi=X.start(P, kind))
        return ph, x, t

    phi_nat, x, t_hist = run("smooth", None)
    phi_u = run("smooth", u)[0]
    out.update(x=x, t_hist=t_hist, u=u, phi0=X.start(P, "smooth"), phi0_sep=X.start(P, "sep"), phi_nat=phi_nat,
               phi_u=phi_u, phi_ushort=run("smooth", u[:X.M])[0], phi_sep_nat=run("sep", None)[0],
               phi_sep_u=run("sep", u)[0])

    # ---- adjoint sweep, cost, gradient, prox --------------------------------------------------------------------------
    o = X.PGD_OPT
    with quiet():
        phi_T, phi_Q = G1.build_targets_1d(x, t_hist, phi_nat[0].copy(), cfg.Lx, cfg.T, interactive=False, choice_t=1,
                                           choice_q=1)
        p, q, r = B1.run_backward(phi_u, x, t_hist, o["b1"], o["b2"], phi_Q, phi_T)
        p0, q0, r0 = B1.run_backward(phi_u, x, t_hist, 1.3, 0.7, None, None)
        uc = u / 20.0              # |u| up to 0.6: the prox step below ends inside the box, on both faces and at zero
        Jv = C1.calculate_cost(phi_u, uc, phi_Q, phi_T, x, t_hist, o["b1"], o["b2"], o["b3"], o["kappa_sparsity"],
                               verbose=False)
    g = C1.calculate_gradient(r, uc, o["b3"])
    a = 7.0
    out.update(phi_T=phi_T, phi_Q=phi_Q, p=p, q=q, r=r, p_none=p0, q_none=q0, r_none=r0, u_cost=uc, J=Jv, grad=g,
               prox=G1.perform_proximal_and_projection(C1.perform_gradient_step(uc, g, a), a, o["kappa_sparsity"],
                                                       o["u_min"], o["u_max"]), prox_alpha=a)

    # ---- free energy of every row -------------------------------------------------------------------------------------
    w_hist = u / 12.0
    out.update(w_hist=w_hist,
               E=np.array([F1.free_energy(ph, P.kappa, P.c1, P.c2, h) for ph in phi_u]),
               E_w=np.array([F1.free_energy(ph, P.kappa, P.c1, P.c2, h, w=w) for ph, w in zip(phi_u, w_hist)]),
               E_sep_eps=np.array([F1.free_energy(ph, P.kappa, P.c1, P.c2, h, eps=0.5 * DELTA_SEP)
                                   for ph in out["phi_sep_u"]]))

    # ---- one Newton call of the capped-step window --------------------------------------------------------------------
    c = X.capped_case(point, N, newton_seed)
    pn, mn, hist = F1.newton_raphson(c["phi"], c["mu"], c["w_old"], c["w_new"], c["dt"], P.tau, P.c1, P.c2, h, DELTA_SEP,
                                     L, P.kappa, return_residual_history=True)
    out.update(nr_seed=newton_seed, nr_phi=c["phi"], nr_mu=F1.initialize_mu(c["phi"], 0.0, P.c1, P.c2, L, P.kappa),
               nr_w_old=c["w_old"], nr_w_new=c["w_new"], nr_dt=c["dt"], nr_phi_new=pn, nr_mu_new=mn,
               nr_hist=np.array(hist))
    save(f"g1d_{tag}_33.npz", **out)


if __name__ == "__main__":
    if not os.path.isdir(REF1D):
        sys.exit("reference checkout not present: golden vectors can only be regenerated in the build container")
    sys.path[:0] = [REF1D, ROOT, os.path.join(ROOT, "tests")]
    os.chdir(tempfile.mkdtemp(prefix="vch_golden_"))
    import warnings
    warnings.filterwarnings("ignore")
    print("1D off-default goldens")
    gen("off", "off", 2)
    gen("off2", "off2", 3)
