"""Host-side mirror of the reusable parts of src/2D/Vch_control_2D/GD2_configured.py: target
construction (G2:149-228), the backtracking line search (G2:71-146) and the optimisation loop
of the `__main__` block (G2:291-382) as a callable that runs device-resident
(vch2d_pgd_init / vch2d_pgd_iterate).  Prompts, previews and plots are out of scope."""
from __future__ import annotations

import contextlib
import io
import time
from typing import Tuple

import numpy as np

from ..engine import make_opt, time_grid
from ._ctx import engine_for_config
from .Forward2_solver import run_main_simulation, init_phi_random, DELTA_SEP
from .backward2_solver import run_backward                                   # noqa: F401
from .cost2_and_function import calculate_cost, calculate_gradient, proximal_step   # noqa: F401
from .config import ForwardSolverConfig, OptimizationConfig, load_params, save_params

INTERACTIVE = False
DEFAULT_TARGET_CHOICE = 1
DEFAULT_TRACKING_CHOICE = 1


def build_targets(x, y, t_hist, phi_initial, Lx, Ly, T, interactive=False, choice_t=1, choice_q=1):
    """phi_T: 0.7 sin(2 pi x/Lx) cos(pi y/Ly) or a centred disc; phi_Q: ramp with the CONFIG T or
    zeros (G2:184-226)."""
    xx, yy = np.meshgrid(x, y, indexing="ij")
    if choice_t == 1:
        phi_T = 0.7 * np.sin(2 * np.pi * xx / Lx) * np.cos(np.pi * yy / Ly)
    else:
        phi_T = -np.ones_like(xx)
        phi_T[(xx - Lx / 2) ** 2 + (yy - Ly / 2) ** 2 < (Lx / 3.5) ** 2] = 1.0
    if choice_q == 1:
        tp = (t_hist / T)[:, np.newaxis, np.newaxis]
        phi_Q = (1 - tp) * phi_initial + tp * phi_T
    else:
        phi_Q = np.zeros((len(t_hist), len(x), len(y)))
    return phi_T, phi_Q


def perform_backtracking_line_search_2D(u_k, cost_k, grad_smooth, phi_Q_target, phi_T_target, x, y, fwd_config,
                                        opt_config, alpha_init: float = 1.0, beta: float = 0.8,
                                        max_ls_iter: int = 10) -> Tuple:
    """G2:71-146 through the function-level mirrors (each call one engine invocation)."""
    alpha, attempts = alpha_init, 0
    u_next, phi_next, t_next, cost_next = u_k, None, None, cost_k
    t0 = time.perf_counter()
    for _ in range(max_ls_iter):
        attempts += 1
        u_next = proximal_step(u_k, grad_smooth, alpha, opt_config)
        phi_next, _, t_next = run_main_simulation(config=fwd_config, store_history=True, control_input=u_next, verbose=False)
        with contextlib.redirect_stdout(io.StringIO()):
            cost_next = calculate_cost(phi_next, u_next, phi_Q_target, phi_T_target, x, y, t_next, opt_config)
        if cost_next < cost_k:
            return alpha, u_next, cost_next, phi_next, t_next, time.perf_counter() - t0, attempts
        alpha *= beta
    return alpha, u_next, cost_next, phi_next, t_next, time.perf_counter() - t0, attempts


def run_optimization(fwd_config: ForwardSolverConfig, opt_config: OptimizationConfig, n_iter=None, seeds=(42,),
                     choice_t=DEFAULT_TARGET_CHOICE, choice_q=DEFAULT_TRACKING_CHOICE, amp=0.1, device=0, sparsity=None):
    """The PGD loop of G2:291-382 for a batch of initial conditions (`seeds`), device-resident.
    `sparsity`: a name of Engine2D.SPARSITY for the batch or one per seed (directional sparsity); None is the
    reference's functional through the calls of before.
    Returns dict(costs [B][it+1], alphas, attempts, changes, tracking_error, terminal_error (the two relative
    error histories the driver appends per iteration, G2:336-363, from the cost kernel's sums), u, phi, r, seconds)."""
    Nx, Ny = int(fwd_config.Nx), int(fwd_config.Ny)
    t_hist, dts = time_grid(float(fwd_config.T), float(fwd_config.dt_initial))
    B = len(seeds)
    eng = engine_for_config(fwd_config, batch=B, max_steps=len(dts), device=device)
    phi0 = np.stack([init_phi_random(Nx, Ny, DELTA_SEP, amp=amp, seed=int(s)) for s in seeds])
    phi_T, _ = build_targets(eng.x, eng.y, t_hist, phi0[0], fwd_config.Lx, fwd_config.Ly, fwd_config.T,
                             choice_t=choice_t, choice_q=2)
    phi_Tb = np.broadcast_to(phi_T, phi0.shape).copy()
    J0 = eng.pgd_init(phi0, phi_Tb, t_hist, make_opt(opt_config), ramp=(choice_q == 1), T=float(fwd_config.T), sparsity=sparsity)
    n = int(opt_config.max_iter if n_iter is None else n_iter)
    res = eng.pgd_iterate(n)
    costs = np.concatenate([J0[:, 4:5], res["cost"]], axis=1)
    return dict(costs=costs, alphas=res["alpha"], attempts=res["attempts"], changes=res["change"],
                tracking_error=res["tracking_error"], terminal_error=res["terminal_error"], iters=res["iters"], seconds=res["seconds"], u=eng.pgd_get("u"), phi=eng.pgd_get("phi"),
                r=eng.pgd_get("r"), phi_T=phi_T, t_hist=t_hist, x=eng.x.copy(), y=eng.y.copy())


def run_sweep(fwd_config: ForwardSolverConfig, opt_configs, n_iter=None, seed=42, amp=0.1, choice_t=DEFAULT_TARGET_CHOICE,
              choice_q=DEFAULT_TRACKING_CHOICE, u0=None, return_controls=False, device=0, n_newton=0, n_trust=0, radius0=1.0,
              sparsity=None):
    """A parameter sweep as ONE batch: member b runs the PGD loop with opt_configs[b] (weights, sparsity parameter, box,
    alpha_max), all members from the same initial state (`seed`, `amp`) and targets, so that they differ by their
    parameters only.  `u0`: start control, one (M+1, Nx+1, Ny+1) array for every member or one per member (continuation
    in kappa_sparsity, resuming from a saved optimal_control.npy); default zeros.  `n_iter` None: the largest max_iter of
    the members (the loop length is one for the batch).  Returns dict(costs [B][it+1], alphas, attempts, changes,
    tracking_error, terminal_error, iters, seconds, kkt = Engine2D.pgd_kkt(refresh=True) -- the sparsity statistic and
    the stationarity measure of every member, counted on the device -- t_hist, x, y, and u only with return_controls);
    the state history never leaves the device.  `n_newton` > 0 polishes every member after its PGD iterations by that many
    damped Newton rounds on its free set (Engine2D.pgd_newton, on the device) and adds `newton` (its records) and
    `costs_newton` [B][n_newton+1] (the cost before the first round, then after every round); kkt and u are then those of
    the polished iterate.  0 leaves the result as it is without the polish.  `n_trust` > 0 does the same (after the Newton
    rounds, if both are asked for) with that many trust-region rounds from the radius `radius0` (Engine2D.pgd_trust), which
    follow a direction of non-positive curvature instead of ending on it, and adds `trust` and `costs_trust` [B][n_trust+1].
    `sparsity`: a name of Engine2D.SPARSITY for the batch or one per member (None: every member "full", the calls of before);
    kkt then counts a group-mode member's groups.  The Newton and trust-region rounds are those of the L1 functional: with a
    member in a group mode n_newton > 0 or n_trust > 0 raises the engine's error."""
    opt_configs = list(opt_configs)
    B = len(opt_configs)
    if B < 1:
        raise ValueError("run_sweep needs at least one OptimizationConfig")
    Nx, Ny = int(fwd_config.Nx), int(fwd_config.Ny)
    t_hist, dts = time_grid(float(fwd_config.T), float(fwd_config.dt_initial))
    eng = engine_for_config(fwd_config, batch=B, max_steps=len(dts), device=device)
    phi0 = np.repeat(init_phi_random(Nx, Ny, DELTA_SEP, amp=amp, seed=int(seed))[None], B, axis=0)
    phi_T, _ = build_targets(eng.x, eng.y, t_hist, phi0[0], fwd_config.Lx, fwd_config.Ly, fwd_config.T,
                             choice_t=choice_t, choice_q=2)
    if u0 is not None:
        u0 = np.asarray(u0, dtype=np.float64)
        if u0.ndim == 3:
            u0 = np.repeat(u0[None], B, axis=0)
    J0 = eng.pgd_init(phi0, np.repeat(phi_T[None], B, axis=0), t_hist, [make_opt(o) for o in opt_configs],
                      ramp=(choice_q == 1), T=float(fwd_config.T), u0=u0, sparsity=sparsity)
    n = int(max(int(o.max_iter) for o in opt_configs) if n_iter is None else n_iter)
    res = eng.pgd_iterate(n)
    newton = eng.pgd_newton(int(n_newton)) if int(n_newton) > 0 else None
    trust = eng.pgd_trust(int(n_trust), radius0) if int(n_trust) > 0 else None
    out = dict(costs=np.concatenate([J0[:, 4:5], res["cost"]], axis=1), alphas=res["alpha"], attempts=res["attempts"],
               changes=res["change"], tracking_error=res["tracking_error"], terminal_error=res["terminal_error"],
               iters=res["iters"], seconds=res["seconds"], kkt=eng.pgd_kkt(refresh=True), phi_T=phi_T, t_hist=t_hist,
               x=eng.x.copy(), y=eng.y.copy())
    for name, rec in (("newton", newton), ("trust", trust)):
        if rec is None:
            continue
        # an idle round carries the cost the member ended with
        cn = np.concatenate([rec["cost"][:, :1], rec["cost_new"]], axis=1)
        for r in range(1, cn.shape[1]):
            cn[:, r] = np.where(np.isnan(cn[:, r]), cn[:, r - 1], cn[:, r])
        out[name], out["costs_" + name] = rec, cn
    if return_controls:
        out["u"] = eng.pgd_get("u").reshape((B, len(t_hist)) + eng.shape)
    return out


def newton_refine(fwd_config: ForwardSolverConfig, opt_config: OptimizationConfig, u, phi_Q_target, phi_T_target,
                  n_newton=3, k=50, cg_tol=1e-8, max_halvings=10, on_device=False):
    """Rounds of a damped Newton method on the free set, from the control `u` (for instance what the PGD loop left).
    Per round: the free set of the iterate (strictly inside the box of `opt_config`, off the kink of the L1 term) and
    the Newton step d of the full cost on it (second_order_conditions_2d.reduced_newton_step_2d: conjugate gradients on
    the device, at most `k` steps to `cg_tol`).  Trials are clip(u + s d, box) for s = 1, 1/2, ..., at most `max_halvings`
    halvings; a free node whose sign the trial flips is set to 0, the kink, where the next round pins it.  The first s
    with J(trial) <= J(u) - 1e-4 s pred is accepted, J the full cost of a march of the trial (Engine2D.forward and
    Engine2D.cost) and pred the decrease the quadratic model predicts for the full step.  The loop ends after `n_newton`
    rounds, when the right-hand side vanishes (stationarity on the free set), when the first CG direction already has
    non-positive curvature, or when no s is accepted.

    Returns (u, records): the final control and one dict per round with cost (before the round), n_free, rnorm0, steps,
    status, s (None when the round moved nothing) and cost_new (the accepted trial's, else the unchanged cost).

    on_device=True runs the rounds on the device (Engine2D.pgd_newton): one context, one pgd_init(u0=u), the step, the
    trials and the decisions without a history crossing the bus; the records have the same keys.  One departure: a CG
    breakdown ends the rounds there (no march under a control that may not be finite), where the host loop tries the step."""
    if on_device:
        return _newton_refine_device(fwd_config, opt_config, u, phi_Q_target, phi_T_target, n_newton, k, cg_tol, max_halvings)
    from .second_order_conditions_2d import free_set, reduced_newton_step_2d
    Nx, Ny = int(fwd_config.Nx), int(fwd_config.Ny)
    t_hist, dts = time_grid(float(fwd_config.T), float(fwd_config.dt_initial))
    M = len(dts)
    lo, hi = float(opt_config.u_min), float(opt_config.u_max)
    u = np.asarray(u, dtype=np.float64)[:M + 1]                     # nodes outside the box are not free: the first trial clips them
    phi0 = init_phi_random(Nx, Ny, DELTA_SEP, amp=0.1, seed=42)
    x, y = np.linspace(0.0, fwd_config.Lx, Nx + 1), np.linspace(0.0, fwd_config.Ly, Ny + 1)
    pq, pt = np.asarray(phi_Q_target)[None, :M + 1], np.asarray(phi_T_target)[None]

    def full_cost(v):
        eng = engine_for_config(fwd_config, batch=1, max_steps=max(M, 1))
        phi, _ = eng.forward(phi0[None], dts, u=v[None], store=True)
        J = eng.cost(phi.reshape((1, M + 1, Nx + 1, Ny + 1)), v[None], pq, pt, t_hist, opt_config, x, y)
        return float(np.atleast_2d(J)[0, 4])

    cost = full_cost(u)
    records = []
    for _ in range(int(n_newton)):
        N = reduced_newton_step_2d(u, x, y, t_hist, opt_config, phi_Q_target=phi_Q_target, phi_T_target=phi_T_target,
                                   u_min=lo, u_max=hi, k=k, cg_tol=cg_tol, fwd_config=fwd_config)
        rec = dict(cost=cost, n_free=N["n_free"], rnorm0=N["rnorm0"], steps=N["steps"], status=N["status"], s=None, cost_new=cost)
        records.append(rec)
        if N["rnorm0"] == 0.0 or (N["status"] == "negcurv" and N["steps"] == 0):
            break
        d, free, s = N["d"], free_set(u, lo, hi), 1.0
        for _ in range(int(max_halvings) + 1):
            trial = np.clip(u + s * d, lo, hi)
            trial[free & (trial * u < 0.0)] = 0.0
            J = full_cost(trial)
            if J <= cost - 1e-4 * s * N["pred"]:
                rec["s"], rec["cost_new"] = s, J
                break
            s *= 0.5
        if rec["s"] is None:
            break
        u, cost = trial, J
    return u, records


def _newton_refine_device(fwd_config, opt_config, u, phi_Q_target, phi_T_target, n_newton, k, cg_tol, max_halvings):
    """newton_refine(on_device=True): the problem of the host loop as a resident PGD problem, then Engine2D.pgd_newton."""
    from ..engine import Engine2D
    Nx, Ny = int(fwd_config.Nx), int(fwd_config.Ny)
    t_hist, dts = time_grid(float(fwd_config.T), float(fwd_config.dt_initial))
    M = len(dts)
    u = np.asarray(u, dtype=np.float64)[:M + 1]
    phi0 = init_phi_random(Nx, Ny, DELTA_SEP, amp=0.1, seed=42)
    x, y = np.linspace(0.0, fwd_config.Lx, Nx + 1), np.linspace(0.0, fwd_config.Ly, Ny + 1)
    eng = engine_for_config(fwd_config, batch=1, max_steps=max(M, 1))
    eng.pgd_init(phi0[None], np.asarray(phi_T_target)[None], t_hist, [make_opt(opt_config)],
                 phi_Q=np.asarray(phi_Q_target)[None, :M + 1], ramp=False, x=x, y=y, u0=u[None])
    R = eng.pgd_newton(int(n_newton), k=k, cg_tol=cg_tol, max_halvings=max_halvings)
    records = []
    for r in range(int(R["rounds"])):
        if Engine2D.NEWTON_STATUS[int(R["status"][0, r])] == "idle":
            break
        s = float(R["s"][0, r])
        records.append(dict(cost=float(R["cost"][0, r]), n_free=int(R["n_free"][0, r]), rnorm0=float(R["rnorm0"][0, r]),
                            steps=int(R["cg_steps"][0, r]), status=Engine2D.CG_STATUS[int(R["cg_status"][0, r])],
                            s=None if np.isnan(s) else s, cost_new=float(R["cost_new"][0, r])))
    return eng.pgd_get("u"), records


def trust_refine(fwd_config: ForwardSolverConfig, opt_config: OptimizationConfig, u, phi_Q_target, phi_T_target,
                 n_trust=3, radius0=1.0, k=50, cg_tol=1e-8, radius_max=None, radius_min=None, on_device=False):
    """Rounds of a trust-region Newton method on the free set, from the control `u`: newton_refine with the damping
    replaced by a radius.  Per round: the Steihaug step x of the full cost on the free set of the iterate inside
    ||x||_D <= radius (Engine2D.hess_cg_trust: a direction of non-positive curvature is followed to the boundary instead
    of ending the loop), one trial clip(u + x, box) with a flipped sign set to 0 (Engine2D.newton_trial(1)), its march
    from the start state of newton_refine and its cost J(t); rho = (J(u) - J(t)) / pred.  The trial is accepted iff J(t) is
    finite and J(t) <= J(u) - 1e-4 pred, else the iterate stays ("rejected") and the loop goes on.  The radius: rho < 1/4
    or not finite: min(radius, ||x||_D) / 4; else rho > 3/4 after a "boundary" or "negcurv" exit: min(2 radius,
    radius_max).  The loop ends after `n_trust` rounds, on a vanishing right-hand side ("stationary"), a CG breakdown, or
    once the radius is below radius_min ("stalled" when that round was rejected).  radius_max / radius_min default to
    1024 radius0 and 1e-10 radius0.

    Returns (u, records): one dict per round with cost, cost_new, pred, rnorm0, radius (the round's), ratio, xnorm,
    steps, cg_status (a name of Engine2D.TRUST_CG_STATUS), status (a name of Engine2D.TRUST_STATUS), n_free.

    on_device=True runs the rounds on the device (Engine2D.pgd_trust): one context, one pgd_init(u0=u) with this loop's
    own start state and targets; the records have the same keys."""
    from ..engine import Engine2D
    Nx, Ny = int(fwd_config.Nx), int(fwd_config.Ny)
    t_hist, dts = time_grid(float(fwd_config.T), float(fwd_config.dt_initial))
    M = len(dts)
    u = np.asarray(u, dtype=np.float64)[:M + 1]
    radius = float(radius0)
    radius_max = 1024.0 * radius if radius_max is None else float(radius_max)
    radius_min = 1e-10 * radius if radius_min is None else float(radius_min)
    phi0 = init_phi_random(Nx, Ny, DELTA_SEP, amp=0.1, seed=42)
    x, y = np.linspace(0.0, fwd_config.Lx, Nx + 1), np.linspace(0.0, fwd_config.Ly, Ny + 1)
    pq, pt = np.asarray(phi_Q_target, dtype=np.float64)[None, :M + 1], np.asarray(phi_T_target, dtype=np.float64)[None]
    opt = make_opt(opt_config)
    eng = engine_for_config(fwd_config, batch=1, max_steps=max(M, 1))
    CGS, NTS = Engine2D.TRUST_CG_STATUS, Engine2D.TRUST_STATUS
    if on_device:
        eng.pgd_init(phi0[None], pt, t_hist, [opt], phi_Q=pq, ramp=False, x=x, y=y, u0=u[None])
        R = eng.pgd_trust(int(n_trust), radius, k=k, cg_tol=cg_tol, radius_max=radius_max, radius_min=radius_min)
        records = []
        for r in range(int(R["rounds"])):
            if NTS[int(R["status"][0, r])] == "idle":
                break
            records.append(dict(cost=float(R["cost"][0, r]), cost_new=float(R["cost_new"][0, r]), pred=float(R["pred"][0, r]),
                                rnorm0=float(R["rnorm0"][0, r]), radius=float(R["radius"][0, r]), ratio=float(R["ratio"][0, r]),
                                xnorm=float(R["xnorm"][0, r]), steps=int(R["cg_steps"][0, r]),
                                cg_status=CGS[int(R["cg_status"][0, r])], status=NTS[int(R["status"][0, r])],
                                n_free=int(R["n_free"][0, r])))
        return eng.pgd_get("u").reshape((M + 1, Nx + 1, Ny + 1)), records

    def full_cost(v):
        phi, _ = eng.forward(phi0[None], dts, u=np.ascontiguousarray(v[None]), store=True)
        J = eng.cost(phi.reshape((1, M + 1, Nx + 1, Ny + 1)), v[None], pq, pt, t_hist, opt_config, x, y)
        return float(np.atleast_2d(J)[0, 4])

    cost = full_cost(u)
    records = []
    for _ in range(int(n_trust)):
        eng.forward(phi0[None], dts, u=np.ascontiguousarray(u[None]), store=False)
        S = eng.hess_cg_trust(int(k), radius, cg_tol=cg_tol, tol=1e-8, dt=dts, t_hist=t_hist, opt=opt, phi_Q=pq, phi_T=pt, x=x, y=y)
        st = int(S["status"][0])
        rec = dict(cost=cost, cost_new=cost, pred=float(S["pred"][0]), rnorm0=float(S["rnorm0"][0]), radius=radius,
                   ratio=float("nan"), xnorm=float(S["xnorm"][0]), steps=int(S["steps"][0]), cg_status=CGS[st], status="stationary",
                   n_free=int(S["n_free"][0]))
        records.append(rec)
        if rec["n_free"] < 1 or rec["rnorm0"] == 0.0:
            break
        if CGS[st] == "breakdown":
            rec["status"] = "breakdown"
            break
        trial = eng.newton_trial(1.0)["u"][0]
        J = full_cost(trial)
        with np.errstate(all="ignore"):
            rho = rec["ratio"] = float((np.float64(cost) - np.float64(J)) / np.float64(rec["pred"]))
        accept = bool(np.isfinite(J)) and J <= cost - 1e-4 * rec["pred"]
        if not np.isfinite(rho) or rho < 0.25:
            radius = 0.25 * min(radius, rec["xnorm"])
        elif rho > 0.75 and CGS[st] in ("boundary", "negcurv"):
            radius = min(2.0 * radius, radius_max)
        small = radius < radius_min
        rec["status"] = "accepted" if accept else ("stalled" if small else "rejected")
        if accept:
            u, cost, rec["cost_new"] = trial, J, J
        if small:
            break
    return u, records


def main(n_iter=None, params_file="last_run_config_2d.json", num_directions=5, verbose=True):
    """Non-interactive equivalent of the reference's `__main__` block (G2:230-441) without previews and
    plots: parameters from the last-run JSON (defaults if absent, K2:181-190), uncontrolled march, targets
    (choice 1/1), the PGD loop (device-resident), the time-study summary (G2:403-416), the final adjoint,
    the coercivity finite-difference test and the sparsity statistic (G2:424-437), `save_params`
    (G2:440).  Returns the run_optimization dict extended by `hessian_values` and `sparsity`."""
    from .second_order_conditions_2d import approximate_second_order_condition_2d, verify_sparsity_condition
    say = print if verbose else (lambda *a, **k: None)
    allp = load_params(params_file)
    fwd, opt = allp.forward_solver, allp.optimization
    say("=" * 60 + "\n    2D GRADIENT DESCENT OPTIMIZATION \n" + "=" * 60)
    say("Forward Solver Config:\n" + fwd.model_dump_json(indent=2) + "\nOptimization Config:\n" + opt.model_dump_json(indent=2))
    t0 = time.time()
    res = run_optimization(fwd, opt, n_iter=n_iter)
    B = res["costs"].shape[0]
    assert B == 1
    costs = res["costs"][0]
    it = int(res["iters"])
    say(f"Completed Iterations: {it}\nFinal Cost: {costs[it]:.5f}\nCost Reduction: {100 * (1 - costs[it] / costs[0]):.2f}%")
    if it > 0:
        say(f"Relative tracking error: {res['tracking_error'][0, it - 1]:.6e}   "
            f"relative terminal error: {res['terminal_error'][0, it - 1]:.6e}")
    sec = res["seconds"]
    say("\n" + "=" * 50 + "\n  TIME STUDY SUMMARY\n" + "=" * 50)
    say(f"Total backward-solve time:        {sec['backward']:.3f}s")
    say(f"Total optimistic forward time:    {sec['optimistic_forward']:.3f}s")
    say(f"Total optimistic cost time:       {sec['cost']:.3f}s")
    say(f"Total backtracking time:          {sec['backtracking']:.3f}s  (attempts={int(res['attempts'].sum())})")
    ok = res["attempts"][0, :it] == 0
    if ok.any():
        say(f"ALPHA ADVISOR: a good initial alpha_max for the next run is {float(np.mean(res['alphas'][0, :it][ok])):.4f}")
    x, y, t_hist = res["x"], res["y"], res["t_hist"]
    phi_T, phi_Q = build_targets(x, y, t_hist, res["phi"][0], fwd.Lx, fwd.Ly, fwd.T, choice_t=DEFAULT_TARGET_CHOICE,
                                 choice_q=DEFAULT_TRACKING_CHOICE)
    out = dict(res, hessian_values=None, sparsity=None, runtime_s=None)
    try:
        _, _, r_opt = run_backward(res["phi"], x, y, t_hist, fwd, opt.b1, opt.b2, phi_Q, phi_T)
        sink = contextlib.nullcontext() if verbose else contextlib.redirect_stdout(io.StringIO())
        with sink:
            hv = approximate_second_order_condition_2d(
                u_star=res["u"], r_star=r_opt, phi_star=res["phi"], x=x, y=y, t_hist=t_hist, b1=opt.b1, b2=opt.b2, b3=opt.b3,
                kappa=opt.kappa_sparsity, phi_Q_target=phi_Q, phi_T_target=phi_T, u_min=opt.u_min, u_max=opt.u_max,
                num_directions=num_directions, epsilon=1e-4, seed=42, fwd_config=fwd)
            say("Coercivity condition appears to hold in tested directions." if all(v > 0 for v in hv)
                else "Coercivity condition may fail; non-positive second derivatives found.")
            out["sparsity"] = verify_sparsity_condition(res["u"], r_opt, opt.kappa_sparsity)
        out["hessian_values"] = hv
    except Exception as e:          # G2:438-439
        say(f"[Warning] Could not perform final analysis (second-order/sparsity): {e}")
    save_params(fwd, opt, it, params_file)
    out["runtime_s"] = time.time() - t0
    return out

