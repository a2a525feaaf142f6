"""Host-side mirror of the reusable parts of src/1D/Vch_control_1D/GD_1D.py: the prox, the
line search, the sparsity (KKT) check, target construction, and the optimisation loop of the
`__main__` block (G1:333-477) as a callable.  Prompts and plots are out of scope."""
from __future__ import annotations

import contextlib
import io

import numpy as np

from ..engine import make_opt
from .Forward_solver import run_main_simulation
from .backward_solver import run_backward
from .cost_and_function import calculate_cost, calculate_gradient, perform_gradient_step
from .config import ForwardSolverConfig, OptimizationConfig, load_params, save_params
from ._ctx import engine_for

INTERACTIVE = False
DEFAULT_TARGET_CHOICE = 1
DEFAULT_TRACKING_CHOICE = 1


def perform_proximal_and_projection(u_temp, alpha, kappa, u_min, u_max):
    """Soft threshold alpha*kappa then box projection (G1:56-71), on the GPU: the engine's fused
    kernel is called with r = 0, b3 = 0 and step 0 on the already stepped control."""
    u_temp = np.asarray(u_temp, dtype=np.float64)
    shp = u_temp.shape
    u2 = u_temp.reshape(-1, shp[-1]) if u_temp.ndim > 1 else u_temp.reshape(1, -1)
    eng = engine_for(u2.shape[1] - 1, max_steps=max(u2.shape[0], 1))
    # prox(v) with v = u - alpha*(r + b3 u): choose r = 0, b3 = 0 so that v = u
    o = make_opt(b3=0.0, kappa_sparsity=float(kappa), u_min=float(u_min), u_max=float(u_max))
    out = eng.grad_prox(u2, np.zeros_like(u2), float(alpha), o)
    return np.asarray(out).reshape(shp)


def perform_group_proximal_and_projection(u_temp, alpha, kappa, u_min, u_max, sparsity, x, t_hist):
    """perform_proximal_and_projection for the directional sparsity functionals: the prox of
    alpha * kappa * sum of the group norms under the box, the groups being the rows ("time") or the columns ("space") of the
    (rows, N+1) control; the engine's group kernel with r = 0, b3 = 0 on the already stepped control."""
    u2 = np.asarray(u_temp, dtype=np.float64)
    eng = engine_for(u2.shape[1] - 1, float(x[-1] - x[0]), max_steps=max(u2.shape[0], 1))
    o = make_opt(b3=0.0, kappa_sparsity=float(kappa), u_min=float(u_min), u_max=float(u_max))
    return np.asarray(eng.grad_prox(u2, np.zeros_like(u2), float(alpha), o, sparsity=sparsity, x=x, t_hist=t_hist))


def _prox(u_temp, alpha, kappa, u_min, u_max, sparsity, x, t_hist):
    if sparsity == "full":
        return perform_proximal_and_projection(u_temp, alpha, kappa, u_min, u_max)
    return perform_group_proximal_and_projection(u_temp, alpha, kappa, u_min, u_max, sparsity, x, t_hist)


def _cost(phi, u, phi_Q, phi_T, x, t_hist, b1, b2, b3, kappa, sparsity):
    """calculate_cost, silent, with J4 of the sparsity mode."""
    if sparsity == "full":
        with contextlib.redirect_stdout(io.StringIO()):
            return calculate_cost(phi, u, phi_Q, phi_T, x, t_hist, b1, b2, b3, kappa, verbose=False)
    rows, n = phi.shape
    eng = engine_for(n - 1, float(x[-1] - x[0]), max_steps=max(rows - 2, 1))
    J = eng.cost(phi, u, phi_Q, phi_T, x, t_hist, make_opt(b1=b1, b2=b2, b3=b3, kappa_sparsity=kappa), sparsity=sparsity)
    return float(J[4])


def perform_backtracking_line_search(u_k, cost_k, grad_smooth, phi_Q_target, phi_T_target, x, t_hist, b1, b2, b3,
                                     kappa, u_min, u_max, fwd_config, alpha_init=10.0, beta=0.8, max_ls_iter=5,
                                     sparsity="full", initial_phi=None):
    """G1:73-113."""
    alpha, n_trials = alpha_init, 0
    u_next = phi_next = None
    cost_next = cost_k
    for _ in range(max_ls_iter):
        n_trials += 1
        u_next = _prox(perform_gradient_step(u_k, grad_smooth, alpha), alpha, kappa, u_min, u_max, sparsity, x, t_hist)
        phi_next, _, _ = run_main_simulation(fwd_config, store_history=True, control_input=u_next, verbose=False,
                                             initial_phi=initial_phi)
        cost_next = _cost(phi_next, u_next, phi_Q_target, phi_T_target, x, t_hist, b1, b2, b3, kappa, sparsity)
        if cost_next < cost_k:
            return alpha, u_next, cost_next, phi_next, 0.0, 0.0, n_trials
        alpha *= beta
    return alpha, u_next, cost_next, phi_next, 0.0, 0.0, n_trials


def verify_sparsity_condition(u_optimal, r_optimal, kappa, tol=1e-6, verbose=True):
    """u* = 0  <=>  |r*| <= kappa match statistics (G1:115-147).  Returns (sparsity %, |r|<=kappa %,
    match %)."""
    is_u_zero = np.abs(u_optimal) < tol
    is_r_small = np.abs(r_optimal) <= kappa
    total = u_optimal.size
    res = (100.0 * np.sum(is_u_zero) / total, 100.0 * np.sum(is_r_small) / total,
           100.0 * np.sum(is_u_zero == is_r_small) / total)
    if verbose:
        print(f"Sparsity of final control (u* ~ 0): {res[0]:.2f}%")
        print(f"Region where |r*| <= kappa:          {res[1]:.2f}%")
        print(f"Percentage of points where the conditions match: {res[2]:.2f}%")
    return res


def build_targets_1d(x, t_hist, phi_initial, Lx, T, interactive=False, choice_t=DEFAULT_TARGET_CHOICE,
                     choice_q=DEFAULT_TRACKING_CHOICE, A_T=0.7, k_tan=0.45):
    """G1:151-254 (non-interactive)."""
    if choice_t == 1:
        phi_T = A_T * np.sin(2.0 * np.pi * x / Lx)
    elif choice_t == 2:
        phi_T = A_T * np.cos(2.0 * np.pi * x / Lx)
    else:
        tr = np.tan(2.0 * np.pi * k_tan * (x / Lx - 0.5))
        sc = np.max(np.abs(tr))
        phi_T = A_T * (tr / (sc if sc > 1e-12 else 1.0))
    if choice_q == 1:
        tp = (t_hist / (t_hist[-1] if t_hist[-1] > 0 else 1.0))[:, np.newaxis]
        phi_Q = (1.0 - tp) * phi_initial + tp * phi_T
    else:
        phi_Q = np.zeros((len(t_hist), len(x)))
    return phi_T, phi_Q


def relative_errors(phi, phi_Q, phi_T, x, t_hist):
    """(tracking, terminal) relative L2 errors of a state history as the driver reports them per iteration
    (G1:425-450): trapezoid rule in x then t, sqrt(L T) as denominator when the tracking target is ~0."""
    trapz = getattr(np, "trapezoid", None) or np.trapz
    sq_x = lambda a: trapz(np.square(a), x=x, axis=-1)
    scale = np.sqrt(max(float(x[-1] - x[0]), 1e-30) * max(float(t_hist[-1] - t_hist[0]), 1e-30))
    num_q = np.sqrt(trapz(sq_x(phi - phi_Q), x=t_hist))
    den_q = np.sqrt(trapz(sq_x(phi_Q), x=t_hist))
    if den_q < 1e-9 * scale:
        den_q = scale
    return float(num_q / (den_q + 1e-12)), float(np.sqrt(sq_x(phi[-1] - phi_T)) / (np.sqrt(sq_x(phi_T)) + 1e-12))


def run_optimization(fwd_config: ForwardSolverConfig, opt_config: OptimizationConfig, n_iter=None, choice_t=1,
                     choice_q=1, sparsity="full", initial_phi=None):
    """The loop of G1:333-477 -> dict(costs, alphas, trials, tracking_error, terminal_error, u, phi, r, converged).
    `sparsity` "time" / "space": the same loop with the prox and J4 of the directional sparsity functional (a name of
    Engine1D.SPARSITY; "full" is the reference's loop).  `initial_phi` (N+1,): the start state of every march (default:
    the reference's seed 42)."""
    from ..engine import Engine1D
    Engine1D._mode(sparsity)
    O = opt_config
    quiet = contextlib.redirect_stdout(io.StringIO())
    phi_k, x, t_hist = run_main_simulation(fwd_config, store_history=True, verbose=False, initial_phi=initial_phi)
    u_k = np.zeros_like(phi_k)
    phi_T, phi_Q = build_targets_1d(x, t_hist, phi_k[0].copy(), float(fwd_config.Lx), float(fwd_config.T),
                                    choice_t=choice_t, choice_q=choice_q)
    if sparsity == "full":
        with quiet:
            cost_k = calculate_cost(phi_k, u_k, phi_Q, phi_T, x, t_hist, O.b1, O.b2, O.b3, O.kappa_sparsity)
    else:
        cost_k = _cost(phi_k, u_k, phi_Q, phi_T, x, t_hist, O.b1, O.b2, O.b3, O.kappa_sparsity, sparsity)
    costs, alphas, trials, track, term = [cost_k], [], [], [], []
    alpha_prev, plateau, converged = O.alpha_max, 0, False
    r_k = None
    for k in range(O.max_iter if n_iter is None else n_iter):
        _, _, r_k = run_backward(phi_k, x, t_hist, O.b1, O.b2, phi_Q, phi_T)
        g = calculate_gradient(r_k, u_k, O.b3)
        u_o = _prox(perform_gradient_step(u_k, g, alpha_prev), alpha_prev, O.kappa_sparsity, O.u_min, O.u_max, sparsity, x,
                    t_hist)
        phi_o, _, _ = run_main_simulation(fwd_config, store_history=True, control_input=u_o, verbose=False,
                                          initial_phi=initial_phi)
        c_o = _cost(phi_o, u_o, phi_Q, phi_T, x, t_hist, O.b1, O.b2, O.b3, O.kappa_sparsity, sparsity)
        if c_o < cost_k:
            a_k, u_n, c_n, phi_n, nt = alpha_prev, u_o, c_o, phi_o, 1
        else:
            a_k, u_n, c_n, phi_n, _, _, nt = perform_backtracking_line_search(
                u_k, cost_k, g, phi_Q, phi_T, x, t_hist, O.b1, O.b2, O.b3, O.kappa_sparsity, O.u_min, O.u_max,
                fwd_config, alpha_init=alpha_prev, sparsity=sparsity, initial_phi=initial_phi)
        costs.append(c_n); alphas.append(a_k); trials.append(nt)
        e_q, e_t = relative_errors(phi_n, phi_Q, phi_T, x, t_hist)
        track.append(e_q); term.append(e_t)
        plateau = plateau + 1 if (k > 0 and abs(costs[-1] - costs[-2]) < 1e-7) else 0
        if plateau >= 10:
            alpha_prev, plateau = min(O.alpha_max, a_k * 2.0), 0
        else:
            alpha_prev = min(O.alpha_max, a_k * 1.2)
        change = np.linalg.norm(u_n - u_k) / (np.linalg.norm(u_k) + 1e-9)
        if change < 1e-5 and k > 10:
            u_k, converged = u_n.copy(), True
            break
        u_k, cost_k, phi_k = u_n.copy(), c_n, phi_n
    return dict(costs=costs, alphas=alphas, trials=trials, tracking_error=track, terminal_error=term, u=u_k, phi=phi_k,
                r=r_k, converged=converged, phi_T=phi_T, phi_Q=phi_Q, x=x, t_hist=t_hist)


def run_optimization_resident(fwd_config: ForwardSolverConfig, opt_config: OptimizationConfig, n_iter=None, choice_t=1,
                              choice_q=1, initial_phi=None, seeds=None, sparsity="full"):
    """The same loop (G1:333-477) run device-resident through `vch1d_pgd_*`: control, state history,
    adjoint and targets never leave HBM between iterations.  `seeds` (a list) or `initial_phi`
    ((B, N+1)) gives a batch of trajectories; default = the reference's seed 42.  Returns the same
    dict as run_optimization, with a leading trajectory axis when batched.  `sparsity`: a name of Engine1D.SPARSITY for
    every trajectory, or a list with one name per trajectory; "full" takes the calls of the reference's loop exactly."""
    from ..engine import Engine1D, time_grid
    from .Forward_solver import init_phi_random, delta_sep
    O = opt_config
    N = int(fwd_config.N)
    tg, dts = time_grid(float(fwd_config.T), float(fwd_config.dt_initial))
    t_hist = np.concatenate([[0.0], tg])
    if initial_phi is not None:
        phi0 = np.atleast_2d(np.asarray(initial_phi, dtype=np.float64))
    else:
        phi0 = np.stack([init_phi_random(N, delta_sep, amp=0.01, seed=s, enforce_zero_mean=True)
                         for s in (seeds if seeds is not None else [42])])
    B = phi0.shape[0]
    eng = Engine1D(N=N, Lx=float(fwd_config.Lx), tau=float(fwd_config.tau), gamma=float(fwd_config.gamma),
                   c1=float(fwd_config.c1), c2=float(fwd_config.c2), kappa=float(fwd_config.kappa), batch=B,
                   max_steps=max(len(dts), 1))
    try:
        x = eng.x.copy()
        phi_T = np.stack([build_targets_1d(x, t_hist, phi0[b], float(fwd_config.Lx), float(fwd_config.T),
                                           choice_t=choice_t, choice_q=2)[0] for b in range(B)])
        phi_Q = None if choice_q == 1 else np.zeros((B, len(t_hist), N + 1))
        J0 = eng.pgd_init(phi0, phi_T, t_hist, dts, make_opt(O), phi_Q=phi_Q, x=x,
                          sparsity=None if isinstance(sparsity, str) and sparsity == "full" else sparsity)
        n = O.max_iter if n_iter is None else n_iter
        res = eng.pgd_iterate(n)
        sq = (lambda a: a[0]) if B == 1 else (lambda a: a)
        costs = np.concatenate([J0.reshape(B, 5)[:, 4:5], res["cost"]], axis=1)
        out = dict(costs=sq(costs), alphas=sq(res["alpha"]), trials=sq(res["trials"]), change=sq(res["change"]),
                   tracking_error=sq(res["tracking_error"]), terminal_error=sq(res["terminal_error"]), iters=res["iters"], u=eng.pgd_get("u"), phi=eng.pgd_get("phi"), r=eng.pgd_get("r"),
                   phi_T=sq(phi_T), phi_Q=eng.pgd_get("phi_Q"), x=x, t_hist=t_hist, seconds=res["seconds"])
    finally:
        eng.close()
    return out


def run_sweep(fwd_config: ForwardSolverConfig, opt_configs, n_iter=None, seed=42, amp=0.01, initial_phi=None, choice_t=1,
              choice_q=1, u0=None, return_controls=False, n_newton=0, n_trust=0, radius0=1.0, sparsity=None):
    """A parameter sweep as ONE batch: member b runs the PGD loop with opt_configs[b] (weights, sparsity parameter, box,
    alpha_max), all members from the same initial state (`initial_phi` (N+1,), else `seed`, `amp`) and targets, so that
    they differ by their parameters only.  `u0`: start control, one (rows, N+1) array for every member or one per member
    (continuation in kappa_sparsity, resuming from a saved optimal_control.npy); default zeros.  `n_iter` None: the
    largest max_iter of the members (the loop length is one for the batch).  Returns dict(costs [B][it+1], alphas, trials,
    changes, tracking_error, terminal_error, iters, seconds, kkt = Engine1D.pgd_kkt(refresh=True) -- the sparsity
    statistic and the stationarity measure of every member, counted on the device -- phi_T, t_hist, x, and u only with
    return_controls); the state history never leaves the device.  `n_newton` > 0 polishes every member after its PGD
    iterations by that many damped Newton rounds on its free set (Engine1D.pgd_newton, on the device) and adds `newton`
    (its records) and `costs_newton` [B][n_newton+1] (the cost before the first round, then after every round); kkt and u
    are then those of the polished iterate.  0 leaves the result as it is without the polish.  `n_trust` > 0 does the same
    (after the Newton rounds, if both are asked for) with that many trust-region rounds from the radius `radius0`
    (Engine1D.pgd_trust), which follow a direction of non-positive curvature instead of ending on it, and adds `trust` and
    `costs_trust` [B][n_trust+1].  `sparsity`: None (every member "full", today's calls), one name of Engine1D.SPARSITY or one
    per member; the Newton and trust-region polish is refused by the engine while a member is in a group mode."""
    from ..engine import Engine1D, time_grid
    from .Forward_solver import init_phi_random, delta_sep
    opt_configs = list(opt_configs)
    B = len(opt_configs)
    if B < 1:
        raise ValueError("run_sweep needs at least one OptimizationConfig")
    N = int(fwd_config.N)
    tg, dts = time_grid(float(fwd_config.T), float(fwd_config.dt_initial))
    t_hist = np.concatenate([[0.0], tg])
    if initial_phi is None:
        initial_phi = init_phi_random(N, delta_sep, amp=amp, seed=int(seed), enforce_zero_mean=True)
    phi0 = np.repeat(np.asarray(initial_phi, dtype=np.float64).reshape(1, N + 1), B, axis=0)
    if u0 is not None:
        u0 = np.asarray(u0, dtype=np.float64)
        if u0.ndim == 2:
            u0 = np.repeat(u0[None], B, axis=0)
    eng = Engine1D(N=N, Lx=float(fwd_config.Lx), tau=float(fwd_config.tau), gamma=float(fwd_config.gamma),
                   c1=float(fwd_config.c1), c2=float(fwd_config.c2), kappa=float(fwd_config.kappa), batch=B,
                   max_steps=max(len(dts), 1))
    try:
        x = eng.x.copy()
        phi_T = build_targets_1d(x, t_hist, phi0[0], float(fwd_config.Lx), float(fwd_config.T), choice_t=choice_t,
                                 choice_q=2)[0]
        phi_Q = None if choice_q == 1 else np.zeros((B, len(t_hist), N + 1))
        J0 = eng.pgd_init(phi0, np.repeat(phi_T[None], B, axis=0), t_hist, dts, [make_opt(o) for o in opt_configs],
                          phi_Q=phi_Q, x=x, u0=u0, sparsity=sparsity)
        n = int(max(int(o.max_iter) for o in opt_configs) if n_iter is None else n_iter)
        res = eng.pgd_iterate(n)
        newton = eng.pgd_newton(int(n_newton)) if int(n_newton) > 0 else None
        trust = eng.pgd_trust(int(n_trust), radius0) if int(n_trust) > 0 else None
        out = dict(costs=np.concatenate([J0[:, 4:5], res["cost"]], axis=1), alphas=res["alpha"], trials=res["trials"],
                   changes=res["change"], tracking_error=res["tracking_error"], terminal_error=res["terminal_error"],
                   iters=res["iters"], seconds=res["seconds"], kkt=eng.pgd_kkt(refresh=True), phi_T=phi_T, t_hist=t_hist,
                   x=x)
        for name, rec in (("newton", newton), ("trust", trust)):
            if rec is None:
                continue
            # an idle round carries the cost the member ended with
            cn = np.concatenate([rec["cost"][:, :1], rec["cost_new"]], axis=1)
            for r in range(1, cn.shape[1]):
                cn[:, r] = np.where(np.isnan(cn[:, r]), cn[:, r - 1], cn[:, r])
            out[name], out["costs_" + name] = rec, cn
        if return_controls:
            out["u"] = eng.pgd_get("u").reshape(B, len(t_hist), N + 1)
    finally:
        eng.close()
    return out


def newton_refine(fwd_config: ForwardSolverConfig, opt_config: OptimizationConfig, u, phi_Q_target, phi_T_target,
                  n_newton=3, k=50, cg_tol=1e-8, max_halvings=10, on_device=False):
    """Rounds of a damped Newton method on the free set, from the control `u` (for instance what the PGD loop left).
    Per round: the free set of the iterate (strictly inside the box of `opt_config`, off the kink of the L1 term) and
    the Newton step d of the full cost on it (second_order_conditions.reduced_newton_step: conjugate gradients on the
    device, at most `k` steps to `cg_tol`).  Trials are clip(u + s d, box) for s = 1, 1/2, ..., at most `max_halvings`
    halvings; a free node whose sign the trial flips is set to 0, the kink, where the next round pins it.  The first s
    with J(trial) <= J(u) - 1e-4 s pred is accepted, J the full cost of a march of the trial from the default start of
    `run_main_simulation` (Engine1D.forward and Engine1D.cost) and pred the decrease the quadratic model predicts for the
    full step.  The loop ends after `n_newton` rounds, when the right-hand side vanishes (stationarity on the free set),
    when the first CG direction already has non-positive curvature, or when no s is accepted.

    Returns (u, records): the final control and one dict per round with cost (before the round), n_free, rnorm0, steps,
    status, s (None when the round moved nothing) and cost_new (the accepted trial's, else the unchanged cost).

    on_device=True runs the rounds on the device (Engine1D.pgd_newton): one context, one pgd_init(u0=u) with this loop's
    own start state and targets, the step, the trials and the decisions without a history crossing the bus; the records
    have the same keys.  Two departures: a CG breakdown ends the rounds there (no march under a control that may not be
    finite), where the host loop tries the step; a trial whose march reports a non-finite mass defect counts as not
    accepted there, where the host loop raises."""
    if on_device:
        return _newton_refine_device(fwd_config, opt_config, u, phi_Q_target, phi_T_target, n_newton, k, cg_tol, max_halvings)
    from ..engine import time_grid
    from ._ctx import engine_for_config
    from .Forward_solver import init_phi_random, delta_sep
    from .second_order_conditions import free_set, reduced_newton_step
    N = int(fwd_config.N)
    tg, dts = time_grid(float(fwd_config.T), float(fwd_config.dt_initial))
    t_hist = np.concatenate([[0.0], tg])
    M = len(dts)
    lo, hi = float(opt_config.u_min), float(opt_config.u_max)
    u = np.asarray(u, dtype=np.float64)[:M + 2]                     # nodes outside the box are not free: the first trial clips them
    phi0 = init_phi_random(N, delta_sep, amp=0.01, seed=42, enforce_zero_mean=True)
    x = np.linspace(0.0, float(fwd_config.Lx), N + 1)
    pq, pt = np.asarray(phi_Q_target, dtype=np.float64)[None, :M + 2], np.asarray(phi_T_target, dtype=np.float64)[None]
    opt = make_opt(opt_config)

    def full_cost(v):
        eng = engine_for_config(fwd_config, batch=1, max_steps=max(M, 1))
        phi, _ = eng.forward(phi0[None], dts, u=v[None], store=True)
        J = eng.cost(phi.reshape((1, M + 2, N + 1)), v[None], pq, pt, x, t_hist, opt)
        return float(np.atleast_2d(J)[0, 4])

    cost = full_cost(u)
    records = []
    for _ in range(int(n_newton)):
        S = reduced_newton_step(fwd_config, u, x, t_hist, opt_config, phi_Q_target=phi_Q_target, phi_T_target=phi_T_target,
                                u_min=lo, u_max=hi, k=k, cg_tol=cg_tol)
        rec = dict(cost=cost, n_free=S["n_free"], rnorm0=S["rnorm0"], steps=S["steps"], status=S["status"], s=None, cost_new=cost)
        records.append(rec)
        if S["rnorm0"] == 0.0 or (S["status"] == "negcurv" and S["steps"] == 0):
            break
        d, free, s = S["d"], free_set(u, lo, hi), 1.0
        for _ in range(int(max_halvings) + 1):
            trial = np.clip(u + s * d, lo, hi)
            trial[free & (trial * u < 0.0)] = 0.0
            J = full_cost(trial)
            if J <= cost - 1e-4 * s * S["pred"]:
                rec["s"], rec["cost_new"] = s, J
                break
            s *= 0.5
        if rec["s"] is None:
            break
        u, cost = trial, J
    return u, records


def _newton_refine_device(fwd_config, opt_config, u, phi_Q_target, phi_T_target, n_newton, k, cg_tol, max_halvings):
    """newton_refine(on_device=True): the problem of the host loop as a resident PGD problem, then Engine1D.pgd_newton."""
    from ..engine import Engine1D, time_grid
    from ._ctx import engine_for_config
    from .Forward_solver import init_phi_random, delta_sep
    N = int(fwd_config.N)
    tg, dts = time_grid(float(fwd_config.T), float(fwd_config.dt_initial))
    t_hist = np.concatenate([[0.0], tg])
    M = len(dts)
    u = np.asarray(u, dtype=np.float64)[:M + 2]
    phi0 = init_phi_random(N, delta_sep, amp=0.01, seed=42, enforce_zero_mean=True)
    x = np.linspace(0.0, float(fwd_config.Lx), N + 1)
    eng = engine_for_config(fwd_config, batch=1, max_steps=max(M, 1))
    eng.pgd_init(phi0[None], np.asarray(phi_T_target, dtype=np.float64)[None], t_hist, dts, [make_opt(opt_config)],
                 phi_Q=np.asarray(phi_Q_target, dtype=np.float64)[None, :M + 2], x=x, u0=u[None])
    R = eng.pgd_newton(int(n_newton), k=k, cg_tol=cg_tol, max_halvings=max_halvings)
    records = []
    for r in range(int(R["rounds"])):
        if Engine1D.NEWTON_STATUS[int(R["status"][0, r])] == "idle":
            break
        s = float(R["s"][0, r])
        records.append(dict(cost=float(R["cost"][0, r]), n_free=int(R["n_free"][0, r]), rnorm0=float(R["rnorm0"][0, r]),
                            steps=int(R["cg_steps"][0, r]), status=Engine1D.CG_STATUS[int(R["cg_status"][0, r])],
                            s=None if np.isnan(s) else s, cost_new=float(R["cost_new"][0, r])))
    return eng.pgd_get("u"), records


def trust_refine(fwd_config: ForwardSolverConfig, opt_config: OptimizationConfig, u, phi_Q_target, phi_T_target,
                 n_rounds=3, radius0=1.0, k=50, cg_tol=1e-8, radius_max=None, radius_min=None, on_device=False):
    """Rounds of a trust-region Newton method on the free set, from the control `u`: newton_refine with the damping
    replaced by a radius.  Per round: the Steihaug step x of the full cost on the free set of the iterate inside
    ||x||_D <= radius (Engine1D.hess_cg_trust: a direction of non-positive curvature is followed to the boundary instead
    of ending the loop), one trial clip(u + x, box) with a flipped sign set to 0 (Engine1D.newton_trial(1)), its march
    from the default start of `run_main_simulation` and its cost J(t); rho = (J(u) - J(t)) / pred.  The trial is accepted
    iff J(t) is finite and J(t) <= J(u) - 1e-4 pred, else the iterate stays ("rejected") and the loop goes on.  The radius:
    rho < 1/4 or not finite: min(radius, ||x||_D) / 4; else rho > 3/4 after a "boundary" or "negcurv" exit:
    min(2 radius, radius_max).  The loop ends after `n_rounds` rounds, on a vanishing right-hand side ("stationary"), a
    CG breakdown, or once the radius is below radius_min ("stalled" when that round was rejected).  radius_max /
    radius_min default to 1024 radius0 and 1e-10 radius0.

    Returns (u, records): one dict per round with cost, cost_new, pred, rnorm0, radius (the round's), ratio, xnorm,
    steps, cg_status (a name of Engine1D.TRUST_CG_STATUS), status (a name of Engine1D.TRUST_STATUS), n_free.

    on_device=True runs the rounds on the device (Engine1D.pgd_trust): one context, one pgd_init(u0=u) with this loop's
    own start state and targets; the records have the same keys."""
    from ..engine import Engine1D, time_grid
    from ._ctx import engine_for_config
    from .Forward_solver import init_phi_random, delta_sep
    N = int(fwd_config.N)
    tg, dts = time_grid(float(fwd_config.T), float(fwd_config.dt_initial))
    t_hist = np.concatenate([[0.0], tg])
    M = len(dts)
    u = np.asarray(u, dtype=np.float64)[:M + 2]
    radius = float(radius0)
    radius_max = 1024.0 * radius if radius_max is None else float(radius_max)
    radius_min = 1e-10 * radius if radius_min is None else float(radius_min)
    phi0 = init_phi_random(N, delta_sep, amp=0.01, seed=42, enforce_zero_mean=True)
    x = np.linspace(0.0, float(fwd_config.Lx), N + 1)
    pq, pt = np.asarray(phi_Q_target, dtype=np.float64)[None, :M + 2], np.asarray(phi_T_target, dtype=np.float64)[None]
    opt = make_opt(opt_config)
    eng = engine_for_config(fwd_config, batch=1, max_steps=max(M, 1))
    CGS, NTS = Engine1D.TRUST_CG_STATUS, Engine1D.TRUST_STATUS
    if on_device:
        eng.pgd_init(phi0[None], pt, t_hist, dts, [opt], phi_Q=pq, x=x, u0=u[None])
        R = eng.pgd_trust(int(n_rounds), radius, k=k, cg_tol=cg_tol, radius_max=radius_max, radius_min=radius_min)
        records = []
        for r in range(int(R["rounds"])):
            if NTS[int(R["status"][0, r])] == "idle":
                break
            records.append(dict(cost=float(R["cost"][0, r]), cost_new=float(R["cost_new"][0, r]), pred=float(R["pred"][0, r]),
                                rnorm0=float(R["rnorm0"][0, r]), radius=float(R["radius"][0, r]), ratio=float(R["ratio"][0, r]),
                                xnorm=float(R["xnorm"][0, r]), steps=int(R["cg_steps"][0, r]),
                                cg_status=CGS[int(R["cg_status"][0, r])], status=NTS[int(R["status"][0, r])],
                                n_free=int(R["n_free"][0, r])))
        return eng.pgd_get("u").reshape(M + 2, N + 1), records

    def full_cost(v):
        phi, _ = eng.forward(phi0[None], dts, u=v[None], store=True)
        J = eng.cost(phi.reshape((1, M + 2, N + 1)), v[None], pq, pt, x, t_hist, opt)
        return float(np.atleast_2d(J)[0, 4])

    cost = full_cost(u)
    records = []
    for _ in range(int(n_rounds)):
        eng.forward(phi0[None], dts, u=np.ascontiguousarray(u[None]), store=False)
        S = eng.hess_cg_trust(int(k), radius, t_hist, opt, cg_tol=cg_tol, u=np.ascontiguousarray(u[None]), phi_Q=pq, phi_T=pt,
                              dt=dts, x=x)
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


def main(n_iter=None, params_file="last_run_config.json", control_file="optimal_control.npy", num_directions=3,
         verbose=True):
    """Non-interactive equivalent of the reference's `__main__` block (G1:256-609) without prompts and
    plots: parameters from the last-run JSON (defaults if absent), the PGD loop (device-resident), the
    final adjoint, `optimal_control.npy` (G1:487), the coercivity finite-difference test (G1:490-509), the
    sparsity statistic (G1:518) and `save_params` (G1:608)."""
    from .second_order_conditions import approximate_second_order_condition
    say = print if verbose else (lambda *a, **k: None)
    allp = load_params(params_file)
    fwd, opt = allp.forward_solver, allp.optimization
    res = run_optimization_resident(fwd, opt, n_iter=n_iter)
    it = int(res["iters"])
    costs = np.asarray(res["costs"])
    say(f"Completed Iterations: {it}\nFinal Cost: {costs[it]:.5f}\nCost Reduction: {100 * (1 - costs[it] / costs[0]):.2f}%")
    x, t_hist = res["x"], res["t_hist"]
    _, _, r_opt = run_backward(res["phi"], x, t_hist, opt.b1, opt.b2, res["phi_Q"], res["phi_T"])
    np.save(control_file, res["u"])
    say(f"Optimal control saved as '{control_file}'")
    sink = contextlib.nullcontext() if verbose else contextlib.redirect_stdout(io.StringIO())
    with sink:
        hv = approximate_second_order_condition(fwd_config=fwd, u_star=res["u"], r_star=r_opt, phi_star=res["phi"], x=x,
                                                t_hist=t_hist, b1=opt.b1, b2=opt.b2, b3=opt.b3, kappa=opt.kappa_sparsity,
                                                phi_Q_target=res["phi_Q"], phi_T_target=res["phi_T"], u_min=opt.u_min,
                                                u_max=opt.u_max, num_directions=num_directions, epsilon=1e-4, seed=42)
        for i, d2 in enumerate(hv, start=1):
            say(f"  Direction {i}: estimated second derivative = {d2:.6e}")
        sp = verify_sparsity_condition(res["u"], r_opt, opt.kappa_sparsity, verbose=verbose)
    save_params(fwd, opt, it, params_file)
    return dict(res, hessian_values=hv, sparsity=sp, r_optimal=r_opt)

