"""Host-side mirror of src/2D/Vch_control_2D/second_order_conditions_2d.py: finite-difference
coercivity test (N extra forward marches + costs, all on the GPU through the mirrored
`run_main_simulation` / `calculate_cost`) and the sparsity (KKT) match statistic; beside the reference's
formula, `exact_second_order_condition_2d` gives the exact second derivative by tangent marches."""
from __future__ import annotations

import contextlib
import io
from typing import List, Optional

import numpy as np

from .Forward2_solver import run_main_simulation
from .cost2_and_function import calculate_cost
from .config import ForwardSolverConfig, OptimizationConfig


def _generate_direction(u_star, r_star, u_min, u_max, rng, tol: float = 1e-8):
    """Random unit direction in the bound-only critical cone (S2:35-88): one `standard_normal` draw, then the
    components at saturated nodes are reflected into the box (where both bounds are hit, the upper one wins, as in
    the reference's assignment order); r_star is part of the signature only."""
    draw = rng.standard_normal(size=u_star.shape)
    inward = np.zeros(u_star.shape, dtype=np.int8)          # +1 at the lower bound, -1 at the upper bound
    inward[u_star <= u_min + tol] = 1
    inward[u_star >= u_max - tol] = -1
    v = np.where(inward == 0, draw, inward * np.abs(draw))
    length = np.linalg.norm(v)
    if length < 1e-12:
        v = np.zeros_like(v)
        v.flat[0] = 1.0
        length = 1.0
    return v / length


def _ensure_opt_config(b1, b2, b3, kappa_sparsity, opt_config) -> OptimizationConfig:
    """The weights as an OptimizationConfig: the object if one is given, else built from the four legacy
    scalars, all of which must then be present (S2:91-117)."""
    if opt_config is not None:
        return opt_config
    weights = dict(b1=b1, b2=b2, b3=b3, kappa_sparsity=kappa_sparsity)
    if None in weights.values():
        raise ValueError("Either provide opt_config or all of (b1, b2, b3, kappa_sparsity).")
    return OptimizationConfig(**{k: float(v) for k, v in weights.items()})


def approximate_second_order_condition_2d(u_star, r_star, phi_star, x, y, t_hist,
                                          opt_config: Optional[OptimizationConfig] = None, b1=None, b2=None, b3=None,
                                          kappa=None, phi_Q_target=None, phi_T_target=None, u_min: float = -np.inf,
                                          u_max: float = np.inf, num_directions: int = 10, epsilon: float = 1e-4,
                                          seed: Optional[int] = None,
                                          fwd_config: Optional[ForwardSolverConfig] = None) -> List[float]:
    """d2 ~ (J(u* + eps h) - J(u*) - eps <grad J(u*), h>) / (eps^2 / 2) for random h (S2:120-235)."""
    rng = np.random.default_rng(seed)
    opt = _ensure_opt_config(b1, b2, b3, kappa, opt_config)
    if phi_Q_target is None:
        phi_Q_target = np.zeros_like(phi_star)
    if phi_T_target is None:
        phi_T_target = np.zeros_like(phi_star[-1])
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())
    with quiet():
        cost_star = calculate_cost(phi_star, u_star, phi_Q_target, phi_T_target, x, y, t_hist, opt)
    grad_star = r_star + opt.b3 * u_star
    print(f"Testing {num_directions} random directions in the critical cone...")
    # all directions are drawn first -- the same draws in the same order as the reference's loop (S2:178-186), so seeded
    # results are unchanged -- and the perturbed controls are then marched as ONE batch of trajectories (MAX_BATCH at a
    # time) with one batched cost evaluation, instead of num_directions marches of batch 1
    dirs = [_generate_direction(u_star, r_star, u_min, u_max, rng) for _ in range(num_directions)]
    costs = _perturbed_costs([u_star + epsilon * h for h in dirs], fwd_config, phi_Q_target, phi_T_target, x, y, t_hist, opt)
    out: List[float] = []
    for i, (h, cost_p) in enumerate(zip(dirs, costs)):
        d2 = (cost_p - cost_star - epsilon * np.sum(grad_star * h)) / (0.5 * epsilon ** 2)
        out.append(float(d2))
        print(f"  Direction {i+1}/{num_directions}: estimated d²J/dh² ≈ {d2:.6e}")
    return out


MAX_BATCH = 8      # perturbed controls marched side by side (each needs its own state and control history on the device)


def _perturbed_costs(controls, fwd_config, phi_Q_target, phi_T_target, x, y, t_hist, opt):
    """J(u) for every control of the list: the marches of `run_main_simulation(config, control_input=u)` (default start:
    init_phi_random(amp=0.1, seed=42), F2:517) and `calculate_cost`, batched over the controls."""
    from ..engine import time_grid
    from ._ctx import engine_for_config
    from .Forward2_solver import init_phi_random, DELTA_SEP
    cfg = fwd_config
    Nx, Ny = int(cfg.Nx), int(cfg.Ny)
    _, dts = time_grid(float(cfg.T), float(cfg.dt_initial))
    phi0 = init_phi_random(Nx, Ny, DELTA_SEP, amp=0.1, seed=42)
    costs = []
    for k0 in range(0, len(controls), MAX_BATCH):
        chunk = controls[k0:k0 + MAX_BATCH]
        nb = len(chunk)
        U = np.stack(chunk)
        rows = U.shape[1]
        eng = engine_for_config(cfg, batch=nb, max_steps=max(len(dts), rows - 1, 1))
        Um = U[:, :len(dts) + 1] if rows > len(dts) + 1 else U            # rows beyond the march are never read (F2:545-548)
        phi_p, _ = eng.forward(np.broadcast_to(phi0, (nb,) + phi0.shape), dts, u=np.ascontiguousarray(Um), store=True)
        phi_p = phi_p.reshape((nb,) + phi_p.shape[-3:])
        tile = lambda a: np.broadcast_to(a, (nb,) + np.shape(a))
        J = eng.cost(phi_p, U, tile(phi_Q_target), tile(phi_T_target), t_hist, opt, x, y)
        costs.extend(float(v) for v in np.atleast_2d(J)[:, 4])
    return costs


def exact_second_order_condition_2d(u_star, r_star, phi_star, x, y, t_hist,
                                    opt_config: Optional[OptimizationConfig] = None, b1=None, b2=None, b3=None,
                                    kappa=None, phi_Q_target=None, phi_T_target=None, u_min: float = -np.inf,
                                    u_max: float = np.inf, num_directions: int = 10, epsilon: float = 1e-4,
                                    seed: Optional[int] = None,
                                    fwd_config: Optional[ForwardSolverConfig] = None) -> List[float]:
    """J''(u*)[h,h] of the smooth part J1 + J2 + J3 of the discrete cost, exactly (to the tolerance of a linear solve), for
    the same seeded directions as `approximate_second_order_condition_2d` draws: no difference quotient, so `epsilon` is
    not used.  One forward march of u* tiled over up to MAX_BATCH directions, then one tangent call per chunk
    (Engine2D.second_order: two linear solves per step and direction).  Per direction the curvature, the exact slope
    J'(u*)h and the adjoint's unweighted `sum(g h)`, g = r* + b3 u*, that the finite-difference formula subtracts, are
    printed side by side.  The L1 term J4 has no curvature away from its kink and is left out; the clip at the end of a time
    step is taken as inactive (|phi| < 1 - delta_sep)."""
    from ..engine import time_grid
    from ._ctx import engine_for_config
    from .Forward2_solver import init_phi_random, DELTA_SEP
    rng = np.random.default_rng(seed)
    opt = _ensure_opt_config(b1, b2, b3, kappa, opt_config)
    if phi_Q_target is None:
        phi_Q_target = np.zeros_like(phi_star)
    if phi_T_target is None:
        phi_T_target = np.zeros_like(phi_star[-1])
    grad_star = r_star + opt.b3 * u_star
    print(f"Testing {num_directions} random directions in the critical cone (exact tangent marches)...")
    dirs = [_generate_direction(u_star, r_star, u_min, u_max, rng) for _ in range(num_directions)]
    cfg = fwd_config
    t_grid, dts = time_grid(float(cfg.T), float(cfg.dt_initial))
    M = len(dts)
    phi0 = init_phi_random(int(cfg.Nx), int(cfg.Ny), DELTA_SEP, amp=0.1, seed=42)
    cut = lambda a: np.asarray(a)[:M + 1]                                   # rows beyond the march are never read (F2:545-548)
    out: List[float] = []
    for k0 in range(0, len(dirs), MAX_BATCH):
        chunk = dirs[k0:k0 + MAX_BATCH]
        nb = len(chunk)
        eng = engine_for_config(cfg, batch=nb, max_steps=max(M, 1))
        tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (nb,) + np.shape(a)))
        eng.forward(tile(phi0), dts, u=tile(cut(u_star)), store=False)
        res = eng.second_order(np.stack([cut(h) for h in chunk]), dts, t_grid, opt, phi_Q=tile(cut(phi_Q_target)),
                               phi_T=tile(phi_T_target), x=x, y=y)
        for i, h in enumerate(chunk):
            d2, slope = float(res["curvature"][i]), float(res["slope"][i])
            out.append(d2)
            print(f"  Direction {k0 + i + 1}/{num_directions}: exact d²J/dh² = {d2:.6e}   exact slope J'h = {slope:.6e}   "
                  f"adjoint sum(g·h) = {np.sum(grad_star * h):.6e}")
    return out


def free_set(u_star, u_min, u_max, tol=1e-8):
    """Nodes where the critical cone is a linear space: strictly inside the box and off the kink of the L1 term, with the
    `tol` of `_generate_direction` (whose rules leave exactly these nodes free whatever the adjoint is)."""
    u_star = np.asarray(u_star)
    return (u_star > u_min + tol) & (u_star < u_max - tol) & (np.abs(u_star) > tol)


def reduced_hessian_extremes_2d(u_star, x, y, t_hist, opt_config: Optional[OptimizationConfig] = None, b1=None, b2=None,
                                b3=None, phi_Q_target=None, phi_T_target=None, u_min: float = -np.inf,
                                u_max: float = np.inf, k: int = 30, seed=None, tol: float = 1e-8,
                                fwd_config: Optional[ForwardSolverConfig] = None, on_device: bool = False,
                                vector: bool = False, reorth: bool = True) -> dict:
    """Extreme eigenvalues of the reduced Hessian P H P of the smooth part J1 + J2 + J3 of the discrete cost at `u_star`,
    by host Lanczos with full reorthogonalisation.  H is the exact Euclidean Hessian with respect to the entries of u
    (Engine2D.hessvec: one tangent and two transposed solves per time step); P masks to the free set
    `free_set(u_star, u_min, u_max, tol)`.  One forward march of u*, as in `exact_second_order_condition_2d`, then one
    hessvec call per Lanczos step.  At most min(k, size of the free set) steps; with k >= that size the Ritz values are all
    eigenvalues of P H P on the free set.

    Returns dict(theta_min, theta_max: the extreme Ritz values; res_min, res_max: their residual norms
    |beta_m s_m| (an eigenvalue of P H P lies within that distance of each); ritz: all Ritz values, ascending; n_free: the
    size of the free set; steps: Lanczos steps taken).  The values are Rayleigh quotients h.Hh / h.h in the Euclidean
    norm of h, the scale of the curvatures `exact_second_order_condition_2d` returns for its unit directions; theta_min is
    not larger than any of those whose direction is supported on the free set.

    What is left out.  The second-order sufficient condition asks for coercivity on the critical cone.  On the free set
    the cone is a linear space and the smallest eigenvalue is the coercivity constant there, which random directions only
    bound from above.  At a node on the kink u* = 0 of kappa |u|_1 the cone admits one sign at most, and at a node on the
    active box it admits the inward sign only: there the cone is a half-line or a point per node, the minimum of the
    quadratic form over it is no eigenvalue problem, and the L1 term adds no curvature along an admitted sign.  Those
    nodes are pinned to zero here, so theta_min bounds the cone's constant from above: a cone direction that mixes free
    and one-signed nodes can still see less curvature.  The sparsity parameter therefore does not enter.  The clip of the
    march is taken as inactive, as in `exact_second_order_condition_2d`.

    on_device=True keeps the iteration on the device (Engine2D.hess_lanczos: the same seeded start vector, the basis and the
    recurrence in device memory, two linear solves per step and time step instead of three); only the tridiagonal matrix
    comes back and its eigh is taken here.  The keys are the same.  reorth=False runs the three-term recurrence with three
    resident vectors (on_device only).  vector=True (on_device with full reorthogonalisation only) adds `v_min`, the unit
    Ritz vector of theta_min in the shape of u_star.  The default path is the host reference."""
    if (vector or not reorth) and not on_device:
        raise ValueError("reduced_hessian_extremes_2d: vector=True and reorth=False need on_device=True")
    if vector and not reorth:
        raise ValueError("reduced_hessian_extremes_2d: vector=True needs full reorthogonalisation")
    from ..engine import time_grid, make_opt
    from ._ctx import engine_for_config
    from .Forward2_solver import init_phi_random, DELTA_SEP
    rng = np.random.default_rng(seed)
    opt = _ensure_opt_config(b1, b2, b3, 0.0, opt_config)
    cfg = fwd_config
    t_grid, dts = time_grid(float(cfg.T), float(cfg.dt_initial))
    M = len(dts)
    u_star = np.asarray(u_star, dtype=np.float64)[:M + 1]           # rows beyond the march are never read (F2:545-548)
    mask = free_set(u_star, u_min, u_max, tol)
    n_free = int(mask.sum())
    if n_free == 0:
        raise ValueError("reduced_hessian_extremes_2d: the free set is empty")
    phi0 = init_phi_random(int(cfg.Nx), int(cfg.Ny), DELTA_SEP, amp=0.1, seed=42)
    eng = engine_for_config(cfg, batch=1, max_steps=max(M, 1))
    one = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[None])
    eng.forward(one(phi0), dts, u=one(u_star), store=False)
    pq = None if phi_Q_target is None else one(np.asarray(phi_Q_target)[:M + 1])
    pt = one(phi_T_target)

    def apply(q):
        res = eng.hessvec(one(q), dts, t_grid, opt, phi_Q=pq, phi_T=pt, x=x, y=y)
        return np.where(mask, res["hv"][0], 0.0)

    q = np.where(mask, rng.standard_normal(u_star.shape), 0.0)
    if on_device:
        box = make_opt(opt, u_min=float(u_min), u_max=float(u_max))
        L = eng.hess_lanczos(one(q), int(k), dts, t_grid, box, phi_Q=pq, phi_T=pt, x=x, y=y, mask=one(mask), tol=tol,
                             reorth=reorth)
        m = int(L["steps"][0])
        alphas, betas = L["alpha"][0, :m], L["beta"][0, :m]
        T = np.diag(alphas) + np.diag(betas[:m - 1], 1) + np.diag(betas[:m - 1], -1)
        theta, S = np.linalg.eigh(T)
        resid = np.abs(betas[m - 1] * S[m - 1])
        out = dict(theta_min=float(theta[0]), theta_max=float(theta[-1]), res_min=float(resid[0]), res_max=float(resid[-1]),
                   ritz=theta, n_free=int(L["n_free"][0]), steps=m)
        if vector:
            v = eng.krylov_vector(S[:, 0][None])[0]
            out["v_min"] = v / np.linalg.norm(v)
        return out
    q /= np.linalg.norm(q)
    Q, alphas, betas = [q], [], []
    steps = min(int(k), n_free)
    for j in range(steps):
        w = apply(Q[j])
        alphas.append(float(np.sum(Q[j] * w)))
        for _ in range(2):                                   # full reorthogonalisation, twice is enough
            for v in Q:
                w -= np.sum(v * w) * v
        beta = float(np.linalg.norm(w))
        betas.append(beta)
        if j + 1 == steps or beta <= 1e-14 * max(abs(a) for a in alphas):     # done, or an invariant subspace
            break
        Q.append(w / beta)
    m = len(alphas)
    T = np.diag(alphas) + np.diag(betas[:m - 1], 1) + np.diag(betas[:m - 1], -1)
    theta, S = np.linalg.eigh(T)
    resid = np.abs(betas[m - 1] * S[m - 1])
    return dict(theta_min=float(theta[0]), theta_max=float(theta[-1]), res_min=float(resid[0]), res_max=float(resid[-1]),
                ritz=theta, n_free=n_free, steps=m)


def reduced_newton_step_2d(u, x, y, t_hist, opt_config: Optional[OptimizationConfig] = None, b1=None, b2=None, b3=None,
                           kappa=None, phi_Q_target=None, phi_T_target=None, u_min: float = -np.inf,
                           u_max: float = np.inf, k: int = 50, cg_tol: float = 1e-8, precond: bool = True,
                           tol: float = 1e-8, fwd_config: Optional[ForwardSolverConfig] = None) -> dict:
    """The Newton step of the full cost J1 + J2 + J3 + J4 on the free set `free_set(u, u_min, u_max, tol)` of the control
    `u`: d solves P H P d = -P (grad(J1+J2+J3) + kappa_sparsity wt W_cost sign(u)) by (preconditioned) conjugate
    gradients that stay on the device (Engine2D.hess_cg with rhs=None).  On the free set |u| > tol, so the L1 term is
    smooth there and the right-hand side is the exact Euclidean gradient of the full cost; H is the exact Hessian of the
    smooth part (the L1 term has no curvature off its kink).  One forward march of u, as in
    `reduced_hessian_extremes_2d`, then one hess_cg call of at most `k` steps: two linear solves per CG step and time
    step.  `precond` scales by the L2(Q) mass diag(wt W_cost) of the control, the function-space metric.

    Returns dict(d: the step, zero off the free set; steps; status: "converged", "limit", "negcurv" or "breakdown";
    resid: the relative residuals of the steps taken; pred: the decrease the quadratic model predicts for the full step;
    rnorm0: the Euclidean norm of the right-hand side; curv_min: the smallest curvature p.Hp / p.Dp seen; n_free; p: the
    direction of non-positive curvature when the status is "negcurv", else None).  With "negcurv" d is the iterate before
    that direction (zero when the first direction already has non-positive curvature)."""
    from ..engine import time_grid, make_opt, Engine2D
    from ._ctx import engine_for_config
    from .Forward2_solver import init_phi_random, DELTA_SEP
    if fwd_config is None:
        raise ValueError("reduced_newton_step_2d: fwd_config is required (the grid and the time steps of the march of u)")
    opt = _ensure_opt_config(b1, b2, b3, kappa, opt_config)
    cfg = fwd_config
    t_grid, dts = time_grid(float(cfg.T), float(cfg.dt_initial))
    M = len(dts)
    u = np.asarray(u, dtype=np.float64)[:M + 1]                     # rows beyond the march are never read (F2:545-548)
    phi0 = init_phi_random(int(cfg.Nx), int(cfg.Ny), DELTA_SEP, amp=0.1, seed=42)
    eng = engine_for_config(cfg, batch=1, max_steps=max(M, 1))
    one = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[None])
    eng.forward(one(phi0), dts, u=one(u), store=False)
    pq = None if phi_Q_target is None else one(np.asarray(phi_Q_target)[:M + 1])
    box = make_opt(opt, u_min=float(u_min), u_max=float(u_max))
    R = eng.hess_cg(int(k), cg_tol=cg_tol, precond=precond, tol=tol, dt=dts, t_hist=t_grid, opt=box, phi_Q=pq,
                    phi_T=one(phi_T_target), x=x, y=y)
    m, status = int(R["steps"][0]), Engine2D.CG_STATUS[int(R["status"][0])]
    curv = R["curv"][0][np.isfinite(R["curv"][0])]
    return dict(d=eng.cg_vector("x")[0], steps=m, status=status, resid=R["resid"][0, :m].copy(), pred=float(R["pred"][0]),
                rnorm0=float(R["rnorm0"][0]), curv_min=float(curv.min()) if curv.size else float("nan"),
                n_free=int(R["n_free"][0]), p=eng.cg_vector("p")[0] if status == "negcurv" else None)


def sparsity_statistics(u_optimal, r_optimal, kappa: float, tol: float = 1e-6):
    """Counts behind the KKT sparsity check `u* = 0 <=> |r*| <= kappa`: (nodes with |u*| < tol, nodes with
    |r*| <= kappa, nodes where the two predicates agree, nodes in total)."""
    u_is_zero = np.abs(np.ravel(u_optimal)) < tol
    r_is_small = np.abs(np.ravel(r_optimal)) <= kappa
    return int(u_is_zero.sum()), int(r_is_small.sum()), int((u_is_zero == r_is_small).sum()), int(u_is_zero.size)


def verify_sparsity_condition(u_optimal, r_optimal, kappa: float, tol: float = 1e-6):
    """The reference's report (S2:238-297) from `sparsity_statistics`; additionally returns the three percentages
    (sparsity of u*, share of |r*| <= kappa, share of matching nodes) that the reference only prints."""
    n_zero, n_small, n_match, total = sparsity_statistics(u_optimal, r_optimal, kappa, tol)
    pct = tuple(100.0 * k / total for k in (n_zero, n_small, n_match))
    bar = "=" * 60
    print(f"\n{bar}\nVERIFYING SPARSITY CONDITION\nCondition: u*(x,t) = 0  <=>  |r*(x,t)| <= kappa\n{bar}")
    print(f"Sparsity of final control (u* ≈ 0): {pct[0]:.2f}% ({n_zero}/{total} points)")
    print(f"Region where |r*| <= kappa:          {pct[1]:.2f}% ({n_small}/{total} points)")
    print(f"Percentage of points where the conditions match: {pct[2]:.2f}%")
    print("\n✓ The sparsity condition is satisfied." if pct[2] > 99.0 else "\n⚠ The sparsity condition is not fully satisfied.")
    print(bar)
    return pct
