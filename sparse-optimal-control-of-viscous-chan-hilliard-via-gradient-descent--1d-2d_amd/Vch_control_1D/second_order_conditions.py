"""Host-side mirror of src/1D/Vch_control_1D/second_order_conditions.py: finite-difference
coercivity test with the kink-aware critical cone; forward marches and costs run on the GPU.
`approximate_second_order_condition` is the reference's formula, `exact_second_order_condition` gives the exact
second derivative by tangent marches on the device, `reduced_hessian_extremes` the extreme eigenvalues of the reduced
Hessian on the free set by Lanczos on exact Hessian-vector products."""
from __future__ import annotations

import contextlib
import io
from typing import List

import numpy as np

from .Forward_solver import run_main_simulation
from .cost_and_function import calculate_cost
from .config import ForwardSolverConfig


# sign code of a node of the critical cone: FREE keeps the drawn value, +1 / -1 force the sign, 0 pins the component
_FREE = 2


def _cone_sign_codes(u_star, s_star, u_min, u_max, kappa, tol, tol_s):
    """Admissible sign per node of the critical cone of `J + kappa |u|_1` over the box (S1:33-55).

    Rules, later ones overriding earlier ones where they overlap (the reference assigns them in this order):
    lower bound -> +, upper bound -> -, and at the kink u = 0 of the L1 term, with s = r + b3 u the smooth
    gradient: |s| < kappa -> pinned, s >= kappa -> -, s <= -kappa -> + (each with the slack tol_s)."""
    code = np.full(u_star.shape, _FREE, dtype=np.int8)
    kink = np.abs(u_star) <= tol
    for mask, c in ((u_star <= u_min + tol, 1),
                    (u_star >= u_max - tol, -1),
                    (kink & (np.abs(s_star) < kappa - tol_s), 0),
                    (kink & (s_star >= kappa - tol_s), -1),
                    (kink & (s_star <= -kappa + tol_s), 1)):
        code[mask] = c
    return code


def _generate_direction(u_star, r_star, u_min, u_max, kappa, b3, rng, tol=1e-8, tol_s=1e-9):
    """Unit direction in the critical cone incl. the L1 kink at u = 0: ONE `standard_normal` draw of the shape of
    u_star (the only thing the seeded goldens pin), signs imposed by `_cone_sign_codes`; an all-pinned cone falls
    back to the coordinate direction of the largest |r + b3 u|."""
    draw = rng.standard_normal(size=u_star.shape)
    s_star = r_star + b3 * u_star
    code = _cone_sign_codes(u_star, s_star, u_min, u_max, kappa, tol, tol_s)
    v = np.where(code == _FREE, draw, code * np.abs(draw))
    nrm = np.linalg.norm(v)
    if nrm == 0:
        v[np.unravel_index(np.argmax(np.abs(s_star)), s_star.shape)] = 1.0
        nrm = 1.0
    return v / nrm


def _as_generator(source=None):
    """A numpy Generator from a Generator, a seed-like value (anything int() accepts) or nothing; values that
    cannot be read as a seed give an unseeded generator, as the reference's helper does (S1:57-68)."""
    if isinstance(source, np.random.Generator):
        return source
    seed = None
    if source is not None:
        try:
            seed = int(source)
        except (TypeError, ValueError):
            seed = None
    try:
        return np.random.default_rng(seed)
    except (TypeError, ValueError):          # e.g. a negative seed
        return np.random.default_rng()


def approximate_second_order_condition(fwd_config: ForwardSolverConfig, u_star, r_star, phi_star, x, t_hist, b1, b2, b3,
                                       kappa, phi_Q_target, phi_T_target, u_min, u_max, num_directions: int = 10,
                                       epsilon: float = 1e-4, seed=None, rng=None) -> List[float]:
    """S1:71-177."""
    rng = _as_generator(rng if rng is not None else seed)
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())
    with quiet():
        cost_star = calculate_cost(phi_star, u_star, phi_Q_target, phi_T_target, x, t_hist, b1, b2, b3, kappa, verbose=False)
    grad_star = r_star + b3 * u_star
    # all directions first (the same draws in the same order as the reference's loop, S1:137-150), then their perturbed
    # controls marched as one batch of trajectories with one batched cost evaluation
    dirs = [_generate_direction(u_star, r_star, u_min, u_max, kappa, b3, rng) for _ in range(num_directions)]
    costs = _perturbed_costs([u_star + epsilon * h for h in dirs], fwd_config, phi_Q_target, phi_T_target, x, t_hist,
                             b1, b2, b3, kappa)
    return [(cost_p - cost_star - epsilon * np.sum(grad_star * h)) / (0.5 * epsilon ** 2) for h, cost_p in zip(dirs, costs)]


MAX_BATCH = 64


def _perturbed_costs(controls, fwd_config, phi_Q_target, phi_T_target, x, t_hist, b1, b2, b3, kappa):
    """J(u) for every control of the list: `run_main_simulation(fwd_config, control_input=u)` (default start:
    init_phi_random(amp=0.01, seed=42), F1:316) and `calculate_cost`, batched over the controls."""
    from ..engine import time_grid, make_opt
    from ._ctx import engine_for_config
    from .Forward_solver import init_phi_random, delta_sep
    cfg = fwd_config if fwd_config is not None else ForwardSolverConfig()
    N = int(cfg.N)
    _, dts = time_grid(float(cfg.T), float(cfg.dt_initial))
    phi0 = init_phi_random(N, delta_sep, amp=0.01, seed=42, enforce_zero_mean=True)
    opt = make_opt(b1=b1, b2=b2, b3=b3, kappa_sparsity=kappa)
    costs = []
    for k0 in range(0, len(controls), MAX_BATCH):
        chunk = controls[k0:k0 + MAX_BATCH]
        nb = len(chunk)
        U = np.stack(chunk)
        eng = engine_for_config(cfg, batch=nb, max_steps=max(len(dts), 1))
        phi_p, _ = eng.forward(np.broadcast_to(phi0, (nb, N + 1)), dts, u=U, store=True)
        phi_p = phi_p.reshape((nb,) + phi_p.shape[-2:])
        tile = lambda a: np.broadcast_to(a, (nb,) + np.shape(a))
        J = eng.cost(phi_p, U, tile(phi_Q_target), tile(phi_T_target), x, t_hist, opt)
        costs.extend(float(v) for v in np.atleast_2d(J)[:, 4])
    return costs


def exact_second_order_condition(fwd_config: ForwardSolverConfig, u_star, r_star, phi_star, x, t_hist, b1, b2, b3, kappa,
                                 phi_Q_target, phi_T_target, u_min, u_max, num_directions: int = 10, seed=None,
                                 rng=None) -> List[float]:
    """J''(u*)[h,h] of the smooth part J1 + J2 + J3 of the discrete cost, exactly (to the round-off of a direct solve), for
    the same seeded directions as `approximate_second_order_condition` draws (`_generate_direction`, one draw each, in the
    same order).  No difference quotient and no nonlinear march, so there is no `epsilon`: the directions run as one
    shared-base batch about `phi_star` as given, in chunks of MAX_BATCH (Engine1D.second_order: one persistent workgroup
    per direction, two linear solves per step).  Per direction the curvature, the exact slope J'(u*)h and the adjoint's
    unweighted `sum(g h)`, g = r* + b3 u*, that the finite-difference formula subtracts, are printed side by side.

    What differs from the reference's number:
      * the smooth part only: the L1 term J4 has no curvature away from its kink and is left out (the one-sided
        difference of J picks up kappa (|u + eps h| - |u|) wherever u* = 0);
      * the exact slope: the derivative of the discrete cost, not the node sum of the hand-derived adjoint, which in 1D
        also runs on parameters frozen at the defaults (B1:29-33);
      * J'' is the quadrature-weighted second derivative for the unit-Euclidean h: with the cost's trapezoid weights in x
        and t, as J itself is, and not rescaled by `n_h = int int h^2`.
    The clip at the end of a time step is taken as inactive (|phi| < 1 - delta_sep), and a step of the march behind
    `phi_star` that left Newton's loop through the line-search-failure return is not detected."""
    from ..engine import make_opt
    from ._ctx import engine_for_config
    rng = _as_generator(rng if rng is not None else seed)
    cfg = fwd_config if fwd_config is not None else ForwardSolverConfig()
    grad_star = r_star + b3 * u_star
    print(f"Testing {num_directions} random directions in the critical cone (exact tangent marches)...")
    dirs = [_generate_direction(u_star, r_star, u_min, u_max, kappa, b3, rng) for _ in range(num_directions)]
    opt = make_opt(b1=b1, b2=b2, b3=b3, kappa_sparsity=kappa)
    t_hist = np.asarray(t_hist, dtype=np.float64)
    rows = int(t_hist.size)
    out: List[float] = []
    for k0 in range(0, len(dirs), MAX_BATCH):
        chunk = dirs[k0:k0 + MAX_BATCH]
        eng = engine_for_config(cfg, batch=len(chunk), max_steps=max(rows - 2, 1))
        res = eng.second_order(np.stack(chunk), t_hist, opt, phi_hist=phi_star, u=u_star, phi_Q=phi_Q_target,
                               phi_T=phi_T_target, x=x, shared_base=True)
        for i, h in enumerate(chunk):
            d2, slope = float(res["curvature"][i]), float(res["slope"][i])
            out.append(d2)
            print(f"  Direction {k0 + i + 1}/{num_directions}: exact d²J/dh² = {d2:.6e}   exact slope J'h = {slope:.6e}   "
                  f"adjoint sum(g·h) = {np.sum(grad_star * h):.6e}")
    return out


def free_set(u_star, u_min, u_max, tol=1e-8):
    """Nodes where the critical cone is a linear space: strictly inside the box and off the kink of the L1 term, with the
    `tol` of `_cone_sign_codes` (whose rules leave exactly these nodes free whatever the adjoint is)."""
    u_star = np.asarray(u_star)
    return (u_star > u_min + tol) & (u_star < u_max - tol) & (np.abs(u_star) > tol)


def reduced_hessian_extremes(fwd_config: ForwardSolverConfig, u_star, phi_star, x, t_hist, b1, b2, b3, kappa, phi_Q_target,
                             phi_T_target, u_min, u_max, k: int = 30, seed=None, tol: float = 1e-8, on_device: bool = False,
                             vector: bool = False, reorth: bool = True) -> dict:
    """Extreme eigenvalues of the reduced Hessian P H P of the smooth part J1 + J2 + J3 of the discrete cost at `u_star`,
    by host Lanczos with full reorthogonalisation.  H is the exact Euclidean Hessian with respect to the entries of u
    (Engine1D.hessvec: one tangent and two transposed solves per time step, about `phi_star` as given, one call per
    Lanczos step with a shared base point); P masks to the free set `free_set(u_star, u_min, u_max, tol)`.  At most
    min(k, size of the free set) steps; with k >= that size the Ritz values are all eigenvalues of P H P on the free set.

    Returns dict(theta_min, theta_max: the extreme Ritz values; res_min, res_max: their residual norms
    |beta_m s_m| (an eigenvalue of P H P lies within that distance of each); ritz: all Ritz values, ascending; n_free: the
    size of the free set; steps: Lanczos steps taken).  The values are Rayleigh quotients h.Hh / h.h in the Euclidean
    norm of h, the scale of the curvatures `exact_second_order_condition` returns for its unit directions; theta_min is
    not larger than any of those whose direction is supported on the free set.

    What is left out.  The second-order sufficient condition asks for coercivity on the critical cone.  On the free set
    the cone is a linear space and the smallest eigenvalue is the coercivity constant there, which random directions only
    bound from above.  At a node on the kink u* = 0 of kappa |u|_1 the cone admits one sign at most (none where
    |r + b3 u| < kappa), and at a node on the active box it admits the inward sign only: there the cone is a half-line or
    a point per node, the minimum of the quadratic form over it is no eigenvalue problem, and the L1 term adds no
    curvature along an admitted sign.  Those nodes are pinned to zero here, so theta_min bounds the cone's constant from
    above: a cone direction that mixes free and one-signed nodes can still see less curvature.  `kappa` therefore does
    not enter.  The clip of the march is taken as inactive, as in `exact_second_order_condition`.

    on_device=True keeps the iteration on the device (Engine1D.hess_lanczos: the same seeded start vector, the basis and the
    recurrence in device memory, two linear solves per step and time step instead of three); only the tridiagonal matrix
    comes back and its eigh is taken here.  The keys are the same.  reorth=False runs the three-term recurrence with three
    resident vectors (on_device only).  vector=True (on_device with full reorthogonalisation only) adds `v_min`, the unit
    Ritz vector of theta_min in the shape of u_star.  The default path is the host reference."""
    if (vector or not reorth) and not on_device:
        raise ValueError("reduced_hessian_extremes: vector=True and reorth=False need on_device=True")
    if vector and not reorth:
        raise ValueError("reduced_hessian_extremes: vector=True needs full reorthogonalisation")
    from ..engine import make_opt
    from ._ctx import engine_for_config
    cfg = fwd_config if fwd_config is not None else ForwardSolverConfig()
    rng = _as_generator(seed)
    u_star = np.asarray(u_star, dtype=np.float64)
    t_hist = np.asarray(t_hist, dtype=np.float64)
    mask = free_set(u_star, u_min, u_max, tol)
    n_free = int(mask.sum())
    if n_free == 0:
        raise ValueError("reduced_hessian_extremes: the free set is empty")
    opt = make_opt(b1=b1, b2=b2, b3=b3, kappa_sparsity=0.0)
    eng = engine_for_config(cfg, batch=1, max_steps=max(t_hist.size - 2, 1))

    def apply(q):
        res = eng.hessvec(q, t_hist, opt, phi_hist=phi_star, u=u_star, phi_Q=phi_Q_target, phi_T=phi_T_target, x=x,
                          shared_base=True)
        return np.where(mask, res["hv"][0], 0.0)

    q = np.where(mask, rng.standard_normal(u_star.shape), 0.0)
    if on_device:
        box = make_opt(b1=b1, b2=b2, b3=b3, kappa_sparsity=0.0, u_min=float(u_min), u_max=float(u_max))
        L = eng.hess_lanczos(q, int(k), t_hist, box, phi_hist=phi_star, u=u_star, phi_Q=phi_Q_target, phi_T=phi_T_target, x=x,
                             mask=mask, tol=tol, reorth=reorth, shared_base=True)
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


def reduced_newton_step(fwd_config: ForwardSolverConfig, u, x, t_hist, opt_config=None, b1=None, b2=None, b3=None, kappa=None,
                        phi_Q_target=None, phi_T_target=None, u_min: float = -np.inf, u_max: float = np.inf, k: int = 50,
                        cg_tol: float = 1e-8, precond: bool = True, tol: float = 1e-8) -> dict:
    """The Newton step of the full cost J1 + J2 + J3 + J4 on the free set `free_set(u, u_min, u_max, tol)` of the control
    `u`: d solves P H P d = -P (grad(J1+J2+J3) + kappa_sparsity wt wx sign(u)) by (preconditioned) conjugate gradients that
    stay on the device (Engine1D.hess_cg with rhs=None).  On the free set |u| > tol, so the L1 term is smooth there and the
    right-hand side is the exact Euclidean gradient of the full cost; H is the exact Hessian of the smooth part (the L1
    term has no curvature off its kink).  One forward march of u from the default start of `run_main_simulation`, then
    one hess_cg call of at most `k` steps: two linear solves per CG step and time step.  The weights come from
    `opt_config`, or from b1, b2, b3 and kappa (the sparsity parameter) when it is None.  `precond` scales by the L2(Q)
    mass diag(wt wx) of the control, row 0 taking the time weight of row 1.

    Returns dict(d: the step, zero off the free set; steps; status: "converged", "limit", "negcurv" or "breakdown";
    resid: the relative residuals of the steps taken; pred: the decrease the quadratic model predicts for the full step;
    rnorm0: the Euclidean norm of the right-hand side; curv_min: the smallest curvature p.Hp / p.Dp seen; n_free; p: the
    direction of non-positive curvature when the status is "negcurv", else None).  With "negcurv" d is the iterate before
    that direction (zero when the first direction already has non-positive curvature)."""
    from ..engine import time_grid, make_opt, Engine1D
    from ._ctx import engine_for_config
    from .Forward_solver import init_phi_random, delta_sep
    if fwd_config is None:
        raise ValueError("reduced_newton_step: fwd_config is required (the grid and the time steps of the march of u)")
    if opt_config is None and None in (b1, b2, b3, kappa):
        raise ValueError("reduced_newton_step: give opt_config, or all of b1, b2, b3 and kappa")
    cfg = fwd_config
    over = {n: v for n, v in (("b1", b1), ("b2", b2), ("b3", b3), ("kappa_sparsity", kappa)) if v is not None}
    box = make_opt(opt_config, u_min=float(u_min), u_max=float(u_max), **over)
    _, dts = time_grid(float(cfg.T), float(cfg.dt_initial))
    M = len(dts)
    t_hist = np.asarray(t_hist, dtype=np.float64)
    if t_hist.size != M + 2:
        raise ValueError(f"reduced_newton_step: t_hist must have the march's {M + 2} rows, got {t_hist.size}")
    u = np.asarray(u, dtype=np.float64)[:M + 2]
    phi0 = init_phi_random(int(cfg.N), delta_sep, amp=0.01, seed=42, enforce_zero_mean=True)
    eng = engine_for_config(cfg, batch=1, max_steps=max(M, 1))
    one = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64)[None])
    eng.forward(one(phi0), dts, u=one(u), store=False)
    R = eng.hess_cg(int(k), t_hist, box, cg_tol=cg_tol, precond=precond, tol=tol, u=one(u),
                    phi_Q=None if phi_Q_target is None else one(np.asarray(phi_Q_target)[:M + 2]), phi_T=one(phi_T_target),
                    dt=dts, x=x)
    m, status = int(R["steps"][0]), Engine1D.CG_STATUS[int(R["status"][0])]
    curv = R["curv"][0][np.isfinite(R["curv"][0])]
    return dict(d=eng.cg_vector("x")[0], steps=m, status=status, resid=R["resid"][0, :m].copy(), pred=float(R["pred"][0]),
                rnorm0=float(R["rnorm0"][0]), curv_min=float(curv.min()) if curv.size else float("nan"),
                n_free=int(R["n_free"][0]), p=eng.cg_vector("p")[0] if status == "negcurv" else None)
