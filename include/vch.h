/* vch.h — C ABI of the MI355X-native viscous Cahn–Hilliard optimal-control engine.
 *
 * This is the drop-in boundary for the reference's hot path.  The
 * reference (a pure-Python research code) has no FFI layer: its seams are Python
 * function calls between sibling modules.  Each entry point below replaces one of
 * those functions; the file:line of the replaced interface is cited per function
 * (paths relative to the reference root):
 *   F2 = src/2D/Vch_control_2D/Forward2_solver.py    B2 = src/2D/Vch_control_2D/backward2_solver.py
 *   C2 = src/2D/Vch_control_2D/cost2_and_function.py G2 = src/2D/Vch_control_2D/GD2_configured.py
 *   K2 = src/2D/Vch_control_2D/config.py
 *   F1 = src/1D/Vch_control_1D/Forward_solver.py     B1 = src/1D/Vch_control_1D/backward_solver.py
 *   C1 = src/1D/Vch_control_1D/cost_and_function.py  G1 = src/1D/Vch_control_1D/GD_1D.py
 *
 * Conventions
 *  - plain C, no torch types; every array argument is a HOST pointer to caller-owned,
 *    C-contiguous float64 memory unless the name ends in `_dev`.  The engine never
 *    frees or keeps caller memory.
 *  - a context owns one GPU's device buffers, stream and batch of B independent
 *    trajectories; all calls on it are synchronous and must come from one host thread.
 *  - 2D fields are (Nx+1, Ny+1) row-major, y fastest (the reference's layout); batched
 *    arguments are [B][...]; histories are [B][rows][Nx+1][Ny+1].
 *  - return value: 0 on success, negative on error; vch_last_error() describes the last
 *    failure of the calling thread.  Newton non-convergence is NOT an error (F2:427).
 */
#ifndef VCH_H
#define VCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VCH_OK 0
#define VCH_ERR_ARG (-1)      /* bad argument / shape (the reference raises ValueError / AssertionError) */
#define VCH_ERR_HIP (-2)      /* HIP runtime failure */
#define VCH_ERR_STATE (-3)    /* call order (e.g. backward before forward with resident history) */
#define VCH_ERR_NOMEM (-4)

const char *vch_last_error(void);
/* Library build/ABI version, and number of visible HIP devices (<0 on error). */
int vch_abi_version(void);
int vch_device_count(void);

/* ------------------------------------------------------------------ 2D ---- */

/* Physical parameters = the fields of ForwardSolverConfig (K2:103-113). */
typedef struct vch2d_params {
    int32_t Nx, Ny;
    double Lx, Ly;
    double tau, gamma, c1, c2, kappa;
} vch2d_params;

/* Weights/bounds = the fields of OptimizationConfig (K2:137-144). */
typedef struct vch_opt_params {
    double b1, b2, b3, kappa_sparsity;
    double alpha_max;
    int32_t max_iter;
    double u_min, u_max;
} vch_opt_params;

/* Solver statistics of one forward march / backward sweep (per trajectory sums). */
typedef struct vch_stats {
    int64_t newton_iters;      /* residual evaluations that entered the Newton loop (len(hist)) */
    int64_t linear_solves;     /* Newton linear solves (spsolve calls in the reference, F2:370) */
    int64_t linear_iters;      /* preconditioned CG iterations spent in them */
    int64_t armijo_trials;     /* residual evaluations in the Armijo loop (F2:398-419) */
    double  max_lin_relres;    /* worst final relative residual of a linear solve */
    double  seconds;           /* device time of the call (HIP events) */
    /* ABI version 2 */
    double  max_lin_absres;    /* worst (final relative residual x ||rhs||_2) of a Newton linear solve: the estimate of
                                  the Schur residual it leaves, which the inexact-Newton rule of a march keeps at
                                  5 % of the Newton tolerance */
    int64_t host_syncs;        /* blocking looks of the host at the device state during the call */
    int64_t launches;          /* kernel launches of the call */
    /* ABI version 3 (a caller must check vch_abi_version() >= 3 before passing a vch_stats: the library writes all fields) */
    int64_t unconverged_solves; /* adjoint solves that the speculative schedule's sweeps did not finish (each ended below
                                  10 x the solve tolerance, or the whole sweep was repeated with the rigorous budget) */
} vch_stats;

typedef struct vch2d_ctx vch2d_ctx;

/* Create a context for `batch` trajectories and marches of at most `max_steps` steps on
 * HIP device `device`.  History buffers are allocated lazily by the calls that need them.
 * Up to 32 trajectories, each one chooses the starting guesses of its march and adjoint solves
 * from its own history, so a trajectory's results are bit for bit those of a single-trajectory
 * context.  Above 32, the batch shares one guess policy, fed by its worst trajectory: results
 * are still correct to the solvers' tolerance, but no longer bitwise equal to single runs. */
vch2d_ctx *vch2d_create(const vch2d_params *p, int batch, int max_steps, int device);
void vch2d_destroy(vch2d_ctx *ctx);
int vch2d_batch(const vch2d_ctx *ctx);
/* 1 when the DCT preconditioner runs as in-LDS FFTs (both Nx, Ny powers of two in 16..2048),
 * 0 when it runs as MFMA f64 matrix products (any grid size). */
int vch2d_uses_fft(const vch2d_ctx *ctx);

/* -- discrete operators (kernel-level parity tests; each replaces one reference helper) -- */

/* out = L v, mirrored-Neumann 5-point Laplacian incl. the reference's Kronecker-order
 * quirk for Nx != Ny.  Replaces apply_laplacian (F2:140-152).  v,out: [B][Nx+1][Ny+1]. */
int vch2d_apply_laplacian(vch2d_ctx *ctx, const double *v, double *out);
/* mu = -kappa L phi + c1 reglog(phi) - 2 c2 phi - w.  Replaces initialize_mu (F2:155-167). */
int vch2d_initialize_mu(vch2d_ctx *ctx, const double *phi, const double *w, double *mu_out);
/* Crank–Nicolson filter step.  Replaces solve_w (F2:170-181).  u_n/u_np1 may be NULL (zeros). */
int vch2d_solve_w(vch2d_ctx *ctx, const double *w_old, double dt, const double *u_n,
                  const double *u_np1, double *w_out);
/* [R_phi; R_mu].  Replaces solve_phi_residual + solve_mu_residual (F2:184-221). */
int vch2d_residuals(vch2d_ctx *ctx, const double *phi_new, const double *phi_old,
                    const double *mu_new, const double *mu_old, const double *w_new,
                    const double *w_old, double dt, double *Rphi_out, double *Rmu_out,
                    double *norm_out /* [B], may be NULL */);
/* (out_phi, out_mu) = J(phi_new) [dphi; dmu], matrix-free.  Replaces
 * assemble_jacobian(...) @ v (F2:224-253). */
int vch2d_jacobian_apply(vch2d_ctx *ctx, const double *phi_new, double dt, const double *dphi,
                         const double *dmu, double *out_phi, double *out_mu);
/* Solve J(phi_new) [dphi; dmu] = [rhs_phi; rhs_mu].  Replaces spsolve(J.tocsc(), -R)
 * (F2:370): Schur reduction to the scalar 13-point system + DCT-I preconditioned
 * conjugate gradients in the weighted inner product.  stats may be NULL. */
int vch2d_jacobian_solve(vch2d_ctx *ctx, const double *phi_new, double dt, const double *rhs_phi,
                         const double *rhs_mu, double *dphi, double *dmu, vch_stats *stats);
/* out = (I/dt + M(kappa/2 M + D)) x, the Schur-reduced Newton operator (M = -L). */
int vch2d_schur_apply(vch2d_ctx *ctx, const double *phi_new, double dt, const double *x,
                      double *out);
/* out = A(phi) v (which=0) or B(phi) v (which=1).  Replaces A_adjoint/B_adjoint @ v
 * (B2:195-203). */
int vch2d_adjoint_apply(vch2d_ctx *ctx, int which, const double *phi, double dt, const double *v,
                        double *out);
/* Solve A(phi_n) p = rhs.  Replaces spsolve(A, rhs) (B2:229); dt = 0 gives the terminal
 * solve (I - tau L) p = rhs (B2:184-185). */
int vch2d_adjoint_solve(vch2d_ctx *ctx, const double *phi_n, double dt, const double *rhs,
                        double *p_out, vch_stats *stats);
/* out = (c0 + m (c1 + c2 m))^{-1} v by fast diagonalisation (DCT-I), m = eigenvalues of
 * -L: the preconditioner itself, exposed for tests. */
int vch2d_spectral_solve(vch2d_ctx *ctx, double c0, double c1, double c2, const double *v,
                         double *out);

/* One implicit time level.  Replaces newton_raphson (F2:323-427): same initial guess,
 * stop rule (||R||_2 < 1e-6, <= 500 its), step ceiling and Armijo rule.
 * hist: [B][hist_cap] residual norms (return_residual_history), n_hist: [B]; may be NULL. */
int vch2d_newton_raphson(vch2d_ctx *ctx, const double *phi_old, const double *mu_old,
                         const double *w_old, const double *w_new, double dt, double *phi_new,
                         double *mu_new, double *hist, int hist_cap, int32_t *n_hist,
                         vch_stats *stats);

/* -- the time march and the adjoint sweep -- */

/* Forward march.  Replaces run_main_simulation (F2:489-596) for B trajectories at once.
 *   phi0   [B][Nx+1][Ny+1]  initial states (the reference hard-codes init_phi_random(seed=42), F2:517)
 *   u      [B][u_rows][Nx+1][Ny+1] control or NULL; rows (step, step+1) are used while
 *          step < u_rows-1, zeros afterwards (F2:545-548).  u == VCH_RESIDENT uses the
 *          control currently resident in the context (PGD state).
 *   dt     [M] step sizes, as produced by the reference's accumulated-time rule (F2:542-543)
 *   phi_hist_out [B][M+1][Nx+1][Ny+1] or NULL (history stays resident on the device)
 * The history (and mu, w at the final level) stays resident for vch2d_backward/vch2d_cost. */
int vch2d_forward(vch2d_ctx *ctx, const double *phi0, const double *u, int u_rows,
                  const double *dt, int M, double *phi_hist_out, vch_stats *stats);

/* Adjoint sweep.  Replaces run_backward (B2:75-246).
 *   phi_hist [B][M+1][..] or NULL = use the resident history of the last forward call
 *   t_hist [M+1]; phi_Q [B][M+1][..] or NULL (zeros, B2:167); phi_T [B][..] or NULL
 *   hx, hy = x[1]-x[0], y[1]-y[0] as the reference takes them (B2:154-155)
 *   p_out, q_out, r_out [B][M+1][..], each may be NULL (r stays resident for the prox). */
int vch2d_backward(vch2d_ctx *ctx, const double *phi_hist, int M, const double *t_hist, double hx,
                   double hy, double b1, double b2, const double *phi_Q, const double *phi_T,
                   double *p_out, double *q_out, double *r_out, vch_stats *stats);

/* J1..J4 and their sum.  Replaces calculate_cost (C2:19-120).  NULL array arguments use the
 * resident state (history of the last forward, resident control and targets).
 *   x [Nx+1], y [Ny+1], t_hist [M+1]; J_out [B][5] = {J1, J2, J3, J4, J}. */
int vch2d_cost(vch2d_ctx *ctx, const double *phi_hist, const double *u, const double *phi_Q,
               const double *phi_T, int M, const double *x, const double *y, const double *t_hist,
               const vch_opt_params *opt, double *J_out);

/* u_out = clip(soft_threshold(u - alpha (r + b3 u), alpha kappa_s), u_min, u_max).
 * Replaces calculate_gradient + proximal_step (C2:123-200).  rows = leading dimension of the
 * histories; alpha [B]. */
int vch2d_grad_prox(vch2d_ctx *ctx, const double *u, const double *r, int rows, const double *alpha,
                    const vch_opt_params *opt, double *u_out);

/* -- device-resident proximal-gradient loop (G2:291-382) -- */

/* Load the optimisation problem: initial states, targets, time grid; u^0 = 0; runs the
 * uncontrolled forward march and evaluates J(u^0) (G2:255-292).
 *   phi_Q == NULL and ramp != 0: phi_Q = (1 - t/T) phi0 + (t/T) phi_T evaluated on the
 *   fly with t/T from the config T (build_targets choice_q = 1, G2:221-222). */
int vch2d_pgd_init(vch2d_ctx *ctx, const double *phi0, const double *phi_T, const double *phi_Q,
                   int ramp, double T, const double *t_hist, int M, const double *x, const double *y,
                   const vch_opt_params *opt, double *J0_out /* [B][5] */);
/* The same with one parameter set PER TRAJECTORY, a warm start and a first step size (ABI version stays 3: detect this
 * entry point and vch2d_pgd_kkt by symbol).  vch2d_pgd_init is this call with n_opts = 1 and u0 = alpha0 = NULL.
 *   opts    n_opts parameter sets, n_opts = 1 (one set for the whole batch) or B (trajectory b takes opts[b]); anything
 *           else is VCH_ERR_ARG.  Trajectory b's own values are used everywhere in the loop: b1 in the adjoint source, b2
 *           in the terminal condition, b3 / kappa_sparsity / u_min / u_max in the gradient + prox step, the four weights
 *           in the cost, alpha_max in the growth and plateau rules.  They live in a [B] table on the device that the
 *           kernels index by trajectory; a kernel's arithmetic is that of the scalar form, so a trajectory computes the
 *           same bits as in a single-trajectory context with its parameters (batches up to 32, see vch2d_create).
 *           VCH_ERR_ARG, with a message that names the trajectory, before anything is launched: non-finite b1, b2, b3 or
 *           kappa_sparsity, kappa_sparsity < 0, alpha_max <= 0, u_min > u_max (infinite bounds are legal).
 *   u0      [B][M+1][Nx+1][Ny+1] start control or NULL (zeros).  Taken as given, NOT clipped to the box: the initial
 *           march runs under it and J0_out is its cost under each trajectory's own weights.
 *   alpha0  [B] or NULL.  NULL: the first alpha_prev is each trajectory's alpha_max (G2:293); otherwise alpha0[b] (finite,
 *           > 0), capped at that trajectory's alpha_max.
 * The iteration counter (the k of the stop rule `change < 1e-5 and k > 20`) and the plateau counter start at 0 as after
 * vch2d_pgd_init, also under a warm start: a resumed run is a new run from u0, it does not inherit the saved run's k.
 * max_iter is not read: the loop length is the n_iters of vch2d_pgd_iterate. */
int vch2d_pgd_init_v(vch2d_ctx *ctx, const double *phi0, const double *phi_T, const double *phi_Q,
                     int ramp, double T, const double *t_hist, int M, const double *x, const double *y,
                     const vch_opt_params *opts, int n_opts, const double *u0 /* or NULL */,
                     const double *alpha0 /* [B] or NULL */, double *J0_out /* [B][5] */);
/* Run n_iters PGD iterations for every trajectory of the batch (optimistic step,
 * backtracking from 0.8 alpha_prev with beta 0.8 and <= 10 trials, alpha growth / plateau
 * rule, stop rule; G2:295-382).  Outputs [B][n_iters] unless noted; any may be NULL.
 *   cost_out      accepted cost after each iteration
 *   alpha_out     step used
 *   attempts_out  backtracking forwards (0 = optimistic step accepted)
 *   change_out    relative control change
 *   seconds_out   [5] time buckets {backward, grad+prox, optimistic forward, cost, backtracking}
 * Returns the number of iterations performed (>= 0) or a negative error. */
int vch2d_pgd_iterate(vch2d_ctx *ctx, int n_iters, double *cost_out, double *alpha_out,
                      int32_t *attempts_out, double *change_out, double *seconds_out);
/* Error metrics the driver appends after every iteration (G2:336-363), for the iterations of the LAST
 * vch2d_pgd_iterate call ([B][n_iters], n_iters as passed there; NaN where no iteration ran):
 *   tracking = ||phi - phi_Q||_L2(Q) / ||phi_Q||_L2(Q)  (denominator sqrt(|Omega| T) when ||phi_Q|| < 1e-9 of it)
 *   terminal = ||phi(T) - phi_T||_L2(Omega) / ||phi_T||_L2(Omega)
 * both from the cost kernel's weighted sums (nested trapezoid rule in y, x, t).  Either output may be NULL. */
int vch2d_pgd_errors(vch2d_ctx *ctx, int n_iters, double *tracking_out, double *terminal_out);
/* Copy resident PGD arrays to the host: what = 0 control u, 1 state history, 2 adjoint r,
 * 3 phi_Q.  out [B][M+1][Nx+1][Ny+1]. */
int vch2d_pgd_get(vch2d_ctx *ctx, int what, double *out);
/* KKT sparsity statistic `u* = 0 <=> |r*| <= kappa_sparsity` of the resident iterate, counted on the device (replaces
 * pulling u and r through vch2d_pgd_get for sparsity_statistics / verify_sparsity_condition, S2:238-297; only 3 B integers
 * cross to the host).
 *   counts_out[b] = { #nodes |u| < tol, #nodes |r| <= kappa_sparsity of trajectory b, #nodes where the two predicates
 *                     agree, #nodes } over all (M+1)(Nx+1)(Ny+1) nodes of trajectory b; tol <= 0 means 1e-6.
 *   refresh != 0  first runs the adjoint sweep on the resident state (each trajectory's own b1, b2; the accuracy of
 *                 vch2d_backward), as the reference's main() does with run_backward after the loop (G2:424).  The result
 *                 stays in the resident r; the next vch2d_pgd_iterate recomputes it anyway.
 *   refresh == 0  uses the resident r as it is: the adjoint the last iteration started from, i.e. that of the iterate
 *                 BEFORE the last accepted step.  VCH_ERR_STATE if no sweep has run since vch2d_pgd_init.
 *   stationarity_out[b] (or NULL) = ||prox_1(u) - u||_2 / (||u||_2 + 1e-9): prox_1 is the gradient + prox step with
 *                 alpha = 1 and trajectory b's parameters, written to the trial-control scratch.
 * The control, the state history and the loop's bookkeeping are not touched: with refresh == 0 the following iterations
 * are bit for bit those of an uninterrupted run.  VCH_ERR_STATE before vch2d_pgd_init.  Launches and looks are counted
 * by vch2d_counters like those of any other call. */
int vch2d_pgd_kkt(vch2d_ctx *ctx, int refresh, double tol, int64_t *counts_out /* [B][4] */,
                  double *stationarity_out /* [B] or NULL */);
/* Exact first and second directional derivatives of the smooth part J1 + J2 + J3 of the cost along h, about the resident
 * control and state history (ABI version stays 3: detect this entry point by symbol).  No adjoint and no nonlinear march:
 * the derivative of one Crank-Nicolson / Newton time level with respect to its inputs is one linear solve with the Newton
 * matrix J(phi*) of vch2d_jacobian_apply at the converged new level, its second derivative one more solve with the
 * same matrix.  phi* is the Newton solution of step n before the march's interior mass fix subtracted the
 * shift s_n (vch2d_mass_shifts) on its set I_n (the interior nodes |phi_c| < 1 - delta_sep - 5e-3 of the clipped solution;
 * every node in the all-node form): phi* = phi_{n+1} + s_n on I_n, phi_{n+1} on the nodes the fix skipped.  With dphi_0 = dmu_0 = dw_0 = 0 and d2phi_0 = d2mu_0 = 0, per step n:
 *   dw'  = ((gamma/dt - 1/2) dw + 1/2 (h_{n+1} + h_n)) / (gamma/dt + 1/2)
 *   J [dphi*; dmu']   = [ tau dphi/dt + kappa/2 L dphi + 2 c2 dphi + 1/2 dmu + 1/2 (dw' + dw) ;  dphi/dt + 1/2 L dmu ]
 *   J [d2phi*; d2mu'] = [ tau d2phi/dt + kappa/2 L d2phi + 2 c2 d2phi + 1/2 d2mu - c1 rho(phi*) (dphi*)^2 ;
 *                         d2phi/dt + 1/2 L d2mu ],      rho(p) = 4 p / (1 - p^2)^2
 *   dphi' = dphi* - sum(wts dphi*) / W_int,   d2phi' = d2phi* - sum(wts d2phi*) / W_int      (on I_n, where s_n != 0)
 * The mass fix is linearised: the linearised step conserves the mass of dphi only in the weights of the Laplacian (its
 * Kronecker-order quirk), which are the fix's weights wts = hx hy outer(trapz_x, trapz_y) only for Nx == Ny.  The weighted
 * mean leaves the nodes of I_n (W_int their weight, as the march recorded it); dmu' and dw' are carried as they are.
 * Nodes outside the interior band are linearised exactly or REFUSED: the march keeps s_n and W_int but not I_n, and the call
 * takes a node for interior where |phi_{n+1} + s_n| < 1 - delta_sep - 5e-3.  A skipped node within |s_n| of that threshold
 * passes too; the classified weight then differs from W_int (by more than n eps, n nodes; checked in both directions)
 * and the call returns VCH_ERR_STATE with
 * "trajectory b, step n: interior set of the mass fix not recoverable ..." in vch_last_error (outputs are then undefined,
 * the context stays usable and unchanged).  The end-of-step clip is taken as the identity (inactive wherever
 * |phi| < 1 - delta_sep); an ACTIVE CLIP IS STILL NOT DETECTED.  Behind a state history the caller uploaded (vch2d_backward, vch2d_cost,
 * vch2d_free_energy) there is no march of this context and the shifts count as zero.  The L1 term J4 has no curvature away
 * from its kink and is left out.
 *   h       [B][h_rows][Nx+1][Ny+1] direction, row rule of a control: rows (n, n+1) drive step n while n < h_rows-1, zeros
 *           afterwards (F2:545-548); in the integrals h counts as zero from row h_rows on
 *   out[b] = { s_state = b1 int int (phi - phi_Q) dphi + b2 int (phi_M - phi_T) dphi_M,   s_ctrl = b3 int int u h,
 *              c_gn    = b1 int int dphi^2 + b2 int dphi_M^2,
 *              c_state = b1 int int (phi - phi_Q) d2phi + b2 int (phi_M - phi_T) d2phi_M,
 *              c_ctrl  = b3 int int h^2,   n_h = int int h^2 }
 *           with the cost's nested trapezoid rule in y, x, t and trajectory b's own b1, b2, b3 (n_opts = 1: one set for
 *           the batch; B: opts[b]; nothing else of opts is read):  J'(u) h = s_state + s_ctrl,
 *           J''(u)[h,h] = c_gn + c_state + c_ctrl.  order = 1 skips the second march; c_state is then NaN.
 *   rtol    relative residual at which the linear solves stop (<= 0: 1e-12); every trajectory is gated by its own solve, and
 *           one whose right-hand side is exactly zero (h == 0) gets exact zeros
 *   dphi_hist_out, d2phi_hist_out  [B][M+1][Nx+1][Ny+1] or NULL: the tangent fields, copied level by level (they are not
 *           kept on the device); d2phi_hist_out is written at level 0 only when order = 1
 * After vch2d_forward: dt, t_hist, x, y are required; phi_Q / phi_T NULL are zeros (as in vch2d_cost); the control is the one
 * that march ran under.  After vch2d_pgd_init / _iterate the call works about the current iterate (what vch2d_pgd_get(0 / 1)
 * return): dt, t_hist, x, y may be NULL (the problem's; x, y if given must equal them) and phi_Q, phi_T must be NULL (the
 * problem's targets).  VCH_ERR_STATE without a resident state history; VCH_ERR_ARG for M != the history's steps, n_opts not
 * 1 or B, order not 1 or 2, h_rows outside 1..max_steps+1, non-finite b1, b2, b3 -- all before anything is launched.
 * The control, the state history, the adjoint and the PGD bookkeeping are not touched (the direction goes through the
 * trial-control scratch): a following vch2d_pgd_iterate is bit for bit that of an uninterrupted run.  Up to 32 trajectories,
 * a trajectory's six scalars are bitwise those of a single-trajectory context.  stats (or NULL): launches, looks, linear
 * solves and iterations, device seconds of the call. */
int vch2d_second_order(vch2d_ctx *ctx, const double *h, int h_rows, const double *dt, int M,
                       const double *t_hist, const double *x, const double *y,
                       const double *phi_Q, const double *phi_T,          /* NULL: resident targets (PGD) */
                       const vch_opt_params *opts, int n_opts,            /* 1 or B; only b1,b2,b3 are read */
                       int order /* 1 or 2 */, double rtol,
                       double *out /* [B][6] */,
                       double *dphi_hist_out, double *d2phi_hist_out      /* [B][M+1][..] or NULL */,
                       vch_stats *stats);
/* What the interior mass fix subtracted at the end of every step of the march behind the resident state history (F2:567-577;
 * 0 where the fix was not applied), read-only: out[b][n] = s_n of trajectory b.  The march records it beside the history it
 * writes (a PGD line-search trial's record follows its history on acceptance); vch2d_second_order linearises the fix about
 * it.  Returns M, the steps of that history.  ABI version stays 3: detect this entry point by symbol.  VCH_ERR_STATE without a resident state history that
 * vch2d_forward or vch2d_pgd_init / _iterate of this context wrote. */
int vch2d_mass_shifts(vch2d_ctx *ctx, double *out /* [B][M] */);
/* Exact gradient field and Hessian-vector product of the smooth part J1 + J2 + J3 of the DISCRETE cost about the resident
 * control and state history: the transposed sweep of vch2d_second_order's tangent march (ABI version stays 3:
 * detect this entry point by symbol).  grad = d(J1+J2+J3)/du and hv = H h are Euclidean fields: J'(u) h = sum grad . h and
 * J''(u)[h,h] = sum h . hv are plain node sums, the s_state + s_ctrl and c_gn + c_state + c_ctrl of vch2d_second_order
 * (the reference's hand-derived adjoint r + b3 u is not this field: it carries no quadrature weights and ignores the mass
 * fix).  The Newton matrix obeys J^T = S J S^-1 with S = diag(-(2/dt) wq, wq), wq the trapezoid weights of the plane as
 * stored, so every transposed solve is the tangent's own solve between two diagonal scalings: one solve per step for the
 * gradient, and for H h one tangent solve, one gradient solve and one more transposed solve per step (3 M per trajectory).
 * The linearised mass fix enters by its transpose, the clip is taken as the identity, and a state history whose interior
 * set of the mass fix is not recoverable is refused with VCH_ERR_STATE (all as in vch2d_second_order).
 *   h        [B][h_rows][Nx+1][Ny+1] direction (row rule of a control) or NULL (allowed iff order 1)
 *   g_rows   rows of the control the gradient refers to: M + 1 about a resident PGD iterate; min(rows of the control, M + 1)
 *            after vch2d_forward with a control; any of 1..M+1 after a forward without one (the zero control of that many
 *            rows gives the same march).  Rows (k, k+1) take part in step k only while k < rows - 1 (F2:545-548), so
 *            sum grad . h equals vch2d_second_order's slope exactly when h_rows == g_rows.
 *   order    1: gradient only; 2: gradient and H h
 *   rtol     relative residual at which the linear solves stop (<= 0: 1e-12)
 *   grad_out [B][g_rows][Nx+1][Ny+1] or NULL;  hv_out [B][h_rows][Nx+1][Ny+1], required iff order 2
 *   dots_out [B][2] or NULL: { sum grad . h over the rows both have, sum h . hv }, NaN where a factor is missing
 * Base point, dt, t_hist, x, y, phi_Q, phi_T, opts / n_opts: the rules of vch2d_second_order, in both of its modes; the state
 * history must be one a march of this context wrote (VCH_ERR_STATE otherwise: the shifts would be unknown).  VCH_ERR_ARG
 * also for a g_rows that breaks the rule above, NULL h or NULL hv_out at order 2.  Every error is returned before anything
 * is enqueued, copied or allocated; a failed lazy allocation returns VCH_ERR_NOMEM with the context usable and unchanged.
 * Device storage, allocated on first use, history layout [B][max_steps+1][plane]: grad, and for order 2 hv, the raw
 * tangent solves v_k and the tangent after the mean removal -- four histories beyond the direction (the trial-control
 * scratch), 16.8 GB each at 512^2 x 1000 steps x 8 trajectories.
 * Stateless like vch2d_second_order: the control, the state history, the adjoint, the shift record, the PGD bookkeeping and
 * the solver tolerance are left as found; a following vch2d_pgd_iterate is bit for bit that of an uninterrupted run.  No
 * atomics: up to 32 trajectories, a trajectory's outputs are bitwise those of a single-trajectory context, and h == 0 gives
 * hv exactly zero.  stats (or NULL): launches, looks, linear solves (B M for order 1, 3 B M for order 2) and iterations, the
 * worst final relative residual, device seconds of the call. */
int vch2d_hessvec(vch2d_ctx *ctx, const double *h /* NULL allowed iff order 1 */, int h_rows, int g_rows,
                  const double *dt, int M, const double *t_hist, const double *x, const double *y,
                  const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts,
                  int order /* 1: gradient; 2: gradient and H h */, double rtol,
                  double *grad_out /* [B][g_rows][Nx+1][Ny+1] or NULL */,
                  double *hv_out   /* [B][h_rows][Nx+1][Ny+1], required iff order 2 */,
                  double *dots_out /* [B][2] or NULL */,
                  vch_stats *stats);
/* Lanczos on the reduced Hessian P H P of J1 + J2 + J3 about the resident control and state history, with the basis, the free
 * set and the three-term recurrence in device memory (ABI version stays 3: detect both entry points by
 * symbol).  H q comes from the transposed sweeps of vch2d_hessvec; P masks to the free set.  Only the tridiagonal
 * coefficients cross to the host: T = tridiag(beta, alpha, beta) of a trajectory has the Ritz values of P H P.
 *   Base point, dt, M, t_hist, x, y, phi_Q, phi_T, opts / n_opts, rtol: the rules of vch2d_hessvec, in both of its modes.  The
 *   direction has M + 1 rows, so after a vch2d_forward with a control that control must have at least M + 1 rows
 *   (VCH_ERR_ARG otherwise).  Beyond b1, b2, b3 the call reads u_min, u_max of opts[b].
 *   mask     [B][M+1][Nx+1][Ny+1] bytes, non-zero = free; NULL: built on the device from the resident control with
 *            trajectory b's own box, u > u_min + tol && u < u_max - tol && |u| > tol (tol <= 0: 1e-8)
 *   q0       [B][M+1][Nx+1][Ny+1] start vector; q_0 = P q0 / ||P q0||
 *   k        steps at most; trajectory b stops after min(k, n_free_b) steps, when beta_j <= 1e-14 max_i |alpha_i| (an
 *            invariant subspace) or when beta_j is not finite; a stopped trajectory's vectors are left alone, the others go on
 *   reorth   1: classical Gram-Schmidt, twice, against all of q_0 .. q_j (k + 1 resident vectors); 0: the same two rounds
 *            against q_{j-1}, q_j only (three resident vectors)
 *   alpha_out, beta_out [B][k]: alpha_j = the sum of the two rounds' coefficients on q_j, beta_j = ||w|| after both rounds;
 *            entries beyond steps_out[b] are NaN.  n_free_out[b]: the size of the free set, counted on the device.
 * The gradient sweep's multipliers are computed once, before step 0 (M solves per trajectory), and kept in one further
 * history; every step then runs the tangent march of q_j and the second transposed sweep only: 2 M solves per trajectory
 * and step instead of vch2d_hessvec's 3 M, with the bits of vch2d_hessvec's hv (VCH_KRYLOV_NOCACHE=1 repeats the gradient
 * sweep in every step: A/B and tests).  The host looks once for the size of the free set, once for ||P q0|| and once per
 * step (B betas and stop cells), beside the looks of the solves.
 * Errors: VCH_ERR_ARG for k < 1, NULL q0 or outputs, reorth outside 0 / 1 and the row rule, VCH_ERR_STATE as for
 * vch2d_hessvec -- all before anything is enqueued, copied or allocated.  Two errors depend on the data and come later, both
 * VCH_ERR_ARG naming the trajectory: an empty free set (after the mask launch, its sum and one look; nothing else has run),
 * and a start vector that vanishes on the free set.  Device storage, allocated on first use as one group: the basis (k + 1
 * or 3 histories), one history for the cached sweep, the mask (one byte per node of a history) and the partials; a refused
 * request releases what the call got and returns VCH_ERR_NOMEM with the context usable and unchanged and a message that
 * states the bytes the group needs (at 512^2 x 1000 steps x 8 trajectories a history is 16.8 GB: use reorth = 0 there).
 * Stateless like vch2d_hessvec (the direction goes through the trial-control scratch); no atomics: up to 32 trajectories, a
 * trajectory's alpha, beta and steps are bitwise those of a single-trajectory context, whatever its batch mates do.
 * stats: linear solves B M (2 s + 1) for a batch whose members all take s steps. */
int vch2d_hess_lanczos(vch2d_ctx *ctx, const double *dt, int M, const double *t_hist, const double *x, const double *y,
                       const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts, double rtol,
                       const uint8_t *mask /* [B][M+1][Nx+1][Ny+1] or NULL */, double tol,
                       const double *q0 /* [B][M+1][Nx+1][Ny+1] */, int k, int reorth /* 0 | 1 */,
                       double *alpha_out /* [B][k] */, double *beta_out /* [B][k] */,
                       int32_t *steps_out /* [B] */, int64_t *n_free_out /* [B] */, vch_stats *stats);
/* out[b] = sum_{j<m} coef[b][j] q_j from the basis the last vch2d_hess_lanczos of this context left resident: the Ritz vector
 * of a Ritz value (coef = an eigenvector of T), or one basis vector (a unit coef).  Masked-off nodes are exact zeros.
 * VCH_ERR_STATE without a resident basis, and after a reorth = 0 run when m exceeds the vectors still held; VCH_ERR_ARG for
 * m < 1 or m above the smallest step count of the batch plus one. */
int vch2d_krylov_vector(vch2d_ctx *ctx, const double *coef /* [B][m] */, int m, double *out /* [B][M+1][Nx+1][Ny+1] */);
/* Newton-CG on the free set: solves P H P x = P b per trajectory by (preconditioned) conjugate gradients from x_0 = 0 with x,
 * r, p, the free set and the recurrence in device memory (ABI version stays 3: detect both entry points by
 * symbol).  H p comes from the sweeps of vch2d_hess_lanczos (the gradient sweep once, then 2 M solves per trajectory and
 * step; VCH_KRYLOV_NOCACHE=1 repeats it), the direction of a step goes through the trial-control scratch.
 *   Base point, dt, M, t_hist, x, y, phi_Q, phi_T, opts / n_opts, rtol, mask, tol, the row rule: as for vch2d_hess_lanczos.
 *   rhs      [B][M+1][Nx+1][Ny+1]: b = rhs.  NULL: the Newton right-hand side of the full cost on the free set, built on the
 *            device: b = -(grad(J1+J2+J3) + kappa_sparsity_b wt_k W_cost_ij sign(u)); on the free set |u| > tol, so
 *            J4 = kappa int int |u| is smooth there and this is its exact Euclidean gradient.
 *   precond  0: D = I.  1: D = diag(wt_k W_cost_ij), the L2(Q) mass of the control (one multiply per node, not stored).
 *   The iteration: r = P b, z = D^-1 r, p = z, rho = r.z; step j: c = p.P H p, n = p.D p, curv[j] = c / n; c not finite
 *   stops with VCH_CG_BREAKDOWN, !(c > 0) with VCH_CG_NEGCURV (x stays as it is and p stays resident as the direction of
 *   non-positive curvature); otherwise alpha = rho / c, x += alpha p, r -= alpha P H p, pred += alpha rho / 2,
 *   resid[j] = ||r||_2 / ||P b||_2; resid[j] <= cg_tol (<= 0: 1e-8) stops with VCH_CG_CONVERGED (a residual that is not
 *   finite with VCH_CG_BREAKDOWN); otherwise beta = rho_new / rho, p = z + beta p.  VCH_CG_LIMIT after k steps; there is no cap
 *   at n_free.  P b == 0 gives zero steps, VCH_CG_CONVERGED and x = 0 (with rhs == NULL: stationarity on the free set).
 *   resid_out, curv_out [B][k]: steps_out[b] counts the updates of x; entries of resid from steps_out[b] on are NaN, and
 *            entries of curv too, except that after VCH_CG_NEGCURV / a breakdown of c, curv[steps_out[b]] is the curvature
 *            that stopped the iteration.
 *   pred_out [B]: the decrease b.x - x.Hx / 2 of the quadratic model, accumulated on the device in a fixed order.
 *   rnorm0_out [B]: ||P b||_2.  status_out [B]: VCH_CG_*.  n_free_out [B]: the size of the free set.
 * The stop state is in device cells: every streaming kernel of a stopped trajectory returns at once and leaves its x, r and
 * p alone, the others go on; the solves of a stopped trajectory are not gated (as in vch2d_hess_lanczos).  No atomics: up
 * to 32 trajectories, a trajectory's outputs are bitwise those of a single-trajectory context, whatever its batch mates do.
 * The host looks once for the size of the free set, once for ||P b|| and once per step (B residuals and stop cells).
 * Errors: VCH_ERR_ARG for k < 1, precond outside 0 / 1, a cg_tol that is not finite, NULL outputs and the row rule,
 * VCH_ERR_STATE as for vch2d_hessvec -- all before anything is enqueued, copied or allocated.  Two errors depend on the data,
 * both VCH_ERR_ARG naming the trajectory: an empty free set (after the mask launch, its sum and one look) and a ||P b|| that
 * is not finite (after the start's look).  Storage: x, r, p are slots 0, 1, 2 of the basis storage of vch2d_hess_lanczos with
 * reorth = 0, the cached sweep, the mask and the partials are shared, no further history is allocated; the call invalidates
 * a resident Lanczos basis (vch2d_krylov_vector: VCH_ERR_STATE) and vch2d_hess_lanczos invalidates x, r, p.  A refused
 * request releases what the call got and returns VCH_ERR_NOMEM with the bytes in the message; the context stays usable,
 * and unchanged but for one case: a call that asks for more steps than the resident Krylov storage holds releases that
 * storage, and the vectors in it, before it asks for the larger one.  Stateless like vch2d_hess_lanczos.  stats: linear solves B M (2 s + 1) when all members take s steps. */
#define VCH_CG_LIMIT 0
#define VCH_CG_CONVERGED 1
#define VCH_CG_NEGCURV 2
#define VCH_CG_BREAKDOWN 3
int vch2d_hess_cg(vch2d_ctx *ctx, const double *dt, int M, const double *t_hist, const double *x, const double *y,
                  const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts, double rtol,
                  const uint8_t *mask /* [B][M+1][Nx+1][Ny+1] or NULL */, double tol,
                  const double *rhs /* [B][M+1][Nx+1][Ny+1] or NULL */, int k, double cg_tol, int precond /* 0 | 1 */,
                  double *resid_out /* [B][k] */, double *curv_out /* [B][k] */, double *pred_out /* [B] */,
                  double *rnorm0_out /* [B] */, int32_t *steps_out /* [B] */, int32_t *status_out /* [B] */,
                  int64_t *n_free_out /* [B] */, vch_stats *stats);
/* out = x (which 0), r (1) or p (2) of the last vch2d_hess_cg of this context; masked-off nodes are exact zeros.
 * VCH_ERR_STATE without resident vectors (no call yet, a failed call, or a vch2d_hess_lanczos since). */
int vch2d_cg_vector(vch2d_ctx *ctx, int which /* 0: x, 1: r, 2: p */, double *out /* [B][M+1][Nx+1][Ny+1] */);
/* Truncated (Steihaug-Toint) Newton-CG in a trust region on the free set of the 2D engine (ABI version stays 3:
 * detect this entry point and vch2d_pgd_trust by symbol).  The arguments, modes, mask, precond, outputs, looks, storage,
 * invalidation rules and errors are those of vch2d_hess_cg, plus radius [B] and xnorm_out [B].  The region is
 * ||x||_D <= radius_b in the preconditioner's norm, ||x||_D^2 = sum D x^2 with D = diag(wt_n W_ij) for precond 1 and the
 * identity for precond 0.  The iteration, its exits (VCH_CG_BOUNDARY = 4 among them, a VCH_CG_NEGCURV that has stepped to the
 * boundary), pred, resid, steps_out and the bitwise equality with vch2d_hess_cg at radius = +inf on a trajectory that ends
 * VCH_CG_CONVERGED or VCH_CG_LIMIT are those of vch1d_hess_cg_tr, word for word.  One kernel differs from vch2d_hess_cg's:
 * k_ncg_fin_tr in place of k_ncg_fin, with six more scalars per trajectory in cells of the Lanczos block that CG leaves
 * unused, so the storage and every request are those of vch2d_hess_cg.  The host uploads the B radii before the start and
 * looks as vch2d_hess_cg does; a boundary exit takes the launches of one ordinary step.  x, r = P b - P H P x and p stay
 * resident for vch2d_cg_vector and vch2d_newton_trial.  xnorm_out [B]: ||x||_D by the recurrence (0 for P b == 0).
 * As in vch1d_hess_cg_tr, a radius whose square is not finite (>= 2^512) has no boundary and acts as +inf, and a radius
 * whose square underflows gives a zero step.
 * VCH_ERR_ARG, before anything is enqueued, copied or allocated, for NULL radius or xnorm_out and a radius_b that is not > 0
 * (NaN included; +inf is allowed). */
int vch2d_hess_cg_tr(vch2d_ctx *ctx, const double *dt, int M, const double *t_hist, const double *x, const double *y,
                     const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts, double rtol,
                     const uint8_t *mask /* [B][M+1][Nx+1][Ny+1] or NULL */, double tol,
                     const double *rhs /* [B][M+1][Nx+1][Ny+1] or NULL */, int k, double cg_tol, int precond /* 0 | 1 */,
                     double *resid_out /* [B][k] */, double *curv_out /* [B][k] */, double *pred_out /* [B] */,
                     double *rnorm0_out /* [B] */, int32_t *steps_out /* [B] */, int32_t *status_out /* [B] */,
                     int64_t *n_free_out /* [B] */, vch_stats *stats, const double *radius /* [B] */,
                     double *xnorm_out /* [B] */);
/* Damped Newton rounds on the free set about the resident PGD iterate, batched, with every trajectory's own parameters and
 * decisions (ABI version stays 3: detect both entry points by symbol).  No history crosses the bus.
 * Per round:
 *   1. the Newton-CG solve of vch2d_hess_cg in its PGD mode (rhs = NULL, mask = NULL, the problem's targets, trajectory b
 *      with the opts[b] of vch2d_pgd_init_v; k, cg_tol, precond, tol, rtol as passed).  Storage: that of vch2d_hess_cg and
 *      the PGD scratch, no further history.
 *   2. a trajectory ends here without a trial with VCH_NEWTON_STATIONARY (||P b|| == 0 or an empty free set, which is no
 *      error in this call), VCH_NEWTON_NEGCURV (the first CG direction has non-positive curvature) or
 *      VCH_NEWTON_BREAKDOWN (CG status VCH_CG_BREAKDOWN: a march under a control that may not be finite is never started).
 *      Otherwise x after VCH_CG_CONVERGED, VCH_CG_LIMIT or VCH_CG_NEGCURV with steps > 0 is the step.
 *   3. trials for s = 1, 1/2, ..., at most max_halvings halvings: t = clip(u + s x, box_b), a free node whose sign the
 *      trial flips is set to 0 (k_nt_trial into the trial-control scratch), a march of t into the trial-state scratch and its
 *      cost.  The first s with J(t) <= cost_b - 1e-4 s pred_b is accepted: control, state history and shift record are
 *      copied as the PGD loop copies an accepted trial, and the five cost scalars become the iterate's (VCH_NEWTON_ACCEPTED).
 *      When no s is accepted the trajectory is left unmoved with VCH_NEWTON_STALLED.
 * A trajectory that has ended sits out all later rounds: VCH_NEWTON_IDLE, its doubles NaN, its integers 0; its solves are not
 * gated.  The others go on; the call returns the number of rounds run (it stops early once every trajectory has ended).
 * Outputs, all [B][n_rounds] and all required: cost_out (the iterate's cost before the round), cost_new_out (the accepted
 * trial's, else the unchanged cost), s_out (the accepted s, else NaN), pred_out, rnorm0_out, halvings_out (halvings made in the
 * round), cg_steps_out, cg_status_out (VCH_CG_*), status_out (VCH_NEWTON_*), counts_out [B][n_rounds][3] = {n_free, and of the
 * round's last trial: nodes pinned to 0, nodes the clip moved}; seconds_out [4] (may be NULL) = {solves, trial kernel, marches,
 * costs}.  Up to 32 trajectories; a trajectory's outputs and its iterate are bitwise those of a single-trajectory context.
 * Afterwards vch2d_pgd_get, vch2d_second_order, vch2d_hessvec, vch2d_hess_lanczos and vch2d_hess_cg work about the new iterate,
 * vch2d_cg_vector returns the last round's vectors, the adjoint r of vch2d_pgd_kkt(refresh = 0) is invalid once any trajectory
 * moved, and the counters of the PGD loop (iteration count, plateau, next first step, stop flags, cost ring) are untouched:
 * a following vch2d_pgd_iterate is that of vch2d_pgd_init_v with u0 = the Newton iterate.  The solver tolerance of the context
 * is restored on every path out.
 * Errors, all before anything is enqueued, copied or allocated: VCH_ERR_STATE before vch2d_pgd_init / _init_v (or when the
 * resident state is no longer the PGD iterate); VCH_ERR_ARG for n_rounds < 1, k < 1, max_halvings < 0, precond outside 0 / 1,
 * a cg_tol that is not finite and NULL outputs.  A ||P b|| that is not finite is VCH_ERR_ARG naming the trajectory, as in
 * vch2d_hess_cg. */
#define VCH_NEWTON_ACCEPTED 0
#define VCH_NEWTON_STATIONARY 1
#define VCH_NEWTON_NEGCURV 2
#define VCH_NEWTON_BREAKDOWN 3
#define VCH_NEWTON_STALLED 4
#define VCH_NEWTON_IDLE 5
#define VCH_NEWTON_REJECTED 6       /* vch1d_pgd_trust, vch2d_pgd_trust: the round's trial was rejected, the trajectory goes on */
int vch2d_pgd_newton(vch2d_ctx *ctx, int n_rounds, int k, double cg_tol, int precond /* 0 | 1 */, double tol, double rtol,
                     int max_halvings, double *cost_out, double *cost_new_out, double *s_out, double *pred_out,
                     double *rnorm0_out /* [B][n_rounds] */, int32_t *halvings_out, int32_t *cg_steps_out,
                     int32_t *cg_status_out, int32_t *status_out /* [B][n_rounds] */,
                     int64_t *counts_out /* [B][n_rounds][3]: n_free, pinned, clipped */, double *seconds_out /* [4] */);
/* Trust-region (Steihaug) Newton-CG rounds on the free set about the resident PGD iterate of the 2D engine, batched, with
 * every trajectory's own parameters, radius and decisions (ABI version stays 3: detect by symbol).  The state
 * checks, the solve's mode (tol, rtol as passed), the trial, its march and cost, the copies of an accepted trial, the
 * resident state afterwards, the refreshed device cost scalars and the untouched PGD counters are those of vch2d_pgd_newton;
 * the adjoint r of vch2d_pgd_kkt(refresh = 0) is invalid once anything moved.  The rounds -- the solve of vch2d_hess_cg_tr
 * inside Delta_b (radius0_b in round 0), no trial after VCH_NEWTON_STATIONARY or VCH_NEWTON_BREAKDOWN, one trial at s = 1
 * after every other CG exit (VCH_CG_NEGCURV included), rho = (J(u) - J(t)) / pred, acceptance, VCH_NEWTON_REJECTED, the radius
 * rule, VCH_NEWTON_STALLED below radius_min, VCH_NEWTON_IDLE afterwards -- and the outputs are those of vch1d_pgd_trust, word
 * for word: one march per round.  Up to 32 trajectories, no atomics: a trajectory's outputs and its iterate are bitwise
 * those of a single-trajectory context.  Storage: that of vch2d_pgd_newton.  Errors, all before anything is enqueued, copied
 * or allocated: VCH_ERR_STATE before vch2d_pgd_init / _init_v (or when the resident state is no longer the PGD iterate);
 * VCH_ERR_ARG for n_rounds < 1, k < 1, precond outside 0 / 1, a cg_tol that is not finite, NULL radius0, a radius0_b,
 * radius_max or radius_min that is not finite or not > 0, and NULL outputs (seconds_out may be NULL). */
int vch2d_pgd_trust(vch2d_ctx *ctx, int n_rounds, int k, double cg_tol, int precond /* 0 | 1 */, double tol, double rtol,
                    const double *radius0 /* [B] */, double radius_max, double radius_min,
                    double *cost_out, double *cost_new_out, double *pred_out, double *rnorm0_out, double *radius_out,
                    double *ratio_out, double *xnorm_out /* [B][n_rounds] */, int32_t *cg_steps_out, int32_t *cg_status_out,
                    int32_t *status_out /* [B][n_rounds] */, int64_t *counts_out /* [B][n_rounds][3]: n_free, pinned, clipped */,
                    double *seconds_out /* [4] or NULL: solves, trial kernel, marches, costs */);
/* The trial kernel's seam: t = min(max(u + s_b x, u_min_b), u_max_b) with u the resident control (rows beyond the march's
 * control are zeros), x and the free set those the last successful vch2d_hess_cg (forward or PGD mode) left resident and the
 * box that call's opts; a free node with t u < 0 becomes 0.  Writes only the trial-control scratch and leaves x, r, p resident.
 * u_out (may be NULL): the trial; chg_out [B][2] = {sum (t - u)^2, sum u^2} in a fixed order, no atomics; counts_out [B][2] =
 * {nodes pinned to 0, nodes the clip moved}.  For s a power of two the trial has the bits of NumPy's np.clip(u + s * x, lo,
 * hi).  VCH_ERR_STATE without resident CG vectors; VCH_ERR_ARG for NULL s, chg_out or counts_out and an s_b that is not
 * finite or not > 0. */
int vch2d_newton_trial(vch2d_ctx *ctx, const double *s /* [B] */, double *u_out /* [B][M+1][Nx+1][Ny+1] or NULL */,
                       double *chg_out /* [B][2] */, int64_t *counts_out /* [B][2]: pinned, clipped */);
/* Per-trajectory cost scalars {J1,J2,J3,J4,J} of the current iterate on the DEVICE
 * (5*B doubles), for the caller's RCCL all-reduce; returns a device pointer via *ptr_dev. */
int vch2d_pgd_cost_dev(vch2d_ctx *ctx, double **ptr_dev);

/* Kernel launches and blocking looks of the host at the device state since the context was created: out[0], out[1]. */
int vch2d_counters(vch2d_ctx *ctx, int64_t *out /* [2] */);

/* -- multi-GPU: the one collective of the path (no reference counterpart) --
 * Trajectories are independent, so ranks share nothing on the data path; per PGD iteration there is ONE
 * all-reduce (sum) of the cost scalars {J1,J2,J3,J4,J} over all trajectories of all ranks, done by RCCL over
 * xGMI on a 5-double device buffer.  The per-trajectory values stay on the device: each context keeps the last
 * 64 iterations' scalars in HBM, a one-workgroup kernel adds them up, RCCL reduces in place, 5 doubles come back.
 * RCCL is bound with dlopen("librccl.so.1") at the first call; the library has no link-time dependency on it.
 *   vch_comm_unique_id   rank 0 only: ncclGetUniqueId; the caller hands the 128 bytes to the other ranks
 *   vch_comm_create      ncclCommInitRank on `device` (collective over all ranks); NULL on failure
 *   vch_comm_allreduce_cost  sum over the trajectories of the nctx contexts of this rank (all on the
 *                        communicator's device) and over all ranks of the cost scalars of PGD iteration
 *                        `iteration` (0-based count since vch2d_pgd_init; < 0: the current iterate);
 *                        J_sum_out [5] on the host.  Every rank must call it, in the same order.  The sum is over
 *                        whatever each trajectory's J is: with per-trajectory weights (vch2d_pgd_init_v) it adds costs of
 *                        different functionals. */
#define VCH_COMM_ID_BYTES 128
typedef struct vch_comm vch_comm;
int vch_comm_unique_id(unsigned char *id_out /* [VCH_COMM_ID_BYTES] */);
vch_comm *vch_comm_create(const unsigned char *id, int rank, int world, int device);
void vch_comm_destroy(vch_comm *comm);
int vch_comm_allreduce_cost(vch_comm *comm, vch2d_ctx *const *ctxs, int nctx, long iteration, double *J_sum_out);

#define VCH_RESIDENT ((const double *)(uintptr_t)1)

/* Replaces free_energy (F2:256-319) for every level of a history at once (the mass/energy
 * invariants of the reference's tests, T2f:252-279): phi_hist [B][rows][Nx+1][Ny+1] or
 * VCH_RESIDENT (the state history of the last march), w_hist the coupling field (same shape) or
 * NULL, eps <= 0 -> 1e-8.  The array is taken as the reference takes it: axis 0 with hy, axis 1
 * with hx.  E_out [B][rows]. */
int vch2d_free_energy(vch2d_ctx *ctx, const double *phi_hist, int rows, const double *w_hist,
                      double hx, double hy, double eps, double *E_out);

/* -- in-situ kernel timing (used by bench.py for the roofline figure; no reference counterpart) --
 * Between _begin and _end every launch of the profiled kernel classes is bracketed by a HIP event
 * pair on the engine's stream (at most max_launches pairs).  _end returns, per class, the summed
 * elapsed milliseconds and the number of launches:
 *   0 Newton stencil SpMV (k_schur_p, fused with the CG updates)  1 DCT as MFMA GEMM (non-power-of-two grids)
 *   2 Newton residual  3 adjoint operator  4 CG vector update  5 adjoint right-hand side  6 cost integrands
 *   7 gradient+prox  8 DCT row pass (forward)  9 DCT column pass (forward, multiplier, inverse)
 *   10 DCT row pass (inverse, with the CG dot products)  11 first sweep of a solve (k_schur_p<1>)
 *   12 first pass of a CG sweep (k_cg_rows_fwd: CG vector updates + Delta p + forward row DCT)  13 the same, first sweep
 *   14 an empty kernel launched 256 times by _begin: the cost of an event pair itself
 *   15 starting guess of a step's first Newton solve (k_guess)  16 starting guess of an adjoint solve (k_adj_guess)
 *   17 row kernel of a reduction-free sweep (k_cheb_rows: inverse row DCT + Chebyshev update + forward row DCT)
 *   18 the same, first kernel of a solve (b~ = P^-1 rhs, y_1)
 *   19 start of a time step (k_eval<0>: old-level terms + initial residual + starting guess; or k_residual<0>)
 *   (class 2 is the Armijo trial: k_eval<2> / k_residual2 / k_residual<1>)
 * _spans (after _end) returns every recorded launch: its class and the elapsed milliseconds of its event pair, in launch
 * order, at most cap entries; the return value is the number recorded.  With these the caller separates launches whose
 * trajectories were all gated off (they last as long as the empty kernel of class 14) from live ones. */
#define VCH_PROF_CLASSES 20
int vch2d_prof_begin(vch2d_ctx *ctx, int max_launches);
int vch2d_prof_end(vch2d_ctx *ctx, double *ms_out, int64_t *count_out, int ncls);
int vch2d_prof_spans(vch2d_ctx *ctx, int32_t *cls_out, float *ms_out, int cap);

/* ------------------------------------------------------------------ 1D ---- */

typedef struct vch1d_params {          /* ForwardSolverConfig of the 1D code (K1:93-102) */
    int32_t N;
    double Lx;
    double tau, gamma, c1, c2, kappa;
} vch1d_params;

typedef struct vch1d_ctx vch1d_ctx;

vch1d_ctx *vch1d_create(const vch1d_params *p, int batch, int max_steps, int device);
void vch1d_destroy(vch1d_ctx *ctx);

/* out = L v (F1:64-80).  v,out [B][N+1]. */
int vch1d_apply_laplacian(vch1d_ctx *ctx, const double *v, double *out);
/* Replaces solve_phi_residual/solve_mu_residual (F1:93-109). */
int vch1d_residuals(vch1d_ctx *ctx, const double *phi_new, const double *phi_old,
                    const double *mu_new, const double *mu_old, const double *w_new,
                    const double *w_old, double dt, double *Rphi_out, double *Rmu_out);
/* Solve the 2(N+1) Newton system.  Replaces np.linalg.solve(J, -R) (F1:185): block
 * (2x2) tridiagonal cyclic reduction in LDS, one workgroup per trajectory (N <= 4096). */
int vch1d_jacobian_solve(vch1d_ctx *ctx, const double *phi_new, double dt, const double *rhs_phi,
                         const double *rhs_mu, double *dphi, double *dmu);
/* Solve A(phi_n) p = rhs with the frozen default parameters (B1:29-33, B1:116). */
int vch1d_adjoint_solve(vch1d_ctx *ctx, const double *phi_n, double dt, const double *rhs,
                        double *p_out);
/* Replaces newton_raphson (F1:139-235). */
int vch1d_newton_raphson(vch1d_ctx *ctx, const double *phi_old, const double *mu_old,
                         const double *w_old, const double *w_new, double dt, double *phi_new,
                         double *mu_new, double *hist, int hist_cap, int32_t *n_hist);
/* Replaces run_main_simulation (F1:286-386): history has M+2 rows (duplicated t=0).
 *   u [B][u_rows][N+1] or NULL; hold-last rule of F1:347-353 (u_rows < M errors like the
 *   reference's IndexError).  phi_hist_out [B][M+2][N+1] or NULL. */
int vch1d_forward(vch1d_ctx *ctx, const double *phi0, const double *u, int u_rows, const double *dt,
                  int M, double *phi_hist_out, vch_stats *stats);
/* Replaces run_backward (B1:48-126); rows = M+2, t_hist [rows]. */
int vch1d_backward(vch1d_ctx *ctx, const double *phi_hist, int rows, const double *t_hist, double h,
                   double b1, double b2, const double *phi_Q, const double *phi_T, double *p_out,
                   double *q_out, double *r_out);
/* Replaces calculate_cost (C1:26-84); J_out [B][5]. */
int vch1d_cost(vch1d_ctx *ctx, const double *phi_hist, const double *u, const double *phi_Q,
               const double *phi_T, int rows, const double *x, const double *t_hist,
               const vch_opt_params *opt, double *J_out);
/* Replaces calculate_gradient + perform_gradient_step + perform_proximal_and_projection
 * (C1:86-112, G1:56-71). */
int vch1d_grad_prox(vch1d_ctx *ctx, const double *u, const double *r, int rows, const double *alpha,
                    const vch_opt_params *opt, double *u_out);

/* Replaces free_energy (F1:243-262) for every level of a history; E_out [B][rows]. */
int vch1d_free_energy(vch1d_ctx *ctx, const double *phi_hist, int rows, const double *w_hist, double h,
                      double eps, double *E_out);

/* Device-resident PGD loop of the 1D driver (the __main__ block of GD_1D.py, G1:333-477, with
 * perform_backtracking_line_search G1:73-113): control, state history, adjoint and targets stay in
 * HBM between iterations.  rows = M+2 (duplicated t = 0 row), t_hist [rows], dt [M], x [N+1].
 *   init: uncontrolled march from phi0 (G1:341), u = 0, targets phi_T [B][N+1] and phi_Q
 *   [B][rows][N+1] or NULL = the ramp (1 - t/T) phi_hist[0] + (t/T) phi_T of build_targets_1d
 *   (G1:238-241); J0_out [B][5] = {J1,J2,J3,J4,J} of the start.
 *   iterate: optimistic step with alpha_prev, else backtracking from alpha_prev with beta 0.8 and
 *   <= 5 trials (the first of which repeats the optimistic step and is not recomputed), alpha growth
 *   1.2 / plateau rule (10 x |dJ| < 1e-7 -> 2.0), stop rule (relative control change < 1e-5 after
 *   k > 10; the control is taken, state and cost keep the previous iterate, G1:462-465).
 *   Outputs [B][n_iters], any may be NULL; trials_out as the reference counts them (1 = optimistic
 *   step accepted); seconds_out [3] = {adjoint sweep, optimistic round, backtracking rounds}.
 *   Returns the number of iterations performed or a negative error.
 *   get: what = 0 control u, 1 state history, 2 adjoint r, 3 phi_Q; out [B][rows][N+1]. */
int vch1d_pgd_init(vch1d_ctx *ctx, const double *phi0, const double *phi_T, const double *phi_Q,
                   const double *x, const double *t_hist, int rows, const double *dt,
                   const vch_opt_params *opt, double *J0_out);
/* vch1d_pgd_init with one parameter set PER TRAJECTORY, a warm start and a first step size: the 1D counterpart of
 * vch2d_pgd_init_v (ABI version stays 3: detect this entry point and vch1d_pgd_kkt by symbol).  vch1d_pgd_init is this
 * call with n_opts = 1 and u0 = alpha0 = NULL.
 *   opts    n_opts parameter sets, n_opts = 1 (one set for the whole batch) or B (trajectory b takes opts[b]); anything
 *           else is VCH_ERR_ARG.  Trajectory b's own values are used everywhere in the loop: b1 in the adjoint source, b2
 *           in the terminal condition, b3 / kappa_sparsity / u_min / u_max in the gradient + prox step, the four weights
 *           in the cost, alpha_max in the growth (x 1.2) and plateau (x 2.0) rules and as the default first step.  The
 *           six numbers the kernels need live in a [B] table on the device, indexed by the trajectory's workgroup; the
 *           arithmetic is that of the scalar form.  One trajectory is one workgroup with fixed reduction orders and the
 *           Newton and adjoint solves are direct, so a member of a mixed batch computes the bits of a batch-1 run with
 *           its parameters.
 *           VCH_ERR_ARG, with a message that names the trajectory, before anything is copied or launched: non-finite b1,
 *           b2, b3 or kappa_sparsity, kappa_sparsity < 0, alpha_max <= 0, u_min > u_max (infinite bounds are legal),
 *           alpha0[b] not finite or <= 0.
 *   u0      [B][rows][N+1] start control or NULL (zeros).  Taken as given, NOT clipped to the box: the initial march
 *           runs under it and J0_out is its cost under each trajectory's own weights.  The ramp target phi_Q (phi_Q ==
 *           NULL) is built from history row 0, the initial state, as without a start control.
 *   alpha0  [B] or NULL.  NULL: the first alpha_prev is each trajectory's alpha_max (the reference's start); otherwise
 *           min(alpha0[b], alpha_max of b).
 * The iteration counter (the k of the stop rule `change < 1e-5 and k > 10`), the plateau counter, the cost history and
 * the done flags start as after vch1d_pgd_init, also under a warm start: a resumed run is a new run from u0.  max_iter is
 * not read: the loop length is the n_iters of vch1d_pgd_iterate. */
int vch1d_pgd_init_v(vch1d_ctx *ctx, const double *phi0, const double *phi_T, const double *phi_Q,
                     const double *x, const double *t_hist, int rows, const double *dt,
                     const vch_opt_params *opts, int n_opts,
                     const double *u0 /* [B][rows][N+1] or NULL */, const double *alpha0 /* [B] or NULL */,
                     double *J0_out /* [B][5] */);
int vch1d_pgd_iterate(vch1d_ctx *ctx, int n_iters, double *cost_out, double *alpha_out,
                      int32_t *trials_out, double *change_out, double *seconds_out);
int vch1d_pgd_get(vch1d_ctx *ctx, int what, double *out);
/* KKT sparsity statistic `u* = 0 <=> |r*| <= kappa_sparsity` of the resident iterate (verify_sparsity_condition,
 * G1:115-147), counted on the device in one launch, one workgroup per trajectory: 4 B integers and 2 B doubles cross to
 * the host instead of the control and the adjoint through vch1d_pgd_get.
 *   counts_out[b] = { #nodes |u| < tol, #nodes |r| <= kappa_sparsity of trajectory b, #nodes where the two predicates
 *                     agree, #nodes } over all rows (N+1) nodes of trajectory b, the duplicated t = 0 row included, as
 *                     u_optimal.size counts them in the reference; tol <= 0 means 1e-6.
 *   refresh != 0  first runs the adjoint sweep on the resident state with each trajectory's own b1, b2, as
 *                 GD_1D.main() does with run_backward after the loop.  The result stays in the resident p, q, r.
 *   refresh == 0  uses the resident r as it is: the adjoint the last iteration started from, i.e. that of the iterate
 *                 BEFORE the last accepted step.  VCH_ERR_STATE if no sweep has run since the init, or if a stateless
 *                 call that writes the same buffer (vch1d_backward, vch1d_grad_prox) ran on this context after it.  Those
 *                 calls, vch1d_forward and vch1d_cost upload into the buffers of a loaded PGD problem: keep them on a
 *                 context of their own while a loop is in progress.
 *   stationarity_out[b] (or NULL) = ||prox_1(u) - u||_2 / (||u||_2 + 1e-9): prox_1 is the gradient + prox step of
 *                 vch1d_grad_prox with alpha = 1 and trajectory b's parameters.  Its image is not stored.
 * The control, the state history, the trial buffers and the loop's bookkeeping are not touched, and the adjoint is a
 * direct solve that the next iteration repeats from the same state: a following vch1d_pgd_iterate is bit for bit that of
 * an uninterrupted run with either value of refresh.  VCH_ERR_STATE before vch1d_pgd_init.
 * Stop quirk: after a trajectory's stop rule fired (G1:462-465) the resident control is the NEW iterate while the resident
 * state history is the PREVIOUS one's.  The refreshed adjoint then belongs to the previous control, and the statistic
 * pairs it with the new one. */
int vch1d_pgd_kkt(vch1d_ctx *ctx, int refresh, double tol, int64_t *counts_out /* [B][4] */,
                  double *stationarity_out /* [B] or NULL */);
/* Relative tracking / terminal errors of the iterations of the last vch1d_pgd_iterate call (G1:425-450);
 * same conventions as vch2d_pgd_errors. */
int vch1d_pgd_errors(vch1d_ctx *ctx, int n_iters, double *tracking_out, double *terminal_out);

/* Directional sparsity in the 1D engine (ABI version stays 3: detect the three entry points below by symbol).
 * Beside the full-sparsity term g(u) = kappa_s int int |u| (VCH_SPARSITY_FULL: a node-wise soft threshold, everything
 * above) the sparsity term and its prox can be taken by groups:
 *   VCH_SPARSITY_TIME   g(u) = kappa_s int_0^T ||u(., t)||_{L2(Omega)} dt: group k is row k of the control,
 *                       ||z||^2 = sum_i wx_i z_i^2; the control vanishes on whole time intervals.
 *   VCH_SPARSITY_SPACE  g(u) = kappa_s int_Omega ||u(x, .)||_{L2(0,T)} dx: group i is column i, ||z||^2 = sum_k wt_k z_k^2;
 *                       the control vanishes on whole regions for all times.
 * wx = the trapezoid weights of x, wt those of t_hist (0 for the duplicated t = 0 row).  The prox is taken in the L2(Q)
 * metric like the node-wise threshold, so the threshold is lam = alpha kappa_s for every group.  With v = u - alpha (r + b3 u)
 * and the box u_min <= 0 <= u_max, per group:
 *   c = ||cone(v)|| <= lam (cone drops the positive entries when u_max == 0, the negative ones when u_min == 0): u+ = 0, s = 0;
 *   otherwise u+ = clip(s v), s in (0, 1] the root of h(s) = ||clip(s v)|| (1 - s) - lam s; where clip(s0 v) = s0 v for
 *   s0 = 1 - lam / ||v|| (always with an infinite box) s = s0, else a safeguarded Newton iteration on the device finds it.
 * The cost's J4 becomes kappa_s * trapezoid in t of sqrt(sum_i wx_i u^2) (TIME) or kappa_s sum_i wx_i sqrt(sum_k wt_k u^2)
 * (SPACE); J1..J3 are unchanged.  No atomics: a member of a mixed batch computes the bits of a single run with its mode and
 * parameters.
 *
 * vch1d_pgd_init_g: vch1d_pgd_init_v with a mode per trajectory: sparsity[n_sparsity], n_sparsity = 1 or B.  All
 * VCH_SPARSITY_FULL is vch1d_pgd_init_v bit for bit; vch1d_pgd_init and vch1d_pgd_init_v reset every mode to FULL.
 * VCH_ERR_ARG, before anything is copied or enqueued and with the resident problem left as it was: NULL sparsity, n_sparsity
 * neither 1 nor B, a mode outside 0..2, a group-mode trajectory whose box does not contain 0.
 * vch1d_pgd_iterate, vch1d_pgd_kkt, vch1d_pgd_get and vch1d_pgd_errors then act per trajectory on its mode.  For a
 * group-mode trajectory vch1d_pgd_kkt counts groups: counts_out[b] = { #groups ||u_g|| < tol, #groups ||r_g|| <=
 * kappa_sparsity, #groups where the two agree, #groups } in the group's norm (a group of the optimal control is zero exactly
 * when ||r_g|| <= kappa_s, for u_min < 0 < u_max), and the stationarity takes the mode's prox at alpha = 1.
 * Refused with VCH_ERR_STATE before anything is enqueued while any trajectory of the resident problem is in a group mode:
 * vch1d_pgd_newton, vch1d_pgd_trust, and vch1d_hess_cg / vch1d_hess_cg_tr with u == VCH_RESIDENT and rhs == NULL: they build
 * the sign term and the free set of the L1 functional.  vch1d_second_order, vch1d_hessvec, vch1d_hess_lanczos and
 * vch1d_hess_cg with an explicit rhs concern the smooth part only and keep working. */
#define VCH_SPARSITY_FULL 0
#define VCH_SPARSITY_TIME 1
#define VCH_SPARSITY_SPACE 2
int vch1d_pgd_init_g(vch1d_ctx *ctx, const double *phi0, const double *phi_T, const double *phi_Q,
                     const double *x, const double *t_hist, int rows, const double *dt,
                     const vch_opt_params *opts, int n_opts,
                     const double *u0 /* [B][rows][N+1] or NULL */, const double *alpha0 /* [B] or NULL */,
                     const int32_t *sparsity /* [n_sparsity] */, int n_sparsity /* 1 or B */,
                     double *J0_out /* [B][5] */);
/* The stateless seam of the prox: vch1d_grad_prox with the mode `sparsity` for the whole batch.  x [N+1] (TIME) and t_hist
 * [rows] (SPACE) give the group's weights and may be NULL where the mode does not read them.  scale_out (or NULL) receives
 * s per group, [B][rows] for TIME or [B][N+1] for SPACE.  VCH_SPARSITY_FULL is vch1d_grad_prox (scale_out is not written).
 * VCH_ERR_ARG for a mode outside 0..2 and, in a group mode, for a box that does not contain 0. */
int vch1d_grad_prox_g(vch1d_ctx *ctx, const double *u, const double *r, int rows, const double *x,
                      const double *t_hist, const double *alpha, const vch_opt_params *opt, int sparsity,
                      double *u_out, double *scale_out);
/* vch1d_cost with J4 of the mode `sparsity`; VCH_SPARSITY_FULL is vch1d_cost. */
int vch1d_cost_g(vch1d_ctx *ctx, const double *phi_hist, const double *u, const double *phi_Q,
                 const double *phi_T, int rows, const double *x, const double *t_hist,
                 const vch_opt_params *opt, int sparsity, double *J_out);

/* Directional sparsity in the 2D engine (ABI version stays 3: detect the three entry points below by symbol).
 * The same two functionals, the same modes and the same prox per group as in 1D (above), with the groups of a control
 * [rows][Nx+1][Ny+1]:
 *   VCH_SPARSITY_TIME   group k is level k, ||z||^2 = sum_ij W_ij z_ij^2, W_ij = wx_i wy_j the product trapezoid weights of
 *                       x and y (the cost's own);
 *   VCH_SPARSITY_SPACE  group (i, j) is the pencil u[:, i, j], ||z||^2 = sum_k wt_k z_k^2, wt the trapezoid weights of t_hist
 *                       (strictly increasing: no level of weight zero but through a grid the caller repeats a node of).
 * J4 becomes kappa_s * trapezoid in t of sqrt(sum_ij W_ij u^2) (TIME) or kappa_s sum_ij W_ij sqrt(sum_k wt_k u^2) (SPACE);
 * J1..J3 are unchanged.  No floating-point atomics and one summation order fixed by the grid: a member of a mixed batch
 * computes the bits of a single run with its mode and parameters.
 *
 * vch2d_pgd_init_g: vch2d_pgd_init_v with a mode per trajectory: sparsity[n_sparsity], n_sparsity = 1 or B.  All
 * VCH_SPARSITY_FULL is vch2d_pgd_init_v bit for bit; vch2d_pgd_init and vch2d_pgd_init_v reset every mode to FULL.
 * VCH_ERR_ARG, before anything is copied or enqueued and with the resident problem left as it was: NULL sparsity, n_sparsity
 * neither 1 nor B, a mode outside 0..2, a group-mode trajectory whose box does not contain 0.
 * vch2d_pgd_iterate, vch2d_pgd_kkt, vch2d_pgd_get and vch2d_pgd_errors then act per trajectory on its mode.  For a
 * group-mode trajectory vch2d_pgd_kkt counts groups: counts_out[b] = { #groups ||u_g|| < tol, #groups ||r_g|| <=
 * kappa_sparsity, #groups where the two agree, #groups = M+1 or (Nx+1)(Ny+1) } in the group's norm, and the stationarity
 * takes the mode's prox at alpha = 1.
 * Refused with VCH_ERR_STATE before anything is enqueued while any trajectory of the resident problem is in a group mode:
 * vch2d_pgd_newton, vch2d_pgd_trust, vch2d_newton_trial, and vch2d_hess_cg / vch2d_hess_cg_tr about the resident iterate
 * with rhs == NULL: they build the sign term and the free set of the L1 functional.  vch2d_second_order, vch2d_hessvec,
 * vch2d_hess_lanczos and vch2d_hess_cg with an explicit rhs concern the smooth part only and keep working. */
int vch2d_pgd_init_g(vch2d_ctx *ctx, const double *phi0, const double *phi_T, const double *phi_Q,
                     int ramp, double T, const double *t_hist, int M, const double *x, const double *y,
                     const vch_opt_params *opts, int n_opts, const double *u0 /* or NULL */,
                     const double *alpha0 /* [B] or NULL */, const int32_t *sparsity /* [n_sparsity] */,
                     int n_sparsity /* 1 or B */, double *J0_out /* [B][5] */);
/* The stateless seam of the prox: vch2d_grad_prox with the mode `sparsity` for the whole batch.  x [Nx+1], y [Ny+1] (TIME)
 * and t_hist [rows] (SPACE) give the group's weights and may be NULL where the mode does not read them.  scale_out (or NULL)
 * receives s per group, [B][rows] for TIME or [B][Nx+1][Ny+1] for SPACE.  VCH_SPARSITY_FULL is vch2d_grad_prox (scale_out
 * is not written).  VCH_ERR_ARG for a mode outside 0..2 and, in a group mode, for a box that does not contain 0.
 * x, y and t_hist need only be non-decreasing here (vch2d_pgd_init_g wants t_hist strictly increasing): a repeated node
 * gives a line of nodes (TIME) or a level (SPACE) of weight zero, which takes the same formulas; what stands there does not
 * enter its group's norm and is scaled and clipped with the rest of the group.
 * A group-mode call overwrites the resident u_hist, r_hist, u_trial and the weights W_cost (TIME) or gp_wt (SPACE): do not
 * interleave it with the iterations of a resident problem on the same context; the next vch2d_pgd_init* restores all five. */
int vch2d_grad_prox_g(vch2d_ctx *ctx, const double *u, const double *r, int rows, const double *x,
                      const double *y, const double *t_hist, const double *alpha,
                      const vch_opt_params *opt, int sparsity, double *u_out, double *scale_out);
/* vch2d_cost with J4 of the mode `sparsity`; VCH_SPARSITY_FULL is vch2d_cost. */
int vch2d_cost_g(vch2d_ctx *ctx, const double *phi_hist, const double *u, const double *phi_Q,
                 const double *phi_T, int M, const double *x, const double *y, const double *t_hist,
                 const vch_opt_params *opt, int sparsity, double *J_out);

/* Exact first and second directional derivatives of the smooth part J1 + J2 + J3 of the 1D cost along h, by a tangent
 * (linearised) march on the device: the 1D counterpart of vch2d_second_order (ABI version stays 3: detect this entry point
 * by symbol).  One persistent workgroup per direction runs the whole march and the quadrature; no adjoint, no nonlinear
 * march, no finite differences, no host round trip between the launch and the six scalars.
 * The history has rows = M + 2 rows (t = 0 twice, F1:329-336); step n = 0..M-1 takes row n+1 to row n+2 with dt_n and is
 * driven by the direction rows (h_n, h_{n+1}), the control's own indexing by step (F1:347-353).  J(phi*) is the Newton
 * matrix of vch1d_jacobian_solve (unclipped diagonal tau/dt + 2 c1 / (1 - phi*^2), F1:122) at phi* = phi_hist[n+2].  All
 * tangent fields start at zero; per step:
 *   dw'  = ((gamma/dt - 1/2) dw + 1/2 (h_{n+1} + h_n)) / (gamma/dt + 1/2)
 *   J [dphi*; dmu']   = [ tau dphi/dt + kappa/2 L dphi + 2 c2 dphi + 1/2 dmu + 1/2 (dw' + dw) ;  dphi/dt + 1/2 L dmu ]
 *   J [d2phi*; d2mu'] = [ tau d2phi/dt + kappa/2 L d2phi + 2 c2 d2phi + 1/2 d2mu - c1 rho(phi*) (dphi*)^2 ;
 *                         d2phi/dt + 1/2 L d2mu ],      rho(p) = 4 p / (1 - p^2)^2
 *   dphi' = dphi* - sum(wts dphi*) / Lx,   d2phi' = d2phi* - sum(wts d2phi*) / Lx,     wts = (Lx / N) trapz
 * Two things differ from 2D.  The concave term is explicit: -2 c2 phi_old sits in the residual (F1:99-109), so +2 c2 dphi
 * is on the right-hand side, not in the matrix.  The mass shift is uniform and always applied (F1:366); its linearisation
 * is the weighted-mean removal over all nodes.  No record of the shifts is needed: the 1D Laplacian conserves mass in
 * exactly these weights, the shift the march subtracted is bounded by the Newton tolerance, and J, rho are taken at the
 * stored row.  The end-of-step clip (F1:361) is taken as the identity.  The call does NOT detect an active clip
 * (|phi| >= 1 - delta_sep somewhere) nor a step the march left through the line-search-failure return (F1:227-229): behind
 * either, the result is not the derivative of the march.
 *   phi_hist [n_base][rows][N+1] base-point state history, or NULL: the resident one (last vch1d_forward / _backward /
 *           _cost upload, or the PGD iterate)
 *   u       [n_base][rows][N+1] base-point control; NULL: zeros; VCH_RESIDENT: the PGD's resident control.  It enters
 *           s_ctrl alone: the tangent depends on the state history and h only.
 *   n_base  1: one base point shared by all B directions (read with stride 0 on the device; of resident arrays, trajectory
 *           0's); B: one per trajectory.  It holds for phi_hist, u, phi_Q and phi_T alike.
 *   h       [B][rows][N+1] direction
 *   dt      [M] step sizes or NULL: t_hist[n+2] - t_hist[n+1];  t_hist [rows], x [N+1]: the cost's quadrature grids
 *   phi_Q   [n_base][rows][N+1], phi_T [n_base][N+1]; NULL: zeros; VCH_RESIDENT: the PGD's targets
 *   opts    n_opts = 1 (one set for the batch) or B (trajectory b takes opts[b]); only b1, b2, b3 are read
 *   order   1 or 2; order 1 skips the second solve of every step, c_state is then NaN
 *   out[b] = { s_state = b1 int int (phi - phi_Q) dphi + b2 int (phi_M - phi_T) dphi_M,   s_ctrl = b3 int int u h,
 *              c_gn    = b1 int int dphi^2 + b2 int dphi_M^2,
 *              c_state = b1 int int (phi - phi_Q) d2phi + b2 int (phi_M - phi_T) d2phi_M,
 *              c_ctrl  = b3 int int h^2,   n_h = int int h^2 }
 *           with the cost's own quadrature (C1:55-73): trapezoid in x, then in t_hist over all rows, so the duplicated
 *           t = 0 row has zero weight.  J'(u) h = s_state + s_ctrl,  J''(u)[h,h] = c_gn + c_state + c_ctrl.  The L1 term J4
 *           has no curvature away from its kink and is left out.  A trajectory with h == 0 gets exact zeros.
 *   dphi_hist_out, d2phi_hist_out  [B][rows][N+1] or NULL: the tangent fields (rows 0 and 1 are zero; with order 1
 *           d2phi_hist_out is all zeros)
 *   stats (or NULL): linear_solves = order M B, launches = 1, device seconds of the march.
 * VCH_ERR_ARG, each with a message naming what failed, before anything is copied or launched: rows outside
 * 3..max_steps+2; n_base or n_opts not 1 or B; order not 1 or 2; NULL h, t_hist, x, out or opts; a dt_n <= 0 or
 * non-finite; non-finite b1, b2, b3.  VCH_ERR_STATE: phi_hist == NULL without a resident history of `rows` rows;
 * VCH_RESIDENT before vch1d_pgd_init (or for a problem with another number of rows).
 * The call is stateless like vch1d_backward and vch1d_cost, and more so: the direction, an uploaded base point, the grids
 * and the tangent fields live in buffers of its own (the work planes in the per-trajectory march scratch, whose contents
 * no call relies on), so the control, the state history, the adjoint, the trial buffers and the PGD bookkeeping are not
 * touched and a following vch1d_pgd_iterate is bit for bit that of an uninterrupted run.  One trajectory is one workgroup
 * with fixed reduction orders: its outputs are bitwise independent of the batch.
 * Stop quirk: after a trajectory's stop rule fired (G1:462-465) the resident control is the NEW iterate while the resident
 * state history is the PREVIOUS one's.  The tangent then belongs to the previous control (it depends on the state history
 * and h only), and only s_ctrl sees the new one. */
int vch1d_second_order(vch1d_ctx *ctx, const double *phi_hist, const double *u, int n_base,
                       const double *h, int rows, const double *dt, const double *t_hist, const double *x,
                       const double *phi_Q, const double *phi_T,
                       const vch_opt_params *opts, int n_opts,            /* 1 or B; only b1,b2,b3 are read */
                       int order /* 1 or 2 */,
                       double *out /* [B][6] */,
                       double *dphi_hist_out, double *d2phi_hist_out      /* [B][rows][N+1] or NULL */,
                       vch_stats *stats);

/* Exact discrete gradient field and Hessian-vector product of the smooth part J1 + J2 + J3 of the 1D cost: one launch,
 * one persistent workgroup per direction (k1d_hessvec).  The tangent step of vch1d_second_order is a linear
 * map on (dphi, dmu, dw) driven by (h_n, h_{n+1}); the exact adjoint of the DISCRETE cost is that map run backwards over
 * the steps with the transposed Newton matrix J(phi*)^T, and a second transposed sweep beside it, fed by the tangent of h,
 * gives H h.  With wx = h trapz, wt the trapezoid weights of t_hist (row 0: 0), e = phi - phi_Q, al = (gamma/dt - 1/2) /
 * (gamma/dt + 1/2), be = (1/2) / (gamma/dt + 1/2), Kp = (tau/dt + 2 c2) I + kappa/2 L, multipliers starting at zero,
 * G = b3 wt (x) wx . u, Hh = b3 wt (x) wx . h, and for k = M-1 .. 0 (phi* = row k+2, step k has dt_k):
 *     l_phi += wt[k+2] b1 wx . e[k+2]                  (+ b2 wx . (phi_M - phi_T) at k = M-1)
 *     l_v    = l_phi - wx sum(l_phi) / Lx              (transpose of the mean removal; plain node sum)
 *     J(phi*)^T [yp; ym] = [l_v; l_mu]
 *     l_dw   = yp/2 + l_w;   G[k] += be l_dw;   G[k+1] += be l_dw
 *     (l_phi, l_mu, l_w) <- (Kp^T yp + ym/dt,  yp/2 + L^T ym / 2,  yp/2 + al l_dw)
 *   order 2, same loop, with v_k = dphi* of step k of the tangent of h before its mean removal and dphi its history:
 *     L_phi += wt[k+2] b1 wx . dphi[k+2]               (+ b2 wx . dphi_M at k = M-1)
 *     L_v    = L_phi - wx sum(L_phi) / Lx - c1 rho(phi*) yp v_k,        rho(p) = 4 p / (1 - p^2)^2
 *     J(phi*)^T [Yp; Ym] = [L_v; L_mu];   Hh and (L_phi, L_mu, L_w) as above.
 * L is not symmetric (the mirrored-Neumann rows carry a 2): the transposed rows take each neighbour's weight from the
 * neighbour's row.  Cost: one linear solve per step for the gradient; one tangent and two transposed solves per step for
 * H h.  No nonlinear march, no finite differences, no host round trip.
 * EUCLIDEAN convention: grad_out[b][row][i] = d(J1+J2+J3)/du[row][i] and hv_out = (d^2(J1+J2+J3)/du^2) h, derivatives with
 * respect to the entries of u, NOT divided by quadrature weights: J'(u)h = sum(grad . h) and J''(u)[h,h] = sum(h . hv) as
 * plain node sums, the s_state + s_ctrl and c_gn + c_state + c_ctrl of vch1d_second_order.  Row 0 has quadrature weight 0
 * but drives step 0, so grad[0] != 0; the last row drives no step and holds b3 wt wx u (resp. h) alone.
 * Arguments and conventions are those of vch1d_second_order (n_base, NULL = zeros, VCH_RESIDENT, resident history,
 * dt == NULL, only b1, b2, b3 of opts are read, the clip taken as the identity with the same caveats), except:
 *   h        [B][rows][N+1] direction; NULL allowed iff order 1 (the gradient does not depend on it)
 *   order    1: gradient alone; 2: gradient and H h
 *   grad_out [B][rows][N+1] or NULL;   hv_out [B][rows][N+1], required iff order 2 (with order 1: NULL, or zero-filled)
 *   dots_out [B][2] or NULL = { sum grad . h, sum h . hv }, reduced on the device in a fixed order; NaN where the factor
 *            does not exist (NULL h; order 1)
 *   stats (or NULL): launches = 1, linear_solves = B M (order == 1 ? 1 : 3), device seconds.
 * A trajectory with h == 0 gets hv exactly zero.  VCH_ERR_ARG / VCH_ERR_STATE as for vch1d_second_order, with the same
 * messages and before anything is copied or launched (NULL hv_out with order 2 in place of NULL out).  The call is
 * stateless in the same sense: it leaves every resident buffer and the PGD bookkeeping as it found them, and a trajectory's
 * outputs are bitwise independent of the batch.  The ABI version stays 3: callers detect the entry point by symbol. */
int vch1d_hessvec(vch1d_ctx *ctx, const double *phi_hist, const double *u, int n_base,
                  const double *h /* NULL allowed iff order 1 */, int rows, const double *dt, const double *t_hist,
                  const double *x, const double *phi_Q, const double *phi_T,
                  const vch_opt_params *opts, int n_opts,                 /* 1 or B; only b1,b2,b3 are read */
                  int order /* 1 or 2 */,
                  double *grad_out /* [B][rows][N+1] or NULL */, double *hv_out /* [B][rows][N+1], required iff order 2 */,
                  double *dots_out /* [B][2] or NULL */, vch_stats *stats);

/* Lanczos on the reduced Hessian P H P of J1 + J2 + J3 of the 1D cost, with the basis, the free set and the recurrence in
 * device memory (the 1D counterpart of vch2d_hess_lanczos; ABI version stays 3: detect both entry points by
 * symbol).  H q comes from the transposed sweeps of vch1d_hessvec; P masks to the free set.  Only the tridiagonal coefficients
 * cross to the host: T = tridiag(beta, alpha, beta) of a trajectory has the Ritz values of P H P.
 *   Base point (phi_hist, u, n_base, rows, dt, t_hist, x, phi_Q, phi_T, opts / n_opts): the rules of vch1d_hessvec, with
 *   NULL = zeros, VCH_RESIDENT, the resident history and the stop quirk.  Beyond b1, b2, b3 the call reads u_min, u_max of
 *   opts[b].
 *   mask     [n_base][rows][N+1] bytes, non-zero = free (one for the batch, or one per trajectory); NULL: built on the
 *            device from the base control with trajectory b's own box, u > u_min + tol && u < u_max - tol && |u| > tol
 *            (tol <= 0: 1e-8).  All rows take part, the duplicated t = 0 row included.  NULL mask with NULL u is
 *            VCH_ERR_ARG: a zero control has no free node.
 *   q0       [B][rows][N+1] start vector; q_0 = P q0 / ||P q0||
 *   k        steps at most; trajectory b stops after min(k, n_free_b) steps, when beta_j <= 1e-14 max_i |alpha_i| (an
 *            invariant subspace) or when beta_j is not finite; a stopped trajectory's vectors are left alone, the others go on
 *   reorth   1: classical Gram-Schmidt, twice, against all of q_0 .. q_j (k + 1 resident vectors); 0: the same two rounds
 *            against q_{j-1}, q_j only (three resident vectors)
 *   alpha_out, beta_out [B][k]: alpha_j = the sum of the two rounds' coefficients on q_j, beta_j = ||w|| after both rounds;
 *            entries beyond steps_out[b] are NaN.  n_free_out[b]: the size of the free set, counted on the device.
 * The set-up launch (one persistent workgroup per trajectory) builds the free set, q_0 and runs the gradient sweep once,
 * keeping every step's multiplier yp in one further history; a step then runs the tangent march of q_j and the second
 * transposed sweep alone: 2 M solves per trajectory and step instead of vch1d_hessvec's 3 M (VCH_KRYLOV_NOCACHE=1 repeats the
 * gradient sweep in every step, with the same bits: A/B and tests).  The recurrence (products, updates, norm, q_{j+1}) runs
 * on a device-wide grid with two-stage reductions in a fixed order.  The stop state lives in device cells, the k steps are
 * enqueued back to back, and the host looks twice: after the set-up (n_free, ||P q0||) and at the end.
 * Errors: VCH_ERR_ARG / VCH_ERR_STATE as for vch1d_hessvec with the same messages, VCH_ERR_ARG for k < 1, NULL q0 or outputs,
 * reorth outside 0 / 1 and NULL mask with NULL u -- all before anything is copied, launched or allocated.  Two errors depend
 * on the data, both VCH_ERR_ARG naming the trajectory: an empty free set, and a start vector that vanishes on the free set;
 * they come after the set-up launch and one look, before any step, and leave no resident basis.  Device storage, allocated
 * on first use as one group: the basis (k + 1 or 3 histories), one history each for the cached sweep, the tangent and w, the
 * mask (one byte per node of a history) and the partials; a refused request releases what the call got and returns
 * VCH_ERR_NOMEM with the context usable and unchanged and a message that states the bytes the group needs.  A later call with
 * a larger k replaces the storage.  Stateless like vch1d_hessvec; no atomics: a trajectory's alpha, beta and steps are
 * bitwise those of a single-trajectory context, whatever its batch mates do.
 * stats: launches, host_syncs = 2, linear_solves = B M (2 s + 1) for a batch whose members all take s steps (3 B M s with the
 * switch), device seconds. */
int vch1d_hess_lanczos(vch1d_ctx *ctx, const double *phi_hist, const double *u, int n_base, int rows,
                       const double *dt, const double *t_hist, const double *x,
                       const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts,
                       const uint8_t *mask /* [n_base][rows][N+1] or NULL */, double tol,
                       const double *q0 /* [B][rows][N+1] */, int k, int reorth /* 0 | 1 */,
                       double *alpha_out /* [B][k] */, double *beta_out /* [B][k] */,
                       int32_t *steps_out /* [B] */, int64_t *n_free_out /* [B] */, vch_stats *stats);
/* out[b] = sum_{j<m} coef[b][j] q_j from the basis the last vch1d_hess_lanczos of this context left resident: the Ritz vector
 * of a Ritz value (coef = an eigenvector of T), or one basis vector (a unit coef).  Masked-off nodes are exact zeros.
 * VCH_ERR_STATE without a resident basis, and after a reorth = 0 run when m exceeds the vectors still held; VCH_ERR_ARG for
 * m < 1 or m above the smallest step count of the batch plus one. */
int vch1d_krylov_vector(vch1d_ctx *ctx, const double *coef /* [B][m] */, int m, double *out /* [B][rows][N+1] */);
/* Newton-CG on the free set of the 1D engine: solves P H P x = P b per trajectory by (preconditioned) conjugate gradients
 * from x_0 = 0 with x, r, p, the free set and the recurrence in device memory (the 1D counterpart of
 * vch2d_hess_cg; ABI version stays 3: detect both entry points by symbol).  The iteration, the stop rules, the NaN
 * conventions of resid_out / curv_out, pred_out, rnorm0_out, steps_out, status_out (VCH_CG_*) and n_free_out are those of
 * vch2d_hess_cg; base point, opts, mask and tol are those of vch1d_hess_lanczos (n_base 1 or B, NULL = zeros, VCH_RESIDENT,
 * the resident history, the stop quirk, the mask built on the device from trajectory b's own box over all rows, NULL mask
 * with NULL u is VCH_ERR_ARG).  H p comes from the step kernel of vch1d_hess_lanczos: 2 M solves per product.  Four points
 * differ from the 2D call:
 *   1. rhs NULL: the Newton right-hand side b = -(grad(J1+J2+J3) + kappa_sparsity_b wt_k wx_i sign(u)), built by the set-up
 *      launch, whose gradient sweep then accumulates the gradient field with the expressions of vch1d_hessvec order 1.  wt
 *      are the trapezoid weights of t_hist over all rows, wx those of x (the weights of the cost).  Row 0 has wt = 0: the
 *      sign term vanishes there, the gradient does not (row 0 drives step 0).  The call reads kappa_sparsity of opts[b]
 *      beside b1, b2, b3, u_min, u_max.
 *   2. precond 1: D = diag(wt'_k wx_i) with wt'_k = wt_k except wt'_0 := wt_1: row 0 is a real unknown with quadrature
 *      weight zero and takes the weight of the row that duplicates its time.  D is computed per node and not stored.  A
 *      wt'_k that is not finite or not > 0 with precond 1 is VCH_ERR_ARG naming the row, before anything is enqueued.
 *   3. The stop state is in device cells and the k steps are enqueued back to back; every kernel of a stopped trajectory
 *      returns at once, the persistent step kernel included.  The host looks twice: after the set-up (n_free, ||P b||) and
 *      at the end.  stats: host_syncs = 2, linear_solves = sum_b M (2 p_b + 1) with p_b the products taken: steps_b, plus
 *      one after an exit on the curvature (VCH_KRYLOV_NOCACHE=1: 3 M p_b, plus the M of the set-up when rhs is NULL).
 *   4. An empty free set and a ||P b|| that is not finite are both VCH_ERR_ARG naming the trajectory, after the set-up's
 *      look and before any step; they leave nothing resident.  P b == 0 gives zero steps, VCH_CG_CONVERGED and x = 0.
 * Further errors, all before anything is copied, launched or allocated: VCH_ERR_ARG / VCH_ERR_STATE as for vch1d_hessvec,
 * VCH_ERR_ARG for k < 1, precond outside 0 / 1, a cg_tol that is not finite and NULL outputs.  Storage: x, r, p are slots 0,
 * 1, 2 of the basis storage of vch1d_hess_lanczos with reorth = 0; the cached sweep, the tangent history, w, the mask and the
 * partials are shared and no further history is allocated.  The call invalidates a resident Lanczos basis
 * (vch1d_krylov_vector: VCH_ERR_STATE) and vch1d_hess_lanczos invalidates x, r, p.  A refused request releases the group and
 * returns VCH_ERR_NOMEM with the bytes in the message; the context stays usable.  Stateless like vch1d_hessvec; no atomics:
 * a trajectory's outputs, x, r and p included, are bitwise those of a single-trajectory context. */
int vch1d_hess_cg(vch1d_ctx *ctx, const double *phi_hist, const double *u, int n_base, int rows,
                  const double *dt, const double *t_hist, const double *x,
                  const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts,
                  const uint8_t *mask /* [n_base][rows][N+1] or NULL */, double tol,
                  const double *rhs  /* [B][rows][N+1] or NULL */, int k, double cg_tol, int precond /* 0 | 1 */,
                  double *resid_out /* [B][k] */, double *curv_out /* [B][k] */, double *pred_out /* [B] */,
                  double *rnorm0_out /* [B] */, int32_t *steps_out /* [B] */, int32_t *status_out /* [B] */,
                  int64_t *n_free_out /* [B] */, vch_stats *stats);
/* Truncated (Steihaug-Toint) Newton-CG in a trust region on the free set of the 1D engine (ABI version stays 3:
 * detect this entry point and vch1d_pgd_trust by symbol).  The arguments, base point, resident mode, mask, precond, outputs,
 * looks, storage, invalidation rules and errors are those of vch1d_hess_cg, plus radius [B] and xnorm_out [B].  The region is
 * ||x||_D <= radius_b in the preconditioner's norm, ||x||_D^2 = sum D x^2 with D = diag(wt'_k wx_i) for precond 1 and the
 * identity for precond 0.  The iteration is vch1d_hess_cg's with xx = ||x||_D^2 and xp = x.D p kept by their recurrences
 * (x_0 = 0: both start at 0), tau the positive root of xx + 2 tau xp + tau^2 pp = radius^2 (pp = p.D p).  At step j, after
 * c = p.P H p:
 *   c not finite: VCH_CG_BREAKDOWN, as vch1d_hess_cg;
 *   !(c > 0): the step tau along p to the boundary, then VCH_CG_NEGCURV ("stepped to the boundary along a direction of
 *     non-positive curvature"; at step 0, x = tau D^-1 P b).  With radius +inf there is no boundary: the call stops as
 *     vch1d_hess_cg does, x the iterate before that direction;
 *   the step rho / c would leave the region: the step tau to the boundary, then VCH_CG_BOUNDARY;
 *   otherwise the step of vch1d_hess_cg, with its stop rules.
 * A step to the boundary updates x and r as any step does (r = P b - P H P x stays true for vch1d_cg_vector), adds
 * tau rho - tau^2 c / 2 to pred, writes resid[j] and counts in steps_out.  xnorm_out [B]: ||x||_D by the recurrence (0 for
 * P b == 0).  With radius = +inf every output, x, r and p are bitwise those of vch1d_hess_cg on a trajectory that ends
 * VCH_CG_CONVERGED or VCH_CG_LIMIT.  The kernel forms radius^2 in a double: a radius whose square is not finite (>= 2^512)
 * has no boundary and acts as +inf; a radius whose square underflows gives a zero step (tau = 0: x = 0, r = P b, pred = 0
 * after one counted step, VCH_CG_BOUNDARY, or VCH_CG_NEGCURV where the first direction has non-positive curvature).
 * VCH_ERR_ARG, before anything is enqueued, for NULL radius or xnorm_out and a radius_b that is not > 0 (NaN included). */
int vch1d_hess_cg_tr(vch1d_ctx *ctx, const double *phi_hist, const double *u, int n_base, int rows,
                     const double *dt, const double *t_hist, const double *x,
                     const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts,
                     const uint8_t *mask /* [n_base][rows][N+1] or NULL */, double tol,
                     const double *rhs  /* [B][rows][N+1] or NULL */, int k, double cg_tol, int precond /* 0 | 1 */,
                     double *resid_out /* [B][k] */, double *curv_out /* [B][k] */, double *pred_out /* [B] */,
                     double *rnorm0_out /* [B] */, int32_t *steps_out /* [B] */, int32_t *status_out /* [B] */,
                     int64_t *n_free_out /* [B] */, vch_stats *stats, const double *radius /* [B] */,
                     double *xnorm_out /* [B] */);
#define VCH_CG_BOUNDARY 4
/* out = x (which 0), r (1) or p (2) of the last vch1d_hess_cg of this context; masked-off nodes are exact zeros.
 * VCH_ERR_STATE without resident vectors (no call yet, a failed call, or a vch1d_hess_lanczos since). */
int vch1d_cg_vector(vch1d_ctx *ctx, int which /* 0: x, 1: r, 2: p */, double *out /* [B][rows][N+1] */);
/* Damped Newton rounds on the free set about the resident PGD iterate of the 1D engine, batched, with every trajectory's own
 * parameters and decisions (the 1D counterpart of vch2d_pgd_newton, whose comment holds every rule not
 * repeated here; ABI version stays 3: detect both entry points by symbol).  The rounds run about the iterate of
 * vch1d_pgd_init / _init_v and whatever vch1d_pgd_iterate did since.  No history crosses the bus.  There is no rtol: the 1D
 * solves are direct.  Three things differ from the 2D round: there is no shift record; the control has rows = M + 2 rows
 * like the state; the free set and the step cover all rows, the duplicated t = 0 row included.  Per round and trajectory:
 *   1. the Newton-CG solve of vch1d_hess_cg in its resident mode (resident phi_hist, u = phi_Q = phi_T = VCH_RESIDENT,
 *      rhs = NULL, mask = NULL, the dt, t_hist, x of vch1d_pgd_init and opts[b]; k, cg_tol, precond, tol as passed).  An empty
 *      free set is no error here: zero steps, VCH_CG_CONVERGED, pred = rnorm0 = 0, and vch1d_cg_vector returns zeros for it.
 *   2. the verdict after the solve, as in 2D: VCH_NEWTON_STATIONARY, VCH_NEWTON_NEGCURV, VCH_NEWTON_BREAKDOWN, or x is the step.
 *   3. trials for s = 1, 1/2, ..., at most max_halvings halvings: t = min(max(u + s x, u_min_b), u_max_b), a free node with
 *      t u < 0 becomes 0 (k1d_nt_trial into the trial-control scratch), a march of t into the trial-state scratch and its
 *      cost.  The first s with J(t) <= cost_b - 1e-4 s pred_b is accepted: control and state history are copied as the PGD
 *      loop copies an accepted trial and the stored cost becomes the trial's (VCH_NEWTON_ACCEPTED).  When no s is accepted
 *      the trajectory is left unmoved with VCH_NEWTON_STALLED.
 * A trajectory that has ended is VCH_NEWTON_IDLE in all later rounds, its doubles NaN, its integers 0; its solves are not
 * gated.  The call returns the number of rounds run and stops early once every trajectory has ended.  The outputs are those of
 * vch2d_pgd_newton (all [B][n_rounds] and required, counts_out [B][n_rounds][3] = {n_free, and of the round's last trial:
 * nodes pinned to 0, nodes the clip moved}; seconds_out [4], may be NULL, = {solves, trial kernel, marches, costs}).  No
 * atomics: a trajectory's outputs and its iterate are bitwise those of a single-trajectory context.
 * Three departures from the host loop GD_1D.newton_refine:
 *   (1) a CG breakdown ends the trajectory; no march is started under a control that may not be finite (as in 2D);
 *   (2) a trial march that reports a non-finite mass defect does not fail the call: that trajectory's trial counts as not
 *       accepted and s is halved (a cost that is not finite is never accepted);
 *   (3) the 1D stop quirk: after a trajectory's PGD stop rule fired the resident control is the new iterate and the
 *       resident state and the stored cost are the previous one's.  Before round 0 the call marches the resident control of
 *       every such trajectory once (one batched march, the other members sit it out), takes its cost, copies the state into
 *       the resident history and stores the cost.  A stopped trajectory is never iterated again, so this changes nothing
 *       that a later vch1d_pgd_iterate computes.
 * Afterwards vch1d_pgd_get, vch1d_second_order, vch1d_hessvec, vch1d_hess_lanczos and vch1d_hess_cg (resident mode) work about
 * the new iterate, vch1d_cg_vector returns the last round's vectors, the adjoint r of vch1d_pgd_kkt(refresh = 0) is invalid
 * once any trajectory moved, and the counters of the PGD loop (iteration count, plateau, next first step, stop flags, error
 * histories) are untouched: a following vch1d_pgd_iterate is bit for bit that of vch1d_pgd_init_v with u0 = the Newton
 * iterate, and after a call that accepted nothing that of an undisturbed run.
 * Storage beyond that of vch1d_hess_cg and the PGD buffers: the [B] step table, the skip flags and the partials of the trial
 * kernel's four sums, which have cells of their own in the block of the Krylov scalars (the same group: a refused request
 * releases the group and returns VCH_ERR_NOMEM with the bytes in the message; the context stays usable).
 * Errors, all before anything is enqueued, copied or allocated: VCH_ERR_STATE before vch1d_pgd_init / _init_v; VCH_ERR_ARG for
 * n_rounds < 1, k < 1, max_halvings < 0, precond outside 0 / 1, a cg_tol that is not finite and NULL outputs, and with
 * precond 1 for the time-weight check of vch1d_hess_cg.  A ||P b|| that is not finite is VCH_ERR_ARG naming the trajectory,
 * after the set-up's look, as in vch1d_hess_cg. */
int vch1d_pgd_newton(vch1d_ctx *ctx, int n_rounds, int k, double cg_tol, int precond /* 0 | 1 */, double tol, int max_halvings,
                     double *cost_out, double *cost_new_out, double *s_out, double *pred_out,
                     double *rnorm0_out /* [B][n_rounds] */, int32_t *halvings_out, int32_t *cg_steps_out,
                     int32_t *cg_status_out, int32_t *status_out /* [B][n_rounds] */,
                     int64_t *counts_out /* [B][n_rounds][3]: n_free, pinned, clipped */,
                     double *seconds_out /* [4] or NULL: solves, trial kernel, marches, costs */);
/* Trust-region (Steihaug) Newton-CG rounds on the free set about the resident PGD iterate of the 1D engine, batched, with
 * every trajectory's own parameters, radius and decisions (ABI version stays 3: detect by symbol).  The
 * checks, the stop quirk before round 0, the resident state afterwards and the untouched PGD counters are those of
 * vch1d_pgd_newton; pgd_r_valid is cleared once anything moved.  Per round and live trajectory b, with radius Delta_b
 * (radius0_b in round 0):
 *   1. the solve of vch1d_hess_cg_tr in its resident mode (as step 1 of vch1d_pgd_newton) inside Delta_b.
 *   2. VCH_NEWTON_STATIONARY (empty free set or ||P b|| == 0) and VCH_NEWTON_BREAKDOWN end the trajectory without a trial.
 *      Every other CG exit, VCH_CG_NEGCURV included, gives a step x.
 *   3. one trial at s = 1 (the trial of vch1d_pgd_newton: clip to the box, a free node with t u < 0 becomes 0), its march
 *      and its cost J(t); rho = (J(u) - J(t)) / pred.
 *   4. accepted iff J(t) is finite and J(t) <= J(u) - 1e-4 pred (the damped rounds' Armijo test at s = 1), copied as
 *      vch1d_pgd_newton copies a trial: VCH_NEWTON_ACCEPTED.  Otherwise the trajectory stays unmoved: VCH_NEWTON_REJECTED,
 *      and it goes on to the next round.
 *   5. the radius: rho < 1/4 or not finite: Delta = min(Delta, ||x||_D) / 4; else rho > 3/4 after VCH_CG_BOUNDARY or
 *      VCH_CG_NEGCURV: Delta = min(2 Delta, radius_max).  A Delta below radius_min ends the trajectory: a rejected one
 *      with VCH_NEWTON_STALLED, an accepted one keeps VCH_NEWTON_ACCEPTED.
 * An ended trajectory is VCH_NEWTON_IDLE in all later rounds, its doubles NaN, its integers 0; its solves are not gated (they
 * run with its radius0).  The call returns the rounds run and stops early once every trajectory has ended.  Outputs, all
 * required and [B][n_rounds]: cost (J(u) before the trial), cost_new (after the round), pred, rnorm0, radius (the round's
 * Delta), ratio (rho; NaN without a trial), xnorm (||x||_D), cg_steps, cg_status (VCH_CG_*), status (VCH_NEWTON_*);
 * counts_out [B][n_rounds][3] = {n_free, pinned, clipped of the trial}; seconds_out [4] or NULL = {solves, trial kernel,
 * marches, costs}.  No atomics: a trajectory's outputs and its iterate are bitwise those of a single-trajectory context.
 * Storage: that of vch1d_pgd_newton.  Errors, all before anything is enqueued, copied or allocated: VCH_ERR_STATE before
 * vch1d_pgd_init / _init_v; VCH_ERR_ARG for n_rounds < 1, k < 1, precond outside 0 / 1, a cg_tol that is not finite, NULL
 * radius0, a radius0_b, radius_max or radius_min that is not finite or not > 0, NULL outputs, and with precond 1 the
 * time-weight check of vch1d_hess_cg. */
int vch1d_pgd_trust(vch1d_ctx *ctx, int n_rounds, int k, double cg_tol, int precond /* 0 | 1 */, double tol,
                    const double *radius0 /* [B] */, double radius_max, double radius_min,
                    double *cost_out, double *cost_new_out, double *pred_out, double *rnorm0_out, double *radius_out,
                    double *ratio_out, double *xnorm_out /* [B][n_rounds] */, int32_t *cg_steps_out, int32_t *cg_status_out,
                    int32_t *status_out /* [B][n_rounds] */, int64_t *counts_out /* [B][n_rounds][3]: n_free, pinned, clipped */,
                    double *seconds_out /* [4] or NULL: solves, trial kernel, marches, costs */);
/* The trial kernel's seam, after any successful vch1d_hess_cg, stateless or resident: t = min(max(u + s_b x, u_min_b),
 * u_max_b) with u that call's base control (a shared base: one for the batch; NULL: zeros), x, the free set and the box the
 * ones it left resident; a free node with t u < 0 becomes 0.  Writes only the trial-control scratch (allocated on first use
 * when no PGD problem was loaded) and leaves x, r, p resident.  u_out (may be NULL): the trial; chg_out [B][2] =
 * {sum (t - u)^2, sum u^2} in a fixed order, no atomics; counts_out [B][2] = {nodes pinned to 0, nodes the clip moved}.  For
 * s a power of two the trial has the bits of NumPy's np.clip(u + s * x, lo, hi).  VCH_ERR_STATE without resident CG vectors
 * (or when a later call has overwritten the copy of an uploaded base control); VCH_ERR_ARG for NULL s, chg_out or
 * counts_out and an s_b that is not finite or not > 0. */
int vch1d_newton_trial(vch1d_ctx *ctx, const double *s /* [B] */, double *u_out /* [B][rows][N+1] or NULL */,
                       double *chg_out /* [B][2] */, int64_t *counts_out /* [B][2]: pinned, clipped */);

/* ---------------------------------------------------------- diagnostics ---- */

/* Every device and pinned-host block of a context belongs to the context's pool (csrc/vch_mem.h): vchNd_destroy, and a
 * vchNd_create that fails, free all of them.  Number of blocks that pools of this process own now (one atomic counter): */
int vch_mem_live(void);
/* The allocation request number k of this process, counted from this call (0 = the next one), is refused once, as an
 * out-of-memory answer of the runtime would refuse it but without a call to the runtime; k < 0 disarms.  For tests of the
 * failure paths: a refused vchNd_create returns NULL with nothing left behind, a refused lazy allocation fails its call with
 * VCH_ERR_HIP or VCH_ERR_NOMEM and leaves its group of buffers unallocated, so the same call succeeds when repeated. */
void vch_mem_refuse_after(int k);

#ifdef __cplusplus
}
#endif
#endif /* VCH_H */
