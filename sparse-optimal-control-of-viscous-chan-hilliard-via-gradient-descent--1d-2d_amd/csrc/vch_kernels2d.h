// vch_kernels2d.h — hand-written HIP kernels of the 2D hot path (gfx950, wave64, fp64).
//
// All kernels are batched over B independent trajectories (blockIdx.z) and work on
// TX x TY tiles of one padded plane, staged through LDS with a mirrored (reflect) halo so
// that the Neumann boundary rows need no branches: the mirrored ghost v[-1] = v[1]
// reproduces the doubled off-diagonals of the reference's Laplacian (F2:119-121), and
// applying the same rule twice reproduces its L@L (B2:159).
//
// Per-trajectory control flow (Newton convergence, Armijo acceptance, linear-solver
// convergence) lives in a small TrajState record in device memory; stencil kernels read
// it and return early for trajectories that are not in the corresponding phase, tiny
// `fin` kernels (one workgroup per trajectory) update it from per-workgroup partials in a
// fixed order, so results are deterministic run to run.
#pragma once
#include "vch_common.h"
#include "vch_gp.h"

struct TrajState {
    // Newton iteration (F2:323-427)
    int slot;            // which of the two iterate buffers holds (phi+, mu+, R_phi, rhs, D)
    int newton_active;   // Newton loop still running for this trajectory
    int need_trial;      // an Armijo trial (or the initial residual) is pending
    int trial_no;        // halvings done in the current Armijo loop
    int force_accept;    // take the pending trial unconditionally (best-trial fallback F2:420-423)
    int iters;           // residual norms recorded (= len(hist))
    int nsolves;         // linear solves started
    int ntrials;         // Armijo residual evaluations
    int stuck;           // 12 trials failed and no trial improved: state can never change again
    int frozen;          // trajectory sits this march out (its line search has already accepted, G2:128-146)
    double normR;        // ||[R_phi;R_mu]||_2 of the current iterate
    double alpha;        // step of the pending trial
    double best_norm, best_alpha;
    double Dmin, Dmax, dbar;   // range of the Jacobian diagonal, preconditioner shift
    double rho;                // bound of the CG contraction per iteration from the spectrum of P^-1 A (cg_setup)
    double kT;                 // the bound of that spectrum itself: spec(P^-1 A) in [1, kT]
    long newton_total;         // residual norms recorded over the whole march
    // linear solve (preconditioned CG on the Schur system)
    int lin_active, lin_it;
    long lin_total;
    double lin_r0, lin_prev, lin_rel, lin_maxrel;
    // conjugate gradients in the weighted inner product (see k_schur_p)
    double cg_gamma, cg_gamma0, cg_alpha, cg_beta;
    int lin_budget;            // rigorous iteration bound from the spectrum of P^-1 A
    // inexact Newton (forward solves inside a march): relative tolerance of THIS solve, chosen in k_fin_residual so that
    // the Schur residual it leaves -- which is the nonlinear residual of the next iterate up to second-order terms --
    // is a small fraction of the Newton tolerance; lin_maxabs = worst (final relative residual x ||rhs||_2) of a solve
    double lin_reltol, lin_maxabs;
    // starting guess of the step's first / second Newton solve (k_guess): the sweeps of THIS solve start from x = x0 instead
    // of 0 and solve for the deflated right-hand side rhs - A x0; lin_rscale = ||rhs - A x0|| / ||rhs|| keeps lin_maxrel
    // relative to ||rhs||
    int x_primed, guess_pad;
    double lin_rscale;
    double guess_ratio;        // ||rhs - A x0|| / ||rhs|| of this step's guess (uncapped), for the host's choice of the order
    double guess_ratio2;       // the same for the guess of the step's SECOND Newton solve (0 = no such guess this step)
    // per time step, for the host's launch schedule: linear solves started and the longest of them
    int step_solves, step_lin_max;
    int step_lin[4];           // sweeps of the first four solves of the step
    double step_tol[4], step_kT[4];   // their relative tolerances and the bounds kappa_T of the spectrum of P^-1 A
    int step_chn[4];           // ... and the sweeps a Chebyshev solve of them needs (cheb_plan), whichever solver ran
    // reduction-free (Chebyshev) form of the forward solve (vch_fft.h, k_cheb_rows): spec(P^-1 A) in [theta - delta,
    // theta + delta] = [1, kT] and the number of sweeps after which the rigorous bound 1 / T_{n+1}(theta/delta) is below
    // the solve's tolerance -- all known before the solve starts, so no inner product steers it
    int cheb_n;
    int use_cheb;              // THIS solve takes the reduction-free form (its plan is short): decided per trajectory and per
                               // solve on the device, so a trajectory's arithmetic does not depend on its batch mates
    double cheb_theta, cheb_delta;
    int step_form[4];          // use_cheb of the step's first four solves (host: which launch sequences the next step needs)
    // CG form on a diagonal that spans a wide range (a few nodes near |phi| = 1 among ordinary ones): the solve runs on the
    // right-scaled system  P^-1 A S y = P^-1 rhs,  x = S y,  S = dbar / D  (see cg_scaled below)
    int scaled;
    int lin_capped;            // adjoint sweep: this solve ended on the trajectory's own sweep cap (lin_cap) above its tolerance
    double step_R[4];          // residual norms of the step's first four iterates (R_0 .. R_3), for the host's statistics
    // ||R_1|| (the residual after the first Newton iteration) of the last three time steps, newest first; 0 = not known yet.
    // It is the quadratic remainder of the first iteration, three to four orders above the Newton tolerance in the bench
    // regime and smooth along a march (ratio from step to step 0.68 .. 1.03 at the 1 % / 99 % quantiles,
    // profiles/r03_first_solve_slack.txt): the first solve of the next step need not be more accurate than a small fraction of it
    double R1_hist[3];
    int lin_took, lin_unconv;  // adjoint: this solve started (its y is valid); solves the enqueued sweeps did not finish
    int cg_pending, cg_pbuf;   // forward CG: step (alpha, p[cg_pbuf]) computed but not yet added to x
    // adjoint sweep: the sweeps a solve of this trajectory may take, from its own record at the host's last look
    // (backward_pass, k_adj_caps); 0 = no cap.  The host enqueues the largest cap of the batch, so what a trajectory's
    // solve gets does not depend on its batch mates
    int lin_cap;
    // forward CG, per-iteration state in two copies: iteration k's stencil kernel derives the step of
    // iteration k-1 itself (every workgroup, redundantly), reading copy (k-1)&1 while one workgroup
    // writes copy k&1 -- no workgroup ever reads a field that another one writes in the same launch
    int ci_active[2], ci_it[2];
    double ci_gamma[2];
    // mass fix (F2:565-577)
    double mass0, mass_err, Wint;
    // scratch for cost / change norms
    double aux[4];
};

// gate codes of the preconditioner kernels: 1 = lin_active, 2 / 3 = copy 0 / 1 of the forward CG's per-iteration flag
// 4 = the adjoint solve of this step took place (lin_took)
// 16 + j = the column pass in front of sweep j of a Chebyshev solve (the trajectory is solving and needs that sweep)
// 5 = solving in the CG form (lin_active and not use_cheb), 8 = solving in the reduction-free form
__device__ __forceinline__ bool gate_open(const TrajState &S, int gate) {
    if (gate >= 16) return S.lin_active != 0 && S.use_cheb != 0 && gate - 16 <= S.cheb_n;
    if (gate == 5) return S.lin_active != 0 && S.use_cheb == 0;
    if (gate == 8) return S.lin_active != 0 && S.use_cheb != 0;
    return gate == 1 ? S.lin_active != 0 : (gate == 4 ? S.lin_took != 0 : S.ci_active[gate - 2] != 0);
}

// sweeps a solve may take: the engine's limit, or below it the trajectory's own cap (adjoint sweep)
__device__ __forceinline__ int lin_limit(const TrajState &S, int maxit) {
    return S.lin_cap > 0 && S.lin_cap < maxit ? S.lin_cap : maxit;
}

struct Phys {
    double tau, gamma, c1, c2, kappa;
    double LxLy;
};

// ---------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------
__device__ __forceinline__ int refl(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return i < 0 ? 0 : i;
}

// Global offset of element e of a thread's share of the haloed tile (e < W * HT).
template <int H>
__device__ __forceinline__ long tile_off(int e, const Geom &G, int c0, int r0) {
    constexpr int W = TX + 2 * H;
    int ly = e / W, lx = e - ly * W;
    int gr = refl(r0 - H + ly, G.ns), gc = refl(c0 - H + lx, G.nf);
    return (long)gr * G.pitch + gc;
}
// A thread's share of a haloed tile, requested into registers (tile_fetch) and written to LDS later (tile_put): a kernel
// puts its other global requests between the two, so that they all travel together.
template <int H>
struct TileRegs {
    static constexpr int N = (TX + 2 * H) * (TY + 2 * H), I = (N + NTH - 1) / NTH;
    double v[I];
};
template <int H>
__device__ __forceinline__ void tile_fetch(TileRegs<H> &t, const double *__restrict__ g, const Geom &G, int c0, int r0) {
#pragma unroll
    for (int i = 0; i < TileRegs<H>::I; ++i) {
        const int e = threadIdx.x + i * NTH;
        t.v[i] = 0.0;
        if (e < TileRegs<H>::N) t.v[i] = g[tile_off<H>(e, G, c0, r0)];
    }
}
template <int H>
__device__ __forceinline__ void tile_put(double *s, const TileRegs<H> &t) {
#pragma unroll
    for (int i = 0; i < TileRegs<H>::I; ++i) {
        const int e = threadIdx.x + i * NTH;
        if (e < TileRegs<H>::N) s[e] = t.v[i];
    }
}

// BATCH (the default): a compile-time trip count, every element of the thread requested before the first LDS write -- one
// wait for global memory per tile.  BATCH = false is the rolled loop (one wait per element) that the _plain kernels keep, and
// k_adj_rhs / k_adj_op, whose batched forms did not pay under the bench's two contexts.
template <int H, bool BATCH = true>
__device__ __forceinline__ void load_tile(double *s, const double *__restrict__ g, const Geom &G,
                                          int c0, int r0) {
    if (BATCH) {
        TileRegs<H> t;
        tile_fetch<H>(t, g, G, c0, r0);
        tile_put<H>(s, t);
    } else {
        constexpr int W = TX + 2 * H, HT = TY + 2 * H;
        for (int e = threadIdx.x; e < W * HT; e += NTH) {
            int ly = e / W, lx = e - ly * W;
            int gr = refl(r0 - H + ly, G.ns), gc = refl(c0 - H + lx, G.nf);
            s[e] = g[(long)gr * G.pitch + gc];
        }
    }
}

// s = a + alpha * d on the haloed tile
template <int H>
__device__ __forceinline__ void load_tile_axpy(double *s, const double *__restrict__ a,
                                               const double *__restrict__ d, double alpha,
                                               const Geom &G, int c0, int r0) {
    constexpr int W = TX + 2 * H, HT = TY + 2 * H;
    for (int e = threadIdx.x; e < W * HT; e += NTH) {
        int ly = e / W, lx = e - ly * W;
        int gr = refl(r0 - H + ly, G.ns), gc = refl(c0 - H + lx, G.nf);
        long o = (long)gr * G.pitch + gc;
        s[e] = a[o] + alpha * d[o];
    }
}

// 5-point mirrored-Neumann Laplacian at LDS position p of a tile with row stride W
template <int W>
__device__ __forceinline__ double lap_at(const double *s, int p, double ax, double ay) {
    double c = s[p];
    return ax * ((s[p - 1] + s[p + 1]) - 2.0 * c) + ay * ((s[p - W] + s[p + W]) - 2.0 * c);
}

__device__ __forceinline__ double reglog(double phi) {   // F2:86-102 with delta_sep = 1e-2
    const double eps = 0.5 * DELTA_SEP;                  // max(1e-8, delta_sep/2)
    double p = fmin(fmax(phi, -1.0 + eps), 1.0 - eps);
    return log((1.0 + p) / (1.0 - p));
}

__device__ __forceinline__ double jac_diag(double phi, double tau_dt, double c1) {   // F2:243-244
    double psq = fmin(fmax(phi * phi, 0.0), 1.0 - DELTA_SEP * DELTA_SEP);
    return tau_dt + 2.0 * c1 / (1.0 - psq);
}

__device__ __forceinline__ double fpp_log(double phi, double c1, double c2) {   // B2:71-72
    double p = fmin(fmax(phi, -1.0 + 1e-8), 1.0 - 1e-8);
    return 2.0 * c1 / (1.0 - p * p) - 2.0 * c2;
}

// trapezoid weight of node (r, c) of the plane as the engine stores it; M = -L is self-adjoint
// in the inner product weighted by it (W L is symmetric)
__device__ __forceinline__ double wdev(int r, int c, const Geom &G) {
    return ((r == 0 || r == G.ns - 1) ? 0.5 : 1.0) * ((c == 0 || c == G.nf - 1) ? 0.5 : 1.0);
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    return v;
}

// Workgroup reduction of up to NPART values per thread (op: 0 sum, 1 min, 2 max); thread 0
// writes the results to part[0..n).  sred must hold NPART*4 doubles.
template <int N>
__device__ __forceinline__ void block_reduce_store(double (&v)[N], const int (&op)[N], double *sred,
                                                   double *part) {
    int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double r = op[k] == 0 ? wave_sum(v[k]) : (op[k] == 1 ? wave_min(v[k]) : wave_max(v[k]));
        if (lane == 0) sred[k * 4 + wv] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double a = sred[k * 4], b = sred[k * 4 + 1], c = sred[k * 4 + 2], d = sred[k * 4 + 3];
            part[k] = op[k] == 0 ? (a + b) + (c + d)
                                 : (op[k] == 1 ? fmin(fmin(a, b), fmin(c, d)) : fmax(fmax(a, b), fmax(c, d)));
        }
    }
}

// XCD-aware bijective remap of a 1-D block index: workgroups are dealt round-robin over the 8
// XCDs (blocks b and b+8 share an L2), so logically adjacent work items -- which here share
// 128-byte lines -- are given to the SAME XCD in contiguous chunks.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int bid, int n) {
    const int q = n >> 3, r = n & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Tile of a stencil workgroup: the workgroups of one plane that land on the same XCD (dispatch index
// mod 8) are given a contiguous, column-major run of tiles, so vertically adjacent tiles -- whose 2-row
// halos are a quarter of a 64 x 16 tile -- meet in one L2; every XCD still gets an equal share of
// every trajectory.  blk doubles as the (bijective) index of the workgroup's reduction partial.
#define TILE_COORDS                                   \
    const int b = blockIdx.z;                         \
    const int nblk = gridDim.x * gridDim.y;           \
    const int blk = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, nblk); \
    const int c0 = (blk / (int)gridDim.y) * TX, r0 = (blk % (int)gridDim.y) * TY; \
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6; \
    (void)blk; (void)nblk; (void)lx; (void)ly0

// ---------------------------------------------------------------------------------
// out = L v                                                  (apply_laplacian, F2:140-152)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_lap(Geom G, const double *__restrict__ v, double *__restrict__ out) {
    TILE_COORDS;
    __shared__ double s[(TY + 2) * (TX + 2)];
    constexpr int W = TX + 2;
    load_tile<1>(s, v + b * G.plane, G, c0, r0);
    __syncthreads();
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf)
            out[b * G.plane + (long)r * G.pitch + c] = lap_at<W>(s, (ly + 1) * W + lx + 1, G.ax, G.ay);
    }
}

// ---------------------------------------------------------------------------------
// mu = -kappa L phi + c1 reglog(phi) - 2 c2 phi - w           (initialize_mu, F2:155-167)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_init_mu(Geom G, Phys P, const double *__restrict__ phi,
                                                 const double *__restrict__ w, double *__restrict__ mu) {
    TILE_COORDS;
    __shared__ double s[(TY + 2) * (TX + 2)];
    constexpr int W = TX + 2;
    load_tile<1>(s, phi + b * G.plane, G, c0, r0);
    __syncthreads();
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p = (ly + 1) * W + lx + 1;
            long o = b * G.plane + (long)r * G.pitch + c;
            double ph = s[p];
            mu[o] = -P.kappa * lap_at<W>(s, p, G.ax, G.ay) + (P.c1 * reglog(ph) - 2.0 * P.c2 * ph) - w[o];
        }
    }
}

// Start of a Newton call: arm the initial residual evaluation (done by one thread of k_prepare: the fields it sets are
// read by no other workgroup of that launch).
__device__ __forceinline__ void newton_begin(TrajState &S) {
    if (S.frozen) {
        S.newton_active = S.need_trial = S.lin_active = 0;
        return;
    }
    S.newton_active = 1;
    S.need_trial = 1;
    S.trial_no = 0;
    S.force_accept = 1;     // the initial residual is always "accepted"
    S.iters = 0;
    S.stuck = 0;
    S.alpha = 0.0;
    S.lin_active = 0;
    S.step_solves = 0;
    S.step_lin_max = 0;
    S.step_lin[0] = S.step_lin[1] = S.step_lin[2] = S.step_lin[3] = 0;
    S.step_chn[0] = S.step_chn[1] = S.step_chn[2] = S.step_chn[3] = 0;
    S.step_form[0] = S.step_form[1] = S.step_form[2] = S.step_form[3] = 0;
    S.use_cheb = 0;
    S.scaled = 0;
    S.x_primed = 0;
    S.lin_rscale = 1.0;
    S.guess_ratio = 1.0;
    S.guess_ratio2 = 0.0;
}

// ---------------------------------------------------------------------------------
// Start of a time step (F2:545-551, F2:350-351).  From the old level (phi, mu, w) and the
// control rows u_n, u_{n+1} (NULL = zeros) form
//   w_new = ((g-1/2) w + (u_n+u_{n+1})/2)/(g+1/2), g = gamma/dt          (solve_w, F2:180-181)
//   mu0   = -kappa L phi + c1 reglog(phi) - 2 c2 phi - w_new            (Newton initial guess)
//   c_phi = -(tau/dt) phi - kappa/2 L phi - 2 c2 phi - mu/2 - (w_new + w)/2   old-level part of R_phi
//   c_mu  = -phi/dt - L mu / 2                                                 old-level part of R_mu
// (wnew_in != NULL: w_new is given, as in a bare newton_raphson call, F2:323)
// so that R_phi = (tau/dt) phi+ - kappa/2 L phi+ + c1 reglog(phi+) - mu+/2 + c_phi and
// R_mu = phi+/dt - L mu+/2 + c_mu (F2:194-221 with the old-level terms pre-combined).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_prepare(Geom G, Phys P, TrajState *__restrict__ st,
                                                 long slot_stride, const double *__restrict__ phi_s,
                                                 const double *__restrict__ mu_s, const double *__restrict__ w,
                                                 const double *__restrict__ un, const double *__restrict__ unp1,
                                                 long u_stride, const double *__restrict__ wnew_in, double dt,
                                                 double *__restrict__ wnew,
                                                 double *__restrict__ mu0, double *__restrict__ cphi,
                                                 double *__restrict__ cmu) {
    TILE_COORDS;
    __shared__ double sp[(TY + 2) * (TX + 2)];
    __shared__ double sm[(TY + 2) * (TX + 2)];
    constexpr int W = TX + 2;
    if (blk == 0 && threadIdx.x == 0) newton_begin(st[b]);
    if (st[b].frozen) return;
    const int slot = st[b].slot;
    load_tile<1>(sp, phi_s + slot * slot_stride + b * G.plane, G, c0, r0);
    load_tile<1>(sm, mu_s + slot * slot_stride + b * G.plane, G, c0, r0);
    __syncthreads();
    const double gdt = P.gamma / dt;
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p = (ly + 1) * W + lx + 1;
            long o = (long)r * G.pitch + c;
            long ob = b * G.plane + o;
            double u0 = un ? un[b * u_stride + o] : 0.0, u1 = unp1 ? unp1[b * u_stride + o] : 0.0;
            double wo = w[ob];
            double wn = wnew_in ? wnew_in[ob] : ((gdt - 0.5) * wo + 0.5 * (u1 + u0)) / (gdt + 0.5);
            double ph = sp[p], lp = lap_at<W>(sp, p, G.ax, G.ay), lm = lap_at<W>(sm, p, G.ax, G.ay);
            wnew[ob] = wn;
            mu0[ob] = -P.kappa * lp + (P.c1 * reglog(ph) - 2.0 * P.c2 * ph) - wn;
            cphi[ob] = -(P.tau / dt) * ph - 0.5 * P.kappa * lp - 2.0 * P.c2 * ph - 0.5 * sm[p] - 0.5 * (wn + wo);
            cmu[ob] = -ph / dt - 0.5 * lm;
        }
    }
}

// ---------------------------------------------------------------------------------
// Residual of a Newton iterate / Armijo trial (F2:357-360, F2:399-408), fused with
// everything the next linear solve needs:
//   MODE 0 (initial residual): iterate = (phi[slot], mu0)      -> written to slot `slot`
//   MODE 1 (trial):            iterate = (phi, mu)[slot] + alpha (dphi, dmu) -> slot 1-slot
// Outputs per node: phi_t, mu_t, R_phi, D = tau/dt + 2c1/(1-clip(phi_t^2)) (F2:243-244) and
// the Schur right-hand side rhs = -R_mu + L R_phi; per workgroup: sum(R_phi^2 + R_mu^2),
// sum(rhs^2), min D, max D.
// ---------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(NTH) void k_residual(Geom G, Phys P, const TrajState *__restrict__ st,
                                                  long slot_stride, double *__restrict__ phi_s,
                                                  double *__restrict__ mu_s, double *__restrict__ Rphi_s,
                                                  double *__restrict__ rhs_s, double *__restrict__ D_s,
                                                  const double *__restrict__ mu0, const double *__restrict__ dphi,
                                                  const double *__restrict__ dmu, const double *__restrict__ cphi,
                                                  const double *__restrict__ cmu, double dt,
                                                  double *__restrict__ part) {
    TILE_COORDS;
    const TrajState S = st[b];
    if (!S.newton_active || !S.need_trial) return;
    __shared__ double sp[(TY + 4) * (TX + 4)];
    __shared__ double sm[(TY + 2) * (TX + 2)];
    __shared__ double sr[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    constexpr int W2 = TX + 4, W1 = TX + 2;
    const long pb = b * G.plane;
    const int src = S.slot, dst = MODE == 0 ? S.slot : 1 - S.slot;
    if (MODE == 0) {
        load_tile<2>(sp, phi_s + src * slot_stride + pb, G, c0, r0);
        load_tile<1>(sm, mu0 + pb, G, c0, r0);
    } else {
        load_tile_axpy<2>(sp, phi_s + src * slot_stride + pb, dphi + pb, S.alpha, G, c0, r0);
        load_tile_axpy<1>(sm, mu_s + src * slot_stride + pb, dmu + pb, S.alpha, G, c0, r0);
    }
    __syncthreads();
    const double tdt = P.tau / dt;
    // R_phi on the tile + halo 1
    for (int e = threadIdx.x; e < (TY + 2) * W1; e += NTH) {
        int ly = e / W1, lxx = e - ly * W1;
        int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
        int p2 = (ly + 1) * W2 + lxx + 1;
        double ph = sp[p2];
        sr[e] = tdt * ph - 0.5 * P.kappa * lap_at<W2>(sp, p2, G.ax, G.ay) + P.c1 * reglog(ph) - 0.5 * sm[e] +
                cphi[pb + (long)gr * G.pitch + gc];
    }
    __syncthreads();
    double acc[4] = {0.0, 0.0, 1e300, -1e300};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
            long o = pb + (long)r * G.pitch + c;
            double ph = sp[p2], rp = sr[p1];
            double rm = ph / dt - 0.5 * lap_at<W1>(sm, p1, G.ax, G.ay) + cmu[o];
            double rh = -rm + lap_at<W1>(sr, p1, G.ax, G.ay);
            double d = jac_diag(ph, tdt, P.c1);
            long od = dst * slot_stride + o;
            if (MODE == 1) phi_s[od] = ph;
            mu_s[od] = sm[p1];
            Rphi_s[od] = rp;
            rhs_s[od] = rh;
            D_s[od] = d;
            acc[0] += rp * rp + rm * rm;
            acc[1] += rh * rh;
            acc[2] = fmin(acc[2], d);
            acc[3] = fmax(acc[3], d);
        }
    }
    const int op[4] = {0, 0, 1, 2};
    block_reduce_store<4>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// The trial form for the reduction-free solves (cheb_solve): the back substitution dmu = 2 (K dphi + R_phi) (F2:241-253,
// second block row) happens HERE, on the haloed tile, from dphi, D and R_phi of the current iterate -- no kernel between
// the solve and the trial writes dmu (the step ceiling is taken by the solve's last row kernel, k_cheb_rows).  Same
// arithmetic, in the same order, as k_dmu_ceiling followed by k_residual<1>: bit-identical results.
// LDS: phi_t and dphi with halo 2, and ONE halo-1 buffer that holds mu_t first and R_phi afterwards (R_phi at a node needs
// mu_t at that node only, so it is formed in place once the Laplacians of mu_t have been taken).
__global__ __launch_bounds__(NTH) void k_residual2(Geom G, Phys P, const TrajState *__restrict__ st, long slot_stride,
                                                   double *__restrict__ phi_s, double *__restrict__ mu_s,
                                                   double *__restrict__ Rphi_s, double *__restrict__ rhs_s,
                                                   double *__restrict__ D_s, const double *__restrict__ dphi,
                                                   const double *__restrict__ cphi, const double *__restrict__ cmu, double dt,
                                                   double *__restrict__ part) {
    TILE_COORDS;
    const TrajState S = st[b];
    if (!S.newton_active || !S.need_trial) return;
    __shared__ double sp[(TY + 4) * (TX + 4)];
    __shared__ double sd[(TY + 4) * (TX + 4)];
    __shared__ double sm[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    constexpr int W2 = TX + 4, W1 = TX + 2;
    const long pb = b * G.plane;
    const int src = S.slot, dst = 1 - S.slot;
    const double *phi_o = phi_s + src * slot_stride + pb, *mu_o = mu_s + src * slot_stride + pb;
    const double *D_o = D_s + src * slot_stride + pb, *R_o = Rphi_s + src * slot_stride + pb;
    for (int e = threadIdx.x; e < W2 * (TY + 4); e += NTH) {
        int ly = e / W2, lxx = e - ly * W2;
        int gr = refl(r0 - 2 + ly, G.ns), gc = refl(c0 - 2 + lxx, G.nf);
        long o = (long)gr * G.pitch + gc;
        const double d = dphi[pb + o];
        sd[e] = d;
        sp[e] = phi_o[o] + S.alpha * d;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < (TY + 2) * W1; e += NTH) {
        int ly = e / W1, lxx = e - ly * W1;
        int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
        int p2 = (ly + 1) * W2 + lxx + 1;
        long o = (long)gr * G.pitch + gc;
        const double dm = 2.0 * ((-0.5 * P.kappa * lap_at<W2>(sd, p2, G.ax, G.ay) + D_o[o] * sd[p2]) + R_o[o]);
        sm[e] = mu_o[o] + S.alpha * dm;
    }
    __syncthreads();
    const double tdt = P.tau / dt;
    double rm[TY / 4], mt[TY / 4];
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        rm[k] = mt[k] = 0.0;
        if (r < G.ns && c < G.nf) {
            int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
            rm[k] = sp[p2] / dt - 0.5 * lap_at<W1>(sm, p1, G.ax, G.ay) + cmu[pb + (long)r * G.pitch + c];
            mt[k] = sm[p1];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < (TY + 2) * W1; e += NTH) {
        int ly = e / W1, lxx = e - ly * W1;
        int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
        int p2 = (ly + 1) * W2 + lxx + 1;
        double ph = sp[p2];
        sm[e] = tdt * ph - 0.5 * P.kappa * lap_at<W2>(sp, p2, G.ax, G.ay) + P.c1 * reglog(ph) - 0.5 * sm[e] +
                cphi[pb + (long)gr * G.pitch + gc];
    }
    __syncthreads();
    double acc[4] = {0.0, 0.0, 1e300, -1e300};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
            long od = dst * slot_stride + pb + (long)r * G.pitch + c;
            double ph = sp[p2], rp = sm[p1];
            double rh = -rm[k] + lap_at<W1>(sm, p1, G.ax, G.ay);
            double d = jac_diag(ph, tdt, P.c1);
            phi_s[od] = ph;
            mu_s[od] = mt[k];
            Rphi_s[od] = rp;
            rhs_s[od] = rh;
            D_s[od] = d;
            acc[0] += rp * rp + rm[k] * rm[k];
            acc[1] += rh * rh;
            acc[2] = fmin(acc[2], d);
            acc[3] = fmax(acc[3], d);
        }
    }
    const int op[4] = {0, 0, 1, 2};
    block_reduce_store<4>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// ---------------------------------------------------------------------------------
// Schur-reduced Newton operator  out = A x = x/dt + M (kappa/2 M x + D x),  M = -L   (13-point), the bare
// operator of vch2d_schur_apply (kernel-level tests); the solver's own application is fused into k_schur_p.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_schur(Geom G, Phys P, const TrajState *__restrict__ st,
                                               long slot_stride, const double *__restrict__ x,
                                               const double *__restrict__ D_s, double dt, double *__restrict__ out) {
    TILE_COORDS;
    const int slot = st ? st[b].slot : 0;
    __shared__ double sx[(TY + 4) * (TX + 4)];
    __shared__ double stt[(TY + 2) * (TX + 2)];
    constexpr int W2 = TX + 4, W1 = TX + 2;
    const long pb = b * G.plane;
    load_tile<2>(sx, x + pb, G, c0, r0);
    __syncthreads();
    const double *Dp = D_s + slot * slot_stride + pb;
    for (int e = threadIdx.x; e < (TY + 2) * W1; e += NTH) {
        int ly = e / W1, lxx = e - ly * W1;
        int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
        int p2 = (ly + 1) * W2 + lxx + 1;
        stt[e] = -0.5 * P.kappa * lap_at<W2>(sx, p2, G.ax, G.ay) + Dp[(long)gr * G.pitch + gc] * sx[p2];
    }
    __syncthreads();
    const double idt = 1.0 / dt;
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
            out[pb + (long)r * G.pitch + c] = sx[p2] * idt - lap_at<W1>(stt, p1, G.ax, G.ay);
        }
    }
}

// ---------------------------------------------------------------------------------
// Starting guess for the first Newton solve of a time step.  Along a march the first Newton increments d_n vary smoothly
// from step to step: measured as the solver sees it, ||A (d_n - guess)|| / ||A d_n|| at 512^2, the previous increment
// alone leaves 1e-2, linear extrapolation 1e-4, quadratic 3e-6 and cubic 1e-7 (scripts/r2_extrap.py; the first dozen
// steps of the spinodal transient are the exception, there the order is kept low by the host, forward_core).  So the
// solve starts from x0 = sum_j c_j d_{n-j} (up to GUESS_ORD previous increments, coefficients = polynomial extrapolation of
// the increment rate over the step midpoints): this kernel, between k_residual<0> and k_fin_residual<0>, stores x0 and
// deflates the right-hand side,
//       rhs <- rhs - A x0        (A = the 13-point Schur operator of k_schur, D of the current iterate),
// and replaces the partial of sum rhs^2 (slot 1; the old one moves to slot 4) so that the forcing rule of the solve
// (newton_lin_tol) sees the deflated norm: the sweeps then reach the SAME absolute Schur residual target with fewer
// sweeps.  The solve itself is unchanged -- its first sweep takes x = x0 instead of 0 (TrajState::x_primed).
// Any x0 is valid; non-finite entries of a stale d plane are read as 0.
// ---------------------------------------------------------------------------------
constexpr int GUESS_RING = 8;     // increments kept (a power of two)
constexpr int GUESS_ORD = 8;      // at most this many planes enter one guess (forward: <= 6 increments; adjoint: every second level)
#ifndef VCH_GUESS_BMAX
#define VCH_GUESS_BMAX 32
#endif
constexpr int GUESS_BMAX = VCH_GUESS_BMAX;    // trajectories per context with coefficients of their own (beyond: one common set, row 0)
struct GuessArgs {
    const double *d[GUESS_ORD];   // first Newton increments of steps n-1 .. n-GUESS_ORD, [B][plane]
    // their coefficients (0 = plane not used), PER TRAJECTORY: the order of the extrapolation is chosen for every
    // trajectory from its own history (forward_core), so a trajectory's arithmetic does not depend on its batch mates
    double c[GUESS_BMAX][GUESS_ORD];
    int per_traj;                 // 0: row 0 holds for every trajectory
    __host__ __device__ const double *row(int b) const { return c[per_traj ? b : 0]; }
};
// bit b of the mask a fin kernel gets: trajectory b's right-hand side was deflated by a starting guess in this launch sequence
__host__ __device__ inline unsigned guess_bit(unsigned mask, int b) { return (mask >> (b & 31)) & 1u; }
// which = 0: the step's first solve (right-hand side of the initial residual, iterate slot S.slot);  which = 1: its second
// solve -- the kernel sits between a trial's k_residual<1> and k_fin_residual<1>, works on the slot the trial wrote
// (1 - S.slot) and only for trajectories whose first solve is done (iters == 1); a trial that is then rejected
// simply discards it (the next trial evaluates the right-hand side afresh and this kernel runs again).
__global__ __launch_bounds__(NTH) void k_guess(Geom G, Phys P, const TrajState *__restrict__ st, long slot_stride,
                                               GuessArgs ga, const double *__restrict__ D_s, double dt,
                                               double *__restrict__ rhs_s, double *__restrict__ x0, double *__restrict__ part,
                                               int which) {
    TILE_COORDS;
    const TrajState S = st[b];
    if (!S.newton_active || !S.need_trial) return;
    if (which == 1 && S.iters != 1) return;
    const double *gcf = ga.row(b);
    if (gcf[0] == 0.0) return;             // no guess for this trajectory in this step
    const int slot = which == 1 ? 1 - S.slot : S.slot;
    __shared__ double sx[(TY + 4) * (TX + 4)];
    __shared__ double stt[(TY + 2) * (TX + 2)];
    __shared__ double sred[4];
    constexpr int W2 = TX + 4, W1 = TX + 2;
    const long pb = b * G.plane;
    for (int e = threadIdx.x; e < W2 * (TY + 4); e += NTH) {
        int ly = e / W2, lxx = e - ly * W2;
        int gr = refl(r0 - 2 + ly, G.ns), gc = refl(c0 - 2 + lxx, G.nf);
        long o = pb + (long)gr * G.pitch + gc;
        double v = gcf[0] * ga.d[0][o];
#pragma unroll
        for (int j = 1; j < GUESS_ORD; ++j)
            if (gcf[j] != 0.0) v += gcf[j] * ga.d[j][o];
        sx[e] = isfinite(v) ? v : 0.0;
    }
    __syncthreads();
    const double *Dp = D_s + slot * slot_stride + pb;
    for (int e = threadIdx.x; e < (TY + 2) * W1; e += NTH) {
        int ly = e / W1, lxx = e - ly * W1;
        int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
        int p2 = (ly + 1) * W2 + lxx + 1;
        stt[e] = -0.5 * P.kappa * lap_at<W2>(sx, p2, G.ax, G.ay) + Dp[(long)gr * G.pitch + gc] * sx[p2];
    }
    __syncthreads();
    const double idt = 1.0 / dt;
    double acc = 0.0;
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
            long o = pb + (long)r * G.pitch + c, os = slot * slot_stride + o;
            const double rh = rhs_s[os] - (sx[p2] * idt - lap_at<W1>(stt, p1, G.ax, G.ay));
            rhs_s[os] = rh;
            x0[o] = sx[p2];
            acc += rh * rh;
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double *pp = part + ((long)b * nblk + blk) * NPART;
        pp[4] = pp[1];
        pp[1] = (sred[0] + sred[1]) + (sred[2] + sred[3]);
    }
}

// ---------------------------------------------------------------------------------
// After the linear solve: dphi = x; dmu = 2 (K dphi + R_phi), K = kappa/2 M + D (back
// substitution of the Schur reduction); per workgroup min over nodes of the step-ceiling
// ratio ((+-(1-delta) - phi)/dphi, F2:381-387).
// ---------------------------------------------------------------------------------
// x_out = the finished dphi.  The kernel reads x (+ alpha p for the fused form of vch_fft.h, k_dmu_ceiling_fin, which also
// resolves the last reduction point of the solve) on the haloed tile and never writes what a neighbour reads.
__global__ __launch_bounds__(NTH) void k_dmu_ceiling(Geom G, Phys P, const TrajState *__restrict__ st,
                                                     long slot_stride, const double *__restrict__ x,
                                                     const double *__restrict__ phi_s,
                                                     const double *__restrict__ D_s,
                                                     const double *__restrict__ Rphi_s, double *__restrict__ dmu,
                                                     double *__restrict__ x_out, double *__restrict__ part) {
    TILE_COORDS;
    const TrajState S = st[b];
    if (!S.newton_active || S.need_trial) return;
    __shared__ double sx[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    constexpr int W = TX + 2;
    const long pb = b * G.plane;
    load_tile<1>(sx, x + pb, G, c0, r0);
    __syncthreads();
    double acc[1] = {1e300};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p = (ly + 1) * W + lx + 1;
            long o = pb + (long)r * G.pitch + c, os = S.slot * slot_stride + o;
            double d = sx[p];
            x_out[o] = d;
            dmu[o] = 2.0 * ((-0.5 * P.kappa * lap_at<W>(sx, p, G.ax, G.ay) + D_s[os] * d) + Rphi_s[os]);
            double ph = phi_s[os];
            if (d > 0.0) acc[0] = fmin(acc[0], (1.0 - DELTA_SEP - ph) / d);
            else if (d < 0.0) acc[0] = fmin(acc[0], (-1.0 + DELTA_SEP - ph) / d);
        }
    }
    const int op[1] = {1};
    block_reduce_store<1>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// (out_phi, out_mu) = J [dphi; dmu]  (F2:241-253), for the kernel-level parity test.
__global__ __launch_bounds__(NTH) void k_jac_apply(Geom G, Phys P, const double *__restrict__ phi,
                                                   const double *__restrict__ dphi, const double *__restrict__ dmu,
                                                   double dt, double *__restrict__ op_, double *__restrict__ om_) {
    TILE_COORDS;
    __shared__ double sa[(TY + 2) * (TX + 2)];
    __shared__ double sb[(TY + 2) * (TX + 2)];
    constexpr int W = TX + 2;
    const long pb = b * G.plane;
    load_tile<1>(sa, dphi + pb, G, c0, r0);
    load_tile<1>(sb, dmu + pb, G, c0, r0);
    __syncthreads();
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p = (ly + 1) * W + lx + 1;
            long o = pb + (long)r * G.pitch + c;
            double d = jac_diag(phi[o], P.tau / dt, P.c1);
            op_[o] = -0.5 * P.kappa * lap_at<W>(sa, p, G.ax, G.ay) + d * sa[p] - 0.5 * sb[p];
            om_[o] = sa[p] / dt - 0.5 * lap_at<W>(sb, p, G.ax, G.ay);
        }
    }
}

// Stand-alone (R_phi, R_mu) in the reference's own form (F2:194-221), for the parity test.
__global__ __launch_bounds__(NTH) void k_residual_plain(Geom G, Phys P, const double *__restrict__ pn,
                                                        const double *__restrict__ po, const double *__restrict__ mn,
                                                        const double *__restrict__ mo, const double *__restrict__ wn,
                                                        const double *__restrict__ wo, double dt,
                                                        double *__restrict__ Rp, double *__restrict__ Rm,
                                                        double *__restrict__ part) {
    TILE_COORDS;
    __shared__ double s[4][(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    constexpr int W = TX + 2;
    const long pb = b * G.plane;
    load_tile<1, false>(s[0], pn + pb, G, c0, r0);
    load_tile<1, false>(s[1], po + pb, G, c0, r0);
    load_tile<1, false>(s[2], mn + pb, G, c0, r0);
    load_tile<1, false>(s[3], mo + pb, G, c0, r0);
    __syncthreads();
    double acc[1] = {0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p = (ly + 1) * W + lx + 1;
            long o = pb + (long)r * G.pitch + c;
            double rp = (P.tau * (s[0][p] - s[1][p]) / dt) -
                        0.5 * P.kappa * (lap_at<W>(s[0], p, G.ax, G.ay) + lap_at<W>(s[1], p, G.ax, G.ay)) +
                        (P.c1 * reglog(s[0][p]) + (-2.0 * P.c2 * s[1][p])) - 0.5 * (s[2][p] + s[3][p]) -
                        0.5 * (wn[o] + wo[o]);
            double rm = (s[0][p] - s[1][p]) / dt - 0.5 * (lap_at<W>(s[2], p, G.ax, G.ay) + lap_at<W>(s[3], p, G.ax, G.ay));
            Rp[o] = rp;
            Rm[o] = rm;
            acc[0] += rp * rp + rm * rm;
        }
    }
    const int op[1] = {0};
    block_reduce_store<1>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// ---------------------------------------------------------------------------------
// End of a time step (F2:562-577): clip to +-(1-delta), weighted mass and interior weight
// (pass 1), then subtract mass_error/W_int on the interior nodes (pass 2) and store the
// level into the history.  wts = hx*hy*outer(trapz_x, trapz_y) (F2:528-531), one shared plane.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_mass(Geom G, const TrajState *__restrict__ st, long slot_stride,
                                              const double *__restrict__ phi_s, const double *__restrict__ wts,
                                              int do_clip, double *__restrict__ part, int ended_only) {
    TILE_COORDS;
    __shared__ double sred[NPART * 4];
    if (st[b].frozen) return;
    // ended_only: the launch sits in front of the host's look at the step (newton_level); a trajectory whose Newton loop is
    // still running has no final iterate yet and is summed by a second launch behind the continuation loop
    if (ended_only && st[b].newton_active) return;
    const int slot = st[b].slot;
    const double hi = 1.0 - DELTA_SEP;
    double acc[2] = {0.0, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            long o = (long)r * G.pitch + c;
            double ph = phi_s[slot * slot_stride + b * G.plane + o];
            if (do_clip) ph = fmin(fmax(ph, -hi), hi);
            double w = wts[o];
            acc[0] += w * ph;
            if (fabs(ph) < hi - 5e-3) acc[1] += w;
        }
    }
    const int op[2] = {0, 0};
    block_reduce_store<2>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// k_post sums the per-workgroup partials of k_mass itself (every workgroup, the same numbers in the same order: the
// first wavefront strides over them like fin_reduce does), so no `fin` launch sits between the two passes.
// The same two pieces serve k_eval<0>, which applies the end of step n to the values it loads at the start of step n + 1
// (PostArgs): post_sums (first wavefront, then a barrier) and PostFix::apply (a pure function of the node's value).
__device__ __forceinline__ void post_sums(const double *__restrict__ part, int nblk, int b, double *sm2) {
    if (threadIdx.x < 64) {
        double a0 = 0.0, a1 = 0.0;
        for (int t = threadIdx.x; t < nblk; t += 64) {
            a0 += part[((long)b * nblk + t) * NPART];
            a1 += part[((long)b * nblk + t) * NPART + 1];
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        if (threadIdx.x == 0) {
            sm2[0] = a0;
            sm2[1] = a1;
        }
    }
}
struct PostFix {
    double shift, hi;
    bool fix, interior_ok;
    __device__ __forceinline__ PostFix(const double *sm2, double mass0, double LxLy) {
        const double mass_err = sm2[0] - mass0, Wint = sm2[1];
        hi = 1.0 - DELTA_SEP;
        fix = fabs(mass_err) > 1e-16;
        interior_ok = Wint > 0.0;
        shift = fix ? (interior_ok ? mass_err / Wint : mass_err / LxLy) : 0.0;
    }
    __device__ __forceinline__ double apply(double v) const {
        double ph = fmin(fmax(v, -hi), hi);
        if (fix) {
            if (interior_ok) {
                if (fabs(ph) < hi - 5e-3) ph -= shift;
            } else {
                ph = fmin(fmax(ph - shift, -hi), hi);
            }
        }
        return ph;
    }
    // the step's cell of the shift record (vch2d_second_order and vch2d_hessvec linearise the fix about it): what was
    // subtracted, and the weight it was divided by -- W_int (sm2[1], the sums the fix was built from) where it went to the
    // interior nodes only, 0.0 for the all-node form, 1.0 where no fix ran; written by one lane of one workgroup per trajectory
    __device__ __forceinline__ void record(double *rec, const double *sm2) const {
        rec[0] = shift;
        rec[1] = fix ? (interior_ok ? sm2[1] : 0.0) : 1.0;
    }
};
constexpr int SHIFT_REC = 2;
struct PostArgs {
    const double *part;        // k_mass partials of the step that has just ended (own buffer), or NULL: nothing pending
    double *hist;              // history level of that step, or NULL
    long hist_stride;
    double *rec;               // that step's cell of the shift record ([B] cells rec_stride apart), or NULL
    long rec_stride;
};

__global__ __launch_bounds__(NTH) void k_post(Geom G, Phys P, const TrajState *__restrict__ st, long slot_stride,
                                              double *__restrict__ phi_s, double *__restrict__ hist_level,
                                              long hist_stride, const double *__restrict__ part, double *__restrict__ rec,
                                              long rec_stride) {
    TILE_COORDS;
    const TrajState S = st[b];
    if (S.frozen) return;
    __shared__ double sm[2];
    post_sums(part, nblk, b, sm);
    __syncthreads();
    const PostFix pf(sm, S.mass0, P.LxLy);
    if (rec && blk == 0 && threadIdx.x == 0) pf.record(rec + b * rec_stride, sm);
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            long o = (long)r * G.pitch + c;
            long os = S.slot * slot_stride + b * G.plane + o;
            const double ph = pf.apply(phi_s[os]);
            phi_s[os] = ph;
            if (hist_level) hist_level[b * hist_stride + o] = ph;
        }
    }
}

// Per-trajectory optimisation parameters on the device: OPT_STRIDE doubles per trajectory, written by the host with a plain
// copy (vch2d_pgd_init_v; the stateless seams fill a table of their own with one row repeated).  A kernel indexes it by
// blockIdx.z, which is uniform over the workgroup, so the values arrive as scalar loads and sit in SGPRs.
constexpr int OPT_STRIDE = 8;
enum { OPT_B1 = 0, OPT_B2 = 1, OPT_B3 = 2, OPT_KS = 3, OPT_UMIN = 4, OPT_UMAX = 5 };

// ---------------------------------------------------------------------------------
// Adjoint sweep (B2:212-242).  With q = -L p carried from the previous step,
//   rhs = B(phi_{n+1}) p_{n+1} + src = p + (tau - dt/2 D+) q + dt/2 L q + src,
//   D+ = f''(phi_{n+1}),  src = dt/2 b1 ((phi_n - phiQ_n) + (phi_{n+1} - phiQ_{n+1})),
// and D_n = f''(phi_n) is stored for the A(phi_n) applications; per workgroup min/max D_n.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_adj_rhs(Geom G, Phys P, const double *__restrict__ p,
                                                 const double *__restrict__ q, const double *__restrict__ phin,
                                                 const double *__restrict__ phin1, const double *__restrict__ qn,
                                                 const double *__restrict__ qn1, long hist_stride, double dt,
                                                 const double *__restrict__ opt_tab, double *__restrict__ rhs,
                                                 double *__restrict__ Dn, double *__restrict__ part) {
    TILE_COORDS;
    const double b1 = opt_tab[b * OPT_STRIDE + OPT_B1];
    __shared__ double sq[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    constexpr int W = TX + 2;
    const long pb = b * G.plane;
    load_tile<1, false>(sq, q + pb, G, c0, r0);
    __syncthreads();
    double acc[3] = {1e300, -1e300, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int pp = (ly + 1) * W + lx + 1;
            long o = (long)r * G.pitch + c, oh = b * hist_stride + o;
            double f0 = phin[oh], f1 = phin1[oh];
            double t0 = qn ? qn[oh] : 0.0, t1 = qn1 ? qn1[oh] : 0.0;
            double src = 0.5 * dt * b1 * ((f0 - t0) + (f1 - t1));
            double dplus = fpp_log(f1, P.c1, P.c2), dn = fpp_log(f0, P.c1, P.c2);
            double v = p[pb + o] + (P.tau - 0.5 * dt * dplus) * sq[pp] + 0.5 * dt * lap_at<W>(sq, pp, G.ax, G.ay) + src;
            rhs[pb + o] = v;
            Dn[pb + o] = dn;
            acc[0] = fmin(acc[0], dn);
            acc[1] = fmax(acc[1], dn);
            acc[2] += v * v;
        }
    }
    const int op[3] = {1, 2, 0};
    block_reduce_store<3>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// A(phi_n) x = x + (tau + dt/2 D) M x + dt/2 M M x  (= I - tau L + dt/2 L^2 - dt/2 D L, B2:198)
//   MODE 0: out = A x; MODE 1: out = rhs - A x with sum(out^2); MODE 2: out = B x (B2:203)
template <int MODE>
__global__ __launch_bounds__(NTH) void k_adj_op(Geom G, Phys P, const TrajState *__restrict__ st,
                                                const double *__restrict__ x, const double *__restrict__ Dn,
                                                const double *__restrict__ rhs, double dt,
                                                double *__restrict__ out, double *__restrict__ part) {
    TILE_COORDS;
    if (MODE == 1 && !st[b].lin_active) return;
    const double dbar = MODE == 1 ? st[b].dbar : 0.0;
    __shared__ double sx[(TY + 4) * (TX + 4)];
    __shared__ double stt[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    constexpr int W2 = TX + 4, W1 = TX + 2;
    const long pb = b * G.plane;
    load_tile<2, false>(sx, x + pb, G, c0, r0);
    __syncthreads();
    for (int e = threadIdx.x; e < (TY + 2) * W1; e += NTH) {
        int ly = e / W1, lxx = e - ly * W1;
        stt[e] = -lap_at<W2>(sx, (ly + 1) * W2 + lxx + 1, G.ax, G.ay);      // t = M x
    }
    __syncthreads();
    double acc[2] = {0.0, 0.0};
    const double sgn = MODE == 2 ? -1.0 : 1.0;
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
            long o = pb + (long)r * G.pitch + c;
            double t = stt[p1], mt = -lap_at<W1>(stt, p1, G.ax, G.ay);
            double ax_ = sx[p2] + (P.tau + sgn * 0.5 * dt * Dn[o]) * t + sgn * 0.5 * dt * mt;
            if (MODE == 1) {
                double rr = rhs[o] - ax_;
                out[o] = rr;
                acc[0] += wdev(r, c, G) / (Dn[o] - dbar) * (rr * rr);
                acc[1] += rr * rr;
            } else {
                out[o] = ax_;
            }
        }
    }
    if (MODE == 1) {
        const int op[2] = {0, 0};
        block_reduce_store<2>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
    }
}

// p_n = x (already in place); q_n = -L p_n; r_n = gb r_{n+1} + gs (q_n + q_{n+1}) (B2:233-242).
// BATCH (the default; VCH_LOADS_BATCH=0 launches k_adj_finish_plain): the tile and r, q_old of the thread's TY / 4 own nodes are
// requested together, in front of the barrier; the nodes are then applied in the same order with the same expressions.
template <bool BATCH>
__device__ __forceinline__ void adj_finish_body(const Geom &G, const double *__restrict__ p,
                                                const double *__restrict__ q_old, double *__restrict__ q_new,
                                                double *__restrict__ r_cur, double gb, double gs,
                                                double *__restrict__ r_hist, double *__restrict__ p_hist,
                                                double *__restrict__ q_hist, long hist_stride) {
    TILE_COORDS;
    constexpr int K = TY / 4;
    __shared__ double s[(TY + 2) * (TX + 2)];
    constexpr int W = TX + 2;
    const long pb = b * G.plane;
    double vr[K], vq[K];
    if (BATCH) {
        TileRegs<1> tp;
        tile_fetch<1>(tp, p + pb, G, c0, r0);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            int r = r0 + ly0 + 4 * k, c = c0 + lx;
            vr[k] = vq[k] = 0.0;
            if (q_old && r < G.ns && c < G.nf) {
                long o = (long)r * G.pitch + c;
                vr[k] = r_cur[pb + o];
                vq[k] = q_old[pb + o];
            }
        }
        tile_put<1>(s, tp);
    } else {
        load_tile<1, false>(s, p + pb, G, c0, r0);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int pp = (ly + 1) * W + lx + 1;
            long o = (long)r * G.pitch + c, oh = b * hist_stride + o;
            double qn = -lap_at<W>(s, pp, G.ax, G.ay);
            double rn = q_old ? gb * (BATCH ? vr[k] : r_cur[pb + o]) + gs * (qn + (BATCH ? vq[k] : q_old[pb + o])) : 0.0;
            q_new[pb + o] = qn;
            r_cur[pb + o] = rn;
            if (r_hist) r_hist[oh] = rn;
            if (p_hist) p_hist[oh] = s[pp];
            if (q_hist) q_hist[oh] = qn;
        }
    }
}
#define ADJ_FINISH_PARAMS Geom G, const double *__restrict__ p, const double *__restrict__ q_old, double *__restrict__ q_new, \
                          double *__restrict__ r_cur, double gb, double gs, double *__restrict__ r_hist,                    \
                          double *__restrict__ p_hist, double *__restrict__ q_hist, long hist_stride
#define ADJ_FINISH_ARGS G, p, q_old, q_new, r_cur, gb, gs, r_hist, p_hist, q_hist, hist_stride
__global__ __launch_bounds__(NTH) void k_adj_finish(ADJ_FINISH_PARAMS) { adj_finish_body<true>(ADJ_FINISH_ARGS); }
__global__ __launch_bounds__(NTH) void k_adj_finish_plain(ADJ_FINISH_PARAMS) { adj_finish_body<false>(ADJ_FINISH_ARGS); }

// out = a_b*(x - y), a_b = a_tab[b * a_stride] (terminal right-hand side b2 (phi_M - phi_T), B2:183); y may be NULL
__global__ __launch_bounds__(NTH) void k_scaled_diff(Geom G, const double *__restrict__ x, long xs,
                                                     const double *__restrict__ y, long ys,
                                                     const double *__restrict__ a_tab, int a_stride,
                                                     double *__restrict__ out, double *__restrict__ part) {
    TILE_COORDS;
    const double a = a_tab[b * a_stride];
    __shared__ double sred[NPART * 4];
    double acc[1] = {0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            long o = (long)r * G.pitch + c;
            double v = a * (x[b * xs + o] - (y ? y[b * ys + o] : 0.0));
            out[b * G.plane + o] = v;
            acc[0] += v * v;
        }
    }
    const int op[1] = {0};
    block_reduce_store<1>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

__global__ __launch_bounds__(NTH) void k_copy_plane(Geom G, const double *__restrict__ src, long ss,
                                                    double *__restrict__ dst, long ds) {
    TILE_COORDS;
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            long o = (long)r * G.pitch + c;
            dst[b * ds + o] = src[b * ss + o];
        }
    }
}

// ---------------------------------------------------------------------------------
// Cost integrands (C2:80-106): per (trajectory, level, tile) partial sums of
//   W (phi - phiQ)^2, W u^2, W |u| and, on the last level, W (phi - phiT)^2,
// W = product trapezoid weights built from the caller's x, y (np.trapz arithmetic).
// grid = (tiles, levels, B)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_cost(Geom G, int tiles_f, const double *__restrict__ phi,
                                              const double *__restrict__ u, const double *__restrict__ pq,
                                              const double *__restrict__ pt, const double *__restrict__ phi0,
                                              const double *__restrict__ tfrac, long hist_stride, int last_level,
                                              const double *__restrict__ W, double *__restrict__ part) {
    const int b = blockIdx.z, lvl = blockIdx.y;
    const int tf = blockIdx.x % tiles_f, ts = blockIdx.x / tiles_f;
    const int c0 = tf * TX, r0 = ts * TY;
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
    __shared__ double sred[NPART * 4];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const long lb = b * hist_stride + (long)lvl * G.plane;
    const double tf_ = tfrac ? tfrac[lvl] : 0.0;
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            long o = (long)r * G.pitch + c;
            double w = W[o], ph = phi[lb + o];
            double uu = u ? u[lb + o] : 0.0;
            double tq;
            if (pq) tq = pq[lb + o];
            else if (tfrac) tq = (1.0 - tf_) * phi0[b * G.plane + o] + tf_ * pt[b * G.plane + o];
            else tq = 0.0;
            double e = ph - tq;
            acc[0] += w * (e * e);
            acc[2] += w * (uu * uu);
            acc[3] += w * fabs(uu);
            if (lvl == last_level) {
                double e2 = ph - (pt ? pt[b * G.plane + o] : 0.0);
                acc[1] += w * (e2 * e2);
            }
        }
    }
    const int op[4] = {0, 0, 0, 0};
    block_reduce_store<4>(acc, op, sred, part + (((long)b * gridDim.y + lvl) * gridDim.x + blockIdx.x) * 4);
}

// ---------------------------------------------------------------------------------
// Free energy of every level of a history (F2:256-319), the array taken as the reference takes it:
// shape (A0, A1) row-major, forward differences along both axes, trapezoid weights outer(A0, A1).
// The engine stores that row-major block as ns rows of nf (flat index f -> (f / nf, f % nf), pitched).
// Per workgroup (1024 flat nodes) partials {sum d0^2, sum d1^2, sum W psi, sum W w phi}.
// grid = (ceil(A0*A1/1024), levels, B)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_energy(Geom G, int A0, int A1, double c1, double c2, double eps,
                                                const double *__restrict__ phi, const double *__restrict__ w,
                                                long hist_stride, double *__restrict__ part) {
    __shared__ double sred[NPART * 4];
    const int b = blockIdx.z, lvl = blockIdx.y;
    const long base = b * hist_stride + (long)lvl * G.plane;
    const double *ph = phi + base;
    const double *wp = w ? w + base : nullptr;
    auto at = [&](const double *p, int f) { return p[(long)(f / G.nf) * G.pitch + (f % G.nf)]; };
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int total = A0 * A1;
    for (int k = 0; k < 4; ++k) {
        const int f = blockIdx.x * 1024 + k * NTH + threadIdx.x;
        if (f < total) {
            const int i = f / A1, j = f - i * A1;
            const double a = at(ph, f);
            if (i + 1 < A0) { const double d = at(ph, f + A1) - a; acc[0] += d * d; }
            if (j + 1 < A1) { const double d = at(ph, f + 1) - a; acc[1] += d * d; }
            const double wt = ((i == 0 || i == A0 - 1) ? 0.5 : 1.0) * ((j == 0 || j == A1 - 1) ? 0.5 : 1.0);
            const double p = fmin(fmax(a, -1.0 + eps), 1.0 - eps);
            const double psi = c1 * ((1.0 + p) * log(1.0 + p) + (1.0 - p) * log(1.0 - p)) - c2 * (p * p);
            acc[2] += wt * psi;
            if (wp) acc[3] += wt * at(wp, f) * a;
        }
    }
    const int op[4] = {0, 0, 0, 0};
    block_reduce_store<4>(acc, op, sred, part + (((long)b * gridDim.y + lvl) * gridDim.x + blockIdx.x) * 4);
}

// sums the tile partials of k_cost: out[b][lvl][4]
__global__ void k_cost_fin(int ntiles, const double *__restrict__ part, double *__restrict__ out) {
    const long idx = (long)blockIdx.x;      // b * levels + lvl
    double a[4] = {0, 0, 0, 0};
    for (int t = threadIdx.x; t < ntiles; t += 64)
        for (int k = 0; k < 4; ++k) a[k] += part[(idx * ntiles + t) * 4 + k];
    for (int k = 0; k < 4; ++k) {
        double v = wave_sum(a[k]);
        if (threadIdx.x == 0) out[idx * 4 + k] = v;
    }
}

// ---------------------------------------------------------------------------------
// gradient + proximal step (C2:150, C2:191-198): g = r + b3 u; v = u - alpha g;
// s = sign(v) max(|v| - alpha kappa_s, 0); u+ = clip(s, u_min, u_max).  Also per-workgroup
// sum (u+ - u)^2 and sum u^2 for the relative-change stop rule (G2:375).
// grid = (tiles, levels, B)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_grad_prox(Geom G, int tiles_f, const double *__restrict__ u,
                                                   const double *__restrict__ r, long hist_stride,
                                                   const double *__restrict__ alpha,
                                                   const double *__restrict__ opt_tab, double *__restrict__ uout,
                                                   double *__restrict__ part) {
    const int b = blockIdx.z, lvl = blockIdx.y;
    const double *ot = opt_tab + b * OPT_STRIDE;
    const double b3 = ot[OPT_B3], ks = ot[OPT_KS], umin = ot[OPT_UMIN], umax = ot[OPT_UMAX];
    const int tf = blockIdx.x % tiles_f, ts = blockIdx.x / tiles_f;
    const int c0 = tf * TX, r0 = ts * TY;
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
    __shared__ double sred[NPART * 4];
    const double al = alpha[b];
    const long lb = b * hist_stride + (long)lvl * G.plane;
    double acc[2] = {0.0, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int rr = r0 + ly0 + 4 * k, c = c0 + lx;
        if (rr < G.ns && c < G.nf) {
            long o = lb + (long)rr * G.pitch + c;
            double uu = u[o];
            double v = uu - al * (r[o] + b3 * uu);
            double sgn = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
            double s = sgn * fmax(fabs(v) - al * ks, 0.0);
            double un = fmin(fmax(s, umin), umax);
            uout[o] = un;
            acc[0] += (un - uu) * (un - uu);
            acc[1] += uu * uu;
        }
    }
    if (part) {
        const int op[2] = {0, 0};
        block_reduce_store<2>(acc, op, sred, part + (((long)b * gridDim.y + lvl) * gridDim.x + blockIdx.x) * 4);
    }
}

// ---------------------------------------------------------------------------------
// KKT sparsity statistic u* = 0 <=> |r*| <= kappa_s (sparsity_statistics of second_order_conditions_2d): per trajectory
// the number of nodes with |u| < tol, with |r| <= kappa_s (trajectory b's own), and where the two predicates agree.
// Pad columns of the pitched rows and rows beyond ns take no part: their lanes vote false in all three ballots.  Every
// wavefront counts by ballot + popcount, the workgroup's four wavefronts meet in LDS, and three lanes add the workgroup's
// three integers to part[b][level][3] with vector integer atomics (integer sums do not depend on the order; one address
// per trajectory and statistic instead of one per level made the atomics the kernel's cost: 20.6 ms against 6.1 ms
// at 512^2 x 1000 x 8).  The caller zeroes part; k_kkt_fin adds the levels up.
// grid = (tiles, levels, B)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_kkt_count(Geom G, int tiles_f, const double *__restrict__ u,
                                                   const double *__restrict__ r, long hist_stride,
                                                   const double *__restrict__ opt_tab, double tol,
                                                   unsigned long long *__restrict__ part) {
    const int b = blockIdx.z, lvl = blockIdx.y;
    const int tf = blockIdx.x % tiles_f, ts = blockIdx.x / tiles_f;
    const int c0 = tf * TX, r0 = ts * TY;
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
    const double ks = opt_tab[b * OPT_STRIDE + OPT_KS];
    const long lb = b * hist_stride + (long)lvl * G.plane;
    unsigned nz = 0, nsm = 0, nm = 0;
    for (int k = 0; k < TY / 4; ++k) {
        const int rr = r0 + ly0 + 4 * k, c = c0 + lx;
        const bool in = rr < G.ns && c < G.nf;
        bool zero = false, small = false;
        if (in) {
            const long o = lb + (long)rr * G.pitch + c;
            zero = fabs(u[o]) < tol;
            small = fabs(r[o]) <= ks;
        }
        nz += __popcll(__ballot(zero));
        nsm += __popcll(__ballot(small));
        nm += __popcll(__ballot(in && zero == small));
    }
    __shared__ unsigned sc[NTH / 64][3];
    if (lx == 0) {
        sc[ly0][0] = nz;
        sc[ly0][1] = nsm;
        sc[ly0][2] = nm;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned v = 0;
        for (int w = 0; w < NTH / 64; ++w) v += sc[w][threadIdx.x];
        if (v) atomicAdd(part + ((long)b * gridDim.y + lvl) * 3 + threadIdx.x, (unsigned long long)v);
    }
}

// counts[b][3] = sum over the levels of part[b][level][3]; one workgroup of 64 threads per trajectory
__global__ void k_kkt_fin(int levels, const unsigned long long *__restrict__ part, unsigned long long *__restrict__ counts) {
    const int b = blockIdx.x;
    __shared__ unsigned long long tot[3];
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long a[3] = {0, 0, 0};
    for (int l = threadIdx.x; l < levels; l += 64)
        for (int k = 0; k < 3; ++k) a[k] += part[((long)b * levels + l) * 3 + k];
    for (int k = 0; k < 3; ++k)
        if (a[k]) atomicAdd(&tot[k], a[k]);
    __syncthreads();
    if (threadIdx.x < 3) counts[3 * b + threadIdx.x] = tot[threadIdx.x];
}

// ---------------------------------------------------------------------------------
// Directional sparsity: the prox of kappa_s * sum over groups of ||u_g|| under the box, a group being a level
// of the control (VCH_SPARSITY_TIME, ||z||^2 = sum_ij W_ij z_ij^2 with the plane W of the cost) or the pencil of one node
// through the levels (VCH_SPARSITY_SPACE, ||z||^2 = sum_k wt_k z_k^2).  gp_v, gp_cone, gp_out and gp_step (vch_gp.h) are the
// 1D kernels' own.  No floating-point atomics; every sum is taken in one order fixed by the geometry alone, so a member of a
// mixed batch has the bits of its single run; every loop has a cap; no workgroup waits on another.  `mode` [B] (or NULL:
// every trajectory): a workgroup of a trajectory in another mode returns at once.  Pad columns of the pitched rows and rows
// beyond ns take no part.
// ---------------------------------------------------------------------------------
constexpr int GT_W = 16, GT_T = 64 * GT_W;       // the plane solver and the pencil kernels: 16 wavefronts

// TIME, stage 1.  Per (tile, level, trajectory) the partials {sum W cone(v)^2, sum W v^2, max(v, 0), min(v, 0)} at
// part[b][level][tile][4]; s0 v is monotone in v, so the extremes decide whether the box is inactive at s0.
// grid = (tiles, levels, B)
__global__ __launch_bounds__(NTH) void k_gp_time_part(Geom G, int tiles_f, const double *__restrict__ u,
                                                      const double *__restrict__ r, long hist_stride,
                                                      const double *__restrict__ alpha, const double *__restrict__ opt_tab,
                                                      const int *__restrict__ mode, const double *__restrict__ W,
                                                      double *__restrict__ part) {
    const int b = blockIdx.z, lvl = blockIdx.y;
    if (mode && mode[b] != GP_TIME) return;
    const double *ot = opt_tab + b * OPT_STRIDE;
    const double b3 = ot[OPT_B3], umin = ot[OPT_UMIN], umax = ot[OPT_UMAX];
    const int tf = blockIdx.x % tiles_f, ts = blockIdx.x / tiles_f;
    const int c0 = tf * TX, r0 = ts * TY;
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
    __shared__ double sred[NPART * 4];
    const double al = alpha[b];
    const long lb = b * hist_stride + (long)lvl * G.plane;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        const int rr = r0 + ly0 + 4 * k, c = c0 + lx;
        if (rr < G.ns && c < G.nf) {
            const long o = (long)rr * G.pitch + c;
            const double v = gp_v(u[lb + o], r[lb + o], al, b3), w = W[o];
            const double cv = gp_cone(v, umin, umax);
            acc[0] += w * (cv * cv);
            acc[1] += w * (v * v);
            acc[2] = fmax(acc[2], v);
            acc[3] = fmin(acc[3], v);
        }
    }
    const int op[4] = {0, 0, 2, 1};
    block_reduce_store<4>(acc, op, sred, part + (((long)b * gridDim.y + lvl) * gridDim.x + blockIdx.x) * 4);
}

// TIME, stage 2.  One workgroup per (level, trajectory): thread 0 adds the tile partials in index order and decides: zero
// (s = 0), the closed form s0 = 1 - lam / ||v|| where the box is inactive at s0, or box-active.  A box-active plane alone
// iterates gp_step, each step one pass over the plane (row = wavefront + 16 j, node = lane + 64 i: the same order whatever
// the batch) and one reduction in wavefront order; thread 0 updates s and broadcasts it through LDS, so that the control
// flow is uniform.  s at sout[b * ss + level].
// grid = (levels, B)
__global__ __launch_bounds__(GT_T) void k_gp_time_solve(Geom G, int ntiles, const double *__restrict__ u,
                                                        const double *__restrict__ r, long hist_stride,
                                                        const double *__restrict__ alpha, const double *__restrict__ opt_tab,
                                                        const int *__restrict__ mode, const double *__restrict__ W,
                                                        const double *__restrict__ part, double *__restrict__ sout, long ss) {
    __shared__ double sk[2][GT_W];
    __shared__ double bc[2];
    const int lvl = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (mode && mode[b] != GP_TIME) return;
    const double *ot = opt_tab + b * OPT_STRIDE;
    const double b3 = ot[OPT_B3], ks = ot[OPT_KS], umin = ot[OPT_UMIN], umax = ot[OPT_UMAX];
    const double al = alpha[b], lam = al * ks;
    if (tid == 0) {
        const double *p = part + ((long)b * gridDim.x + lvl) * ntiles * 4;
        double cc = 0.0, vv = 0.0, mx = 0.0, mn = 0.0;
        for (int t = 0; t < ntiles; ++t) {
            cc += p[4 * t]; vv += p[4 * t + 1];
            mx = fmax(mx, p[4 * t + 2]); mn = fmin(mn, p[4 * t + 3]);
        }
        double s = 0.0, act = 0.0;
        if (sqrt(cc) > lam) {
            s = 1.0 - lam / sqrt(vv);
            act = (s * mx > umax || s * mn < umin) ? 1.0 : 0.0;
        }
        bc[0] = s; bc[1] = act;
        if (act == 0.0) sout[b * ss + lvl] = s;
    }
    __syncthreads();
    double s = bc[0];
    if (bc[1] == 0.0) return;                 // the same in every thread
    const long lb = b * hist_stride + (long)lvl * G.plane;
    double lo = 0.0, hi = 1.0;                // thread 0's
    for (int it = 0; it < GP_MAXIT; ++it) {
        double q = 0.0, a = 0.0;
        for (int rr = wv; rr < G.ns; rr += GT_W)
            for (int c = lane; c < G.nf; c += 64) {
                const long o = (long)rr * G.pitch + c;
                const double v = gp_v(u[lb + o], r[lb + o], al, b3), w = W[o];
                const double sv = s * v, cl = fmin(fmax(sv, umin), umax);
                q += w * (cl * cl);
                a += cl == sv ? w * (v * v) : 0.0;
            }
        q = wave_sum(q); a = wave_sum(a);
        if (lane == 0) { sk[0][wv] = q; sk[1][wv] = a; }
        __syncthreads();
        if (tid == 0) {
            q = sk[0][0]; a = sk[1][0];
            for (int w = 1; w < GT_W; ++w) { q += sk[0][w]; a += sk[1][w]; }
            const bool done = gp_step(q, a, lam, s, lo, hi);
            bc[0] = s; bc[1] = done ? 1.0 : 0.0;
        }
        __syncthreads();                      // the next write of bc comes after the next step's barrier, which follows these reads
        s = bc[0];
        if (bc[1] != 0.0) break;
    }
    if (tid == 0) sout[b * ss + lvl] = s;
}

// TIME, stage 3.  u+ = clip(s v) of every node with its level's s into uout (or NULL: the sums alone), and the change
// partials {sum (u+ - u)^2, sum u^2} in the layout of k_grad_prox, which k_cost_fin folds.
// grid = (tiles, levels, B)
__global__ __launch_bounds__(NTH) void k_gp_time_apply(Geom G, int tiles_f, const double *__restrict__ u,
                                                       const double *__restrict__ r, long hist_stride,
                                                       const double *__restrict__ alpha, const double *__restrict__ opt_tab,
                                                       const int *__restrict__ mode, const double *__restrict__ sv, long ss,
                                                       double *__restrict__ uout, double *__restrict__ part) {
    const int b = blockIdx.z, lvl = blockIdx.y;
    if (mode && mode[b] != GP_TIME) return;
    const double *ot = opt_tab + b * OPT_STRIDE;
    const double b3 = ot[OPT_B3], umin = ot[OPT_UMIN], umax = ot[OPT_UMAX];
    const int tf = blockIdx.x % tiles_f, ts = blockIdx.x / tiles_f;
    const int c0 = tf * TX, r0 = ts * TY;
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
    __shared__ double sred[NPART * 4];
    const double al = alpha[b], s = sv[b * ss + lvl];
    const long lb = b * hist_stride + (long)lvl * G.plane;
    double acc[2] = {0.0, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        const int rr = r0 + ly0 + 4 * k, c = c0 + lx;
        if (rr < G.ns && c < G.nf) {
            const long o = lb + (long)rr * G.pitch + c;
            const double uu = u[o];
            const double un = gp_out(s, gp_v(uu, r[o], al, b3), umin, umax);
            if (uout) uout[o] = un;
            acc[0] += (un - uu) * (un - uu);
            acc[1] += uu * uu;
        }
    }
    if (part) {
        const int op[2] = {0, 0};
        block_reduce_store<2>(acc, op, sred, part + (((long)b * gridDim.y + lvl) * gridDim.x + blockIdx.x) * 4);
    }
}

// SPACE: one workgroup of GT_W wavefronts per (64 consecutive doubles of the pitched plane, trajectory); lane = node, so
// every level read is one coalesced 512-byte segment; wavefront w takes levels w, w + GT_W, ... and the wavefronts' partial
// sums are added in wavefront order through LDS.  Pass one: ||cone(v)||^2, ||v||^2 and the extremes of v.  Pencils the box
// holds iterate together (__syncthreads_or ends the loop), each step re-reading the pencil; the last pass writes u+ (uout
// or NULL: the sums alone).  chg (or NULL): [B][gridDim.x][2], this workgroup's share of sum (u+ - u)^2 and sum u^2; sout
// (or NULL): s at [b * ss + node], node = row * nf + column.
// grid = (ceil(plane / 64), B)
__global__ __launch_bounds__(GT_T) void k_gp_space(Geom G, int levels, const double *__restrict__ u, const double *__restrict__ r,
                                                   long hist_stride, const double *__restrict__ alpha,
                                                   const double *__restrict__ opt_tab, const int *__restrict__ mode,
                                                   const double *__restrict__ wt, double *__restrict__ uout,
                                                   double *__restrict__ sout, long ss, double *__restrict__ chg) {
    __shared__ double part[4][GT_W][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (mode && mode[b] != GP_SPACE) return;
    const long e = (long)blockIdx.x * 64 + lane;
    const int row = (int)(e / G.pitch), col = (int)(e - (long)row * G.pitch);
    const bool ok = e < G.plane && col < G.nf;
    const double *ot = opt_tab + b * OPT_STRIDE;
    const double b3 = ot[OPT_B3], ks = ot[OPT_KS], umin = ot[OPT_UMIN], umax = ot[OPT_UMAX];
    const long o = b * hist_stride + e;
    const double al = alpha[b], lam = al * ks;
    double cc = 0.0, vv = 0.0, mx = 0.0, mn = 0.0;
    if (ok) {
#pragma unroll 4
        for (int k = wv; k < levels; k += GT_W) {
            const double v = gp_v(u[o + k * G.plane], r[o + k * G.plane], al, b3), w = wt[k];
            const double cv = gp_cone(v, umin, umax);
            cc += w * (cv * cv);
            vv += w * (v * v);
            mx = fmax(mx, v);
            mn = fmin(mn, v);
        }
    }
    part[0][wv][lane] = cc; part[1][wv][lane] = vv; part[2][wv][lane] = mx; part[3][wv][lane] = mn;
    __syncthreads();
    cc = part[0][0][lane]; vv = part[1][0][lane]; mx = part[2][0][lane]; mn = part[3][0][lane];
    for (int w = 1; w < GT_W; ++w) {
        cc += part[0][w][lane]; vv += part[1][w][lane];
        mx = fmax(mx, part[2][w][lane]); mn = fmin(mn, part[3][w][lane]);
    }
    // from here on the wavefronts hold the same numbers for a pencil and take the same steps
    double s = 0.0, lo = 0.0, hi = 1.0;
    bool active = false;
    if (ok && sqrt(cc) > lam) {
        s = 1.0 - lam / sqrt(vv);
        active = s * mx > umax || s * mn < umin;
    }
    for (int it = 0; it < GP_MAXIT; ++it) {
        if (!__syncthreads_or(active)) break;         // also the barrier between two uses of part
        double q = 0.0, a = 0.0;
        if (active) {
#pragma unroll 4
            for (int k = wv; k < levels; k += GT_W) {
                const double v = gp_v(u[o + k * G.plane], r[o + k * G.plane], al, b3), w = wt[k];
                const double sv = s * v, cl = fmin(fmax(sv, umin), umax);
                q += w * (cl * cl);
                a += cl == sv ? w * (v * v) : 0.0;
            }
        }
        part[0][wv][lane] = q; part[1][wv][lane] = a;
        __syncthreads();
        if (active) {
            q = part[0][0][lane]; a = part[1][0][lane];
            for (int w = 1; w < GT_W; ++w) { q += part[0][w][lane]; a += part[1][w][lane]; }
            active = !gp_step(q, a, lam, s, lo, hi);
        }
    }
    double d2 = 0.0, n2 = 0.0;
    if (ok) {
#pragma unroll 4
        for (int k = wv; k < levels; k += GT_W) {
            const double uu = u[o + k * G.plane];
            const double un = gp_out(s, gp_v(uu, r[o + k * G.plane], al, b3), umin, umax);
            if (uout) uout[o + k * G.plane] = un;
            d2 += (un - uu) * (un - uu);
            n2 += uu * uu;
        }
    }
    if (ok && wv == 0 && sout) sout[b * ss + (long)row * G.nf + col] = s;
    if (!chg) return;
    d2 = wave_sum(d2); n2 = wave_sum(n2);
    __syncthreads();
    if (lane == 0) { part[0][wv][0] = d2; part[1][wv][0] = n2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        d2 = part[0][0][0]; n2 = part[1][0][0];
        for (int w = 1; w < GT_W; ++w) { d2 += part[0][w][0]; n2 += part[1][w][0]; }
        double *q = chg + ((long)b * gridDim.x + blockIdx.x) * 2;
        q[0] = d2; q[1] = n2;
    }
}

// The pencil norms of the SPACE cost, in the order of the kernel above: out [B][gridDim.x] = this workgroup's share of
// sum_ij W_ij sqrt(sum_k wt_k u_kij^2), its 64 nodes added by the wavefront's fixed tree; the host adds the workgroups in
// index order.
// grid = (ceil(plane / 64), B)
__global__ __launch_bounds__(GT_T) void k_gp_pencil(Geom G, int levels, const double *__restrict__ u, long hist_stride,
                                                    const int *__restrict__ mode, const double *__restrict__ wt,
                                                    const double *__restrict__ W, double *__restrict__ out) {
    __shared__ double part[GT_W][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (mode && mode[b] != GP_SPACE) return;
    const long e = (long)blockIdx.x * 64 + lane;
    const bool ok = e < G.plane && (int)(e % G.pitch) < G.nf;
    double a = 0.0;
    if (ok) {
#pragma unroll 4
        for (int k = wv; k < levels; k += GT_W) {
            const double uu = u[b * hist_stride + k * G.plane + e];
            a += wt[k] * (uu * uu);
        }
    }
    part[wv][lane] = a;
    __syncthreads();
    if (wv == 0) {
        a = part[0][lane];
        for (int w = 1; w < GT_W; ++w) a += part[w][lane];
        a = wave_sum(ok ? W[e] * sqrt(a) : 0.0);
        if (lane == 0) out[(long)b * gridDim.x + blockIdx.x] = a;
    }
}

// The KKT statistic by pencils for the SPACE trajectories (the others are left to k_kkt_count and to the level sums):
// cnt [B][3] += {#pencils ||u_g|| < tol, #pencils ||r_g|| <= kappa_s, #agree} in the pencil's norm, by ballot + popcount and
// three vector integer atomics per workgroup (integer sums do not depend on the order).  The caller zeroes cnt.
// grid = (ceil(plane / 64), B)
__global__ __launch_bounds__(GT_T) void k_gp_kkt_space(Geom G, int levels, const double *__restrict__ u,
                                                       const double *__restrict__ r, long hist_stride,
                                                       const double *__restrict__ opt_tab, const int *__restrict__ mode,
                                                       const double *__restrict__ wt, double tol,
                                                       unsigned long long *__restrict__ cnt) {
    __shared__ double part[2][GT_W][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (mode[b] != GP_SPACE) return;
    const long e = (long)blockIdx.x * 64 + lane;
    const bool ok = e < G.plane && (int)(e % G.pitch) < G.nf;
    const double ks = opt_tab[b * OPT_STRIDE + OPT_KS];
    double a0 = 0.0, a1 = 0.0;
    if (ok) {
#pragma unroll 4
        for (int k = wv; k < levels; k += GT_W) {
            const long o = b * hist_stride + k * G.plane + e;
            const double uu = u[o], rr = r[o], w = wt[k];
            a0 += w * (uu * uu);
            a1 += w * (rr * rr);
        }
    }
    part[0][wv][lane] = a0; part[1][wv][lane] = a1;
    __syncthreads();
    if (wv == 0) {
        a0 = part[0][0][lane]; a1 = part[1][0][lane];
        for (int w = 1; w < GT_W; ++w) { a0 += part[0][w][lane]; a1 += part[1][w][lane]; }
        const bool zero = ok && sqrt(a0) < tol, small = ok && sqrt(a1) <= ks;
        const unsigned nz = __popcll(__ballot(zero)), nsm = __popcll(__ballot(small)), nm = __popcll(__ballot(ok && zero == small));
        if (lane < 3) {
            const unsigned v = lane == 0 ? nz : (lane == 1 ? nsm : nm);
            if (v) atomicAdd(cnt + 3 * b + lane, (unsigned long long)v);
        }
    }
}

// =================================================================================
// `fin` kernels: one workgroup (64 threads) per trajectory; sum the per-workgroup partials
// in a fixed order and advance the trajectory's state machine.
// =================================================================================
__device__ __forceinline__ void fin_reduce(const double *part, int nblk, int b, double (&out)[NPART],
                                           const int (&op)[NPART], int n) {
    // all n slots in one pass over the workgroups' partials (the loads of a pass are independent), then the n wavefront
    // reductions side by side -- one slot after the other made this a chain of n x (loads + 6 shuffle steps)
    double a[NPART];
#pragma unroll
    for (int k = 0; k < NPART; ++k) a[k] = op[k] == 0 ? 0.0 : (op[k] == 1 ? 1e300 : -1e300);
    for (int t = threadIdx.x; t < nblk; t += 64) {
        const double *p = part + ((long)b * nblk + t) * NPART;
#pragma unroll
        for (int k = 0; k < NPART; ++k)
            if (k < n) {
                const double v = p[k];
                a[k] = op[k] == 0 ? a[k] + v : (op[k] == 1 ? fmin(a[k], v) : fmax(a[k], v));
            }
    }
#pragma unroll
    for (int k = 0; k < NPART; ++k)
        if (k < n) out[k] = op[k] == 0 ? wave_sum(a[k]) : (op[k] == 1 ? wave_min(a[k]) : wave_max(a[k]));
}

// The same reduction with FIN_PU workgroups' partials per lane in flight (VCH_LOADS_BATCH, the default): fin_fetch requests
// them -- a kernel does so before it waits for anything else -- and fin_reduce folds them in the loop's order, t = lane,
// lane + 64, ..., with the rolled loop for grids of more than 64 * FIN_PU tiles.
constexpr int FIN_PU = 5;      // 64 * FIN_PU = 320 tiles: the bench's 512 x 512 grid has 297
struct FinRegs {
    double q[FIN_PU][NPART];
};
// (a lane past the last workgroup reads the last workgroup's record -- a valid address, no branch -- and leaves it unused;
// all NPART slots of a record are read, whichever the caller sums)
__device__ __forceinline__ void fin_fetch(FinRegs &f, const double *part, int nblk, int b) {
#pragma unroll
    for (int i = 0; i < FIN_PU; ++i) {
        const int t = min((int)threadIdx.x + 64 * i, nblk - 1);
        const double *p = part + ((long)b * nblk + t) * NPART;
#pragma unroll
        for (int k = 0; k < NPART; ++k) f.q[i][k] = p[k];
    }
}
__device__ __forceinline__ void fin_reduce(const FinRegs &f, const double *part, int nblk, int b, double (&out)[NPART],
                                           const int (&op)[NPART], int n) {
    double a[NPART];
#pragma unroll
    for (int k = 0; k < NPART; ++k) a[k] = op[k] == 0 ? 0.0 : (op[k] == 1 ? 1e300 : -1e300);
#pragma unroll
    for (int i = 0; i < FIN_PU; ++i)
        if ((int)threadIdx.x + 64 * i < nblk) {
#pragma unroll
            for (int k = 0; k < NPART; ++k)
                if (k < n) {
                    const double v = f.q[i][k];
                    a[k] = op[k] == 0 ? a[k] + v : (op[k] == 1 ? fmin(a[k], v) : fmax(a[k], v));
                }
        }
    for (int t = threadIdx.x + 64 * FIN_PU; t < nblk; t += 64) {
        const double *p = part + ((long)b * nblk + t) * NPART;
#pragma unroll
        for (int k = 0; k < NPART; ++k)
            if (k < n) {
                const double v = p[k];
                a[k] = op[k] == 0 ? a[k] + v : (op[k] == 1 ? fmin(a[k], v) : fmax(a[k], v));
            }
    }
#pragma unroll
    for (int k = 0; k < NPART; ++k)
        if (k < n) out[k] = op[k] == 0 ? wave_sum(a[k]) : (op[k] == 1 ? wave_min(a[k]) : wave_max(a[k]));
}

// The fin kernels work on a trajectory's record in LDS: the 64 lanes copy it in (and out) together, one lane advances it.
// (A per-thread copy `TrajState S = st[b]` lives in private memory -- the record has arrays indexed at run time -- and
// costs ~120 scratch instructions and 70 one-lane global loads / stores per launch; through a reference to global memory
// every field access is a round trip.)
__device__ __forceinline__ void traj_copy_in(TrajState &dst, const TrajState *src) {
    const unsigned *s = reinterpret_cast<const unsigned *>(src);
    unsigned *d = reinterpret_cast<unsigned *>(&dst);
    for (int i = threadIdx.x; i < (int)(sizeof(TrajState) / 4); i += 64) d[i] = s[i];
    __syncthreads();
}
// ... in two halves (VCH_LOADS_BATCH): every dword of the record requested at once, and written to LDS behind the
// kernel's other requests.
struct TrajRegs {
    static constexpr int N = (int)(sizeof(TrajState) / 4), I = (N + 63) / 64;
    unsigned v[I];
};
__device__ __forceinline__ void traj_fetch(TrajRegs &t, const TrajState *src) {
    const unsigned *s = reinterpret_cast<const unsigned *>(src);
#pragma unroll
    for (int i = 0; i < TrajRegs::I; ++i) {
        t.v[i] = s[min((int)threadIdx.x + 64 * i, TrajRegs::N - 1)];
    }
}
__device__ __forceinline__ void traj_put(TrajState &dst, const TrajRegs &t) {
    unsigned *d = reinterpret_cast<unsigned *>(&dst);
#pragma unroll
    for (int i = 0; i < TrajRegs::I; ++i) {
        const int e = threadIdx.x + 64 * i;
        if (e < TrajRegs::N) d[e] = t.v[i];
    }
    __syncthreads();
}
__device__ __forceinline__ void traj_copy_out(TrajState *dst, const TrajState &src) {
    __syncthreads();
    const unsigned *s = reinterpret_cast<const unsigned *>(&src);
    unsigned *d = reinterpret_cast<unsigned *>(dst);
    for (int i = threadIdx.x; i < (int)(sizeof(TrajState) / 4); i += 64) d[i] = s[i];
}

constexpr int HIST_CAP = 512;          // >= max_iter + 1 residual norms (F2:353)
constexpr double NEWTON_TOL = 1e-6;    // F2:353
constexpr int NEWTON_MAXIT = 500;      // F2:353
constexpr double ARMIJO_ETA = 1e-4;    // F2:394
constexpr int ARMIJO_TRIALS = 12;      // F2:398

// Mark the trajectories that skip the coming march (flags[b] != 0).
__global__ void k_set_frozen(TrajState *st, const int *__restrict__ flags, int B) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) st[b].frozen = flags[b];
}

// After k_residual: the Armijo test (F2:411-419) or the bookkeeping of the initial residual,
// then the Newton stop test for the new iterate (F2:364, F2:356) and the setup of the next
// linear solve (preconditioner shift dbar = midpoint of the range of D).
// Preconditioner shift and CG iteration budget.  With A = P + M (D - dbar) (forward) or
// A = P + c (D - dbar) M (adjoint, c = dt/2), P the constant-coefficient operator with shift
// dbar < min D, the preconditioned operator is self-adjoint and positive in the inner product
// weighted by W (D - dbar) (forward, left preconditioning) resp. W / (D - dbar) (adjoint, right
// preconditioning), with spectrum in [1, kappa_T], kappa_T <= 1 + c (Dmax - dbar) / (c dbar + g0),
// g0 = lower bound of (P - c dbar M)/M.  CG therefore needs at most
// ln(2/tol) / -ln((sqrt(kappa_T)-1)/(sqrt(kappa_T)+1)) iterations.
__device__ __forceinline__ void cg_setup(TrajState &S, double g0, double cscale, double tol) {
    const double range = S.Dmax - S.Dmin;
    S.dbar = S.Dmin - fmax(1e-12, 0.05 * fmin(range, fabs(S.Dmin) + 1.0));
    const double den = cscale * S.dbar + g0;
    double kT = den > 0.0 ? 1.0 + cscale * (S.Dmax - S.dbar) / den : 1e12;
    const double sq = sqrt(kT);
    const double rate = (sq - 1.0) / (sq + 1.0);
    S.kT = kT;
    S.rho = rate;
    double k = rate > 1e-300 ? log(2.0 / tol) / -log(rate) : 1.0;
    S.lin_budget = (int)fmin(4000.0, ceil(k) + 2.0);
}

// Relative tolerance (Z-norm of the preconditioned residual) of a Newton linear solve inside a march.  The Schur
// residual s = rhs - A dphi that the solve leaves IS the second block row of the nonlinear residual of the next iterate
// (the first row is exact by back substitution), up to second-order terms, and P^-1 A has its spectrum in [1, ~1.04], so
// every component of s falls at the rate of the preconditioned residual.  eta = the absolute target for ||s||_2, a small
// fraction of the Newton tolerance (F2:353): the iteration ends when the reference's does.  A right-hand side above 1e8
// cannot be brought there by one fp64 solve (the 2-norm of s saturates near 1e-13..1e-10 ||rhs|| whatever the Z-norm
// does, which is why the reference's own first Newton step at 512^2 leaves ||R|| ~ 2 from 9e9): such a solve stops at
// 1e-12 and the next Newton iteration, which the reference needs as well, removes the rest.  eta = 0: lin_tol always.
__device__ __forceinline__ double newton_lin_tol(double r0, double lin_tol, double eta) {
    if (!(eta > 0.0) || !(r0 > 0.0)) return lin_tol;
    if (r0 > 1e8) return fmax(lin_tol, 1e-12);
    return fmin(fmax(lin_tol, eta / r0), 0.5);
}

// Options of the forward solves of a march, passed to the fin kernels that set a solve up.
struct SolveOpts {
    int cheb_max;              // plans of at most that many sweeps take the reduction-free form (-1: never, the CG form always)
    double scale_ratio;        // CG form: Dmax > scale_ratio * Dmin switches to the right-scaled system (0: never)
    double eta1_factor;        // first solve of a step: Schur-residual target max(eta, eta1_factor * min ||R_1|| of the last
                               // three steps) (0: eta always)
    unsigned long long *cell;  // [B][CeilCell::STRIDE] step-ceiling cells (below), reset where a solve is armed; NULL: not in use
};

// Step ceiling of a reduction-free solve in ONE 64-bit cell per trajectory: the workgroups of the solve's last row kernel
// fold their minima into it with an atomic minimum on an order-preserving integer key of the double (sign-flip map: the
// ratios are negative where phi has left the band).  A minimum is exact in any order, so the cell holds the same double as
// a fixed-order reduction over the workgroups' values; 1e300 = no constraint, as there.  Only the step alpha = min(1, 0.9 v)
// is ever taken from the cell (ceiling_alpha), and a ratio v >= FREE gives alpha = 1 whatever the other ratios are, like an
// empty cell: such a minimum is not folded, so a solve whose step no node constrains -- nearly every one -- makes no atomic
// at all.  The cells of a batch lie 128 B apart (atomics on one line are executed one after the other).
struct CeilCell {
    static constexpr int STRIDE = 16;
    static constexpr double FREE = 2.0;
    static __device__ __forceinline__ unsigned long long key(double v) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(v);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double value(unsigned long long k) {
        return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
    }
    static __device__ __forceinline__ void reset(unsigned long long *c) {
        __hip_atomic_store(c, key(1e300), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void fold(unsigned long long *c, double v) {
        if (v < FREE) __hip_atomic_fetch_min(c, key(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // (false for a NaN: skipped, as fmin skips it)
    }
    static __device__ __forceinline__ double load(const unsigned long long *c) {
        return value(__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
};
// F2:381-387: the first Armijo step from the smallest ceiling ratio (>= 1e299: no node constrains the step)
__device__ __forceinline__ double ceiling_alpha(double vmin) {
    double amax = 2.0;
    if (vmin < 1e299) amax = fmin(amax, 0.9 * vmin);
    if (!isfinite(amax) || amax <= 0.0) amax = 1.0;
    return fmin(1.0, amax);
}

// Right-scaled CG form.  With S = dbar / D (a diagonal in (0, 1]) the Schur operator is
//     A S = (I/dt + kappa/2 M^2)(I - F) + dbar M (I - F) + M D S ... = P - (I/dt + kappa/2 M^2) F,     F = I - S = (D - dbar) / D,
// so  T = P^-1 A S = I - E F  with the spectral multiplier  E = (I/dt + kappa/2 M^2) P^-1  in (0, 1).  T is self-adjoint and
// positive in <x, y>_F = sum W F x y, spectrum in [dbar / Dmax, 1]: the same worst-case bound as the unscaled form, but a node
// whose D is a hundred times its neighbours' -- |phi| within 1e-2 of 1, F ~ 1 -- now contributes an eigenvalue near
// 1 - mean(E) ~ 0.3-0.5 instead of 1 + (D - dbar) mean(M P^-1) ~ 50, and CG, which adapts to the spectrum it meets, needs a
// tenth of the sweeps on the clipped-noise start of BASELINE config 5 (profiles/r03_config5.txt).
// In kernel terms, against the unscaled form  q = p + (M P^-1)((D - dbar) p):  weight (D - dbar) / D instead of D - dbar,
// multiplier -(1/dt + kappa/2 m^2) / P(m) instead of m / P(m), and x = (dbar / D) y at the end.
__device__ __forceinline__ double cg_weight(double D, double dbar, int scaled) {
    const double dl = D - dbar;
    return scaled ? dl / D : dl;
}

// Chebyshev plan of a forward solve: with spec(P^-1 A) in [1, kT] (cg_setup) the iteration
//     y_1 = b~ / theta,   y_{j+1} = y_j + rho_j rho_{j-1} (y_j - y_{j-1}) + (2 rho_j / delta) (b~ - P^-1 A y_j)
// (b~ = P^-1 rhs, rho_0 = delta / theta, rho_j = 1 / (2 theta / delta - rho_{j-1})) leaves, in the norm the stop test of the
// CG form uses, ||z_{n+1}||_Z <= ||z_0||_Z / T_{n+1}(theta / delta) after n sweeps: n is the smallest count for which that
// bound is below the solve's tolerance.  The first iterate costs no sweep (the preconditioner application alone).
constexpr int CHEB_NCAP = 200;
__device__ __forceinline__ void cheb_plan(TrajState &S, double tol) {
    const double kT = S.kT > 1.0 ? S.kT : 1.0;
    S.cheb_theta = 0.5 * (kT + 1.0);
    S.cheb_delta = 0.5 * (kT - 1.0);
    int n = 0;
    if (S.cheb_delta > 0.0) {
        const double sigma = S.cheb_theta / S.cheb_delta;
        double tkm1 = 1.0, tk = sigma;                       // T_0, T_1
        while (n < CHEB_NCAP && !(1.0 / tk <= tol)) {
            const double tn = 2.0 * sigma * tk - tkm1;
            tkm1 = tk;
            tk = tn;
            ++n;
        }
    }
    S.cheb_n = n;
}
// T_n(sigma) / T_{n+1}(sigma): what the bound promises for the last step of an n-sweep solve
__device__ __forceinline__ double cheb_last_factor(double theta, double delta, int n) {
    if (!(delta > 0.0)) return 0.0;
    const double sigma = theta / delta;
    double tkm1 = 1.0, tk = sigma;
    for (int k = 0; k < n; ++k) {
        const double tn = 2.0 * sigma * tk - tkm1;
        tkm1 = tk;
        tk = tn;
        if (!(tk < 1e280)) return 1.0 / (2.0 * sigma);      // far in the asymptotic range
    }
    return tkm1 / tk;
}

// gpart: partials written by the GEMM epilogue (gnblk per trajectory, 1 value each)
__device__ __forceinline__ double fin_sum1(const double *part, int n, int b, int stride, int k) {
    double a = 0.0;
    for (int t = threadIdx.x; t < n; t += 64) a += part[((long)b * n + t) * stride + k];
    return wave_sum(a);
}
// ... with FIN_PU partials per lane in flight (VCH_LOADS_BATCH): sum1_fetch, then fin_sum1 in the loop's order
struct Sum1Regs {
    double q[FIN_PU];
};
__device__ __forceinline__ void sum1_fetch(Sum1Regs &f, const double *part, int n, int b, int stride, int k) {
#pragma unroll
    for (int i = 0; i < FIN_PU; ++i) {
        f.q[i] = part[((long)b * n + min((int)threadIdx.x + 64 * i, n - 1)) * stride + k];      // n >= 1
    }
}
__device__ __forceinline__ double fin_sum1(const Sum1Regs &f, const double *part, int n, int b, int stride, int k) {
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < FIN_PU; ++i)
        if ((int)threadIdx.x + 64 * i < n) a += f.q[i];
    for (int t = threadIdx.x + 64 * FIN_PU; t < n; t += 64) a += part[((long)b * n + t) * stride + k];
    return wave_sum(a);
}

// What k_fin_ceiling gets after a Chebyshev solve with `enq` sweeps enqueued (enq < 0: no such solve).
struct ChebFin {
    int enq, gnblk;
    const double *g0, *gn;                  // [B][gnblk] partials of <z_0,z_0>_Z and of <z_n,z_n>_Z
    const double *cmin;                     // [B][gnblk] step-ceiling ratios taken by the solve's last row kernel
};
// The books of a finished reduction-free solve: the relative residual it left, estimated as the last directly summed
// ||z_n||_Z / ||z_0||_Z (partials of k_cheb_rows; all 64 lanes) times the factor T_n / T_{n+1} the bound promises for the last
// step, and the sweep counts (one lane).
__device__ __forceinline__ double cheb_solve_rel(int cheb_n, const ChebFin &cheb, int b) {
    if (cheb_n < 1) return 1.0;
    const double g0 = fin_sum1(cheb.g0, cheb.gnblk, b, 1, 0), gn = fin_sum1(cheb.gn, cheb.gnblk, b, 1, 0);
    return g0 > 0.0 ? sqrt(fmax(gn, 0.0) / g0) : 0.0;
}
__device__ __forceinline__ double cheb_solve_rel(int cheb_n, const ChebFin &cheb, int b, const Sum1Regs &r0, const Sum1Regs &rn) {
    if (cheb_n < 1) return 1.0;
    const double g0 = fin_sum1(r0, cheb.g0, cheb.gnblk, b, 1, 0), gn = fin_sum1(rn, cheb.gn, cheb.gnblk, b, 1, 0);
    return g0 > 0.0 ? sqrt(fmax(gn, 0.0) / g0) : 0.0;
}
__device__ __forceinline__ void cheb_close_books(TrajState &S, double rel) {
    rel *= cheb_last_factor(S.cheb_theta, S.cheb_delta, S.cheb_n);
    S.lin_rel = rel;
    S.lin_it = S.cheb_n;
    S.lin_total += S.cheb_n;
    if (rel * S.lin_rscale > S.lin_maxrel) S.lin_maxrel = rel * S.lin_rscale;
    S.lin_maxabs = fmax(S.lin_maxabs, rel * S.lin_r0);
    if (S.cheb_n > S.step_lin_max) S.step_lin_max = S.cheb_n;
    if (S.step_solves >= 1 && S.step_solves <= 4) S.step_lin[S.step_solves - 1] = S.cheb_n;
}
// Start of the Armijo loop (F2:388-396) from the smallest ceiling ratio; lin_active: the solve was cut short by the host's budget
__device__ __forceinline__ void ceiling_arm(TrajState &S, double vmin, int lin_active) {
    S.alpha = ceiling_alpha(vmin);
    if (lin_active && S.lin_rel > S.lin_maxrel) S.lin_maxrel = S.lin_rel;     // the host's sweep budget ran out: go on
    S.lin_active = 0;                                                         // with an inexact step
    S.need_trial = 1;
    S.trial_no = 0;
    S.force_accept = 0;
    S.best_norm = 1e300;
    S.best_alpha = S.alpha;
}

// Optional tails of k_fin_residual.
//   cheb.enq >= 0 (MODE 1, the trial that follows a reduction-free solve with cheb.enq sweeps enqueued; so.cell set): no
//   k_fin_ceiling launch has run.  A trajectory whose solve has just finished (Newton running, no trial pending, use_cheb,
//   and not a plan longer than cheb.enq that is still lin_active) had its trial armed by k_eval<2> itself from the ceiling
//   cell; the same is done to the record here -- the solve's books, alpha from the cell, trial 0 -- before the Armijo /
//   Newton step.
//   pub != NULL (the launch the host's look follows): the workgroup of trajectory b copies its record to the mapped host
//   memory pub[b] and then stores val to seq[b] (system-scope release behind a system fence), on every path through the kernel.
struct FinTail {
    ChebFin cheb;
    TrajState *pub;
    unsigned long long *seq, val;
};

template <int MODE>
__device__ __forceinline__ void fin_residual_update(TrajState &S, const double (&v)[NPART], bool primed, double *__restrict__ hist,
                                                    double kappa, double dt, double lin_tol, double eta, SolveOpts so);

// BATCH (the default; VCH_LOADS_BATCH=0 launches k_fin_residual_plain): everything whose address does not depend on the
// record -- the partials, the two sums of a reduction-free solve and the ceiling cell, each guarded by kernel arguments only
// -- is requested with the record, in front of the barrier behind its copy; a path that returns early leaves them unused.
template <int MODE, bool BATCH>
__device__ __forceinline__ void fin_residual_body(TrajState *st, const double *__restrict__ part, int nblk,
                                                  double *__restrict__ hist, double kappa, double dt, double lin_tol, double eta,
                                                  int guess, SolveOpts so, const FinTail &tail) {
    const int b = blockIdx.x;
    __shared__ TrajState S;
    FinRegs fr;
    Sum1Regs r0, rn;
    double cell_v = 1e300;
    const bool pre_cheb = BATCH && MODE == 1 && tail.cheb.enq >= 0 && tail.cheb.g0 && tail.cheb.gn && tail.cheb.gnblk > 0;
    const bool pre_cell = BATCH && MODE == 1 && tail.cheb.enq >= 0 && so.cell;
    if (BATCH) {
        TrajRegs tr;
        traj_fetch(tr, st + b);
        fin_fetch(fr, part, nblk, b);
        if (pre_cheb) {
            sum1_fetch(r0, tail.cheb.g0, tail.cheb.gnblk, b, 1, 0);
            sum1_fetch(rn, tail.cheb.gn, tail.cheb.gnblk, b, 1, 0);
        }
        if (pre_cell && threadIdx.x == 0) cell_v = CeilCell::load(so.cell + b * CeilCell::STRIDE);
        traj_put(S, tr);
    } else {
        traj_copy_in(S, st + b);
    }
    bool go = true;                // (the same for all 64 lanes)
    if (MODE == 2) {               // after k_eval<0> without the fin step inside: the record has not been armed yet
        go = !S.frozen;
        if (go && threadIdx.x == 0) {
            newton_begin(S);
            S.slot = 1 - S.slot;
        }
        __syncthreads();
    }
    go = go && S.newton_active && S.need_trial;
    if (MODE == 1 && !go && tail.cheb.enq >= 0 && S.newton_active && S.use_cheb && !(S.lin_active && S.cheb_n > tail.cheb.enq)) {
        const int books = S.lin_active;             // as in k_fin_ceiling: not after k_cg_publish has taken the flag back
        const double rel = !books ? 1.0 : (pre_cheb ? cheb_solve_rel(S.cheb_n, tail.cheb, b, r0, rn) : cheb_solve_rel(S.cheb_n, tail.cheb, b));
        __syncthreads();
        if (threadIdx.x == 0) {
            if (books) cheb_close_books(S, rel);
            ceiling_arm(S, pre_cell ? cell_v : CeilCell::load(so.cell + b * CeilCell::STRIDE), 0);
        }
        __syncthreads();
        go = true;
    }
    if (go) {
        double v[NPART];
        const int op[NPART] = {0, 0, 1, 2, 0, 0};
        // guess: k_guess has deflated the right-hand side (MODE 0: of the step's first solve; MODE 1: of its second solve, for
        // a trajectory whose first solve is done); slot 1 holds sum (rhs - A x0)^2, slot 4 sum rhs^2
        const bool primed = guess_bit((unsigned)guess, b) && (MODE != 1 || S.iters == 1);
        if (BATCH) fin_reduce(fr, part, nblk, b, v, op, primed ? 5 : 4);
        else fin_reduce(part, nblk, b, v, op, primed ? 5 : 4);
        if (so.cell) so.cell += b * CeilCell::STRIDE;
        if (threadIdx.x == 0)
            fin_residual_update<(MODE == 1 ? 1 : 0)>(S, v, primed, hist + (long)b * HIST_CAP, kappa, dt, lin_tol, eta, so);
        traj_copy_out(st + b, S);
    }
    if (tail.pub) {
        __syncthreads();
        const unsigned *s = reinterpret_cast<const unsigned *>(&S);
        unsigned *d = reinterpret_cast<unsigned *>(tail.pub + b);
        for (int i = threadIdx.x; i < (int)(sizeof(TrajState) / 4); i += 64) d[i] = s[i];
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(tail.seq + b, tail.val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
#define FIN_RESIDUAL_PARAMS TrajState *st, const double *__restrict__ part, int nblk, double *__restrict__ hist, double kappa, \
                            double dt, double lin_tol, double eta, int guess, SolveOpts so, FinTail tail
#define FIN_RESIDUAL_ARGS st, part, nblk, hist, kappa, dt, lin_tol, eta, guess, so, tail
template <int MODE>
__global__ void k_fin_residual(FIN_RESIDUAL_PARAMS) { fin_residual_body<MODE, true>(FIN_RESIDUAL_ARGS); }
template <int MODE>
__global__ void k_fin_residual_plain(FIN_RESIDUAL_PARAMS) { fin_residual_body<MODE, false>(FIN_RESIDUAL_ARGS); }

template <int MODE>
__device__ __forceinline__ void fin_residual_update(TrajState &S, const double (&v)[NPART], bool primed, double *__restrict__ hist,
                                                    double kappa, double dt, double lin_tol, double eta, SolveOpts so) {
    const double nt = sqrt(v[0]);
    bool accept;
    if (MODE == 0) {
        accept = true;
    } else {
        S.ntrials++;
        if (S.force_accept) {
            accept = true;
        } else {
            if (nt < S.best_norm) { S.best_norm = nt; S.best_alpha = S.alpha; }
            accept = nt <= (1.0 - ARMIJO_ETA * S.alpha) * S.normR;
        }
    }
    if (accept) {
        if (MODE == 1) S.slot = 1 - S.slot;
        S.normR = nt;
        S.need_trial = 0;
        S.force_accept = 0;
        if (S.iters < HIST_CAP) hist[S.iters] = nt;
        if (S.iters < 4) S.step_R[S.iters] = nt;
        if (S.iters == 1) {                     // the residual after this step's first Newton iteration
            S.R1_hist[2] = S.R1_hist[1];
            S.R1_hist[1] = S.R1_hist[0];
            S.R1_hist[0] = nt;
        }
        S.iters++;
        S.newton_total++;
        // F2:364: converged; F2:356: the loop body runs at most max_iter times
        if (!(nt >= NEWTON_TOL) || S.iters > NEWTON_MAXIT) {
            // note: a NaN norm also ends the loop here (the reference would spin on NaN)
            if (S.iters > NEWTON_MAXIT) S.iters = NEWTON_MAXIT;
            S.newton_active = 0;
            return;
        }
        // next linear solve
        S.Dmin = v[2];
        S.Dmax = v[3];
        S.lin_r0 = sqrt(v[1]);
        S.x_primed = primed ? 1 : 0;
        S.lin_rscale = (primed && v[4] > 0.0) ? fmin(1.0, sqrt(v[1] / v[4])) : 1.0;
        if (MODE == 0) S.guess_ratio = (primed && v[4] > 0.0) ? sqrt(v[1] / v[4]) : 1.0;
        else if (primed) S.guess_ratio2 = v[4] > 0.0 ? sqrt(v[1] / v[4]) : 1.0;
        // Forcing rule.  The Schur residual a solve leaves enters the next iterate's residual additively; what decides the
        // Newton loop is whether that residual is below the tolerance.  After the FIRST iteration of a step it is dominated by
        // the quadratic remainder ||R_1||, known from the previous steps to within a factor (R1_hist): a first solve that
        // leaves eta1_factor (1 %) of it changes ||R_1|| by 1 % -- the decision only if ||R_1|| is within 1 % of the tolerance,
        // and there (||R_1|| < 5e-6) the rule below gives eta itself, as for every later solve.
        double eta_eff = eta;
        if (MODE == 0 && eta > 0.0 && so.eta1_factor > 0.0 && S.R1_hist[0] > 0.0 && S.R1_hist[1] > 0.0 && S.R1_hist[2] > 0.0)
            eta_eff = fmax(eta, so.eta1_factor * fmin(S.R1_hist[0], fmin(S.R1_hist[1], S.R1_hist[2])));
        S.lin_reltol = newton_lin_tol(S.lin_r0, lin_tol, eta_eff);
        cg_setup(S, 2.0 * sqrt(0.5 * kappa / dt), 1.0, S.lin_reltol);
        cheb_plan(S, S.lin_reltol);
        S.use_cheb = (so.cheb_max >= 0 && S.cheb_n <= so.cheb_max) ? 1 : 0;
        S.scaled = (!S.use_cheb && so.scale_ratio > 0.0 && S.Dmax > so.scale_ratio * S.Dmin) ? 1 : 0;
        S.lin_active = 1;
        if (so.cell) CeilCell::reset(so.cell);          // (the caller's pointer is this trajectory's cell)
        S.lin_it = 0;
        S.lin_prev = 1e300;
        S.lin_rel = 1.0;
        S.nsolves++;
        S.step_solves++;
        if (S.step_solves <= 4) {
            S.step_tol[S.step_solves - 1] = S.lin_reltol;
            S.step_kT[S.step_solves - 1] = S.kT;
            S.step_chn[S.step_solves - 1] = S.cheb_n;
            S.step_form[S.step_solves - 1] = S.use_cheb;
        }
        // (a zero right-hand side is not special-cased: the solve starts, zeroes x and ends at its first reduction point)
    } else {
        S.alpha *= 0.5;
        S.trial_no++;
        if (S.trial_no >= ARMIJO_TRIALS) {
            if (S.best_norm < S.normR) {     // F2:422-423: fall back to the best trial
                S.alpha = S.best_alpha;
                S.force_accept = 1;
            } else {
                // F2:424-425: state unchanged -> every later iteration repeats this one
                // bit for bit until max_iter; record that and stop.
                S.stuck = 1;
                S.need_trial = 0;
                while (S.iters < NEWTON_MAXIT) {
                    if (S.iters < HIST_CAP) hist[S.iters] = S.normR;
                    S.iters++;
                }
                S.newton_active = 0;
            }
        }
    }
}

// =================================================================================
// Fused evaluation kernels of a march on the stencil-free path (one launch where the separate form has three or four):
//   MODE 0  start of a time step:  k_prepare + k_residual<0> + k_guess(first solve) + k_fin_residual<0>
//   MODE 2  Armijo trial after a reduction-free solve:  k_residual2 + k_guess(second solve) + k_fin_residual<1>
// Same arithmetic on the same numbers in the same order as the separate kernels: bit-identical results.
//
// The `fin` step (sum the workgroups' partials, Armijo / Newton tests, set-up of the next solve) is done by the workgroup
// of a trajectory that finishes LAST: every workgroup stores its partials write-through (agent-scope stores), drains them
// (s_waitcnt vmcnt(0)) and adds 1 to the trajectory's counter (agent-scope atomic, value returned); the one whose add
// returns nblk - 1 reads all partials with agent-scope loads (never through this CU's L1 or a stale line of its XCD's L2:
// MI355X_MICROARCH.md, inter-workgroup visibility, 8-byte stores / loads, one lane signalling for its workgroup), sums them
// in the fixed order of fin_reduce -- whichever workgroup that is, the result has the same bits -- and resets the counter.
// =================================================================================
struct EvalFin {
    unsigned *counter;         // [B], zero between launches
    double *hist;              // [B][HIST_CAP] residual-norm histories
    double kappa, lin_tol, eta;
    SolveOpts so;
    int cheb_enq;              // MODE 2 without the fin step inside: sweeps enqueued for the reduction-free solve this trial follows,
                               // with no k_fin_ceiling launch in between (FinTail); -1: off
};

__device__ __forceinline__ void store_agent(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double load_agent(const double *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// fin_reduce on partials handed over inside a launch (agent-scope loads); same order of operations
__device__ __forceinline__ void fin_reduce_agent(const double *part, int nblk, int b, double (&out)[NPART], const int (&op)[NPART], int n) {
    double a[NPART];
#pragma unroll
    for (int k = 0; k < NPART; ++k) a[k] = op[k] == 0 ? 0.0 : (op[k] == 1 ? 1e300 : -1e300);
    for (int t = threadIdx.x; t < nblk; t += 64) {
        const double *p = part + ((long)b * nblk + t) * NPART;
#pragma unroll
        for (int k = 0; k < NPART; ++k)
            if (k < n) {
                const double v = load_agent(p + k);
                a[k] = op[k] == 0 ? a[k] + v : (op[k] == 1 ? fmin(a[k], v) : fmax(a[k], v));
            }
    }
#pragma unroll
    for (int k = 0; k < NPART; ++k)
        if (k < n) out[k] = op[k] == 0 ? wave_sum(a[k]) : (op[k] == 1 ? wave_min(a[k]) : wave_max(a[k]));
}

#ifndef EVAL_MINBLK
#define EVAL_MINBLK 5          // workgroups per CU the register allocation must allow (LDS allows 5)
#endif
// Every global operand of the later phases is loaded into registers BEFORE the first barrier, so a workgroup pays the
// global-memory latency once instead of once per phase (march at 8 trajectories 0.533 -> 0.517 s, bench 5.17 -> 5.31; with
// the register cap lifted to fit them all, 122 VGPRs = 4 workgroups per CU: 0.551 s; profiles/r03_fused_ab.txt).
// FIN_INSIDE: the hand-off variant (VCH_FUSED=1).  The default variant ends with the partials and carries neither the record
// copy of the fin step (584 B of private memory per thread) nor the counter traffic.
//
// HOIST (the default; VCH_EVAL_HOIST=0 selects the kernels without it, k_eval_plain): the same is done for the step start
// and for the guess tail.  Values, expressions and summation orders are those of the plain form, only the place where a load
// is issued and where a value is kept differs, so the two forms agree bit for bit.
//   step start   every global operand -- k_mass's partials (first wavefront), raw phi, mu of the old level, w, u_n, u_{n+1}
//                -- is requested before the first barrier; the partials are summed in post_sums' order behind the requests,
//                and sp / sm are written from registers behind post_sums' barrier.  The plain form asks for mu, w and the
//                u pair only behind that barrier: two global latencies in series for every workgroup.
//   guess tail   plane 0 of the increments is requested behind the last halo-1 pass and arrives under the own-node pass, every
//                further plane is read with the thread's halo-2 elements in flight together, and the sum is kept in registers
//                up to the tail's barrier.  D on halo 1 needs no pass and no barrier of its own: MODE 2 writes it into sd in
//                the last halo-1 pass, which has phi in a register; MODE 0 (no free LDS plane) takes it from sp in front of
//                the tail's barrier.  (Two planes in flight, or MODE 0's D in registers from the halo-1 pass on, spill at
//                EVAL_MINBLK workgroups per CU: DESIGN.md 4.)
constexpr int POST_PU = 5;     // partials of k_mass held per lane of the first wavefront (64 * POST_PU workgroups per round)
template <int MODE, bool FIN_INSIDE, bool HOIST>
__device__ __forceinline__ void eval_body(const Geom &G, const Phys &P, TrajState *st, long slot_stride, double *phi_s, double *mu_s,
                                          double *Rphi_s, double *rhs_s, double *D_s, const double *dphi, double *cphi,
                                          double *cmu, double dt, double *part, const double *w, const double *un,
                                          const double *unp1, long u_stride, double *wnew, const GuessArgs &ga, double *x0,
                                          const EvalFin &fin, const PostArgs &post) {
    TILE_COORDS;
    // only the few fields the evaluation needs are read here; the record as a whole is read, advanced and written back by
    // one thread of the workgroup that finishes last (a per-thread copy of the record would live in private memory)
    const int S_slot = st[b].slot, S_iters = MODE == 0 ? 0 : st[b].iters;
    double S_alpha = MODE == 0 ? 0.0 : st[b].alpha;
    // (read beside the record, not behind it: the cell's address does not depend on the record)
    const bool use_cell = MODE == 2 && !FIN_INSIDE && fin.cheb_enq >= 0;
    const double cell_min = use_cell ? CeilCell::load(fin.so.cell + b * CeilCell::STRIDE) : 1e300;
    if (MODE == 0) {
        if (st[b].frozen) {    // what newton_begin does for a trajectory that sits this march out
            if (blk == 0 && threadIdx.x == 0) st[b].newton_active = st[b].need_trial = st[b].lin_active = 0;
            return;
        }
    } else {
        if (!st[b].newton_active) return;
        if (!st[b].need_trial) {
            // a reduction-free solve that has just finished (no k_fin_ceiling launch: the record is armed by the k_fin_residual
            // behind this kernel): trial 0 with the step the ceiling cell allows, the same number in every workgroup
            // (k_fin_ceiling's conditions: an unfinished plan is left alone; lin_active may already have been taken back by
            // k_cg_publish when a long CG solve of a batch mate ran behind this trajectory's solve)
            if (!use_cell || !st[b].use_cheb || (st[b].lin_active && st[b].cheb_n > fin.cheb_enq)) return;
            S_alpha = ceiling_alpha(cell_min);
        }
    }
    __shared__ double sp[(TY + 4) * (TX + 4)];
    __shared__ double sd[MODE == 2 ? (TY + 4) * (TX + 4) : 1];
    __shared__ double sm[(TY + 2) * (TX + 2)];
    __shared__ double sr[MODE == 0 ? (TY + 2) * (TX + 2) : 1];
    __shared__ double sred[NPART * 4];
    __shared__ int s_last;
    constexpr int W2 = TX + 4, W1 = TX + 2;
    const long pb = b * G.plane;
    // both modes write the evaluated iterate into the OTHER slot: in MODE 0 the new mu (the Newton start value) must not
    // land where a neighbouring workgroup may still be loading the halo of the old one
    const int src = S_slot, dst = 1 - S_slot;
    const double tdt = P.tau / dt;
    const double *gcf = ga.row(b);
    const bool do_guess = gcf[0] != 0.0 && (MODE == 0 || S_iters == 1);
    double rm[TY / 4], rh[TY / 4];
    double acc[5] = {0.0, 0.0, 1e300, -1e300, 0.0};
    // HOIST, guess tail: D on halo 1 (MODE 0; MODE 2 has sd free for it) and an increment plane on halo 2 (plane 0 in gT[0], every
    // further one in turn in gT[1]), per thread
    constexpr int GN2 = W2 * (TY + 4), GI2 = (GN2 + NTH - 1) / NTH, GN1 = (TY + 2) * W1, GI1 = (GN1 + NTH - 1) / NTH;
    double gD[GI1], gT[2][GI2];
    auto guess_load = [&](int j) {
#pragma unroll
        for (int i = 0; i < GI2; ++i) {
            const int e = threadIdx.x + i * NTH;
            gT[j != 0][i] = 0.0;
            if (e < GN2) {
                int ly = e / W2, lxx = e - ly * W2;
                int gr = refl(r0 - 2 + ly, G.ns), gc = refl(c0 - 2 + lxx, G.nf);
                gT[j != 0][i] = ga.d[j][pb + (long)gr * G.pitch + gc];
            }
        }
    };
    if (MODE == 0) {
        // ---- k_prepare + k_residual<0> ----
        constexpr int N1 = (TY + 2) * W1, I1 = (N1 + NTH - 1) / NTH;      // halo-1 elements, per thread
        double vW[I1], vU0[I1], vU1[I1];
        if (HOIST) {
            __shared__ double s_post[2];
            constexpr int N2 = W2 * (TY + 4), I2 = (N2 + NTH - 1) / NTH;
            // k_mass's partials first (the longest dependent chain hangs on them): post_sums' lanes and order, POST_PU
            // partials per lane in flight instead of one
            const bool sums = post.part && threadIdx.x < 64;
            const double *pq = post.part ? post.part + (long)b * nblk * NPART : nullptr;
            double q0[POST_PU], q1[POST_PU];
            if (sums) {
#pragma unroll
                for (int k = 0; k < POST_PU; ++k) {
                    const int t = threadIdx.x + 64 * k;
                    q0[k] = q1[k] = 0.0;
                    if (t < nblk) {
                        q0[k] = pq[(long)t * NPART];
                        q1[k] = pq[(long)t * NPART + 1];
                    }
                }
            }
            const double mass0 = st[b].mass0;
            double raw[I2], vM[I1];
#pragma unroll
            for (int i = 0; i < I2; ++i) {
                const int e = threadIdx.x + i * NTH;
                raw[i] = 0.0;
                if (e < N2) {
                    int ly = e / W2, lxx = e - ly * W2;
                    int gr = refl(r0 - 2 + ly, G.ns), gc = refl(c0 - 2 + lxx, G.nf);
                    raw[i] = phi_s[src * slot_stride + pb + (long)gr * G.pitch + gc];
                }
            }
#pragma unroll
            for (int i = 0; i < I1; ++i) {                                   // mu first: it goes to LDS with phi
                const int e = threadIdx.x + i * NTH;
                vM[i] = 0.0;
                if (e < N1) {
                    int ly = e / W1, lxx = e - ly * W1;
                    int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
                    vM[i] = mu_s[src * slot_stride + pb + (long)gr * G.pitch + gc];
                }
            }
#pragma unroll
            for (int i = 0; i < I1; ++i) {
                const int e = threadIdx.x + i * NTH;
                vW[i] = vU0[i] = vU1[i] = 0.0;
                if (e < N1) {
                    int ly = e / W1, lxx = e - ly * W1;
                    int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
                    long o = (long)gr * G.pitch + gc;
                    vW[i] = w[pb + o];
                    vU0[i] = un ? un[b * u_stride + o] : 0.0;
                    vU1[i] = unp1 ? unp1[b * u_stride + o] : 0.0;
                }
            }
            if (post.part) {
                if (sums) {
                    double a0 = 0.0, a1 = 0.0;
#pragma unroll
                    for (int k = 0; k < POST_PU; ++k)
                        if ((int)threadIdx.x + 64 * k < nblk) {
                            a0 += q0[k];
                            a1 += q1[k];
                        }
                    for (int t = threadIdx.x + 64 * POST_PU; t < nblk; t += 64) {     // grids of more than 64 * POST_PU tiles
                        a0 += pq[(long)t * NPART];
                        a1 += pq[(long)t * NPART + 1];
                    }
                    a0 = wave_sum(a0);
                    a1 = wave_sum(a1);
                    if (threadIdx.x == 0) {
                        s_post[0] = a0;
                        s_post[1] = a1;
                    }
                }
                __syncthreads();
                const PostFix pf(s_post, mass0, P.LxLy);
                if (post.rec && blk == 0 && threadIdx.x == 0) pf.record(post.rec + b * post.rec_stride, s_post);
#pragma unroll
                for (int i = 0; i < I2; ++i) raw[i] = pf.apply(raw[i]);
            }
#pragma unroll
            for (int i = 0; i < I2; ++i) {
                const int e = threadIdx.x + i * NTH;
                if (e < N2) sp[e] = raw[i];
            }
#pragma unroll
            for (int i = 0; i < I1; ++i) {
                const int e = threadIdx.x + i * NTH;
                if (e < N1) sm[e] = vM[i];
            }
        } else {                                                             // the plain form
            if (post.part) {
                // the end of the previous step (F2:562-577: clip, mass fix, history) applied to the level as it is loaded: the sums
                // of k_mass's partials by the first wavefront while everybody's loads are in flight, then the fix in registers
                __shared__ double s_post[2];
                constexpr int I2 = (W2 * (TY + 4) + NTH - 1) / NTH;
                double raw[I2];
#pragma unroll
                for (int i = 0; i < I2; ++i) {
                    const int e = threadIdx.x + i * NTH;
                    raw[i] = 0.0;
                    if (e < W2 * (TY + 4)) {
                        int ly = e / W2, lxx = e - ly * W2;
                        int gr = refl(r0 - 2 + ly, G.ns), gc = refl(c0 - 2 + lxx, G.nf);
                        raw[i] = phi_s[src * slot_stride + pb + (long)gr * G.pitch + gc];
                    }
                }
                post_sums(post.part, nblk, (int)b, s_post);
                __syncthreads();
                const PostFix pf(s_post, st[b].mass0, P.LxLy);
                if (post.rec && blk == 0 && threadIdx.x == 0) pf.record(post.rec + b * post.rec_stride, s_post);
#pragma unroll
                for (int i = 0; i < I2; ++i) {
                    const int e = threadIdx.x + i * NTH;
                    if (e < W2 * (TY + 4)) sp[e] = pf.apply(raw[i]);
                }
            } else {
                load_tile<2, false>(sp, phi_s + src * slot_stride + pb, G, c0, r0);
            }
            load_tile<1, false>(sm, mu_s + src * slot_stride + pb, G, c0, r0);          // mu of the old level
#pragma unroll
            for (int i = 0; i < I1; ++i) {
                const int e = threadIdx.x + i * NTH;
                vW[i] = vU0[i] = vU1[i] = 0.0;
                if (e < N1) {
                    int ly = e / W1, lxx = e - ly * W1;
                    int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
                    long o = (long)gr * G.pitch + gc;
                    vW[i] = w[pb + o];
                    vU0[i] = un ? un[b * u_stride + o] : 0.0;
                    vU1[i] = unp1 ? unp1[b * u_stride + o] : 0.0;
                }
            }
        }
        __syncthreads();
        if (HOIST) {                                                         // the u pair is needed as its sum only
#pragma unroll
            for (int i = 0; i < I1; ++i) vU1[i] = vU1[i] + vU0[i];
        }
        for (int k = 0; k < TY / 4; ++k) {                                   // c_mu needs the Laplacian of the old mu
            int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
            rm[k] = 0.0;
            if (r < G.ns && c < G.nf) {
                int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
                const double cm = -sp[p2] / dt - 0.5 * lap_at<W1>(sm, p1, G.ax, G.ay);
                cmu[pb + (long)r * G.pitch + c] = cm;
                rm[k] = cm;
            }
        }
        __syncthreads();
        const double gdt = P.gamma / dt;
#pragma unroll
        for (int i = 0; i < I1; ++i) {
            const int e = threadIdx.x + i * NTH;
            if (e >= N1) continue;
            int ly = e / W1, lxx = e - ly * W1;
            int rr = r0 - 1 + ly, cc = c0 - 1 + lxx;
            int gr = refl(rr, G.ns), gc = refl(cc, G.nf);
            int p2 = (ly + 1) * W2 + lxx + 1;
            long o = (long)gr * G.pitch + gc, ob = pb + o;
            const double us = HOIST ? vU1[i] : vU1[i] + vU0[i], wo = vW[i];
            const double wn = ((gdt - 0.5) * wo + 0.5 * us) / (gdt + 0.5);
            const double ph = sp[p2], lp = lap_at<W2>(sp, p2, G.ax, G.ay);
            const double m0 = -P.kappa * lp + (P.c1 * reglog(ph) - 2.0 * P.c2 * ph) - wn;
            const double cp = -(P.tau / dt) * ph - 0.5 * P.kappa * lp - 2.0 * P.c2 * ph - 0.5 * sm[e] - 0.5 * (wn + wo);
            sr[e] = tdt * ph - 0.5 * P.kappa * lp + P.c1 * reglog(ph) - 0.5 * m0 + cp;
            sm[e] = m0;                                                      // mu of the old level is not needed any more
            if (ly >= 1 && ly <= TY && lxx >= 1 && lxx <= TX && rr < G.ns && cc < G.nf) {   // this workgroup's own nodes
                wnew[ob] = wn;
                cphi[ob] = cp;
            }
        }
        if (HOIST && do_guess) {                                             // the hoisted operands are dead from here on
            guess_load(0);
        }
        __syncthreads();
        for (int k = 0; k < TY / 4; ++k) {
            int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
            rh[k] = 0.0;
            if (r < G.ns && c < G.nf) {
                int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
                long od = dst * slot_stride + pb + (long)r * G.pitch + c;
                const double ph = sp[p2], rp = sr[p1];
                const double rmv = ph / dt - 0.5 * lap_at<W1>(sm, p1, G.ax, G.ay) + rm[k];
                const double rhv = -rmv + lap_at<W1>(sr, p1, G.ax, G.ay);
                const double d = jac_diag(ph, tdt, P.c1);
                phi_s[od] = ph;
                if (post.part && post.hist) post.hist[b * post.hist_stride + (long)r * G.pitch + c] = ph;
                mu_s[od] = sm[p1];
                Rphi_s[od] = rp;
                D_s[od] = d;
                rh[k] = rhv;
                acc[0] += rp * rp + rmv * rmv;
                acc[2] = fmin(acc[2], d);
                acc[3] = fmax(acc[3], d);
            }
        }
    } else {
        // ---- k_residual2 ----
        const double *phi_o = phi_s + src * slot_stride + pb, *mu_o = mu_s + src * slot_stride + pb;
        const double *D_o = D_s + src * slot_stride + pb, *R_o = Rphi_s + src * slot_stride + pb;
        constexpr int N1 = (TY + 2) * W1, I1 = (N1 + NTH - 1) / NTH;      // halo-1 elements, per thread
        // phase-1 loads first (the compiler's vmcnt then waits for them only), the later phases' operands right behind
        double pd[(W2 * (TY + 4) + NTH - 1) / NTH], pp[(W2 * (TY + 4) + NTH - 1) / NTH];
        {
            int i = 0;
#pragma unroll
            for (int e = threadIdx.x; e < W2 * (TY + 4); e += NTH, ++i) {
                int ly = e / W2, lxx = e - ly * W2;
                int gr = refl(r0 - 2 + ly, G.ns), gc = refl(c0 - 2 + lxx, G.nf);
                long o = (long)gr * G.pitch + gc;
                pd[i] = dphi[pb + o];
                pp[i] = phi_o[o];
            }
        }
        double vD[I1], vR[I1], vM[I1], vC[I1], vcm[TY / 4];
#pragma unroll
        for (int i = 0; i < I1; ++i) {
            const int e = threadIdx.x + i * NTH;
            vD[i] = vR[i] = vM[i] = vC[i] = 0.0;
            if (e < N1) {
                int ly = e / W1, lxx = e - ly * W1;
                int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
                long o = (long)gr * G.pitch + gc;
                vD[i] = D_o[o];
                vR[i] = R_o[o];
                vM[i] = mu_o[o];
                vC[i] = cphi[pb + o];
            }
        }
#pragma unroll
        for (int k = 0; k < TY / 4; ++k) {
            int r = r0 + ly0 + 4 * k, c = c0 + lx;
            vcm[k] = (r < G.ns && c < G.nf) ? cmu[pb + (long)r * G.pitch + c] : 0.0;
        }
        {
            int i = 0;
#pragma unroll
            for (int e = threadIdx.x; e < W2 * (TY + 4); e += NTH, ++i) {
                sd[e] = pd[i];
                sp[e] = pp[i] + S_alpha * pd[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < I1; ++i) {
            const int e = threadIdx.x + i * NTH;
            if (e < N1) {
                int ly = e / W1, lxx = e - ly * W1;
                int p2 = (ly + 1) * W2 + lxx + 1;
                const double Dv = vD[i], Rv = vR[i], Mv = vM[i];
                const double dm = 2.0 * ((-0.5 * P.kappa * lap_at<W2>(sd, p2, G.ax, G.ay) + Dv * sd[p2]) + Rv);
                sm[e] = Mv + S_alpha * dm;
            }
        }
        __syncthreads();
        double mt[TY / 4];
        for (int k = 0; k < TY / 4; ++k) {
            int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
            rm[k] = mt[k] = 0.0;
            if (r < G.ns && c < G.nf) {
                int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
                const double cm = vcm[k];
                rm[k] = sp[p2] / dt - 0.5 * lap_at<W1>(sm, p1, G.ax, G.ay) + cm;
                mt[k] = sm[p1];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < I1; ++i) {
            const int e = threadIdx.x + i * NTH;
            if (e < N1) {
                int ly = e / W1, lxx = e - ly * W1;
                int p2 = (ly + 1) * W2 + lxx + 1;
                const double cp = vC[i];
                double ph = sp[p2];
                sm[e] = tdt * ph - 0.5 * P.kappa * lap_at<W2>(sp, p2, G.ax, G.ay) + P.c1 * reglog(ph) - 0.5 * sm[e] + cp;
                if (HOIST && do_guess) sd[e] = jac_diag(ph, tdt, P.c1);      // the guess tail's D on the tile + halo 1 (sd is free)
            }
        }
        if (HOIST && do_guess) {                                             // the prefetched operands are dead from here on
            guess_load(0);
        }
        __syncthreads();
        for (int k = 0; k < TY / 4; ++k) {
            int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
            rh[k] = 0.0;
            if (r < G.ns && c < G.nf) {
                int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
                long od = dst * slot_stride + pb + (long)r * G.pitch + c;
                double ph = sp[p2], rp = sm[p1];
                double rhv = -rm[k] + lap_at<W1>(sm, p1, G.ax, G.ay);
                double d = jac_diag(ph, tdt, P.c1);
                phi_s[od] = ph;
                mu_s[od] = mt[k];
                Rphi_s[od] = rp;
                D_s[od] = d;
                rh[k] = rhv;
                acc[0] += rp * rp + rm[k] * rm[k];
                acc[2] = fmin(acc[2], d);
                acc[3] = fmax(acc[3], d);
            }
        }
    }
    // ---- k_guess: x0 = sum c_j d_j, rhs -= A x0 (A with the D of the iterate just evaluated), sum rhs^2 before / after ----
    if (do_guess) {
        // plain form      MODE 0: X = sp (phi is not needed once D has been taken), STT = sr;  MODE 2: X = sd, STT = sp;  D in sm
        // HOIST, MODE 2   D went into sd while phi (sp) was still needed: X = sp, STT = sm
        double *X = (MODE == 0 || HOIST) ? sp : sd;                          // x0 with halo 2
        double *STT = MODE == 0 ? sr : (HOIST ? sm : sp);                    // kappa/2 M x0 + D x0 with halo 1
        const double *Dg = (MODE == 2 && HOIST) ? sd : sm;                   // D with halo 1
        if (HOIST) {
            // plane 0 is on its way since the last halo-1 pass; of every further plane the thread's elements are in flight together
            if (MODE == 0) {
                // D on the tile + halo 1 from phi, which stays in sp up to the barrier below (held in registers across the halo-1
                // and own-node passes, two or three of the five values spill at 5 workgroups per CU)
#pragma unroll
                for (int i = 0; i < GI1; ++i) {
                    const int e = threadIdx.x + i * NTH;
                    if (e < GN1) {
                        int ly = e / W1, lxx = e - ly * W1;
                        gD[i] = jac_diag(sp[(ly + 1) * W2 + lxx + 1], tdt, P.c1);
                    }
                }
            }
            double v[GI2];
#pragma unroll
            for (int i = 0; i < GI2; ++i) v[i] = gcf[0] * gT[0][i];
#pragma unroll
            for (int j = 1; j < GUESS_ORD; ++j)
                if (gcf[j] != 0.0) {
                    guess_load(j);
#pragma unroll
                    for (int i = 0; i < GI2; ++i) v[i] += gcf[j] * gT[j != 0][i];
                }
            __syncthreads();                      // everybody is done with sp / sm / sr (and sd)
            if (MODE == 0) {
#pragma unroll
                for (int i = 0; i < GI1; ++i) {
                    const int e = threadIdx.x + i * NTH;
                    if (e < GN1) sm[e] = gD[i];
                }
            }
#pragma unroll
            for (int i = 0; i < GI2; ++i) {
                const int e = threadIdx.x + i * NTH;
                if (e < GN2) X[e] = isfinite(v[i]) ? v[i] : 0.0;
            }
        } else {
            __syncthreads();                      // everybody is done with sm / sr (and sd)
            for (int e = threadIdx.x; e < (TY + 2) * W1; e += NTH) {
                int ly = e / W1, lxx = e - ly * W1;
                sm[e] = jac_diag(sp[(ly + 1) * W2 + lxx + 1], tdt, P.c1);    // D on the tile + halo 1
            }
            __syncthreads();
            for (int e = threadIdx.x; e < W2 * (TY + 4); e += NTH) {
                int ly = e / W2, lxx = e - ly * W2;
                int gr = refl(r0 - 2 + ly, G.ns), gc = refl(c0 - 2 + lxx, G.nf);
                long o = pb + (long)gr * G.pitch + gc;
                double v = gcf[0] * ga.d[0][o];
#pragma unroll
                for (int j = 1; j < GUESS_ORD; ++j)
                    if (gcf[j] != 0.0) v += gcf[j] * ga.d[j][o];
                X[e] = isfinite(v) ? v : 0.0;
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < (TY + 2) * W1; e += NTH) {             // STT is neither X nor Dg in any form
            int ly = e / W1, lxx = e - ly * W1;
            int p2 = (ly + 1) * W2 + lxx + 1;
            STT[e] = -0.5 * P.kappa * lap_at<W2>(X, p2, G.ax, G.ay) + Dg[e] * X[p2];
        }
        double xv[TY / 4];
        for (int k = 0; k < TY / 4; ++k) xv[k] = X[(ly0 + 4 * k + 2) * W2 + lx + 2];
        __syncthreads();
        const double idt = 1.0 / dt;
        for (int k = 0; k < TY / 4; ++k) {
            int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
            if (r < G.ns && c < G.nf) {
                int p1 = (ly + 1) * W1 + lx + 1;
                const double full = rh[k];
                const double defl = full - (xv[k] * idt - lap_at<W1>(STT, p1, G.ax, G.ay));
                x0[pb + (long)r * G.pitch + c] = xv[k];
                acc[4] += full * full;
                rh[k] = defl;
            }
        }
    }
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            rhs_s[dst * slot_stride + pb + (long)r * G.pitch + c] = rh[k];
            acc[1] += rh[k] * rh[k];
        }
    }
    // ---- per-workgroup partials, handed to the workgroup that finishes last ----
    {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int op5[5] = {0, 0, 1, 2, 0};
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double r_ = op5[k] == 0 ? wave_sum(acc[k]) : (op5[k] == 1 ? wave_min(acc[k]) : wave_max(acc[k]));
            if (lane == 0) sred[k * 4 + wv] = r_;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double *pp = part + ((long)b * nblk + blk) * NPART;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const double a = sred[k * 4], bb = sred[k * 4 + 1], cc = sred[k * 4 + 2], dd = sred[k * 4 + 3];
                const double v = op5[k] == 0 ? (a + bb) + (cc + dd)
                                             : (op5[k] == 1 ? fmin(fmin(a, bb), fmin(cc, dd)) : fmax(fmax(a, bb), fmax(cc, dd)));
                if (FIN_INSIDE) store_agent(pp + k, v);
                else pp[k] = v;
            }
            if (FIN_INSIDE) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const unsigned old = __hip_atomic_fetch_add(fin.counter + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_last = old == (unsigned)(nblk - 1) ? 1 : 0;
            }
        }
        if (!FIN_INSIDE) return;                  // a k_fin_residual launch follows
        __syncthreads();
        if (!s_last || threadIdx.x >= 64) return;
    }
    // ---- k_fin_residual, by the first wavefront of the last workgroup ----
    if (FIN_INSIDE) {
        double v[NPART];
        const int op[NPART] = {0, 0, 1, 2, 0, 0};
        fin_reduce_agent(part, nblk, b, v, op, do_guess ? 5 : 4);
        if (threadIdx.x != 0) return;
        __hip_atomic_store(fin.counter + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        TrajState S = st[b];
        if (MODE == 0) {
            newton_begin(S);
            S.slot = dst;                         // the evaluated start iterate lives there (a trial flips the slot when accepted)
        }
        fin_residual_update<(MODE == 0 ? 0 : 1)>(S, v, do_guess, fin.hist + (long)b * HIST_CAP, fin.kappa, dt, fin.lin_tol, fin.eta,
                                                 fin.so);
        st[b] = S;
    }
}
#define EVAL_PARAMS                                                                                                          \
    Geom G, Phys P, TrajState *st, long slot_stride, double *phi_s, double *mu_s, double *Rphi_s, double *rhs_s, double *D_s, \
        const double *dphi, double *cphi, double *cmu, double dt, double *part, const double *w, const double *un,           \
        const double *unp1, long u_stride, double *wnew, GuessArgs ga, double *x0, EvalFin fin, PostArgs post
#define EVAL_ARGS                                                                                                            \
    G, P, st, slot_stride, phi_s, mu_s, Rphi_s, rhs_s, D_s, dphi, cphi, cmu, dt, part, w, un, unp1, u_stride, wnew, ga, x0, fin, post
template <int MODE, bool FIN_INSIDE>
__global__ __launch_bounds__(NTH, EVAL_MINBLK) void k_eval(EVAL_PARAMS) {
    eval_body<MODE, FIN_INSIDE, true>(EVAL_ARGS);
}
template <int MODE, bool FIN_INSIDE>
__global__ __launch_bounds__(NTH, EVAL_MINBLK) void k_eval_plain(EVAL_PARAMS) {      // VCH_EVAL_HOIST=0
    eval_body<MODE, FIN_INSIDE, false>(EVAL_ARGS);
}
#undef EVAL_PARAMS
#undef EVAL_ARGS

// ---- CG scalar updates (one thread per trajectory does the arithmetic; fin_sum1 is above k_fin_residual) ----
// forward set-up: gamma0 = <z, z>_Z with z = P^-1 rhs (from the GEMM epilogue)
__global__ void k_fin_cg_init(TrajState *st, const double *__restrict__ gpart, int gnblk) {
    const int b = blockIdx.x;
    TrajState &S = st[b];
    if (threadIdx.x == 0) {
        S.cg_pending = 0;
        if (!S.lin_active) S.ci_active[0] = 0;
    }
    if (!S.lin_active) return;
    double g = fin_sum1(gpart, gnblk, b, 1, 0);
    if (threadIdx.x != 0) return;
    S.cg_gamma = S.cg_gamma0 = g;
    S.cg_beta = 0.0;
    S.lin_it = 0;
    S.lin_rel = 1.0;
    // (g == 0, a zero right-hand side: the first sweep still runs -- it zeroes x -- and the solve ends at its
    //  first reduction point through the breakdown branch of cg_next)
    S.ci_active[0] = S.lin_active;
    S.ci_it[0] = 0;
    S.ci_gamma[0] = g;
}

// Forward CG, the scalar step of one iteration from the three sums of its reduction point
// (see the header of the CG section).
struct CgNext {
    int active, breakdown, it;
    double alpha, beta, gamma, rel;
};
// The step every CG form shares: breakdown test, alpha, the predicted gamma' = alpha^2 <q,q> - gamma with its restart,
// beta, the iteration count and the stop test.  The forms differ in the relative residual only: rel_bd() is its value on
// breakdown, rel_step(gamma') its prediction after a step.
template <class RelBd, class RelStep>
__device__ __forceinline__ CgNext cg_step(double pq, double qq, double gamma, int it_old, double tol, int maxit, RelBd rel_bd,
                                          RelStep rel_step) {
    CgNext n;
    n.it = it_old;
    if (!(pq > 0.0) || !(gamma > 0.0)) {     // round-off level residual: stop here, no step
        n.active = 0; n.breakdown = 1; n.alpha = 0.0; n.beta = 0.0; n.gamma = fmax(gamma, 0.0); n.rel = rel_bd();
        return n;
    }
    n.breakdown = 0;
    n.alpha = gamma / pq;
    double gn = n.alpha * n.alpha * qq - gamma;
    if (gn > 1e-13 * gamma) {
        n.beta = gn / gamma;
    } else {                                  // prediction lost in cancellation: restart the direction
        gn = 1e-13 * gamma;
        n.beta = 0.0;
    }
    n.gamma = gn;
    n.it = it_old + 1;
    n.rel = rel_step(gn);
    n.active = (n.rel > tol && n.it < maxit) ? 1 : 0;
    return n;
}
__device__ __forceinline__ CgNext cg_next(double pq, double qq, double gamma, double gamma0, int it_old, double tol,
                                          int maxit) {
    return cg_step(pq, qq, gamma, it_old, tol, maxit, [&] { return gamma0 > 0.0 ? sqrt(fmax(gamma, 0.0) / gamma0) : 0.0; },
                   [&](double gn) { return sqrt(gn / gamma0); });
}

// the three sums, one wavefront each (fixed order); all threads of the workgroup call it (>= 192 threads)
__device__ __forceinline__ void cg_sums(const double *__restrict__ gpart, const double *__restrict__ gpart2, int gnblk,
                                        const double *__restrict__ part, int nblk, int pslot, int direct, int b,
                                        double *s3 /* LDS [3] */) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wv < 3) {
        const double *src = wv == 0 ? gpart : (wv == 1 ? gpart2 : part + pslot);
        const int n = wv == 2 ? nblk : gnblk, stride = wv == 2 ? NPART : 1;
        double a = 0.0;
        if (wv < 2 || direct)
            for (int t = lane; t < n; t += 64) a += src[((long)b * n + t) * stride];
        a = wave_sum(a);
        if (lane == 0) s3[wv] = a;
    }
    __syncthreads();
}

// record the step in the trajectory's state (one thread); wr = copy of the per-iteration state to write
__device__ __forceinline__ void cg_record(TrajState &S, const CgNext &n, int wr) {
    S.cg_alpha = n.alpha;
    S.cg_beta = n.beta;
    S.cg_gamma = n.gamma;
    S.lin_rel = n.rel;
    if (!n.breakdown) {
        S.lin_it = n.it;
        S.lin_total++;
    }
    if (!n.active && n.rel * S.lin_rscale > S.lin_maxrel) S.lin_maxrel = n.rel * S.lin_rscale;
    if (!n.active) S.lin_maxabs = fmax(S.lin_maxabs, n.rel * S.lin_r0);
    if (n.it > S.step_lin_max) S.step_lin_max = n.it;
    if (S.step_solves >= 1 && S.step_solves <= 4 && n.it > S.step_lin[S.step_solves - 1]) S.step_lin[S.step_solves - 1] = n.it;
    S.ci_active[wr] = n.active;
    S.ci_it[wr] = n.it;
    S.ci_gamma[wr] = n.gamma;
}

// The reduction point of the LAST enqueued iteration (the earlier ones are resolved inside the next
// k_schur_p): reads copy rd of the per-iteration state, leaves the step pending for k_cg_finish and
// publishes lin_active for the kernels and the host code outside the CG loop.
__global__ void k_fin_cg_step(TrajState *st, const double *__restrict__ gpart, const double *__restrict__ gpart2,
                              int gnblk, const double *__restrict__ part, int nblk, int pslot, int direct, int pbuf,
                              int rd, double tol, int maxit) {
    const int b = blockIdx.x;
    TrajState &S = st[b];
    __shared__ double s3[3];
    if (!S.lin_active) return;
    if (!S.ci_active[rd]) {                  // converged earlier: its last step is already in x
        if (threadIdx.x == 0) { S.lin_active = 0; S.cg_pending = 0; }
        return;
    }
    cg_sums(gpart, gpart2, gnblk, part, nblk, pslot, direct, b, s3);
    if (threadIdx.x != 0) return;
    const CgNext n = cg_next(s3[0], s3[1], direct ? s3[2] : S.ci_gamma[rd], S.cg_gamma0, S.ci_it[rd], S.lin_reltol, maxit);
    cg_record(S, n, rd ^ 1);
    S.cg_pending = n.breakdown ? 0 : 1;
    S.cg_pbuf = pbuf;
    S.lin_active = n.active;
}

// lin_active <- copy rd of the per-iteration state (before the host looks at the state inside a long solve)
__global__ void k_cg_publish(TrajState *st, int rd, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && st[b].lin_active && !st[b].ci_active[rd]) st[b].lin_active = 0;
}

// alpha = gamma / <p, q>_Z ; src 0: GEMM partials (1 value), src 1: stencil partials (slot k)
__global__ void k_fin_cg_alpha(TrajState *st, const double *__restrict__ part, int n, int stride, int k) {
    const int b = blockIdx.x;
    TrajState &S = st[b];
    if (!S.lin_active) return;
    double pq = fin_sum1(part, n, b, stride, k);
    if (threadIdx.x != 0) return;
    if (!(pq > 0.0)) {                       // breakdown (round-off level residual): stop here
        S.lin_active = 0;
        S.cg_alpha = 0.0;
        if (S.lin_rel > S.lin_maxrel) S.lin_maxrel = S.lin_rel;
        return;
    }
    S.cg_alpha = S.cg_gamma / pq;
}

// beta = gamma_new / gamma; convergence test.  mode 0 (forward): relative decrease of the
// Z-norm of the preconditioned residual; mode 1 (adjoint): ||r||_2 / ||rhs||_2 (slot k+1).
__global__ void k_fin_cg_beta(TrajState *st, const double *__restrict__ part, int nblk, int mode, double tol,
                              int maxit, int init) {
    const int b = blockIdx.x;
    TrajState &S = st[b];
    if (!S.lin_active) return;
    double gn = fin_sum1(part, nblk, b, NPART, 0);
    double rr = mode == 1 ? fin_sum1(part, nblk, b, NPART, 1) : 0.0;
    if (threadIdx.x != 0) return;
    if (init) {
        S.cg_gamma = S.cg_gamma0 = gn;
        S.cg_beta = 0.0;
        S.lin_it = 0;
    } else {
        S.cg_beta = S.cg_gamma > 0.0 ? gn / S.cg_gamma : 0.0;
        S.cg_gamma = gn;
        S.lin_it++;
        S.lin_total++;
        if (S.lin_it > S.step_lin_max) S.step_lin_max = S.lin_it;      // the host's schedule (backward_pass)
    }
    S.lin_rel = mode == 1 ? (S.lin_r0 > 0.0 ? sqrt(rr) / S.lin_r0 : 0.0)
                          : (S.cg_gamma0 > 0.0 ? sqrt(gn / S.cg_gamma0) : 0.0);
    if (!(S.lin_rel > tol) || S.lin_it >= lin_limit(S, maxit)) {
        S.lin_active = 0;
        if (S.lin_rel > S.lin_maxrel) S.lin_maxrel = S.lin_rel;
        if (S.lin_rel > tol && S.lin_cap > 0 && S.lin_it >= S.lin_cap) S.lin_capped = 1;
    }
}

// After k_dmu_ceiling: the step ceiling (F2:383-391) and the start of the Armijo loop.
// strict: a solve that the enqueued sweeps did not finish is left as it is (lin_active stays set, no trial is armed), so the
// next solve slot of the schedule -- or the host's continuation loop -- runs it again with the budget it needs.
// fin_copy >= 0 (after k_dmu_ceiling_fin): the solve's last reduction point was resolved by that kernel into copy
// fin_copy of the per-sweep state, from which lin_active is taken over here.
// cheb.enq >= 0 (after a Chebyshev solve with cheb.enq sweeps enqueued): a trajectory whose plan asked for more sweeps has
// not finished (it is left as it is, like an unfinished CG solve under `strict`); for the others the solve's books are
// closed here: sweeps done, and the relative residual the solve left, estimated as the last directly summed
// ||z_n||_Z / ||z_0||_Z (partials of k_cheb_rows) times the factor T_n / T_{n+1} the bound promises for the last step.
__global__ void k_fin_ceiling(TrajState *st, const double *__restrict__ part, int nblk, int strict, int fin_copy, ChebFin cheb) {
    const int b = blockIdx.x;
    __shared__ TrajState S;                 // the record in LDS, copied in and out by the whole wavefront (see k_fin_residual)
    traj_copy_in(S, st + b);
    if (!S.newton_active || S.need_trial) return;
    if ((cheb.enq >= 0) != (S.use_cheb != 0)) return;      // the other form's launch sequence looks after this trajectory
    int lin_active = S.lin_active;          // (a value every lane keeps: the record itself is advanced by lane 0 only)
    if (cheb.enq >= 0 && lin_active) {
        if (S.cheb_n > cheb.enq) return;    // unfinished: taken up again by the next solve slot / the host's loop
        const double rel = cheb_solve_rel(S.cheb_n, cheb, b);
        if (threadIdx.x == 0) cheb_close_books(S, rel);
        lin_active = 0;
    }
    if (fin_copy >= 0 && lin_active) {
        lin_active = fin_copy == 0 ? S.ci_active[0] : S.ci_active[1];
        if (strict && lin_active) {         // unfinished: only the flag goes back
            if (threadIdx.x == 0) st[b].lin_active = lin_active;
            return;
        }
    }
    if (strict && lin_active) return;
    double v[NPART];
    const int op[NPART] = {1, 0, 0, 0, 0, 0};
    if (cheb.enq >= 0 && cheb.cmin) {
        double a = 1e300;
        for (int t = threadIdx.x; t < cheb.gnblk; t += 64) a = fmin(a, cheb.cmin[(long)b * cheb.gnblk + t]);
        v[0] = wave_min(a);
    } else {
        fin_reduce(part, nblk, b, v, op, 1);
    }
    if (threadIdx.x == 0) ceiling_arm(S, v[0], lin_active);
    traj_copy_out(st + b, S);
}

__global__ void k_fin_mass(TrajState *st, const double *__restrict__ part, int nblk, int init) {
    const int b = blockIdx.x;
    TrajState &S = st[b];
    if (S.frozen) return;
    double v[NPART];
    const int op[NPART] = {0, 0, 0, 0, 0, 0};
    fin_reduce(part, nblk, b, v, op, 2);
    if (threadIdx.x != 0) return;
    if (init) {
        S.mass0 = v[0];
        S.mass_err = 0.0;
    } else {
        S.mass_err = v[0] - S.mass0;
    }
    S.Wint = v[1];
}

// Linear-solve setup outside the Newton loop.
//   mode 0: partial slots {min D, max D, sum rhs^2}, adjoint operator A(phi_n)  (B2:198)
//   mode 1: partial slot  {sum rhs^2}, constant-coefficient operator (D = 0)     (B2:184)
//   mode 2: partial slots {sum(.), sum rhs^2, min D, max D}, forward Schur operator
//           scale_ratio > 0: Dmax > scale_ratio * Dmin takes the right-scaled CG form (cg_weight), as in the march
__global__ void k_fin_lin_begin(TrajState *st, const double *__restrict__ part, int nblk, int mode,
                                double tau, double kappa, double dt, double lin_tol, double scale_ratio) {
    const int b = blockIdx.x;
    TrajState &S = st[b];
    if (threadIdx.x == 0 && (S.lin_active || S.lin_capped)) {      // the previous solve of this trajectory ended on its sweep budget
        S.lin_unconv++;
        if (S.lin_rel > S.lin_maxrel) S.lin_maxrel = S.lin_rel;
    }
    double v[NPART];
    const int op0[NPART] = {1, 2, 0, 0, 0, 0};
    const int op1[NPART] = {0, 0, 0, 0, 0, 0};
    const int op2[NPART] = {0, 0, 1, 2, 0, 0};
    if (mode == 0) fin_reduce(part, nblk, b, v, op0, 3);
    else if (mode == 1) fin_reduce(part, nblk, b, v, op1, 1);
    else fin_reduce(part, nblk, b, v, op2, 4);
    if (threadIdx.x != 0) return;
    double dmin = 0.0, dmax = 0.0, r0;
    if (mode == 0) { dmin = v[0]; dmax = v[1]; r0 = sqrt(v[2]); }
    else if (mode == 1) { r0 = sqrt(v[0]); }
    else { dmin = v[2]; dmax = v[3]; r0 = sqrt(v[1]); }
    S.Dmin = dmin;
    S.Dmax = dmax;
    if (mode == 2) cg_setup(S, 2.0 * sqrt(0.5 * kappa / dt), 1.0, lin_tol);
    else cg_setup(S, tau + 2.0 * sqrt(0.5 * dt), 0.5 * dt, lin_tol);
    S.lin_r0 = r0;
    S.lin_active = (mode == 2 || r0 > 0.0) ? 1 : 0;
    S.lin_capped = 0;
    S.lin_it = 0;
    S.lin_prev = 1e300;
    S.lin_rel = 1.0;
    S.lin_reltol = lin_tol;
    S.use_cheb = 0;
    // mode 2, on request: the rule of the march's CG-form solves (fin_residual_update)
    S.scaled = (mode == 2 && scale_ratio > 0.0 && dmax > scale_ratio * dmin) ? 1 : 0;
    S.nsolves++;
}

// ---------------------------------------------------------------------------------
// Set-up kernels of the stand-alone linear-solve entry points (kernel-level parity tests).
// ---------------------------------------------------------------------------------
// J [dphi;dmu] = [a;b]  ->  Schur form: R_phi := -a, rhs := b - L a, D from phi (slot 0).
__global__ __launch_bounds__(NTH) void k_solve_setup(Geom G, Phys P, const double *__restrict__ a,
                                                     const double *__restrict__ bv, const double *__restrict__ phi,
                                                     double dt, double *__restrict__ Rphi, double *__restrict__ rhs,
                                                     double *__restrict__ D, double *__restrict__ part) {
    TILE_COORDS;
    __shared__ double s[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    constexpr int W = TX + 2;
    const long pb = b * G.plane;
    load_tile<1>(s, a + pb, G, c0, r0);
    __syncthreads();
    double acc[4] = {0.0, 0.0, 1e300, -1e300};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p = (ly + 1) * W + lx + 1;
            long o = pb + (long)r * G.pitch + c;
            double rh = bv[o] - lap_at<W>(s, p, G.ax, G.ay);
            double d = jac_diag(phi[o], P.tau / dt, P.c1);
            Rphi[o] = -s[p];
            rhs[o] = rh;
            D[o] = d;
            acc[1] += rh * rh;
            acc[2] = fmin(acc[2], d);
            acc[3] = fmax(acc[3], d);
        }
    }
    const int op[4] = {0, 0, 1, 2};
    block_reduce_store<4>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// D = f''(phi) (or 0 when phi == NULL) and sum rhs^2, min/max D: slots {min D, max D, sum rhs^2}
__global__ __launch_bounds__(NTH) void k_adj_setup(Geom G, Phys P, const double *__restrict__ phi,
                                                   const double *__restrict__ rhs, double *__restrict__ Dn,
                                                   double *__restrict__ part) {
    TILE_COORDS;
    __shared__ double sred[NPART * 4];
    double acc[3] = {1e300, -1e300, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            long o = b * G.plane + (long)r * G.pitch + c;
            double d = phi ? fpp_log(phi[o], P.c1, P.c2) : 0.0;
            Dn[o] = d;
            acc[0] = fmin(acc[0], d);
            acc[1] = fmax(acc[1], d);
            if (rhs) acc[2] += rhs[o] * rhs[o];
        }
    }
    const int op[3] = {1, 2, 0};
    block_reduce_store<3>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

__global__ __launch_bounds__(NTH) void k_solve_w(Geom G, const double *__restrict__ w, const double *__restrict__ un,
                                                 const double *__restrict__ unp1, double gdt, double *__restrict__ out) {
    TILE_COORDS;
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            long o = b * G.plane + (long)r * G.pitch + c;
            double u0 = un ? un[o] : 0.0, u1 = unp1 ? unp1[o] : 0.0;
            out[o] = ((gdt - 0.5) * w[o] + 0.5 * (u1 + u0)) / (gdt + 0.5);
        }
    }
}

// Adjoint sweep, starting guess of the solve for p_n (the solve starts from the content of x): x holds p_{n+1}; it is
// saved into the ring slot `keep` and replaced by c_0 p_{n+1} + sum_{j>=1} c_j p_{n+1+j} over levels the ring holds.
// Crank-Nicolson does not damp the highest modes (amplification -> -1), so p carries a component that alternates from
// level to level and dominates the residual of a guess: p_{n+1} itself leaves ||rhs - A x0|| = 2 ||rhs||, p_{n+2} leaves
// 1e-3 and the extrapolation over levels of the SAME parity, n+2, n+4, ..., 5e-6 and below (scripts/r2_extrap_adj.py).
// backward_pass therefore sets c_0 = 0 and weights on j = 1, 3, 5, 7.
// BATCH (the default; VCH_LOADS_BATCH=0 launches k_adj_guess_plain): the tests on the coefficients are uniform over the
// trajectory, so x and every plane with a coefficient are requested for the thread's TY / 4 nodes before the first use; v is
// then formed in the same order with the same test in front of each term.
template <bool BATCH>
__device__ __forceinline__ void adj_guess_body(const Geom &G, double *__restrict__ x, const GuessArgs &ga, double *__restrict__ keep) {
    TILE_COORDS;
    constexpr int K = TY / 4;
    double vx[K], vd[K][GUESS_ORD];
    double cf[GUESS_ORD];          // BATCH: the trajectory's coefficients and the planes' addresses, read once
    const double *dp[GUESS_ORD];
    if (BATCH) {
        const double *gcf = ga.row(b);
#pragma unroll
        for (int j = 0; j < GUESS_ORD; ++j) {
            cf[j] = gcf[j];
            dp[j] = ga.d[j];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            int r = r0 + ly0 + 4 * k, c = c0 + lx;
            const bool in = r < G.ns && c < G.nf;
            const long o = b * G.plane + (long)r * G.pitch + c;
            vx[k] = in ? x[o] : 0.0;
#pragma unroll
            for (int j = 1; j < GUESS_ORD; ++j) {
                vd[k][j] = 0.0;
                if (in && cf[j] != 0.0) vd[k][j] = dp[j][o];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            const long o = b * G.plane + (long)r * G.pitch + c;
            const double p1 = BATCH ? vx[k] : x[o];
            const double *gcf = BATCH ? cf : ga.row(b);
            double v = gcf[0] * p1;
#pragma unroll
            for (int j = 1; j < GUESS_ORD; ++j)
                if (gcf[j] != 0.0) v += gcf[j] * (BATCH ? vd[k][j] : ga.d[j][o]);
            keep[o] = p1;
            x[o] = isfinite(v) ? v : p1;
        }
    }
}
__global__ __launch_bounds__(NTH) void k_adj_guess(Geom G, double *__restrict__ x, GuessArgs ga, double *__restrict__ keep) {
    adj_guess_body<true>(G, x, ga, keep);
}
__global__ __launch_bounds__(NTH) void k_adj_guess_plain(Geom G, double *__restrict__ x, GuessArgs ga, double *__restrict__ keep) {
    adj_guess_body<false>(G, x, ga, keep);
}

// the longest solve since the host's last look (adjoint launch schedule)
__global__ void k_reset_longest(TrajState *st, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) st[b].step_lin_max = 0;
}

// The sweep caps of the adjoint launch schedule, written at the host's look (batches of at most GUESS_BMAX): the solves of
// trajectory b stop after cap[b] sweeps (0 = no cap), whatever the host enqueues for its batch mates.  reset: the longest
// solve counts from this look on.  One workgroup per trajectory: the table is indexed by a wave-uniform value.
struct AdjCaps {
    int cap[GUESS_BMAX];
};
__global__ void k_adj_caps(TrajState *st, AdjCaps caps, int reset) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    st[b].lin_cap = b < GUESS_BMAX ? caps.cap[b] : 0;
    if (reset) st[b].step_lin_max = 0;
}

// zero-fill / constant fill of valid nodes
__global__ __launch_bounds__(NTH) void k_fill(Geom G, double *__restrict__ x, double v) {
    TILE_COORDS;
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) x[b * G.plane + (long)r * G.pitch + c] = v;
    }
}

// phi_Q[lvl] = (1 - t_lvl/T) phi_0 + (t_lvl/T) phi_T  (build_targets choice_q = 1, G2:221-222)
// grid = (tiles, levels, B)
__global__ __launch_bounds__(NTH) void k_ramp(Geom G, int tiles_f, const double *__restrict__ phi0,
                                              const double *__restrict__ phiT, const double *__restrict__ tfrac,
                                              long hist_stride, double *__restrict__ pq) {
    const int b = blockIdx.z, lvl = blockIdx.y;
    const int c0 = (blockIdx.x % tiles_f) * TX, r0 = (blockIdx.x / tiles_f) * TY;
    const int lx = threadIdx.x & 63, ly0 = threadIdx.x >> 6;
    const double tp = tfrac[lvl];
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            long o = (long)r * G.pitch + c;
            pq[b * hist_stride + (long)lvl * G.plane + o] = (1 - tp) * phi0[b * G.plane + o] + tp * phiT[b * G.plane + o];
        }
    }
}


// =================================================================================
// Conjugate gradients on the preconditioned Schur / adjoint systems.
//
// Forward (left preconditioning):  T = P^-1 A,  A = I/dt + M (kappa/2 M + D) = P + M Delta,
//   Delta = D - dbar > 0.  T is self-adjoint and positive in <x, y>_Z = sum W Delta x y, so
//   plain CG applies with z = P^-1 (rhs - A x) as residual.  One reduction point per iteration:
//       [k_schur_p]   x += alpha p; z' = z - alpha q; p' = z' + beta p; v = A p'; gamma = <z',z'>_Z
//       [3 DCT passes] q' = P^-1 v with <p',q'>_Z and <q',q'>_Z
//       [start of the next k_schur_p] alpha' = gamma / <p',q'>;  gamma' ~ alpha'^2 <q',q'> - gamma  (the value
//                     <z'',z''>_Z will take, by conjugacy);  beta' = gamma'/gamma;  stop test on gamma'
//   gamma itself is always the directly summed <z',z'>_Z of the previous line; the predicted
//   gamma' only steers beta and the stop test, and a prediction lost in cancellation
//   (gamma' < 1e-13 gamma) restarts the direction (beta = 0) instead.
// Adjoint (right preconditioning): A P^-1 is self-adjoint in <x, y>_Z' = sum W x y / Delta:
//       pv = P^-1 ph; q = A pv; alpha = <r,r>_Z' / <ph,q>_Z'; x += alpha pv; r -= alpha q;
//       beta = <r',r'>_Z' / <r,r>_Z'; ph = r' + beta ph.
// =================================================================================

// Iteration k of the forward CG (it = k; FIRST: k = 0, p_new = z, v = A p_new).  For k >= 1 every
// workgroup first resolves the reduction point of iteration k-1 from its partial sums (gpart/gpart2 from
// the preconditioner epilogue, part[., (k-1)&1] from the previous launch of this kernel) -- the same
// arithmetic on the same numbers in every workgroup; the workgroup with blk == 0 records the result --
// and then applies that step on the way:
//   x += alpha p_old; z_new = z - alpha q; p_new = z_new + beta p_old (z_new and p_new recomputed on
//   the halo, z_new written to its own buffer so that neighbours still read z), v = A p_new, and the
//   partial of <z_new, z_new>_Z goes to part[., k&1].  A trajectory that the step brings below the
//   tolerance only takes the step (x += alpha p_old).
template <int FIRST>
__global__ __launch_bounds__(NTH) void k_schur_p(Geom G, Phys P, TrajState *__restrict__ st,
                                                 long slot_stride, const double *__restrict__ z,
                                                 const double *__restrict__ q, const double *__restrict__ p_old,
                                                 const double *__restrict__ D_s, double dt,
                                                 double *__restrict__ x, double *__restrict__ z_new,
                                                 double *__restrict__ p_new, double *__restrict__ v,
                                                 double *__restrict__ part, const double *__restrict__ gpart,
                                                 const double *__restrict__ gpart2, int gnblk, int it, double tol,
                                                 int maxit) {
    TILE_COORDS;
    __shared__ double sx[(TY + 4) * (TX + 4)];
    __shared__ double stt[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    constexpr int W2 = TX + 4, W1 = TX + 2;
    const long pb = b * G.plane;
    const int rd = (it + 1) & 1, wr = it & 1;          // per-iteration state copies / partial slots
    const int slot = st[b].slot;
    const double dbar = st[b].dbar;
    double alpha = 0.0, beta = 0.0;
    if (FIRST) {
        if (!st[b].ci_active[0]) return;
        load_tile<2>(sx, z + pb, G, c0, r0);
    } else {
        const int was_active = st[b].ci_active[rd];
        if (!was_active) {
            if (blk == 0 && threadIdx.x == 0) {           // hand the (finished) state on to the other copy
                st[b].ci_active[wr] = 0;
                st[b].ci_it[wr] = st[b].ci_it[rd];
                st[b].ci_gamma[wr] = st[b].ci_gamma[rd];
            }
            return;
        }
        const double gamma0 = st[b].cg_gamma0, gamma_old = st[b].ci_gamma[rd];
        const int it_old = st[b].ci_it[rd];
        cg_sums(gpart, gpart2, gnblk, part, nblk, rd, it >= 2, b, sred);
        const CgNext n = cg_next(sred[0], sred[1], it >= 2 ? sred[2] : gamma_old, gamma0, it_old, st[b].lin_reltol, maxit);
        __syncthreads();                                   // sred is reused below
        if (blk == 0 && threadIdx.x == 0) cg_record(st[b], n, wr);
        alpha = n.alpha;
        beta = n.beta;
        if (!n.active) {                                   // converged (or broke down, alpha = 0): take the step only
            if (!n.breakdown)
                for (int k = 0; k < TY / 4; ++k) {
                    int r = r0 + ly0 + 4 * k, c = c0 + lx;
                    if (r < G.ns && c < G.nf) {
                        long o = pb + (long)r * G.pitch + c;
                        x[o] += alpha * p_old[o];
                    }
                }
            return;
        }
        for (int e = threadIdx.x; e < W2 * (TY + 4); e += NTH) {
            int ly = e / W2, lxx = e - ly * W2;
            int gr = refl(r0 - 2 + ly, G.ns), gc = refl(c0 - 2 + lxx, G.nf);
            long o = pb + (long)gr * G.pitch + gc;
            sx[e] = (z[o] - alpha * q[o]) + beta * p_old[o];
        }
    }
    __syncthreads();
    const double *Dp = D_s + slot * slot_stride + pb;
    for (int e = threadIdx.x; e < (TY + 2) * W1; e += NTH) {
        int ly = e / W1, lxx = e - ly * W1;
        int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
        int p2 = (ly + 1) * W2 + lxx + 1;
        stt[e] = -0.5 * P.kappa * lap_at<W2>(sx, p2, G.ax, G.ay) + Dp[(long)gr * G.pitch + gc] * sx[p2];
    }
    __syncthreads();
    const double idt = 1.0 / dt;
    double acc[1] = {0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
            long o = pb + (long)r * G.pitch + c;
            if (!FIRST) {
                double po = p_old[o];
                double zn = z[o] - alpha * q[o];
                x[o] += alpha * po;
                z_new[o] = zn;
                acc[0] += wdev(r, c, G) * (Dp[(long)r * G.pitch + c] - dbar) * (zn * zn);
            } else {
                x[o] = 0.0;          // start of a solve (only for the trajectories that take part in it)
            }
            p_new[o] = sx[p2];
            v[o] = sx[p2] * idt - lap_at<W1>(stt, p1, G.ax, G.ay);
        }
    }
    if (!FIRST) {
        const int op[1] = {0};
        block_reduce_store<1>(acc, op, sred, part + ((long)b * nblk + blk) * NPART + wr);
    }
}

// End of a forward CG solve: add the step that is still pending, x += alpha p[cg_pbuf].
__global__ __launch_bounds__(NTH) void k_cg_finish(Geom G, const TrajState *__restrict__ st,
                                                   const double *__restrict__ p0, const double *__restrict__ p1,
                                                   double *__restrict__ x) {
    TILE_COORDS;
    const TrajState S = st[b];
    if (!S.cg_pending) return;
    const double *p = S.cg_pbuf ? p1 : p0;
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            long o = b * G.plane + (long)r * G.pitch + c;
            x[o] += S.cg_alpha * p[o];
        }
    }
}

// ph = r + beta ph (FIRST: ph = r)
template <int FIRST>
__global__ __launch_bounds__(NTH) void k_cg_dir(Geom G, const TrajState *__restrict__ st,
                                                const double *__restrict__ r, double *__restrict__ ph) {
    TILE_COORDS;
    const TrajState S = st[b];
    if (!S.lin_active) return;
    for (int k = 0; k < TY / 4; ++k) {
        int rr = r0 + ly0 + 4 * k, c = c0 + lx;
        if (rr < G.ns && c < G.nf) {
            long o = b * G.plane + (long)rr * G.pitch + c;
            ph[o] = FIRST ? r[o] : r[o] + S.cg_beta * ph[o];
        }
    }
}

// q = A(phi_n) pv with partial sum W ph q / (D_n - dbar)
__global__ __launch_bounds__(NTH) void k_adj_q(Geom G, Phys P, const TrajState *__restrict__ st,
                                               const double *__restrict__ pv, const double *__restrict__ Dn,
                                               const double *__restrict__ ph, double dt, double *__restrict__ q,
                                               double *__restrict__ part) {
    TILE_COORDS;
    const TrajState S = st[b];
    if (!S.lin_active) return;
    __shared__ double sx[(TY + 4) * (TX + 4)];
    __shared__ double stt[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    constexpr int W2 = TX + 4, W1 = TX + 2;
    const long pb = b * G.plane;
    load_tile<2>(sx, pv + pb, G, c0, r0);
    __syncthreads();
    for (int e = threadIdx.x; e < (TY + 2) * W1; e += NTH) {
        int ly = e / W1, lxx = e - ly * W1;
        stt[e] = -lap_at<W2>(sx, (ly + 1) * W2 + lxx + 1, G.ax, G.ay);
    }
    __syncthreads();
    double acc[1] = {0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            int p1 = (ly + 1) * W1 + lx + 1, p2 = (ly + 2) * W2 + lx + 2;
            long o = pb + (long)r * G.pitch + c;
            double d = Dn[o];
            double qv = sx[p2] + (P.tau + 0.5 * dt * d) * stt[p1] - 0.5 * dt * lap_at<W1>(stt, p1, G.ax, G.ay);
            q[o] = qv;
            acc[0] += wdev(r, c, G) / (d - S.dbar) * (ph[o] * qv);
        }
    }
    const int op[1] = {0};
    block_reduce_store<1>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// x += alpha pv; r -= alpha q; partials: sum W r^2/(D_n - dbar), sum r^2
__global__ __launch_bounds__(NTH) void k_cg_update_adj(Geom G, const TrajState *__restrict__ st,
                                                       const double *__restrict__ pv, const double *__restrict__ q,
                                                       const double *__restrict__ Dn, double *__restrict__ x,
                                                       double *__restrict__ r, double *__restrict__ part) {
    TILE_COORDS;
    const TrajState S = st[b];
    if (!S.lin_active) return;
    __shared__ double sred[NPART * 4];
    double acc[2] = {0.0, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int rr = r0 + ly0 + 4 * k, c = c0 + lx;
        if (rr < G.ns && c < G.nf) {
            long o = b * G.plane + (long)rr * G.pitch + c;
            x[o] += S.cg_alpha * pv[o];
            double rn = r[o] - S.cg_alpha * q[o];
            r[o] = rn;
            acc[0] += wdev(rr, c, G) / (Dn[o] - S.dbar) * (rn * rn);
            acc[1] += rn * rn;
        }
    }
    const int op[2] = {0, 0};
    block_reduce_store<2>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// ---------------------------------------------------------------------------------
// Tangent (linearised) march of vch2d_second_order: J'(u)h and J''(u)[h,h] about the resident control and state history.
//
// With delta-phi_0 = delta-mu_0 = delta-w_0 = 0 and the second-order fields delta2-phi_0 = delta2-mu_0 = 0, step n is
//   dw'  = ((gamma/dt - 1/2) dw + 1/2 (h_{n+1} + h_n)) / (gamma/dt + 1/2)                              (the solve_w rule)
//   J(phi*) [dphi*; dmu']   = [ tau dphi/dt + kappa/2 L dphi + 2 c2 dphi + 1/2 dmu + 1/2 (dw' + dw) ;  dphi/dt + 1/2 L dmu ]
//   J(phi*) [d2phi*; d2mu'] = [ tau d2phi/dt + kappa/2 L d2phi + 2 c2 d2phi + 1/2 d2mu - c1 rho(phi*) (dphi*)^2 ;
//                               d2phi/dt + 1/2 L d2mu ],             rho(p) = 4 p / (1 - p^2)^2 = reglog''(p)
//   dphi' = dphi* - sum(wts dphi*) / W_int,   d2phi' = d2phi* - sum(wts d2phi*) / W_int            (on the fix's set I_n only)
// phi* is the Newton solution of the step before the march's mass fix subtracted s_n ON ITS SET I_n (the interior nodes, or
// every node in the all-node form): phi* = phi_{n+1} + s_n on I_n and phi_{n+1} elsewhere; s_n and the weight W_int the fix
// divided by come from the shift record the march keeps beside its history (PostFix::record).  J = the Newton matrix of
// k_jac_apply at phi*: one linear solve per field
// and step, by the Schur reduction + preconditioned CG of the Newton solves (k_fin_lin_begin -> schur_solve -> dmu_ceiling).
// The mass fix is linearised, not taken as the identity: the linearised step conserves the mass of dphi in the weights of
// the Laplacian (its Kronecker-order quirk), which are the fix's weights wts = hx hy outer(trapz_x, trapz_y) only for
// Nx == Ny.  The weighted mean leaves the nodes of I_n, as the shift did; where the march did not apply the fix (s_n == 0)
// nothing is subtracted; dmu' and dw' are carried as they are.
// I_n is not kept by the march and is NOT recoverable from phi_{n+1} and s_n in general: the sweeps classify a node as
// interior where |phi_{n+1} + s_n| < 1 - delta_sep - 5e-3, which every interior node passes, and so does a skipped node that
// lies within |s_n| of the threshold with s_n pointing inward.  In exact arithmetic misclassification can only add weight
// (in floating point (phi_c - s) + s may also round an interior node one ulp under the threshold up to it, which takes
// weight away), so the classified weight (k_tan_mass slot 1, k_hv_emit acc[1]) equals the recorded W_int when every node is
// classified right: where the two differ by more than round-off, in either direction (TanFix::unrecoverable; one node
// changes the sum by at least hx hy / 4) the step is marked in the
// context's refusal cells and the call returns an error instead of a wrong derivative.  So nodes outside the interior band
// are linearised exactly or refused.  The clip is inactive wherever |phi| < 1 - delta_sep; an ACTIVE CLIP IS STILL NOT
// DETECTED.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ double tan_rho(double phi) {      // reglog''(p), p clipped to the band of jac_diag
    const double lim = sqrt(1.0 - DELTA_SEP * DELTA_SEP);
    const double p = fmin(fmax(phi, -lim), lim), q = 1.0 - p * p;
    return 4.0 * p / (q * q);
}

// The set the mass fix of a step shifted, as far as the history tells: phi1 = the stored level (after the fix), s = the
// step's shift, all = the all-node form.  s == 0 (no fix): phi* = phi1 whatever the answer.
__device__ __forceinline__ bool fix_in_set(double phi1, double s, bool all) {
    return all || fabs(phi1 + s) < (1.0 - DELTA_SEP) - 5e-3;
}
__device__ __forceinline__ double fix_phi_star(double phi1, double s, bool all) { return fix_in_set(phi1, s, all) ? phi1 + s : phi1; }
__device__ __forceinline__ bool fix_all(const double *rec) { return rec && rec[1] == 0.0; }

// The linearised mass fix of one solve's output x: sums = {sum wts x, classified interior weight} (k_tan_mass's partials
// through post_sums, read only where the step has a shift), rec = the step's cell of the shift record {s_n, W_int}.
struct TanFix {
    double mean, shift, w_rec;
    bool all;
    __device__ __forceinline__ TanFix(const double *sums, const double *rec, double LxLy) {
        shift = rec ? rec[0] : 0.0;
        w_rec = rec ? rec[1] : 1.0;
        all = fix_all(rec);                      // the march fell back to the all-node form (no interior node)
        mean = shift != 0.0 ? sums[0] / (all ? LxLy : w_rec) : 0.0;
    }
    __device__ __forceinline__ double apply(double v, double phi1) const {
        return fix_in_set(phi1, shift, all) ? v - mean : v;
    }
    // The classified weight is not the weight the march divided by.  Above it: a skipped node passes for an interior one.
    // Below it, in exact arithmetic impossible (an interior node has |phi_c| < thr and phi1 + s = phi_c), in floating point
    // possible where (phi_c - s) + s rounds up to the threshold for an interior node one ulp under it: then the node is
    // taken for a skipped one.  Either way the set is not the march's, so the check is two-sided.
    __device__ __forceinline__ bool unrecoverable(const double *sums, double wtol) const {
        return shift != 0.0 && !all && fabs(sums[1] - w_rec) > w_rec * wtol;
    }
};
// Refusal cells of a call, one int per trajectory: the first step whose interior set is not recoverable, -1 = none.  Written
// by one lane of one workgroup per trajectory in the kernels that have just reduced the sums (no per-node pass of its own).
struct FixCheck {
    int *bad;           // [B]
    int step;
    double wtol;        // round-off allowance of the weight comparison: nodes x eps
    __device__ __forceinline__ void look(const TanFix &tf, const double *sums, long b, int blk) const {
        if (blk == 0 && threadIdx.x == 0 && tf.unrecoverable(sums, wtol) && (bad[b] < 0 || step < bad[b])) bad[b] = step;
    }
};

// Workgroup partials {sum wts x, sum of wts over the interior nodes of phi* = phi1 + s} of a solve's output x, in the slots
// post_sums reads; a trajectory whose step has no shift is left out (its consumers do not read the sums).
__global__ __launch_bounds__(NTH) void k_tan_mass(Geom G, const double *__restrict__ x, const double *__restrict__ phi1,
                                                  long hist_stride, const double *__restrict__ rec, long rec_stride,
                                                  const double *__restrict__ wts, double *__restrict__ part) {
    TILE_COORDS;
    __shared__ double sred[NPART * 4];
    const double s = rec[b * rec_stride];
    if (s == 0.0) return;
    const bool all = fix_all(rec + b * rec_stride);
    const long pb = b * G.plane, hb = b * hist_stride;
    double acc[2] = {0.0, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            const long o = (long)r * G.pitch + c;
            const double w = wts[o];
            acc[0] += w * x[pb + o];
            if (fix_in_set(phi1[hb + o], s, all)) acc[1] += w;
        }
    }
    const int op[2] = {0, 0};
    block_reduce_store<2>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

struct TanRhsArgs {
    const double *a, *m;            // [B][plane] dphi, dmu of level n (SECOND: d2phi, d2mu)
    const double *w_in;             // first order: dw of level n ...
    double *w_out;                  // ... and where dw' goes (another plane: neighbours read w_in on their halo)
    const double *hn, *hp;          // first order: rows n, n+1 of the direction (history layout), NULL = zeros (F2:545-548)
    const double *phi1;             // level n+1 of the state history
    long hist_stride;               // trajectory stride of hn, hp, phi1
    const double *d1, *m1;          // SECOND: this step's finished dphi', dmu' (the solver's output planes) ...
    double *keep_phi, *keep_mu;     // ... and the planes that keep them while the second solve reuses the solver's
    const double *rec;              // this step's cell of the shift record ([B] cells rec_stride apart), NULL = no shifts
    long rec_stride;
    const double *mpart;            // SECOND: k_tan_mass's partials of d1 (keep_phi gets d1 with the fix's mean taken out)
};

// Right-hand side of a tangent solve in the form k_solve_setup leaves: with [A; Bv] the right-hand side above,
// R_phi := -A, rhs := Bv - L A (Schur), D from phi_{n+1}, partials {-, sum rhs^2, min D, max D} for k_fin_lin_begin (mode 2).
// A is evaluated on the tile and its one-node halo (from dphi with a two-node halo), so that L A needs no second launch.
// D and rho are taken at phi* (fix_phi_star).
template <int SECOND>
__global__ __launch_bounds__(NTH) void k_tan_rhs(Geom G, Phys P, TanRhsArgs a, double dt, double *__restrict__ Rphi,
                                                 double *__restrict__ rhs, double *__restrict__ D, double *__restrict__ part) {
    TILE_COORDS;
    __shared__ double sa[(TY + 4) * (TX + 4)];
    __shared__ double sm[(TY + 2) * (TX + 2)];
    __shared__ double sr[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    __shared__ double s_fix[2];
    constexpr int W2 = TX + 4, W = TX + 2;
    const long pb = b * G.plane, hb = b * a.hist_stride;
    const double *rec = a.rec ? a.rec + b * a.rec_stride : (const double *)nullptr;
    const double shift = rec ? rec[0] : 0.0;
    const bool all = fix_all(rec);
    load_tile<2>(sa, a.a + pb, G, c0, r0);
    load_tile<1>(sm, a.m + pb, G, c0, r0);
    if (SECOND && shift != 0.0) post_sums(a.mpart, nblk, (int)b, s_fix);
    __syncthreads();
    const TanFix tf(s_fix, SECOND ? rec : (const double *)nullptr, P.LxLy);
    const double gdt = P.gamma / dt;
    auto w_new = [&](long o, double w0) {
        const double h0 = a.hn ? a.hn[hb + o] : 0.0, h1 = a.hp ? a.hp[hb + o] : 0.0;
        return ((gdt - 0.5) * w0 + 0.5 * (h1 + h0)) / (gdt + 0.5);
    };
    for (int e = threadIdx.x; e < W * (TY + 2); e += NTH) {
        const int ly = e / W, lxx = e - ly * W;
        const int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
        const long o = (long)gr * G.pitch + gc;
        const int p2 = (ly + 1) * W2 + lxx + 1;
        const double av = sa[p2];
        double v = P.tau * av / dt + 0.5 * P.kappa * lap_at<W2>(sa, p2, G.ax, G.ay) + 2.0 * P.c2 * av + 0.5 * sm[e];
        if (SECOND) {
            const double d = a.d1[pb + o];
            v -= P.c1 * tan_rho(fix_phi_star(a.phi1[hb + o], shift, all)) * (d * d);
        } else {
            const double w0 = a.w_in[pb + o];
            v += 0.5 * (w_new(o, w0) + w0);
        }
        sr[e] = v;
    }
    __syncthreads();
    double acc[4] = {0.0, 0.0, 1e300, -1e300};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            const int p = (ly + 1) * W + lx + 1;
            const long o = (long)r * G.pitch + c;
            const double rm = sa[(ly + 2) * W2 + lx + 2] / dt + 0.5 * lap_at<W>(sm, p, G.ax, G.ay);
            const double rh = rm - lap_at<W>(sr, p, G.ax, G.ay);
            const double p1 = a.phi1[hb + o];
            const double d = jac_diag(fix_phi_star(p1, shift, all), P.tau / dt, P.c1);
            Rphi[pb + o] = -sr[p];
            rhs[pb + o] = rh;
            D[pb + o] = d;
            if (SECOND) {
                a.keep_phi[pb + o] = tf.apply(a.d1[pb + o], p1);
                a.keep_mu[pb + o] = a.m1[pb + o];
            } else {
                a.w_out[pb + o] = w_new(o, a.w_in[pb + o]);
            }
            acc[1] += rh * rh;
            acc[2] = fmin(acc[2], d);
            acc[3] = fmax(acc[3], d);
        }
    }
    const int op[4] = {0, 0, 1, 2};
    block_reduce_store<4>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// The stand-alone solve sequence outside a Newton loop: after k_fin_lin_begin, the record is put into the phase the back
// substitution (k_dmu_ceiling / k_dmu_ceiling_fin, k_fin_ceiling) expects -- Newton running, no trial pending.  The trial
// those kernels arm and the step ceiling they take are never consumed: the next solve's k_tan_arm clears them.
__global__ void k_tan_arm(TrajState *st, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    st[b].newton_active = 1;
    st[b].need_trial = 0;
    st[b].x_primed = 0;
    st[b].lin_rscale = 1.0;
}

// Integrands of one level, weighted with W_cost (nested trapezoid rule in y, x), per workgroup:
//   {W e dphi, W dphi^2, W e d2phi, W u h, W h^2, W eT dphi, W eT d2phi, 0},  e = phi - phi_Q, eT = phi_M - phi_T (last level only)
// and the hand-over of the level's fields from the solver's output planes to the planes the next step reads.  fix = 1 / 2:
// d1 / d2 is the raw output of this step's last solve (and src_phi): the linearised mass fix (TanFix, sums from mpart) is
// applied to it before the integrands, and dst_phi receives the fixed field.
constexpr int TAN_NSUM = 8;
struct TanLevelArgs {
    const double *phi, *pq, *u, *h;     // this level of the histories (trajectory stride hist_stride); pq, u, h may be NULL (zeros)
    long hist_stride;
    const double *pt;                   // [B][plane] terminal target or NULL (zeros); read on the last level
    int last;
    const double *d1, *d2;              // [B][plane] dphi, d2phi of this level, NULL = zeros
    const double *src_phi, *src_mu;     // copy src -> dst at every node (NULL dst: no copy)
    double *dst_phi, *dst_mu;
    const double *W;
    int fix;                            // 0: none, 1: d1, 2: d2
    const double *rec;                  // the cell of the step that led to this level in the shift record, or NULL
    long rec_stride;
    const double *mpart;                // k_tan_mass's partials of the field to fix
    double LxLy;
    FixCheck chk;                       // the step that led to this level
};
__global__ __launch_bounds__(NTH) void k_tan_level(Geom G, TanLevelArgs a, double *__restrict__ part /* this level's [B][nblk][8] */,
                                                   long part_stride) {
    TILE_COORDS;
    __shared__ double sred[TAN_NSUM * 4];
    __shared__ double s_fix[2];
    const long pb = b * G.plane, hb = b * a.hist_stride;
    const double *rec = (a.fix && a.rec) ? a.rec + b * a.rec_stride : (const double *)nullptr;
    const double shift = rec ? rec[0] : 0.0;
    if (shift != 0.0) {                 // uniform over the workgroup
        post_sums(a.mpart, nblk, (int)b, s_fix);
        __syncthreads();
    }
    const TanFix tf(s_fix, rec, a.LxLy);
    a.chk.look(tf, s_fix, b, blk);
    double acc[TAN_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            const long o = (long)r * G.pitch + c;
            const double w = a.W[o], ph = a.phi[hb + o];
            const double e = ph - (a.pq ? a.pq[hb + o] : 0.0);
            const double uu = a.u ? a.u[hb + o] : 0.0, hh = a.h ? a.h[hb + o] : 0.0;
            double d1 = a.d1 ? a.d1[pb + o] : 0.0, d2 = a.d2 ? a.d2[pb + o] : 0.0;
            if (a.fix == 1) d1 = tf.apply(d1, ph);
            else if (a.fix == 2) d2 = tf.apply(d2, ph);
            acc[0] += w * (e * d1);
            acc[1] += w * (d1 * d1);
            acc[2] += w * (e * d2);
            acc[3] += w * (uu * hh);
            acc[4] += w * (hh * hh);
            if (a.last) {
                const double eT = ph - (a.pt ? a.pt[pb + o] : 0.0);
                acc[5] += w * (eT * d1);
                acc[6] += w * (eT * d2);
            }
            if (a.dst_phi) {
                a.dst_phi[pb + o] = a.fix == 1 ? d1 : a.fix == 2 ? d2 : a.src_phi[pb + o];
                a.dst_mu[pb + o] = a.src_mu[pb + o];
            }
        }
    }
    const int op[TAN_NSUM] = {0, 0, 0, 0, 0, 0, 0, 0};
    block_reduce_store<TAN_NSUM>(acc, op, sred, part + b * part_stride + (long)blk * TAN_NSUM);
}

// level sums out[b][lvl][8] from the workgroup partials [b][lvl][ntiles][8], in a fixed order; grid = B * levels
__global__ void k_tan_fin(int ntiles, const double *__restrict__ part, double *__restrict__ out) {
    const long idx = (long)blockIdx.x;
    double a[TAN_NSUM] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = threadIdx.x; t < ntiles; t += 64)
        for (int k = 0; k < TAN_NSUM; ++k) a[k] += part[(idx * ntiles + t) * TAN_NSUM + k];
    for (int k = 0; k < TAN_NSUM; ++k) {
        double v = wave_sum(a[k]);
        if (threadIdx.x == 0) out[idx * TAN_NSUM + k] = v;
    }
}

// np.trapz over t of the level sums and the six scalars of a trajectory, with its own b1, b2, b3; grid = B, 64 threads
//   out[b] = {s_state, s_ctrl, c_gn, c_state, c_ctrl, n_h}   (c_state = NaN when order == 1)
__global__ void k_tan_scalars(int M, const double *__restrict__ lvl, const double *__restrict__ t,
                              const double *__restrict__ opt_tab, int order, double *__restrict__ out) {
    const int b = blockIdx.x, k = threadIdx.x;
    __shared__ double I[TAN_NSUM];
    const double *s = lvl + (long)b * (M + 1) * TAN_NSUM;
    if (k < TAN_NSUM) {
        double acc = 0.0;
        for (int n = 0; n < M; ++n) acc += (t[n + 1] - t[n]) * (s[(n + 1) * TAN_NSUM + k] + s[n * TAN_NSUM + k]) / 2.0;
        I[k] = acc;
    }
    __syncthreads();
    if (k != 0) return;
    const double b1 = opt_tab[b * OPT_STRIDE + OPT_B1], b2 = opt_tab[b * OPT_STRIDE + OPT_B2], b3 = opt_tab[b * OPT_STRIDE + OPT_B3];
    const double *sM = s + (long)M * TAN_NSUM;
    double *o = out + 6 * b;
    o[0] = b1 * I[0] + b2 * sM[5];
    o[1] = b3 * I[3];
    o[2] = b1 * I[1] + b2 * sM[1];
    o[3] = order == 2 ? b1 * I[2] + b2 * sM[6] : __longlong_as_double(0x7ff8000000000000LL);
    o[4] = b3 * I[4];
    o[5] = I[4];
}

// ---------------------------------------------------------------------------------
// Transposed (adjoint) sweep of the tangent march, vch2d_hessvec: the exact gradient field G = d(J1+J2+J3)/du and the
// Hessian-vector product H h as Euclidean fields.
//
// The Newton matrix J = [[Kpp, -I/2], [I/dt, -L/2]] obeys J^T = S J S^-1 with S = diag(-(2/dt) wq, wq), wq = the trapezoid
// weights of the plane as it is stored (wdev): wq L is symmetric and the off-diagonal blocks are multiples of I.  In the
// scaled multipliers lam^ = lam / wq every transposed stencil is the plain one again, so a transposed solve is the tangent's
// own solve chain between two diagonal scalings.  Backward over the steps, k = M-1 .. 0, dt = dt_k:
//   lam^phi += wt[k+1] b1 (Wc/wq) e[k+1]                                   (+ b2 (Wc/wq) (phi_M - phi_T) at k = M-1)
//   lam^v    = lam^phi - (wts/wq) sum_int(wq lam^phi) / W_k               (where s_k != 0: transpose of the linearised fix)
//   J(phi*) [xp; xm] = [ -(dt/2) lam^v ; lam^mu ],   y^p = -(2/dt) xp,  y^m = xm
//   lam^dw = y^p / 2 + lam^w;   G[k] += beta wq lam^dw,  G[k+1] += beta wq lam^dw            (while k < rows - 1)
//   lam^  <- ( Kp y^p + y^m / dt,  y^p / 2 + L y^m / 2,  y^p / 2 + alpha lam^dw )
// Kp = (tau/dt + 2 c2) I + kappa/2 L, alpha = (gamma/dt - 1/2) / (gamma/dt + 1/2), beta = (1/2) / (gamma/dt + 1/2).
// The second sweep (H h) runs beside the first with the same matrix: its level source is the tangent of h after the mean
// removal instead of e, and its right-hand side carries - c1 rho(phi*) y^p v_k, v_k the tangent's raw solve of step k.
// No atomics: every thread updates its own nodes, every sum goes through workgroup partials read in a fixed order.
// ---------------------------------------------------------------------------------
struct HvRhsArgs {
    const double *lphi, *lmu;       // [B][plane] scaled multipliers lam^phi, lam^mu
    const double *phi1;             // level k+1 of the state history
    long hist_stride;               // trajectory stride of phi1 and v
    const double *rec;              // step k's cell of the shift record ([B] cells rec_stride apart), NULL = no shifts
    long rec_stride;
    const double *mpart;            // partials {sum_int wq lam^phi, sum_int wts} of the emit kernel that wrote lphi
    const double *wts;              // the mass fix's weights (one plane)
    const double *xp1;              // SECOND: xp of the first sweep's solve of this step (y^p = -(2/dt) xp) ...
    const double *v;                // ... and level k of the history of raw tangent solves
    FixCheck chk;                   // step k
};

// Right-hand side of a transposed solve in the form k_solve_setup / k_tan_rhs leave: A = -(dt/2) lam^v on the tile and its
// one-node halo (a pointwise function of the mirrored node), R_phi := -A, rhs := lam^mu - L A, D and the partials
// {-, sum rhs^2, min D, max D} for k_fin_lin_begin (mode 2).  D and rho are taken at phi* (fix_phi_star).
template <int SECOND>
__global__ __launch_bounds__(NTH) void k_hv_rhs(Geom G, Phys P, HvRhsArgs a, double dt, double *__restrict__ Rphi,
                                                double *__restrict__ rhs, double *__restrict__ D, double *__restrict__ part) {
    TILE_COORDS;
    __shared__ double sr[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    __shared__ double s_fix[2];
    constexpr int W = TX + 2;
    const long pb = b * G.plane, hb = b * a.hist_stride;
    const double *rec = a.rec ? a.rec + b * a.rec_stride : (const double *)nullptr;
    const double shift = rec ? rec[0] : 0.0;
    if (shift != 0.0) {                 // uniform over the workgroup
        post_sums(a.mpart, nblk, (int)b, s_fix);
        __syncthreads();
    }
    const TanFix tf(s_fix, rec, P.LxLy);
    a.chk.look(tf, s_fix, b, blk);
    const double ys = -2.0 / dt;
    for (int e = threadIdx.x; e < W * (TY + 2); e += NTH) {
        const int ly = e / W, lxx = e - ly * W;
        const int gr = refl(r0 - 1 + ly, G.ns), gc = refl(c0 - 1 + lxx, G.nf);
        const long o = (long)gr * G.pitch + gc;
        double v = a.lphi[pb + o];
        if (tf.mean != 0.0) v -= (a.wts[o] / wdev(gr, gc, G)) * tf.mean;
        if (SECOND) v -= P.c1 * tan_rho(fix_phi_star(a.phi1[hb + o], shift, tf.all)) * (ys * a.xp1[pb + o]) * a.v[hb + o];
        sr[e] = -(0.5 * dt) * v;
    }
    __syncthreads();
    double acc[4] = {0.0, 0.0, 1e300, -1e300};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            const int p = (ly + 1) * W + lx + 1;
            const long o = (long)r * G.pitch + c;
            const double rh = a.lmu[pb + o] - lap_at<W>(sr, p, G.ax, G.ay);
            const double d = jac_diag(fix_phi_star(a.phi1[hb + o], shift, tf.all), P.tau / dt, P.c1);
            Rphi[pb + o] = -sr[p];
            rhs[pb + o] = rh;
            D[pb + o] = d;
            acc[1] += rh * rh;
            acc[2] = fmin(acc[2], d);
            acc[3] = fmax(acc[3], d);
        }
    }
    const int op[4] = {0, 0, 1, 2};
    block_reduce_store<4>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

struct HvEmitArgs {
    const double *xp, *xm;          // [B][plane] output of the transposed solve; NULL: the start of the sweep (y = 0)
    double *lphi, *lmu, *lw;        // [B][plane] scaled multipliers, updated in place (every thread its own nodes)
    double *out_k, *out_k1;         // rows k, k+1 of G or Hh (history layout), NULL = the rows drive no step (F2:545-548)
    const double *src_a, *src_b;    // the new level's source field src_a - src_b (history layout; src_b NULL = zeros;
                                    // src_a NULL = no source: level 0)
    const double *src_T;            // terminal level: [B][plane] target taken off src_a in the b2 term (NULL = zeros)
    int terminal;
    long hist_stride;
    double wt;                      // trapezoid weight in t of the new level
    const double *opt_tab;          // b1, b2 of every trajectory
    const double *Wc, *wts;         // the cost's and the mass fix's weights (one plane each)
    const double *phi_fix;          // the new level of the state history: the step below it shifted the nodes fix_in_set names
    const double *rec;              // that step's cell of the shift record, NULL = no shifts (or no step below)
    long rec_stride;
    double *part;                   // [B][nblk][NPART] partials {sum_int wq lam^phi, sum_int wts (the classified weight)} for that step's k_hv_rhs
    double dt, kp, half_kappa, alpha, beta;
};

// After a transposed solve: y^, lam^dw, the two row updates of G (or Hh), the multipliers of the level below with that
// level's source, and the partials of the next step's transposed fix.  Reads xp, xm with a one-node halo.
__global__ __launch_bounds__(NTH) void k_hv_emit(Geom G, HvEmitArgs a) {
    TILE_COORDS;
    __shared__ double sp[(TY + 2) * (TX + 2)];
    __shared__ double sm[(TY + 2) * (TX + 2)];
    __shared__ double sred[NPART * 4];
    constexpr int W = TX + 2;
    const long pb = b * G.plane, hb = b * a.hist_stride;
    const bool start = a.xp == nullptr;
    if (!start) {
        load_tile<1>(sp, a.xp + pb, G, c0, r0);
        load_tile<1>(sm, a.xm + pb, G, c0, r0);
    }
    __syncthreads();
    const double *rec = a.rec ? a.rec + b * a.rec_stride : (const double *)nullptr;
    const double shift = rec ? rec[0] : 0.0;
    const bool all = fix_all(rec);
    const double b1 = a.opt_tab[b * OPT_STRIDE + OPT_B1], b2 = a.opt_tab[b * OPT_STRIDE + OPT_B2];
    const double ys = -2.0 / a.dt;
    double acc[2] = {0.0, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int ly = ly0 + 4 * k, r = r0 + ly, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            const int p = (ly + 1) * W + lx + 1;
            const long o = (long)r * G.pitch + c;
            const double wq = wdev(r, c, G);
            double nphi = 0.0, nmu = 0.0, nw = 0.0;
            if (!start) {
                const double yp = ys * sp[p], ym = sm[p];
                const double ldw = 0.5 * yp + a.lw[pb + o];
                if (a.out_k) {
                    const double g = a.beta * wq * ldw;
                    a.out_k[hb + o] += g;
                    a.out_k1[hb + o] += g;
                }
                nphi = a.kp * yp + a.half_kappa * (ys * lap_at<W>(sp, p, G.ax, G.ay)) + ym / a.dt;
                nmu = 0.5 * yp + 0.5 * lap_at<W>(sm, p, G.ax, G.ay);
                nw = 0.5 * yp + a.alpha * ldw;
            }
            if (a.src_a) {
                const double sa = a.src_a[hb + o];
                double s = a.wt * b1 * (sa - (a.src_b ? a.src_b[hb + o] : 0.0));
                if (a.terminal) s += b2 * (sa - (a.src_T ? a.src_T[pb + o] : 0.0));
                nphi += (a.Wc[o] / wq) * s;
            }
            a.lphi[pb + o] = nphi;
            a.lmu[pb + o] = nmu;
            a.lw[pb + o] = nw;
            if (shift != 0.0 && fix_in_set(a.phi_fix[hb + o], shift, all)) {
                acc[0] += wq * nphi;
                acc[1] += a.wts[o];
            }
        }
    }
    if (shift == 0.0) return;           // uniform over the workgroup: nobody reads the partials of a step without a shift
    const int op[2] = {0, 0};
    block_reduce_store<2>(acc, op, sred, a.part + ((long)b * nblk + blk) * NPART);
}

// The start of the fields: out[lvl] = b3 wt[lvl] Wc src[lvl] for lvl < src_rows (src NULL: none), zeros up to rows.
__global__ __launch_bounds__(NTH) void k_hv_init(Geom G, int rows, const double *__restrict__ src, int src_rows,
                                                 const double *__restrict__ wt, const double *__restrict__ opt_tab,
                                                 const double *__restrict__ Wc, long hist_stride, double *__restrict__ out) {
    TILE_COORDS;
    const long hb = b * hist_stride;
    const double b3 = opt_tab[b * OPT_STRIDE + OPT_B3];
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            const long o = (long)r * G.pitch + c;
            const double w = Wc[o];
            for (int lvl = 0; lvl < rows; ++lvl) {
                const long q = hb + (long)lvl * G.plane + o;
                out[q] = (src && lvl < src_rows) ? (b3 * wt[lvl]) * (w * src[q]) : 0.0;
            }
        }
    }
}

// Order 2, one step of the tangent of h: keeps the raw solve x (v_k), applies the linearised mass fix (TanFix, sums from
// k_tan_mass's partials) and stores the fixed field into the history dphi' and the plane the next step reads; dmu' moves on.
__global__ __launch_bounds__(NTH) void k_hv_keep(Geom G, const double *__restrict__ x, const double *__restrict__ m,
                                                 const double *__restrict__ phi1, long hist_stride,
                                                 const double *__restrict__ rec_, long rec_stride,
                                                 const double *__restrict__ mpart, double LxLy, FixCheck chk,
                                                 double *__restrict__ v_k,
                                                 double *__restrict__ dp_k1, double *__restrict__ dphi,
                                                 double *__restrict__ dmu) {
    TILE_COORDS;
    __shared__ double s_fix[2];
    const long pb = b * G.plane, hb = b * hist_stride;
    const double *rec = rec_ ? rec_ + b * rec_stride : (const double *)nullptr;
    const double shift = rec ? rec[0] : 0.0;
    if (shift != 0.0) {                 // uniform over the workgroup
        post_sums(mpart, nblk, (int)b, s_fix);
        __syncthreads();
    }
    const TanFix tf(s_fix, rec, LxLy);
    chk.look(tf, s_fix, b, blk);
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            const long o = (long)r * G.pitch + c;
            const double v = x[pb + o];
            const double f = tf.apply(v, phi1[hb + o]);
            v_k[hb + o] = v;
            dp_k1[hb + o] = f;
            dphi[pb + o] = f;
            dmu[pb + o] = m[pb + o];
        }
    }
}

// Workgroup partials {sum G h over the rows both have, sum h Hh} of a trajectory, the levels summed in order per node.
__global__ __launch_bounds__(NTH) void k_hv_dots(Geom G, const double *__restrict__ g, int g_rows, const double *__restrict__ h,
                                                 int h_rows, const double *__restrict__ hv, long hist_stride,
                                                 double *__restrict__ part) {
    TILE_COORDS;
    __shared__ double sred[NPART * 4];
    const long hb = b * hist_stride;
    double acc[2] = {0.0, 0.0};
    for (int k = 0; k < TY / 4; ++k) {
        int r = r0 + ly0 + 4 * k, c = c0 + lx;
        if (r < G.ns && c < G.nf) {
            const long o = (long)r * G.pitch + c;
            for (int lvl = 0; lvl < h_rows; ++lvl) {
                const long q = hb + (long)lvl * G.plane + o;
                const double hh = h[q];
                if (lvl < g_rows) acc[0] += g[q] * hh;
                if (hv) acc[1] += hh * hv[q];
            }
        }
    }
    const int op[2] = {0, 0};
    block_reduce_store<2>(acc, op, sred, part + ((long)b * nblk + blk) * NPART);
}

// dots[b] = the two sums from the partials in a fixed order (post_sums); NaN where a factor is missing.  grid = B, 64 threads
__global__ void k_hv_dots_fin(const double *__restrict__ part, int nblk, int have_h, int have_hv, double *__restrict__ out) {
    __shared__ double s[2];
    const int b = blockIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (have_h) post_sums(part, nblk, b, s);
    __syncthreads();
    if (threadIdx.x == 0) {
        out[2 * b] = have_h ? s[0] : nan;
        out[2 * b + 1] = (have_h && have_hv) ? s[1] : nan;
    }
}

// ---------------------------------------------------------------------------------
// Device-resident Lanczos on the reduced Hessian P H P (vch2d_hess_lanczos): the streaming passes between two
// transposed sweeps.  Every vector is a history [B][max_steps+1][plane]; the basis is a ring of `nslots` of them, vector i
// of the `nv` a pass works against sits in slot (first + i) % nslots.  A workgroup owns one plane tile of one chunk of
// levels of one trajectory: grid = (tiles, chunks, B), so that a single trajectory of 1000 levels still fills the device.
// Partials are [B][chunks][tiles][pstride]; k_kr_fin sums them per trajectory in a fixed order.  No atomics.  A trajectory
// whose iteration has stopped (stop[b] != 0) is skipped by every pass.
// ---------------------------------------------------------------------------------
constexpr int KR_GROUP = 8;           // basis vectors a pass holds accumulators for at a time
struct KrArgs {
    const double *Q;                  // the basis
    long slot_stride, hist_stride;    // doubles between two slots / two trajectories
    int levels, lchunk;               // rows of a vector (M + 1), levels per workgroup
    int first, nv, nslots;
    int pstride;                      // slots per workgroup partial
    const unsigned char *mask;        // [B][max_steps+1][plane] bytes, non-zero = free
    const long long *stop;            // [B]
};
#define KR_COORDS                                                                       \
    const int b = blockIdx.z, blk = blockIdx.x;                                         \
    const int c0 = (blk / G.tiles_s) * TX, r0 = (blk % G.tiles_s) * TY;                 \
    const int c = c0 + (threadIdx.x & 63), ly0 = threadIdx.x >> 6;                      \
    const int l0 = blockIdx.y * a.lchunk, l1 = min(l0 + a.lchunk, a.levels);            \
    const long hb = (long)b * a.hist_stride;                                            \
    double *const my_part = part ? part + (((long)b * gridDim.y + blockIdx.y) * gridDim.x + blk) * a.pstride : nullptr; \
    (void)my_part
// the nodes of the workgroup's tile and chunk that this thread owns: o = offset inside the trajectory's history
#define KR_NODES(body)                                                                  \
    for (int lvl = l0; lvl < l1; ++lvl)                                                 \
        for (int k = 0; k < TY / 4; ++k) {                                              \
            const int r = r0 + ly0 + 4 * k;                                             \
            if (r < G.ns && c < G.nf) {                                                 \
                const long o = hb + (long)lvl * G.plane + (long)r * G.pitch + c;        \
                body                                                                    \
            }                                                                           \
        }
__device__ __forceinline__ const double *kr_slot(const KrArgs &a, int i) {
    return a.Q + (long)((a.first + i) % a.nslots) * a.slot_stride;
}

// The free set of a trajectory and its size.  build: from the resident control (rows beyond u_rows are zeros) and the
// trajectory's own box, mask = u > u_min + tol && u < u_max - tol && |u| > tol, stored as bytes; otherwise the bytes are
// the caller's.  Partial slot 0 = the count (exact in a double).
__global__ __launch_bounds__(NTH) void k_kr_mask(Geom G, KrArgs a, const double *__restrict__ u, int u_rows,
                                                 const double *__restrict__ opt_tab, double tol, int build,
                                                 unsigned char *__restrict__ mask, double *__restrict__ part) {
    KR_COORDS;
    __shared__ double sred[NPART * 4];
    const double lo = opt_tab[b * OPT_STRIDE + OPT_UMIN] + tol, hi = opt_tab[b * OPT_STRIDE + OPT_UMAX] - tol;
    double acc[1] = {0.0};
    KR_NODES(
        bool m;
        if (build) {
            const double v = (u && lvl < u_rows) ? u[o] : 0.0;
            m = v > lo && v < hi && fabs(v) > tol;
            mask[o] = m ? 1 : 0;
        } else {
            m = mask[o] != 0;
        }
        acc[0] += m ? 1.0 : 0.0;
    )
    const int op[1] = {0};
    block_reduce_store<1>(acc, op, sred, my_part);
}

// The start: dst = P src (dst and src may be the same history), partial slot 0 = sum (P src)^2.
__global__ __launch_bounds__(NTH) void k_kr_start(Geom G, KrArgs a, const double *src, double *dst, double *__restrict__ part) {
    KR_COORDS;
    __shared__ double sred[NPART * 4];
    double acc[1] = {0.0};
    KR_NODES(
        const double v = a.mask[o] ? src[o] : 0.0;
        dst[o] = v;
        acc[0] += v * v;
    )
    const int op[1] = {0};
    block_reduce_store<1>(acc, op, sred, my_part);
}

// One pass of the Gram-Schmidt step over w (in place), 8 - 16 B per node and vector:
//   MODE 0   partials i = sum q_i (P w)                                            (w is read through the mask, not written)
//   MODE 1   w := P w - sum_i coef[b][i] q_i, then partials i = sum q_i w          (round 1's subtraction, round 2's products)
//   MODE 2   w := w - sum_i coef[b][i] q_i, partial 0 = sum w^2                    (round 2's subtraction, the norm)
// Masked-off nodes of every q_i are exact zeros, so w leaves MODE 1 with exact zeros there.  The products run over the
// basis in groups of KR_GROUP accumulators; w is read again per group (the workgroup's own lines, just touched).
template <int MODE>
__global__ __launch_bounds__(NTH) void k_kr_pass(Geom G, KrArgs a, double *w, const double *__restrict__ coef,
                                                 double *__restrict__ part) {
    KR_COORDS;
    if (a.stop[b]) return;                  // uniform over the workgroup
    __shared__ double sred[KR_GROUP * 4];
    if (MODE != 0) {
        const double *cf = coef + (long)b * a.pstride;
        double nrm[1] = {0.0};
        KR_NODES(
            double v = w[o];
            if (MODE == 1) v = a.mask[o] ? v : 0.0;
            for (int i = 0; i < a.nv; ++i) v -= cf[i] * kr_slot(a, i)[o];
            w[o] = v;
            nrm[0] += v * v;
        )
        if (MODE == 2) {
            const int op[1] = {0};
            block_reduce_store<1>(nrm, op, sred, my_part);
            return;
        }
    }
    for (int g0 = 0; g0 < a.nv; g0 += KR_GROUP) {
        double acc[KR_GROUP];
        const double *q[KR_GROUP];
#pragma unroll
        for (int i = 0; i < KR_GROUP; ++i) {
            acc[i] = 0.0;
            q[i] = kr_slot(a, min(g0 + i, a.nv - 1));       // past the end: the last vector again, its sum is not stored
        }
        KR_NODES(
            double v = w[o];
            if (MODE == 0) v = a.mask[o] ? v : 0.0;
            _Pragma("unroll")
            for (int i = 0; i < KR_GROUP; ++i) acc[i] += q[i][o] * v;
        )
        int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
        for (int i = 0; i < KR_GROUP; ++i) {
            const double s = wave_sum(acc[i]);
            if (lane == 0) sred[i * 4 + wv] = s;
        }
        __syncthreads();
        if (threadIdx.x < KR_GROUP && g0 + (int)threadIdx.x < a.nv) {
            const int i = threadIdx.x;
            my_part[g0 + i] = (sred[i * 4] + sred[i * 4 + 1]) + (sred[i * 4 + 2] + sred[i * 4 + 3]);
        }
        __syncthreads();
    }
}

// q_{j+1} = w / beta_j into its basis slot and into the direction buffer of the next sweep.  By the trajectory's stop cell:
// 0 both stores; 1 (the last step, a valid q_{j+1}) the slot only; 2 (no valid q_{j+1}) zeros into the slot; 3 nothing.
__global__ __launch_bounds__(NTH) void k_kr_next(Geom G, KrArgs a, const double *src, const double *__restrict__ scal,
                                                 double *slot, double *__restrict__ dir) {
    double *part = nullptr;
    KR_COORDS;
    const long long st = a.stop[b];
    if (st == 3) return;
    const double s = scal[b];
    KR_NODES(
        const double v = st == 2 ? 0.0 : src[o] / s;
        slot[o] = v;
        if (st == 0) dir[o] = v;
    )
}

// out = sum_{i<nv} coef[b][i] q_i  (vch2d_krylov_vector)
__global__ __launch_bounds__(NTH) void k_kr_lincomb(Geom G, KrArgs a, const double *__restrict__ coef, double *__restrict__ out) {
    double *part = nullptr;
    KR_COORDS;
    const double *cf = coef + (long)b * a.pstride;
    KR_NODES(
        double v = 0.0;
        for (int i = 0; i < a.nv; ++i) v += cf[i] * kr_slot(a, i)[o];
        out[o] = v;
    )
}

// The scalars of a pass, one workgroup of NTH threads per trajectory: the partials summed in a fixed order (thread t takes
// elements t, t + NTH, ... in turn, then a tree over the threads).
struct KrCells {
    double *coef1, *coef2;            // [B][pstride] coefficients of the two Gram-Schmidt rounds
    double *alpha, *beta;             // [B][k]
    double *look;                     // [B][2] what the host reads per step: beta_j, the stop cell
    double *scal;                     // [B] the divisor of the next k_kr_next
    double *amax;                     // [B] max_i |alpha_i| so far
    long long *nfree, *lim, *stop;    // [B] size of the free set, min(k, n_free), the stop cell
};
__device__ __forceinline__ double kr_sum(const double *__restrict__ part, long n, int pstride, int slot, double *sh) {
    double s = 0.0;
    for (long e = threadIdx.x; e < n; e += NTH) s += part[e * pstride + slot];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int h = NTH / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
// mode 0: the count of k_kr_mask -> nfree, lim = min(k, nfree), the cells of a new iteration
// mode 1: the start's norm -> scal, look[0]
// mode 2 / 3: the nv products of round 1 / 2 -> coef1 / coef2
// mode 4: step j's norm -> beta_j, alpha_j = coef1 + coef2 on q_j, the stop rules and the stop cell
__global__ __launch_bounds__(NTH) void k_kr_fin(KrCells x, const double *__restrict__ part, long n, int pstride, int mode, int nv,
                                                int j, int k) {
    __shared__ double sh[NTH];
    const int b = blockIdx.x;
    const double *p = part + (long)b * n * pstride;
    if (mode == 0) {
        const double cnt = kr_sum(p, n, pstride, 0, sh);
        if (threadIdx.x == 0) {
            x.nfree[b] = (long long)cnt;
            x.lim[b] = min((long long)k, (long long)cnt);
            x.stop[b] = 0;
            x.amax[b] = 0.0;
        }
        return;
    }
    if (mode == 1) {
        const double s = sqrt(kr_sum(p, n, pstride, 0, sh));
        if (threadIdx.x == 0) x.scal[b] = x.look[2 * b] = s;
        return;
    }
    if (x.stop[b]) {                       // uniform: stopped at an earlier step
        if (threadIdx.x == 0 && mode == 4) x.stop[b] = 3;
        return;
    }
    if (mode == 2 || mode == 3) {
        double *cf = (mode == 2 ? x.coef1 : x.coef2) + (long)b * pstride;
        for (int i = 0; i < nv; ++i) {
            const double s = kr_sum(p, n, pstride, i, sh);
            if (threadIdx.x == 0) cf[i] = s;
        }
        return;
    }
    const double beta = sqrt(kr_sum(p, n, pstride, 0, sh));
    if (threadIdx.x != 0) return;
    const double alpha = x.coef1[(long)b * pstride + nv - 1] + x.coef2[(long)b * pstride + nv - 1];
    const double am = fmax(x.amax[b], fabs(alpha));
    x.amax[b] = am;
    x.alpha[(long)b * k + j] = alpha;
    x.beta[(long)b * k + j] = beta;
    const bool broke = !isfinite(beta) || beta <= 1e-14 * am;          // an invariant subspace, or nothing to go on with
    const bool last = j + 1 >= x.lim[b];
    const long long st = broke || j + 1 >= x.nfree[b] ? 2 : (last ? 1 : 0);
    x.stop[b] = st;
    x.scal[b] = beta;
    x.look[2 * b] = beta;
    x.look[2 * b + 1] = (double)st;
}

// ---------------------------------------------------------------------------------
// Device-resident Newton-CG on the free set (vch2d_hess_cg): (preconditioned) conjugate gradients on
// P H P x = P b from x_0 = 0 with x, r and p in slots 0, 1, 2 of the Krylov basis storage.  Tiling, partials and the
// fixed-order sums are those of the Lanczos passes above (KrArgs, KR_COORDS / KR_NODES, the order of kr_sum; first, nv and
// nslots of KrArgs are not read).  D = diag(wt (x) W_cost), the L2(Q) mass of the control, is computed per node from the level's
// trapezoid weight and the plane's cost weight when precond != 0 and is the identity otherwise.  Masked-off nodes of x, r
// and p are exact zeros; P is applied where H p is read.  A trajectory whose stop cell is non-zero is skipped by every
// pass, so its x, r and p stay as the stopping step left them.  No atomics.
// ---------------------------------------------------------------------------------
enum { NCG_X = 0, NCG_R = 1, NCG_P = 2 };
enum { NCG_RUNNING = 0, NCG_CONVERGED = 1, NCG_NEGCURV = 2, NCG_BREAKDOWN = 3 };      // the stop cell: VCH_CG_* of vch.h
__device__ __forceinline__ double *ncg_slot(const KrArgs &a, int i) { return const_cast<double *>(a.Q) + (long)i * a.slot_stride; }
#define NCG_D(lvl, r, c) (precond ? wt[lvl] * Wc[(long)(r) * G.pitch + (c)] : 1.0)

// The start: r = P b, x = 0, p = D^-1 r into its slot and into the direction buffer of the first sweep; partials
// {r.r, r.D^-1 r}.  NEWTON 0: b = src (the uploaded right-hand side; src may be dir).  NEWTON 1: src is the gradient field
// of J1 + J2 + J3 and b = -(src + kappa_sparsity_b wt_k W_cost_ij sign(u)), the Newton right-hand side of the full cost
// (rows of the control beyond u_rows are zeros).
template <int NEWTON>
__global__ __launch_bounds__(NTH) void k_ncg_start(Geom G, KrArgs a, const double *src, const double *__restrict__ u, int u_rows,
                                                   const double *__restrict__ wt, const double *__restrict__ Wc,
                                                   const double *__restrict__ opt_tab, int precond, double *dir,
                                                   double *__restrict__ part) {
    KR_COORDS;
    __shared__ double sred[NPART * 4];
    const double ks = opt_tab[b * OPT_STRIDE + OPT_KS];
    double *const xs = ncg_slot(a, NCG_X), *const rs = ncg_slot(a, NCG_R), *const ps = ncg_slot(a, NCG_P);
    double acc[2] = {0.0, 0.0};
    KR_NODES(
        double rv = 0.0;
        double z = 0.0;
        if (a.mask[o]) {
            rv = src[o];
            if (NEWTON) {
                const double v = (u && lvl < u_rows) ? u[o] : 0.0;
                const double sgn = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
                rv = -(rv + (ks * wt[lvl]) * (Wc[(long)r * G.pitch + c] * sgn));
            }
            z = rv / NCG_D(lvl, r, c);
        }
        xs[o] = 0.0;
        rs[o] = rv;
        ps[o] = z;
        dir[o] = z;
        acc[0] += rv * rv;
        acc[1] += rv * z;
    )
    const int op[2] = {0, 0};
    block_reduce_store<2>(acc, op, sred, my_part);
}

// Partials {p.(P H p), p.D p}; hp = H p of the sweep just run.
__global__ __launch_bounds__(NTH) void k_ncg_curv(Geom G, KrArgs a, const double *__restrict__ hp, const double *__restrict__ wt,
                                                  const double *__restrict__ Wc, int precond, double *__restrict__ part) {
    KR_COORDS;
    if (a.stop[b]) return;                  // uniform over the workgroup
    __shared__ double sred[NPART * 4];
    const double *const ps = ncg_slot(a, NCG_P);
    double acc[2] = {0.0, 0.0};
    KR_NODES(
        const double pv = ps[o];
        const double hv = a.mask[o] ? hp[o] : 0.0;
        acc[0] += pv * hv;
        acc[1] += pv * (NCG_D(lvl, r, c) * pv);
    )
    const int op[2] = {0, 0};
    block_reduce_store<2>(acc, op, sred, my_part);
}

// x += alpha p, r -= alpha P H p; partials {r.r, r.D^-1 r} of the new residual.
__global__ __launch_bounds__(NTH) void k_ncg_update(Geom G, KrArgs a, const double *__restrict__ hp, const double *__restrict__ alpha,
                                                    const double *__restrict__ wt, const double *__restrict__ Wc, int precond,
                                                    double *__restrict__ part) {
    KR_COORDS;
    if (a.stop[b]) return;
    __shared__ double sred[NPART * 4];
    double *const xs = ncg_slot(a, NCG_X), *const rs = ncg_slot(a, NCG_R);
    const double *const ps = ncg_slot(a, NCG_P);
    const double al = alpha[b];
    double acc[2] = {0.0, 0.0};
    KR_NODES(
        const double pv = ps[o];
        const double hv = a.mask[o] ? hp[o] : 0.0;
        xs[o] += al * pv;
        const double rv = rs[o] - al * hv;
        rs[o] = rv;
        acc[0] += rv * rv;
        acc[1] += rv * (rv / NCG_D(lvl, r, c));
    )
    const int op[2] = {0, 0};
    block_reduce_store<2>(acc, op, sred, my_part);
}

// p = D^-1 r + beta p into its slot and into the direction buffer of the next sweep.
__global__ __launch_bounds__(NTH) void k_ncg_dir(Geom G, KrArgs a, const double *__restrict__ beta, const double *__restrict__ wt,
                                                 const double *__restrict__ Wc, int precond, double *__restrict__ dir) {
    double *part = nullptr;
    KR_COORDS;
    if (a.stop[b]) return;
    const double *const rs = ncg_slot(a, NCG_R);
    double *const ps = ncg_slot(a, NCG_P);
    const double be = beta[b];
    KR_NODES(
        const double v = rs[o] / NCG_D(lvl, r, c) + be * ps[o];
        ps[o] = v;
        dir[o] = v;
    )
}
#undef NCG_D

// The scalars of the iteration, one workgroup per trajectory, sums in the fixed order of kr_sum (ncg_sum below).
//   mode 1   the start: ||P b|| -> rnorm0, look[0]; rho = r.D^-1 r; pred = 0; steps = 0; a zero right-hand side has converged
//   mode 2   step j, after k_ncg_curv: c = p.P H p, n = p.D p, curv[j] = c / n; c not finite: BREAKDOWN; !(c > 0): NEGCURV;
//            otherwise alpha = rho / c
//   mode 3   step j, after k_ncg_update: pred += alpha rho / 2, resid[j] = ||r|| / ||P b||, steps = j + 1; not finite:
//            BREAKDOWN; resid[j] <= cg_tol: CONVERGED; otherwise beta = rho_new / rho
// look = {mode 1: ||P b||, later: the last residual; the stop cell}.
struct NcgCells {
    double *resid, *curv;             // [B][k]
    double *look;                     // [B][2]
    double *alpha, *beta;             // [B] the step length of k_ncg_update, the factor of k_ncg_dir
    double *rho, *rnorm0, *pred;      // [B]
    long long *steps, *stop;          // [B]
};
// kr_sum, word for word (the same order of additions).  A copy, not a call: with a second kernel calling kr_sum its LDS
// buffer is no longer the same constant at every call site, and k_kr_fin compiles to 17 VGPRs / 57 SGPRs instead of 14 / 56.
__device__ __forceinline__ double ncg_sum(const double *__restrict__ part, long n, int pstride, int slot, double *sh) {
    double s = 0.0;
    for (long e = threadIdx.x; e < n; e += NTH) s += part[e * pstride + slot];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int h = NTH / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
__global__ __launch_bounds__(NTH) void k_ncg_fin(NcgCells x, const double *__restrict__ part, long n, int pstride, int mode, int j,
                                                 int k, double cg_tol) {
    __shared__ double sh[NTH];
    const int b = blockIdx.x;
    const double *p = part + (long)b * n * pstride;
    if (mode != 1 && x.stop[b]) return;     // uniform: stopped at an earlier step
    const double s0 = ncg_sum(p, n, pstride, 0, sh), s1 = ncg_sum(p, n, pstride, 1, sh);
    if (threadIdx.x != 0) return;
    long long st = NCG_RUNNING;
    if (mode == 1) {
        const double nb = sqrt(s0);
        x.rnorm0[b] = nb;
        x.rho[b] = s1;
        x.pred[b] = 0.0;
        x.steps[b] = 0;
        x.look[2 * b] = nb;
        st = nb == 0.0 ? NCG_CONVERGED : NCG_RUNNING;
    } else if (mode == 2) {
        x.curv[(long)b * k + j] = s0 / s1;
        if (!isfinite(s0)) st = NCG_BREAKDOWN;
        else if (!(s0 > 0.0)) st = NCG_NEGCURV;
        else x.alpha[b] = x.rho[b] / s0;
    } else {
        const double rho = x.rho[b], res = sqrt(s0) / x.rnorm0[b];
        x.pred[b] += 0.5 * x.alpha[b] * rho;
        x.resid[(long)b * k + j] = res;
        x.steps[b] = j + 1;
        x.look[2 * b] = res;
        if (!isfinite(res) || !isfinite(s1)) st = NCG_BREAKDOWN;
        else if (res <= cg_tol) st = NCG_CONVERGED;
        else {
            x.beta[b] = s1 / rho;
            x.rho[b] = s1;
        }
    }
    x.stop[b] = st;
    x.look[2 * b + 1] = (double)st;
}

// ---------------------------------------------------------------------------------
// Truncated (Steihaug-Toint) conjugate gradients in a trust region (vch2d_hess_cg_tr): the iteration above
// with k_ncg_fin_tr in place of k_ncg_fin, every other kernel unchanged.  The region is ||x||_D <= radius with the
// preconditioner's D (the identity without it).  Since x_0 = 0, the recurrences xx = ||x||_D^2 and xp = x.D p start at 0:
//   x' = x + alpha p:   xx' = xx + 2 alpha xp + alpha^2 pp
//   p' = D^-1 r' + beta p, x'.r' = 0:   xp' = beta (xp + alpha pp)
// tau = the positive root of xx + 2 tau xp + tau^2 pp = radius^2.  An exit on the boundary is pending between mode 2 and
// mode 3: the stop cell and look[1] stay 0, so that k_ncg_update runs once more with alpha = tau and r stays P b - P H P x.
// ---------------------------------------------------------------------------------
enum { NCG_BOUNDARY = 4 };                      // VCH_CG_BOUNDARY of vch.h
struct NtrCells {
    const double *radius;             // [B]
    double *xx, *xp, *pp, *c;         // [B] ||x||_D^2, x.D p, p.D p and p.P H p of the step
    long long *pend;                  // [B] the exit mode 3 takes: 0, NCG_NEGCURV or NCG_BOUNDARY
};
// tau >= 0 with xx + 2 tau xp + tau^2 pp = d2 (xx <= d2, pp > 0), in the form without cancellation for either sign of xp
__device__ __forceinline__ double ntr_tau(double xx, double xp, double pp, double d2) {
    const double gap = fmax(d2 - xx, 0.0), disc = sqrt(xp * xp + pp * gap);
    return xp > 0.0 ? gap / (xp + disc) : (disc - xp) / pp;
}
// ncg_sum, word for word: a copy for the reason given there, so that k_ncg_fin keeps its registers too.
__device__ __forceinline__ double ntr_sum(const double *__restrict__ part, long n, int pstride, int slot, double *sh) {
    double s = 0.0;
    for (long e = threadIdx.x; e < n; e += NTH) s += part[e * pstride + slot];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int h = NTH / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
// mode 1   as k_ncg_fin, then xx = xp = 0 and nothing pending.
// mode 2   as k_ncg_fin, then: c not finite: BREAKDOWN; !(c > 0): alpha = tau, pending NEGCURV; the step rho / c would
//          leave the region (xx + 2 alpha xp + alpha^2 pp >= radius^2): alpha = tau, pending BOUNDARY; otherwise alpha = rho / c.
//          A tau that is not finite (radius = +inf on a direction of non-positive curvature) stops at once with NEGCURV as
//          k_ncg_fin does: x stays as it is.
// mode 3   pending: pred += tau rho - tau^2 c / 2, resid[j], steps = j + 1, xx by its recurrence, stop = the pending exit;
//          otherwise k_ncg_fin's arithmetic, then xx and (still running) xp by their recurrences.
__global__ __launch_bounds__(NTH) void k_ncg_fin_tr(NcgCells x, NtrCells t, const double *__restrict__ part, long n, int pstride,
                                                    int mode, int j, int k, double cg_tol) {
    __shared__ double sh[NTH];
    const int b = blockIdx.x;
    const double *p = part + (long)b * n * pstride;
    if (mode != 1 && x.stop[b]) return;     // uniform: stopped at an earlier step
    const double s0 = ntr_sum(p, n, pstride, 0, sh), s1 = ntr_sum(p, n, pstride, 1, sh);
    if (threadIdx.x != 0) return;
    long long st = NCG_RUNNING;
    if (mode == 1) {
        const double nb = sqrt(s0);
        x.rnorm0[b] = nb;
        x.rho[b] = s1;
        x.pred[b] = 0.0;
        x.steps[b] = 0;
        x.look[2 * b] = nb;
        st = nb == 0.0 ? NCG_CONVERGED : NCG_RUNNING;
        t.xx[b] = 0.0;
        t.xp[b] = 0.0;
        t.pend[b] = NCG_RUNNING;
    } else if (mode == 2) {
        const double xx = t.xx[b], xp = t.xp[b];
        x.curv[(long)b * k + j] = s0 / s1;
        long long pend = NCG_RUNNING;
        if (!isfinite(s0)) {
            st = NCG_BREAKDOWN;
        } else {
            const double rad = t.radius[b], d2 = rad * rad;
            double al = 0.0;
            if (!(s0 > 0.0)) {
                pend = NCG_NEGCURV;
            } else {
                al = x.rho[b] / s0;
                if (xx + 2.0 * al * xp + al * al * s1 >= d2) pend = NCG_BOUNDARY;
            }
            if (pend) al = ntr_tau(xx, xp, s1, d2);
            if (pend && !isfinite(al)) {
                st = NCG_NEGCURV;
                pend = NCG_RUNNING;
            } else {
                x.alpha[b] = al;
            }
        }
        t.pp[b] = s1;
        t.c[b] = s0;
        t.pend[b] = pend;
    } else {
        const long long pend = t.pend[b];
        const double xx = t.xx[b], xp = t.xp[b];
        const double rho = x.rho[b], res = sqrt(s0) / x.rnorm0[b], al = x.alpha[b], pp = t.pp[b];
        x.resid[(long)b * k + j] = res;
        x.steps[b] = j + 1;
        x.look[2 * b] = res;
        if (pend) {
            x.pred[b] += al * rho - 0.5 * (al * al) * t.c[b];
            st = pend;
        } else {
            x.pred[b] += 0.5 * x.alpha[b] * rho;
            if (!isfinite(res) || !isfinite(s1)) st = NCG_BREAKDOWN;
            else if (res <= cg_tol) st = NCG_CONVERGED;
            else {
                x.beta[b] = s1 / rho;
                x.rho[b] = s1;
            }
        }
        t.xx[b] = xx + 2.0 * al * xp + al * al * pp;
        if (st == NCG_RUNNING) t.xp[b] = x.beta[b] * (xp + al * pp);
    }
    x.stop[b] = st;
    x.look[2 * b + 1] = (double)st;
}

// ---------------------------------------------------------------------------------
// Damped Newton rounds on the free set (vch2d_pgd_newton, vch2d_newton_trial): the trial control of a step
// length.  Tiling and partials are those of the Newton-CG passes above (KrArgs, KR_COORDS / KR_NODES; x is slot NCG_X), the
// partials here have 4 slots per workgroup: {sum (t - u)^2, sum u^2, nodes pinned to 0, nodes the clip moved}, the counts
// exact in a double.  No atomics.  A trajectory whose verdict is in (skip[b] != 0; skip may be NULL) is left alone.
//
// Per node t = min(max(u + s_b x, u_min_b), u_max_b) with NumPy's order of comparisons (a NaN stays a NaN); a free node with
// t u < 0 becomes 0, the kink, where the next round pins it.  Rows of u beyond u_rows are zeros.  Every s the rounds use is
// a power of two, so s x is exact (short of an underflow) and u + s x rounds once whether or not the compiler fuses the
// multiply-add: the trial has the bits of np.clip(u + s * d, lo, hi).  A node's three operands (u, x, the mask byte) are
// requested together, in front of the first use of any of them.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NTH) void k_nt_trial(Geom G, KrArgs a, const double *__restrict__ u, int u_rows,
                                                  const double *__restrict__ s_tab, const double *__restrict__ opt_tab,
                                                  const int *__restrict__ skip, double *__restrict__ trial,
                                                  double *__restrict__ part) {
    KR_COORDS;
    if (skip && skip[b]) return;            // uniform over the workgroup
    __shared__ double sred[NPART * 4];
    const double s = s_tab[b], lo = opt_tab[b * OPT_STRIDE + OPT_UMIN], hi = opt_tab[b * OPT_STRIDE + OPT_UMAX];
    const double *const xs = ncg_slot(a, NCG_X);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    KR_NODES(
        const bool have_u = u && lvl < u_rows;
        const double uv = have_u ? u[o] : 0.0;
        const double xv = xs[o];
        const unsigned char fr = a.mask[o];
        const double v = uv + s * xv;
        double t = (v != v || v > lo) ? v : lo;
        t = (t != t || t < hi) ? t : hi;
        const bool moved = t != v;
        const bool pin = fr && t * uv < 0.0;
        t = pin ? 0.0 : t;
        trial[o] = t;
        const double d = t - uv;
        acc[0] += d * d;
        acc[1] += uv * uv;
        acc[2] += pin ? 1.0 : 0.0;
        acc[3] += moved ? 1.0 : 0.0;
    )
    const int op[4] = {0, 0, 0, 0};
    block_reduce_store<4>(acc, op, sred, my_part);
}

// The four sums of a trajectory's partials, one workgroup of NTH threads per trajectory, in the fixed order of kr_sum (a
// copy, as ncg_sum is, so that k_kr_fin and k_ncg_fin keep their registers).  out [B][4].
__global__ __launch_bounds__(NTH) void k_nt_fin(const double *__restrict__ part, long n, const int *__restrict__ skip,
                                                double *__restrict__ out) {
    __shared__ double sh[NTH];
    const int b = blockIdx.x;
    if (skip && skip[b]) return;
    const double *p = part + (long)b * n * 4;
    for (int slot = 0; slot < 4; ++slot) {
        double s = 0.0;
        for (long e = threadIdx.x; e < n; e += NTH) s += p[e * 4 + slot];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int h = NTH / 2; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[4 * b + slot] = sh[0];
        __syncthreads();
    }
}
