// vch_kernels1d.h — the 1D hot path (reference: src/1D/Vch_control_1D/{Forward_solver,
// backward_solver,cost_and_function,GD_1D}.py = F1, B1, C1, G1).
//
// One PERSISTENT workgroup per trajectory runs a whole time march (or adjoint sweep) on the
// device: the N+1 <= 4097 nodes of a trajectory are a few values per thread, all per-trajectory
// decisions (Newton stop test, step ceiling, Armijo) are workgroup reductions, and there is no
// host round trip inside a march.  Batches of trajectories fill the 256 CUs.
//
// Linear systems.  The reference solves the dense 2(N+1) Newton system and the dense (N+1)
// adjoint system with LAPACK dgesv (F1:185, B1:94,116).  Both are 2x2-block tridiagonal in the
// unknowns (dphi_i, dmu_i) resp. (p_i, q_i = -(Lp)_i):
//   Newton (F1:111-137):  [ -kappa/2 L + D   -1/2 I ] [dphi]   [-R_phi]
//                         [  I/dt            -1/2 L ] [dmu ] = [-R_mu ]
//   adjoint (B1:99-101):  [ I - tau L   -dt/2 (L - D) ] [p]   [rhs]
//                         [ L            I            ] [q] = [ 0 ]      (<=> (I - tau L + dt/2 L^2 - dt/2 D L) p = rhs)
// They are solved by cyclic reduction: the first LVL levels are formed on the fly from the
// analytic level-0 rows (constant off-diagonal blocks, diagonal block from phi_i), the remaining
// <= 1025 block rows live in LDS (14 doubles per row, SoA), log2 levels forward and backward, then
// the implicit levels are back-substituted.  Any N+1 works (missing neighbours = zero blocks).
#pragma once
#include "vch_common.h"
#include "vch_gp.h"

#ifndef VCH_T1
#define VCH_T1 512
#endif
constexpr int T1 = VCH_T1;              // threads per trajectory workgroup
constexpr int NR_MAX = 1025;            // block rows kept in LDS
constexpr double DSEP1 = 1e-2;          // F1:42

struct Phys1 {
    double tau, gamma, c1, c2, kappa, Lx;
};

struct M2 {            // 2x2 block, row-major
    double a, b, c, d;
};
struct V2 {
    double x, y;
};
__device__ __forceinline__ M2 mm(const M2 &p, const M2 &q) {
    return M2{p.a * q.a + p.b * q.c, p.a * q.b + p.b * q.d, p.c * q.a + p.d * q.c, p.c * q.b + p.d * q.d};
}
__device__ __forceinline__ V2 mv(const M2 &p, const V2 &v) { return V2{p.a * v.x + p.b * v.y, p.c * v.x + p.d * v.y}; }
__device__ __forceinline__ M2 minv(const M2 &p) {
    const double id = 1.0 / (p.a * p.d - p.b * p.c);
    return M2{p.d * id, -p.b * id, -p.c * id, p.a * id};
}
__device__ __forceinline__ M2 madd(const M2 &p, const M2 &q) { return M2{p.a + q.a, p.b + q.b, p.c + q.c, p.d + q.d}; }
__device__ __forceinline__ M2 mneg(const M2 &p) { return M2{-p.a, -p.b, -p.c, -p.d}; }

struct Row {           // A x_{i-s} + B x_i + C x_{i+s} = d
    M2 A, B, C;
    V2 d;
};

// Level-0 rows.  SYS 0: Newton system at iterate phi (F1:111-137); SYS 1: adjoint system at phi_n; SYS 2: the transpose of
// the Newton system (k1d_hessvec).  L is not symmetric (the mirrored rows 0 and n-1 carry a 2), so the transposed row i
// takes the weight of neighbour i-1 from row i-1's upper entry and that of neighbour i+1 from row i+1's lower entry; the
// diagonal 2x2 block is transposed, the off-diagonal blocks are diagonal.
struct SysArgs {
    const double *phi;       // D_i from phi_i
    const double *r0, *r1;   // right-hand side components (r1 may be NULL = 0)
    double dt, a;            // a = 1/h^2
    double tau, c1, c2, kappa;
    int n;
};

template <int SYS>
__device__ __forceinline__ Row row0(const SysArgs &S, int i) {
    const double fl = i == 0 ? 0.0 : (SYS == 2 ? (i == 1 ? 2.0 : 1.0) : (i == S.n - 1 ? 2.0 : 1.0));      // weight of neighbour i-1
    const double fu = i == S.n - 1 ? 0.0 : (SYS == 2 ? (i == S.n - 2 ? 2.0 : 1.0) : (i == 0 ? 2.0 : 1.0));  // weight of neighbour i+1
    Row R;
    const double ph = S.phi[i];
    if (SYS == 0 || SYS == 2) {
        const double D = S.tau / S.dt + 2.0 * S.c1 / (1.0 - ph * ph);           // F1:122-124 (not clipped)
        R.B = SYS == 0 ? M2{S.kappa * S.a + D, -0.5, 1.0 / S.dt, S.a} : M2{S.kappa * S.a + D, 1.0 / S.dt, -0.5, S.a};
        R.A = M2{-0.5 * S.kappa * S.a * fl, 0.0, 0.0, -0.5 * S.a * fl};
        R.C = M2{-0.5 * S.kappa * S.a * fu, 0.0, 0.0, -0.5 * S.a * fu};
    } else {
        const double p = fmin(fmax(ph, -1.0 + 1e-8), 1.0 - 1e-8);               // B1:45-46
        const double D = 2.0 * S.c1 / (1.0 - p * p) - 2.0 * S.c2;
        R.B = M2{1.0 + 2.0 * S.tau * S.a, 0.5 * S.dt * (2.0 * S.a + D), -2.0 * S.a, 1.0};
        R.A = M2{-S.tau * S.a * fl, -0.5 * S.dt * S.a * fl, S.a * fl, 0.0};
        R.C = M2{-S.tau * S.a * fu, -0.5 * S.dt * S.a * fu, S.a * fu, 0.0};
    }
    R.d = V2{S.r0[i], S.r1 ? S.r1[i] : 0.0};
    return R;
}

// one cyclic-reduction step: eliminate the neighbours lo and hi (where present) from row mid.  The neighbours are
// passed by value with presence flags: a `present ? &row : nullptr` argument makes the compiler keep the rows in
// private (scratch) memory, 232 bytes per lane and a memory round trip per field (profiles/r02_1d_scratch.txt).
__device__ __forceinline__ Row cr_reduce(bool hl, const Row &lo, const Row &mid, bool hh, const Row &hi) {
    Row R = mid;
    R.A = M2{0, 0, 0, 0};
    R.C = M2{0, 0, 0, 0};
    if (hl) {
        const M2 al = mneg(mm(mid.A, minv(lo.B)));
        R.A = mm(al, lo.A);
        R.B = madd(R.B, mm(al, lo.C));
        const V2 t = mv(al, lo.d);
        R.d.x += t.x; R.d.y += t.y;
    }
    if (hh) {
        const M2 ga = mneg(mm(mid.C, minv(hi.B)));
        R.C = mm(ga, hi.C);
        R.B = madd(R.B, mm(ga, hi.A));
        const V2 t = mv(ga, hi.d);
        R.d.x += t.x; R.d.y += t.y;
    }
    return R;
}

__device__ __forceinline__ Row row_identity() {          // placeholder for an absent neighbour (never used in arithmetic)
    return Row{M2{0, 0, 0, 0}, M2{1, 0, 0, 1}, M2{0, 0, 0, 0}, V2{0, 0}};
}

// row of the system at implicit level LVL (stride 2^LVL) centred at level-0 index i
template <int SYS, int LVL>
struct RowAt {
    static __device__ __forceinline__ Row get(const SysArgs &S, int i) {
        constexpr int s = 1 << (LVL - 1);
        const Row mid = RowAt<SYS, LVL - 1>::get(S, i);
        const bool hl = i - s >= 0, hh = i + s < S.n;
        const Row lo = hl ? RowAt<SYS, LVL - 1>::get(S, i - s) : row_identity();
        const Row hi = hh ? RowAt<SYS, LVL - 1>::get(S, i + s) : row_identity();
        return cr_reduce(hl, lo, mid, hh, hi);
    }
};
template <int SYS>
struct RowAt<SYS, 0> {
    static __device__ __forceinline__ Row get(const SysArgs &S, int i) { return row0<SYS>(S, i); }
};
template <int SYS>
__device__ __forceinline__ Row row_at(const SysArgs &S, int i, int lvl) {
    if (lvl == 0) return RowAt<SYS, 0>::get(S, i);
    if (lvl == 1) return RowAt<SYS, 1>::get(S, i);
    return RowAt<SYS, 2>::get(S, i);
}

// LDS image of the explicit rows: 14 arrays of NR_MAX doubles (A,B,C: 4 each; d: 2; x overwrites d)
struct CrLds {
    double *v;      // base
    // rows are XOR-swizzled inside their block of 32: the cyclic-reduction levels address rows at strides
    // 2, 4, ..., 1024, which un-swizzled fall on one or two LDS banks; (m >> 5) & 31 is 0 for m = 1024
    __device__ __forceinline__ double &at(int comp, int m) { return v[comp * NR_MAX + (m ^ ((m >> 5) & 31))]; }
    __device__ __forceinline__ Row load(int m) {
        Row R;
        R.A = M2{at(0, m), at(1, m), at(2, m), at(3, m)};
        R.B = M2{at(4, m), at(5, m), at(6, m), at(7, m)};
        R.C = M2{at(8, m), at(9, m), at(10, m), at(11, m)};
        R.d = V2{at(12, m), at(13, m)};
        return R;
    }
    __device__ __forceinline__ void store(int m, const Row &R) {
        at(0, m) = R.A.a; at(1, m) = R.A.b; at(2, m) = R.A.c; at(3, m) = R.A.d;
        at(4, m) = R.B.a; at(5, m) = R.B.b; at(6, m) = R.B.c; at(7, m) = R.B.d;
        at(8, m) = R.C.a; at(9, m) = R.C.b; at(10, m) = R.C.c; at(11, m) = R.C.d;
        at(12, m) = R.d.x; at(13, m) = R.d.y;
    }
};

// Solve the block-tridiagonal system; results x0[i], x1[i] (global).  All T1 threads of the
// workgroup must call it.  lvl = number of implicit levels (0..2), nr = rows kept in LDS.
template <int SYS>
__device__ void cr_solve(const SysArgs &S, int lvl, double *lds, double *x0, double *x1) {
    CrLds Q{lds};
    const int tid = threadIdx.x, n = S.n, st = 1 << lvl;
    const int nr = (n - 1) / st + 1;
    // explicit level: rows m <-> level-0 index m * st
    for (int m = tid; m < nr; m += T1) {
        Q.store(m, row_at<SYS>(S, m * st, lvl));
    }
    __syncthreads();
    int s = 1;
    for (; s < nr; s <<= 1) {                // forward reduction: rows m = 0, 2s, 4s, ...
        // row m is written by its owner only and rows m +- s are not touched at this level, so
        // the update is done in place without a barrier between loads and stores
        for (int m = tid * 2 * s; m < nr; m += T1 * 2 * s) {
            const Row mid = Q.load(m);
            const bool hl = m - s >= 0, hh = m + s < nr;
            const Row lo = hl ? Q.load(m - s) : row_identity();
            const Row hi = hh ? Q.load(m + s) : row_identity();
            Q.store(m, cr_reduce(hl, lo, mid, hh, hi));
        }
        __syncthreads();
    }
    if (tid == 0) {
        Row R = Q.load(0);
        V2 x = mv(minv(R.B), R.d);
        Q.at(12, 0) = x.x; Q.at(13, 0) = x.y;
    }
    __syncthreads();
    for (s >>= 1; s >= 1; s >>= 1) {         // back substitution: rows m = s, 3s, 5s, ...
        for (int m = s + tid * 2 * s; m < nr; m += T1 * 2 * s) {
            Row R = Q.load(m);
            V2 r = R.d;
            V2 t = mv(R.A, V2{Q.at(12, m - s), Q.at(13, m - s)});
            r.x -= t.x; r.y -= t.y;
            if (m + s < nr) {
                t = mv(R.C, V2{Q.at(12, m + s), Q.at(13, m + s)});
                r.x -= t.x; r.y -= t.y;
            }
            V2 x = mv(minv(R.B), r);
            Q.at(12, m) = x.x; Q.at(13, m) = x.y;
        }
        __syncthreads();
    }
    for (int m = tid; m < nr; m += T1) {
        x0[m * st] = Q.at(12, m);
        x1[m * st] = Q.at(13, m);
    }
    __syncthreads();
    // implicit levels: nodes i = s, 3s, ... with s = st/2, ..., 1
    for (int l = lvl - 1; l >= 0; --l) {
        const int sp = 1 << l;
        for (int i = sp + tid * 2 * sp; i < n; i += T1 * 2 * sp) {
            Row R = row_at<SYS>(S, i, l);
            V2 r = R.d;
            V2 t = mv(R.A, V2{x0[i - sp], x1[i - sp]});
            r.x -= t.x; r.y -= t.y;
            if (i + sp < n) {
                t = mv(R.C, V2{x0[i + sp], x1[i + sp]});
                r.x -= t.x; r.y -= t.y;
            }
            V2 x = mv(minv(R.B), r);
            x0[i] = x.x; x1[i] = x.y;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------
// workgroup reductions (T1 threads); result broadcast to all threads
// ---------------------------------------------------------------------------------
__device__ __forceinline__ double wsum1(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ double wmin1(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o, 64));
    return v;
}
__device__ __forceinline__ double wmax1(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    return v;
}
template <int OP>      // 0 sum, 1 min, 2 max
__device__ __forceinline__ double block_red(double v, double *s4) {
    v = OP == 0 ? wsum1(v) : (OP == 1 ? wmin1(v) : wmax1(v));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = s4[0];
    for (int w = 1; w < T1 / 64; ++w) r = OP == 0 ? r + s4[w] : (OP == 1 ? fmin(r, s4[w]) : fmax(r, s4[w]));
    return r;
}

__device__ __forceinline__ double lap1(const double *v, int i, int n, double a) {      // F1:64-80
    if (i == 0) return 2.0 * a * (v[1] - v[0]);
    if (i == n - 1) return 2.0 * a * (v[n - 2] - v[n - 1]);
    return a * ((v[i - 1] + v[i + 1]) - 2.0 * v[i]);
}
// transpose of lap1: (L^T v)_i = sum_j L_ji v_j; the 2 of the mirrored rows 0 and n-1 sits in columns 1 and n-2
__device__ __forceinline__ double lap1t(const double *v, int i, int n, double a) {
    const double lo = i == 0 ? 0.0 : (i == 1 ? 2.0 : 1.0) * v[i - 1];
    const double hi = i == n - 1 ? 0.0 : (i == n - 2 ? 2.0 : 1.0) * v[i + 1];
    return a * ((lo + hi) - 2.0 * v[i]);
}
__device__ __forceinline__ double reglog1(double phi) {                                  // F1:57-62
    const double eps = 0.5 * DSEP1;
    const double p = fmin(fmax(phi, -1.0 + eps), 1.0 - eps);
    return log((1.0 + p) / (1.0 - p));
}

// Scratch arrays of one trajectory (global memory, L2 resident): n doubles each.
struct Scr1 {
    double *phi, *mu, *w, *wnew, *phin, *mun, *phit, *mut, *dphi, *dmu, *cphi, *cmu, *rp, *rm;
};
constexpr int NSCR1 = 14;
__device__ __forceinline__ Scr1 scr_of(double *base, int b, int n) {
    double *q = base + (long)b * NSCR1 * n;
    return Scr1{q, q + n, q + 2 * n, q + 3 * n, q + 4 * n, q + 5 * n, q + 6 * n, q + 7 * n, q + 8 * n,
                q + 9 * n, q + 10 * n, q + 11 * n, q + 12 * n, q + 13 * n};
}

struct Newton1Stats {
    int iters;       // residual norms recorded
    int solves;
    int trials;
    int failed_ls;   // left through the line-search-failure return (F1:227-229)
    int error;       // 1 = non-finite mass defect (RuntimeError in the reference, F1:166-170)
};

// residual of (ph, mu_) with the old-level parts pre-combined in cphi, cmu; returns sum of squares
// over this thread's nodes; optionally stores -R into (rp, rm).
__device__ __forceinline__ double resid1(const Phys1 &P, int n, double a, double dt, const double *ph,
                                         const double *mu_, const double *cphi, const double *cmu, double *rp,
                                         double *rm, double *mass_defect_acc, double h) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += T1) {
        const double p = ph[i];
        const double Rp = (P.tau / dt) * p - 0.5 * P.kappa * lap1(ph, i, n, a) + P.c1 * reglog1(p) - 0.5 * mu_[i] + cphi[i];
        const double Rm = p / dt - 0.5 * lap1(mu_, i, n, a) + cmu[i];
        if (rp) { rp[i] = -Rp; rm[i] = -Rm; }
        if (mass_defect_acc) *mass_defect_acc += ((i == 0 || i == n - 1) ? 0.5 : 1.0) * h * Rm;
        acc += Rp * Rp + Rm * Rm;
    }
    return acc;
}

// One implicit time level (F1:139-235) for the trajectory owned by this workgroup.  On entry
// the old level is (S.phi, S.mu, S.w) and S.wnew holds w_new; on exit (S.phin, S.mun) hold the
// result.  hist (may be NULL) receives the residual norms.
__device__ void newton1(const Phys1 &P, int n, double h, double dt, int lvl, Scr1 &S, double *lds, double *s4,
                        double *hist, int hist_cap, Newton1Stats &ST) {
    const double a = 1.0 / (h * h);
    const int tid = threadIdx.x;
    // old-level parts of the residuals, initial guess (phi_old, mu_old) (F1:141-142)
    for (int i = tid; i < n; i += T1) {
        const double ph = S.phi[i];
        S.cphi[i] = -(P.tau / dt) * ph - 0.5 * P.kappa * lap1(S.phi, i, n, a) - 2.0 * P.c2 * ph - 0.5 * S.mu[i] -
                    0.5 * (S.wnew[i] + S.w[i]);
        S.cmu[i] = -ph / dt - 0.5 * lap1(S.mu, i, n, a);
        S.phin[i] = ph;
        S.mun[i] = S.mu[i];
    }
    __syncthreads();
    SysArgs A{S.phin, S.rp, S.rm, dt, a, P.tau, P.c1, P.c2, P.kappa, n};
    for (int k = 0; k < 50; ++k) {                                   // F1:144,156
        double md = 0.0;
        double ss = resid1(P, n, a, dt, S.phin, S.mun, S.cphi, S.cmu, S.rp, S.rm, (k % 10 == 0) ? &md : nullptr, h);
        const double nR = sqrt(block_red<0>(ss, s4));
        if (hist && tid == 0 && ST.iters < hist_cap) hist[ST.iters] = nR;
        ST.iters++;
        if (k % 10 == 0) {                                            // F1:166-170
            const double mdt = block_red<0>(md, s4);
            if (!isfinite(mdt)) { ST.error = 1; return; }
        }
        if (nR < 1e-6) return;                                        // F1:174
        __syncthreads();
        cr_solve<0>(A, lvl, lds, S.dphi, S.dmu);
        ST.solves++;
        // step ceiling (F1:194-212)
        double am = 1e300;
        for (int i = tid; i < n; i += T1) {
            const double d = S.dphi[i], ph = S.phin[i];
            if (d > 0.0) am = fmin(am, (1.0 - DSEP1 - ph) / d);
            else if (d < 0.0) am = fmin(am, (-1.0 + DSEP1 - ph) / d);
        }
        am = block_red<1>(am, s4);
        if (am >= 1e299) am = INFINITY;
        if (!isfinite(am) || am <= 0.0) am = 1.0;
        double alpha = fmin(1.0, 0.9 * am);
        bool accepted = false;
        for (int t = 0; t < 12; ++t) {                                // F1:216-226
            double mx = 0.0;
            for (int i = tid; i < n; i += T1) {
                const double pt = S.phin[i] + alpha * S.dphi[i];
                S.phit[i] = pt;
                S.mut[i] = S.mun[i] + alpha * S.dmu[i];
                mx = fmax(mx, fabs(pt));
            }
            mx = block_red<2>(mx, s4);            // (also orders the stores before the stencil reads)
            if (mx < 1.0 - DSEP1) {
                ST.trials++;
                const double st = resid1(P, n, a, dt, S.phit, S.mut, S.cphi, S.cmu, nullptr, nullptr, nullptr, h);
                const double nt = sqrt(block_red<0>(st, s4));
                if (nt <= (1.0 - 1e-3 * alpha) * nR) {
                    for (int i = tid; i < n; i += T1) { S.phin[i] = S.phit[i]; S.mun[i] = S.mut[i]; }
                    __syncthreads();
                    accepted = true;
                    break;
                }
            }
            alpha *= 0.5;
            __syncthreads();
        }
        if (!accepted) { ST.failed_ls = 1; return; }                  // F1:227-229
    }
}

// ---------------------------------------------------------------------------------
// persistent forward march (F1:286-386): grid = B workgroups
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(T1) void k1d_forward(Phys1 P, int n, double h, int lvl, int M, const double *__restrict__ dts,
                                                  const double *__restrict__ phi0, const double *u, int u_rows,
                                                  long u_stride, double *__restrict__ hist, long hist_stride,
                                                  double *scratch, int *__restrict__ stats /* [B][8] */,
                                                  const int *__restrict__ skip /* [B] or NULL */) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double s4[T1 / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (skip && skip[b]) return;            // line search already over for this trajectory (G1:98-108)
    Scr1 S = scr_of(scratch, b, n);
    const double a = 1.0 / (h * h);
    // phi = phi0, w = 0, mu = initialize_mu(phi, w) (F1:316-324), history rows 0 and 1 (F1:329-336)
    for (int i = tid; i < n; i += T1) {
        const double ph = phi0[(long)b * n + i];
        S.phi[i] = ph;
        S.w[i] = 0.0;
        if (hist) { hist[b * hist_stride + i] = ph; hist[b * hist_stride + n + i] = ph; }
    }
    __syncthreads();
    double ms = 0.0;
    for (int i = tid; i < n; i += T1) {
        const double ph = S.phi[i];
        S.mu[i] = -P.kappa * lap1(S.phi, i, n, a) + (P.c1 * reglog1(ph) - 2.0 * P.c2 * ph) - S.w[i];
        ms += ((i == 0 || i == n - 1) ? 0.5 : 1.0) * h * ph;
    }
    const double mass0 = block_red<0>(ms, s4);
    Newton1Stats ST{0, 0, 0, 0, 0};
    int nfail = 0;
    for (int step = 0; step < M; ++step) {
        const double dt = dts[step];
        const double gdt = P.gamma / dt;
        const double *un = nullptr, *u1 = nullptr;
        if (u) {                                                      // F1:347-353 (hold-last)
            un = u + b * u_stride + (long)step * n;
            u1 = step < u_rows - 1 ? un + n : un;
        }
        for (int i = tid; i < n; i += T1)
            S.wnew[i] = ((gdt - 0.5) * S.w[i] + 0.5 * ((u1 ? u1[i] : 0.0) + (un ? un[i] : 0.0))) / (gdt + 0.5);
        __syncthreads();
        ST.failed_ls = 0;
        newton1(P, n, h, dt, lvl, S, lds, s4, nullptr, 0, ST);
        nfail += ST.failed_ls;
        if (ST.error) break;
        __syncthreads();
        // clip, carry mu/w, uniform mass shift (F1:361-366), store
        double mc = 0.0;
        for (int i = tid; i < n; i += T1) {
            const double ph = fmin(fmax(S.phin[i], -1.0 + DSEP1), 1.0 - DSEP1);
            S.phi[i] = ph;
            S.mu[i] = S.mun[i];
            S.w[i] = S.wnew[i];
            mc += ((i == 0 || i == n - 1) ? 0.5 : 1.0) * h * ph;
        }
        const double shift = (block_red<0>(mc, s4) - mass0) / P.Lx;
        for (int i = tid; i < n; i += T1) {
            const double ph = S.phi[i] - shift;
            S.phi[i] = ph;
            if (hist) hist[b * hist_stride + (long)(step + 2) * n + i] = ph;
        }
        __syncthreads();
    }
    if (tid == 0) {
        stats[b * 8 + 0] = ST.iters; stats[b * 8 + 1] = ST.solves; stats[b * 8 + 2] = ST.trials;
        stats[b * 8 + 3] = nfail; stats[b * 8 + 4] = ST.error;
    }
}

// single Newton call (F1:139-235) for the parity tests: state preloaded in scratch (phi, mu, w, wnew)
__global__ __launch_bounds__(T1) void k1d_newton(Phys1 P, int n, double h, int lvl, double dt, double *scratch,
                                                 double *__restrict__ hist, int hist_cap, int *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double s4[T1 / 64];
    const int b = blockIdx.x;
    Scr1 S = scr_of(scratch, b, n);
    Newton1Stats ST{0, 0, 0, 0, 0};
    newton1(P, n, h, dt, lvl, S, lds, s4, hist ? hist + (long)b * hist_cap : nullptr, hist_cap, ST);
    if (threadIdx.x == 0) {
        stats[b * 8 + 0] = ST.iters; stats[b * 8 + 1] = ST.solves; stats[b * 8 + 2] = ST.trials;
        stats[b * 8 + 3] = ST.failed_ls; stats[b * 8 + 4] = ST.error;
    }
}

// stand-alone block-tridiagonal solves for the kernel-level parity tests
template <int SYS>
__global__ __launch_bounds__(T1) void k1d_solve(SysArgs A0, int lvl, const double *phi, const double *r0, const double *r1,
                                                double *x0, double *x1) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = blockIdx.x;
    SysArgs A = A0;
    A.phi = phi + (long)b * A.n;
    A.r0 = r0 + (long)b * A.n;
    A.r1 = r1 ? r1 + (long)b * A.n : nullptr;
    cr_solve<SYS>(A, lvl, lds, x0 + (long)b * A.n, x1 + (long)b * A.n);
}

// ---------------------------------------------------------------------------------
// persistent adjoint sweep (B1:48-126): rows = M+2 history rows; parameters are the frozen
// defaults of B1:29-33 (passed in F).  p, q, r histories [B][rows][n] must be zero-initialised.
// b1, b2 come from row blockIdx.x * opt_stride of a parameter table: the [B] table of vch1d_pgd_init_v (opt_stride =
// OPT1_STRIDE) or the one row the function seam fills from its scalar arguments (opt_stride = 0).  The index is
// wave-uniform, hence scalar loads, issued beside the kernel's other first loads; the arithmetic below is that of the
// scalar form.
// ---------------------------------------------------------------------------------
constexpr int OPT1_STRIDE = 6;          // one row of the table: {b1, b2, b3, kappa_sparsity, u_min, u_max}
enum { OPT1_B1 = 0, OPT1_B2, OPT1_B3, OPT1_KS, OPT1_UMIN, OPT1_UMAX };

__global__ __launch_bounds__(T1) void k1d_backward(Phys1 F, int n, double h, int lvl, int rows,
                                                   const double *__restrict__ t, const double *__restrict__ phi,
                                                   const double *__restrict__ phiQ, const double *__restrict__ phiT,
                                                   const double *__restrict__ opt_tab, int opt_stride, double *p,
                                                   double *q, double *r, long hs, double *scratch) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double b1 = opt_tab[b * opt_stride + OPT1_B1], b2 = opt_tab[b * opt_stride + OPT1_B2];
    const double a = 1.0 / (h * h);
    double *rhs = scratch + (long)b * NSCR1 * n, *x1 = rhs + n;
    const double *ph = phi + b * hs;
    const double *pq = phiQ ? phiQ + b * hs : nullptr;
    double *pp = p + b * hs, *qq = q + b * hs, *rr = r + b * hs;
    const int last = rows - 1;
    // terminal: (I - tau L) p = b2 (phi_M - phi_T); q = -L p; r = 0 (B1:93-96)
    for (int i = tid; i < n; i += T1) rhs[i] = b2 * (ph[(long)last * n + i] - (phiT ? phiT[(long)b * n + i] : 0.0));
    __syncthreads();
    SysArgs A{ph + (long)last * n, rhs, nullptr, 0.0, a, F.tau, F.c1, F.c2, 0.0, n};
    cr_solve<1>(A, lvl, lds, pp + (long)last * n, x1);
    for (int i = tid; i < n; i += T1) qq[(long)last * n + i] = -lap1(pp + (long)last * n, i, n, a);
    __syncthreads();
    for (int k = last - 1; k >= 0; --k) {
        const double dt = t[k + 1] - t[k];
        if (dt <= 0.0) continue;                                       // B1:110
        const double *pn = pp + (long)(k + 1) * n, *qn = qq + (long)(k + 1) * n, *rn = rr + (long)(k + 1) * n;
        const double *f0 = ph + (long)k * n, *f1 = ph + (long)(k + 1) * n;
        // rhs = B(phi_{k+1}) p_{k+1} + src,  B p = p + (tau - dt/2 D+) q + dt/2 L q  with q = -L p  (B1:103-113)
        for (int i = tid; i < n; i += T1) {
            const double pc = fmin(fmax(f1[i], -1.0 + 1e-8), 1.0 - 1e-8);
            const double Dp = 2.0 * F.c1 / (1.0 - pc * pc) - 2.0 * F.c2;
            const double src = 0.5 * dt * b1 * ((f0[i] - (pq ? pq[(long)k * n + i] : 0.0)) +
                                               (f1[i] - (pq ? pq[(long)(k + 1) * n + i] : 0.0)));
            rhs[i] = pn[i] + (F.tau - 0.5 * dt * Dp) * qn[i] + 0.5 * dt * lap1(qn, i, n, a) + src;
        }
        __syncthreads();
        SysArgs Ak{f0, rhs, nullptr, dt, a, F.tau, F.c1, F.c2, 0.0, n};
        cr_solve<1>(Ak, lvl, lds, pp + (long)k * n, x1);
        const double gb = (F.gamma - 0.5 * dt) / (F.gamma + 0.5 * dt), gs = (dt * 0.5) / (F.gamma + 0.5 * dt);
        for (int i = tid; i < n; i += T1) {
            const double qk = -lap1(pp + (long)k * n, i, n, a);       // B1:120
            qq[(long)k * n + i] = qk;
            rr[(long)k * n + i] = gb * rn[i] + gs * (qk + qn[i]);     // B1:122-124
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------
// persistent tangent march (vch1d_second_order): J'(u)h and J''(u)[h,h] of J1 + J2 + J3 about a state
// history.  grid = B workgroups, one direction each.  All tangent fields start at zero; step s takes history row s+1 to
// row s+2 with phi* = row s+2 and the direction rows (s, s+1):
//   dw'  = ((gamma/dt - 1/2) dw + 1/2 (h_{s+1} + h_s)) / (gamma/dt + 1/2)
//   J(phi*) [dphi*; dmu']   = [tau dphi/dt + kappa/2 L dphi + 2 c2 dphi + dmu/2 + (dw' + dw)/2 ;  dphi/dt + L dmu / 2]
//   J(phi*) [d2phi*; d2mu'] = [tau d2phi/dt + kappa/2 L d2phi + 2 c2 d2phi + d2mu/2 - c1 rho(phi*) dphi*^2 ;
//                              d2phi/dt + L d2mu / 2],      rho(p) = 4 p / (1 - p^2)^2
//   dphi' = dphi* - sum(wts dphi*) / Lx,  d2phi' = d2phi* - sum(wts d2phi*) / Lx,   wts = h trapz
// J is the Newton matrix of row0<0> (unclipped diagonal); the concave term -2 c2 phi_old is explicit in 1D (F1:99-109),
// hence on the right-hand side; the mean removal is the linearisation of the uniform mass shift (F1:366).  The clip of
// F1:361 is taken as the identity.  No Newton loop, no line search: two solves per step (one with ORDER 1).
// The level sums are folded into trapezoid sums over t in row order, every reduction in block_red's order: a
// trajectory's results do not depend on the batch.
// ---------------------------------------------------------------------------------
struct Tan1Args {
    const double *phi; long phi_s;      // base point: state history, stride per trajectory (0 = one base for the batch)
    const double *u; long u_s;          // control (or NULL = zeros)
    const double *pq; long pq_s;        // phi_Q (or NULL)
    const double *pt; long pt_s;        // phi_T (or NULL)
    const double *hd; long hs;          // direction [B][hs]
    const double *dts, *t, *wx, *wts;   // [rows-2], [rows], [n] trapezoid weights of the cost, [B][3] = {b1, b2, b3}
    double *d1, *d2;                    // tangent histories [B][hs] or NULL
    double *out;                        // [B][6]
};

template <int K>       // K sums at once, each in block_red<0>'s order; sk: K * (T1 / 64) doubles
__device__ __forceinline__ void block_sums(double (&v)[K], double *sk) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wsum1(v[k]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sk[k * (T1 / 64) + (threadIdx.x >> 6)] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double r = sk[k * (T1 / 64)];
        for (int w = 1; w < T1 / 64; ++w) r += sk[k * (T1 / 64) + w];
        v[k] = r;
    }
}

template <int ORDER>
__global__ __launch_bounds__(T1) void k1d_tangent(Phys1 P, int n, double h, int lvl, int rows, Tan1Args G, double *scratch) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double sk[5 * (T1 / 64)];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double a = 1.0 / (h * h);
    double *q = scratch + (long)b * NSCR1 * n;
    double *dphi = q, *dmu = q + n, *dw = q + 2 * n, *ephi = q + 3 * n, *emu = q + 4 * n, *rp = q + 5 * n, *rm = q + 6 * n,
           *nphi = q + 7 * n, *nmu = q + 8 * n, *rp2 = q + 9 * n, *rm2 = q + 10 * n, *nephi = q + 11 * n, *nemu = q + 12 * n;
    const double *ph = G.phi + b * G.phi_s;
    const double *uu = G.u ? G.u + b * G.u_s : nullptr;
    const double *pq = G.pq ? G.pq + b * G.pq_s : nullptr;
    const double *pt = G.pt ? G.pt + b * G.pt_s : nullptr;
    const double *hd = G.hd + b * G.hs;
    double *d1 = G.d1 ? G.d1 + b * G.hs : nullptr, *d2 = G.d2 ? G.d2 + b * G.hs : nullptr;
    for (int i = tid; i < n; i += T1) {
        dphi[i] = dmu[i] = dw[i] = ephi[i] = emu[i] = 0.0;
        if (d1) d1[i] = d1[n + i] = 0.0;
        if (d2) d2[i] = d2[n + i] = 0.0;
    }
    // S = {sum wx (phi - phi_Q) dphi, sum wx dphi^2, sum wx (phi - phi_Q) d2phi, sum wx u h, sum wx h^2} of one history row
    auto level = [&](int row, double (&S)[5]) {
        const long o = (long)row * n;
        S[0] = S[1] = S[2] = S[3] = S[4] = 0.0;
        for (int i = tid; i < n; i += T1) {
            const double w = G.wx[i], e = ph[o + i] - (pq ? pq[o + i] : 0.0), d = dphi[i], hh = hd[o + i];
            S[0] += w * (e * d);
            S[1] += w * (d * d);
            if (ORDER == 2) S[2] += w * (e * ephi[i]);
            S[3] += w * ((uu ? uu[o + i] : 0.0) * hh);
            S[4] += w * (hh * hh);
        }
        block_sums<5>(S, sk);
    };
    double I[5] = {0, 0, 0, 0, 0}, S0[5], S1[5];
    auto fold = [&](int row) {           // interval (row - 1, row) of the trapezoid rule in t (C1:55-73)
        const double d = G.t[row] - G.t[row - 1];
#pragma unroll
        for (int k = 0; k < 5; ++k) { I[k] += d * (S1[k] + S0[k]) / 2.0; S0[k] = S1[k]; }
    };
    level(0, S0);
    level(1, S1);
    fold(1);
    for (int s = 0; s < rows - 2; ++s) {
        const double dt = G.dts[s], gdt = P.gamma / dt;
        const double *ps = ph + (long)(s + 2) * n;
        const double *h0 = hd + (long)s * n, *h1 = h0 + n;
        for (int i = tid; i < n; i += T1) {
            const double wo = dw[i], wn = ((gdt - 0.5) * wo + 0.5 * (h1[i] + h0[i])) / (gdt + 0.5);
            const double d = dphi[i];
            rp[i] = (P.tau / dt) * d + 0.5 * P.kappa * lap1(dphi, i, n, a) + 2.0 * P.c2 * d + 0.5 * dmu[i] + 0.5 * (wn + wo);
            rm[i] = d / dt + 0.5 * lap1(dmu, i, n, a);
            dw[i] = wn;
            if (ORDER == 2) {
                const double e = ephi[i];
                rp2[i] = (P.tau / dt) * e + 0.5 * P.kappa * lap1(ephi, i, n, a) + 2.0 * P.c2 * e + 0.5 * emu[i];
                rm2[i] = e / dt + 0.5 * lap1(emu, i, n, a);
            }
        }
        __syncthreads();
        SysArgs A{ps, rp, rm, dt, a, P.tau, P.c1, P.c2, P.kappa, n};
        cr_solve<0>(A, lvl, lds, nphi, nmu);
        double ms = 0.0;
        for (int i = tid; i < n; i += T1) ms += ((i == 0 || i == n - 1) ? 0.5 : 1.0) * h * nphi[i];
        const double m1 = block_red<0>(ms, sk) / P.Lx;
        for (int i = tid; i < n; i += T1) {
            const double v = nphi[i];
            dphi[i] = v - m1;
            dmu[i] = nmu[i];
            if (d1) d1[(long)(s + 2) * n + i] = v - m1;
            if (ORDER == 2) {
                const double p = ps[i], om = 1.0 - p * p;
                rp2[i] -= P.c1 * (4.0 * p / (om * om)) * (v * v);
            }
        }
        __syncthreads();
        if (ORDER == 2) {
            SysArgs A2{ps, rp2, rm2, dt, a, P.tau, P.c1, P.c2, P.kappa, n};
            cr_solve<0>(A2, lvl, lds, nephi, nemu);
            double es = 0.0;
            for (int i = tid; i < n; i += T1) es += ((i == 0 || i == n - 1) ? 0.5 : 1.0) * h * nephi[i];
            const double m2 = block_red<0>(es, sk) / P.Lx;
            for (int i = tid; i < n; i += T1) {
                ephi[i] = nephi[i] - m2;
                emu[i] = nemu[i];
                if (d2) d2[(long)(s + 2) * n + i] = nephi[i] - m2;
            }
            __syncthreads();
        }
        level(s + 2, S1);
        fold(s + 2);
    }
    // terminal terms (C1:63): sum wx (phi_M - phi_T) dphi_M and the same with d2phi_M; sum wx dphi_M^2 is S0[1]
    double T[2] = {0.0, 0.0};
    const long ol = (long)(rows - 1) * n;
    for (int i = tid; i < n; i += T1) {
        const double w = G.wx[i], e = ph[ol + i] - (pt ? pt[i] : 0.0);
        T[0] += w * (e * dphi[i]);
        if (ORDER == 2) T[1] += w * (e * ephi[i]);
    }
    block_sums<2>(T, sk);
    if (tid == 0) {
        const double b1 = G.wts[3 * b], b2 = G.wts[3 * b + 1], b3 = G.wts[3 * b + 2];
        double *o = G.out + 6 * (long)b;
        o[0] = b1 * I[0] + b2 * T[0];
        o[1] = b3 * I[3];
        o[2] = b1 * I[1] + b2 * S0[1];
        o[3] = ORDER == 2 ? b1 * I[2] + b2 * T[1] : (double)NAN;
        o[4] = b3 * I[4];
        o[5] = I[4];
    }
}

// ---------------------------------------------------------------------------------
// exact discrete gradient and Hessian-vector product (vch1d_hessvec): the tangent step above is a linear
// map on (dphi, dmu, dw) driven by (h_s, h_{s+1}); its transpose run backwards over the steps, fed by the derivative of
// the cost with respect to the tangent state, is the exact adjoint of the discrete cost.  grid = B workgroups, one
// direction each.  With wx = h trapz, wt the trapezoid weights of t (row 0: 0), e = phi - phi_Q, al = (gamma/dt - 1/2) /
// (gamma/dt + 1/2), be = (1/2) / (gamma/dt + 1/2), Kp = (tau/dt + 2 c2) I + kappa/2 L, all multipliers zero at the start,
// G = b3 wt (x) wx . u, and for k = M-1 .. 0 (phi* = row k+2):
//   l_phi += wt[k+2] b1 wx . e[k+2]   (+ b2 wx . (phi_M - phi_T) at k = M-1)
//   l_v    = l_phi - wx sum(l_phi) / Lx                       (transpose of the mean removal; plain node sum)
//   J(phi*)^T [yp; ym] = [l_v; l_mu]                          (row0<2>)
//   l_dw   = yp/2 + l_w;   G[k] += be l_dw;   G[k+1] += be l_dw
//   (l_phi, l_mu, l_w) <- (Kp^T yp + ym/dt,  yp/2 + L^T ym / 2,  yp/2 + al l_dw)
// ORDER 2 first marches the order-1 tangent of h, keeping every step's dphi* BEFORE its mean removal (v_k, row k+2 of
// G.v) and the mean it removed (G.mean[k]), then runs a second sweep (capital letters) in lockstep, so yp is never stored:
//   L_phi += wt[k+2] b1 wx . dphi[k+2]   (+ b2 wx . dphi_M at k = M-1),      dphi[k+2] = v_k - mean_k
//   L_v    = L_phi - wx sum(L_phi) / Lx - c1 rho(phi*) yp v_k,               rho(p) = 4 p / (1 - p^2)^2
//   J(phi*)^T [Yp; Ym] = [L_v; L_mu];   Hh and (L_phi, L_mu, L_w) as above, Hh starting from b3 wt (x) wx . h.
// G and Hh are Euclidean derivatives with respect to the entries of u (no division by quadrature weights): row 0 has
// wt = 0 but drives step 0, the last row drives no step and keeps its b3 term alone.  One solve per step (ORDER 1), one
// tangent and two transposed solves (ORDER 2).  The clip is the identity, as in k1d_tangent.  Every reduction runs in
// block_red's order: a trajectory's results do not depend on the batch.
// ---------------------------------------------------------------------------------
struct Hv1Args {
    const double *phi; long phi_s;      // base point: state history, stride per trajectory (0 = one base for the batch)
    const double *u; long u_s;          // control (or NULL = zeros)
    const double *pq; long pq_s;        // phi_Q (or NULL)
    const double *pt; long pt_s;        // phi_T (or NULL)
    const double *hd; long hs;          // direction [B][hs] (NULL allowed with ORDER 1)
    const double *dts, *wt, *wx, *wts;  // [rows-2], [rows] trapezoid weights of t, [n] of x, [B][3] = {b1, b2, b3}
    double *g, *hv;                     // G, Hh [B][hs] (hv: ORDER 2)
    double *v, *mean;                   // ORDER 2: v_k [B][hs], removed means [B][rows]
    double *dots;                       // [B][2] = {sum G h, sum h Hh}
};

template <int ORDER>
__global__ __launch_bounds__(T1) void k1d_hessvec(Phys1 P, int n, double h, int lvl, int rows, Hv1Args G, double *scratch) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double sk[2 * (T1 / 64)];
    const int b = blockIdx.x, tid = threadIdx.x, M = rows - 2;
    const double a = 1.0 / (h * h);
    double *q = scratch + (long)b * NSCR1 * n;
    double *lphi = q, *lmu = q + n, *lw = q + 2 * n, *rv = q + 3 * n, *yp = q + 4 * n, *ym = q + 5 * n;
    double *Lphi = q + 6 * n, *Lmu = q + 7 * n, *Lw = q + 8 * n, *Rv = q + 9 * n, *Yp = q + 10 * n, *Ym = q + 11 * n;
    const double *ph = G.phi + b * G.phi_s;
    const double *uu = G.u ? G.u + b * G.u_s : nullptr;
    const double *pq = G.pq ? G.pq + b * G.pq_s : nullptr;
    const double *pt = G.pt ? G.pt + b * G.pt_s : nullptr;
    const double *hd = G.hd ? G.hd + b * G.hs : nullptr;
    double *g = G.g + b * G.hs, *hv = ORDER == 2 ? G.hv + b * G.hs : nullptr;
    double *vb = ORDER == 2 ? G.v + b * G.hs : nullptr, *mean = ORDER == 2 ? G.mean + (long)b * rows : nullptr;
    const double b1 = G.wts[3 * b], b2 = G.wts[3 * b + 1], b3 = G.wts[3 * b + 2];
    for (int row = 0; row < rows; ++row) {
        const long o = (long)row * n;
        const double wr = G.wt[row];
        for (int i = tid; i < n; i += T1) {
            const double w = b3 * (wr * G.wx[i]);
            g[o + i] = w * (uu ? uu[o + i] : 0.0);
            if (ORDER == 2) hv[o + i] = w * hd[o + i];
        }
    }
    if (ORDER == 2) {
        // the order-1 tangent march of k1d_tangent, on the planes the second sweep takes over afterwards
        double *dphi = Lphi, *dmu = Lmu, *dw = Lw, *rp = Rv, *rm = Yp, *nphi = Ym, *nmu = q + 12 * n;
        for (int i = tid; i < n; i += T1) dphi[i] = dmu[i] = dw[i] = 0.0;
        __syncthreads();
        for (int s = 0; s < M; ++s) {
            const double dt = G.dts[s], gdt = P.gamma / dt;
            const double *ps = ph + (long)(s + 2) * n;
            const double *h0 = hd + (long)s * n, *h1 = h0 + n;
            for (int i = tid; i < n; i += T1) {
                const double wo = dw[i], wn = ((gdt - 0.5) * wo + 0.5 * (h1[i] + h0[i])) / (gdt + 0.5);
                const double d = dphi[i];
                rp[i] = (P.tau / dt) * d + 0.5 * P.kappa * lap1(dphi, i, n, a) + 2.0 * P.c2 * d + 0.5 * dmu[i] + 0.5 * (wn + wo);
                rm[i] = d / dt + 0.5 * lap1(dmu, i, n, a);
                dw[i] = wn;
            }
            __syncthreads();
            SysArgs A{ps, rp, rm, dt, a, P.tau, P.c1, P.c2, P.kappa, n};
            cr_solve<0>(A, lvl, lds, nphi, nmu);
            double ms = 0.0;
            for (int i = tid; i < n; i += T1) ms += ((i == 0 || i == n - 1) ? 0.5 : 1.0) * h * nphi[i];
            const double m1 = block_red<0>(ms, sk) / P.Lx;
            for (int i = tid; i < n; i += T1) {
                const double v = nphi[i];
                vb[(long)(s + 2) * n + i] = v;
                dphi[i] = v - m1;
                dmu[i] = nmu[i];
            }
            if (tid == 0) mean[s] = m1;
            __syncthreads();
        }
    }
    for (int i = tid; i < n; i += T1) {
        lphi[i] = lmu[i] = lw[i] = 0.0;
        if (ORDER == 2) Lphi[i] = Lmu[i] = Lw[i] = 0.0;
    }
    __syncthreads();
    for (int k = M - 1; k >= 0; --k) {
        const double dt = G.dts[k], gdt = P.gamma / dt, al = (gdt - 0.5) / (gdt + 0.5), be = 0.5 / (gdt + 0.5);
        const long o = (long)(k + 2) * n;
        const double *ps = ph + o;
        const double wb = G.wt[k + 2] * b1, mk = ORDER == 2 ? mean[k] : 0.0;
        const bool term = k == M - 1;
        double S[ORDER];
        for (int j = 0; j < ORDER; ++j) S[j] = 0.0;
        for (int i = tid; i < n; i += T1) {
            const double w = G.wx[i], p = ps[i];
            double l = lphi[i] + wb * (w * (p - (pq ? pq[o + i] : 0.0)));
            if (term) l += b2 * (w * (p - (pt ? pt[i] : 0.0)));
            lphi[i] = l;
            S[0] += l;
            if (ORDER == 2) {
                const double d = vb[o + i] - mk;
                double L = Lphi[i] + wb * (w * d);
                if (term) L += b2 * (w * d);
                Lphi[i] = L;
                S[ORDER - 1] += L;
            }
        }
        block_sums<ORDER>(S, sk);
        for (int i = tid; i < n; i += T1) rv[i] = lphi[i] - G.wx[i] * (S[0] / P.Lx);
        __syncthreads();
        SysArgs A{ps, rv, lmu, dt, a, P.tau, P.c1, P.c2, P.kappa, n};
        cr_solve<2>(A, lvl, lds, yp, ym);
        if (ORDER == 2) {
            for (int i = tid; i < n; i += T1) {
                const double p = ps[i], om = 1.0 - p * p;
                Rv[i] = (Lphi[i] - G.wx[i] * (S[ORDER - 1] / P.Lx)) - P.c1 * (4.0 * p / (om * om)) * (yp[i] * vb[o + i]);
            }
            __syncthreads();
            SysArgs A2{ps, Rv, Lmu, dt, a, P.tau, P.c1, P.c2, P.kappa, n};
            cr_solve<2>(A2, lvl, lds, Yp, Ym);
        }
        // the multipliers of the step before, and this step's share of rows k and k+1 (each thread its own nodes)
        const double kd = P.tau / dt + 2.0 * P.c2;
        for (int i = tid; i < n; i += T1) {
            const double y = yp[i], ldw = 0.5 * y + lw[i];
            g[(long)k * n + i] += be * ldw;
            g[(long)(k + 1) * n + i] += be * ldw;
            lphi[i] = kd * y + 0.5 * P.kappa * lap1t(yp, i, n, a) + ym[i] / dt;
            lmu[i] = 0.5 * y + 0.5 * lap1t(ym, i, n, a);
            lw[i] = 0.5 * y + al * ldw;
            if (ORDER == 2) {
                const double Y = Yp[i], Ldw = 0.5 * Y + Lw[i];
                hv[(long)k * n + i] += be * Ldw;
                hv[(long)(k + 1) * n + i] += be * Ldw;
                Lphi[i] = kd * Y + 0.5 * P.kappa * lap1t(Yp, i, n, a) + Ym[i] / dt;
                Lmu[i] = 0.5 * Y + 0.5 * lap1t(Ym, i, n, a);
                Lw[i] = 0.5 * Y + al * Ldw;
            }
        }
        __syncthreads();
    }
    // sum G h and sum h Hh as plain node sums: rows in order per thread, then one reduction
    double D[2] = {0.0, 0.0};
    if (hd)
        for (int row = 0; row < rows; ++row) {
            const long o = (long)row * n;
            for (int i = tid; i < n; i += T1) {
                const double hh = hd[o + i];
                D[0] += g[o + i] * hh;
                if (ORDER == 2) D[1] += hh * hv[o + i];
            }
        }
    block_sums<2>(D, sk);
    if (tid == 0) {
        G.dots[2 * b] = hd ? D[0] : (double)NAN;
        G.dots[2 * b + 1] = ORDER == 2 ? D[1] : (double)NAN;
    }
}

// ---------------------------------------------------------------------------------
// element-wise / reduction kernels: Laplacian, residuals, cost (C1:55-73), gradient+prox
// (C1:99,111, G1:68-70); grid = (rows or 1, B)
// ---------------------------------------------------------------------------------
__global__ void k1d_lap(int n, double a, const double *__restrict__ v, double *__restrict__ out) {
    const long o = (long)blockIdx.y * n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[o + i] = lap1(v + o, i, n, a);
}

__global__ void k1d_residuals(Phys1 P, int n, double a, double dt, const double *pn, const double *po, const double *mn,
                              const double *mo, const double *wn, const double *wo, double *Rp, double *Rm) {
    const long o = (long)blockIdx.y * n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        Rp[o + i] = (P.tau * (pn[o + i] - po[o + i]) / dt) - 0.5 * P.kappa * (lap1(pn + o, i, n, a) + lap1(po + o, i, n, a)) +
                    (P.c1 * reglog1(pn[o + i]) + (-2.0 * P.c2 * po[o + i])) - 0.5 * (mn[o + i] + mo[o + i]) -
                    0.5 * (wn[o + i] + wo[o + i]);
        Rm[o + i] = (pn[o + i] - po[o + i]) / dt - 0.5 * (lap1(mn + o, i, n, a) + lap1(mo + o, i, n, a));
    }
}

// per (trajectory, row): sum wx (phi-phiQ)^2, sum wx (phi - phiT)^2 (last row), sum wx u^2, sum wx |u|
__global__ __launch_bounds__(T1) void k1d_cost(int n, int rows, const double *__restrict__ wx, const double *__restrict__ phi,
                                               const double *__restrict__ u, const double *__restrict__ pq,
                                               const double *__restrict__ pt, long hs, double *__restrict__ out) {
    __shared__ double s4[T1 / 64];
    const int row = blockIdx.x, b = blockIdx.y;
    const long o = b * hs + (long)row * n;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = threadIdx.x; i < n; i += T1) {
        const double w = wx[i], ph = phi[o + i], uu = u ? u[o + i] : 0.0;
        const double e = ph - (pq ? pq[o + i] : 0.0);
        a0 += w * (e * e);
        a2 += w * (uu * uu);
        a3 += w * fabs(uu);
        if (row == rows - 1) {
            const double e2 = ph - (pt ? pt[(long)b * n + i] : 0.0);
            a1 += w * (e2 * e2);
        }
    }
    a0 = block_red<0>(a0, s4); a1 = block_red<0>(a1, s4); a2 = block_red<0>(a2, s4); a3 = block_red<0>(a3, s4);
    if (threadIdx.x == 0) {
        double *q = out + ((long)b * rows + row) * 4;
        q[0] = a0; q[1] = a1; q[2] = a2; q[3] = a3;
    }
}

// prox(u - alpha (r + b3 u)): gradient step (C1:99, C1:111), soft threshold alpha ks, box (G1:68-70)
__device__ __forceinline__ double grad_prox1(double uu, double rr, double al, double b3, double ks, double umin, double umax) {
    const double v = uu - al * (rr + b3 * uu);
    const double sg = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
    return fmin(fmax(sg * fmax(fabs(v) - al * ks, 0.0), umin), umax);
}

// b3, ks, umin, umax: row blockIdx.y * opt_stride of the parameter table (see k1d_backward)
__global__ __launch_bounds__(T1) void k1d_grad_prox(int n, const double *__restrict__ u, const double *__restrict__ r, long hs,
                                                    const double *__restrict__ alpha, const double *__restrict__ opt_tab,
                                                    int opt_stride, double *__restrict__ uout, double *__restrict__ chg) {
    __shared__ double s4[T1 / 64];
    const int row = blockIdx.x, b = blockIdx.y, rows = gridDim.x;
    const double *ot = opt_tab + b * opt_stride;
    const double b3 = ot[OPT1_B3], ks = ot[OPT1_KS], umin = ot[OPT1_UMIN], umax = ot[OPT1_UMAX];
    const long o = b * hs + (long)row * n;
    const double al = alpha[b];
    double d2 = 0, n2 = 0;
    for (int i = threadIdx.x; i < n; i += T1) {
        const double uu = u[o + i];
        const double un = grad_prox1(uu, r[o + i], al, b3, ks, umin, umax);
        uout[o + i] = un;
        d2 += (un - uu) * (un - uu);
        n2 += uu * uu;
    }
    d2 = block_red<0>(d2, s4); n2 = block_red<0>(n2, s4);
    if (chg && threadIdx.x == 0) { chg[((long)b * rows + row) * 2] = d2; chg[((long)b * rows + row) * 2 + 1] = n2; }
}

// KKT sparsity statistic of one trajectory (verify_sparsity_condition, G1:115-147) and the two squared norms of the
// stationarity measure ||prox_1(u) - u|| / (||u|| + 1e-9), prox_1 = grad_prox1 with alpha = 1.  grid = B workgroups of T1
// threads, each striding over the rows * n nodes of its trajectory (the duplicated t = 0 row included).  A thread's counts
// are integers below 2^31, their sums go through block_red as doubles, where integers up to 2^53 add exactly in any
// order; the norms take block_red's fixed order.  Writes cnt [B][4] = {#|u| < tol, #|r| <= ks, #agree, #nodes} and
// nrm [B][2] = {||prox_1(u) - u||^2, ||u||^2} and nothing else: the prox image is not stored.
__global__ __launch_bounds__(T1) void k1d_kkt(int n, int rows, const double *__restrict__ u, const double *__restrict__ r,
                                              long hs, const double *__restrict__ opt_tab, double tol,
                                              long long *__restrict__ cnt, double *__restrict__ nrm) {
    __shared__ double s4[T1 / 64];
    const int b = blockIdx.x;
    const double *ot = opt_tab + b * OPT1_STRIDE;
    const double b3 = ot[OPT1_B3], ks = ot[OPT1_KS], umin = ot[OPT1_UMIN], umax = ot[OPT1_UMAX];
    const long o = b * hs, tot = (long)rows * n;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    double d2 = 0, n2 = 0;
    for (long i = threadIdx.x; i < tot; i += T1) {
        const double uu = u[o + i], rr = r[o + i];
        const bool zero = fabs(uu) < tol, small = fabs(rr) <= ks;
        c0 += zero; c1 += small; c2 += (zero == small); c3 += 1;
        const double un = grad_prox1(uu, rr, 1.0, b3, ks, umin, umax);
        d2 += (un - uu) * (un - uu);
        n2 += uu * uu;
    }
    const double s0 = block_red<0>((double)c0, s4), s1 = block_red<0>((double)c1, s4), s2 = block_red<0>((double)c2, s4),
                 s3 = block_red<0>((double)c3, s4);
    d2 = block_red<0>(d2, s4); n2 = block_red<0>(n2, s4);
    if (threadIdx.x == 0) {
        cnt[4 * b] = (long long)s0; cnt[4 * b + 1] = (long long)s1; cnt[4 * b + 2] = (long long)s2; cnt[4 * b + 3] = (long long)s3;
        nrm[2 * b] = d2; nrm[2 * b + 1] = n2;
    }
}

// ---------------------------------------------------------------------------------
// Directional sparsity: the prox of kappa_s * sum over groups of ||u_g|| under the box, a group being a row
// of the control (VCH_SPARSITY_TIME, ||z||^2 = sum_i wx_i z_i^2) or a column (VCH_SPARSITY_SPACE, ||z||^2 = sum_k wt_k z_k^2).
// With v = u - alpha (r + b3 u) and lam = alpha kappa_s:  c = ||cone(v)|| <= lam gives u+ = 0, s = 0; otherwise
// u+ = clip(s v) with s the root of h(s) = ||clip(s v)|| (1 - s) - lam s, which is s0 = 1 - lam / ||v|| where clip(s0 v) = s0 v.
// No atomics; every sum has one fixed order, so a trajectory's bits do not depend on the batch it runs in.
// ---------------------------------------------------------------------------------
constexpr int GP_NV = (4096 + 1 + T1 - 1) / T1;            // values of a row per thread at the largest N
constexpr int GC_W = 16, GC_T = 64 * GC_W;                 // the column kernels: 64 columns across the lanes, rows over GC_W waves
// values per thread the rows kernel is instantiated with: the smallest of 1, 2, 4, GP_NV that holds a row of n nodes (a short
// row in a kernel built for the longest would leave most registers, and with them most of the CU, idle)
inline int gp_rows_nv(int n) {
    const int nv = (n + T1 - 1) / T1;
    return nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 && 4 < GP_NV ? 4 : GP_NV));
}

// gp_v, gp_cone, gp_out and gp_step, the prox of one group whatever its norm, are in vch_gp.h (shared with the 2D kernels)

// TIME: one workgroup per (row, trajectory), the row's v, weights and u in registers (NV each, fully unrolled; NV * T1 >= n,
// gp_rows_nv): one read of u and r, one write of u+.  The sums add the nodes in index order whatever NV is.  mode (or NULL: every trajectory): [B], a trajectory of another mode is left alone.
// sout (or NULL): s of the group at [b * ss + row]; uout (or NULL: the sums alone); chg (or NULL): the sums of k1d_grad_prox.
template <int NV>
__global__ __launch_bounds__(T1) void k1d_group_prox_rows(int n, const double *__restrict__ u, const double *__restrict__ r, long hs,
                                                          const double *__restrict__ alpha, const double *__restrict__ opt_tab,
                                                          int opt_stride, const int *__restrict__ mode,
                                                          const double *__restrict__ wx, double *__restrict__ uout,
                                                          double *__restrict__ sout, long ss, double *__restrict__ chg) {
    __shared__ double sk[3 * (T1 / 64)];
    __shared__ double bc[2];
    const int row = blockIdx.x, b = blockIdx.y, rows = gridDim.x, tid = threadIdx.x;
    if (mode && mode[b] != GP_TIME) return;
    const double *ot = opt_tab + b * opt_stride;
    const double b3 = ot[OPT1_B3], ks = ot[OPT1_KS], umin = ot[OPT1_UMIN], umax = ot[OPT1_UMAX];
    const long o = b * hs + (long)row * n;
    const double al = alpha[b], lam = al * ks;
    double v[NV], w[NV], uu[NV];
    double a3[3] = {0.0, 0.0, 0.0};           // ||cone(v)||^2, ||v||^2, sum u^2
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = tid + k * T1;
        uu[k] = 0.0; w[k] = 0.0; v[k] = 0.0;
        if (i < n) {
            uu[k] = u[o + i];
            w[k] = wx[i];
            v[k] = gp_v(uu[k], r[o + i], al, b3);
        }
        const double cv = gp_cone(v[k], umin, umax);
        a3[0] += w[k] * (cv * cv);
        a3[1] += w[k] * (v[k] * v[k]);
        a3[2] += uu[k] * uu[k];
    }
    block_sums<3>(a3, sk);
    double s = 0.0;
    if (sqrt(a3[0]) > lam) {                  // the same in every thread: the sums are broadcast
        s = 1.0 - lam / sqrt(a3[1]);
        double out = 0.0;                     // the vote: does s0 leave the box inactive?
#pragma unroll
        for (int k = 0; k < NV; ++k) out = (s * v[k] < umin || s * v[k] > umax) ? 1.0 : out;
        if (block_red<2>(out, sk) != 0.0) {
            double lo = 0.0, hi = 1.0;        // thread 0's
            for (int it = 0; it < GP_MAXIT; ++it) {
                double qa[2] = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const double sv = s * v[k], cl = fmin(fmax(sv, umin), umax);
                    qa[0] += w[k] * (cl * cl);
                    qa[1] += cl == sv ? w[k] * (v[k] * v[k]) : 0.0;
                }
                block_sums<2>(qa, sk);
                if (tid == 0) {
                    const bool done = gp_step(qa[0], qa[1], lam, s, lo, hi);
                    bc[0] = s; bc[1] = done ? 1.0 : 0.0;
                }
                __syncthreads();              // the next write of bc comes after the two barriers of block_sums
                s = bc[0];
                if (bc[1] != 0.0) break;
            }
        }
    }
    double d2 = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = tid + k * T1;
        const double un = gp_out(s, v[k], umin, umax);
        if (i < n) {
            if (uout) uout[o + i] = un;
            d2 += (un - uu[k]) * (un - uu[k]);
        }
    }
    d2 = block_red<0>(d2, sk);
    if (tid == 0) {
        if (sout) sout[b * ss + row] = s;
        if (chg) { chg[((long)b * rows + row) * 2] = d2; chg[((long)b * rows + row) * 2 + 1] = a3[2]; }
    }
}

// SPACE: one workgroup of GC_W waves per (64 columns, trajectory); lane = column, so every row read is coalesced; wave w
// takes rows w, w + GC_W, ... and the waves' partial sums are added in wave order.  Pass one: ||cone(v)||^2, ||v||^2 and the extremes of
// v, which say whether s0 leaves the box inactive (s0 v is monotone in v).  Columns the box holds iterate together, each
// step re-reading the column; the last pass writes u+.  chg (or NULL): [B][gridDim.x][2], this workgroup's share of
// sum (u+ - u)^2 and sum u^2; sout (or NULL): s at [b * ss + column].
__global__ __launch_bounds__(GC_T) void k1d_group_prox_cols(int n, int rows, const double *__restrict__ u, const double *__restrict__ r,
                                                            long hs, const double *__restrict__ alpha,
                                                            const double *__restrict__ opt_tab, int opt_stride,
                                                            const int *__restrict__ mode, const double *__restrict__ wt,
                                                            double *__restrict__ uout, double *__restrict__ sout, long ss,
                                                            double *__restrict__ chg) {
    __shared__ double part[4][GC_W][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (mode && mode[b] != GP_SPACE) return;
    const int i = blockIdx.x * 64 + lane;
    const bool ok = i < n;
    const double *ot = opt_tab + b * opt_stride;
    const double b3 = ot[OPT1_B3], ks = ot[OPT1_KS], umin = ot[OPT1_UMIN], umax = ot[OPT1_UMAX];
    const long o = b * hs + i;
    const double al = alpha[b], lam = al * ks;
    double cc = 0.0, vv = 0.0, mx = 0.0, mn = 0.0;
    if (ok) {
#pragma unroll 4
        for (int k = wv; k < rows; k += GC_W) {
            const double uu = u[o + (long)k * n], v = gp_v(uu, r[o + (long)k * n], al, b3), w = wt[k];
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
    for (int w = 1; w < GC_W; ++w) {
        cc += part[0][w][lane]; vv += part[1][w][lane];
        mx = fmax(mx, part[2][w][lane]); mn = fmin(mn, part[3][w][lane]);
    }
    // from here on the waves hold the same numbers for a column and take the same steps
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
            for (int k = wv; k < rows; k += GC_W) {
                const double uu = u[o + (long)k * n], v = gp_v(uu, r[o + (long)k * n], al, b3), w = wt[k];
                const double sv = s * v, cl = fmin(fmax(sv, umin), umax);
                q += w * (cl * cl);
                a += cl == sv ? w * (v * v) : 0.0;
            }
        }
        part[0][wv][lane] = q; part[1][wv][lane] = a;
        __syncthreads();
        if (active) {
            q = part[0][0][lane]; a = part[1][0][lane];
            for (int w = 1; w < GC_W; ++w) { q += part[0][w][lane]; a += part[1][w][lane]; }
            active = !gp_step(q, a, lam, s, lo, hi);
        }
    }
    double d2 = 0.0, n2 = 0.0;
    if (ok) {
#pragma unroll 4
        for (int k = wv; k < rows; k += GC_W) {
            const double uu = u[o + (long)k * n], v = gp_v(uu, r[o + (long)k * n], al, b3);
            const double un = gp_out(s, v, umin, umax);
            if (uout) uout[o + (long)k * n] = un;
            d2 += (un - uu) * (un - uu);
            n2 += uu * uu;
        }
    }
    if (ok && wv == 0 && sout) sout[b * ss + i] = s;
    if (!chg) return;
    d2 = wsum1(d2); n2 = wsum1(n2);
    __syncthreads();
    if (lane == 0) { part[0][wv][0] = d2; part[1][wv][0] = n2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        d2 = part[0][0][0]; n2 = part[1][0][0];
        for (int w = 1; w < GC_W; ++w) { d2 += part[0][w][0]; n2 += part[1][w][0]; }
        double *q = chg + ((long)b * gridDim.x + blockIdx.x) * 2;
        q[0] = d2; q[1] = n2;
    }
}

// out [B][n] = sum_k wt_k u_{k,i}^2, the squared column norms of the SPACE cost, in the order of the kernel above
__global__ __launch_bounds__(GC_T) void k1d_colnorm(int n, int rows, const double *__restrict__ u, long hs, const int *__restrict__ mode,
                                                    const double *__restrict__ wt, double *__restrict__ out) {
    __shared__ double part[GC_W][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (mode && mode[b] != GP_SPACE) return;
    const int i = blockIdx.x * 64 + lane;
    double a = 0.0;
    if (i < n) {
#pragma unroll 4
        for (int k = wv; k < rows; k += GC_W) {
            const double uu = u[b * hs + (long)k * n + i];
            a += wt[k] * (uu * uu);
        }
    }
    part[wv][lane] = a;
    __syncthreads();
    if (wv == 0 && i < n) {
        a = part[0][lane];
        for (int w = 1; w < GC_W; ++w) a += part[w][lane];
        out[(long)b * n + i] = a;
    }
}

// The KKT statistic by groups, one workgroup per trajectory of a group mode (the others are left to k1d_kkt): cnt [B][4] =
// {#groups ||u_g|| < tol, #groups ||r_g|| <= kappa_s, #agree, #groups} in the group's norm, and nrm [B][2] = the change sums
// of the mode's prox at alpha = 1, which the prox kernel left as partials (chg_t [B][rows][2] of the rows kernel, chg_s
// [B][nblk][2] of the column kernel), added here in index order.
__global__ __launch_bounds__(T1) void k1d_kkt_g(int n, int rows, const double *__restrict__ u, const double *__restrict__ r, long hs,
                                                const double *__restrict__ opt_tab, const int *__restrict__ mode,
                                                const double *__restrict__ wx, const double *__restrict__ wt, double tol,
                                                const double *__restrict__ chg_t, const double *__restrict__ chg_s, int nblk,
                                                long long *__restrict__ cnt, double *__restrict__ nrm) {
    __shared__ double sk[3 * (T1 / 64)];
    const int b = blockIdx.x, tid = threadIdx.x, m = mode[b];
    if (m != GP_TIME && m != GP_SPACE) return;
    const double ks = opt_tab[b * OPT1_STRIDE + OPT1_KS];
    const long o = b * hs;
    double c3[3] = {0.0, 0.0, 0.0};
    if (m == GP_TIME) {
        for (int k = 0; k < rows; ++k) {
            double a2[2] = {0.0, 0.0};
            for (int i = tid; i < n; i += T1) {
                const double uu = u[o + (long)k * n + i], rr = r[o + (long)k * n + i], w = wx[i];
                a2[0] += w * (uu * uu);
                a2[1] += w * (rr * rr);
            }
            block_sums<2>(a2, sk);
            const bool zero = sqrt(a2[0]) < tol, small = sqrt(a2[1]) <= ks;
            c3[0] += zero; c3[1] += small; c3[2] += (zero == small);
        }
    } else {
        for (int i = tid; i < n; i += T1) {
            double a0 = 0.0, a1 = 0.0;
            for (int k = 0; k < rows; ++k) {
                const double uu = u[o + (long)k * n + i], rr = r[o + (long)k * n + i], w = wt[k];
                a0 += w * (uu * uu);
                a1 += w * (rr * rr);
            }
            const bool zero = sqrt(a0) < tol, small = sqrt(a1) <= ks;
            c3[0] += zero; c3[1] += small; c3[2] += (zero == small);
        }
        block_sums<3>(c3, sk);                // counts: integers add exactly in any order
    }
    if (tid == 0) {
        const int ng = m == GP_TIME ? rows : n, np = m == GP_TIME ? rows : nblk;
        const double *q = (m == GP_TIME ? chg_t : chg_s) + (long)b * np * 2;
        double d2 = 0.0, n2 = 0.0;
        for (int j = 0; j < np; ++j) { d2 += q[2 * j]; n2 += q[2 * j + 1]; }
        cnt[4 * b] = (long long)c3[0]; cnt[4 * b + 1] = (long long)c3[1]; cnt[4 * b + 2] = (long long)c3[2]; cnt[4 * b + 3] = ng;
        nrm[2 * b] = d2; nrm[2 * b + 1] = n2;
    }
}

// phi_Q = (1 - t/T) phi_initial + (t/T) phi_T, phi_initial = history row 0 (build_targets_1d, G1:238-241)
__global__ __launch_bounds__(T1) void k1d_ramp(int n, const double *__restrict__ tp, const double *__restrict__ phi_hist,
                                               const double *__restrict__ phiT, long hs, double *__restrict__ phiQ) {
    const int row = blockIdx.x, b = blockIdx.y;
    const double f = tp[row];
    for (int i = threadIdx.x; i < n; i += T1)
        phiQ[b * hs + (long)row * n + i] = (1.0 - f) * phi_hist[b * hs + i] + f * phiT[(long)b * n + i];
}

// free energy of every level of a history (F1:243-262): partial sums {sum dphi^2, sum W psi, sum W w phi}
__global__ __launch_bounds__(T1) void k1d_energy(int n, double c1, double c2, double eps, const double *__restrict__ phi,
                                                 const double *__restrict__ w, long hs, double *__restrict__ out) {
    __shared__ double s4[T1 / 64];
    const int row = blockIdx.x, b = blockIdx.y, rows = gridDim.x;
    const long o = b * hs + (long)row * n;
    double a0 = 0, a1 = 0, a2 = 0;
    for (int i = threadIdx.x; i < n; i += T1) {
        const double a = phi[o + i];
        if (i + 1 < n) { const double d = phi[o + i + 1] - a; a0 += d * d; }
        const double wt = (i == 0 || i == n - 1) ? 0.5 : 1.0;
        const double p = fmin(fmax(a, -1.0 + eps), 1.0 - eps);
        a1 += wt * (c1 * ((1.0 + p) * log(1.0 + p) + (1.0 - p) * log(1.0 - p)) - c2 * (p * p));
        if (w) a2 += wt * (w[o + i] * a);
    }
    a0 = block_red<0>(a0, s4); a1 = block_red<0>(a1, s4); a2 = block_red<0>(a2, s4);
    if (threadIdx.x == 0) {
        double *q = out + ((long)b * rows + row) * 4;
        q[0] = a0; q[1] = a1; q[2] = a2; q[3] = 0.0;
    }
}

// ---------------------------------------------------------------------------------
// Device-resident Lanczos on the reduced Hessian P H P (vch1d_hess_lanczos).  Every vector is a history
// [B][max_steps+2][n]; the basis is a ring of `nslots` of them, vector i sits in slot i % nslots.
//
// The sequential part stays one persistent workgroup per trajectory, on the planes and with the reductions of k1d_hessvec:
//   k1d_kr_setup   the free set and its size, q_0 = P q0 / ||P q0||, and the gradient sweep of k1d_hessvec<1> once, whose
//                  yp of every step goes to row k + 2 of one further history X (all the second sweep needs of the first)
//   k1d_kr_step    the order-1 tangent march of q_j (v_k, mean_k) and the second transposed sweep alone, yp read from X:
//                  w = H q_j, 2 M solves.  NOCACHE repeats the gradient sweep in lockstep (3 M solves); the product
//                  yp v_k is the same expression on the same numbers, so both variants give the same bits.
// The recurrence is streaming work over (j + 1) histories and runs on a wide grid, (chunks of KR1_CHUNK nodes, B): the
// passes k1d_kr_pass<MODE> write one partial per workgroup and basis vector into [B][chunks][S], k1d_kr_fin (one workgroup
// per trajectory) sums them in a fixed order.  No atomics: a trajectory's scalars do not depend on the batch.  The stop
// state lives in device cells: every kernel of a stopped trajectory returns at once, so the host enqueues k steps back to
// back and never looks between them.
// ---------------------------------------------------------------------------------
constexpr int KR1_T = 256;            // threads of a streaming workgroup
constexpr int KR1_CHUNK = 4096;       // nodes of a trajectory's history per streaming workgroup
constexpr int KR1_GROUP = 8;          // basis vectors a pass holds accumulators for at a time
constexpr int KR1_PER = KR1_CHUNK / KR1_T;      // nodes per thread
struct Kr1Cells {
    double *coef1, *coef2;            // [B][S] coefficients of the two Gram-Schmidt rounds
    double *alpha, *beta;             // [B][k]
    double *look;                     // [B][2] what the host reads after the set-up: n_free, ||P q0||
    double *scal;                     // [B] the divisor of the next k1d_kr_next
    double *amax;                     // [B] max_i |alpha_i| so far
    long long *lim, *stop, *steps;    // [B] min(k, n_free); 0 running, 1 last step with a valid q_{j+1}, 2 without, 3 over; steps taken
};
struct Kr1Args {
    double *Q;                        // the basis
    long slot_stride, hs;             // doubles between two slots / two trajectories
    long tot;                         // nodes of a trajectory's vector (rows * n)
    int nslots, S;                    // slots of the ring; stride of a partial and of a coefficient row
    unsigned char *mask;              // [B or 1][hs] bytes, non-zero = free
    long mask_s;                      // bytes between two trajectories' masks (0: one for the batch)
    Kr1Cells x;
};
__device__ __forceinline__ double *kr1_slot(const Kr1Args &a, int i) { return a.Q + (long)(i % a.nslots) * a.slot_stride; }

// Step k of the gradient sweep of k1d_hessvec on the planes (lphi, lmu, lw, rv, yp, ym) = q .. q + 5 n, in two halves
// around the caller's use of yp: the solve, and the multipliers of the step before.  G is not accumulated.
struct Kr1Base {
    const double *ph, *pq, *pt;       // this trajectory's base point
    double b1, b2;
};
__device__ __forceinline__ void kr1_grad_solve(const Phys1 &P, int n, double a, int lvl, const Hv1Args &G, const Kr1Base &T,
                                               int k, int M, double *q, double *lds, double *sk) {
    const int tid = threadIdx.x;
    double *lphi = q, *lmu = q + n, *rv = q + 3 * n, *yp = q + 4 * n, *ym = q + 5 * n;
    const long o = (long)(k + 2) * n;
    const double *ps = T.ph + o;
    const double wb = G.wt[k + 2] * T.b1;
    const bool term = k == M - 1;
    double S[1] = {0.0};
    for (int i = tid; i < n; i += T1) {
        const double w = G.wx[i], p = ps[i];
        double l = lphi[i] + wb * (w * (p - (T.pq ? T.pq[o + i] : 0.0)));
        if (term) l += T.b2 * (w * (p - (T.pt ? T.pt[i] : 0.0)));
        lphi[i] = l;
        S[0] += l;
    }
    block_sums<1>(S, sk);
    for (int i = tid; i < n; i += T1) rv[i] = lphi[i] - G.wx[i] * (S[0] / P.Lx);
    __syncthreads();
    SysArgs A{ps, rv, lmu, G.dts[k], a, P.tau, P.c1, P.c2, P.kappa, n};
    cr_solve<2>(A, lvl, lds, yp, ym);
}
__device__ __forceinline__ void kr1_grad_update(const Phys1 &P, int n, double a, const Hv1Args &G, int k, double *q,
                                                double *keep /* row k + 2 of X or NULL */) {
    double *lphi = q, *lmu = q + n, *lw = q + 2 * n, *yp = q + 4 * n, *ym = q + 5 * n;
    const double dt = G.dts[k], gdt = P.gamma / dt, al = (gdt - 0.5) / (gdt + 0.5), kd = P.tau / dt + 2.0 * P.c2;
    for (int i = threadIdx.x; i < n; i += T1) {
        const double y = yp[i], ldw = 0.5 * y + lw[i];
        if (keep) keep[i] = y;
        lphi[i] = kd * y + 0.5 * P.kappa * lap1t(yp, i, n, a) + ym[i] / dt;
        lmu[i] = 0.5 * y + 0.5 * lap1t(ym, i, n, a);
        lw[i] = 0.5 * y + al * ldw;
    }
}

// grid = B workgroups.  The start vector is in slot 0 on entry; box [B][2] = {u_min, u_max}.  A trajectory whose free set is
// empty, or whose start vector vanishes on it (or is not finite), gets stop = 3 and nothing else: the host reads look.
__global__ __launch_bounds__(T1) void k1d_kr_setup(Phys1 P, int n, double h, int lvl, int rows, Hv1Args G, Kr1Args K,
                                                   const double *__restrict__ box, double tol, int build, int kmax, int sweep,
                                                   double *X, double *scratch) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double sk[2 * (T1 / 64)];
    const int b = blockIdx.x, tid = threadIdx.x, M = rows - 2;
    const double a = 1.0 / (h * h);
    const double *uu = G.u ? G.u + b * G.u_s : nullptr;
    unsigned char *mk = K.mask + b * K.mask_s;
    double *q0 = K.Q + b * K.hs;
    const double lo = box[2 * b] + tol, hi = box[2 * b + 1] - tol;
    double S[2] = {0.0, 0.0};
    for (long i = tid; i < K.tot; i += T1) {
        bool m;
        if (build) {
            const double v = uu ? uu[i] : 0.0;
            m = v > lo && v < hi && fabs(v) > tol;
            mk[i] = m ? 1 : 0;
        } else {
            m = mk[i] != 0;
        }
        const double v = m ? q0[i] : 0.0;
        q0[i] = v;
        S[0] += m ? 1.0 : 0.0;              // exact in a double
        S[1] += v * v;
    }
    block_sums<2>(S, sk);
    const double nrm = sqrt(S[1]);
    const bool bad = S[0] < 1.0 || !(nrm > 0.0) || !isfinite(nrm);
    if (tid == 0) {
        K.x.look[2 * b] = S[0];
        K.x.look[2 * b + 1] = nrm;
        K.x.lim[b] = min((long long)kmax, (long long)S[0]);
        K.x.stop[b] = bad ? 3 : 0;
        K.x.steps[b] = 0;
        K.x.amax[b] = 0.0;
    }
    if (bad) return;                        // uniform over the workgroup
    for (long i = tid; i < K.tot; i += T1) q0[i] = q0[i] / nrm;
    if (!sweep) return;
    double *q = scratch + (long)b * NSCR1 * n;
    const Kr1Base T{G.phi + b * G.phi_s, G.pq ? G.pq + b * G.pq_s : nullptr, G.pt ? G.pt + b * G.pt_s : nullptr, G.wts[3 * b],
                    G.wts[3 * b + 1]};
    for (int i = tid; i < n; i += T1) q[i] = q[n + i] = q[2 * n + i] = 0.0;
    __syncthreads();
    for (int k = M - 1; k >= 0; --k) {
        kr1_grad_solve(P, n, a, lvl, G, T, k, M, q, lds, sk);
        kr1_grad_update(P, n, a, G, k, q, X + b * K.hs + (long)(k + 2) * n);
        __syncthreads();
    }
}

// One Lanczos step's sequential part: G.hd = q_j (a basis slot), G.hv = w, G.v, G.mean the tangent's history; grid = B.
template <int NOCACHE>
__global__ __launch_bounds__(T1) void k1d_kr_step(Phys1 P, int n, double h, int lvl, int rows, Hv1Args G,
                                                  const long long *__restrict__ stop, const double *X, double *scratch) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double sk[2 * (T1 / 64)];
    const int b = blockIdx.x, tid = threadIdx.x, M = rows - 2;
    if (stop[b]) return;                    // uniform over the workgroup
    const double a = 1.0 / (h * h);
    double *q = scratch + (long)b * NSCR1 * n;
    double *yp = q + 4 * n;
    double *Lphi = q + 6 * n, *Lmu = q + 7 * n, *Lw = q + 8 * n, *Rv = q + 9 * n, *Yp = q + 10 * n, *Ym = q + 11 * n;
    const Kr1Base T{G.phi + b * G.phi_s, G.pq ? G.pq + b * G.pq_s : nullptr, G.pt ? G.pt + b * G.pt_s : nullptr, G.wts[3 * b],
                    G.wts[3 * b + 1]};
    const double *ph = T.ph;
    const double *hd = G.hd + b * G.hs;
    const double *xb = X + b * G.hs;
    double *hv = G.hv + b * G.hs, *vb = G.v + b * G.hs, *mean = G.mean + (long)b * rows;
    const double b3 = G.wts[3 * b + 2];
    for (int row = 0; row < rows; ++row) {
        const long o = (long)row * n;
        const double wr = G.wt[row];
        for (int i = tid; i < n; i += T1) {
            const double w = b3 * (wr * G.wx[i]);
            hv[o + i] = w * hd[o + i];
        }
    }
    {
        // the order-1 tangent march of k1d_hessvec<2>, on the planes the second sweep takes over afterwards
        double *dphi = Lphi, *dmu = Lmu, *dw = Lw, *rp = Rv, *rm = Yp, *nphi = Ym, *nmu = q + 12 * n;
        for (int i = tid; i < n; i += T1) dphi[i] = dmu[i] = dw[i] = 0.0;
        __syncthreads();
        for (int s = 0; s < M; ++s) {
            const double dt = G.dts[s], gdt = P.gamma / dt;
            const double *ps = ph + (long)(s + 2) * n;
            const double *h0 = hd + (long)s * n, *h1 = h0 + n;
            for (int i = tid; i < n; i += T1) {
                const double wo = dw[i], wn = ((gdt - 0.5) * wo + 0.5 * (h1[i] + h0[i])) / (gdt + 0.5);
                const double d = dphi[i];
                rp[i] = (P.tau / dt) * d + 0.5 * P.kappa * lap1(dphi, i, n, a) + 2.0 * P.c2 * d + 0.5 * dmu[i] + 0.5 * (wn + wo);
                rm[i] = d / dt + 0.5 * lap1(dmu, i, n, a);
                dw[i] = wn;
            }
            __syncthreads();
            SysArgs A{ps, rp, rm, dt, a, P.tau, P.c1, P.c2, P.kappa, n};
            cr_solve<0>(A, lvl, lds, nphi, nmu);
            double ms = 0.0;
            for (int i = tid; i < n; i += T1) ms += ((i == 0 || i == n - 1) ? 0.5 : 1.0) * h * nphi[i];
            const double m1 = block_red<0>(ms, sk) / P.Lx;
            for (int i = tid; i < n; i += T1) {
                const double v = nphi[i];
                vb[(long)(s + 2) * n + i] = v;
                dphi[i] = v - m1;
                dmu[i] = nmu[i];
            }
            if (tid == 0) mean[s] = m1;
            __syncthreads();
        }
    }
    for (int i = tid; i < n; i += T1) {
        Lphi[i] = Lmu[i] = Lw[i] = 0.0;
        if (NOCACHE) q[i] = q[n + i] = q[2 * n + i] = 0.0;
    }
    __syncthreads();
    for (int k = M - 1; k >= 0; --k) {
        const double dt = G.dts[k], gdt = P.gamma / dt, al = (gdt - 0.5) / (gdt + 0.5), be = 0.5 / (gdt + 0.5);
        const long o = (long)(k + 2) * n;
        const double *ps = ph + o;
        const double wb = G.wt[k + 2] * T.b1, mk = mean[k];
        const bool term = k == M - 1;
        if (NOCACHE) kr1_grad_solve(P, n, a, lvl, G, T, k, M, q, lds, sk);
        const double *ypk = NOCACHE ? yp : xb + o;
        double S[1] = {0.0};
        for (int i = tid; i < n; i += T1) {
            const double d = vb[o + i] - mk;
            double L = Lphi[i] + wb * (G.wx[i] * d);
            if (term) L += T.b2 * (G.wx[i] * d);
            Lphi[i] = L;
            S[0] += L;
        }
        block_sums<1>(S, sk);
        for (int i = tid; i < n; i += T1) {
            const double p = ps[i], om = 1.0 - p * p;
            Rv[i] = (Lphi[i] - G.wx[i] * (S[0] / P.Lx)) - P.c1 * (4.0 * p / (om * om)) * (ypk[i] * vb[o + i]);
        }
        __syncthreads();
        SysArgs A2{ps, Rv, Lmu, dt, a, P.tau, P.c1, P.c2, P.kappa, n};
        cr_solve<2>(A2, lvl, lds, Yp, Ym);
        const double kd = P.tau / dt + 2.0 * P.c2;
        for (int i = tid; i < n; i += T1) {
            const double Y = Yp[i], Ldw = 0.5 * Y + Lw[i];
            hv[(long)k * n + i] += be * Ldw;
            hv[(long)(k + 1) * n + i] += be * Ldw;
            Lphi[i] = kd * Y + 0.5 * P.kappa * lap1t(Yp, i, n, a) + Ym[i] / dt;
            Lmu[i] = 0.5 * Y + 0.5 * lap1t(Ym, i, n, a);
            Lw[i] = 0.5 * Y + al * Ldw;
        }
        if (NOCACHE) kr1_grad_update(P, n, a, G, k, q, nullptr);
        __syncthreads();
    }
}

// One pass of the Gram-Schmidt step over w (in place) against q_first .. q_{first+nv-1}; grid = (chunks, B):
//   MODE 0   partials i = sum q_i (P w)                                            (w is read through the mask, not written)
//   MODE 1   w := P w - sum_i coef[b][i] q_i, then partials i = sum q_i w          (round 1's subtraction, round 2's products)
//   MODE 2   w := w - sum_i coef[b][i] q_i, partial 0 = sum w^2                    (round 2's subtraction, the norm)
// Masked-off nodes of every q_i are exact zeros, so w leaves MODE 1 with exact zeros there.  A thread keeps its
// KR1_PER nodes of w in registers across the basis vectors: w is read once and written once per pass.
template <int MODE>
__global__ __launch_bounds__(KR1_T) void k1d_kr_pass(Kr1Args a, int first, int nv, double *w, const double *__restrict__ coef,
                                                     double *__restrict__ part) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (a.x.stop[b]) return;                // uniform over the workgroup
    __shared__ double sred[KR1_GROUP * (KR1_T / 64)];
    const long hb = b * a.hs, i0 = (long)blockIdx.x * KR1_CHUNK + tid, i1 = min((long)(blockIdx.x + 1) * KR1_CHUNK, a.tot);
    const unsigned char *mk = a.mask + b * a.mask_s;
    double *wb = w + hb;
    double *my = part + ((long)b * gridDim.x + blockIdx.x) * a.S;
    double v[KR1_PER];
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        const long i = i0 + t * KR1_T;
        v[t] = i < i1 ? wb[i] : 0.0;
        if (MODE != 2) v[t] = (i < i1 && mk[i]) ? v[t] : 0.0;
    }
    if (MODE != 0) {
        const double *cf = coef + (long)b * a.S;
        for (int j = 0; j < nv; ++j) {
            const double cj = cf[j];
            const double *qj = kr1_slot(a, first + j) + hb;
#pragma unroll
            for (int t = 0; t < KR1_PER; ++t) {
                const long i = i0 + t * KR1_T;
                if (i < i1) v[t] -= cj * qj[i];
            }
        }
        double nrm = 0.0;
#pragma unroll
        for (int t = 0; t < KR1_PER; ++t) {
            const long i = i0 + t * KR1_T;
            if (i < i1) {
                wb[i] = v[t];
                nrm += v[t] * v[t];
            }
        }
        if (MODE == 2) {
            nrm = wsum1(nrm);
            if (lane == 0) sred[wv] = nrm;
            __syncthreads();
            if (tid == 0) my[0] = (sred[0] + sred[1]) + (sred[2] + sred[3]);
            return;
        }
    }
    for (int g0 = 0; g0 < nv; g0 += KR1_GROUP) {
        double acc[KR1_GROUP];
        const double *q[KR1_GROUP];
#pragma unroll
        for (int j = 0; j < KR1_GROUP; ++j) {
            acc[j] = 0.0;
            q[j] = kr1_slot(a, first + min(g0 + j, nv - 1)) + hb;     // past the end: the last vector again, its sum is not stored
        }
#pragma unroll
        for (int t = 0; t < KR1_PER; ++t) {
            const long i = i0 + t * KR1_T;
            if (i < i1) {
#pragma unroll
                for (int j = 0; j < KR1_GROUP; ++j) acc[j] += q[j][i] * v[t];
            }
        }
#pragma unroll
        for (int j = 0; j < KR1_GROUP; ++j) {
            const double s = wsum1(acc[j]);
            if (lane == 0) sred[j * (KR1_T / 64) + wv] = s;
        }
        __syncthreads();
        if (tid < KR1_GROUP && g0 + tid < nv) my[g0 + tid] = (sred[tid * 4] + sred[tid * 4 + 1]) + (sred[tid * 4 + 2] + sred[tid * 4 + 3]);
        __syncthreads();
    }
}
static_assert(KR1_T / 64 == 4, "the passes add four wave sums");

// q_{j+1} = w / beta_j into its basis slot, by the trajectory's stop cell: 0, 1 the quotient; 2 (no valid q_{j+1}) zeros;
// 3 nothing.  The next step reads its direction from the slot.
__global__ __launch_bounds__(KR1_T) void k1d_kr_next(Kr1Args a, const double *__restrict__ w, double *__restrict__ slot) {
    const int b = blockIdx.y;
    const long long st = a.x.stop[b];
    if (st == 3) return;
    const double s = a.x.scal[b];
    const long hb = b * a.hs, i0 = (long)blockIdx.x * KR1_CHUNK, i1 = min(i0 + (long)KR1_CHUNK, a.tot);
    for (long i = i0 + threadIdx.x; i < i1; i += KR1_T) slot[hb + i] = st == 2 ? 0.0 : w[hb + i] / s;
}

// out = sum_{i<nv} coef[b][i] q_i  (vch1d_krylov_vector)
__global__ __launch_bounds__(KR1_T) void k1d_kr_lincomb(Kr1Args a, int nv, const double *__restrict__ coef, double *__restrict__ out) {
    const int b = blockIdx.y;
    const double *cf = coef + (long)b * a.S;
    const long hb = b * a.hs, i0 = (long)blockIdx.x * KR1_CHUNK + threadIdx.x, i1 = min((long)(blockIdx.x + 1) * KR1_CHUNK, a.tot);
    double v[KR1_PER];
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) v[t] = 0.0;
    for (int j = 0; j < nv; ++j) {
        const double cj = cf[j];
        const double *qj = kr1_slot(a, j) + hb;
#pragma unroll
        for (int t = 0; t < KR1_PER; ++t) {
            const long i = i0 + t * KR1_T;
            if (i < i1) v[t] += cj * qj[i];
        }
    }
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        const long i = i0 + t * KR1_T;
        if (i < i1) out[hb + i] = v[t];
    }
}

// The scalars of a pass, one workgroup per trajectory: the nch partials of a slot summed in a fixed order (thread t takes
// elements t, t + KR1_T, ... in turn, then a tree over the threads).
__device__ __forceinline__ double kr1_sum(const double *__restrict__ part, int nch, int S, int slot, double *sh) {
    double s = 0.0;
    for (int e = threadIdx.x; e < nch; e += KR1_T) s += part[(long)e * S + slot];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int hh = KR1_T / 2; hh > 0; hh >>= 1) {
        if ((int)threadIdx.x < hh) sh[threadIdx.x] += sh[threadIdx.x + hh];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
// mode 2 / 3: the nv products of round 1 / 2 -> coef1 / coef2
// mode 4: step j's norm -> beta_j, alpha_j = coef1 + coef2 on q_j, the stop rules, the stop cell and the step count
__global__ __launch_bounds__(KR1_T) void k1d_kr_fin(Kr1Cells x, const double *__restrict__ part, int nch, int S, int mode, int nv,
                                                    int j, int k) {
    __shared__ double sh[KR1_T];
    const int b = blockIdx.x;
    const double *p = part + (long)b * nch * S;
    if (x.stop[b]) {                        // uniform: stopped at an earlier step
        if (threadIdx.x == 0 && mode == 4) x.stop[b] = 3;
        return;
    }
    if (mode == 2 || mode == 3) {
        double *cf = (mode == 2 ? x.coef1 : x.coef2) + (long)b * S;
        for (int i = 0; i < nv; ++i) {
            const double s = kr1_sum(p, nch, S, i, sh);
            if (threadIdx.x == 0) cf[i] = s;
        }
        return;
    }
    const double beta = sqrt(kr1_sum(p, nch, S, 0, sh));
    if (threadIdx.x != 0) return;
    const double alpha = x.coef1[(long)b * S + nv - 1] + x.coef2[(long)b * S + nv - 1];
    const double am = fmax(x.amax[b], fabs(alpha));
    x.amax[b] = am;
    x.alpha[(long)b * k + j] = alpha;
    x.beta[(long)b * k + j] = beta;
    x.steps[b] = j + 1;
    const bool broke = !isfinite(beta) || beta <= 1e-14 * am;          // an invariant subspace, or nothing to go on with
    const long long lim = x.lim[b];
    // n_free steps span the free set: no q_{j+1}
    x.stop[b] = (broke || j + 1 >= (long long)x.look[2 * b]) ? 2 : (j + 1 >= lim ? 1 : 0);
    x.scal[b] = beta;
}

// ---------------------------------------------------------------------------------
// Device-resident Newton-CG on the free set (vch1d_hess_cg): (preconditioned) conjugate gradients on
// P H P x = P b from x_0 = 0 with x, r and p in slots 0, 1, 2 of the basis storage of the Lanczos iteration above.
//   k1d_ncg_setup  (persistent, grid B) the free set and its size, the gradient sweep once (yp of every step to X; NEWTON:
//                  G accumulated with the expressions of k1d_hessvec<1>), r = P b, x = 0, p = D^-1 r, ||P b|| and
//                  rho = r.D^-1 r by the workgroup's fixed-order sums, the cells of a new iteration
//   k1d_kr_step    as above, unchanged: G.hd = the p slot, G.hv = w.  The stop cell holds VCH_CG_* of vch.h: running is
//                  VCH_CG_LIMIT = 0, so every way of stopping is non-zero, which is all k1d_kr_step tests
//   k1d_ncg_curv, k1d_ncg_update, k1d_ncg_dir   the recurrence on the (chunks of KR1_CHUNK, B) grid, partials
//                  [B][chunks][S]; k1d_ncg_fin (grid B) sums them in the order of kr1_sum and keeps the scalars
// D = diag(wt'_k wx_i) with wt' = the trapezoid weights of t_hist except wt'_0 := wt_1 (row 0 has quadrature weight zero
// but is a real unknown: it drives step 0), computed per node and not stored; the identity without the preconditioner.
// A thread keeps its KR1_PER nodes in registers and requests every global operand of its chunk before the first use.
// P is applied where w is read; masked-off nodes of x, r and p are exact zeros.  Every kernel of a stopped trajectory
// returns at once, so its x, r and p stay as the stopping step left them.  No atomics.
// ---------------------------------------------------------------------------------
enum { NCG1_X = 0, NCG1_R = 1, NCG1_P = 2 };
enum { NCG1_RUNNING = 0, NCG1_CONVERGED = 1, NCG1_NEGCURV = 2, NCG1_BREAKDOWN = 3 };    // the stop cell: VCH_CG_* of vch.h
struct Ncg1Cells {
    double *resid, *curv;             // [B][k]
    double *look;                     // [B][2] what the host reads after the set-up: n_free, ||P b||
    double *alpha, *beta;             // [B] the step length of k1d_ncg_update, the factor of k1d_ncg_dir
    double *rho, *rnorm0, *pred;      // [B]
    long long *steps, *prods, *stop;  // [B] updates of x, products H p taken, VCH_CG_*
};
struct Ncg1Args {
    double *Q;                        // x, r, p: slots 0, 1, 2
    long slot_stride, hs;             // doubles between two slots / two trajectories
    long tot;                         // nodes of a trajectory's vector (rows * n)
    int n, S;                         // nodes of a row; stride of a partial
    unsigned char *mask;              // [B or 1][hs] bytes, non-zero = free
    long mask_s;                      // bytes between two trajectories' masks (0: one for the batch)
    const double *wtp, *wx;           // [rows] wt', [n]
    int precond;
    Ncg1Cells x;
};
__device__ __forceinline__ double *ncg1_slot(const Ncg1Args &a, int i) { return a.Q + (long)i * a.slot_stride; }

// grid = B workgroups.  NEWTON 0: the right-hand side is in slot 1 on entry.  NEWTON 1: b = -(G + ks_b wt_k wx_i sign(u)),
// G the gradient field of J1 + J2 + J3 accumulated in slot 1 by the sweep.  box [B][2] = {u_min, u_max}, ks [B].
// sweep 0: no gradient sweep for an uploaded right-hand side (the steps repeat it); X NULL: yp is not kept.  A trajectory
// whose free set is empty or whose ||P b|| is not finite gets stop = BREAKDOWN and the host reads look; ||P b|| == 0 is
// CONVERGED.  With an uploaded right-hand side all three return before the sweep.
template <int NEWTON>
__global__ __launch_bounds__(T1) void k1d_ncg_setup(Phys1 P, int n, double h, int lvl, int rows, Hv1Args G, Ncg1Args K,
                                                    const double *__restrict__ box, const double *__restrict__ ks, double tol,
                                                    int build, int sweep, double *X, double *scratch) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double sk[3 * (T1 / 64)];
    const int b = blockIdx.x, tid = threadIdx.x, M = rows - 2;
    const double a = 1.0 / (h * h);
    const double *uu = G.u ? G.u + b * G.u_s : nullptr;
    unsigned char *mk = K.mask + b * K.mask_s;
    double *xs = ncg1_slot(K, NCG1_X) + b * K.hs, *rs = ncg1_slot(K, NCG1_R) + b * K.hs, *ps = ncg1_slot(K, NCG1_P) + b * K.hs;
    const double lo = box[2 * b] + tol, hi = box[2 * b + 1] - tol;
    double S[3] = {0.0, 0.0, 0.0};          // n_free (exact in a double), r.r, r.D^-1 r
    // r = P b, x = 0, p = D^-1 r of row `row` from the right-hand side bv(o, i), with the sums
    auto start_row = [&](int row, auto bv) {
        const long o = (long)row * n;
        const double wr = K.precond ? K.wtp[row] : 1.0;
        for (int i = tid; i < n; i += T1) {
            const double rv = mk[o + i] ? bv(o, i) : 0.0;
            const double z = rv / (K.precond ? wr * K.wx[i] : 1.0);
            xs[o + i] = 0.0;
            rs[o + i] = rv;
            ps[o + i] = z;
            S[1] += rv * rv;
            S[2] += rv * z;
        }
    };
    for (int row = 0; row < rows; ++row) {
        const long o = (long)row * n;
        for (int i = tid; i < n; i += T1) {
            bool m;
            if (build) {
                const double v = uu ? uu[o + i] : 0.0;
                m = v > lo && v < hi && fabs(v) > tol;
                mk[o + i] = m ? 1 : 0;
            } else {
                m = mk[o + i] != 0;
            }
            S[0] += m ? 1.0 : 0.0;
        }
        if (!NEWTON) start_row(row, [&](long oo, int i) { return rs[oo + i]; });
    }
    if (NEWTON) {
        double C[1] = {S[0]};
        block_sums<1>(C, sk);
        if (C[0] < 1.0) {                   // uniform over the workgroup: nothing to sweep for
            if (tid == 0) {
                K.x.look[2 * b] = 0.0;
                K.x.look[2 * b + 1] = 0.0;
                K.x.stop[b] = NCG1_BREAKDOWN;
            }
            return;
        }
        // the gradient sweep of k1d_hessvec<1>, G in slot 1: each thread its own nodes of every row
        double *q = scratch + (long)b * NSCR1 * n;
        const Kr1Base T{G.phi + b * G.phi_s, G.pq ? G.pq + b * G.pq_s : nullptr, G.pt ? G.pt + b * G.pt_s : nullptr, G.wts[3 * b],
                        G.wts[3 * b + 1]};
        const double b3 = G.wts[3 * b + 2];
        for (int row = 0; row < rows; ++row) {
            const long o = (long)row * n;
            const double wr = G.wt[row];
            for (int i = tid; i < n; i += T1) {
                const double w = b3 * (wr * G.wx[i]);
                rs[o + i] = w * (uu ? uu[o + i] : 0.0);
            }
        }
        for (int i = tid; i < n; i += T1) q[i] = q[n + i] = q[2 * n + i] = 0.0;
        __syncthreads();
        for (int k = M - 1; k >= 0; --k) {
            kr1_grad_solve(P, n, a, lvl, G, T, k, M, q, lds, sk);
            const double gdt = P.gamma / G.dts[k], be = 0.5 / (gdt + 0.5);
            for (int i = tid; i < n; i += T1) {
                const double y = q[4 * n + i], ldw = 0.5 * y + q[2 * n + i];
                rs[(long)k * n + i] += be * ldw;
                rs[(long)(k + 1) * n + i] += be * ldw;
            }
            kr1_grad_update(P, n, a, G, k, q, X ? X + b * K.hs + (long)(k + 2) * n : nullptr);
            __syncthreads();
        }
        const double kb = ks[b];
        for (int row = 0; row < rows; ++row) {
            const double kw = kb * G.wt[row];
            start_row(row, [&](long oo, int i) {
                const double v = uu ? uu[oo + i] : 0.0;
                const double sgn = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
                return -(rs[oo + i] + kw * (G.wx[i] * sgn));
            });
        }
        S[0] = 0.0;                         // summed above: the count comes back below
        block_sums<3>(S, sk);
        S[0] = C[0];
    } else {
        block_sums<3>(S, sk);
    }
    const double nrm = sqrt(S[1]);
    const bool bad = S[0] < 1.0 || !isfinite(nrm);
    if (tid == 0) {
        K.x.look[2 * b] = S[0];
        K.x.look[2 * b + 1] = nrm;
        K.x.rnorm0[b] = nrm;
        K.x.rho[b] = S[2];
        K.x.pred[b] = 0.0;
        K.x.steps[b] = 0;
        K.x.prods[b] = 0;
        K.x.stop[b] = bad ? NCG1_BREAKDOWN : (nrm == 0.0 ? NCG1_CONVERGED : NCG1_RUNNING);
    }
    if (NEWTON || bad || nrm == 0.0 || !sweep) return;      // uniform over the workgroup
    double *q = scratch + (long)b * NSCR1 * n;
    const Kr1Base T{G.phi + b * G.phi_s, G.pq ? G.pq + b * G.pq_s : nullptr, G.pt ? G.pt + b * G.pt_s : nullptr, G.wts[3 * b],
                    G.wts[3 * b + 1]};
    for (int i = tid; i < n; i += T1) q[i] = q[n + i] = q[2 * n + i] = 0.0;
    __syncthreads();
    for (int k = M - 1; k >= 0; --k) {
        kr1_grad_solve(P, n, a, lvl, G, T, k, M, q, lds, sk);
        kr1_grad_update(P, n, a, G, k, q, X + b * K.hs + (long)(k + 2) * n);
        __syncthreads();
    }
}

// The nodes of a thread of the streaming kernels are i0 + t KR1_T, t < KR1_PER, below i1; d[t] = D of node t (1 beyond i1).
#define NCG1_COORDS                                                                                                      \
    const int b = blockIdx.y, tid = threadIdx.x;                                                                         \
    const long hb = b * a.hs, i0 = (long)blockIdx.x * KR1_CHUNK + tid, i1 = min((long)(blockIdx.x + 1) * KR1_CHUNK, a.tot)
__device__ __forceinline__ void ncg1_diag(const Ncg1Args &a, long i0, long i1, double (&d)[KR1_PER]) {
    if (!a.precond) {
#pragma unroll
        for (int t = 0; t < KR1_PER; ++t) d[t] = 1.0;
        return;
    }
    long row = i0 / a.n;
    int col = (int)(i0 - row * a.n);
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        d[t] = i0 + t * KR1_T < i1 ? a.wtp[row] * a.wx[col] : 1.0;
        col += KR1_T;
        const int up = col / a.n;
        row += up;
        col -= up * a.n;
    }
}
// The two sums of a workgroup into its partial: wave sums, then the four waves in a fixed order.
__device__ __forceinline__ void ncg1_store2(double s0, double s1, double *sred, double *my) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    s0 = wsum1(s0);
    s1 = wsum1(s1);
    if (lane == 0) {
        sred[wv] = s0;
        sred[KR1_T / 64 + wv] = s1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double *s = sred + threadIdx.x * (KR1_T / 64);
        my[threadIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
    }
}

// Partials {p.(P w), p.D p}; w = H p of the step kernel just run.
__global__ __launch_bounds__(KR1_T) void k1d_ncg_curv(Ncg1Args a, const double *__restrict__ w, double *__restrict__ part) {
    NCG1_COORDS;
    if (a.x.stop[b]) return;                // uniform over the workgroup
    __shared__ double sred[2 * (KR1_T / 64)];
    const unsigned char *mk = a.mask + b * a.mask_s;
    const double *ps = ncg1_slot(a, NCG1_P) + hb, *wb = w + hb;
    double pv[KR1_PER], hv[KR1_PER], d[KR1_PER];
    unsigned char m[KR1_PER];
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        const long i = i0 + t * KR1_T;
        const bool in = i < i1;
        pv[t] = in ? ps[i] : 0.0;
        hv[t] = in ? wb[i] : 0.0;
        m[t] = in ? mk[i] : 0;
    }
    ncg1_diag(a, i0, i1, d);
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        s0 += pv[t] * (m[t] ? hv[t] : 0.0);
        s1 += pv[t] * (d[t] * pv[t]);
    }
    ncg1_store2(s0, s1, sred, part + ((long)b * gridDim.x + blockIdx.x) * a.S);
}

// x += alpha p, r -= alpha P w; partials {r.r, r.D^-1 r} of the new residual.
__global__ __launch_bounds__(KR1_T) void k1d_ncg_update(Ncg1Args a, const double *__restrict__ w, double *__restrict__ part) {
    NCG1_COORDS;
    if (a.x.stop[b]) return;
    __shared__ double sred[2 * (KR1_T / 64)];
    const unsigned char *mk = a.mask + b * a.mask_s;
    double *xs = ncg1_slot(a, NCG1_X) + hb, *rs = ncg1_slot(a, NCG1_R) + hb;
    const double *ps = ncg1_slot(a, NCG1_P) + hb, *wb = w + hb;
    const double al = a.x.alpha[b];
    double xv[KR1_PER], rv[KR1_PER], pv[KR1_PER], hv[KR1_PER], d[KR1_PER];
    unsigned char m[KR1_PER];
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        const long i = i0 + t * KR1_T;
        const bool in = i < i1;
        xv[t] = in ? xs[i] : 0.0;
        rv[t] = in ? rs[i] : 0.0;
        pv[t] = in ? ps[i] : 0.0;
        hv[t] = in ? wb[i] : 0.0;
        m[t] = in ? mk[i] : 0;
    }
    ncg1_diag(a, i0, i1, d);
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        const long i = i0 + t * KR1_T;
        const double r = rv[t] - al * (m[t] ? hv[t] : 0.0);
        if (i < i1) {
            xs[i] = xv[t] + al * pv[t];
            rs[i] = r;
        }
        s0 += r * r;
        s1 += r * (r / d[t]);
    }
    ncg1_store2(s0, s1, sred, part + ((long)b * gridDim.x + blockIdx.x) * a.S);
}

// p = D^-1 r + beta p, in its slot: the next step kernel reads its direction there.
__global__ __launch_bounds__(KR1_T) void k1d_ncg_dir(Ncg1Args a) {
    NCG1_COORDS;
    if (a.x.stop[b]) return;
    const double *rs = ncg1_slot(a, NCG1_R) + hb;
    double *ps = ncg1_slot(a, NCG1_P) + hb;
    const double be = a.x.beta[b];
    double rv[KR1_PER], pv[KR1_PER], d[KR1_PER];
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        const long i = i0 + t * KR1_T;
        rv[t] = i < i1 ? rs[i] : 0.0;
        pv[t] = i < i1 ? ps[i] : 0.0;
    }
    ncg1_diag(a, i0, i1, d);
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        const long i = i0 + t * KR1_T;
        if (i < i1) ps[i] = rv[t] / d[t] + be * pv[t];
    }
}
// kr1_sum, word for word (the same order of additions).  A copy, not a call: a second kernel calling kr1_sum can change
// the registers k1d_kr_fin compiles to (DESIGN.md 10g found that for the 2D pair).
__device__ __forceinline__ double ncg1_sum(const double *__restrict__ part, int nch, int S, int slot, double *sh) {
    double s = 0.0;
    for (int e = threadIdx.x; e < nch; e += KR1_T) s += part[(long)e * S + slot];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int hh = KR1_T / 2; hh > 0; hh >>= 1) {
        if ((int)threadIdx.x < hh) sh[threadIdx.x] += sh[threadIdx.x + hh];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
// The scalars of a step, one workgroup per trajectory:
//   mode 2   step j, after k1d_ncg_curv: c = p.P H p, n = p.D p, curv[j] = c / n, one more product taken; c not finite:
//            BREAKDOWN; !(c > 0): NEGCURV; otherwise alpha = rho / c
//   mode 3   step j, after k1d_ncg_update: pred += alpha rho / 2, resid[j] = ||r|| / ||P b||, steps = j + 1; not finite:
//            BREAKDOWN; resid[j] <= cg_tol: CONVERGED; otherwise beta = rho_new / rho
__global__ __launch_bounds__(KR1_T) void k1d_ncg_fin(Ncg1Cells x, const double *__restrict__ part, int nch, int S, int mode, int j,
                                                     int k, double cg_tol) {
    __shared__ double sh[KR1_T];
    const int b = blockIdx.x;
    const double *p = part + (long)b * nch * S;
    if (x.stop[b]) return;                  // uniform: stopped at an earlier step
    const double s0 = ncg1_sum(p, nch, S, 0, sh), s1 = ncg1_sum(p, nch, S, 1, sh);
    if (threadIdx.x != 0) return;
    long long st = NCG1_RUNNING;
    if (mode == 2) {
        x.curv[(long)b * k + j] = s0 / s1;
        x.prods[b] = j + 1;
        if (!isfinite(s0)) st = NCG1_BREAKDOWN;
        else if (!(s0 > 0.0)) st = NCG1_NEGCURV;
        else x.alpha[b] = x.rho[b] / s0;
    } else {
        const double rho = x.rho[b], res = sqrt(s0) / x.rnorm0[b];
        x.pred[b] += 0.5 * x.alpha[b] * rho;
        x.resid[(long)b * k + j] = res;
        x.steps[b] = j + 1;
        if (!isfinite(res) || !isfinite(s1)) st = NCG1_BREAKDOWN;
        else if (res <= cg_tol) st = NCG1_CONVERGED;
        else {
            x.beta[b] = s1 / rho;
            x.rho[b] = s1;
        }
    }
    x.stop[b] = st;
}

// ---------------------------------------------------------------------------------
// Truncated (Steihaug-Toint) conjugate gradients in a trust region (vch1d_hess_cg_tr): the iteration above
// with k1d_ncg_fin_tr in place of k1d_ncg_fin, every other kernel unchanged.  The region is ||x||_D <= radius with the
// preconditioner's D (the identity without it).  Since x_0 = 0, the recurrences xx = ||x||_D^2 and xp = x.D p start at 0:
//   x' = x + alpha p:   xx' = xx + 2 alpha xp + alpha^2 pp
//   p' = D^-1 r' + beta p, x'.r' = 0:   xp' = beta (xp + alpha pp)
// tau = the positive root of xx + 2 tau xp + tau^2 pp = radius^2.  An exit on the boundary is pending between mode 2 and
// mode 3, so that k1d_ncg_update runs once more with alpha = tau and r stays P b - P H P x.
// ---------------------------------------------------------------------------------
enum { NCG1_BOUNDARY = 4 };                     // VCH_CG_BOUNDARY of vch.h
struct Ntr1Cells {
    const double *radius;             // [B]
    double *xx, *xp, *pp, *c;         // [B] ||x||_D^2, x.D p, p.D p and p.P H p of the step
    long long *pend;                  // [B] the exit mode 3 takes: 0, NCG1_NEGCURV or NCG1_BOUNDARY
};
// tau >= 0 with xx + 2 tau xp + tau^2 pp = d2 (xx <= d2, pp > 0), in the form without cancellation for either sign of xp
__device__ __forceinline__ double ntr1_tau(double xx, double xp, double pp, double d2) {
    const double gap = fmax(d2 - xx, 0.0), disc = sqrt(xp * xp + pp * gap);
    return xp > 0.0 ? gap / (xp + disc) : (disc - xp) / pp;
}
// mode 2   as k1d_ncg_fin, then: c not finite: BREAKDOWN; !(c > 0): alpha = tau, pending NEGCURV; the step rho / c would
//          leave the region (xx + 2 alpha xp + alpha^2 pp >= radius^2): alpha = tau, pending BOUNDARY; otherwise alpha = rho / c.
//          A tau that is not finite (radius = +inf on a direction of non-positive curvature) stops at once with NEGCURV as
//          k1d_ncg_fin does: x stays as it is.
// mode 3   pending: pred += tau rho - tau^2 c / 2, resid[j], steps = j + 1, xx by its recurrence, stop = the pending exit;
//          otherwise k1d_ncg_fin's arithmetic, then xx and (still running) xp by their recurrences.
__global__ __launch_bounds__(KR1_T) void k1d_ncg_fin_tr(Ncg1Cells x, Ntr1Cells t, const double *__restrict__ part, int nch, int S,
                                                        int mode, int j, int k, double cg_tol) {
    __shared__ double sh[KR1_T];
    const int b = blockIdx.x;
    const double *p = part + (long)b * nch * S;
    if (x.stop[b]) return;                  // uniform: stopped at an earlier step
    const double s0 = ncg1_sum(p, nch, S, 0, sh), s1 = ncg1_sum(p, nch, S, 1, sh);
    if (threadIdx.x != 0) return;
    long long st = NCG1_RUNNING;
    const double xx = t.xx[b], xp = t.xp[b];
    if (mode == 2) {
        x.curv[(long)b * k + j] = s0 / s1;
        x.prods[b] = j + 1;
        long long pend = NCG1_RUNNING;
        if (!isfinite(s0)) {
            st = NCG1_BREAKDOWN;
        } else {
            const double rad = t.radius[b], d2 = rad * rad;
            double al = 0.0;
            if (!(s0 > 0.0)) {
                pend = NCG1_NEGCURV;
            } else {
                al = x.rho[b] / s0;
                if (xx + 2.0 * al * xp + al * al * s1 >= d2) pend = NCG1_BOUNDARY;
            }
            if (pend) al = ntr1_tau(xx, xp, s1, d2);
            if (pend && !isfinite(al)) {
                st = NCG1_NEGCURV;
                pend = NCG1_RUNNING;
            } else {
                x.alpha[b] = al;
            }
        }
        t.pp[b] = s1;
        t.c[b] = s0;
        t.pend[b] = pend;
    } else {
        const long long pend = t.pend[b];
        const double rho = x.rho[b], res = sqrt(s0) / x.rnorm0[b], al = x.alpha[b], pp = t.pp[b];
        x.resid[(long)b * k + j] = res;
        x.steps[b] = j + 1;
        if (pend) {
            x.pred[b] += al * rho - 0.5 * (al * al) * t.c[b];
            st = pend;
        } else {
            x.pred[b] += 0.5 * x.alpha[b] * rho;
            if (!isfinite(res) || !isfinite(s1)) st = NCG1_BREAKDOWN;
            else if (res <= cg_tol) st = NCG1_CONVERGED;
            else {
                x.beta[b] = s1 / rho;
                x.rho[b] = s1;
            }
        }
        t.xx[b] = xx + 2.0 * al * xp + al * al * pp;
        if (st == NCG1_RUNNING) t.xp[b] = x.beta[b] * (xp + al * pp);
    }
    x.stop[b] = st;
}

// ---------------------------------------------------------------------------------
// Damped Newton rounds on the free set (vch1d_pgd_newton, vch1d_newton_trial): the trial control of a step
// length, on the streaming grid of the Newton-CG kernels above (chunks of KR1_CHUNK nodes, B) with their indexing: node i of
// trajectory b sits at b hs + i, hs the stride of a history of max_steps + 2 rows, not rows n.  x is slot NCG1_X, the mask
// the bytes of the set-up, box [B][2] its table, s_tab [B] the step lengths; u is the base control of the solve (stride u_s,
// 0 for a shared base; NULL: zeros).  A trajectory whose verdict is in (skip[b] != 0; skip may be NULL) returns at once.
//
// Per node t = min(max(u + s_b x, u_min_b), u_max_b) with NumPy's order of comparisons (a NaN stays a NaN); a free node with
// t u < 0 becomes 0, the kink, where the next round pins it.  Every s the rounds use is a power of two, so s x is exact
// (short of an underflow) and u + s x rounds once whether or not the compiler fuses the multiply-add: the trial has the
// bits of np.clip(u + s * d, lo, hi).  A thread keeps its KR1_PER nodes in registers and requests u, x and the mask byte of
// all of them before the first use: 17 bytes read and 8 written per node.  Partials [B][chunks][4] = {sum (t - u)^2,
// sum u^2, nodes pinned to 0, nodes the clip moved} (the counts exact in a double): lane shuffle, then the four wave sums
// in turn.  No atomics.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(KR1_T) void k1d_nt_trial(Ncg1Args a, const double *__restrict__ u, long u_s,
                                                      const double *__restrict__ s_tab, const double *__restrict__ box,
                                                      const int *__restrict__ skip, double *__restrict__ trial,
                                                      double *__restrict__ part) {
    NCG1_COORDS;
    if (skip && skip[b]) return;            // uniform over the workgroup
    __shared__ double sred[4 * (KR1_T / 64)];
    const unsigned char *mk = a.mask + b * a.mask_s;
    const double *xs = ncg1_slot(a, NCG1_X) + hb;
    const double *ub = u ? u + b * u_s : nullptr;
    double *tb = trial + hb;
    const double s = s_tab[b], lo = box[2 * b], hi = box[2 * b + 1];
    double uv[KR1_PER], xv[KR1_PER];
    unsigned int m[KR1_PER];
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        const long i = i0 + t * KR1_T;
        const bool in = i < i1;
        uv[t] = (in && ub) ? ub[i] : 0.0;
        xv[t] = in ? xs[i] : 0.0;
        m[t] = in ? (unsigned int)mk[i] : 0u;
    }
    // the mask bytes stay in registers as they came: a test of one here would wait for it in front of the next node's requests
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) asm volatile("" : "+v"(m[t]));
    // no branch between the requests and the stores: a node beyond the chunk adds zeros, and its trial (in xv) is not stored
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        const bool in = i0 + t * KR1_T < i1;
        const double v = uv[t] + s * xv[t];
        double tv = (v != v || v > lo) ? v : lo;
        tv = (tv != tv || tv < hi) ? tv : hi;
        const bool moved = tv != v;
        const bool pin = m[t] != 0u && tv * uv[t] < 0.0;
        tv = pin ? 0.0 : tv;
        const double d = in ? tv - uv[t] : 0.0;
        acc[0] += d * d;
        acc[1] += uv[t] * uv[t];
        acc[2] += (in && pin) ? 1.0 : 0.0;
        acc[3] += (in && moved) ? 1.0 : 0.0;
        xv[t] = tv;
    }
#pragma unroll
    for (int t = 0; t < KR1_PER; ++t) {
        const long i = i0 + t * KR1_T;
        if (i < i1) tb[i] = xv[t];
    }
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double w = wsum1(acc[q]);
        if (lane == 0) sred[q * (KR1_T / 64) + wv] = w;
    }
    __syncthreads();
    if (tid < 4) {
        const double *w = sred + tid * (KR1_T / 64);
        part[((long)b * gridDim.x + blockIdx.x) * 4 + tid] = ((w[0] + w[1]) + w[2]) + w[3];
    }
}
#undef NCG1_COORDS

// The four sums of a trajectory's partials, one workgroup of KR1_T threads per trajectory, in the order of kr1_sum (a copy,
// as ncg1_sum is, so that k1d_kr_fin and k1d_ncg_fin keep their registers).  out [B][4]; a skipped trajectory's cells are
// left alone.
__global__ __launch_bounds__(KR1_T) void k1d_nt_fin(const double *__restrict__ part, int nch, const int *__restrict__ skip,
                                                    double *__restrict__ out) {
    __shared__ double sh[KR1_T];
    const int b = blockIdx.x;
    if (skip && skip[b]) return;            // uniform over the workgroup
    const double *p = part + (long)b * nch * 4;
    for (int slot = 0; slot < 4; ++slot) {
        double s = 0.0;
        for (int e = threadIdx.x; e < nch; e += KR1_T) s += p[(long)e * 4 + slot];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int hh = KR1_T / 2; hh > 0; hh >>= 1) {
            if ((int)threadIdx.x < hh) sh[threadIdx.x] += sh[threadIdx.x + hh];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[4 * b + slot] = sh[0];
        __syncthreads();
    }
}
