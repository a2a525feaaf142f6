// vch_engine1d.hip — host side of the 1D engine (C ABI vch1d_* of include/vch.h).
// Fields are [B][N+1], histories [B][rows][N+1] (rows = M+2: the reference's duplicated t=0 row,
// F1:329-336), contiguous on host and device alike.
#include "vch_common.h"
#include "vch_kernels1d.h"
#include "vch_pgd.h"
#include "vch_newton.h"
#include <algorithm>
#include <cmath>
#include <vector>

// Made by `new vch1d_ctx()` alone: a member without an initialiser starts as zero (NULL).
struct vch1d_ctx {
    vch_pool pool{vch_hip_mem()};  // owns every device and pinned buffer below (vch_mem.h); teardown() releases it
    vch1d_params prm;
    int B, Mmax, device, n, lvl;
    double h;
    Phys1 P, F;                    // run-time parameters; frozen defaults for the adjoint (B1:29-33)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double *scratch;               // [B][NSCR1][n]
    double *tmp[8];                // [B][n]
    double *phi_hist, *u_hist, *u_trial, *phiQ, *p_hist, *q_hist, *r_hist;   // [B][Mmax+2][n], lazy
    double *phiT, *dts, *tgrid, *wx, *alpha_dev, *cost_lvl, *hist_dev;
    double *cost_host;
    int *stats_dev, *stats_host;
    size_t lds_bytes = sizeof(double) * 14 * NR_MAX;
    int rows_res;
    // device-resident PGD (vch1d_pgd_*)
    bool pgd_ready = false;
    int pgd_rows = 0;
    std::vector<vch_opt_params> opts;      // one set per trajectory (vch1d_pgd_init repeats one set)
    std::vector<double> opt_tab_host;      // the table's host copy: the source of an asynchronous upload outlives the call
    double *seam_tab = nullptr;            // [OPT1_STRIDE]: the one row vch1d_backward / vch1d_grad_prox fill from their scalars
    double seam_tab_host[6] = {0, 0, 0, 0, 0, 0};
    double *opt_tab = nullptr;             // [B][OPT1_STRIDE]: the device copy the kernels index by trajectory
    bool pgd_r_valid = false;              // an adjoint sweep has run since the last init
    long long *kkt_cnt = nullptr;          // vch1d_pgd_kkt: [B][4] counts
    double *kkt_nrm = nullptr;             //                [B][2] squared norms
    double *phi0_dev = nullptr, *phi_trial = nullptr, *chg_dev = nullptr, *tp_dev = nullptr;
    int *skip_dev = nullptr;
    std::vector<double> t_host, chg_host;
    vch_pgd_state pgd;                     // the line search's books and the error metrics of the driver loop (vch_pgd.h)
    // vch1d_second_order (lazy): its own copies of the base point, the direction and the grids, so that the call leaves
    // every resident buffer as it found it
    double *so_base = nullptr, *so_u = nullptr, *so_pq = nullptr, *so_h = nullptr, *so_d1 = nullptr, *so_d2 = nullptr;   // [B][Mmax+2][n]
    double *so_pt = nullptr, *so_dts = nullptr, *so_t = nullptr, *so_wx = nullptr, *so_wts = nullptr, *so_out = nullptr;
    // vch1d_hessvec (lazy; it shares the base point, direction and grid buffers above): G, Hh and the tangent's v_k
    // [B][Mmax+2][n], the time weights [Mmax+2], the removed means [B][Mmax+2], the two dot products [B][2]
    double *hv_g = nullptr, *hv_hv = nullptr, *hv_v = nullptr, *hv_wt = nullptr, *hv_mean = nullptr, *hv_dots = nullptr;
    // vch1d_hess_lanczos (lazy, one group): the basis [kr_slots][B][Mmax+2][n], the gradient sweep's yp of every step, the
    // tangent's v_k and w (one history each), the mask (one byte per node of a history) and the block of partials, scalars
    // and small tables (Kr1Layout); what the last iteration left for vch1d_krylov_vector
    double *kr_Q = nullptr, *kr_X = nullptr, *kr_V = nullptr, *kr_W = nullptr, *kr_sc = nullptr;
    unsigned char *kr_mask = nullptr;
    int kr_slots = 0, kr_kcap = 0;
    bool kr_valid = false;
    int kr_rows = 0, kr_run_slots = 0, kr_min_steps = 0, kr_window = 0;
    bool kr_nocache = false;               // VCH_KRYLOV_NOCACHE=1 (A/B and tests): every step repeats the gradient sweep
    // vch1d_hess_cg keeps x, r, p in slots 0, 1, 2 of kr_Q (either call invalidates what the other left resident)
    bool ncg_valid = false;
    int ncg_rows = 0;
    // what vch1d_newton_trial needs of the last vch1d_hess_cg beside x: its base control (NULL: zeros) with its stride and
    // the stride of its mask; ncg_u_live: the call's own copy of an uploaded control has not been overwritten since
    const double *ncg_u = nullptr;
    long ncg_us = 0, ncg_mask_s = 0;
    bool ncg_u_live = false;
    // vch1d_pgd_newton: the PGD problem's own dt and x on the host, and who of the trajectories the stop rule ended has had
    // its state history and stored cost brought up to its control (the stop quirk)
    std::vector<double> dt_host, x_host;
    std::vector<int> pgd_synced;
    // directional sparsity: the resident problem's mode per trajectory (empty or all VCH_SPARSITY_FULL: none
    // of what follows is allocated or launched), its device copy, the time weights [Mmax+2], s per group [B][max(Mmax+2, n)],
    // the column kernel's change partials [B][gp_nblk][2], the squared column norms [B][n] with their host copy, alpha = 1
    std::vector<int> modes;
    int *mode_dev = nullptr;
    double *gp_wt = nullptr, *gp_s = nullptr, *gp_chg = nullptr, *gp_col = nullptr, *gp_one = nullptr;
    std::vector<double> gp_chg_host, gp_col_host, wx_host;
};

static inline int gp_nblk(const vch1d_ctx *c) { return (c->n + 63) / 64; }
static inline long gp_ss(const vch1d_ctx *c) { return std::max(c->Mmax + 2, c->n); }
static bool gp_any(const vch1d_ctx *c, int mode) { return std::find(c->modes.begin(), c->modes.end(), mode) != c->modes.end(); }
static bool gp_group(const vch1d_ctx *c) { return gp_any(c, VCH_SPARSITY_TIME) || gp_any(c, VCH_SPARSITY_SPACE); }
static int gp_mode(const vch1d_ctx *c, int b) { return c->modes.empty() ? VCH_SPARSITY_FULL : c->modes[b]; }

// no launch bookkeeping (LAUNCH_LDS, vch_common.h)
static bool launch_begin(vch1d_ctx *, int) { return false; }
static void launch_end(vch1d_ctx *, int, bool) {}

// n zeroed doubles into *p, unless it has them already
static int dalloc1(vch1d_ctx *c, double **p, size_t n) {
    if (*p) return 0;
    MEMCHK(c->pool.dev(p, n * sizeof(double)));
    HIPCHK(hipMemsetAsync(*p, 0, n * sizeof(double), c->stream));
    return 0;
}
static inline long hs1(const vch1d_ctx *c) { return (long)(c->Mmax + 2) * c->n; }
static int ensure1(vch1d_ctx *c, double **p) { return dalloc1(c, p, (size_t)c->B * hs1(c)); }
static int up(vch1d_ctx *c, double *dev, const double *host, size_t n) {
    HIPCHK(hipMemcpyAsync(dev, host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return 0;
}
// the function seams' scalar parameters as one table row on the device (read by every trajectory: stride 0)
static int seam_row(vch1d_ctx *c, double b1, double b2, double b3, double ks, double umin, double umax) {
    VCHCHK(dalloc1(c, &c->seam_tab, OPT1_STRIDE));
    double *row = c->seam_tab_host;
    row[OPT1_B1] = b1; row[OPT1_B2] = b2; row[OPT1_B3] = b3; row[OPT1_KS] = ks; row[OPT1_UMIN] = umin; row[OPT1_UMAX] = umax;
    return up(c, c->seam_tab, row, OPT1_STRIDE);
}
static int down(vch1d_ctx *c, double *host, const double *dev, size_t n) {
    HIPCHK(hipMemcpyAsync(host, dev, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
// host [B][rows][n] <-> device [B][Mmax+2][n]
static int up_hist(vch1d_ctx *c, double *dev, const double *host, int rows) {
    for (int b = 0; b < c->B; ++b) VCHCHK(up(c, dev + b * hs1(c), host + (size_t)b * rows * c->n, (size_t)rows * c->n));
    return 0;
}
static int down_hist(vch1d_ctx *c, double *host, const double *dev, int rows) {
    for (int b = 0; b < c->B; ++b)
        HIPCHK(hipMemcpyAsync(host + (size_t)b * rows * c->n, dev + b * hs1(c), sizeof(double) * rows * c->n,
                              hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// Everything a context holds, in the order that is safe for one that vch1d_create only half built.
static void teardown(vch1d_ctx *c) {
    if (c->stream) hipStreamSynchronize(c->stream);
    c->pool.release();
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

extern "C" vch1d_ctx *vch1d_create(const vch1d_params *p, int batch, int max_steps, int device) {
    if (!p || p->N < 2 || batch < 1 || max_steps < 1 || !(p->Lx > 0)) {
        vch_fail(VCH_ERR_ARG, "vch1d_create: bad arguments");
        return nullptr;
    }
    int lvl = 0;
    while ((p->N) / (1 << lvl) + 1 > NR_MAX && lvl < 3) ++lvl;
    if (lvl > 2) {
        vch_fail(VCH_ERR_ARG, "vch1d_create: N = %d exceeds the supported 4096 (cyclic-reduction rows kept in LDS)", p->N);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        (void)hipGetLastError();          // do not leave the sticky error for the next launch check
        vch_fail(VCH_ERR_HIP, "hipSetDevice(%d) failed", device);
        return nullptr;
    }
    vch1d_ctx *c = new vch1d_ctx();
    c->prm = *p;
    c->B = batch;
    c->Mmax = max_steps;
    c->device = device;
    c->n = p->N + 1;
    c->lvl = lvl;
    c->h = p->Lx / p->N;
    c->P = Phys1{p->tau, p->gamma, p->c1, p->c2, p->kappa, p->Lx};
    c->F = Phys1{0.05, 10.0, 0.75, 1.0, 0.03 * 0.03, 1.0};      // K1:95-102 defaults, frozen at import in B1:29-33
    auto fail = [&](const char *what) {
        vch_fail(VCH_ERR_HIP, "vch1d_create: %s failed: %s", what, hipGetErrorString(hipGetLastError()));
        teardown(c);
        return (vch1d_ctx *)nullptr;
    };
    if (hipStreamCreate(&c->stream) != hipSuccess) return fail("hipStreamCreate");
    hipEventCreate(&c->ev0);
    hipEventCreate(&c->ev1);
    const size_t bn = (size_t)batch * c->n, lv = (size_t)batch * (max_steps + 2) * 4;
    if (dalloc1(c, &c->scratch, bn * NSCR1)) return fail("hipMalloc");
    for (auto &t : c->tmp)
        if (dalloc1(c, &t, bn)) return fail("hipMalloc");
    if (dalloc1(c, &c->phiT, bn) || dalloc1(c, &c->dts, max_steps + 2) || dalloc1(c, &c->tgrid, max_steps + 2) ||
        dalloc1(c, &c->wx, c->n) || dalloc1(c, &c->alpha_dev, batch) || dalloc1(c, &c->cost_lvl, lv) ||
        dalloc1(c, &c->hist_dev, (size_t)batch * 64))
        return fail("hipMalloc");
    if (c->pool.dev(&c->stats_dev, sizeof(int) * 8 * batch)) return fail("hipMalloc");
    if (c->pool.host(&c->stats_host, sizeof(int) * 8 * batch)) return fail("hipHostMalloc");
    if (c->pool.host(&c->cost_host, sizeof(double) * lv)) return fail("hipHostMalloc");
    // > 64 KiB of dynamic LDS needs the opt-in attribute
    for (const void *k : {(const void *)k1d_forward, (const void *)k1d_newton, (const void *)k1d_backward, (const void *)k1d_solve<0>,
                          (const void *)k1d_solve<1>, (const void *)k1d_tangent<1>, (const void *)k1d_tangent<2>,
                          (const void *)k1d_hessvec<1>, (const void *)k1d_hessvec<2>, (const void *)k1d_kr_setup,
                          (const void *)k1d_kr_step<0>, (const void *)k1d_kr_step<1>, (const void *)k1d_ncg_setup<0>,
                          (const void *)k1d_ncg_setup<1>})
        hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_bytes);
    c->kr_nocache = getenv("VCH_KRYLOV_NOCACHE") && atoi(getenv("VCH_KRYLOV_NOCACHE")) != 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail("hipStreamSynchronize");
    return c;
}

extern "C" void vch1d_destroy(vch1d_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    teardown(c);
}

extern "C" int vch1d_apply_laplacian(vch1d_ctx *c, const double *v, double *out) {
    CTXCHK(c);
    ARGCHK(v && out, "NULL array");
    const size_t bn = (size_t)c->B * c->n;
    VCHCHK(up(c, c->tmp[0], v, bn));
    LAUNCH(k1d_lap, dim3((c->n + 255) / 256, c->B), dim3(256), c->n, 1.0 / (c->h * c->h), (const double *)c->tmp[0], c->tmp[1]);
    return down(c, out, c->tmp[1], bn);
}

extern "C" int vch1d_residuals(vch1d_ctx *c, const double *pn, const double *po, const double *mn, const double *mo,
                               const double *wn, const double *wo, double dt, double *Rp, double *Rm) {
    CTXCHK(c);
    ARGCHK(pn && po && mn && mo && wn && wo && Rp && Rm && dt > 0, "NULL array or dt <= 0");
    const size_t bn = (size_t)c->B * c->n;
    const double *src[6] = {pn, po, mn, mo, wn, wo};
    for (int k = 0; k < 6; ++k) VCHCHK(up(c, c->tmp[k], src[k], bn));
    LAUNCH(k1d_residuals, dim3((c->n + 255) / 256, c->B), dim3(256), c->P, c->n, 1.0 / (c->h * c->h), dt,
            (const double *)c->tmp[0], (const double *)c->tmp[1], (const double *)c->tmp[2], (const double *)c->tmp[3],
            (const double *)c->tmp[4], (const double *)c->tmp[5], c->tmp[6], c->tmp[7]);
    VCHCHK(down(c, Rp, c->tmp[6], bn));
    return down(c, Rm, c->tmp[7], bn);
}

extern "C" int vch1d_jacobian_solve(vch1d_ctx *c, const double *phi_new, double dt, const double *rhs_phi,
                                    const double *rhs_mu, double *dphi, double *dmu) {
    CTXCHK(c);
    ARGCHK(phi_new && rhs_phi && rhs_mu && dphi && dmu && dt > 0, "NULL array or dt <= 0");
    const size_t bn = (size_t)c->B * c->n;
    VCHCHK(up(c, c->tmp[0], phi_new, bn));
    VCHCHK(up(c, c->tmp[1], rhs_phi, bn));
    VCHCHK(up(c, c->tmp[2], rhs_mu, bn));
    SysArgs A{nullptr, nullptr, nullptr, dt, 1.0 / (c->h * c->h), c->P.tau, c->P.c1, c->P.c2, c->P.kappa, c->n};
    LAUNCH_LDS(-1, (k1d_solve<0>), dim3(c->B), dim3(T1), c->lds_bytes, A, c->lvl, (const double *)c->tmp[0], (const double *)c->tmp[1],
            (const double *)c->tmp[2], c->tmp[3], c->tmp[4]);
    VCHCHK(down(c, dphi, c->tmp[3], bn));
    return down(c, dmu, c->tmp[4], bn);
}

extern "C" int vch1d_adjoint_solve(vch1d_ctx *c, const double *phi_n, double dt, const double *rhs, double *p_out) {
    CTXCHK(c);
    ARGCHK(rhs && p_out && dt >= 0 && (phi_n || dt == 0), "NULL array or dt < 0");
    const size_t bn = (size_t)c->B * c->n;
    if (phi_n) VCHCHK(up(c, c->tmp[0], phi_n, bn));
    else HIPCHK(hipMemsetAsync(c->tmp[0], 0, bn * sizeof(double), c->stream));
    VCHCHK(up(c, c->tmp[1], rhs, bn));
    SysArgs A{nullptr, nullptr, nullptr, dt, 1.0 / (c->h * c->h), c->F.tau, c->F.c1, c->F.c2, 0.0, c->n};
    LAUNCH_LDS(-1, (k1d_solve<1>), dim3(c->B), dim3(T1), c->lds_bytes, A, c->lvl, (const double *)c->tmp[0], (const double *)c->tmp[1],
            (const double *)nullptr, c->tmp[3], c->tmp[4]);
    return down(c, p_out, c->tmp[3], bn);
}

extern "C" int vch1d_newton_raphson(vch1d_ctx *c, const double *phi_old, const double *mu_old, const double *w_old,
                                    const double *w_new, double dt, double *phi_new, double *mu_new, double *hist,
                                    int hist_cap, int32_t *n_hist) {
    CTXCHK(c);
    ARGCHK(phi_old && mu_old && w_old && w_new && phi_new && mu_new && dt > 0, "NULL array or dt <= 0");
    const int n = c->n;
    for (int b = 0; b < c->B; ++b) {          // scratch layout: phi, mu, w, wnew are the first four arrays
        double *q = c->scratch + (size_t)b * NSCR1 * n;
        VCHCHK(up(c, q, phi_old + (size_t)b * n, n));
        VCHCHK(up(c, q + n, mu_old + (size_t)b * n, n));
        VCHCHK(up(c, q + 2 * n, w_old + (size_t)b * n, n));
        VCHCHK(up(c, q + 3 * n, w_new + (size_t)b * n, n));
    }
    LAUNCH_LDS(-1, k1d_newton, dim3(c->B), dim3(T1), c->lds_bytes, c->P, n, c->h, c->lvl, dt, c->scratch, c->hist_dev, 64, c->stats_dev);
    HIPCHK(hipMemcpyAsync(c->stats_host, c->stats_dev, sizeof(int) * 8 * c->B, hipMemcpyDeviceToHost, c->stream));
    for (int b = 0; b < c->B; ++b) {
        double *q = c->scratch + (size_t)b * NSCR1 * n;
        VCHCHK(down(c, phi_new + (size_t)b * n, q + 4 * n, n));
        VCHCHK(down(c, mu_new + (size_t)b * n, q + 5 * n, n));
    }
    std::vector<double> hh((size_t)c->B * 64);
    VCHCHK(down(c, hh.data(), c->hist_dev, hh.size()));
    for (int b = 0; b < c->B; ++b) {
        if (c->stats_host[b * 8 + 4]) return vch_fail(VCH_ERR_STATE, "Non-finite mass_defect; check phi bounds/log regularization.");
        const int k = std::min(c->stats_host[b * 8 + 0], 64);
        if (n_hist) n_hist[b] = k;
        if (hist)
            for (int j = 0; j < std::min(k, hist_cap); ++j) hist[(size_t)b * hist_cap + j] = hh[(size_t)b * 64 + j];
    }
    return 0;
}

extern "C" int vch1d_forward(vch1d_ctx *c, const double *phi0, const double *u, int u_rows, const double *dt, int M,
                             double *phi_hist_out, vch_stats *stats) {
    CTXCHK(c);
    ARGCHK(phi0 && dt && M >= 1 && M <= c->Mmax, "NULL array or M out of range (1..max_steps)");
    // F1:347-353 indexes control_input[step] for every step: fewer than M rows is an IndexError there
    if (u) ARGCHK(u_rows >= M && u_rows <= c->Mmax + 2, "control rows: need M <= rows <= max_steps+2 (IndexError in the reference)");
    VCHCHK(ensure1(c, &c->phi_hist));
    if (u) {
        VCHCHK(ensure1(c, &c->u_hist));
        VCHCHK(up_hist(c, c->u_hist, u, u_rows));
    }
    VCHCHK(up(c, c->tmp[0], phi0, (size_t)c->B * c->n));
    VCHCHK(up(c, c->dts, dt, M));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    LAUNCH_LDS(-1, k1d_forward, dim3(c->B), dim3(T1), c->lds_bytes, c->P, c->n, c->h, c->lvl, M, (const double *)c->dts,
            (const double *)c->tmp[0], (const double *)(u ? c->u_hist : nullptr), u_rows, hs1(c), c->phi_hist, hs1(c),
            c->scratch, c->stats_dev, (const int *)nullptr);
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipMemcpyAsync(c->stats_host, c->stats_dev, sizeof(int) * 8 * c->B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->rows_res = M + 2;
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        for (int b = 0; b < c->B; ++b) {
            stats->newton_iters += c->stats_host[b * 8 + 0];
            stats->linear_solves += c->stats_host[b * 8 + 1];
            stats->armijo_trials += c->stats_host[b * 8 + 2];
            stats->linear_iters += c->stats_host[b * 8 + 3];      // 1D: steps left through the line-search-failure return
        }
        stats->seconds = ms * 1e-3;
    }
    for (int b = 0; b < c->B; ++b)
        if (c->stats_host[b * 8 + 4]) return vch_fail(VCH_ERR_STATE, "Non-finite mass_defect; check phi bounds/log regularization.");
    if (phi_hist_out) VCHCHK(down_hist(c, phi_hist_out, c->phi_hist, M + 2));
    return 0;
}

extern "C" int vch1d_backward(vch1d_ctx *c, const double *phi_hist, int rows, const double *t_hist, double h, double b1,
                              double b2, const double *phi_Q, const double *phi_T, double *p_out, double *q_out,
                              double *r_out) {
    CTXCHK(c);
    ARGCHK(t_hist && rows >= 2 && rows <= c->Mmax + 2, "NULL t_hist or rows out of range");
    ARGCHK(std::fabs(h - c->h) <= 1e-12 * c->h, "grid spacing differs from the context's Lx/N");
    if (phi_hist) {
        VCHCHK(ensure1(c, &c->phi_hist));
        VCHCHK(up_hist(c, c->phi_hist, phi_hist, rows));
        c->rows_res = rows;
    } else if (c->rows_res != rows) {
        return vch_fail(VCH_ERR_STATE, "vch1d_backward: no resident history with %d rows", rows);
    }
    if (phi_Q) {
        VCHCHK(ensure1(c, &c->phiQ));
        VCHCHK(up_hist(c, c->phiQ, phi_Q, rows));
    }
    if (phi_T) VCHCHK(up(c, c->phiT, phi_T, (size_t)c->B * c->n));
    VCHCHK(ensure1(c, &c->p_hist));
    VCHCHK(ensure1(c, &c->q_hist));
    VCHCHK(ensure1(c, &c->r_hist));
    c->pgd_r_valid = false;               // the resident r is no longer the loop's (vch1d_pgd_kkt with refresh == 0)
    const size_t hb = (size_t)c->B * hs1(c) * sizeof(double);
    HIPCHK(hipMemsetAsync(c->p_hist, 0, hb, c->stream));
    HIPCHK(hipMemsetAsync(c->q_hist, 0, hb, c->stream));
    HIPCHK(hipMemsetAsync(c->r_hist, 0, hb, c->stream));
    VCHCHK(up(c, c->tgrid, t_hist, rows));
    VCHCHK(seam_row(c, b1, b2, 0.0, 0.0, 0.0, 0.0));
    LAUNCH_LDS(-1, k1d_backward, dim3(c->B), dim3(T1), c->lds_bytes, c->F, c->n, c->h, c->lvl, rows, (const double *)c->tgrid,
            (const double *)c->phi_hist, (const double *)(phi_Q ? c->phiQ : nullptr),
            (const double *)(phi_T ? c->phiT : nullptr), (const double *)c->seam_tab, 0, c->p_hist, c->q_hist, c->r_hist, hs1(c),
            c->scratch);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (p_out) VCHCHK(down_hist(c, p_out, c->p_hist, rows));
    if (q_out) VCHCHK(down_hist(c, q_out, c->q_hist, rows));
    if (r_out) VCHCHK(down_hist(c, r_out, c->r_hist, rows));
    return 0;
}

// np.trapezoid weights of the n abscissae t: of the caller's grid (C1:57), or of t_hist over all rows (C1:55-73), where the
// duplicated t = 0 row gets 0
static std::vector<double> trapz_w1(const double *t, int n) {
    std::vector<double> w(n, 0.0);
    for (int i = 0; i + 1 < n; ++i) {
        const double d = t[i + 1] - t[i];
        w[i] += 0.5 * d;
        w[i + 1] += 0.5 * d;
    }
    return w;
}

// what a group-mode function seam needs beyond its histories: the column norms, s per group and the time weights of t_hist
// (NULL: not needed) on the device
static int gp_tables(vch1d_ctx *c, const double *t_hist, int rows) {
    VCHCHK(dalloc1(c, &c->gp_wt, c->Mmax + 2));
    VCHCHK(dalloc1(c, &c->gp_col, (size_t)c->B * c->n));
    VCHCHK(dalloc1(c, &c->gp_s, (size_t)c->B * gp_ss(c)));
    if (!t_hist) return 0;
    const std::vector<double> wt = trapz_w1(t_hist, rows);
    VCHCHK(up(c, c->gp_wt, wt.data(), rows));
    HIPCHK(hipStreamSynchronize(c->stream));          // wt is a local
    return 0;
}

// J4 of a group mode for one trajectory: s [rows][4] the level sums of k1d_cost (TIME: column 2 = sum_i wx_i u^2), t [rows];
// colsq [n] the squared column norms of k1d_colnorm and wx [n] (SPACE).  Host sums in index order.
static double gp_j4(int mode, const double *s, const double *t, int rows, const double *colsq, const double *wx, int n) {
    double acc = 0;
    if (mode == VCH_SPARSITY_TIME)
        for (int k = 0; k + 1 < rows; ++k) acc += (t[k + 1] - t[k]) * (std::sqrt(s[(k + 1) * 4 + 2]) + std::sqrt(s[k * 4 + 2])) / 2.0;
    else
        for (int i = 0; i < n; ++i) acc += wx[i] * std::sqrt(colsq[i]);
    return acc;
}

static int cost1_seam(vch1d_ctx *c, const double *phi_hist, const double *u, const double *phi_Q, const double *phi_T, int rows,
                      const double *x, const double *t_hist, const vch_opt_params *o, int mode, double *J_out) {
    VCHCHK(ensure1(c, &c->phi_hist));
    VCHCHK(up_hist(c, c->phi_hist, phi_hist, rows));
    c->rows_res = rows;
    if (u) { VCHCHK(ensure1(c, &c->u_hist)); VCHCHK(up_hist(c, c->u_hist, u, rows)); }
    if (phi_Q) { VCHCHK(ensure1(c, &c->phiQ)); VCHCHK(up_hist(c, c->phiQ, phi_Q, rows)); }
    if (phi_T) VCHCHK(up(c, c->phiT, phi_T, (size_t)c->B * c->n));
    const std::vector<double> wx = trapz_w1(x, c->n);
    VCHCHK(up(c, c->wx, wx.data(), c->n));
    LAUNCH(k1d_cost, dim3(rows, c->B), dim3(T1), c->n, rows, (const double *)c->wx, (const double *)c->phi_hist,
            (const double *)(u ? c->u_hist : nullptr), (const double *)(phi_Q ? c->phiQ : nullptr),
            (const double *)(phi_T ? c->phiT : nullptr), hs1(c), c->cost_lvl);
    VCHCHK(down(c, c->cost_host, c->cost_lvl, (size_t)c->B * rows * 4));
    if (mode == VCH_SPARSITY_SPACE) {
        c->gp_col_host.assign((size_t)c->B * c->n, 0.0);
        if (u) {
            VCHCHK(gp_tables(c, t_hist, rows));
            LAUNCH(k1d_colnorm, dim3(gp_nblk(c), c->B), dim3(GC_T), c->n, rows, (const double *)c->u_hist, hs1(c), (const int *)nullptr,
                   (const double *)c->gp_wt, c->gp_col);
            VCHCHK(down(c, c->gp_col_host.data(), c->gp_col, c->gp_col_host.size()));
        }
    }
    for (int b = 0; b < c->B; ++b) {
        const double *s = c->cost_host + (size_t)b * rows * 4;
        double i1 = 0, i3 = 0, i4 = 0;
        for (int k = 0; k + 1 < rows; ++k) {
            const double d = t_hist[k + 1] - t_hist[k];
            i1 += d * (s[(k + 1) * 4 + 0] + s[k * 4 + 0]) / 2.0;
            i3 += d * (s[(k + 1) * 4 + 2] + s[k * 4 + 2]) / 2.0;
            i4 += d * (s[(k + 1) * 4 + 3] + s[k * 4 + 3]) / 2.0;
        }
        if (mode != VCH_SPARSITY_FULL) i4 = gp_j4(mode, s, t_hist, rows, c->gp_col_host.data() + (size_t)b * c->n, wx.data(), c->n);
        double *J = J_out + 5 * b;
        J[0] = (o->b1 / 2.0) * i1;
        J[1] = (o->b2 / 2.0) * s[(rows - 1) * 4 + 1];
        J[2] = (o->b3 / 2.0) * i3;
        J[3] = o->kappa_sparsity * i4;
        J[4] = J[0] + J[1] + J[2] + J[3];
    }
    return 0;
}

extern "C" int vch1d_cost(vch1d_ctx *c, const double *phi_hist, const double *u, const double *phi_Q, const double *phi_T,
                          int rows, const double *x, const double *t_hist, const vch_opt_params *o, double *J_out) {
    CTXCHK(c);
    ARGCHK(phi_hist && x && t_hist && o && J_out && rows >= 2 && rows <= c->Mmax + 2, "NULL argument or rows out of range");
    return cost1_seam(c, phi_hist, u, phi_Q, phi_T, rows, x, t_hist, o, VCH_SPARSITY_FULL, J_out);
}

extern "C" int vch1d_cost_g(vch1d_ctx *c, const double *phi_hist, const double *u, const double *phi_Q, const double *phi_T,
                            int rows, const double *x, const double *t_hist, const vch_opt_params *o, int sparsity, double *J_out) {
    CTXCHK(c);
    ARGCHK(phi_hist && x && t_hist && o && J_out && rows >= 2 && rows <= c->Mmax + 2, "NULL argument or rows out of range");
    ARGCHK(sparsity >= VCH_SPARSITY_FULL && sparsity <= VCH_SPARSITY_SPACE, "sparsity is none of VCH_SPARSITY_FULL, _TIME, _SPACE");
    return cost1_seam(c, phi_hist, u, phi_Q, phi_T, rows, x, t_hist, o, sparsity, J_out);
}

extern "C" int vch1d_grad_prox(vch1d_ctx *c, const double *u, const double *r, int rows, const double *alpha,
                               const vch_opt_params *o, double *u_out) {
    CTXCHK(c);
    ARGCHK(u && r && alpha && o && u_out && rows >= 1 && rows <= c->Mmax + 2, "NULL argument or rows out of range");
    VCHCHK(ensure1(c, &c->u_hist));
    VCHCHK(ensure1(c, &c->r_hist));
    VCHCHK(ensure1(c, &c->u_trial));
    c->pgd_r_valid = false;               // as in vch1d_backward
    VCHCHK(up_hist(c, c->u_hist, u, rows));
    VCHCHK(up_hist(c, c->r_hist, r, rows));
    VCHCHK(up(c, c->alpha_dev, alpha, c->B));
    VCHCHK(seam_row(c, 0.0, 0.0, o->b3, o->kappa_sparsity, o->u_min, o->u_max));
    LAUNCH(k1d_grad_prox, dim3(rows, c->B), dim3(T1), c->n, (const double *)c->u_hist, (const double *)c->r_hist, hs1(c),
            (const double *)c->alpha_dev, (const double *)c->seam_tab, 0, c->u_trial, (double *)nullptr);
    return down_hist(c, u_out, c->u_trial, rows);
}

// The group prox kernels for the trajectories of `mode` (mode_dev NULL: all of them): u, r -> uout (or NULL), s in gp_s, the
// change partials in chg_t (rows kernel, [B][rows][2]) or gp_chg (column kernel); tab / stride as for k1d_grad_prox.
static int gp_launch(vch1d_ctx *c, int mode, const int *mode_dev, int rows, const double *alpha_dev, const double *tab, int stride,
                     double *uout, double *chg_t) {
#define GP_ROWS(NV)                                                                                                        \
    LAUNCH((k1d_group_prox_rows<NV>), dim3(rows, c->B), dim3(T1), c->n, (const double *)c->u_hist, (const double *)c->r_hist, \
           hs1(c), alpha_dev, tab, stride, mode_dev, (const double *)c->wx, uout, c->gp_s, gp_ss(c), chg_t)
    if (mode == VCH_SPARSITY_TIME) {
        switch (gp_rows_nv(c->n)) {       // the values per thread that hold a row
        case 1: GP_ROWS(1); break;
        case 2: GP_ROWS(2); break;
        case 4: GP_ROWS(4); break;
        default: GP_ROWS(GP_NV);
        }
    } else
        LAUNCH(k1d_group_prox_cols, dim3(gp_nblk(c), c->B), dim3(GC_T), c->n, rows, (const double *)c->u_hist,
               (const double *)c->r_hist, hs1(c), alpha_dev, tab, stride, mode_dev, (const double *)c->gp_wt, uout, c->gp_s, gp_ss(c),
               c->gp_chg);
#undef GP_ROWS
    return 0;
}

extern "C" int vch1d_grad_prox_g(vch1d_ctx *c, const double *u, const double *r, int rows, const double *x, const double *t_hist,
                                 const double *alpha, const vch_opt_params *o, int sparsity, double *u_out, double *scale_out) {
    CTXCHK(c);
    ARGCHK(sparsity >= VCH_SPARSITY_FULL && sparsity <= VCH_SPARSITY_SPACE, "sparsity is none of VCH_SPARSITY_FULL, _TIME, _SPACE");
    if (sparsity == VCH_SPARSITY_FULL) return vch1d_grad_prox(c, u, r, rows, alpha, o, u_out);
    ARGCHK(u && r && alpha && o && u_out && rows >= 1 && rows <= c->Mmax + 2, "NULL argument or rows out of range");
    ARGCHK(sparsity == VCH_SPARSITY_TIME ? x != nullptr : (t_hist != nullptr), "NULL x (TIME) or t_hist (SPACE): the group's weights");
    ARGCHK(o->u_min <= 0.0 && o->u_max >= 0.0, "a group mode needs a box with u_min <= 0 <= u_max");
    ARGCHK(std::isfinite(o->kappa_sparsity) && o->kappa_sparsity >= 0, "kappa_sparsity must be finite and >= 0");
    VCHCHK(ensure1(c, &c->u_hist));
    VCHCHK(ensure1(c, &c->r_hist));
    VCHCHK(ensure1(c, &c->u_trial));
    VCHCHK(dalloc1(c, &c->gp_chg, (size_t)c->B * gp_nblk(c) * 2));
    c->pgd_r_valid = false;               // as in vch1d_backward
    VCHCHK(up_hist(c, c->u_hist, u, rows));
    VCHCHK(up_hist(c, c->r_hist, r, rows));
    VCHCHK(up(c, c->alpha_dev, alpha, c->B));
    VCHCHK(seam_row(c, 0.0, 0.0, o->b3, o->kappa_sparsity, o->u_min, o->u_max));
    if (sparsity == VCH_SPARSITY_TIME) {
        VCHCHK(gp_tables(c, nullptr, 0));
        const std::vector<double> wx = trapz_w1(x, c->n);
        VCHCHK(up(c, c->wx, wx.data(), c->n));
        HIPCHK(hipStreamSynchronize(c->stream));      // wx is a local
    } else {
        VCHCHK(gp_tables(c, t_hist, rows));
    }
    VCHCHK(gp_launch(c, sparsity, nullptr, rows, c->alpha_dev, c->seam_tab, 0, c->u_trial, nullptr));
    if (scale_out) {
        const int ng = sparsity == VCH_SPARSITY_TIME ? rows : c->n;
        for (int b = 0; b < c->B; ++b)
            HIPCHK(hipMemcpyAsync(scale_out + (size_t)b * ng, c->gp_s + b * gp_ss(c), sizeof(double) * ng, hipMemcpyDeviceToHost,
                                  c->stream));
    }
    return down_hist(c, u_out, c->u_trial, rows);
}

extern "C" int vch1d_free_energy(vch1d_ctx *c, const double *phi_hist, int rows, const double *w_hist, double h, double eps,
                                 double *E_out) {
    CTXCHK(c);
    ARGCHK(phi_hist && E_out && rows >= 1 && rows <= c->Mmax + 2 && h > 0, "NULL argument, rows out of range or h <= 0");
    VCHCHK(ensure1(c, &c->phi_hist));
    VCHCHK(up_hist(c, c->phi_hist, phi_hist, rows));
    c->rows_res = rows;
    if (w_hist) {
        VCHCHK(ensure1(c, &c->u_trial));
        VCHCHK(up_hist(c, c->u_trial, w_hist, rows));
    }
    LAUNCH(k1d_energy, dim3(rows, c->B), dim3(T1), c->n, c->P.c1, c->P.c2, eps > 0 ? eps : 1e-8, (const double *)c->phi_hist,
            (const double *)(w_hist ? c->u_trial : nullptr), hs1(c), c->cost_lvl);
    VCHCHK(down(c, c->cost_host, c->cost_lvl, (size_t)c->B * rows * 4));
    for (long k = 0; k < (long)c->B * rows; ++k) {
        const double *s = c->cost_host + 4 * k;
        double E = (c->P.kappa / (2.0 * h)) * s[0] + h * s[1];
        if (w_hist) E -= h * s[2];
        E_out[k] = E;
    }
    return 0;
}

// ------------------------------------------------------------------------------------
// device-resident PGD loop (G1:333-477): control, state history, adjoint and targets stay in HBM
// ------------------------------------------------------------------------------------
// J[b][5] of (phi, u) on the device; wx already uploaded
static int cost1_core(vch1d_ctx *c, const double *phi_dev, const double *u_dev, int rows, double *J_out,
                      double *raw_out = nullptr /* [B][2] = {int int (phi - phi_Q)^2, int (phi_end - phi_T)^2} */) {
    LAUNCH(k1d_cost, dim3(rows, c->B), dim3(T1), c->n, rows, (const double *)c->wx, phi_dev, u_dev,
            (const double *)c->phiQ, (const double *)c->phiT, hs1(c), c->cost_lvl);
    VCHCHK(down(c, c->cost_host, c->cost_lvl, (size_t)c->B * rows * 4));
    if (gp_any(c, VCH_SPARSITY_SPACE)) {      // the squared column norms of the SPACE trajectories
        LAUNCH(k1d_colnorm, dim3(gp_nblk(c), c->B), dim3(GC_T), c->n, rows, u_dev, hs1(c), (const int *)c->mode_dev,
               (const double *)c->gp_wt, c->gp_col);
        VCHCHK(down(c, c->gp_col_host.data(), c->gp_col, c->gp_col_host.size()));
    }
    const double *t = c->t_host.data();
    for (int b = 0; b < c->B; ++b) {
        const double *s = c->cost_host + (size_t)b * rows * 4;
        double i1 = 0, i3 = 0, i4 = 0;
        for (int k = 0; k + 1 < rows; ++k) {
            const double d = t[k + 1] - t[k];
            i1 += d * (s[(k + 1) * 4 + 0] + s[k * 4 + 0]) / 2.0;
            i3 += d * (s[(k + 1) * 4 + 2] + s[k * 4 + 2]) / 2.0;
            i4 += d * (s[(k + 1) * 4 + 3] + s[k * 4 + 3]) / 2.0;
        }
        if (gp_mode(c, b) != VCH_SPARSITY_FULL)
            i4 = gp_j4(gp_mode(c, b), s, t, rows, c->gp_col_host.data() + (size_t)b * c->n, c->wx_host.data(), c->n);
        const vch_opt_params *o = &c->opts[b];
        double *J = J_out + 5 * b;
        J[0] = (o->b1 / 2.0) * i1;
        J[1] = (o->b2 / 2.0) * s[(rows - 1) * 4 + 1];
        J[2] = (o->b3 / 2.0) * i3;
        J[3] = o->kappa_sparsity * i4;
        J[4] = J[0] + J[1] + J[2] + J[3];
        if (raw_out) {
            raw_out[2 * b] = i1;
            raw_out[2 * b + 1] = s[(rows - 1) * 4 + 1];
        }
    }
    return 0;
}

// int_t int_x a^2 (rows > 1) or int_x a^2 (rows == 1) per trajectory with the cost's weights; arr [B][stride]
static int l2sq1_core(vch1d_ctx *c, const double *arr, long stride, int rows, double *out) {
    LAUNCH(k1d_cost, dim3(rows, c->B), dim3(T1), c->n, rows, (const double *)c->wx, arr, (const double *)nullptr,
            (const double *)nullptr, (const double *)nullptr, stride, c->cost_lvl);
    VCHCHK(down(c, c->cost_host, c->cost_lvl, (size_t)c->B * rows * 4));
    const double *t = c->t_host.data();
    for (int b = 0; b < c->B; ++b) {
        const double *s = c->cost_host + (size_t)b * rows * 4;
        if (rows == 1) { out[b] = s[0]; continue; }
        double acc = 0;
        for (int k = 0; k + 1 < rows; ++k) acc += (t[k + 1] - t[k]) * (s[(k + 1) * 4] + s[k * 4]) / 2.0;
        out[b] = acc;
    }
    return 0;
}

// bad_out (NULL for every caller but the Newton rounds): [B], a march that reports a non-finite mass defect does not fail
// the call; bad_out[b] says whose did, and that trajectory's flag is cleared on the device, where a later march that it
// sits out would find it again.  A skipped trajectory's entry is what its last march left.
static int fwd1_core(vch1d_ctx *c, const double *u_dev, int rows, double *hist_dev, const int *skip_dev, int *bad_out = nullptr) {
    const int M = rows - 2;
    LAUNCH_LDS(-1, k1d_forward, dim3(c->B), dim3(T1), c->lds_bytes, c->P, c->n, c->h, c->lvl, M, (const double *)c->dts,
            (const double *)c->phi0_dev, u_dev, rows, hs1(c), hist_dev, hs1(c), c->scratch, c->stats_dev, skip_dev);
    HIPCHK(hipMemcpyAsync(c->stats_host, c->stats_dev, sizeof(int) * 8 * c->B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < c->B; ++b) {
        const bool bad = c->stats_host[b * 8 + 4] != 0;
        if (bad && !bad_out) return vch_fail(VCH_ERR_STATE, "Non-finite mass_defect; check phi bounds/log regularization.");
        if (bad_out) bad_out[b] = bad;
        if (bad) HIPCHK(hipMemsetAsync(c->stats_dev + b * 8 + 4, 0, sizeof(int), c->stream));
    }
    return 0;
}

// adjoint sweep of the resident state history into the resident p, q, r; trajectory b with b1, b2 of row b of the table
static int backward1_core(vch1d_ctx *c, int rows) {
    const size_t hb = (size_t)c->B * hs1(c) * sizeof(double);
    HIPCHK(hipMemsetAsync(c->p_hist, 0, hb, c->stream));
    HIPCHK(hipMemsetAsync(c->q_hist, 0, hb, c->stream));
    HIPCHK(hipMemsetAsync(c->r_hist, 0, hb, c->stream));
    LAUNCH_LDS(-1, k1d_backward, dim3(c->B), dim3(T1), c->lds_bytes, c->F, c->n, c->h, c->lvl, rows, (const double *)c->tgrid,
            (const double *)c->phi_hist, (const double *)c->phiQ, (const double *)c->phiT, (const double *)c->opt_tab, OPT1_STRIDE,
            c->p_hist, c->q_hist, c->r_hist, hs1(c), c->scratch);
    return 0;
}

// vch1d_pgd_init_v and vch1d_pgd_init_g (fn: who the messages name).  sparsity NULL: every trajectory VCH_SPARSITY_FULL.
static int pgd_init1(vch1d_ctx *c, const char *fn, const double *phi0, const double *phi_T, const double *phi_Q, const double *x,
                     const double *t_hist, int rows, const double *dt, const vch_opt_params *opts, int n_opts, const double *u0,
                     const double *alpha0, const int32_t *sparsity, int n_sparsity, double *J0_out) {
    if (!(phi0 && phi_T && x && t_hist && dt && opts)) return vch_fail(VCH_ERR_ARG, "%s: NULL argument", fn);
    if (!(rows >= 3 && rows <= c->Mmax + 2)) return vch_fail(VCH_ERR_ARG, "%s: rows out of range (3..max_steps+2)", fn);
    if (!(n_opts == 1 || n_opts == c->B)) return vch_fail(VCH_ERR_ARG, "%s: n_opts must be 1 or the context's batch", fn);
    const int B = c->B, M = rows - 2;
    for (int k = 0; k < M; ++k)
        if (!(dt[k] > 0)) return vch_fail(VCH_ERR_ARG, "%s: dt must be positive", fn);
    // all of this before anything is copied or launched, or any resident state changes
    for (int b = 0; b < B; ++b)
        if (const char *bad = vch_pgd_check(opts, n_opts, alpha0, b))
            return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: %s", fn, b, bad);
    bool grouped = false;
    if (sparsity) {
        if (!(n_sparsity == 1 || n_sparsity == B)) return vch_fail(VCH_ERR_ARG, "%s: n_sparsity must be 1 or the context's batch", fn);
        for (int b = 0; b < B; ++b) {
            const int m = sparsity[n_sparsity == 1 ? 0 : b];
            const vch_opt_params &o = vch_pgd_opt(opts, n_opts, b);
            if (m < VCH_SPARSITY_FULL || m > VCH_SPARSITY_SPACE)
                return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: sparsity %d is none of VCH_SPARSITY_FULL, _TIME, _SPACE", fn, b, m);
            if (m != VCH_SPARSITY_FULL && !(o.u_min <= 0.0 && o.u_max >= 0.0))
                return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: a group mode needs a box with u_min <= 0 <= u_max", fn, b);
            grouped = grouped || m != VCH_SPARSITY_FULL;
        }
    }
    c->modes.assign(B, VCH_SPARSITY_FULL);
    if (sparsity)
        for (int b = 0; b < B; ++b) c->modes[b] = sparsity[n_sparsity == 1 ? 0 : b];
    c->opts.resize(B);
    std::vector<double> &tab = c->opt_tab_host;
    tab.assign((size_t)B * OPT1_STRIDE, 0.0);
    for (int b = 0; b < B; ++b) {
        const vch_opt_params &o = c->opts[b] = vch_pgd_opt(opts, n_opts, b);
        double *row = tab.data() + (size_t)b * OPT1_STRIDE;
        row[OPT1_B1] = o.b1; row[OPT1_B2] = o.b2; row[OPT1_B3] = o.b3;
        row[OPT1_KS] = o.kappa_sparsity; row[OPT1_UMIN] = o.u_min; row[OPT1_UMAX] = o.u_max;
    }
    c->pgd_ready = false;                 // until this init has gone through
    c->pgd_r_valid = false;
    c->pgd_rows = rows;
    c->t_host.assign(t_hist, t_hist + rows);
    c->dt_host.assign(dt, dt + M);
    c->x_host.assign(x, x + c->n);
    c->pgd_synced.assign(B, 0);
    {   // what the resident problem needs beyond the buffers of vch1d_create: all of it, or nothing more than there was
        vch_group g(c->pool);
        double **hs[] = {&c->phi_hist, &c->u_hist, &c->u_trial, &c->phiQ, &c->p_hist, &c->q_hist, &c->r_hist, &c->phi_trial};
        for (auto p : hs) VCHCHK(ensure1(c, p));
        VCHCHK(dalloc1(c, &c->phi0_dev, (size_t)B * c->n));
        VCHCHK(dalloc1(c, &c->chg_dev, (size_t)B * (c->Mmax + 2) * 2));
        VCHCHK(dalloc1(c, &c->tp_dev, c->Mmax + 2));
        if (!c->skip_dev) MEMCHK(c->pool.dev(&c->skip_dev, sizeof(int) * B));
        VCHCHK(dalloc1(c, &c->opt_tab, tab.size()));
        if (!c->kkt_cnt) MEMCHK(c->pool.dev(&c->kkt_cnt, sizeof(long long) * 4 * B));
        VCHCHK(dalloc1(c, &c->kkt_nrm, 2 * (size_t)B));
        if (grouped) {      // the mode table and what the group kernels write
            if (!c->mode_dev) MEMCHK(c->pool.dev(&c->mode_dev, sizeof(int) * B));
            VCHCHK(dalloc1(c, &c->gp_wt, c->Mmax + 2));
            VCHCHK(dalloc1(c, &c->gp_s, (size_t)B * gp_ss(c)));
            VCHCHK(dalloc1(c, &c->gp_chg, (size_t)B * gp_nblk(c) * 2));
            VCHCHK(dalloc1(c, &c->gp_col, (size_t)B * c->n));
            VCHCHK(dalloc1(c, &c->gp_one, B));
        }
        g.keep();
    }
    if (grouped) {
        c->gp_chg_host.assign((size_t)B * gp_nblk(c) * 2, 0.0);
        c->gp_col_host.assign((size_t)B * c->n, 0.0);
        const std::vector<double> wt = trapz_w1(t_hist, rows), one(B, 1.0);
        HIPCHK(hipMemcpyAsync(c->mode_dev, c->modes.data(), sizeof(int) * B, hipMemcpyHostToDevice, c->stream));
        VCHCHK(up(c, c->gp_wt, wt.data(), rows));
        VCHCHK(up(c, c->gp_one, one.data(), B));
        HIPCHK(hipStreamSynchronize(c->stream));      // wt, one are locals
    }
    VCHCHK(up(c, c->opt_tab, tab.data(), tab.size()));
    c->chg_host.assign((size_t)B * rows * 2, 0.0);
    VCHCHK(up(c, c->phi0_dev, phi0, (size_t)B * c->n));
    VCHCHK(up(c, c->phiT, phi_T, (size_t)B * c->n));
    VCHCHK(up(c, c->dts, dt, M));
    VCHCHK(up(c, c->tgrid, t_hist, rows));
    const std::vector<double> wx = trapz_w1(x, c->n);
    VCHCHK(up(c, c->wx, wx.data(), c->n));
    HIPCHK(hipStreamSynchronize(c->stream));          // wx is a local
    c->wx_host = wx;
    // u = 0 and the uncontrolled march (G1:341), or the caller's u0 as given (not clipped) and the march under it
    HIPCHK(hipMemsetAsync(c->u_hist, 0, sizeof(double) * B * hs1(c), c->stream));
    if (u0) VCHCHK(up_hist(c, c->u_hist, u0, rows));
    VCHCHK(fwd1_core(c, u0 ? c->u_hist : nullptr, rows, c->phi_hist, nullptr));
    c->rows_res = rows;
    if (phi_Q) {
        VCHCHK(up_hist(c, c->phiQ, phi_Q, rows));
    } else {
        std::vector<double> tp(rows);
        const double Tend = t_hist[rows - 1] > 0 ? t_hist[rows - 1] : 1.0;
        for (int k = 0; k < rows; ++k) tp[k] = t_hist[k] / Tend;
        VCHCHK(up(c, c->tp_dev, tp.data(), rows));
        HIPCHK(hipStreamSynchronize(c->stream));
        LAUNCH(k1d_ramp, dim3(rows, B), dim3(T1), c->n, (const double *)c->tp_dev, (const double *)c->phi_hist,
                (const double *)c->phiT, hs1(c), c->phiQ);
    }
    std::vector<double> J(5 * B);
    VCHCHK(cost1_core(c, c->phi_hist, c->u_hist, rows, J.data()));
    c->pgd.denQ2.assign(B, 0.0);
    c->pgd.denT2.assign(B, 0.0);
    VCHCHK(l2sq1_core(c, c->phiQ, hs1(c), rows, c->pgd.denQ2.data()));
    VCHCHK(l2sq1_core(c, c->phiT, c->n, 1, c->pgd.denT2.data()));
    c->pgd.rms = std::sqrt(std::max(x[c->n - 1] - x[0], 1e-30) * std::max(t_hist[rows - 1] - t_hist[0], 1e-30));
    c->pgd.reset(B, J.data(), c->opts.data(), alpha0);
    if (J0_out) memcpy(J0_out, J.data(), sizeof(double) * 5 * B);
    c->pgd_ready = true;
    return 0;
}

extern "C" int vch1d_pgd_init_v(vch1d_ctx *c, const double *phi0, const double *phi_T, const double *phi_Q, const double *x,
                                const double *t_hist, int rows, const double *dt, const vch_opt_params *opts, int n_opts,
                                const double *u0, const double *alpha0, double *J0_out) {
    CTXCHK(c);
    return pgd_init1(c, "vch1d_pgd_init_v", phi0, phi_T, phi_Q, x, t_hist, rows, dt, opts, n_opts, u0, alpha0, nullptr, 0, J0_out);
}

extern "C" int vch1d_pgd_init_g(vch1d_ctx *c, const double *phi0, const double *phi_T, const double *phi_Q, const double *x,
                                const double *t_hist, int rows, const double *dt, const vch_opt_params *opts, int n_opts,
                                const double *u0, const double *alpha0, const int32_t *sparsity, int n_sparsity, double *J0_out) {
    CTXCHK(c);
    if (!sparsity) return vch_fail(VCH_ERR_ARG, "vch1d_pgd_init_g: NULL sparsity");
    return pgd_init1(c, "vch1d_pgd_init_g", phi0, phi_T, phi_Q, x, t_hist, rows, dt, opts, n_opts, u0, alpha0, sparsity, n_sparsity,
                     J0_out);
}

extern "C" int vch1d_pgd_init(vch1d_ctx *c, const double *phi0, const double *phi_T, const double *phi_Q, const double *x,
                              const double *t_hist, int rows, const double *dt, const vch_opt_params *opt, double *J0_out) {
    return vch1d_pgd_init_v(c, phi0, phi_T, phi_Q, x, t_hist, rows, dt, opt, 1, nullptr, nullptr, J0_out);
}

static int copy_traj1(vch1d_ctx *c, double *dst, const double *src, int b, int rows) {
    HIPCHK(hipMemcpyAsync(dst + b * hs1(c), src + b * hs1(c), sizeof(double) * rows * c->n, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

extern "C" int vch1d_pgd_iterate(vch1d_ctx *c, int n_iters, double *cost_out, double *alpha_out, int32_t *trials_out,
                                 double *change_out, double *seconds_out) {
    CTXCHK(c);
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch1d_pgd_iterate: call vch1d_pgd_init first");
    ARGCHK(n_iters >= 1, "n_iters must be >= 1");
    const int B = c->B, rows = c->pgd_rows;
    constexpr vch_pgd_rule R = VCH_PGD_1D;
    vch_pgd_state &st = c->pgd;
    double sec[3] = {0, 0, 0};                // backward, optimistic round, backtracking rounds
    auto tick = [&](hipEvent_t e) { return hipEventRecord(e, c->stream); };
    auto lap = [&]() {
        float ms = 0;
        hipEventSynchronize(c->ev1);
        hipEventElapsedTime(&ms, c->ev0, c->ev1);
        return (double)ms * 1e-3;
    };
    std::vector<double> Jt(5 * B), raw(2 * B);
    st.begin_call(n_iters);
    int done_iters = 0;
    for (int it = 0; it < n_iters; ++it) {
        if (!st.begin_iteration()) break;
        // --- adjoint sweep (G1:356); only r is consumed
        HIPCHK(tick(c->ev0));
        VCHCHK(backward1_core(c, rows));
        c->pgd_r_valid = true;
        HIPCHK(tick(c->ev1));
        sec[0] += lap();
        // round 0: optimistic step with alpha_prev (G1:365-372), which is also the first trial of the line
        // search (alpha_init = alpha_prev, G1:383) -- that repetition is not recomputed; later rounds: alpha *= beta
        for (int round = 0; round < R.rounds; ++round) {
            HIPCHK(tick(c->ev0));
            VCHCHK(up(c, c->alpha_dev, st.alpha.data(), B));
            HIPCHK(hipMemcpyAsync(c->skip_dev, st.accepted.data(), sizeof(int) * B, hipMemcpyHostToDevice, c->stream));
            // k1d_grad_prox for every run of FULL trajectories (without a group mode: one launch over the batch, as ever), the
            // group kernels for the others: the mode table makes them leave a trajectory that is not theirs alone
            for (int b0 = 0; b0 < B;) {
                if (gp_mode(c, b0) != VCH_SPARSITY_FULL) { ++b0; continue; }
                int b1 = b0;
                while (b1 < B && gp_mode(c, b1) == VCH_SPARSITY_FULL) ++b1;
                LAUNCH(k1d_grad_prox, dim3(rows, b1 - b0), dim3(T1), c->n, (const double *)(c->u_hist + b0 * hs1(c)),
                        (const double *)(c->r_hist + b0 * hs1(c)), hs1(c), (const double *)(c->alpha_dev + b0),
                        (const double *)(c->opt_tab + (size_t)b0 * OPT1_STRIDE), OPT1_STRIDE, c->u_trial + b0 * hs1(c),
                        c->chg_dev + (size_t)b0 * rows * 2);
                b0 = b1;
            }
            for (int mode : {VCH_SPARSITY_TIME, VCH_SPARSITY_SPACE})
                if (gp_any(c, mode))
                    VCHCHK(gp_launch(c, mode, c->mode_dev, rows, c->alpha_dev, c->opt_tab, OPT1_STRIDE, c->u_trial, c->chg_dev));
            VCHCHK(fwd1_core(c, c->u_trial, rows, c->phi_trial, c->skip_dev));
            VCHCHK(cost1_core(c, c->phi_trial, c->u_trial, rows, Jt.data(), raw.data()));
            VCHCHK(down(c, c->chg_host.data(), c->chg_dev, (size_t)B * rows * 2));
            if (gp_any(c, VCH_SPARSITY_SPACE)) VCHCHK(down(c, c->gp_chg_host.data(), c->gp_chg, c->gp_chg_host.size()));
            HIPCHK(tick(c->ev1));
            sec[round == 0 ? 1 : 2] += lap();
            bool pending = false;
            for (int b = 0; b < B; ++b) {
                if (st.accepted[b]) continue;
                double d2 = 0, n2 = 0;
                // the partials of the change sums: one per row, or one per workgroup of the column kernel
                const bool cols = gp_mode(c, b) == VCH_SPARSITY_SPACE;
                const int np = cols ? gp_nblk(c) : rows;
                const double *part = cols ? c->gp_chg_host.data() : c->chg_host.data();
                for (int r = 0; r < np; ++r) {
                    d2 += part[((size_t)b * np + r) * 2];
                    n2 += part[((size_t)b * np + r) * 2 + 1];
                }
                vch_pgd_step s;
                const vch_pgd_verdict v =
                    st.judge(R, b, it, round, c->opts[b].alpha_max, Jt[5 * b + 4], d2, n2, raw[2 * b], raw[2 * b + 1], s);
                if (v == VCH_PGD_PENDING) {
                    pending = true;
                    continue;
                }
                VCHCHK(copy_traj1(c, c->u_hist, c->u_trial, b, rows));
                // G1:462-465: on a stop u_k is taken, the state (like the stored cost) keeps the previous iterate
                if (!(v == VCH_PGD_STOP && R.stop_keeps_state)) VCHCHK(copy_traj1(c, c->phi_hist, c->phi_trial, b, rows));
                if (cost_out) cost_out[(long)b * n_iters + it] = Jt[5 * b + 4];
                if (alpha_out) alpha_out[(long)b * n_iters + it] = s.alpha_k;
                if (trials_out) trials_out[(long)b * n_iters + it] = s.count;
                if (change_out) change_out[(long)b * n_iters + it] = s.change;
            }
            HIPCHK(hipStreamSynchronize(c->stream));
            if (!pending) break;
        }
        done_iters = it + 1;
    }
    if (seconds_out) memcpy(seconds_out, sec, sizeof(sec));
    return done_iters;
}

extern "C" int vch1d_pgd_errors(vch1d_ctx *c, int n_iters, double *tracking_out, double *terminal_out) {
    CTXCHK(c);
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch1d_pgd_errors: call vch1d_pgd_init first");
    ARGCHK(c->pgd.errors(n_iters, tracking_out, terminal_out), "n_iters differs from the last vch1d_pgd_iterate call");
    return 0;
}

extern "C" int vch1d_pgd_get(vch1d_ctx *c, int what, double *out) {
    CTXCHK(c);
    ARGCHK(out && what >= 0 && what <= 3, "NULL out or what not in 0..3");
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch1d_pgd_get: call vch1d_pgd_init first");
    const double *src = what == 0 ? c->u_hist : what == 1 ? c->phi_hist : what == 2 ? c->r_hist : c->phiQ;
    return down_hist(c, out, src, c->pgd_rows);
}

extern "C" int vch1d_pgd_kkt(vch1d_ctx *c, int refresh, double tol, int64_t *counts_out, double *stationarity_out) {
    CTXCHK(c);
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch1d_pgd_kkt: call vch1d_pgd_init first");
    ARGCHK(counts_out, "NULL counts_out");
    if (!refresh && !c->pgd_r_valid)
        return vch_fail(VCH_ERR_STATE, "vch1d_pgd_kkt: no adjoint sweep has run since vch1d_pgd_init (pass refresh != 0)");
    const int B = c->B, rows = c->pgd_rows;
    if (!(tol > 0)) tol = 1e-6;
    if (refresh) {      // the adjoint of the resident state, as GD_1D.main() takes it after the loop; it stays in r
        VCHCHK(backward1_core(c, rows));
        c->pgd_r_valid = true;
    }
    LAUNCH(k1d_kkt, dim3(B), dim3(T1), c->n, rows, (const double *)c->u_hist, (const double *)c->r_hist, hs1(c),
            (const double *)c->opt_tab, tol, c->kkt_cnt, c->kkt_nrm);
    if (gp_group(c)) {      // the group modes: their prox at alpha = 1 for the change sums alone, then the counts by groups
        for (int mode : {VCH_SPARSITY_TIME, VCH_SPARSITY_SPACE})
            if (gp_any(c, mode))
                VCHCHK(gp_launch(c, mode, c->mode_dev, rows, c->gp_one, c->opt_tab, OPT1_STRIDE, nullptr, c->chg_dev));
        LAUNCH(k1d_kkt_g, dim3(B), dim3(T1), c->n, rows, (const double *)c->u_hist, (const double *)c->r_hist, hs1(c),
               (const double *)c->opt_tab, (const int *)c->mode_dev, (const double *)c->wx, (const double *)c->gp_wt, tol,
               (const double *)c->chg_dev, (const double *)c->gp_chg, gp_nblk(c), c->kkt_cnt, c->kkt_nrm);
    }
    std::vector<long long> cnt(4 * (size_t)B);
    std::vector<double> nh(2 * (size_t)B);
    HIPCHK(hipMemcpyAsync(cnt.data(), c->kkt_cnt, sizeof(long long) * 4 * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(nh.data(), c->kkt_nrm, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < B; ++b) {
        for (int k = 0; k < 4; ++k) counts_out[4 * b + k] = (int64_t)cnt[4 * b + k];
        if (stationarity_out) stationarity_out[b] = std::sqrt(nh[2 * b]) / (std::sqrt(nh[2 * b + 1]) + 1e-9);
    }
    return 0;
}


// ------------------------------------------------------------------------------------
// exact J'(u)h and J''(u)[h,h] by a tangent march on the device (k1d_tangent)
// ------------------------------------------------------------------------------------
// host [nb][rows][n] -> device [nb][Mmax+2][n]
static int up_hist_n(vch1d_ctx *c, double *dev, const double *host, int rows, int nb) {
    for (int b = 0; b < nb; ++b) VCHCHK(up(c, dev + b * hs1(c), host + (size_t)b * rows * c->n, (size_t)rows * c->n));
    return 0;
}

// What vch1d_second_order and vch1d_hessvec check alike, in two parts around the caller's own NULL checks; nothing is
// copied or launched by either.  The second part fills the step sizes and the [B][3] weight table.
static int so1_check_shape(vch1d_ctx *c, const char *fn, int n_base, int rows, int n_opts, int order) {
    const int B = c->B;
    if (rows < 3 || rows > c->Mmax + 2)
        return vch_fail(VCH_ERR_ARG, "%s: rows = %d outside 3..%d (max_steps + 2)", fn, rows, c->Mmax + 2);
    if (n_base != 1 && n_base != B) return vch_fail(VCH_ERR_ARG, "%s: n_base = %d is neither 1 nor the batch %d", fn, n_base, B);
    if (n_opts != 1 && n_opts != B) return vch_fail(VCH_ERR_ARG, "%s: n_opts = %d is neither 1 nor the batch %d", fn, n_opts, B);
    if (order != 1 && order != 2) return vch_fail(VCH_ERR_ARG, "%s: order = %d is neither 1 nor 2", fn, order);
    return 0;
}
static int so1_check_rest(vch1d_ctx *c, const char *fn, const double *phi_hist, const double *u, int rows, const double *dt,
                          const double *t_hist, const double *x, const double *phi_Q, const double *phi_T,
                          const vch_opt_params *opts, int n_opts, std::vector<double> &dts, std::vector<double> &wts) {
    const int B = c->B;
    if (!t_hist) return vch_fail(VCH_ERR_ARG, "%s: NULL t_hist", fn);
    if (!x) return vch_fail(VCH_ERR_ARG, "%s: NULL x", fn);
    if (!opts) return vch_fail(VCH_ERR_ARG, "%s: NULL opts", fn);
    const int M = rows - 2;
    dts.resize(M);
    for (int k = 0; k < M; ++k) {
        dts[k] = dt ? dt[k] : t_hist[k + 2] - t_hist[k + 1];
        if (!(dts[k] > 0.0) || !std::isfinite(dts[k]))
            return vch_fail(VCH_ERR_ARG, "%s: step %d: dt = %g must be positive and finite", fn, k, dts[k]);
    }
    wts.resize(3 * (size_t)B);
    for (int b = 0; b < B; ++b) {
        const vch_opt_params &o = vch_pgd_opt(opts, n_opts, b);
        if (const char *bad = vch_pgd_check_weights(opts, n_opts, b)) return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: %s", fn, b, bad);
        wts[3 * b] = o.b1; wts[3 * b + 1] = o.b2; wts[3 * b + 2] = o.b3;
    }
    if (!phi_hist && (!c->phi_hist || c->rows_res != rows))
        return vch_fail(VCH_ERR_STATE, "%s: no resident state history with %d rows", fn, rows);
    if ((u == VCH_RESIDENT || phi_Q == VCH_RESIDENT || phi_T == VCH_RESIDENT) && !c->pgd_ready)
        return vch_fail(VCH_ERR_STATE, "%s: VCH_RESIDENT control or targets before vch1d_pgd_init", fn);
    if ((u == VCH_RESIDENT || phi_Q == VCH_RESIDENT) && c->pgd_rows != rows)
        return vch_fail(VCH_ERR_STATE, "%s: the resident PGD problem has %d rows, not %d", fn, c->pgd_rows, rows);
    return 0;
}

// The base point of both calls on the device: the caller's arrays in the call's own buffers, or the resident ones.
struct So1Base {
    const double *phi = nullptr, *u = nullptr, *pq = nullptr, *pt = nullptr;
    long bs = 0, pts = 0;          // strides per trajectory of the histories and of phi_T (0: one base for the batch)
};
static int so1_base(vch1d_ctx *c, const double *phi_hist, const double *u, const double *phi_Q, const double *phi_T, int n_base,
                    int rows, So1Base &S) {
    const int B = c->B, n = c->n;
    S.bs = n_base == 1 ? 0 : hs1(c);
    S.pts = n_base == 1 ? 0 : n;
    if (phi_hist) {
        VCHCHK(ensure1(c, &c->so_base));
        VCHCHK(up_hist_n(c, c->so_base, phi_hist, rows, n_base));
        S.phi = c->so_base;
    } else {
        S.phi = c->phi_hist;
    }
    if (u == VCH_RESIDENT) {
        S.u = c->u_hist;
    } else if (u) {
        VCHCHK(ensure1(c, &c->so_u));
        c->ncg_u_live = false;          // vch1d_newton_trial: the copy an earlier vch1d_hess_cg made is gone
        VCHCHK(up_hist_n(c, c->so_u, u, rows, n_base));
        S.u = c->so_u;
    }
    if (phi_Q == VCH_RESIDENT) {
        S.pq = c->phiQ;
    } else if (phi_Q) {
        VCHCHK(ensure1(c, &c->so_pq));
        VCHCHK(up_hist_n(c, c->so_pq, phi_Q, rows, n_base));
        S.pq = c->so_pq;
    }
    if (phi_T == VCH_RESIDENT) {
        S.pt = c->phiT;
    } else if (phi_T) {
        VCHCHK(dalloc1(c, &c->so_pt, (size_t)B * n));
        VCHCHK(up(c, c->so_pt, phi_T, (size_t)n_base * n));
        S.pt = c->so_pt;
    }
    return 0;
}
// step sizes, t_hist, the trapezoid weights of x and the weight table (host vectors: the caller synchronises before they go)
static int so1_grids_alloc(vch1d_ctx *c) {
    if (c->so_out) return 0;       // the last of the group: there are all five or none
    vch_group g(c->pool);
    VCHCHK(dalloc1(c, &c->so_dts, c->Mmax + 2));
    VCHCHK(dalloc1(c, &c->so_t, c->Mmax + 2));
    VCHCHK(dalloc1(c, &c->so_wx, c->n));
    VCHCHK(dalloc1(c, &c->so_wts, 3 * (size_t)c->B));
    VCHCHK(dalloc1(c, &c->so_out, 6 * (size_t)c->B));
    return g.keep();
}
static int so1_grids(vch1d_ctx *c, const std::vector<double> &dts, const double *t_hist, int rows, const std::vector<double> &wx,
                     const std::vector<double> &wts) {
    VCHCHK(so1_grids_alloc(c));
    VCHCHK(up(c, c->so_dts, dts.data(), rows - 2));
    VCHCHK(up(c, c->so_t, t_hist, rows));
    VCHCHK(up(c, c->so_wx, wx.data(), c->n));
    return up(c, c->so_wts, wts.data(), wts.size());
}
// the base point of a call in the arguments of its kernel (Tan1Args, Hv1Args)
template <class A>
static void so1_args(const vch1d_ctx *c, const So1Base &S, A &G) {
    G.hs = hs1(c);
    G.phi = S.phi; G.u = S.u; G.pq = S.pq; G.pt = S.pt;
    G.phi_s = G.u_s = G.pq_s = S.bs;
    G.pt_s = S.pts;
}
// the stats of a call timed between the context's two events
static void so1_stats(vch1d_ctx *c, vch_stats *stats, int64_t solves, int64_t launches, int64_t host_syncs) {
    if (!stats) return;
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    memset(stats, 0, sizeof(*stats));
    stats->linear_solves = solves;
    stats->launches = launches;
    stats->host_syncs = host_syncs;
    stats->seconds = ms * 1e-3;
}

extern "C" int vch1d_second_order(vch1d_ctx *c, const double *phi_hist, const double *u, int n_base, const double *h,
                                  int rows, const double *dt, const double *t_hist, const double *x, const double *phi_Q,
                                  const double *phi_T, const vch_opt_params *opts, int n_opts, int order, double *out,
                                  double *dphi_hist_out, double *d2phi_hist_out, vch_stats *stats) {
    CTXCHK(c);
    const int B = c->B, n = c->n;
    const char *fn = "vch1d_second_order";
    VCHCHK(so1_check_shape(c, fn, n_base, rows, n_opts, order));
    if (!h) return vch_fail(VCH_ERR_ARG, "%s: NULL direction h", fn);
    if (!out) return vch_fail(VCH_ERR_ARG, "%s: NULL out", fn);
    std::vector<double> dts, wts, wx;
    VCHCHK(so1_check_rest(c, fn, phi_hist, u, rows, dt, t_hist, x, phi_Q, phi_T, opts, n_opts, dts, wts));
    // ---- nothing was launched or copied up to here
    const int M = rows - 2;
    So1Base S;
    VCHCHK(so1_base(c, phi_hist, u, phi_Q, phi_T, n_base, rows, S));
    Tan1Args G{};
    so1_args(c, S, G);
    VCHCHK(ensure1(c, &c->so_h));
    VCHCHK(up_hist(c, c->so_h, h, rows));
    G.hd = c->so_h;
    wx = trapz_w1(x, c->n);
    VCHCHK(so1_grids(c, dts, t_hist, rows, wx, wts));
    G.dts = c->so_dts; G.t = c->so_t; G.wx = c->so_wx; G.wts = c->so_wts; G.out = c->so_out;
    if (dphi_hist_out) { VCHCHK(ensure1(c, &c->so_d1)); G.d1 = c->so_d1; }
    if (d2phi_hist_out && order == 2) { VCHCHK(ensure1(c, &c->so_d2)); G.d2 = c->so_d2; }
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    if (order == 2)
        LAUNCH_LDS(-1, (k1d_tangent<2>), dim3(B), dim3(T1), c->lds_bytes, c->P, n, c->h, c->lvl, rows, G, c->scratch);
    else
        LAUNCH_LDS(-1, (k1d_tangent<1>), dim3(B), dim3(T1), c->lds_bytes, c->P, n, c->h, c->lvl, rows, G, c->scratch);
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    VCHCHK(down(c, out, c->so_out, 6 * (size_t)B));          // synchronises: the host vectors above are done with
    if (dphi_hist_out) VCHCHK(down_hist(c, dphi_hist_out, c->so_d1, rows));
    if (d2phi_hist_out) {
        if (order == 2) VCHCHK(down_hist(c, d2phi_hist_out, c->so_d2, rows));
        else memset(d2phi_hist_out, 0, sizeof(double) * B * rows * n);
    }
    so1_stats(c, stats, (int64_t)order * M * B, 1, 0);
    return 0;
}

// ------------------------------------------------------------------------------------
// exact discrete gradient field and Hessian-vector product by transposed tangent sweeps (k1d_hessvec)
// ------------------------------------------------------------------------------------
extern "C" int vch1d_hessvec(vch1d_ctx *c, const double *phi_hist, const double *u, int n_base, const double *h, int rows,
                             const double *dt, const double *t_hist, const double *x, const double *phi_Q,
                             const double *phi_T, const vch_opt_params *opts, int n_opts, int order, double *grad_out,
                             double *hv_out, double *dots_out, vch_stats *stats) {
    CTXCHK(c);
    const int B = c->B, n = c->n;
    const char *fn = "vch1d_hessvec";
    VCHCHK(so1_check_shape(c, fn, n_base, rows, n_opts, order));
    if (!h && order == 2) return vch_fail(VCH_ERR_ARG, "%s: NULL direction h", fn);
    if (!hv_out && order == 2) return vch_fail(VCH_ERR_ARG, "%s: NULL hv_out", fn);
    std::vector<double> dts, wts, wx;
    VCHCHK(so1_check_rest(c, fn, phi_hist, u, rows, dt, t_hist, x, phi_Q, phi_T, opts, n_opts, dts, wts));
    // ---- nothing was launched or copied up to here
    const int M = rows - 2;
    So1Base S;
    VCHCHK(so1_base(c, phi_hist, u, phi_Q, phi_T, n_base, rows, S));
    Hv1Args G{};
    so1_args(c, S, G);
    if (h) {
        VCHCHK(ensure1(c, &c->so_h));
        VCHCHK(up_hist(c, c->so_h, h, rows));
        G.hd = c->so_h;
    }
    wx = trapz_w1(x, c->n);
    VCHCHK(so1_grids(c, dts, t_hist, rows, wx, wts));
    const std::vector<double> wt = trapz_w1(t_hist, rows);
    if (!c->hv_dots) {             // all three or none
        vch_group g(c->pool);
        VCHCHK(dalloc1(c, &c->hv_wt, c->Mmax + 2));
        VCHCHK(dalloc1(c, &c->hv_mean, (size_t)B * (c->Mmax + 2)));
        VCHCHK(dalloc1(c, &c->hv_dots, 2 * (size_t)B));
        g.keep();
    }
    VCHCHK(up(c, c->hv_wt, wt.data(), rows));
    VCHCHK(ensure1(c, &c->hv_g));
    G.dts = c->so_dts; G.wt = c->hv_wt; G.wx = c->so_wx; G.wts = c->so_wts;
    G.g = c->hv_g; G.mean = c->hv_mean; G.dots = c->hv_dots;
    if (order == 2) {
        VCHCHK(ensure1(c, &c->hv_hv));
        VCHCHK(ensure1(c, &c->hv_v));
        G.hv = c->hv_hv; G.v = c->hv_v;
    }
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    if (order == 2)
        LAUNCH_LDS(-1, (k1d_hessvec<2>), dim3(B), dim3(T1), c->lds_bytes, c->P, n, c->h, c->lvl, rows, G, c->scratch);
    else
        LAUNCH_LDS(-1, (k1d_hessvec<1>), dim3(B), dim3(T1), c->lds_bytes, c->P, n, c->h, c->lvl, rows, G, c->scratch);
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                 // the host vectors above are done with
    if (dots_out) VCHCHK(down(c, dots_out, c->hv_dots, 2 * (size_t)B));
    if (grad_out) VCHCHK(down_hist(c, grad_out, c->hv_g, rows));
    if (hv_out) {
        if (order == 2) VCHCHK(down_hist(c, hv_out, c->hv_hv, rows));
        else memset(hv_out, 0, sizeof(double) * B * rows * n);
    }
    so1_stats(c, stats, (int64_t)(order == 1 ? 1 : 3) * M * B, 1, 0);
    return 0;
}

// ------------------------------------------------------------------------------------
// Lanczos on the reduced Hessian P H P with the basis, the free set and the recurrence on the device (kernels: "Device-
// resident Lanczos" in vch_kernels1d.h)
// ------------------------------------------------------------------------------------
// The block behind kr_sc, in doubles; S = basis slots (the stride of a partial and of a coefficient row), K = entries of
// alpha / beta per trajectory.
struct Kr1Layout {
    size_t part, coef1, coef2, ucoef, alpha, beta, look, scal, amax, lim, stop, steps, box, wt, mean, wtp, ks, total;
    size_t ntpart, nts, ntsum;      // vch1d_newton_trial: its partials [B][chunks][4], the step table [B], the sums [B][4]
    size_t tr;                      // vch1d_hess_cg_tr: [6][B] = radius, xx, xp, pp, c, the pending exit
};
static int kr1_chunks(const vch1d_ctx *c, int rows) { return (int)(((long)rows * c->n + KR1_CHUNK - 1) / KR1_CHUNK); }
static Kr1Layout kr1_layout(const vch1d_ctx *c, int S, int K) {
    const size_t B = c->B, R = c->Mmax + 2;
    Kr1Layout L;
    size_t at = 0;
    auto take = [&](size_t n) { const size_t o = at; at += n; return o; };
    L.part = take(B * kr1_chunks(c, (int)R) * S);
    L.coef1 = take(B * S);
    L.coef2 = take(B * S);
    L.ucoef = take(B * S);
    L.alpha = take(B * K);
    L.beta = take(B * K);
    L.look = take(2 * B);
    L.scal = take(B);
    L.amax = take(B);
    L.lim = take(B);
    L.stop = take(B);
    L.steps = take(B);
    L.box = take(2 * B);
    L.wt = take(R);
    L.mean = take(B * R);
    L.wtp = take(R);
    L.ks = take(B);
    L.ntpart = take(B * kr1_chunks(c, (int)R) * 4);
    L.nts = take(B);
    L.ntsum = take(4 * B);
    L.tr = take(6 * B);
    L.total = at;
    return L;
}
static Kr1Args kr1_args(const vch1d_ctx *c, const Kr1Layout &L, int rows, int slots, long mask_s) {
    double *p = c->kr_sc;
    const Kr1Cells x{p + L.coef1, p + L.coef2, p + L.alpha, p + L.beta, p + L.look, p + L.scal, p + L.amax,
                     (long long *)(p + L.lim), (long long *)(p + L.stop), (long long *)(p + L.steps)};
    return Kr1Args{c->kr_Q, (long)c->B * hs1(c), hs1(c), (long)rows * c->n, slots, c->kr_slots, c->kr_mask, mask_s, x};
}

// The lazy storage of a Krylov call (fn: vch1d_hess_lanczos or vch1d_hess_cg), one group: a refused request gives back what
// this call got and leaves the context usable.  A request for more than the resident storage holds releases that storage
// first.  kr_valid / ncg_valid, in both engines: what an earlier call left resident stays valid until this call has released
// it or has all of its storage, so a refused request leaves the context as it was; then the caller overwrites it.
static int kr1_storage(vch1d_ctx *c, const char *fn, int slots, int k, const double *phi_hist, const double *u, const double *phi_Q,
                       const double *phi_T) {
    const int B = c->B, n = c->n;
    const size_t hist_bytes = (size_t)B * hs1(c) * sizeof(double);
    if (c->kr_Q && (slots > c->kr_slots || k > c->kr_kcap)) {       // a larger basis than the resident storage holds
        c->kr_valid = c->ncg_valid = false;
        c->pool.drop((void **)&c->kr_sc);
        c->pool.drop((void **)&c->kr_mask);
        c->pool.drop((void **)&c->kr_W);
        c->pool.drop((void **)&c->kr_V);
        c->pool.drop((void **)&c->kr_X);
        c->pool.drop((void **)&c->kr_Q);
        c->kr_slots = c->kr_kcap = 0;
    }
    vch_group g(c->pool);
    if (phi_hist) VCHCHK(ensure1(c, &c->so_base));
    if (u && u != VCH_RESIDENT) VCHCHK(ensure1(c, &c->so_u));
    if (phi_Q && phi_Q != VCH_RESIDENT) VCHCHK(ensure1(c, &c->so_pq));
    if (phi_T && phi_T != VCH_RESIDENT) VCHCHK(dalloc1(c, &c->so_pt, (size_t)B * n));
    VCHCHK(so1_grids_alloc(c));
    if (!c->kr_Q) {
        const Kr1Layout L = kr1_layout(c, slots, k);
        const size_t need = (size_t)(slots + 3) * hist_bytes + hist_bytes / 8 + L.total * 8;
        const bool ok = c->pool.dev(&c->kr_Q, (size_t)slots * hist_bytes) == 0 && c->pool.dev(&c->kr_X, hist_bytes) == 0 &&
                        c->pool.dev(&c->kr_V, hist_bytes) == 0 && c->pool.dev(&c->kr_W, hist_bytes) == 0 &&
                        c->pool.dev(&c->kr_mask, hist_bytes / 8) == 0 && c->pool.dev(&c->kr_sc, L.total * 8) == 0;
        if (!ok) {
            (void)hipGetLastError();
            return vch_fail(VCH_ERR_NOMEM,
                            "%s: the Krylov storage needs %zu bytes (%d basis vectors of %zu bytes, three more histories for "
                            "the cached sweep, the tangent and w, %zu bytes of mask, %zu of partials) and was refused",
                            fn, need, slots, hist_bytes, hist_bytes / 8, L.total * 8);
        }
        c->kr_slots = slots;
        c->kr_kcap = k;
    }
    g.keep();
    c->kr_valid = c->ncg_valid = false;
    return 0;
}

// The trapezoid weights wt of t_hist as in vch1d_hessvec and the preconditioner's wt', which gives row 0 (weight zero, but a
// real unknown) the weight of row 1, which duplicates its time; with precond every wt' must be positive and finite.
static int ncg1_weights(const char *fn, const double *t_hist, int rows, int precond, std::vector<double> &wt, std::vector<double> &wtp) {
    wt = trapz_w1(t_hist, rows);
    wtp = wt;
    wtp[0] = wt[1];
    if (precond)
        for (int r = 0; r < rows; ++r)
            if (!(wtp[r] > 0.0) || !std::isfinite(wtp[r]))
                return vch_fail(VCH_ERR_ARG, "%s: row %d: the preconditioner's time weight %g must be positive and finite (t_hist "
                                "must increase from row 1 on)", fn, r, wtp[r]);
    return 0;
}

// What vch1d_hess_lanczos and vch1d_hess_cg have in common once kr1_open is through.
struct Kr1Call {
    std::vector<double> dts, wts, wx, wt, wtp, box, ks;    // host vectors: they live until the first look
    Kr1Layout L;
    long mask_s;
    So1Base Sb;
    Hv1Args G;                          // all but hd
};
// After so1_check_shape and the entry's own checks: the rest of the checks (precond: of the preconditioner's weights), then
// everything ahead of the set-up kernel and the start of the timed span.  cg: the tables of vch1d_hess_cg (wt', kappa_sparsity)
// go up as well.  v0 (or NULL): the start vector or right-hand side, into slot v0_slot of the basis.
static int kr1_open(vch1d_ctx *c, const char *fn, Kr1Call &C, int slots, int k, bool cg, int precond, const double *phi_hist,
                    const double *u, int n_base, int rows, const double *dt, const double *t_hist, const double *x, const double *phi_Q,
                    const double *phi_T, const vch_opt_params *opts, int n_opts, const uint8_t *mask, const double *v0, int v0_slot) {
    if (!mask && !u) return vch_fail(VCH_ERR_ARG, "%s: NULL mask with a NULL (zero) control: no node is free", fn);
    VCHCHK(so1_check_rest(c, fn, phi_hist, u, rows, dt, t_hist, x, phi_Q, phi_T, opts, n_opts, C.dts, C.wts));
    VCHCHK(ncg1_weights(fn, t_hist, rows, precond, C.wt, C.wtp));
    // ---- nothing was launched, copied or allocated up to here
    const int B = c->B, n = c->n;
    const long hs = hs1(c);
    VCHCHK(kr1_storage(c, fn, slots, k, phi_hist, u, phi_Q, phi_T));
    const Kr1Layout &L = C.L = kr1_layout(c, c->kr_slots, c->kr_kcap);
    C.mask_s = (!mask || n_base == B) ? hs : 0;
    double *sc = c->kr_sc;
    VCHCHK(so1_base(c, phi_hist, u, phi_Q, phi_T, n_base, rows, C.Sb));
    C.wx = trapz_w1(x, c->n);
    VCHCHK(so1_grids(c, C.dts, t_hist, rows, C.wx, C.wts));
    C.box.resize(2 * (size_t)B); C.ks.resize(B);
    for (int b = 0; b < B; ++b) {
        const vch_opt_params &o = vch_pgd_opt(opts, n_opts, b);
        C.box[2 * b] = o.u_min;
        C.box[2 * b + 1] = o.u_max;
        C.ks[b] = o.kappa_sparsity;
    }
    VCHCHK(up(c, sc + L.wt, C.wt.data(), rows));
    if (cg) VCHCHK(up(c, sc + L.wtp, C.wtp.data(), rows));
    VCHCHK(up(c, sc + L.box, C.box.data(), C.box.size()));
    if (cg) VCHCHK(up(c, sc + L.ks, C.ks.data(), C.ks.size()));
    if (v0) VCHCHK(up_hist(c, c->kr_Q + (long)v0_slot * B * hs, v0, rows));
    if (mask)
        for (int b = 0; b < n_base; ++b)
            HIPCHK(hipMemcpyAsync(c->kr_mask + (size_t)b * hs, mask + (size_t)b * rows * n, (size_t)rows * n, hipMemcpyHostToDevice,
                                  c->stream));
    HIPCHK(hipMemsetAsync(sc + L.alpha, 0xff, sizeof(double) * 2 * B * c->kr_kcap, c->stream));    // NaN: alpha, beta (resid, curv)
    Hv1Args &G = C.G = Hv1Args{};
    so1_args(c, C.Sb, G);
    G.dts = c->so_dts; G.wt = sc + L.wt; G.wx = c->so_wx; G.wts = c->so_wts;
    G.hv = c->kr_W; G.v = c->kr_V; G.mean = sc + L.mean;
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    return 0;
}
// One product w = H hd into kr_W: the step kernel with or without the cached sweep; a stopped trajectory returns at once.
static int kr1_step(vch1d_ctx *c, int rows, const Hv1Args &G, const long long *stop) {
    if (c->kr_nocache)
        LAUNCH_LDS(-1, (k1d_kr_step<1>), dim3(c->B), dim3(T1), c->lds_bytes, c->P, c->n, c->h, c->lvl, rows, G, stop, (const double *)c->kr_X,
                   c->scratch);
    else
        LAUNCH_LDS(-1, (k1d_kr_step<0>), dim3(c->B), dim3(T1), c->lds_bytes, c->P, c->n, c->h, c->lvl, rows, G, stop, (const double *)c->kr_X,
                   c->scratch);
    return 0;
}

extern "C" int vch1d_hess_lanczos(vch1d_ctx *c, const double *phi_hist, const double *u, int n_base, int rows, const double *dt,
                                  const double *t_hist, const double *x, const double *phi_Q, const double *phi_T,
                                  const vch_opt_params *opts, int n_opts, const uint8_t *mask, double tol, const double *q0, int k,
                                  int reorth, double *alpha_out, double *beta_out, int32_t *steps_out, int64_t *n_free_out,
                                  vch_stats *stats) {
    CTXCHK(c);
    const int B = c->B, n = c->n;
    const char *fn = "vch1d_hess_lanczos";
    VCHCHK(so1_check_shape(c, fn, n_base, rows, n_opts, 2));
    if (!q0) return vch_fail(VCH_ERR_ARG, "%s: NULL q0", fn);
    if (!alpha_out || !beta_out || !steps_out || !n_free_out)
        return vch_fail(VCH_ERR_ARG, "%s: NULL alpha_out, beta_out, steps_out or n_free_out", fn);
    if (k < 1) return vch_fail(VCH_ERR_ARG, "%s: k = %d must be >= 1", fn, k);
    if (reorth != 0 && reorth != 1) return vch_fail(VCH_ERR_ARG, "%s: reorth = %d is neither 0 nor 1", fn, reorth);
    const int M = rows - 2, slots = reorth ? k + 1 : 3;
    Kr1Call C;
    VCHCHK(kr1_open(c, fn, C, slots, k, false, 0, phi_hist, u, n_base, rows, dt, t_hist, x, phi_Q, phi_T, opts, n_opts, mask, q0, 0));
    const Kr1Args K = kr1_args(c, C.L, rows, slots, C.mask_s);
    double *part = c->kr_sc + C.L.part;
    const int S = c->kr_slots, nch = kr1_chunks(c, rows);
    const dim3 kgrid(nch, B);
    auto slot_of = [&](int i) { return c->kr_Q + (long)(i % slots) * B * hs1(c); };
    // the set-up: the free set, q_0 and (once per base point) the gradient sweep, whose yp of every step stays in kr_X
    LAUNCH_LDS(-1, k1d_kr_setup, dim3(B), dim3(T1), c->lds_bytes, c->P, n, c->h, c->lvl, rows, C.G, K, (const double *)(c->kr_sc + C.L.box),
               tol > 0 ? tol : 1e-8, mask ? 0 : 1, k, c->kr_nocache ? 0 : 1, c->kr_X, c->scratch);
    std::vector<double> look(2 * (size_t)B);
    VCHCHK(down(c, look.data(), K.x.look, look.size()));            // the first look; the host vectors above are done with
    for (int b = 0; b < B; ++b) {
        if (look[2 * b] < 1.0) return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: the free set is empty", fn, b);
        if (!(look[2 * b + 1] > 0.0) || !std::isfinite(look[2 * b + 1]))
            return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: the start vector vanishes on the free set (or is not finite)", fn, b);
    }
    // k steps back to back: a stopped trajectory's kernels return at once, the host does not look
    for (int j = 0; j < k; ++j) {
        C.G.hd = slot_of(j);
        VCHCHK(kr1_step(c, rows, C.G, K.x.stop));
        // w = H q_j in kr_W; classical Gram-Schmidt twice against q_first .. q_j, the passes reading w through the mask
        const int first = reorth ? 0 : std::max(j - 1, 0), nv = j + 1 - first;
        LAUNCH((k1d_kr_pass<0>), kgrid, dim3(KR1_T), K, first, nv, c->kr_W, (const double *)nullptr, part);
        LAUNCH(k1d_kr_fin, dim3(B), dim3(KR1_T), K.x, (const double *)part, nch, S, 2, nv, j, k);
        LAUNCH((k1d_kr_pass<1>), kgrid, dim3(KR1_T), K, first, nv, c->kr_W, (const double *)K.x.coef1, part);
        LAUNCH(k1d_kr_fin, dim3(B), dim3(KR1_T), K.x, (const double *)part, nch, S, 3, nv, j, k);
        LAUNCH((k1d_kr_pass<2>), kgrid, dim3(KR1_T), K, first, nv, c->kr_W, (const double *)K.x.coef2, part);
        LAUNCH(k1d_kr_fin, dim3(B), dim3(KR1_T), K.x, (const double *)part, nch, S, 4, nv, j, k);
        LAUNCH(k1d_kr_next, kgrid, dim3(KR1_T), K, (const double *)c->kr_W, slot_of(j + 1));
    }
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    std::vector<long long> steps(B);
    HIPCHK(hipMemcpyAsync(alpha_out, K.x.alpha, sizeof(double) * B * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(beta_out, K.x.beta, sizeof(double) * B * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(steps.data(), K.x.steps, sizeof(long long) * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                        // the second look
    int smin = (int)steps[0], smax = 0;
    int64_t solves = 0;
    for (int b = 0; b < B; ++b) {
        steps_out[b] = (int32_t)steps[b];
        n_free_out[b] = (int64_t)look[2 * b];
        smin = std::min(smin, (int)steps[b]);
        smax = std::max(smax, (int)steps[b]);
        solves += c->kr_nocache ? 3 * (int64_t)M * steps[b] : (int64_t)M * (2 * steps[b] + 1);
    }
    so1_stats(c, stats, solves, 1 + 8 * (int64_t)k, 2);
    c->kr_valid = true;
    c->kr_rows = rows;
    c->kr_run_slots = slots;
    c->kr_min_steps = smin;
    c->kr_window = reorth ? INT32_MAX : (smax <= 2 ? 3 : 0);        // three resident vectors: q_0 is gone once q_3 is stored
    return 0;
}

extern "C" int vch1d_krylov_vector(vch1d_ctx *c, const double *coef, int m, double *out) {
    CTXCHK(c);
    ARGCHK(coef && out, "NULL coef or out");
    ARGCHK(m >= 1, "m must be >= 1");
    if (!c->kr_valid || !c->kr_Q)
        return vch_fail(VCH_ERR_STATE, "vch1d_krylov_vector: no resident basis (call vch1d_hess_lanczos first)");
    if (m > c->kr_window)
        return vch_fail(VCH_ERR_STATE, "vch1d_krylov_vector: m = %d exceeds the %d vectors a run without reorthogonalisation still holds",
                        m, c->kr_window);
    ARGCHK(m <= c->kr_min_steps + 1, "m exceeds the smallest step count of the batch plus one");
    const int B = c->B, S = c->kr_slots, rows = c->kr_rows;
    const Kr1Layout L = kr1_layout(c, c->kr_slots, c->kr_kcap);
    const Kr1Args K = kr1_args(c, L, rows, c->kr_run_slots, 0);
    double *ucoef = c->kr_sc + L.ucoef;
    HIPCHK(hipMemcpy2DAsync(ucoef, sizeof(double) * S, coef, sizeof(double) * m, sizeof(double) * m, (size_t)B, hipMemcpyHostToDevice,
                            c->stream));
    LAUNCH(k1d_kr_lincomb, dim3(kr1_chunks(c, rows), B), dim3(KR1_T), K, m, (const double *)ucoef, c->kr_W);
    return down_hist(c, out, c->kr_W, rows);
}

// ------------------------------------------------------------------------------------
// Newton-CG on the free set: (preconditioned) conjugate gradients on P H P x = P b with x, r, p, the free set and the
// recurrence on the device (kernels: "Device-resident Newton-CG" in vch_kernels1d.h).  The storage, the
// step kernel and the look schedule are those of vch1d_hess_lanczos without reorthogonalisation.
// ------------------------------------------------------------------------------------
// the cells of the iteration in the block of the Lanczos scalars: resid, curv where alpha, beta live
static Ncg1Cells ncg1_cells(const vch1d_ctx *c, const Kr1Layout &L) {
    double *sc = c->kr_sc;
    const int B = c->B;
    return Ncg1Cells{sc + L.alpha, sc + L.beta, sc + L.look, sc + L.scal, sc + L.amax, sc + L.coef1, sc + L.coef1 + B,
                     sc + L.coef1 + 2 * B, (long long *)(sc + L.steps), (long long *)(sc + L.lim), (long long *)(sc + L.stop)};
}
static Ncg1Args ncg1_args(const vch1d_ctx *c, const Kr1Layout &L, int rows, long mask_s, int precond) {
    const long hs = hs1(c);
    return Ncg1Args{c->kr_Q, (long)c->B * hs, hs, (long)rows * c->n, c->n, c->kr_slots, c->kr_mask, mask_s,
                    c->kr_sc + L.wtp, c->so_wx, precond, ncg1_cells(c, L)};
}

// The body of vch1d_hess_cg, shared with the rounds of vch1d_pgd_newton.  fn: the entry point the messages name.
// empty_ok (the Newton rounds): a trajectory with an empty free set is no error.  The set-up returns for it before it
// writes x, r, p and its cells, so the host takes n_free = 0 from the look alone: zero steps, VCH_CG_CONVERGED,
// pred = rnorm0 = 0, none of the stale cells read, and its three slots zeroed for vch1d_cg_vector.
// radius (or NULL): the trust region of vch1d_hess_cg_tr, k1d_ncg_fin_tr in place of k1d_ncg_fin and xnorm_out [B] = ||x||_D
// by the recurrence (0 for an empty free set); NULL runs the launches of vch1d_hess_cg exactly.
// The right-hand side that vch1d_hess_cg builds itself (rhs == NULL) and the free set are those of the L1 functional: with
// the resident control (`resident`) of a problem that has a trajectory in a group mode they would belong to another cost.
static int gp_refuse(const vch1d_ctx *c, const char *fn, bool resident) {
    if (resident && c->pgd_ready && gp_group(c))
        return vch_fail(VCH_ERR_STATE, "%s: the resident problem has a trajectory in a directional-sparsity mode; the sign term and "
                        "the free set of this call are those of the L1 functional", fn);
    return 0;
}

static int hess_cg1_core(vch1d_ctx *c, const char *fn, bool empty_ok, const double *phi_hist, const double *u, int n_base, int rows,
                         const double *dt, const double *t_hist, const double *x, const double *phi_Q, const double *phi_T,
                         const vch_opt_params *opts, int n_opts, const uint8_t *mask, double tol, const double *rhs, int k,
                         double cg_tol, int precond, double *resid_out, double *curv_out, double *pred_out, double *rnorm0_out,
                         int32_t *steps_out, int32_t *status_out, int64_t *n_free_out, vch_stats *stats,
                         const double *radius = nullptr, double *xnorm_out = nullptr) {
    const int B = c->B, n = c->n;
    VCHCHK(gp_refuse(c, fn, !rhs && u == VCH_RESIDENT));
    VCHCHK(so1_check_shape(c, fn, n_base, rows, n_opts, 2));
    if (!resid_out || !curv_out || !pred_out || !rnorm0_out || !steps_out || !status_out || !n_free_out)
        return vch_fail(VCH_ERR_ARG, "%s: NULL resid_out, curv_out, pred_out, rnorm0_out, steps_out, status_out or n_free_out", fn);
    if (k < 1) return vch_fail(VCH_ERR_ARG, "%s: k = %d must be >= 1", fn, k);
    if (precond != 0 && precond != 1) return vch_fail(VCH_ERR_ARG, "%s: precond = %d is neither 0 nor 1", fn, precond);
    if (!std::isfinite(cg_tol)) return vch_fail(VCH_ERR_ARG, "%s: cg_tol must be finite", fn);
    if (radius)
        for (int b = 0; b < B; ++b)
            if (!(radius[b] > 0.0))
                return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: radius %g must be > 0 (+inf allowed, NaN not)", fn, b, radius[b]);
    const int M = rows - 2;
    const long hs = hs1(c);
    Kr1Call C;
    VCHCHK(kr1_open(c, fn, C, 3, k, true, precond, phi_hist, u, n_base, rows, dt, t_hist, x, phi_Q, phi_T, opts, n_opts, mask, rhs, NCG1_R));
    const Kr1Layout &L = C.L;
    double *sc = c->kr_sc, *part = sc + L.part;
    const Ncg1Args K = ncg1_args(c, L, rows, C.mask_s, precond);
    const Ncg1Cells &cells = K.x;
    const int S = c->kr_slots, nch = kr1_chunks(c, rows);
    const dim3 kgrid(nch, B);
    const double stop_at = cg_tol > 0 ? cg_tol : 1e-8;
    C.G.hd = c->kr_Q + (long)NCG1_P * B * hs;
    double *tr = sc + L.tr;
    const Ntr1Cells tcells{tr, tr + B, tr + 2 * B, tr + 3 * B, tr + 4 * B, (long long *)(tr + 5 * B)};
    if (radius) {
        VCHCHK(up(c, tr, radius, B));
        HIPCHK(hipMemsetAsync(tr + B, 0, sizeof(double) * 5 * B, c->stream));     // xx = xp = 0 (x_0 = 0), nothing pending
    }
    // the set-up: the free set, the gradient sweep once per base point (yp of every step stays in kr_X), r = P b, x, p
    double *keepX = c->kr_nocache ? nullptr : c->kr_X;
    if (rhs)
        LAUNCH_LDS(-1, (k1d_ncg_setup<0>), dim3(B), dim3(T1), c->lds_bytes, c->P, n, c->h, c->lvl, rows, C.G, K,
                   (const double *)(sc + L.box), (const double *)(sc + L.ks), tol > 0 ? tol : 1e-8, mask ? 0 : 1,
                   c->kr_nocache ? 0 : 1, keepX, c->scratch);
    else
        LAUNCH_LDS(-1, (k1d_ncg_setup<1>), dim3(B), dim3(T1), c->lds_bytes, c->P, n, c->h, c->lvl, rows, C.G, K,
                   (const double *)(sc + L.box), (const double *)(sc + L.ks), tol > 0 ? tol : 1e-8, mask ? 0 : 1, 1, keepX,
                   c->scratch);
    std::vector<double> look(2 * (size_t)B);
    VCHCHK(down(c, look.data(), cells.look, look.size()));          // the first look; the host vectors above are done with
    for (int b = 0; b < B; ++b) {
        if (look[2 * b] < 1.0 && !empty_ok) return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: the free set is empty", fn, b);
        if (!std::isfinite(look[2 * b + 1]))
            return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: the right-hand side is not finite on the free set", fn, b);
    }
    // an empty free set (empty_ok): the set-up wrote nothing of x, r, p; its stop cell keeps the kernels below off them
    for (int b = 0; b < B; ++b)
        if (look[2 * b] < 1.0)
            for (int slot = 0; slot < 3; ++slot)
                HIPCHK(hipMemsetAsync(c->kr_Q + (long)slot * B * hs + b * hs, 0, sizeof(double) * rows * n, c->stream));
    // k steps back to back: a stopped trajectory's kernels return at once, the host does not look
    for (int j = 0; j < k; ++j) {
        VCHCHK(kr1_step(c, rows, C.G, cells.stop));
        // w = H p in kr_W
        LAUNCH(k1d_ncg_curv, kgrid, dim3(KR1_T), K, (const double *)c->kr_W, part);
        if (radius) LAUNCH(k1d_ncg_fin_tr, dim3(B), dim3(KR1_T), cells, tcells, (const double *)part, nch, S, 2, j, k, stop_at);
        else LAUNCH(k1d_ncg_fin, dim3(B), dim3(KR1_T), cells, (const double *)part, nch, S, 2, j, k, stop_at);
        LAUNCH(k1d_ncg_update, kgrid, dim3(KR1_T), K, (const double *)c->kr_W, part);
        if (radius) LAUNCH(k1d_ncg_fin_tr, dim3(B), dim3(KR1_T), cells, tcells, (const double *)part, nch, S, 3, j, k, stop_at);
        else LAUNCH(k1d_ncg_fin, dim3(B), dim3(KR1_T), cells, (const double *)part, nch, S, 3, j, k, stop_at);
        if (j + 1 < k) LAUNCH(k1d_ncg_dir, kgrid, dim3(KR1_T), K);
    }
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    std::vector<long long> steps(B), prods(B), stop(B);
    std::vector<double> xx(radius ? B : 0);
    if (radius) HIPCHK(hipMemcpyAsync(xx.data(), tcells.xx, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(resid_out, cells.resid, sizeof(double) * B * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(curv_out, cells.curv, sizeof(double) * B * k, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pred_out, cells.pred, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(rnorm0_out, cells.rnorm0, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(steps.data(), cells.steps, sizeof(long long) * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(prods.data(), cells.prods, sizeof(long long) * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(stop.data(), cells.stop, sizeof(long long) * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                        // the second look
    int64_t solves = 0;
    for (int b = 0; b < B; ++b) {
        if (look[2 * b] < 1.0) {                    // empty_ok: the cells of this trajectory are stale, and there was no sweep
            steps_out[b] = 0;
            status_out[b] = VCH_CG_CONVERGED;
            n_free_out[b] = 0;
            pred_out[b] = rnorm0_out[b] = 0.0;
            if (radius) xnorm_out[b] = 0.0;
            continue;
        }
        if (radius) xnorm_out[b] = std::sqrt(xx[b]);
        steps_out[b] = (int32_t)steps[b];
        status_out[b] = (int32_t)stop[b];           // 0: still running after k steps, VCH_CG_LIMIT
        n_free_out[b] = (int64_t)look[2 * b];
        // the set-up's sweep: always with the cache; with the switch only where the right-hand side is built from it
        solves += c->kr_nocache ? 3 * (int64_t)M * prods[b] + (rhs ? 0 : M) : (int64_t)M * (2 * prods[b] + 1);
    }
    so1_stats(c, stats, solves, 6 * (int64_t)k, 2);       // the set-up, five per step, the direction between two steps
    c->ncg_valid = true;
    c->ncg_rows = rows;
    c->ncg_u = C.Sb.u;
    c->ncg_us = C.Sb.bs;
    c->ncg_mask_s = K.mask_s;
    c->ncg_u_live = true;
    return 0;
}

extern "C" int vch1d_hess_cg(vch1d_ctx *c, const double *phi_hist, const double *u, int n_base, int rows, const double *dt,
                             const double *t_hist, const double *x, const double *phi_Q, const double *phi_T,
                             const vch_opt_params *opts, int n_opts, const uint8_t *mask, double tol, const double *rhs, int k,
                             double cg_tol, int precond, double *resid_out, double *curv_out, double *pred_out, double *rnorm0_out,
                             int32_t *steps_out, int32_t *status_out, int64_t *n_free_out, vch_stats *stats) {
    CTXCHK(c);
    return hess_cg1_core(c, "vch1d_hess_cg", false, phi_hist, u, n_base, rows, dt, t_hist, x, phi_Q, phi_T, opts, n_opts, mask, tol, rhs,
                         k, cg_tol, precond, resid_out, curv_out, pred_out, rnorm0_out, steps_out, status_out, n_free_out, stats);
}

extern "C" int vch1d_hess_cg_tr(vch1d_ctx *c, const double *phi_hist, const double *u, int n_base, int rows, const double *dt,
                                const double *t_hist, const double *x, const double *phi_Q, const double *phi_T,
                                const vch_opt_params *opts, int n_opts, const uint8_t *mask, double tol, const double *rhs, int k,
                                double cg_tol, int precond, double *resid_out, double *curv_out, double *pred_out,
                                double *rnorm0_out, int32_t *steps_out, int32_t *status_out, int64_t *n_free_out, vch_stats *stats,
                                const double *radius, double *xnorm_out) {
    CTXCHK(c);
    const char *fn = "vch1d_hess_cg_tr";
    if (!radius || !xnorm_out) return vch_fail(VCH_ERR_ARG, "%s: NULL radius or xnorm_out", fn);
    return hess_cg1_core(c, fn, false, phi_hist, u, n_base, rows, dt, t_hist, x, phi_Q, phi_T, opts, n_opts, mask, tol, rhs, k, cg_tol,
                         precond, resid_out, curv_out, pred_out, rnorm0_out, steps_out, status_out, n_free_out, stats, radius,
                         xnorm_out);
}

extern "C" int vch1d_cg_vector(vch1d_ctx *c, int which, double *out) {
    CTXCHK(c);
    ARGCHK(out, "NULL out");
    ARGCHK(which >= 0 && which <= 2, "which must be 0 (x), 1 (r) or 2 (p)");
    if (!c->ncg_valid || !c->kr_Q)
        return vch_fail(VCH_ERR_STATE, "vch1d_cg_vector: no resident vectors (call vch1d_hess_cg first)");
    return down_hist(c, out, c->kr_Q + (long)which * c->B * hs1(c), c->ncg_rows);
}

// ------------------------------------------------------------------------------------
// Damped Newton rounds on the free set about the resident PGD iterate (kernels: "Damped Newton rounds" in vch_kernels1d.h,
// verdicts: vch_newton.h)
// ------------------------------------------------------------------------------------
// The trial control of the step lengths s_host [B] into the trial-control scratch, about the base control, the x, the free
// set and the box table the last Newton-CG solve left; skip (device flags, or NULL) leaves a trajectory alone.  The step
// table, the partials and the sums have cells of their own in the block of the Krylov scalars; sums_out [B][4] =
// {sum (t - u)^2, sum u^2, pinned, clipped} after one look (the cells of a skipped trajectory are not written).
static int newton_trial1_core(vch1d_ctx *c, const double *s_host, const int *skip, double *sums_out) {
    const int B = c->B, rows = c->ncg_rows, nch = kr1_chunks(c, rows);
    const Kr1Layout L = kr1_layout(c, c->kr_slots, c->kr_kcap);
    double *sc = c->kr_sc;
    const Ncg1Args K = ncg1_args(c, L, rows, c->ncg_mask_s, 0);
    VCHCHK(up(c, sc + L.nts, s_host, B));
    LAUNCH(k1d_nt_trial, dim3(nch, B), dim3(KR1_T), K, c->ncg_u, c->ncg_us, (const double *)(sc + L.nts), (const double *)(sc + L.box),
           skip, c->u_trial, sc + L.ntpart);
    LAUNCH(k1d_nt_fin, dim3(B), dim3(KR1_T), (const double *)(sc + L.ntpart), nch, skip, sc + L.ntsum);
    return down(c, sums_out, sc + L.ntsum, 4 * (size_t)B);         // synchronises: s_host is done with
}

extern "C" int vch1d_newton_trial(vch1d_ctx *c, const double *s, double *u_out, double *chg_out, int64_t *counts_out) {
    CTXCHK(c);
    ARGCHK(s && chg_out && counts_out, "NULL s, chg_out or counts_out");
    for (int b = 0; b < c->B; ++b) ARGCHK(std::isfinite(s[b]) && s[b] > 0, "s must be finite and > 0");
    if (!c->ncg_valid || !c->kr_Q)
        return vch_fail(VCH_ERR_STATE, "vch1d_newton_trial: no resident vectors (call vch1d_hess_cg first)");
    if (c->ncg_u && c->ncg_u == c->so_u && !c->ncg_u_live)
        return vch_fail(VCH_ERR_STATE, "vch1d_newton_trial: the base control of the last vch1d_hess_cg has been replaced by a later call");
    VCHCHK(ensure1(c, &c->u_trial));
    std::vector<double> sums(4 * (size_t)c->B);
    VCHCHK(newton_trial1_core(c, s, nullptr, sums.data()));
    for (int b = 0; b < c->B; ++b) {
        chg_out[2 * b] = sums[4 * b];
        chg_out[2 * b + 1] = sums[4 * b + 1];
        counts_out[2 * b] = (int64_t)sums[4 * b + 2];
        counts_out[2 * b + 1] = (int64_t)sums[4 * b + 3];
    }
    return u_out ? down_hist(c, u_out, c->u_trial, c->ncg_rows) : 0;
}

// The engine's side of the Newton and trust-region rounds (vch_newton.h) about the resident PGD iterate; sec = {solves, trial
// controls, marches, costs}.
struct Pgd1Rounds {
    vch1d_ctx *c;
    const char *fn;
    int rows, k, precond;
    double cg_tol, tol;
    std::vector<double> resid, curv, Jt;
    std::vector<int> bad;
    double sec[4];
    double lap() {
        float ms = 0;
        hipEventSynchronize(c->ev1);
        hipEventElapsedTime(&ms, c->ev0, c->ev1);
        return (double)ms * 1e-3;
    }
    // The stop quirk: a trajectory the PGD stop rule ended holds the new control beside the previous iterate's state and
    // cost (G1:462-465).  One march of the resident control, the others sitting it out, brings both up to the control.
    int stop_quirk() {
        const int B = c->B;
        std::vector<int> sit(B);
        bool stale = false;
        for (int b = 0; b < B; ++b) {
            sit[b] = !(c->pgd.done[b] && !c->pgd_synced[b]);
            stale = stale || !sit[b];
        }
        if (!stale) return 0;
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        HIPCHK(hipMemcpyAsync(c->skip_dev, sit.data(), sizeof(int) * B, hipMemcpyHostToDevice, c->stream));
        VCHCHK(fwd1_core(c, c->u_hist, rows, c->phi_trial, c->skip_dev));
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        sec[2] += lap();
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        VCHCHK(cost1_core(c, c->phi_trial, c->u_hist, rows, Jt.data()));
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        sec[3] += lap();
        for (int b = 0; b < B; ++b) {
            if (sit[b]) continue;
            VCHCHK(copy_traj1(c, c->phi_hist, c->phi_trial, b, rows));
            c->pgd.cost[b] = Jt[5 * b + 4];
            c->pgd_synced[b] = 1;
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        return 0;
    }
    int solve(double *pred, double *rnorm0, int32_t *steps, int32_t *status, int64_t *n_free) {
        vch_stats st;
        VCHCHK(hess_cg1_core(c, fn, true, nullptr, VCH_RESIDENT, c->B, rows, c->dt_host.data(), c->t_host.data(), c->x_host.data(),
                             VCH_RESIDENT, VCH_RESIDENT, c->opts.data(), c->B, nullptr, tol, nullptr, k, cg_tol, precond, resid.data(),
                             curv.data(), pred, rnorm0, steps, status, n_free, &st));
        sec[0] += st.seconds;
        return 0;
    }
    // the trust-region rounds: the Steihaug solve inside radius [B]
    int solve(const double *radius, double *pred, double *rnorm0, int32_t *steps, int32_t *status, int64_t *n_free, double *xnorm) {
        vch_stats st;
        VCHCHK(hess_cg1_core(c, fn, true, nullptr, VCH_RESIDENT, c->B, rows, c->dt_host.data(), c->t_host.data(), c->x_host.data(),
                             VCH_RESIDENT, VCH_RESIDENT, c->opts.data(), c->B, nullptr, tol, nullptr, k, cg_tol, precond, resid.data(),
                             curv.data(), pred, rnorm0, steps, status, n_free, &st, radius, xnorm));
        sec[0] += st.seconds;
        return 0;
    }
    // the trust-region rounds' one trial at s = 1
    int trial(const std::vector<int> &decided, double *sums, double *c_new) {
        return trial(decided, std::vector<double>(c->B, 1.0), sums, c_new);
    }
    double cost(int b) const { return c->pgd.cost[b]; }
    int trial(const std::vector<int> &decided, const std::vector<double> &s, double *sums, double *c_new) {
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        HIPCHK(hipMemcpyAsync(c->skip_dev, decided.data(), sizeof(int) * c->B, hipMemcpyHostToDevice, c->stream));
        VCHCHK(newton_trial1_core(c, s.data(), c->skip_dev, sums));
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        sec[1] += lap();
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        VCHCHK(fwd1_core(c, c->u_trial, rows, c->phi_trial, c->skip_dev, bad.data()));
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        sec[2] += lap();
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        VCHCHK(cost1_core(c, c->phi_trial, c->u_trial, rows, Jt.data()));
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        sec[3] += lap();
        // a march that reported a non-finite mass defect: the trial counts as not accepted
        for (int b = 0; b < c->B; ++b) c_new[b] = bad[b] ? std::nan("") : Jt[5 * b + 4];
        return 0;
    }
    int accept(int b, double c_new) {
        c->pgd.cost[b] = c_new;
        VCHCHK(copy_traj1(c, c->u_hist, c->u_trial, b, rows));
        return copy_traj1(c, c->phi_hist, c->phi_trial, b, rows);
    }
    int after_trial() {
        HIPCHK(hipStreamSynchronize(c->stream));
        return 0;
    }
    int after_round() { return 0; }
};

extern "C" int vch1d_pgd_newton(vch1d_ctx *c, int n_rounds, int k, double cg_tol, int precond, double tol, int max_halvings,
                                double *cost_out, double *cost_new_out, double *s_out, double *pred_out, double *rnorm0_out,
                                int32_t *halvings_out, int32_t *cg_steps_out, int32_t *cg_status_out, int32_t *status_out,
                                int64_t *counts_out, double *seconds_out) {
    CTXCHK(c);
    const char *fn = "vch1d_pgd_newton";
    // everything below is checked before anything is enqueued, copied or allocated
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "%s: call vch1d_pgd_init first", fn);
    VCHCHK(gp_refuse(c, fn, true));
    const int B = c->B, rows = c->pgd_rows;
    const vch_newton_call call{B, n_rounds, k, cg_tol, precond, max_halvings, cost_out, cost_new_out, s_out, pred_out, rnorm0_out,
                               halvings_out, cg_steps_out, cg_status_out, status_out, counts_out};
    if (const char *bad = vch_newton_check(call)) return vch_fail(VCH_ERR_ARG, "%s: %s", fn, bad);
    {   // what the solve of a round checks, here as well: the stop quirk below marches before the first solve
        std::vector<double> dts, wts, wt, wtp;
        VCHCHK(so1_check_shape(c, fn, B, rows, B, 2));
        VCHCHK(so1_check_rest(c, fn, nullptr, VCH_RESIDENT, rows, c->dt_host.data(), c->t_host.data(), c->x_host.data(), VCH_RESIDENT,
                              VCH_RESIDENT, c->opts.data(), B, dts, wts));
        VCHCHK(ncg1_weights(fn, c->t_host.data(), rows, precond, wt, wtp));
    }
    // the engine's side of the rounds (vch_newton.h)
    Pgd1Rounds eng{c, fn, rows, k, precond, cg_tol, tol, std::vector<double>((size_t)B * k), std::vector<double>((size_t)B * k),
                   std::vector<double>(5 * (size_t)B), std::vector<int>(B), {0, 0, 0, 0}};
    VCHCHK(eng.stop_quirk());
    bool moved = false;
    const int rc = vch_newton_rounds(eng, call, moved);
    if (moved) c->pgd_r_valid = false;      // r_hist is the adjoint of an iterate that has been replaced
    if (rc >= 0 && seconds_out) memcpy(seconds_out, eng.sec, sizeof(eng.sec));
    return rc;
}

// ------------------------------------------------------------------------------------
// Trust-region (Steihaug) Newton-CG rounds on the free set about the resident PGD iterate (kernels: k1d_ncg_fin_tr in
// vch_kernels1d.h, verdicts: vch_trust_state in vch_newton.h)
// ------------------------------------------------------------------------------------
extern "C" int vch1d_pgd_trust(vch1d_ctx *c, int n_rounds, int k, double cg_tol, int precond, double tol, const double *radius0,
                               double radius_max, double radius_min, double *cost_out, double *cost_new_out, double *pred_out,
                               double *rnorm0_out, double *radius_out, double *ratio_out, double *xnorm_out, int32_t *cg_steps_out,
                               int32_t *cg_status_out, int32_t *status_out, int64_t *counts_out, double *seconds_out) {
    CTXCHK(c);
    const char *fn = "vch1d_pgd_trust";
    // everything below is checked before anything is enqueued, copied or allocated
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "%s: call vch1d_pgd_init first", fn);
    VCHCHK(gp_refuse(c, fn, true));
    const int B = c->B, rows = c->pgd_rows;
    const vch_trust_call call{B, n_rounds, k, cg_tol, precond, radius0, radius_max, radius_min, cost_out, cost_new_out, pred_out,
                              rnorm0_out, radius_out, ratio_out, xnorm_out, cg_steps_out, cg_status_out, status_out, counts_out};
    if (const char *bad = vch_trust_check(call)) return vch_fail(VCH_ERR_ARG, "%s: %s", fn, bad);
    {   // what the solve of a round checks, here as well: the stop quirk below marches before the first solve
        std::vector<double> dts, wts, wt, wtp;
        VCHCHK(so1_check_shape(c, fn, B, rows, B, 2));
        VCHCHK(so1_check_rest(c, fn, nullptr, VCH_RESIDENT, rows, c->dt_host.data(), c->t_host.data(), c->x_host.data(), VCH_RESIDENT,
                              VCH_RESIDENT, c->opts.data(), B, dts, wts));
        VCHCHK(ncg1_weights(fn, c->t_host.data(), rows, precond, wt, wtp));
    }
    Pgd1Rounds eng{c, fn, rows, k, precond, cg_tol, tol, std::vector<double>((size_t)B * k), std::vector<double>((size_t)B * k),
                   std::vector<double>(5 * (size_t)B), std::vector<int>(B), {0, 0, 0, 0}};
    VCHCHK(eng.stop_quirk());
    bool moved = false;
    const int rc = vch_trust_rounds(eng, call, moved);
    if (moved) c->pgd_r_valid = false;      // r_hist is the adjoint of an iterate that has been replaced
    if (rc >= 0 && seconds_out) memcpy(seconds_out, eng.sec, sizeof(eng.sec));
    return rc;
}
