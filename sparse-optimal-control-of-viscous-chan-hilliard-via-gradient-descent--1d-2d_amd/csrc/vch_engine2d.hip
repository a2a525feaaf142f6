// vch_engine2d.hip — host side of the 2D engine: context, launch sequencing, C ABI (include/vch.h).
//
// One context = one GPU, one HIP stream, B independent trajectories.  All per-trajectory
// decisions are taken on the device (TrajState + `fin` kernels); the host only decides how many
// more launches to enqueue, reading the B state records back once per Newton iteration.
#include "vch_common.h"
#include "vch_kernels2d.h"
#include "vch_gemm.h"
#include "vch_fft.h"
#include "vch_pgd.h"
#include "vch_newton.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>

thread_local char g_vch_err[512] = "";

// the runtime behind every context's pool (vch_mem.h): the only callers of these four
const vch_mem_fns *vch_hip_mem() {
    static const vch_mem_fns hip = {[](void **p, size_t bytes) { return (int)hipMalloc(p, bytes); },
                                    [](void *p) { return (int)hipFree(p); },
                                    [](void **p, size_t bytes, unsigned flags) { return (int)hipHostMalloc(p, bytes, flags); },
                                    [](void *p) { return (int)hipHostFree(p); }};
    return &hip;
}

extern "C" const char *vch_last_error(void) { return g_vch_err; }
extern "C" int vch_abi_version(void) { return 3; }
extern "C" int vch_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

constexpr int J_RING = 64;        // iterations whose cost scalars stay readable on the device

// How many previous increments the starting guess of a step's first Newton solve extrapolates over (forward_core).
// The best order depends on the march: without a control the increments are smooth enough for order 6 (the deflated
// right-hand side falls to 1e-9 of the full one), under a PGD control order 3-4 is the optimum, and in the spinodal
// transient of the first steps no extrapolation pays.  So the order is found by trial: it climbs one step at a time while
// each step more than halves the ratio ||rhs - A x0|| / ||rhs|| the guess leaves; afterwards every PROBE_EVERY-th step
// tries the neighbouring order (alternately one up, one down) and the order moves if the neighbour is better (down on
// ties: fewer planes to read).  A guess that leaves more than 0.7 of the right-hand side sends the order down at once.
struct GuessPolicy {
    static constexpr int PROBE_EVERY = 8;
    int order, probe, since, next_dir;
    bool climbing;
    double r_base;
    void reset() { order = 1; probe = 0; since = 0; next_dir = 1; climbing = true; r_base = 1e300; }
    // order to use for the coming step; avail = increments kept so far, cap = largest order allowed
    int choose(int avail, int cap) const { return std::max(0, std::min(std::min(order + probe, cap), avail)); }
    // ratio left by the guess of the step just finished (worst trajectory), used = the order it was made with
    void report(double r, int used, int cap) {
        if (used < 1) return;
        if (climbing) {
            if (r > 0.7) {                                 // transient of the first steps: wait at order 1
                order = std::max(1, used - 1);
                r_base = 1e300;
                if (used > 1) climbing = false;
                return;
            }
            if (r_base < 1e299 && r > 0.5 * r_base) {      // the last step up did not pay: back, and hold
                order = std::max(1, used - 1);
                climbing = false;
                return;
            }
            r_base = r;
            order = used;
            if (used >= cap) climbing = false;
            else order = used + 1;
            return;
        }
        if (probe == 0) {
            r_base = r;
            if (r > 0.7 && order > 1) { --order; since = 0; return; }
            if (++since >= PROBE_EVERY) {
                since = 0;
                probe = next_dir;
                next_dir = -next_dir;
                if (order + probe < 1 || order + probe > cap) probe = 0;
            }
            return;
        }
        if (probe > 0 ? r < 0.5 * r_base : r <= r_base) order = used;
        probe = 0;
    }
};

// Made by `new vch2d_ctx()` alone: a member without an initialiser starts as zero (false, NULL), and vch2d_create assigns only
// what depends on its arguments or on the environment.
struct vch2d_ctx {
    vch_pool pool{vch_hip_mem()};          // owns every device and pinned buffer below (vch_mem.h); teardown() releases it
    vch2d_params prm;
    int B, Mmax, device;
    Geom G;
    Phys P;
    double hx, hy;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    dim3 grid;
    int nblk;
    long slot_stride;
    // Newton iterate, two slots each: [2][B][plane]
    double *phi_s, *mu_s, *Rphi_s, *rhs_s, *D_s;
    // work planes [B][plane]
    double *w, *wnew, *mu0, *cphi, *cmu, *x, *r, *dmu, *t1, *t2;
    double *cg_p[2], *cg_v, *cg_q;        // CG search directions / operator images
    double *cg_z2;                        // second residual buffer of the forward CG (z ping-pongs r <-> cg_z2)
    double *xf;                           // finished dphi of a Newton solve (written by the back-substitution kernel)
    int cg_last;                          // index of the last sweep schur_solve enqueued (-1: none), for dmu_ceiling()
    // reduction-free (Chebyshev) form of the forward solves of a march (cheb_solve): allowed at all (VCH_CHEB=0 turns it
    // off), chosen for the step being enqueued, sweeps enqueued by the last cheb_solve (-1: the last solve was a CG solve),
    // sweeps per Newton slot of the schedule, and the margin added to what the previous step's plans asked for
    bool cheb_on;
    int spec_form[4] = {3, 3, 3, 3};      // per Newton slot: bit 0 = enqueue the reduction-free sequence, bit 1 = the CG sequence
    bool debug_guess;                     // VCH_DEBUG_GUESS, read once at creation
    bool adj_guess_off, adj_safe;         // VCH_ADJ_GUESS_OFF, VCH_ADJ_SAFE (diagnostics), read at the start of every sweep
    long redo_iters;                      // sweeps of an adjoint pass that had to be repeated (0 otherwise)
    // fused evaluation kernels (k_eval: step start and Armijo trial with the starting guess and the `fin` step folded in;
    // VCH_FUSED=0 restores the separate kernels, results bit-identical) and the per-trajectory arrival counters of their
    // last-workgroup-done hand-off
    bool fused_on;
    int fused_mode;                       // 0 separate kernels, 1 fused with the fin step inside, 2 fused + fin launches
    unsigned *fin_counter;
    int cheb_enq = -1, spec_chn[4] = {2, 2, 2, 2}, cheb_margin, cheb_max;
    double pgd_adj_tol;                   // relative residual at which the adjoint solves of the PGD loop stop (VCH_ADJ_TOL)
    double eta1_factor;                   // first solve of a step: target = max(lin_eta, eta1_factor x recent ||R_1||) (VCH_ETA1; 0 = off)
    double cg_scale_ratio;                // CG form: Dmax / Dmin beyond which a solve runs right-scaled (0 = never; VCH_CG_SCALE)
    // starting guess of a step's first Newton solve (k_guess): the first increments of the last GUESS_RING steps (ring,
    // written by k_dmu_ceiling_fin; the adjoint sweep keeps its levels there instead), the guess itself (also that of the
    // second solve), its coefficients for the step being enqueued (all 0 = no guess) and the ring slot this step's
    // increment goes to
    double *dprev[GUESS_RING], *x0g;
    bool guess_on;
    int guess_wr = -1, guess_step;        // ring slot of this step's increment (-1: not kept); step index within the march
    int guess_max;                        // largest order allowed
    // per trajectory (a trajectory's orders follow from its own history, whatever its batch mates do): order policies of the
    // first / second solve, orders used in the step being enqueued, length of the run of steps with a second solve
    std::vector<GuessPolicy> pol1, pol2;
    std::vector<int> used1, used2, run2;
    GuessPolicy pol1_all, pol2_all;       // batches beyond GUESS_BMAX trajectories: one policy fed with the worst trajectory
    int run2_all;
    GuessArgs gtab1, gtab2;               // coefficient tables of the step being enqueued (all 0 = no guess)
    unsigned gmask1, gmask2;              // bit b: trajectory b has a guess for its first / second solve this step
    // the same for the step's SECOND Newton solve (its own ring)
    double *dprev2[GUESS_RING];
    bool guess2_on;
    double *gpart2;                       // second half of gpart
    double *gpart3;                       // [2][B][gnblk + ns] partials of <z',z'>_Z of the stencil-free sweep
    double *gpart;                        // [B][gnblk] partials written by the GEMM epilogue
    int gnblk;
    double *tmp[6];
    double *wts_mass, *W_cost;            // single planes
    double *part;                         // [B][nblk][NPART]
    double *part_mass;                    // [B][nblk][NPART]: k_mass's partials (read by the NEXT kernel: k_post or k_eval<0>)
    bool post_fold;                       // VCH_POST_FOLD (default 1): the end of a step is applied by the next step's k_eval<0>
    bool post_pending;                    // a step's clip / mass fix / history store waits for the next k_eval<0>
    double *post_hist;                    // ... its history level (or NULL)
    double *post_rec;                     // ... and its cell of the shift record (or NULL)
    // what the mass fix subtracted at the end of every step of a march, beside the history the march wrote:
    // [B][Mmax][SHIFT_REC] = {shift, the weight it was divided by: W_int where it went to the interior nodes only, 0.0 for the
    // all-node form, 1.0 where no fix ran}; shift_hist belongs to phi_hist, shift_trial to phi_trial (a line-search trial's
    // record moves with its history, copy_traj_shifts)
    double *shift_hist, *shift_trial;
    int *fix_bad = nullptr;               // [B] refusal cells of vch2d_second_order / vch2d_hessvec (FixCheck); lazy, so that
                                          // the buffers every context has stay where they were
    bool shift_res = false;               // shift_hist is the record of the resident state history
    TrajState *st, *st_host;
    // look at the device state without a copy command and a stream wait: a one-workgroup kernel writes the records into
    // mapped host memory (st_pub) and then a sequence number (seq_pub) the host spins on (sync_state)
    TrajState *st_pub;
    unsigned long long *seq_pub, seq_next;          // one sequence slot per trajectory
    bool look_spin;
    // The forward step's chain on the default path (fused evaluation kernels with the fin step as its own launch, looks through
    // mapped memory); each switch defaults to on and =0 restores the launches it replaces:
    //   VCH_MASS_EARLY   the step's k_mass is enqueued in front of the look (newton_level), not behind it
    //   VCH_FIN_PUBLISH  the k_fin_residual<1> in front of a look publishes the state itself (no k_publish_state launch)
    //   VCH_CEIL_CELL    the ceiling of a reduction-free solve goes through one cell per trajectory (no k_fin_ceiling launch)
    bool mass_early, fin_publish, ceil_cell_on;
    // VCH_EVAL_HOIST (default 1; 0 = A/B and tests): k_eval with the step start's operands and the guess tail's planes requested
    // ahead of the barriers that use them (vch_kernels2d.h); 0 launches k_eval_plain, the same arithmetic without that
    bool eval_hoist;
    // VCH_ROWS_BATCH (default 1; 0 = A/B and tests): k_dct_cols and k_cheb_rows with a phase's global operands requested
    // together (vch_fft.h: column data, multiplier entries, the operands of the Chebyshev update); 0 launches
    // k_dct_cols_plain and k_cheb_rows_plain, the same arithmetic one node at a time
    bool rows_batch;
    // VCH_LOADS_BATCH (default 1; 0 = A/B and tests): k_adj_guess, k_adj_finish and k_fin_residual with their global
    // operands requested together (vch_kernels2d.h); 0 launches their _plain forms, the same arithmetic with one wait per load
    bool loads_batch;
    unsigned long long *ceil_cell;        // [B][CeilCell::STRIDE] (vch_kernels2d.h)
    bool cell_now;                        // the level being enqueued uses the cells
    int trial_enq = -1;                   // sweeps of the reduction-free solve the NEXT trial launch arms the trial for (-1: none)
    unsigned long long pub_pending;       // sequence number a fin launch already enqueued will publish (0: none)
    bool mass_done;                       // newton_level has enqueued the step's k_mass
    int *frozen_dev;                      // [B] line-search flags for k_set_frozen
    double *hist_dev, *hist_host;         // [B][HIST_CAP]
    // DCT-I matrices and eigenvalues
    double *Q1f, *Q2f, *Q1s, *Q2s, *mf, *ms;
    bool use_fft;                         // both axes power-of-two: in-LDS FFT instead of the GEMMs
    int cols_c;                           // complex image per workgroup of the column pass at 1024-point length (columns = 2 C / 1024)
    FftAxis fax, sax;
    FftAxis fax_h, sax_h;                 // half-length plans (FFT length N) of the half-size DCT-I, N = 512 only
    double2 *tw_fh = nullptr, *tw_sh = nullptr;
    bool half_f = false, half_s = false;
    double2 *tw_f, *tw_s;
    // resident histories [B][Mmax+1][plane] (lazy)
    double *phi_hist, *u_hist, *u_trial, *phi_trial, *phiQ, *r_hist, *p_hist, *q_hist;
    double *phiT, *phi0;                  // [B][plane]
    double *cost_part, *cost_lvl;         // cost partials
    double *cost_lvl_host;
    double *alpha_dev;
    int M_res = -1;                       // steps of the resident state history (-1 none)
    int u_rows_res;                       // rows of the resident control (0 none)
    // resident PGD problem
    bool pgd_ready;
    bool ramp;
    double rampT;
    std::vector<double> t_hist, dt, xg, yg, tfrac;
    double *tfrac_dev;
    // optimisation parameters, one set per trajectory (vch2d_pgd_init_v; vch2d_pgd_init repeats one set): the host copy,
    // its device table [B][OPT_STRIDE] read by k_adj_rhs / k_scaled_diff / k_grad_prox / k_kkt_count, and a second table
    // (with its host staging) that the stateless seams vch2d_backward / vch2d_grad_prox fill with their scalar arguments,
    // so that they leave the resident problem's table alone
    std::vector<vch_opt_params> opts;
    double *opt_tab, *seam_tab;
    std::vector<double> tab_host;
    bool pgd_r_valid;                     // r_hist holds an adjoint of the resident problem (a sweep has run since the init)
    unsigned long long *kkt_dev;          // vch2d_pgd_kkt: [B][3] counts, then [B][Mmax+1][3] per-level partials
    // directional sparsity: the mode of every trajectory (empty = all VCH_SPARSITY_FULL) with its device
    // copy; and, allocated as one group only when a trajectory is in a group mode (or a group seam is called): the time
    // weights [Mmax+1], s per group [B][gp2_ss], the tile partials of the TIME prox [B][Mmax+1][nblk][4], the change
    // partials [B][gp2_nsb][2] and the cost partials [B][gp2_nsb] of the pencil kernels with their host copies, alpha = 1
    std::vector<int> modes;
    int *mode_dev = nullptr;
    double *gp_wt = nullptr, *gp_s = nullptr, *gp_tpart = nullptr, *gp_chg = nullptr, *gp_j4 = nullptr, *gp_one = nullptr;
    std::vector<double> gp_chg_host, gp_j4_host;
    // vch2d_second_order (lazy): workgroup partials [B][Mmax+1][nblk][TAN_NSUM], level sums [B][Mmax+1][TAN_NSUM], the time
    // levels [Mmax+1] and the six scalars [B][6] on the device; rows of the control the resident state history was marched
    // under (0: none)
    double *tan_part = nullptr, *tan_lvl = nullptr, *tan_t = nullptr, *tan_out = nullptr;
    int fwd_u_rows = 0;
    // vch2d_hessvec (lazy): histories of G, H h, the raw tangent solves v_k and the tangent after the mean removal; one
    // block {partials [2][B][nblk][NPART], time weights [Mmax+1], dots [B][2]}
    double *hv_G = nullptr, *hv_H = nullptr, *hv_V = nullptr, *hv_DP = nullptr, *hv_part = nullptr, *hv_wt = nullptr,
           *hv_dots = nullptr;
    // vch2d_hess_lanczos (lazy, one group): the basis [kr_slots][B][Mmax+1][plane], the gradient sweep's xp of every step
    // [Mmax][B][plane] (level-major: k_hv_rhs<1> reads one step's planes with the trajectory stride of a work plane), the
    // free set as bytes [B][Mmax+1][plane] and one block of partials and scalars (KrLayout); what the last run left
    // for vch2d_krylov_vector
    double *kr_Q = nullptr, *kr_X = nullptr, *kr_sc = nullptr;
    unsigned char *kr_mask = nullptr;
    int kr_slots = 0, kr_kcap = 0;        // capacity: basis slots, entries of alpha / beta per trajectory
    int kr_lchunk;                        // VCH_KR_LCHUNK: levels per workgroup of the Krylov kernels
    bool kr_nocache;                      // VCH_KRYLOV_NOCACHE=1 (A/B and tests): every step repeats the gradient sweep
    bool kr_valid = false;                // a basis is resident
    int kr_levels, kr_run_slots, kr_window, kr_min_steps;   // its rows, ring size, addressable vectors, smallest step count
    // vch2d_hess_cg keeps x, r, p in slots 0, 1, 2 of kr_Q (either call invalidates what the other left resident)
    bool ncg_valid = false;
    int ncg_levels;
    bool res_pgd = false;                 // the resident state history is the resident PGD problem's iterate
    vch_pgd_state pgd;                    // the line search's books and the error metrics of the driver loop (vch_pgd.h)
    std::vector<double> J_host;           // [B][5] cost terms of the accepted iterate, the source of J_dev and the ring
    double *J_dev;
    // cost scalars of the last J_RING iterations, [J_RING][B][5] on the device (slot = iteration index mod J_RING), so
    // that the collective of iteration k (vch_comm_allreduce_cost) reads iteration k's values even when the context
    // has already gone on; J_ring_host is the pinned staging copy
    double *J_ring_dev, *J_ring_host;
    std::atomic<long> pgd_iter_total{0};  // iterations performed since vch2d_pgd_init (read by the collective's thread)
    long tot_launch, tot_sync;            // launches / looks accumulated over the context's life (vch2d_counters)
    // per-kernel-class HIP-event timing (bench.py roofline leg)
    bool prof_on;
    std::vector<hipEvent_t> prof_ev;
    std::vector<int> prof_cls;
    size_t prof_used;
    // knobs (read_knobs)
    bool knob_gemm_dct, knob_dct_half, knob_guess;   // VCH_FORCE_GEMM_DCT, VCH_DCT_HALF, VCH_GUESS as make_plan takes them
    int lin_maxit = 4000;
    double lin_tol;
    double lin_eta;                       // target for the Schur residual a Newton solve inside a march leaves (0 = lin_tol)
    // speculative launch schedule of a time step (newton_level): Newton slots and CG sweeps per slot, adapted from the
    // state the host reads once per step
    bool spec;
    int spec_slots = 2, spec_cgb[4] = {12, 12, 12, 12};
    // counters since the last reset_counters(): kernel launches and blocking looks at the device state
    long n_launch, n_sync;
};

// Kernel classes for the in-situ timing of vch2d_prof_begin/_end.
enum { PC_SCHUR_P = 0, PC_GEMM = 1, PC_RESIDUAL = 2, PC_ADJ_Q = 3, PC_CG_UPDATE = 4, PC_ADJ_RHS = 5, PC_COST = 6,
       PC_PROX = 7, PC_DCT_R0 = 8, PC_DCT_C = 9, PC_DCT_R3 = 10, PC_SCHUR_P1 = 11, PC_CG_ROWS = 12, PC_CG_ROWS1 = 13,
       PC_NOOP = 14, PC_GUESS = 15, PC_ADJ_GUESS = 16, PC_CHEB_ROWS = 17, PC_CHEB_ROWS0 = 18, PC_RESIDUAL0 = 19,
       PC_KRYLOV = 20 /* the streaming passes of vch2d_hess_lanczos, all in one class */, PC_NCLS = 21 };

// an empty kernel: what an event pair measures around it is the cost of the pair itself (vch2d_prof_begin)
__global__ void k_noop() {}

// Bookkeeping of LAUNCH_LDS (vch_common.h): every launch is counted; a launch of class cls >= 0 gets an event pair around
// it when profiling is on (events are recorded on the engine's own stream, the one the kernel is launched on).
static bool launch_begin(vch2d_ctx *c, int cls) {
    const bool rec = cls >= 0 && c->prof_on && c->prof_used + 2 <= c->prof_ev.size();
    if (rec) hipEventRecord(c->prof_ev[c->prof_used], c->stream);
    return rec;
}
static void launch_end(vch2d_ctx *c, int cls, bool rec) {
    c->n_launch++;
    if (rec) {
        hipEventRecord(c->prof_ev[c->prof_used + 1], c->stream);
        c->prof_cls.push_back(cls);
        c->prof_used += 2;
    }
}
#define LAUNCHC(cls, kern, grid, block, ...) LAUNCH_LDS(cls, kern, grid, block, 0, __VA_ARGS__)

static int dalloc(vch2d_ctx *c, double **p, size_t n) {
    MEMCHK(c->pool.dev(p, n * sizeof(double)));
    HIPCHK(hipMemsetAsync(*p, 0, n * sizeof(double), c->stream));
    return 0;
}

// host [nplanes][ns][nf] contiguous  <->  device [nplanes][ns][pitch]
static int h2d(vch2d_ctx *c, double *dev, const double *host, long nplanes) {
    HIPCHK(hipMemcpy2DAsync(dev, (size_t)c->G.pitch * 8, host, (size_t)c->G.nf * 8, (size_t)c->G.nf * 8,
                            (size_t)c->G.ns * nplanes, hipMemcpyHostToDevice, c->stream));
    return 0;
}
static int d2h(vch2d_ctx *c, double *host, const double *dev, long nplanes) {
    HIPCHK(hipMemcpy2DAsync(host, (size_t)c->G.nf * 8, dev, (size_t)c->G.pitch * 8, (size_t)c->G.nf * 8,
                            (size_t)c->G.ns * nplanes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
// histories: host [B][rows][ns][nf] <-> device [B][rows_alloc][plane]
static int h2d_hist(vch2d_ctx *c, double *dev, const double *host, int rows) {
    const long hs = (long)(c->Mmax + 1) * c->G.plane;
    for (int b = 0; b < c->B; ++b)
        VCHCHK(h2d(c, dev + b * hs, host + (long)b * rows * c->G.nf * c->G.ns, rows));
    return 0;
}
static int d2h_hist(vch2d_ctx *c, double *host, const double *dev, int rows) {
    const long hs = (long)(c->Mmax + 1) * c->G.plane;
    for (int b = 0; b < c->B; ++b) {
        HIPCHK(hipMemcpy2DAsync(host + (long)b * rows * c->G.nf * c->G.ns, (size_t)c->G.nf * 8, dev + b * hs,
                                (size_t)c->G.pitch * 8, (size_t)c->G.nf * 8, (size_t)c->G.ns * rows,
                                hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
static int ensure_hist(vch2d_ctx *c, double **p) {
    if (*p) return 0;
    size_t n = (size_t)c->B * (c->Mmax + 1) * c->G.plane;
    const hipError_t e = (hipError_t)c->pool.dev(p, n * sizeof(double));
    if (e != hipSuccess) {
        return vch_fail(VCH_ERR_NOMEM, "hipMalloc of a %.2f GB history failed: %s", n * 8e-9, hipGetErrorString(e));
    }
    HIPCHK(hipMemsetAsync(*p, 0, n * sizeof(double), c->stream));
    return 0;
}
static inline long hist_stride(const vch2d_ctx *c) { return (long)(c->Mmax + 1) * c->G.plane; }

// records -> mapped host memory, then the sequence number (system-scope release after a system fence)
__global__ void k_publish_state(const unsigned *__restrict__ st, int nwords, unsigned *__restrict__ dst,
                                unsigned long long *seq, int nseq, unsigned long long val) {
    for (int i = threadIdx.x; i < nwords; i += blockDim.x) dst[i] = st[i];
    __threadfence_system();
    __syncthreads();
    for (int i = threadIdx.x; i < nseq; i += blockDim.x) __hip_atomic_store(seq + i, val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One look of the host at the per-trajectory state machine.  full = false (the per-step looks of a march): the stream is
// NOT drained by a host wait -- the state arrives in mapped host memory behind everything enqueued so far and the host
// polls for it (a copy command + hipStreamSynchronize cost ~35 us of idle device per look, this path ~10).  full = true,
// or VCH_LOOK_SPIN=0: copy command and stream synchronisation (callers that go on to read other results or event times).
static int sync_state(vch2d_ctx *c, bool full = true) {
    c->n_sync++;
    if (full || !c->look_spin) {
        c->pub_pending = 0;
        HIPCHK(hipMemcpyAsync(c->st_host, c->st, sizeof(TrajState) * c->B, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return 0;
    }
    static_assert(sizeof(TrajState) % 4 == 0, "TrajState is copied in 32-bit words");
    // every trajectory's slot carries the look's number: stored by the one-workgroup kernel, or each by the workgroup of its
    // trajectory in a k_fin_residual launch that is already enqueued (pub_pending, see publish_tail)
    unsigned long long want = c->pub_pending;
    c->pub_pending = 0;
    if (!want) {
        want = ++c->seq_next;
        hipLaunchKernelGGL(k_publish_state, dim3(1), dim3(256), 0, c->stream, (const unsigned *)c->st,
                           (int)(sizeof(TrajState) / 4 * c->B), (unsigned *)c->st_pub, c->seq_pub, c->B, want);
        HIPCHK(hipGetLastError());
    }
    auto arrived = [&]() {
        for (int b = 0; b < c->B; ++b)
            if (__atomic_load_n(c->seq_pub + b, __ATOMIC_ACQUIRE) != want) return false;
        return true;
    };
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 1; !arrived(); ++spins) {
        __builtin_ia32_pause();
        if ((spins & 0x3fff) == 0) {
            const hipError_t q = hipStreamQuery(c->stream);
            if (q != hipSuccess && q != hipErrorNotReady) return vch_fail(VCH_ERR_HIP, "sync_state: %s", hipGetErrorString(q));
            if (q == hipSuccess && !arrived())
                return vch_fail(VCH_ERR_STATE, "sync_state: stream drained but the state was not published");
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
                return vch_fail(VCH_ERR_STATE, "sync_state: no state from the device after 120 s");
        }
    }
    memcpy(c->st_host, c->st_pub, sizeof(TrajState) * c->B);
    return 0;
}

// DCT-I matrices Q1 = S C^ and Q2 = C^ S^-1 and eigenvalues of the 1-D factor of M = -L.
static void dct_tables(int N, double h, std::vector<double> &Q1, std::vector<double> &Q2, std::vector<double> &m) {
    const int n = N + 1;
    Q1.assign((size_t)n * n, 0.0);
    Q2.assign((size_t)n * n, 0.0);
    m.assign(n, 0.0);
    const long double pi = 3.14159265358979323846264338327950288L;
    const long double sc = sqrtl(2.0L / N), is2 = 1.0L / sqrtl(2.0L);
    for (int j = 0; j < n; ++j) {
        long double sj = (j == 0 || j == N) ? is2 : 1.0L;
        for (int k = 0; k < n; ++k) {
            long double sk = (k == 0 || k == N) ? is2 : 1.0L;
            // exact argument reduction: cos(pi * (j k mod 2N) / N)
            long long jk = ((long long)j * k) % (2LL * N);
            long double cv = cosl(pi * (long double)jk / (long double)N);
            Q1[(size_t)j * n + k] = (double)(sc * sj * sj * sk * cv);
            Q2[(size_t)j * n + k] = (double)(sc * sj * cv);
        }
        m[j] = (double)((2.0L - 2.0L * cosl(pi * j / (long double)N)) / ((long double)h * h));
    }
}

// ---- vch2d_create in its parts: geometry, knobs, allocations, table uploads, plan.  The last three return NULL, or the name of
// the step that failed for vch2d_create's message.
static void set_geometry(vch2d_ctx *c, const vch2d_params *p, int batch, int max_steps, int device) {
    c->prm = *p;
    c->B = batch;
    c->Mmax = max_steps;
    c->device = device;
    c->hx = p->Lx / p->Nx;
    c->hy = p->Ly / p->Ny;
    Geom &G = c->G;
    G.nf = p->Nx + 1;
    G.ns = p->Ny + 1;
    G.pitch = (G.nf + 7) / 8 * 8;
    G.plane = (long)G.ns * G.pitch;
    G.tiles_f = (G.nf + TX - 1) / TX;
    G.tiles_s = (G.ns + TY - 1) / TY;
    G.ax = 1.0 / (c->hx * c->hx);
    G.ay = 1.0 / (c->hy * c->hy);
    c->P = Phys{p->tau, p->gamma, p->c1, p->c2, p->kappa, p->Lx * p->Ly};
    c->grid = dim3(G.tiles_f, G.tiles_s, batch);
    c->nblk = G.tiles_f * G.tiles_s;
    c->slot_stride = (long)batch * G.plane;
    c->gnblk = ((G.nf + GN - 1) / GN) * ((G.ns + GM - 1) / GM);      // the GEMM epilogue's workgroups: gpart is sized by them
    c->pol1.resize(batch);
    c->pol2.resize(batch);
    c->used1.assign(batch, 0);
    c->used2.assign(batch, 0);
    c->run2.assign(batch, 0);
}

// Every environment knob that is read once, at creation (VCH_ADJ_GUESS_OFF and VCH_ADJ_SAFE are read at the start of every
// sweep, backward_core).  A switch is either on unless it is set to 0 (env_on) or on when it is set at all (env_set).
// The kernel a launch takes under VCH_LOADS_BATCH: k (the default) or k_plain; LB_T for a template's instance.
#define LB(k) (c->loads_batch ? k : k##_plain)
#define LB_T(k, ...) (c->loads_batch ? k<__VA_ARGS__> : k##_plain<__VA_ARGS__>)
static void read_knobs(vch2d_ctx *c) {
    auto env_on = [](const char *name) { const char *e = getenv(name); return !(e && atoi(e) == 0); };
    auto env_set = [](const char *name) { return getenv(name) != nullptr; };
    c->lin_tol = 1e-15;
    if (const char *e = getenv("VCH_LIN_TOL")) c->lin_tol = atof(e);      // tuning/experiments only
    // Newton solves inside a march are stopped when the Schur residual they leave is 5 % of the Newton tolerance
    // (newton_lin_tol in vch_kernels2d.h); 0 = always lin_tol
    c->lin_eta = 0.05 * NEWTON_TOL;
    if (const char *e = getenv("VCH_LIN_ETA")) c->lin_eta = atof(e);
    c->cols_c = 1024;          // 2048 equal, 4096 slower (profiles/r02_cols_width.txt)
    if (const char *e = getenv("VCH_COLS_C")) c->cols_c = atoi(e);
    c->spec = !env_set("VCH_NO_SPEC");
    c->cheb_on = env_on("VCH_CHEB");
    c->debug_guess = env_set("VCH_DEBUG_GUESS");
    // measured on the 512^2 x 1000 x 8 march (profiles/r03_fused_ab.txt): separate kernels 0.564 s, fused with the fin step
    // by the last-finishing workgroup 0.566 s (the serial tail of that workgroup costs what the saved launch gained), fused
    // with the fin step as its own launch 0.523 s -- the default
    c->fused_mode = getenv("VCH_FUSED") ? atoi(getenv("VCH_FUSED")) : 2;
    c->fused_on = c->fused_mode != 0;
    c->post_fold = true;
    if (const char *e = getenv("VCH_POST_FOLD")) c->post_fold = atoi(e) != 0;
    c->mass_early = env_on("VCH_MASS_EARLY");
    c->fin_publish = env_on("VCH_FIN_PUBLISH");
    c->ceil_cell_on = env_on("VCH_CEIL_CELL");
    c->eval_hoist = env_on("VCH_EVAL_HOIST");
    c->rows_batch = env_on("VCH_ROWS_BATCH");
    c->loads_batch = env_on("VCH_LOADS_BATCH");
    c->cheb_margin = 1;
    if (const char *e = getenv("VCH_CHEB_MARGIN")) c->cheb_margin = std::max(0, atoi(e));
    c->cheb_max = 6;           // plans longer than this (a wide spectrum: CG's adaptivity pays) keep the CG form
    if (const char *e = getenv("VCH_CHEB_MAX")) c->cheb_max = std::max(0, atoi(e));
    c->pgd_adj_tol = 1e-12;
    if (const char *e = getenv("VCH_ADJ_TOL")) c->pgd_adj_tol = atof(e);
    c->eta1_factor = 1e-2;
    if (const char *e = getenv("VCH_ETA1")) c->eta1_factor = atof(e);
    c->cg_scale_ratio = 4.0;
    if (const char *e = getenv("VCH_CG_SCALE")) c->cg_scale_ratio = atof(e);
    c->look_spin = env_on("VCH_LOOK_SPIN");
    // consumed by make_plan
    c->knob_gemm_dct = env_set("VCH_FORCE_GEMM_DCT");
    c->knob_dct_half = env_set("VCH_DCT_HALF");
    c->knob_guess = env_on("VCH_GUESS");
    c->guess2_on = env_on("VCH_GUESS2");
    c->guess_max = 6;          // beyond, the weights (sum |c_j| = 2^order - 1) amplify what the inexact solves left in the increments
    if (const char *e = getenv("VCH_GUESS_MAX")) c->guess_max = std::max(1, std::min(GUESS_ORD, atoi(e)));
    c->kr_lchunk = 16;         // 512^2, one trajectory of 1001 levels: 297 tiles x 63 chunks of workgroups
    if (const char *e = getenv("VCH_KR_LCHUNK")) c->kr_lchunk = std::max(1, atoi(e));
    c->kr_nocache = getenv("VCH_KRYLOV_NOCACHE") && atoi(getenv("VCH_KRYLOV_NOCACHE")) != 0;
}

// The buffers every context has (histories and the buffers of single calls come lazily).  zero(): doubles, cleared on the
// stream; dev(): bytes of any type, cleared where a kernel reads them before anything writes them.
static const char *alloc_buffers(vch2d_ctx *c) {
    const Geom &G = c->G;
    const size_t B = c->B, bp = B * G.plane, ng = B * (c->gnblk + G.ns);
    bool ok = true;                    // nothing more is requested after the first refusal
    auto zero = [&](double **q, size_t n) { ok = ok && dalloc(c, q, n) == 0; };
    auto dev = [&](auto **q, size_t bytes, bool clear) {
        ok = ok && c->pool.dev(q, bytes) == 0;
        if (ok && clear) hipMemsetAsync(*q, 0, bytes, c->stream);
    };
    for (double **q : {&c->phi_s, &c->mu_s, &c->Rphi_s, &c->rhs_s, &c->D_s}) zero(q, 2 * bp);
    for (double **q : {&c->w, &c->wnew, &c->mu0, &c->cphi, &c->cmu, &c->x, &c->r, &c->dmu, &c->t1, &c->t2, &c->cg_p[0],
                       &c->cg_p[1], &c->cg_v, &c->cg_q, &c->cg_z2, &c->xf})
        zero(q, bp);
    for (double *&q : c->dprev) zero(&q, bp);
    for (double *&q : c->dprev2) zero(&q, bp);
    zero(&c->x0g, bp);
    for (double *&q : c->tmp) zero(&q, bp);
    zero(&c->phiT, bp);
    zero(&c->phi0, bp);
    zero(&c->wts_mass, G.plane);
    zero(&c->W_cost, G.plane);
    zero(&c->part, B * c->nblk * NPART);
    zero(&c->part_mass, B * c->nblk * NPART);
    zero(&c->gpart, 2 * ng);
    c->gpart2 = c->gpart + ng;
    zero(&c->gpart3, 4 * ng);
    zero(&c->hist_dev, B * HIST_CAP);
    zero(&c->shift_hist, B * c->Mmax * SHIFT_REC);
    zero(&c->shift_trial, B * c->Mmax * SHIFT_REC);
    zero(&c->alpha_dev, B);
    zero(&c->J_dev, 5 * B);
    zero(&c->opt_tab, OPT_STRIDE * B);
    zero(&c->seam_tab, OPT_STRIDE * B);
    dev(&c->kkt_dev, sizeof(unsigned long long) * 3 * B * (c->Mmax + 2), false);
    zero(&c->J_ring_dev, J_RING * 5 * B);
    if (!ok) return "hipMalloc";
    if (c->pool.host(&c->J_ring_host, sizeof(double) * J_RING * 5 * B)) return "hipHostMalloc";
    dev(&c->st, sizeof(TrajState) * B, true);
    dev(&c->frozen_dev, sizeof(int) * B, false);
    dev(&c->fin_counter, sizeof(unsigned) * B, true);
    dev(&c->ceil_cell, sizeof(unsigned long long) * CeilCell::STRIDE * B, true);
    if (!ok) return "hipMalloc";
    if (c->pool.host(&c->st_host, sizeof(TrajState) * B)) return "hipHostMalloc";
    // looks through mapped host memory (sync_state); where the platform refuses mapped coherent memory the looks fall back
    // to a copy command and a stream synchronisation
    if (c->look_spin) {
        const unsigned mapped = hipHostMallocMapped | hipHostMallocCoherent;
        vch_group look(c->pool);
        if (c->pool.host(&c->st_pub, sizeof(TrajState) * B, mapped) ||
            c->pool.host(&c->seq_pub, std::max<size_t>(64, sizeof(unsigned long long) * B), mapped)) {
            (void)hipGetLastError();
            c->look_spin = false;      // and the group takes st_pub back
        } else {
            for (size_t b = 0; b < B; ++b) c->seq_pub[b] = 0;
            look.keep();
        }
    }
    if (c->pool.host(&c->hist_host, sizeof(double) * B * HIST_CAP)) return "hipHostMalloc";
    return nullptr;
}

static const char *upload_tables(vch2d_ctx *c) {
    const Geom &G = c->G;
    // mass weights hx*hy*outer(trapz(Nx+1), trapz(Ny+1)) on the TRUE (i, j) of each flat entry (F2:528-531)
    std::vector<double> wm((size_t)G.plane, 0.0);
    const int nx1 = c->prm.Nx + 1, ny1 = c->prm.Ny + 1;
    for (int i = 0; i < nx1; ++i)
        for (int j = 0; j < ny1; ++j) {
            long f = (long)i * ny1 + j;
            double wi = (i == 0 || i == nx1 - 1) ? 0.5 : 1.0, wj = (j == 0 || j == ny1 - 1) ? 0.5 : 1.0;
            wm[(f / G.nf) * G.pitch + (f % G.nf)] = c->hx * c->hy * (wi * wj);
        }
    if (hipMemcpy(c->wts_mass, wm.data(), wm.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return "hipMemcpy";
    // DCT tables
    std::vector<double> Q1, Q2, m;
    auto up = [&](double **d, const std::vector<double> &v) {
        return c->pool.dev(d, v.size() * 8) == 0 && hipMemcpy(*d, v.data(), v.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
    };
    dct_tables(c->prm.Nx, c->hx, Q1, Q2, m);
    if (!up(&c->Q1f, Q1) || !up(&c->Q2f, Q2) || !up(&c->mf, m)) return "DCT table upload";
    dct_tables(c->prm.Ny, c->hy, Q1, Q2, m);
    if (!up(&c->Q1s, Q1) || !up(&c->Q2s, Q2) || !up(&c->ms, m)) return "DCT table upload";
    return nullptr;
}

// FFT plan (power-of-two grids) and what follows from it
static const char *make_plan(vch2d_ctx *c) {
    const vch2d_params *p = &c->prm;
    const Geom &G = c->G;
    auto pow2 = [](int n) { return n >= 16 && n <= 2048 && (n & (n - 1)) == 0; };
    c->use_fft = pow2(p->Nx) && pow2(p->Ny) && !c->knob_gemm_dct;
    if (c->use_fft) {
        auto mk = [&](int N, double2 **tw, FftAxis &ax) {
            const int L = 2 * N;
            std::vector<double2> t(L);
            const long double pi = 3.14159265358979323846264338327950288L;
            for (int m = 0; m < L; ++m) {
                long double a = -2.0L * pi * m / L;
                t[m] = make_double2((double)cosl(a), (double)sinl(a));
            }
            if (c->pool.dev(tw, sizeof(double2) * L)) return false;
            if (hipMemcpy(*tw, t.data(), sizeof(double2) * L, hipMemcpyHostToDevice) != hipSuccess) return false;
            int lg = 0;
            while ((1 << lg) < L) ++lg;
            ax = FftAxis{N, L, lg, *tw};
            return true;
        };
        if (!mk(p->Nx, &c->tw_f, c->fax) || !mk(p->Ny, &c->tw_s, c->sax)) return "FFT twiddle upload";
        // half-size DCT-I (vch_fft.h, k_dcth_*) where the axis has 512 intervals: opt-in (VCH_DCT_HALF=1), it does half
        // the butterflies but measured 5-30 % slower per pass on MI355X (profiles/r01_c_fft_variants.txt)
        if (c->knob_dct_half && p->Nx == HN) {
            if (!mk(HN / 2, &c->tw_fh, c->fax_h)) return "FFT twiddle upload";
            c->half_f = true;
        }
        if (c->knob_dct_half && p->Ny == HN) {
            if (!mk(HN / 2, &c->tw_sh, c->sax_h)) return "FFT twiddle upload";
            c->half_s = true;
        }
        if (c->half_f) {
            c->gnblk = (G.ns + 3) / 4;
        } else {
            const int Cc = c->fax.L <= 1024 ? 1024 : c->fax.L;
            const int rpw = 2 * (Cc >> c->fax.logL);
            c->gnblk = (G.ns + rpw - 1) / rpw;
        }
    }
    // starting guess of a step's first Newton solve (k_guess): stencil-free sweep only; VCH_GUESS=0 turns it off
    c->guess_on = c->use_fft && !c->half_f && !c->half_s && c->knob_guess;
    return nullptr;
}

// Everything a context holds, in the order that is safe for one that vch2d_create only half built.
static void teardown(vch2d_ctx *c) {
    if (c->stream) hipStreamSynchronize(c->stream);
    c->pool.release();
    for (hipEvent_t e : c->prof_ev) hipEventDestroy(e);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

extern "C" vch2d_ctx *vch2d_create(const vch2d_params *p, int batch, int max_steps, int device) {
    if (!p || p->Nx < 2 || p->Ny < 2 || batch < 1 || max_steps < 1 || !(p->Lx > 0) || !(p->Ly > 0)) {
        vch_fail(VCH_ERR_ARG, "vch2d_create: bad arguments (Nx,Ny >= 2, batch >= 1, max_steps >= 1)");
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        (void)hipGetLastError();          // do not leave the sticky error for the next launch check
        vch_fail(VCH_ERR_HIP, "hipSetDevice(%d) failed", device);
        return nullptr;
    }
    vch2d_ctx *c = new vch2d_ctx();
    set_geometry(c, p, batch, max_steps, device);
    read_knobs(c);
    auto fail = [&](const char *what) {
        vch_fail(VCH_ERR_HIP, "vch2d_create: %s failed: %s", what, hipGetErrorString(hipGetLastError()));
        teardown(c);
        return (vch2d_ctx *)nullptr;
    };
    if (hipStreamCreate(&c->stream) != hipSuccess) return fail("hipStreamCreate");
    hipEventCreate(&c->ev0);
    hipEventCreate(&c->ev1);
    if (const char *what = alloc_buffers(c)) return fail(what);
    if (const char *what = upload_tables(c)) return fail(what);
    if (const char *what = make_plan(c)) return fail(what);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail("hipStreamSynchronize");
    return c;
}

extern "C" void vch2d_destroy(vch2d_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    teardown(c);
}

extern "C" int vch2d_batch(const vch2d_ctx *c) { return c ? c->B : VCH_ERR_ARG; }

// ------------------------------------------------------------------------------------
// FFT pass launches.  A compile-time plan is C complex doubles per workgroup (1024 unless the FFT is longer) and LOGL =
// log2 of the FFT length, 0 for a run-time length; lengths 512 / 1024 / 2048 (grids 256^2, 512^2, 1024^2) are compiled
// with a constant length.  with_plan calls f with the plan of `ax` as two std::integral_constant and returns its status.
// ------------------------------------------------------------------------------------
template <class F>
static int with_plan(const FftAxis &ax, F &&f) {
    using std::integral_constant;
    if (ax.logL == 10) return f(integral_constant<int, 1024>(), integral_constant<int, 10>());
    if (ax.logL == 9) return f(integral_constant<int, 1024>(), integral_constant<int, 9>());
    if (ax.logL < 10) return f(integral_constant<int, 1024>(), integral_constant<int, 0>());
    if (ax.logL == 11) return f(integral_constant<int, 2048>(), integral_constant<int, 11>());
    return f(integral_constant<int, 4096>(), integral_constant<int, 0>());
}

// grid and block of the row kernels (vch_fft.h) for the plan (C, LG) of c->fax: a workgroup owns 2 C / L rows
struct RowsDims { dim3 grid, block; };
template <int C, int LG>
static RowsDims rows_dims(const vch2d_ctx *c) {
    const int rpw = 2 * (C >> c->fax.logL);
    return {dim3((c->G.ns + rpw - 1) / rpw, 1, c->B), dim3(FftThreads<C, LG>::T)};
}

// k_dct_rows<EPI> (E along the fast axis): in -> out
template <int EPI>
static int dct_rows(vch2d_ctx *c, const double *in, long in_slot_stride, double *out, const SpecArgs &sp, int gate) {
    return with_plan(c->fax, [&](auto C, auto LG) {
        const RowsDims d = rows_dims<C, LG>(c);
        LAUNCHC(EPI >= 3 ? PC_DCT_R3 : PC_DCT_R0, (k_dct_rows<EPI, C, LG>), d.grid, d.block, c->G, c->fax, in, in_slot_stride,
                out, 1.0, sp, c->st, gate);
        return 0;
    });
}
// the same by the half-size DCT (k_dcth_rows, opt-in)
template <int EPI>
static int dcth_rows(vch2d_ctx *c, const double *in, long in_slot_stride, double *out, const SpecArgs &sp, int gate) {
    LAUNCHC(EPI == 3 ? PC_DCT_R3 : PC_DCT_R0, (k_dcth_rows<EPI>), dim3((c->G.ns + 3) / 4, 1, c->B), dim3(HT), c->G, c->fax,
            c->fax_h, in, in_slot_stride, out, 1.0, sp, c->st, gate);
    return 0;
}

// k_dct_cols (E along the slow axis, spectral multiplier, E again): c->t1 -> c->t2
template <int C, int LOGL>
static int dct_cols_plan(vch2d_ctx *c, const SpecArgs &sp, double scale, int gate) {
    const int cpw = 2 * (C >> c->sax.logL);
    auto k_cols = c->rows_batch ? k_dct_cols<C, LOGL> : k_dct_cols_plain<C, LOGL>;
    LAUNCHC(PC_DCT_C, k_cols, dim3((c->G.nf + cpw - 1) / cpw, 1, c->B), dim3(FftThreads<C, LOGL>::T), c->G,
            c->sax, (const double *)c->t1, c->t2, scale, sp, c->st, gate);
    return 0;
}
static int dct_cols(vch2d_ctx *c, const SpecArgs &sp, double scale, int gate) {
    // the column pass reads 16 bytes per row and column pair: at length 1024 a workgroup that owns 2 C / 1024 adjacent
    // columns uses that share of every 128-byte line it pulls through L2 (profiles/r02_cols_width.txt)
    const int wide = c->sax.logL == 10 ? c->cols_c : 0;
    if (wide == 4096) return dct_cols_plan<4096, 10>(c, sp, scale, gate);
    if (wide == 2048) return dct_cols_plan<2048, 10>(c, sp, scale, gate);
    return with_plan(c->sax, [&](auto C, auto LG) { return dct_cols_plan<C, LG>(c, sp, scale, gate); });
}

// first pass of a stencil-free forward CG sweep (k_cg_rows_fwd): E_rows(Delta p) -> c->t1
static int cg_rows(vch2d_ctx *c, const CgSweepArgs &a, bool first) {
    return with_plan(c->fax, [&](auto C, auto LG) {
        const RowsDims d = rows_dims<C, LG>(c);
        auto k_rows = first ? k_cg_rows_fwd<1, C, LG> : k_cg_rows_fwd<0, C, LG>;
        LAUNCHC(first ? PC_CG_ROWS1 : PC_CG_ROWS, k_rows, d.grid, d.block, c->G, c->fax, a, c->t1, c->st);
        return 0;
    });
}

// row kernel of a reduction-free sweep (k_cheb_rows): c->t2 -> c->t1
static int cheb_rows(vch2d_ctx *c, const ChebSweepArgs &a, bool first) {
    return with_plan(c->fax, [&](auto C, auto LG) {
        const RowsDims d = rows_dims<C, LG>(c);
        auto k_rows = c->rows_batch ? (first ? k_cheb_rows<C, LG, 1> : k_cheb_rows<C, LG, 0>)
                                    : (first ? k_cheb_rows_plain<C, LG, 1> : k_cheb_rows_plain<C, LG, 0>);
        LAUNCHC(first ? PC_CHEB_ROWS0 : PC_CHEB_ROWS, k_rows, d.grid, d.block, c->G, c->fax, a, (const double *)c->t2, c->t1,
                (const TrajState *)c->st);
        return 0;
    });
}

// first pass of an adjoint CG sweep (k_adj_rows_fwd): -> c->t1
static int adj_rows(vch2d_ctx *c, const AdjSweepArgs &a, bool first) {
    return with_plan(c->fax, [&](auto C, auto LG) {
        const RowsDims d = rows_dims<C, LG>(c);
        auto k_rows = first ? k_adj_rows_fwd<1, C, LG> : k_adj_rows_fwd<0, C, LG>;
        LAUNCHC(PC_ADJ_Q, k_rows, d.grid, d.block, c->G, c->fax, a, c->t1, c->st);
        return 0;
    });
}

// ------------------------------------------------------------------------------------
// fast-diagonalisation preconditioner:  out = (c0 + m (c1a + c1b dbar + c2 m))^-1 in
//   last: 0 store; 3 store + partial of sum W (D[slot] - dbar) other*out into c->gpart
//         (other == NULL: out*out); 4 (FFT path only): out = other + result
// ------------------------------------------------------------------------------------
static int precond(vch2d_ctx *c, const double *in, long in_slot_stride, double *out, int last, const double *other,
                   double c0, double c1a, double c1b, double c2, int gate) {
    const Geom &G = c->G;
    const int ns = G.ns, nf = G.nf;
    dim3 g((nf + GN - 1) / GN, (ns + GM - 1) / GM, c->B);
    SpecArgs sp{c0, c1a, c1b, c2, c->ms, c->mf, other, c->D_s, c->slot_stride, c->gpart, c->gpart2, 0};
    if (c->use_fft) {
        const double scale = 1.0 / (4.0 * (double)c->fax.N * (double)c->sax.N);
        if (c->half_f) VCHCHK(dcth_rows<0>(c, in, in_slot_stride, c->t1, sp, gate));
        else VCHCHK(dct_rows<0>(c, in, in_slot_stride, c->t1, sp, gate));
        if (c->half_s)
            LAUNCHC(PC_DCT_C, k_dcth_cols, dim3((nf + 3) / 4, 1, c->B), dim3(HT), G, c->sax, c->sax_h, (const double *)c->t1, c->t2,
                    scale, sp, c->st, gate);
        else VCHCHK(dct_cols(c, sp, scale, gate));
        if (c->half_f) {
            if (last == 3) VCHCHK(dcth_rows<3>(c, c->t2, 0L, out, sp, gate));
            else VCHCHK(dcth_rows<0>(c, c->t2, 0L, out, sp, gate));
        } else if (last == 3) VCHCHK(dct_rows<3>(c, c->t2, 0L, out, sp, gate));
        else if (last == 4) VCHCHK(dct_rows<4>(c, c->t2, 0L, out, sp, gate));
        else VCHCHK(dct_rows<0>(c, c->t2, 0L, out, sp, gate));
        return 0;
    }
    // T1 = g Q1f
    LAUNCHC(PC_GEMM, (k_gemm<false, 0>), g, dim3(256), ns, nf, nf, in, (long)G.pitch, G.plane, in_slot_stride, c->Q1f, (long)nf, 0L,
           c->t1, (long)G.pitch, G.plane, sp, c->st, gate);
    // T2 = (Q1s^T T1) o mult
    LAUNCHC(PC_GEMM, (k_gemm<true, 1>), g, dim3(256), ns, nf, ns, c->Q1s, (long)ns, 0L, 0L, c->t1, (long)G.pitch, G.plane, c->t2,
           (long)G.pitch, G.plane, sp, c->st, gate);
    // T3 = Q2s^T T2
    LAUNCHC(PC_GEMM, (k_gemm<true, 0>), g, dim3(256), ns, nf, ns, c->Q2s, (long)ns, 0L, 0L, c->t2, (long)G.pitch, G.plane, c->t1,
           (long)G.pitch, G.plane, sp, c->st, gate);
    // out = T3 Q2f
    if (last == 3)
        LAUNCHC(PC_GEMM, (k_gemm<false, 3>), g, dim3(256), ns, nf, nf, c->t1, (long)G.pitch, G.plane, 0L, c->Q2f, (long)nf, 0L, out,
               (long)G.pitch, G.plane, sp, c->st, gate);
    else
        LAUNCHC(PC_GEMM, (k_gemm<false, 0>), g, dim3(256), ns, nf, nf, c->t1, (long)G.pitch, G.plane, 0L, c->Q2f, (long)nf, 0L, out,
               (long)G.pitch, G.plane, sp, c->st, gate);
    return 0;
}

// Passes 2 and 3 of a stencil-free forward CG sweep (after k_cg_rows_fwd has left E_rows(Delta p) in c->t1):
// column transforms with the multiplier m / P(m), then q = p + E_rows(.) with the partials of <p,q>_Z, <q,q>_Z.
static int sweep_tail(vch2d_ctx *c, const double *p, double *q, double c0, double c2, int gate) {
    const SpecArgs sp{c0, 0.0, 1.0, c2, c->ms, c->mf, p, c->D_s, c->slot_stride, c->gpart, c->gpart2, 1};
    VCHCHK(dct_cols(c, sp, 1.0 / (4.0 * (double)c->fax.N * (double)c->sax.N), gate));
    return dct_rows<4>(c, c->t2, 0L, q, sp, gate);
}

// CG iterations to enqueue: the largest rigorous bound among the trajectories still solving
static int cg_budget(const vch2d_ctx *c, bool only_newton_active) {
    int n = 0;
    for (int b = 0; b < c->B; ++b) {
        const TrajState &S = c->st_host[b];
        if (!S.lin_active) continue;
        if (only_newton_active && !S.newton_active) continue;
        n = std::max(n, S.lin_budget);
    }
    return std::min(n, c->lin_maxit);
}
static bool any_lin_active(const vch2d_ctx *c) {
    for (int b = 0; b < c->B; ++b)
        if (c->st_host[b].lin_active) return true;
    return false;
}
constexpr int CG_CHUNK = 24;      // iterations enqueued between two looks at the state

// CG on the Schur system of the current Newton iterate (left-preconditioned, weighted inner
// product W (D - dbar)); on return x = dphi.  `budget` sweeps are enqueued; `look` = the host may look at the
// state inside a long solve (every CG_CHUNK sweeps) to stop enqueueing once every trajectory has converged.
// Every kernel is gated per trajectory (lin_active / the per-iteration copies), so trajectories that are not
// solving -- converged, frozen, or waiting for an Armijo trial -- keep their x.
static int schur_solve(vch2d_ctx *c, double dt, int budget, bool look) {
    c->cg_last = -1;
    if (budget <= 0) return 0;
    const double c0 = 1.0 / dt, c2 = 0.5 * c->P.kappa;
    double *zb[2] = {c->r, c->cg_z2};               // z_k lives in zb[k & 1]
    VCHCHK(precond(c, c->rhs_s, c->slot_stride, zb[0], 3, nullptr, c0, 0.0, 1.0, c2, 5));      // z = P^-1 rhs, <z,z>_Z (CG-form trajectories)
    const bool spectral = c->use_fft && !c->half_f && !c->half_s;      // stencil-free sweep (k_cg_rows_fwd)
    if (!spectral) LAUNCH(k_fin_cg_init, dim3(c->B), dim3(64), c->st, c->gpart, c->gnblk);     // else: inside the first sweep
    int done = 0;
    while (done < budget) {
        const int chunk = look ? std::min(budget - done, CG_CHUNK) : budget - done;
        for (int j = 0; j < chunk; ++j, ++done) {
            double *pn = c->cg_p[done & 1], *po = c->cg_p[(done + 1) & 1];
            if (spectral) {
                // sweep `done`: the reduction point of sweep done-1 is resolved inside the first kernel and its step goes
                // into x and z on the way into the row transform; 3 launches per sweep, no stencil
                CgSweepArgs a{done == 0 ? zb[0] : zb[(done + 1) & 1], c->cg_q, po, c->x, zb[done & 1], pn, c->D_s, c->slot_stride,
                              c->gpart, c->gpart2, c->gpart3, done, c->lin_maxit, c->B, c->x0g};
                VCHCHK(cg_rows(c, a, done == 0));
                VCHCHK(sweep_tail(c, pn, c->cg_q, c0, c2, 2 + (done & 1)));      // q = P^-1 A p, <p,q>_Z, <q,q>_Z
                continue;
            }
            // GEMM-DCT grids: the 13-point operator as a stencil, fused with the CG vector updates; 4 launches + the GEMMs
            if (done == 0) {
                LAUNCHC(PC_SCHUR_P1, (k_schur_p<1>), c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, zb[0], c->cg_q, po, c->D_s, dt,
                        c->x, zb[1], pn, c->cg_v, c->part, (const double *)c->gpart, (const double *)c->gpart2, c->gnblk, 0,
                        c->lin_tol, c->lin_maxit);
            } else {
                LAUNCHC(PC_SCHUR_P, (k_schur_p<0>), c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, zb[(done + 1) & 1], c->cg_q, po,
                        c->D_s, dt, c->x, zb[done & 1], pn, c->cg_v, c->part, (const double *)c->gpart, (const double *)c->gpart2,
                        c->gnblk, done, c->lin_tol, c->lin_maxit);
            }
            VCHCHK(precond(c, c->cg_v, 0, c->cg_q, 3, pn, c0, 0.0, 1.0, c2, 2 + (done & 1)));   // q = P^-1 A p, <p,q>_Z, <q,q>_Z
        }
        if (done < budget) {
            LAUNCH(k_cg_publish, dim3((c->B + 63) / 64), dim3(64), c->st, (done - 1) & 1, c->B);
            VCHCHK(sync_state(c, false));
            if (!any_lin_active(c)) break;
        }
    }
    // the reduction point of the last enqueued sweep and its step: inside the back-substitution kernel on the spectral
    // path (dmu_ceiling below), two small launches on the GEMM path
    c->cg_last = done - 1;
    if (!spectral) {
        LAUNCH(k_fin_cg_step, dim3(c->B), dim3(192), c->st, c->gpart, c->gpart2, c->gnblk, c->part, c->nblk, (done - 1) & 1,
               done - 1 >= 1 ? 1 : 0, (done - 1) & 1, (done - 1) & 1, c->lin_tol, c->lin_maxit);
        LAUNCHC(PC_CG_UPDATE, k_cg_finish, c->grid, dim3(NTH), c->G, c->st, c->cg_p[0], c->cg_p[1], c->x);
    }
    return 0;
}

// The same solve in the reduction-free form (vch_fft.h, k_cheb_rows): `n_enq` sweeps are enqueued, every trajectory runs
// the number its own plan asks for (TrajState::cheb_n, set with the solve's tolerance by k_fin_residual) and stores its
// finished increment x0 + y in c->x; one whose plan is longer than n_enq is left unfinished (k_fin_ceiling).
static int cheb_solve(vch2d_ctx *c, double dt, int n_enq) {
    c->cheb_enq = n_enq;
    const double c0 = 1.0 / dt, c2 = 0.5 * c->P.kappa;
    const double scale = 1.0 / (4.0 * (double)c->fax.N * (double)c->sax.N);
    {   // E_rows(rhs), then E_cols, 1 / P(m), E_cols (the transform pair's scale is applied by k_cheb_rows)
        const SpecArgs sp{c0, 0.0, 1.0, c2, c->ms, c->mf, nullptr, c->D_s, c->slot_stride, c->gpart, c->gpart2, 0};
        VCHCHK(dct_rows<0>(c, c->rhs_s, c->slot_stride, c->t1, sp, 8));
        VCHCHK(dct_cols(c, sp, 1.0, 8));
    }
    for (int j = 0; j <= n_enq; ++j) {
        // y_j lives in cg_p[j & 1] (y_{j+1} overwrites y_{j-1}), b~ in c->r
        ChebSweepArgs a{c->r, c->r, c->cg_p[j & 1], c->cg_p[(j + 1) & 1], c->cg_p[(j + 1) & 1], c->xf, c->x0g, c->D_s, c->slot_stride,
                        j == 0 ? c->gpart : c->gpart2, j, scale, c->phi_s, c->gpart3,
                        c->guess_wr >= 0 ? c->dprev[c->guess_wr] : (double *)nullptr,
                        (c->guess_wr >= 0 && c->guess2_on) ? c->dprev2[c->guess_wr] : (double *)nullptr,
                        c->cell_now ? c->ceil_cell : (unsigned long long *)nullptr};
        VCHCHK(cheb_rows(c, a, j == 0));
        if (j < n_enq) {   // E_cols, m / P(m), E_cols of E_rows(Delta y_{j+1}) for the trajectories that go on to sweep j + 1
            const SpecArgs sp{c0, 0.0, 1.0, c2, c->ms, c->mf, nullptr, c->D_s, c->slot_stride, c->gpart, c->gpart2, 1};
            VCHCHK(dct_cols(c, sp, 1.0, 16 + j + 1));
        }
    }
    return 0;
}

// After schur_solve: dphi -> c->xf, dmu = 2 (K dphi + R_phi), step ceiling, start of the Armijo loop (F2:377-396).
static int dmu_ceiling(vch2d_ctx *c, int strict) {
    const bool spectral = c->use_fft && !c->half_f && !c->half_s;
    const ChebFin nocheb{-1, 0, nullptr, nullptr, nullptr};
    if (spectral && c->cheb_enq >= 0) {
        // reduction-free solves: the last row kernel has stored dphi (c->xf), kept it for the guesses and taken the ceiling
        // ratios; the trial kernel does the back substitution itself.  With the ceiling cells the trial launches that follow
        // (k_eval<2>, k_fin_residual<1>) also do what k_fin_ceiling does here
        if (c->cell_now) c->trial_enq = c->cheb_enq;
        else
            LAUNCH(k_fin_ceiling, dim3(c->B), dim3(64), c->st, c->part, c->nblk, strict, -1,
                   ChebFin{c->cheb_enq, c->gnblk, c->gpart, c->gpart2, c->gpart3});
    }
    if (spectral && c->cg_last >= 0) {
        const int last = c->cg_last, rd = last & 1;
        FinSolveArgs f{c->gpart, c->gpart2, c->gpart3 + (size_t)rd * c->B * c->gnblk, c->gnblk, last >= 1 ? 1 : 0, rd, c->lin_maxit,
                       c->cg_p[last & 1], -1};
        LAUNCH(k_dmu_ceiling_fin, c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, (const double *)c->x, f, (const double *)c->phi_s,
               (const double *)c->D_s, (const double *)c->Rphi_s, c->dmu, c->xf, c->part,
               c->guess_wr >= 0 ? c->dprev[c->guess_wr] : (double *)nullptr,
               (c->guess_wr >= 0 && c->guess2_on) ? c->dprev2[c->guess_wr] : (double *)nullptr);
        LAUNCH(k_fin_ceiling, dim3(c->B), dim3(64), c->st, c->part, c->nblk, strict, rd ^ 1, nocheb);
    } else if (!spectral) {
        LAUNCH(k_dmu_ceiling, c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, c->x, c->phi_s, c->D_s, c->Rphi_s, c->dmu, c->xf,
               c->part);
        LAUNCH(k_fin_ceiling, dim3(c->B), dim3(64), c->st, c->part, c->nblk, strict, -1, nocheb);
    }
    c->cg_last = -1;
    c->cheb_enq = -1;
    return 0;
}

static const FinTail NO_FIN_TAIL{ChebFin{-1, 0, nullptr, nullptr, nullptr}, nullptr, nullptr, 0};
// The tail that makes a k_fin_residual launch publish the state for the look that follows it (sync_state(c, false)).
static FinTail publish_tail(vch2d_ctx *c, FinTail t) {
    c->pub_pending = ++c->seq_next;
    t.pub = c->st_pub;
    t.seq = c->seq_pub;
    t.val = c->pub_pending;
    return t;
}

// One residual evaluation of the pending Armijo trials.  inline_dmu (marches on the stencil-free path): the back
// substitution happens inside the trial kernel, whichever form the solve took (k_eval<2>, or k_residual2 with VCH_FUSED=0).
// publish (the default path only): the host's look follows this launch, and its k_fin_residual<1> publishes the state.
static int residual_trial(vch2d_ctx *c, double dt, bool inline_dmu, bool fused, bool fin_inside, bool guess, double eta,
                          const SolveOpts &so, const EvalFin &efin, bool publish) {
    if (inline_dmu && fused) {
        GuessArgs gt = c->gtab2;
        if (!guess) memset(gt.c, 0, sizeof(gt.c));
        // the trial of a reduction-free solve that no k_fin_ceiling launch has closed (dmu_ceiling): this launch pair only
        EvalFin ef = efin;
        ef.cheb_enq = c->trial_enq;
        c->trial_enq = -1;
        auto k_trial = c->eval_hoist ? (fin_inside ? k_eval<2, true> : k_eval<2, false>)
                                     : (fin_inside ? k_eval_plain<2, true> : k_eval_plain<2, false>);
        LAUNCHC(PC_RESIDUAL, k_trial, c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, c->phi_s, c->mu_s, c->Rphi_s, c->rhs_s,
                c->D_s, (const double *)c->xf, c->cphi, c->cmu, dt, c->part, (const double *)nullptr, (const double *)nullptr,
                (const double *)nullptr, 0L, (double *)nullptr, gt, c->x0g, ef, PostArgs{nullptr, nullptr, 0});
        if (!fin_inside) {
            FinTail tail{ChebFin{ef.cheb_enq, c->gnblk, c->gpart, c->gpart2, nullptr}, nullptr, nullptr, 0};
            if (publish) tail = publish_tail(c, tail);
            LAUNCH(LB_T(k_fin_residual, 1), dim3(c->B), dim3(64), c->st, c->part, c->nblk, c->hist_dev, c->P.kappa, dt, c->lin_tol, eta,
                   guess ? (int)c->gmask2 : 0, so, tail);
        }
        return 0;
    }
    if (inline_dmu)
        LAUNCHC(PC_RESIDUAL, k_residual2, c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, c->phi_s, c->mu_s, c->Rphi_s,
                c->rhs_s, c->D_s, (const double *)c->xf, c->cphi, c->cmu, dt, c->part);
    else
        LAUNCHC(PC_RESIDUAL, (k_residual<1>), c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, c->phi_s, c->mu_s, c->Rphi_s,
                c->rhs_s, c->D_s, c->mu0, c->xf, c->dmu, c->cphi, c->cmu, dt, c->part);
    if (guess)
        LAUNCHC(PC_GUESS, k_guess, c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, c->gtab2, (const double *)c->D_s, dt,
                c->rhs_s, c->x0g, c->part, 1);
    LAUNCH(LB_T(k_fin_residual, 1), dim3(c->B), dim3(64), c->st, c->part, c->nblk, c->hist_dev, c->P.kappa, dt, c->lin_tol, eta,
           guess ? (int)c->gmask2 : 0, so, NO_FIN_TAIL);
    return 0;
}

// One implicit time level for the whole batch (F2:323-427).  On entry the old level is
// (phi_s, mu_s)[slot], w; on exit the new iterate is in (phi_s, mu_s)[slot] and w_new in c->wnew.
//
// Launch schedule.  The Newton / Armijo / CG state machine runs on the device (TrajState + the fin kernels) and
// every kernel is gated by it, so the host enqueues a whole time step without looking: `spec_slots` slots of
// [linear solve with spec_cgb sweeps, step ceiling, one residual evaluation].  A slot is either a Newton
// iteration or, for a trajectory whose Armijo trial failed, just the next trial (its solve and ceiling kernels
// exit at once); a solve that needs more sweeps than were enqueued is left untouched by the strict ceiling
// kernel and taken up again by the next slot.  The host looks at the state ONCE per step, finishes the rare
// step that did not fit (the loop below, one look per Armijo trial) and sizes the next step's schedule from
// what this one used.  in_march = false (a bare newton_raphson call): the solves go to lin_tol.
static int newton_level(vch2d_ctx *c, double dt, const double *un, const double *unp1, long u_stride,
                        const double *wnew_in, bool in_march) {
    const double eta_ = in_march ? c->lin_eta : 0.0;
    const bool spectral = c->use_fft && !c->half_f && !c->half_s;
    const bool fused = in_march && c->fused_on && spectral && !wnew_in;
    const bool inline_dmu = in_march && spectral;
    // the form of every solve is decided on the device, per trajectory (k_fin_residual: plans of at most cheb_max sweeps take
    // the reduction-free form); -1 = the CG form always (bare Newton calls, solves to round-off, GEMM-DCT grids)
    const int cheb_max_ = (in_march && spectral && c->cheb_on && eta_ > 0.0) ? c->cheb_max : -1;
    // VCH_FUSED=2: fused evaluation kernels, but the `fin` step as its own launch (no hand-off inside the launch)
    const bool fin_inside = c->fused_mode == 1;
    // CG-form solves whose diagonal spans more than cg_scale_ratio run on the right-scaled system (cg_weight, vch_kernels2d.h)
    // the shortened chain (vch2d_ctx::mass_early ...): the default path only
    const bool chain = fused && !fin_inside && c->look_spin;
    c->cell_now = chain && c->ceil_cell_on && cheb_max_ >= 0;
    c->trial_enq = -1;
    const bool fin_pub = chain && c->fin_publish;
    const SolveOpts so_{cheb_max_, spectral ? c->cg_scale_ratio : 0.0, in_march ? c->eta1_factor : 0.0,
                        c->cell_now ? c->ceil_cell : (unsigned long long *)nullptr};
    const EvalFin efin_{fin_inside ? c->fin_counter : (unsigned *)nullptr, c->hist_dev, c->P.kappa, c->lin_tol, eta_, so_, -1};
    // starting guesses (marches on the stencil-free path only; forward_core fills the coefficient tables): of the first
    // solve here, of the second solve inside the residual trial of slot 0
    const bool guess = in_march && c->guess_on && c->gmask1 != 0;
    const bool guess2 = in_march && c->guess_on && c->guess2_on && c->gmask2 != 0;
    if (fused) {
        // step start in one launch: old-level terms, Newton start value, initial residual, starting guess (, `fin` step)
        GuessArgs g1_ = c->gtab1;
        if (!guess) memset(g1_.c, 0, sizeof(g1_.c));
        // the previous step's clip / mass fix / history store, if forward_core left it to this kernel
        const PostArgs post_{c->post_pending ? (const double *)c->part_mass : (const double *)nullptr, c->post_hist, hist_stride(c), c->post_rec,
                             (long)c->Mmax * SHIFT_REC};
        c->post_pending = false;
        auto k_start = c->eval_hoist ? (fin_inside ? k_eval<0, true> : k_eval<0, false>)
                                     : (fin_inside ? k_eval_plain<0, true> : k_eval_plain<0, false>);
        LAUNCHC(PC_RESIDUAL0, k_start, c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, c->phi_s, c->mu_s, c->Rphi_s, c->rhs_s,
                c->D_s, (const double *)nullptr, c->cphi, c->cmu, dt, c->part, (const double *)c->w, un, unp1, u_stride, c->wnew, g1_,
                c->x0g, efin_, post_);
        if (!fin_inside)
            LAUNCH(LB_T(k_fin_residual, 2), dim3(c->B), dim3(64), c->st, c->part, c->nblk, c->hist_dev, c->P.kappa, dt, c->lin_tol, eta_,
                   guess ? (int)c->gmask1 : 0, so_, NO_FIN_TAIL);
    } else {
        LAUNCH(k_prepare, c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, c->phi_s, c->mu_s, c->w, un, unp1, u_stride,
               wnew_in, dt, c->wnew, c->mu0, c->cphi, c->cmu);
        LAUNCHC(PC_RESIDUAL0, (k_residual<0>), c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, c->phi_s, c->mu_s, c->Rphi_s, c->rhs_s,
               c->D_s, c->mu0, c->x, c->dmu, c->cphi, c->cmu, dt, c->part);
        if (guess)
            LAUNCHC(PC_GUESS, k_guess, c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, c->gtab1, (const double *)c->D_s, dt, c->rhs_s,
                   c->x0g, c->part, 0);
        LAUNCH(LB_T(k_fin_residual, 0), dim3(c->B), dim3(64), c->st, c->part, c->nblk, c->hist_dev, c->P.kappa, dt, c->lin_tol, eta_,
               guess ? (int)c->gmask1 : 0, so_, NO_FIN_TAIL);
    }
    if (c->spec) {
        for (int s = 0; s < c->spec_slots; ++s) {
            // the launch sequences of the forms the trajectories took in this slot of the previous step (both where they
            // differed; a trajectory whose form has no sequence here is finished by the loop below)
            if (cheb_max_ >= 0 && (c->spec_form[s] & 1)) VCHCHK(cheb_solve(c, dt, c->spec_chn[s]));
            if (cheb_max_ < 0 || (c->spec_form[s] & 2)) VCHCHK(schur_solve(c, dt, c->spec_cgb[s], false));
            VCHCHK(dmu_ceiling(c, 1));
            // the second solve's guess goes with the trial that follows a trajectory's FIRST solve (the kernels check
            // iters == 1), in whichever slot that solve finished: the result must not depend on the launch schedule
            VCHCHK(residual_trial(c, dt, inline_dmu, fused, fin_inside, guess2, eta_, so_, efin_,
                                  fin_pub && s == c->spec_slots - 1));
        }
    }
    // the step's weighted mass (F2:565) in front of the look: it reads the final iterate only, so the host's look, its guess
    // tables and the enqueue of the next step's first kernel overlap it.  A trajectory the schedule did not finish is summed
    // behind the continuation loop, by a second launch over all of them (a pure function of the final iterate)
    c->mass_done = chain && c->mass_early;
    if (c->mass_done) LAUNCH(k_mass, c->grid, dim3(NTH), c->G, c->st, c->slot_stride, c->phi_s, c->wts_mass, 1, c->part_mass, 1);
    VCHCHK(sync_state(c, false));
    auto any_active = [&]() {
        for (int b = 0; b < c->B; ++b)
            if (c->st_host[b].newton_active) return true;
        return false;
    };
    auto any_trial = [&]() {
        for (int b = 0; b < c->B; ++b)
            if (c->st_host[b].newton_active && c->st_host[b].need_trial) return true;
        return false;
    };
    if (c->debug_guess) {
        const TrajState &S = c->st_host[0];
        fprintf(stderr, "guess order %d / %d (run %d) | traj 0: ratio %.3e / %.3e solves %d sweeps %d %d %d normR %.3e active %d "
                "tol %.3e %.3e %.3e kT %.6f %.6f %.6f form %d %d %d | norms %d total sweeps %ld newton %ld trials %d lastform %d lastn %d R %.3e %.3e %.3e r0 %.3e\n",
                c->used1[0], c->used2[0], c->run2[0], S.guess_ratio, S.guess_ratio2, S.step_solves, S.step_lin[0],
                S.step_lin[1], S.step_lin[2], S.normR, S.newton_active, S.step_tol[0], S.step_tol[1], S.step_tol[2],
                S.step_kT[0], S.step_kT[1], S.step_kT[2], S.step_form[0], S.step_form[1], S.step_form[2], S.iters, S.lin_total,
                S.newton_total, S.ntrials, S.use_cheb, S.cheb_n, S.step_R[0], S.step_R[1], S.step_R[2], S.lin_r0);
    }
    int guard = 0;
    const bool unfit = any_active();
    while (any_active()) {
        if (++guard > NEWTON_MAXIT + 2) return vch_fail(VCH_ERR_STATE, "newton_level: state machine did not terminate");
        // the pending solves' forms and plans are in the state the host has just read
        int need = -1, budget = 0;
        for (int b = 0; b < c->B; ++b) {
            const TrajState &S = c->st_host[b];
            if (!S.newton_active || !S.lin_active) continue;
            if (S.use_cheb) need = std::max(need, S.cheb_n);
            else budget = std::max(budget, S.lin_budget);
        }
        if (need >= 0) VCHCHK(cheb_solve(c, dt, need));
        if (budget > 0) VCHCHK(schur_solve(c, dt, std::min(budget, c->lin_maxit), true));
        VCHCHK(dmu_ceiling(c, 0));
        int tguard = 0;
        do {
            VCHCHK(residual_trial(c, dt, inline_dmu, fused, fin_inside, guess2, eta_, so_, efin_, fin_pub));
            VCHCHK(sync_state(c, false));
            if (++tguard > ARMIJO_TRIALS + 2) return vch_fail(VCH_ERR_STATE, "newton_level: Armijo loop did not terminate");
        } while (any_trial());
    }
    if (unfit && c->mass_done) LAUNCH(k_mass, c->grid, dim3(NTH), c->G, c->st, c->slot_stride, c->phi_s, c->wts_mass, 1, c->part_mass, 0);
    {
        // next step's schedule: as many slots as the busiest trajectory had linear solves (failed trials do not count: they
        // are rare and the loop above absorbs them); per slot the launch sequences of the forms seen there, CG sweeps for the
        // longest CG solve + 1 within the rigorous bound, Chebyshev sweeps for the longest plan + the margin
        int solves = 1, sweeps[4] = {1, 1, 1, 1}, chn[4] = {0, 0, 0, 0}, form[4] = {0, 0, 0, 0}, longest = 1, bound = 1, chmax = 0,
            form_any = 0;
        for (int b = 0; b < c->B; ++b) {
            const TrajState &S = c->st_host[b];
            if (S.frozen) continue;
            solves = std::max(solves, S.step_solves);
            bound = std::max(bound, S.lin_budget);
            for (int s = 0; s < 4 && s < S.step_solves; ++s) {
                if (S.step_form[s]) {
                    chn[s] = std::max(chn[s], S.step_chn[s]);
                    chmax = std::max(chmax, S.step_chn[s]);
                    form[s] |= 1;
                } else {
                    sweeps[s] = std::max(sweeps[s], S.step_lin[s]);
                    longest = std::max(longest, S.step_lin[s]);
                    form[s] |= 2;
                }
                form_any |= form[s];
            }
        }
        if (!form_any) form_any = cheb_max_ >= 0 ? 1 : 2;
        c->spec_slots = std::min(solves, 4);
        for (int s = 0; s < 4; ++s) {
            const bool seen = s < solves && form[s] != 0;
            c->spec_form[s] = seen ? form[s] : form_any;                    // a slot this step did not use: any form seen
            const int want = ((seen && (form[s] & 2)) ? sweeps[s] : longest) + 1;
            c->spec_cgb[s] = std::max(2, std::min(std::min(want, bound), 64));
            c->spec_chn[s] = ((seen && (form[s] & 1)) ? chn[s] : chmax) + c->cheb_margin;
        }
    }
    return 0;
}

static void fill_stats(vch2d_ctx *c, vch_stats *s, float ms) {
    if (!s) return;
    memset(s, 0, sizeof(*s));
    for (int b = 0; b < c->B; ++b) {
        const TrajState &S = c->st_host[b];
        s->newton_iters += S.newton_total;
        s->linear_solves += S.nsolves;
        s->linear_iters += S.lin_total;
        s->armijo_trials += S.ntrials;
        s->max_lin_relres = std::max(s->max_lin_relres, S.lin_maxrel);
        s->max_lin_absres = std::max(s->max_lin_absres, S.lin_maxabs);
        s->unconverged_solves += S.lin_unconv;
    }
    s->linear_iters += c->redo_iters;          // a repeated adjoint sweep: its first pass counts too
    s->host_syncs += 0;
    s->host_syncs = c->n_sync;
    s->launches = c->n_launch;
    s->seconds = ms * 1e-3;
}

static int reset_counters(vch2d_ctx *c) {
    HIPCHK(hipMemsetAsync(c->st, 0, sizeof(TrajState) * c->B, c->stream));
    c->tot_launch += c->n_launch;
    c->tot_sync += c->n_sync;
    c->n_launch = c->n_sync = 0;
    c->redo_iters = 0;        // the books of a repeated adjoint sweep close with the call that made them (fill_stats)
    return 0;
}

// Trajectories with flags[b] != 0 skip the following marches (their kernels exit at once) until
// the next reset_counters().
static int freeze(vch2d_ctx *c, const std::vector<int> &flags) {
    HIPCHK(hipMemcpyAsync(c->frozen_dev, flags.data(), sizeof(int) * c->B, hipMemcpyHostToDevice, c->stream));
    LAUNCH(k_set_frozen, dim3((c->B + 63) / 64), dim3(64), c->st, (const int *)c->frozen_dev, c->B);
    return 0;
}

// ------------------------------------------------------------------------------------
// operator-level entry points
// ------------------------------------------------------------------------------------
extern "C" int vch2d_apply_laplacian(vch2d_ctx *c, const double *v, double *out) {
    CTXCHK(c);
    ARGCHK(v && out, "NULL array");
    VCHCHK(h2d(c, c->tmp[0], v, c->B));
    LAUNCH(k_lap, c->grid, dim3(NTH), c->G, c->tmp[0], c->tmp[1]);
    return d2h(c, out, c->tmp[1], c->B);
}

extern "C" int vch2d_initialize_mu(vch2d_ctx *c, const double *phi, const double *w, double *mu_out) {
    CTXCHK(c);
    ARGCHK(phi && w && mu_out, "NULL array");
    VCHCHK(h2d(c, c->tmp[0], phi, c->B));
    VCHCHK(h2d(c, c->tmp[1], w, c->B));
    LAUNCH(k_init_mu, c->grid, dim3(NTH), c->G, c->P, c->tmp[0], c->tmp[1], c->tmp[2]);
    return d2h(c, mu_out, c->tmp[2], c->B);
}

extern "C" int vch2d_solve_w(vch2d_ctx *c, const double *w_old, double dt, const double *u_n, const double *u_np1,
                             double *w_out) {
    CTXCHK(c);
    ARGCHK(w_old && w_out && dt > 0, "NULL array or dt <= 0");
    VCHCHK(h2d(c, c->tmp[0], w_old, c->B));
    if (u_n) VCHCHK(h2d(c, c->tmp[1], u_n, c->B));
    if (u_np1) VCHCHK(h2d(c, c->tmp[2], u_np1, c->B));
    LAUNCH(k_solve_w, c->grid, dim3(NTH), c->G, c->tmp[0], u_n ? c->tmp[1] : nullptr, u_np1 ? c->tmp[2] : nullptr,
           c->P.gamma / dt, c->tmp[3]);
    return d2h(c, w_out, c->tmp[3], c->B);
}

static int read_norms(vch2d_ctx *c, int slot, double *norm_out) {
    // sums partial slot `slot` per trajectory on the host (test helper path)
    std::vector<double> hp((size_t)c->B * c->nblk * NPART);
    HIPCHK(hipMemcpyAsync(hp.data(), c->part, hp.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < c->B; ++b) {
        double s = 0.0;
        for (int t = 0; t < c->nblk; ++t) s += hp[((size_t)b * c->nblk + t) * NPART + slot];
        norm_out[b] = std::sqrt(s);
    }
    return 0;
}

extern "C" int vch2d_residuals(vch2d_ctx *c, const double *pn, const double *po, const double *mn, const double *mo,
                               const double *wn, const double *wo, double dt, double *Rp, double *Rm, double *norm_out) {
    CTXCHK(c);
    ARGCHK(pn && po && mn && mo && wn && wo && Rp && Rm && dt > 0, "NULL array or dt <= 0");
    const double *src[6] = {pn, po, mn, mo, wn, wo};
    for (int k = 0; k < 6; ++k) VCHCHK(h2d(c, c->tmp[k], src[k], c->B));
    LAUNCH(k_residual_plain, c->grid, dim3(NTH), c->G, c->P, c->tmp[0], c->tmp[1], c->tmp[2], c->tmp[3], c->tmp[4],
           c->tmp[5], dt, c->t1, c->t2, c->part);
    VCHCHK(d2h(c, Rp, c->t1, c->B));
    VCHCHK(d2h(c, Rm, c->t2, c->B));
    if (norm_out) VCHCHK(read_norms(c, 0, norm_out));
    return 0;
}

extern "C" int vch2d_jacobian_apply(vch2d_ctx *c, const double *phi_new, double dt, const double *dphi, const double *dmu,
                                    double *out_phi, double *out_mu) {
    CTXCHK(c);
    ARGCHK(phi_new && dphi && dmu && out_phi && out_mu && dt > 0, "NULL array or dt <= 0");
    VCHCHK(h2d(c, c->tmp[0], phi_new, c->B));
    VCHCHK(h2d(c, c->tmp[1], dphi, c->B));
    VCHCHK(h2d(c, c->tmp[2], dmu, c->B));
    LAUNCH(k_jac_apply, c->grid, dim3(NTH), c->G, c->P, c->tmp[0], c->tmp[1], c->tmp[2], dt, c->tmp[3], c->tmp[4]);
    VCHCHK(d2h(c, out_phi, c->tmp[3], c->B));
    return d2h(c, out_mu, c->tmp[4], c->B);
}

extern "C" int vch2d_schur_apply(vch2d_ctx *c, const double *phi_new, double dt, const double *x, double *out) {
    CTXCHK(c);
    ARGCHK(phi_new && x && out && dt > 0, "NULL array or dt <= 0");
    VCHCHK(reset_counters(c));
    VCHCHK(h2d(c, c->tmp[0], phi_new, c->B));
    VCHCHK(h2d(c, c->tmp[1], x, c->B));
    // D into slot 0 through the solve set-up kernel (a = b = x, results other than D unused)
    LAUNCH(k_solve_setup, c->grid, dim3(NTH), c->G, c->P, c->tmp[1], c->tmp[1], c->tmp[0], dt, c->Rphi_s, c->rhs_s, c->D_s,
           c->part);
    LAUNCH(k_schur, c->grid, dim3(NTH), c->G, c->P, (const TrajState *)nullptr, c->slot_stride, c->tmp[1], c->D_s, dt, c->tmp[2]);
    return d2h(c, out, c->tmp[2], c->B);
}

extern "C" int vch2d_spectral_solve(vch2d_ctx *c, double c0, double c1, double c2, const double *v, double *out) {
    CTXCHK(c);
    ARGCHK(v && out, "NULL array");
    VCHCHK(h2d(c, c->tmp[0], v, c->B));
    VCHCHK(precond(c, c->tmp[0], 0, c->tmp[1], 0, nullptr, c0, c1, 0.0, c2, 0));
    return d2h(c, out, c->tmp[1], c->B);
}

extern "C" int vch2d_jacobian_solve(vch2d_ctx *c, const double *phi_new, double dt, const double *rhs_phi,
                                    const double *rhs_mu, double *dphi, double *dmu, vch_stats *stats) {
    CTXCHK(c);
    ARGCHK(phi_new && rhs_phi && rhs_mu && dphi && dmu && dt > 0, "NULL array or dt <= 0");
    VCHCHK(reset_counters(c));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    VCHCHK(h2d(c, c->tmp[0], phi_new, c->B));
    VCHCHK(h2d(c, c->tmp[1], rhs_phi, c->B));
    VCHCHK(h2d(c, c->tmp[2], rhs_mu, c->B));
    // slot 0: phi, R_phi = -a, rhs = b - L a, D
    HIPCHK(hipMemcpyAsync(c->phi_s, c->tmp[0], sizeof(double) * c->B * c->G.plane, hipMemcpyDeviceToDevice, c->stream));
    LAUNCH(k_solve_setup, c->grid, dim3(NTH), c->G, c->P, c->tmp[1], c->tmp[2], c->tmp[0], dt, c->Rphi_s, c->rhs_s, c->D_s,
           c->part);
    LAUNCH(k_fin_lin_begin, dim3(c->B), dim3(64), c->st, c->part, c->nblk, 2, c->P.tau, c->P.kappa, dt, c->lin_tol, 0.0);
    VCHCHK(sync_state(c));
    VCHCHK(schur_solve(c, dt, cg_budget(c, false), true));
    // back substitution needs newton_active && !need_trial
    HIPCHK(hipStreamSynchronize(c->stream));
    {   // keep the device-side linear-solve results, flip only the two flags
        std::vector<TrajState> tmp(c->B);
        HIPCHK(hipMemcpy(tmp.data(), c->st, sizeof(TrajState) * c->B, hipMemcpyDeviceToHost));
        for (auto &S : tmp) { S.newton_active = 1; S.need_trial = 0; }
        HIPCHK(hipMemcpy(c->st, tmp.data(), sizeof(TrajState) * c->B, hipMemcpyHostToDevice));
    }
    VCHCHK(dmu_ceiling(c, 0));
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    VCHCHK(d2h(c, dphi, c->xf, c->B));
    VCHCHK(d2h(c, dmu, c->dmu, c->B));
    VCHCHK(sync_state(c));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    fill_stats(c, stats, ms);
    return 0;
}

// ------------------------------------------------------------------------------------
// adjoint operator / solve
// ------------------------------------------------------------------------------------
// CG for A(phi_n) x = rhs, right-preconditioned, weighted inner product W / (D_n - dbar);
// initial guess = current content of c->x.  Buffers: rhs = c->cphi, D_n = c->cmu, r = c->r.
//
// Power-of-two grids: the stencil-free single-reduction form of vch_fft.h (k_adj_rows_fwd): x = x0 + P^-1 y, three
// launches per sweep.  `look` = the host may look at the state every CG_CHUNK sweeps of a long solve.  A solve that the
// enqueued sweeps do not finish keeps lin_active set; the next k_fin_lin_begin counts it (lin_unconv).
static int adjoint_solve_cg(vch2d_ctx *c, double dt, int budget, bool look) {
    const bool spectral = c->use_fft && !c->half_f && !c->half_s;
    // r = rhs - A x0, <r,r>_Z', ||r||_2
    LAUNCH((k_adj_op<1>), c->grid, dim3(NTH), c->G, c->P, c->st, c->x, c->cmu, c->cphi, dt, c->r, c->part);
    if (spectral) {
        if (budget <= 0) return 0;
        const double cadj = 0.5 * dt;
        double *rb[2] = {c->r, c->cg_z2}, *y = c->cg_v;
        int done = 0;
        while (done < budget) {
            const int chunk = look ? std::min(budget - done, CG_CHUNK) : budget - done;
            for (int j = 0; j < chunk; ++j, ++done) {
                double *pn = c->cg_p[done & 1], *po = c->cg_p[(done + 1) & 1];
                AdjSweepArgs a{done == 0 ? rb[0] : rb[(done + 1) & 1], c->cg_q, po, y, rb[done & 1], pn, c->cmu,
                               c->gpart, c->gpart2, c->gpart3, done, c->lin_maxit, c->B, c->part, c->nblk, c->lin_tol};
                VCHCHK(adj_rows(c, a, done == 0));
                // q = ph + c Delta (M P^-1 ph), <ph,q>_Z', <q,q>_Z'
                const SpecArgs sp{1.0, c->P.tau, cadj, cadj, c->ms, c->mf, pn, c->cmu, 0L, c->gpart, c->gpart2, 1, cadj};
                const int gate = 2 + (done & 1);
                VCHCHK(dct_cols(c, sp, 1.0 / (4.0 * (double)c->fax.N * (double)c->sax.N), gate));
                VCHCHK(dct_rows<5>(c, c->t2, 0L, c->cg_q, sp, gate));
            }
            if (done < budget) {
                LAUNCH(k_cg_publish, dim3((c->B + 63) / 64), dim3(64), c->st, (done - 1) & 1, c->B);
                VCHCHK(sync_state(c, false));
                if (!any_lin_active(c)) break;
            }
        }
        LAUNCH(k_fin_adj_step, dim3(c->B), dim3(192), c->st, (const double *)c->gpart, (const double *)c->gpart2,
               (const double *)(c->gpart3 + (size_t)((done - 1) & 1) * c->B * c->gnblk * 2), c->gnblk, done - 1 >= 1 ? 1 : 0,
               (done - 1) & 1, (done - 1) & 1, c->lin_maxit);
        LAUNCHC(PC_CG_UPDATE, k_cg_finish, c->grid, dim3(NTH), c->G, c->st, c->cg_p[0], c->cg_p[1], y);       // pending y += alpha ph
        // x = x0 + P^-1 y for the trajectories whose solve took place
        VCHCHK(precond(c, y, 0, c->x, 4, c->x, 1.0, c->P.tau, cadj, cadj, 4));
        return 0;
    }
    double *ph = c->cg_p[0], *pv = c->cg_p[1], *q = c->cg_q;
    LAUNCH(k_fin_cg_beta, dim3(c->B), dim3(64), c->st, c->part, c->nblk, 1, c->lin_tol, c->lin_maxit, 1);
    int done = 0;
    while (done < budget) {
        const int chunk = std::min(budget - done, CG_CHUNK);
        for (int j = 0; j < chunk; ++j, ++done) {
            if (done == 0) LAUNCH((k_cg_dir<1>), c->grid, dim3(NTH), c->G, c->st, c->r, ph);
            else LAUNCH((k_cg_dir<0>), c->grid, dim3(NTH), c->G, c->st, c->r, ph);
            VCHCHK(precond(c, ph, 0, pv, 0, nullptr, 1.0, c->P.tau, 0.5 * dt, 0.5 * dt, 1));
            LAUNCHC(PC_ADJ_Q, k_adj_q, c->grid, dim3(NTH), c->G, c->P, c->st, pv, c->cmu, ph, dt, q, c->part);
            LAUNCH(k_fin_cg_alpha, dim3(c->B), dim3(64), c->st, c->part, c->nblk, NPART, 0);
            LAUNCHC(PC_CG_UPDATE, k_cg_update_adj, c->grid, dim3(NTH), c->G, c->st, pv, q, c->cmu, c->x, c->r, c->part);
            LAUNCH(k_fin_cg_beta, dim3(c->B), dim3(64), c->st, c->part, c->nblk, 1, c->lin_tol, c->lin_maxit, 0);
        }
        if (done < budget && look) {
            VCHCHK(sync_state(c, false));
            if (!any_lin_active(c)) break;
        }
    }
    return 0;
}

extern "C" int vch2d_adjoint_apply(vch2d_ctx *c, int which, const double *phi, double dt, const double *v, double *out) {
    CTXCHK(c);
    ARGCHK(phi && v && out && (which == 0 || which == 1), "NULL array or which not in {0,1}");
    VCHCHK(h2d(c, c->tmp[0], phi, c->B));
    VCHCHK(h2d(c, c->tmp[1], v, c->B));
    LAUNCH(k_adj_setup, c->grid, dim3(NTH), c->G, c->P, c->tmp[0], (const double *)nullptr, c->cmu, c->part);
    if (which == 0)
        LAUNCH((k_adj_op<0>), c->grid, dim3(NTH), c->G, c->P, c->st, c->tmp[1], c->cmu, c->cphi, dt, c->tmp[2], c->part);
    else
        LAUNCH((k_adj_op<2>), c->grid, dim3(NTH), c->G, c->P, c->st, c->tmp[1], c->cmu, c->cphi, dt, c->tmp[2], c->part);
    return d2h(c, out, c->tmp[2], c->B);
}

extern "C" int vch2d_adjoint_solve(vch2d_ctx *c, const double *phi_n, double dt, const double *rhs, double *p_out,
                                   vch_stats *stats) {
    CTXCHK(c);
    ARGCHK(rhs && p_out && dt >= 0 && (phi_n || dt == 0), "NULL array or dt < 0");
    VCHCHK(reset_counters(c));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    if (phi_n) VCHCHK(h2d(c, c->tmp[0], phi_n, c->B));
    VCHCHK(h2d(c, c->cphi, rhs, c->B));
    LAUNCH(k_adj_setup, c->grid, dim3(NTH), c->G, c->P, (dt > 0 ? c->tmp[0] : (const double *)nullptr), c->cphi, c->cmu,
           c->part);
    LAUNCH(k_fin_lin_begin, dim3(c->B), dim3(64), c->st, c->part, c->nblk, 0, c->P.tau, c->P.kappa, dt, c->lin_tol, 0.0);
    LAUNCH(k_fill, c->grid, dim3(NTH), c->G, c->x, 0.0);
    VCHCHK(sync_state(c));
    VCHCHK(adjoint_solve_cg(c, dt, cg_budget(c, false), true));
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    VCHCHK(d2h(c, p_out, c->x, c->B));
    VCHCHK(sync_state(c));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    fill_stats(c, stats, ms);
    return 0;
}

// ------------------------------------------------------------------------------------
// Newton call and forward march
// ------------------------------------------------------------------------------------
extern "C" int vch2d_newton_raphson(vch2d_ctx *c, const double *phi_old, const double *mu_old, const double *w_old,
                                    const double *w_new, double dt, double *phi_new, double *mu_new, double *hist,
                                    int hist_cap, int32_t *n_hist, vch_stats *stats) {
    CTXCHK(c);
    ARGCHK(phi_old && mu_old && w_old && w_new && phi_new && mu_new && dt > 0, "NULL array or dt <= 0");
    VCHCHK(reset_counters(c));
    VCHCHK(h2d(c, c->phi_s, phi_old, c->B));
    VCHCHK(h2d(c, c->mu_s, mu_old, c->B));
    VCHCHK(h2d(c, c->w, w_old, c->B));
    VCHCHK(h2d(c, c->tmp[0], w_new, c->B));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    VCHCHK(newton_level(c, dt, nullptr, nullptr, 0, c->tmp[0], false));
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < c->B; ++b) {
        const int slot = c->st_host[b].slot;
        VCHCHK(d2h(c, phi_new + (long)b * c->G.nf * c->G.ns, c->phi_s + slot * c->slot_stride + b * c->G.plane, 1));
        VCHCHK(d2h(c, mu_new + (long)b * c->G.nf * c->G.ns, c->mu_s + slot * c->slot_stride + b * c->G.plane, 1));
    }
    if (hist || n_hist) {
        HIPCHK(hipMemcpy(c->hist_host, c->hist_dev, sizeof(double) * c->B * HIST_CAP, hipMemcpyDeviceToHost));
        for (int b = 0; b < c->B; ++b) {
            int n = std::min(c->st_host[b].iters, HIST_CAP);
            if (n_hist) n_hist[b] = n;
            if (hist)
                for (int k = 0; k < std::min(n, hist_cap); ++k) hist[(long)b * hist_cap + k] = c->hist_host[(long)b * HIST_CAP + k];
        }
    }
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    fill_stats(c, stats, ms);
    return 0;
}

// March M steps from the state in phi_s[slot 0] (already uploaded), control in u_dev
// ([B][Mmax+1][plane], u_rows valid rows) or NULL; history into hist_dev_out.
static int forward_core(vch2d_ctx *c, const double *u_dev, int u_rows, const double *dt, int M, double *hist_out) {
    const long hs = hist_stride(c);
    // slot 0 holds phi0; w = 0; mu = initialize_mu(phi0, 0) (F2:518-520); mass0 (F2:532)
    HIPCHK(hipMemsetAsync(c->w, 0, sizeof(double) * c->B * c->G.plane, c->stream));
    LAUNCH(k_init_mu, c->grid, dim3(NTH), c->G, c->P, c->phi_s, c->w, c->mu_s);
    LAUNCH(k_mass, c->grid, dim3(NTH), c->G, c->st, c->slot_stride, c->phi_s, c->wts_mass, 0, c->part, 0);
    LAUNCH(k_fin_mass, dim3(c->B), dim3(64), c->st, c->part, c->nblk, 1);
    c->post_pending = false;
    // the shift record goes beside the history the march writes
    double *const rec_out = hist_out && hist_out == c->phi_hist ? c->shift_hist
                          : hist_out && hist_out == c->phi_trial ? c->shift_trial : (double *)nullptr;
    const long rec_stride = (long)c->Mmax * SHIFT_REC;
    // marches whose steps start with k_eval<0> (newton_level: the fused path) leave the end of every step but the last to it
    const bool fold_post = c->post_fold && c->fused_on && c->use_fft && !c->half_f && !c->half_s;
    if (hist_out) LAUNCH(k_copy_plane, c->grid, dim3(NTH), c->G, c->phi_s, c->G.plane, hist_out, hs);
    const bool per_traj = c->B <= GUESS_BMAX;
    for (auto &q : c->pol1) q.reset();
    for (auto &q : c->pol2) q.reset();
    std::fill(c->run2.begin(), c->run2.end(), 0);
    c->pol1_all.reset();
    c->pol2_all.reset();
    c->run2_all = 0;
    for (int &f : c->spec_form) f = 3;      // the first step of a march has nothing to go by: both launch sequences
    for (int step = 0; step < M; ++step) {
        const double *un = nullptr, *unp1 = nullptr;
        if (u_dev && step < u_rows - 1) {        // F2:545-548
            un = u_dev + (long)step * c->G.plane;
            unp1 = u_dev + (long)(step + 1) * c->G.plane;
        }
        // guess for the step's first Newton solve: the increment rate d_k / dt_k, taken at the step midpoints, is
        // extrapolated to this step's midpoint by the polynomial through the last `order` steps; this step's increment
        // replaces the oldest one in the ring.  The order is every trajectory's own (its policy sees its own ratios only).
        memset(c->gtab1.c, 0, sizeof(c->gtab1.c));
        memset(c->gtab2.c, 0, sizeof(c->gtab2.c));
        c->gtab1.per_traj = c->gtab2.per_traj = per_traj ? 1 : 0;
        c->gmask1 = c->gmask2 = 0;
        c->guess_wr = -1;
        c->guess_step = step;
        if (c->guess_on) {
            c->guess_wr = step & (GUESS_RING - 1);
            for (int j = 0; j < GUESS_ORD; ++j) {
                c->gtab1.d[j] = c->dprev[(step - 1 - j) & (GUESS_RING - 1)];
                c->gtab2.d[j] = c->dprev2[(step - 1 - j) & (GUESS_RING - 1)];
            }
            // returns the order actually used: on ragged time grids the weights of a high order can grow large, and a guess
            // of large magnitude costs accuracy when the solve cancels it again (x = x0 + y); the weights of order 6 on a
            // uniform grid sum to 63 in magnitude, anything above is answered with a lower order
            auto weights = [&](int m, double *cf) -> int {
                for (; m >= 1; --m) {
                    double mid[GUESS_ORD + 1];                // midpoints of steps n, n-1, .. n-m relative to the start of step n
                    mid[0] = 0.5 * dt[step];
                    double t0 = 0.0, mag = 0.0;
                    for (int j = 1; j <= m; ++j) {
                        t0 -= dt[step - j];
                        mid[j] = t0 + 0.5 * dt[step - j];
                    }
                    for (int j = 0; j < GUESS_ORD; ++j) cf[j] = 0.0;
                    for (int j = 1; j <= m; ++j) {   // Lagrange weight of node j at mid[0]
                        double w = 1.0;
                        for (int k = 1; k <= m; ++k)
                            if (k != j) w *= (mid[0] - mid[k]) / (mid[j] - mid[k]);
                        cf[j - 1] = w * dt[step] / dt[step - j];
                        mag += std::fabs(cf[j - 1]);
                    }
                    if (std::isfinite(mag) && mag <= 64.0) return m;
                }
                for (int j = 0; j < GUESS_ORD; ++j) cf[j] = 0.0;
                return 0;
            };
            if (per_traj) {
                for (int b = 0; b < c->B; ++b) {
                    c->used1[b] = weights(c->pol1[b].choose(step, c->guess_max), c->gtab1.c[b]);
                    c->used2[b] = weights(c->guess2_on ? c->pol2[b].choose(std::min(step, c->run2[b]), c->guess_max) : 0, c->gtab2.c[b]);
                    if (c->used1[b] >= 1) c->gmask1 |= 1u << b;
                    if (c->used2[b] >= 1) c->gmask2 |= 1u << b;
                }
            } else {
                const int u1 = weights(c->pol1_all.choose(step, c->guess_max), c->gtab1.c[0]);
                const int u2 = weights(c->guess2_on ? c->pol2_all.choose(std::min(step, c->run2_all), c->guess_max) : 0, c->gtab2.c[0]);
                std::fill(c->used1.begin(), c->used1.end(), u1);
                std::fill(c->used2.begin(), c->used2.end(), u2);
                c->gmask1 = u1 >= 1 ? ~0u : 0u;
                c->gmask2 = u2 >= 1 ? ~0u : 0u;
            }
        }
        VCHCHK(newton_level(c, dt[step], un, unp1, hs, nullptr, true));
        // clip, mass fix, store (F2:562-585); the mass sums may be on their way already (newton_level)
        if (!c->mass_done) LAUNCH(k_mass, c->grid, dim3(NTH), c->G, c->st, c->slot_stride, c->phi_s, c->wts_mass, 1, c->part_mass, 0);
        c->mass_done = false;
        double *const lvl = hist_out ? hist_out + (long)(step + 1) * c->G.plane : (double *)nullptr;
        double *const rec = rec_out ? rec_out + (long)step * SHIFT_REC : (double *)nullptr;
        if (fold_post && step + 1 < M) {
            c->post_pending = true;
            c->post_hist = lvl;
            c->post_rec = rec;
        } else {
            LAUNCH(k_post, c->grid, dim3(NTH), c->G, c->P, c->st, c->slot_stride, c->phi_s, lvl, hs, (const double *)c->part_mass,
                   rec, rec_stride);
        }
        std::swap(c->w, c->wnew);
        if (c->guess_on) {
            // what each guess achieved decides the order of that trajectory's next one (GuessPolicy); the second solves' ring
            // is usable while the trajectory takes a second solve step after step
            auto fin = [](double r) { return std::isfinite(r) ? r : 1e300; };
            if (per_traj) {
                for (int b = 0; b < c->B; ++b) {
                    const TrajState &S = c->st_host[b];
                    if (S.frozen) continue;
                    if (c->used1[b] >= 1 && S.step_solves >= 1) c->pol1[b].report(fin(S.guess_ratio), c->used1[b], c->guess_max);
                    if (!c->guess2_on) continue;
                    if (S.step_solves >= 2) {
                        c->run2[b]++;
                        if (c->used2[b] >= 1) c->pol2[b].report(fin(S.guess_ratio2), c->used2[b], c->guess_max);
                    } else {
                        c->run2[b] = 0;
                        c->pol2[b].reset();
                    }
                }
            } else {
                double worst = 0.0, worst2 = 0.0;
                bool any = false, anyb = false, all2 = true;
                for (int b = 0; b < c->B; ++b) {
                    const TrajState &S = c->st_host[b];
                    if (S.frozen) continue;
                    anyb = true;
                    if (S.step_solves >= 1) { any = true; worst = std::max(worst, fin(S.guess_ratio)); }
                    if (S.step_solves < 2) all2 = false;
                    worst2 = std::max(worst2, fin(S.guess_ratio2));
                }
                if (any && c->used1[0] >= 1) c->pol1_all.report(worst, c->used1[0], c->guess_max);
                if (c->guess2_on) {
                    if (anyb && all2) {
                        c->run2_all++;
                        if (c->used2[0] >= 1) c->pol2_all.report(worst2, c->used2[0], c->guess_max);
                    } else {
                        c->run2_all = 0;
                        c->pol2_all.reset();
                    }
                }
            }
        }
    }
    memset(c->gtab1.c, 0, sizeof(c->gtab1.c));
    memset(c->gtab2.c, 0, sizeof(c->gtab2.c));
    c->gmask1 = c->gmask2 = 0;
    c->guess_wr = -1;
    return 0;
}

extern "C" int vch2d_forward(vch2d_ctx *c, const double *phi0, const double *u, int u_rows, const double *dt, int M,
                             double *phi_hist_out, vch_stats *stats) {
    CTXCHK(c);
    ARGCHK(phi0 && dt && M >= 1 && M <= c->Mmax, "NULL array or M out of range (1..max_steps)");
    for (int k = 0; k < M; ++k) ARGCHK(dt[k] > 0, "dt must be positive");
    VCHCHK(ensure_hist(c, &c->phi_hist));
    const double *u_dev = nullptr;
    if (u == VCH_RESIDENT) {
        ARGCHK(c->u_hist && c->u_rows_res > 0, "no resident control");
        u_dev = c->u_hist;
        u_rows = c->u_rows_res;
    } else if (u) {
        ARGCHK(u_rows >= 1 && u_rows <= c->Mmax + 1, "control rows out of range (1..max_steps+1)");
        VCHCHK(ensure_hist(c, &c->u_hist));
        VCHCHK(h2d_hist(c, c->u_hist, u, u_rows));
        c->u_rows_res = u_rows;
        u_dev = c->u_hist;
    }
    VCHCHK(reset_counters(c));
    VCHCHK(h2d(c, c->phi_s, phi0, c->B));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    VCHCHK(forward_core(c, u_dev, u_rows, dt, M, c->phi_hist));
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    VCHCHK(sync_state(c));
    c->M_res = M;
    c->res_pgd = false;
    c->shift_res = true;
    c->fwd_u_rows = u_dev ? u_rows : 0;
    if (phi_hist_out) VCHCHK(d2h_hist(c, phi_hist_out, c->phi_hist, M + 1));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    fill_stats(c, stats, ms);
    return 0;
}

// Fill a device parameter table from n_o (1 or B) host parameter sets: an ordinary host-to-device copy on the engine's stream.
static int write_opt_tab(vch2d_ctx *c, double *tab_dev, const vch_opt_params *o, int n_o) {
    c->tab_host.assign((size_t)OPT_STRIDE * c->B, 0.0);
    for (int b = 0; b < c->B; ++b) {
        const vch_opt_params &s = o[n_o == 1 ? 0 : b];
        double *t = c->tab_host.data() + (size_t)OPT_STRIDE * b;
        t[OPT_B1] = s.b1; t[OPT_B2] = s.b2; t[OPT_B3] = s.b3;
        t[OPT_KS] = s.kappa_sparsity; t[OPT_UMIN] = s.u_min; t[OPT_UMAX] = s.u_max;
    }
    HIPCHK(hipMemcpyAsync(tab_dev, c->tab_host.data(), sizeof(double) * OPT_STRIDE * c->B, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// ------------------------------------------------------------------------------------
// adjoint sweep (B2:75-246)
// ------------------------------------------------------------------------------------
// phi history in phi_hist_dev ([B][Mmax+1][plane]); targets phiQ_dev (same layout) or NULL, phiT_dev [B][plane] or NULL.
// Launch schedule: the sweeps a solve needs change slowly along the sweep (the start p_{n+1} is a good guess), so the
// host looks at the device state only every ADJ_LOOK steps and enqueues (longest solve so far) + 1 sweeps per step, within
// the rigorous bound; solves are gated per trajectory, and one that its sweeps did not finish is counted on the device
// (lin_unconv).  In a batch of at most GUESS_BMAX every trajectory has a sweep cap of its own -- its own longest solve since
// the last look + 1 (+ 2 at a look that changed its own guess order), within its own bound -- written into its record at
// the look (k_adj_caps); its solves stop there, and the host enqueues the largest cap of the batch: the sweeps a
// trajectory's solve gets are those of its single run (vch.h, vch2d_create).  Larger batches share one count, from the
// longest solve of the batch.  safe = true: a look and the rigorous budget at every step (the fallback of backward_core).
constexpr int ADJ_LOOK = 8, ADJ_SETTLE = 16;
// opt_tab: the device table whose rows give every trajectory its b1 (adjoint source) and b2 (terminal condition).
static int backward_pass(vch2d_ctx *c, const double *phi_hist_dev, int M, const double *t_hist, const double *opt_tab,
                         const double *phiQ_dev, const double *phiT_dev, double *r_out, double *p_out, double *q_out, bool safe) {
    const long hs = hist_stride(c);
    const Geom &G = c->G;
    double *rhs = c->cphi, *Dn = c->cmu, *rcur = c->wnew;
    double *qa = c->mu0, *qb = c->dmu;
    // no sweep caps from an earlier sweep: the terminal solve, the first solve and the safe schedule run without
    LAUNCH(k_adj_caps, dim3(c->B), dim3(64), c->st, AdjCaps{}, 0);
    // terminal condition (B2:183-187): (I - tau L) p_M = b2 (phi_M - phi_T), q_M = -L p_M, r_M = 0
    LAUNCH(k_scaled_diff, c->grid, dim3(NTH), G, phi_hist_dev + (long)M * G.plane, hs, phiT_dev, G.plane, opt_tab + OPT_B2, OPT_STRIDE, rhs,
           c->part);
    LAUNCH(k_adj_setup, c->grid, dim3(NTH), G, c->P, (const double *)nullptr, (const double *)rhs, Dn, c->part);
    LAUNCH(k_fin_lin_begin, dim3(c->B), dim3(64), c->st, c->part, c->nblk, 0, c->P.tau, c->P.kappa, 0.0, c->lin_tol, 0.0);
    LAUNCH(k_fill, c->grid, dim3(NTH), G, c->x, 0.0);
    VCHCHK(adjoint_solve_cg(c, 0.0, 3, false));
    int sweeps = -1, steps_since_look = 0;
    bool first_solve = true;
    // starting guess of the solve for p_n (k_adj_guess; the forward ring dprev is free during the sweep): polynomial
    // extrapolation in time over the levels n+2, n+4, .. n+2*order already solved.  order grows by one per look while the
    // guess keeps paying, and the looks come every step until it has settled
    const bool guess = c->guess_on && !safe && !c->adj_guess_off;
    // the order is every trajectory's own (raised / lowered on its own ratios); batches beyond GUESS_BMAX share entry 0
    const bool per_traj = c->B <= GUESS_BMAX;
    std::vector<int> order(per_traj ? c->B : 1, 1);
    int kept = 0;
    LAUNCH(LB(k_adj_finish), c->grid, dim3(NTH), G, c->x, (const double *)nullptr, qa, rcur, 0.0, 0.0,
           r_out ? r_out + (long)M * G.plane : (double *)nullptr, p_out ? p_out + (long)M * G.plane : (double *)nullptr,
           q_out ? q_out + (long)M * G.plane : (double *)nullptr, hs);
    for (int n = M - 1; n >= 0; --n) {
        const double dtn = t_hist[n + 1] - t_hist[n];
        double *rl = r_out ? r_out + (long)n * G.plane : nullptr;
        double *pl = p_out ? p_out + (long)n * G.plane : nullptr;
        double *ql = q_out ? q_out + (long)n * G.plane : nullptr;
        if (dtn <= 1e-14) {       // B2:214-216: copy level n+1
            if (rl) LAUNCH(k_copy_plane, c->grid, dim3(NTH), G, r_out + (long)(n + 1) * G.plane, hs, rl, hs);
            if (pl) LAUNCH(k_copy_plane, c->grid, dim3(NTH), G, p_out + (long)(n + 1) * G.plane, hs, pl, hs);
            if (ql) LAUNCH(k_copy_plane, c->grid, dim3(NTH), G, q_out + (long)(n + 1) * G.plane, hs, ql, hs);
            kept = 0;                 // the ring would miss this level: start it again
            continue;
        }
        LAUNCHC(PC_ADJ_RHS, k_adj_rhs, c->grid, dim3(NTH), G, c->P, c->x, qa, phi_hist_dev + (long)n * G.plane,
               phi_hist_dev + (long)(n + 1) * G.plane, phiQ_dev ? phiQ_dev + (long)n * G.plane : (const double *)nullptr,
               phiQ_dev ? phiQ_dev + (long)(n + 1) * G.plane : (const double *)nullptr, hs, dtn, opt_tab, rhs, Dn, c->part);
        LAUNCH(k_fin_lin_begin, dim3(c->B), dim3(64), c->st, c->part, c->nblk, 0, c->P.tau, c->P.kappa, dtn, c->lin_tol, 0.0);
        // looks at levels fixed in advance (every level for the first ADJ_SETTLE ones, where the orders of the guesses are
        // being raised, then every ADJ_LOOK-th): when a trajectory's order changes depends on its own ratios only
        if (safe || steps_since_look >= ((guess && M - 1 - n < ADJ_SETTLE) ? 1 : ADJ_LOOK) || sweeps < 0) {
            VCHCHK(sync_state(c, false));
            steps_since_look = 0;
            int longest = 0;
            for (int b = 0; b < c->B; ++b) longest = std::max(longest, c->st_host[b].step_lin_max);
            const int bound = cg_budget(c, false);
            int margin = 1;
            std::vector<char> moved(order.size(), 0);         // trajectories whose guess order this look changed
            if (guess && !first_solve) {
                // the state shows the solve of the previous level, started from a guess of the trajectory's current order
                bool changed = false;
                auto adapt = [&](int &ord, double ratio) {
                    const int before = ord;
                    if (ratio < 0.25) ord = std::min(ord + 1, GUESS_ORD / 2);
                    else if (ratio > 0.7) ord = std::max(ord - 1, 1);
                    changed |= ord != before;
                    return ord != before;
                };
                auto fin = [](double r) { return std::isfinite(r) ? r : 1e300; };
                if (per_traj) {
                    for (int b = 0; b < c->B; ++b) moved[b] = adapt(order[b], fin(c->st_host[b].guess_ratio));
                } else {
                    double worst = 0.0;
                    for (int b = 0; b < c->B; ++b) worst = std::max(worst, fin(c->st_host[b].guess_ratio));
                    adapt(order[0], worst);
                }
                if (changed) margin = 2;
                if (c->debug_guess)
                    fprintf(stderr, "adjoint level %d: order (traj 0) %d ratio %.3e longest %d\n", n, order[0],
                            c->st_host[0].guess_ratio, longest);
                if (!per_traj) LAUNCH(k_reset_longest, dim3((c->B + 63) / 64), dim3(64), c->st, c->B);     // longest = since this look
            }
            if (safe || first_solve) {
                sweeps = bound;       // the first solve of the sweep has nothing to go by: rigorous bound, with looks
            } else if (per_traj) {
                // every trajectory's cap from its own record; the host enqueues the largest
                AdjCaps caps{};
                sweeps = 2;
                for (int b = 0; b < c->B; ++b) {
                    const TrajState &S = c->st_host[b];
                    const int own = S.lin_active ? std::min(S.lin_budget, c->lin_maxit) : 0;
                    caps.cap[b] = std::max(2, std::min(S.step_lin_max + (moved[b] ? 2 : 1), own));
                    sweeps = std::max(sweeps, caps.cap[b]);
                }
                LAUNCH(k_adj_caps, dim3(c->B), dim3(64), c->st, caps, guess ? 1 : 0);      // reset: longest = since this look
            } else {
                sweeps = std::max(2, std::min(longest + margin, bound));
            }
        }
        ++steps_since_look;
        if (guess) {
            // c->x = p_{n+1} goes into the ring (slot kept mod GUESS_RING); level n+1+j was kept j saves ago.  The guess is
            // the polynomial through the levels n+2k, k = 1..m, at t_n; nothing kept yet: p_{n+1} as it stands
            GuessArgs ga;
            memset(ga.c, 0, sizeof(ga.c));
            ga.per_traj = per_traj ? 1 : 0;
            for (int j = 0; j < GUESS_ORD; ++j) ga.d[j] = c->dprev[(kept - j) & (GUESS_RING - 1)];
            for (size_t b = 0; b < order.size(); ++b) {
                double *cf = ga.c[b];
                int mu = std::min(order[b], (kept + 1) / 2);
                for (; mu >= 1; --mu) {                      // weights of large magnitude (ragged time grids): a lower order
                    double mag = 0.0;
                    for (int j = 0; j < GUESS_ORD; ++j) cf[j] = 0.0;
                    for (int j = 1; j <= mu; ++j) {
                        double w = 1.0;
                        for (int k = 1; k <= mu; ++k)
                            if (k != j) w *= (t_hist[n] - t_hist[n + 2 * k]) / (t_hist[n + 2 * j] - t_hist[n + 2 * k]);
                        cf[2 * j - 1] = w;
                        mag += std::fabs(w);
                    }
                    if (std::isfinite(mag) && mag <= 64.0) break;
                }
                if (mu == 0) {
                    for (int j = 0; j < GUESS_ORD; ++j) cf[j] = 0.0;
                    cf[0] = 1.0;                             // p_{n+1} as it stands
                }
            }
            LAUNCHC(PC_ADJ_GUESS, LB(k_adj_guess), c->grid, dim3(NTH), G, c->x, ga, c->dprev[kept & (GUESS_RING - 1)]);
            ++kept;
        }
        VCHCHK(adjoint_solve_cg(c, dtn, sweeps, safe || first_solve));
        if (first_solve) { sweeps = -1; first_solve = false; }       // look again right after it
        const double den = c->P.gamma + 0.5 * dtn;
        LAUNCH(LB(k_adj_finish), c->grid, dim3(NTH), G, c->x, qa, qb, rcur, (c->P.gamma - 0.5 * dtn) / den, (0.5 * dtn) / den, rl,
               pl, ql, hs);
        std::swap(qa, qb);
    }
    return 0;
}

static int backward_core(vch2d_ctx *c, const double *phi_hist_dev, int M, const double *t_hist, const double *opt_tab,
                         const double *phiQ_dev, const double *phiT_dev, double *r_out, double *p_out, double *q_out) {
    c->adj_guess_off = getenv("VCH_ADJ_GUESS_OFF") != nullptr;
    c->adj_safe = getenv("VCH_ADJ_SAFE") != nullptr;
    if (c->adj_safe)                  // diagnostics: the fallback schedule (a look and the rigorous budget at every step)
        return backward_pass(c, phi_hist_dev, M, t_hist, opt_tab, phiQ_dev, phiT_dev, r_out, p_out, q_out, true);
    c->redo_iters = 0;
    VCHCHK(backward_pass(c, phi_hist_dev, M, t_hist, opt_tab, phiQ_dev, phiT_dev, r_out, p_out, q_out, false));
    VCHCHK(sync_state(c));
    bool redo = false;
    long iters = 0;
    const double accept = 10.0 * c->lin_tol;
    std::vector<int> keep;                     // trajectories whose first pass stands
    for (int b = 0; b < c->B; ++b) {
        const TrajState &S = c->st_host[b];
        iters += S.lin_total;
        // a solve that ran out of sweeps above the solve tolerance's class: the schedule was too short somewhere
        if ((S.lin_unconv > 0 && S.lin_maxrel > accept) || ((S.lin_active || S.lin_capped) && S.lin_rel > accept)) redo = true;
        else keep.push_back(b);
    }
    if (!redo) return 0;
    // The second pass (rigorous budgets, no starting guesses) is for the trajectories whose schedule fell short.  It runs for
    // the whole batch, so the sweeps of the others are set aside and put back afterwards: what a trajectory gets must not
    // depend on its batch mates (vch.h, vch2d_create).  A rare path: the copies cost nothing where it matters.
    double *outs[3] = {r_out, p_out, q_out};
    const size_t blk = (size_t)(M + 1) * c->G.plane;
    const long hs = hist_stride(c);
    size_t nsave = 0;
    for (double *o : outs)
        if (o) nsave += keep.size();
    double *save = nullptr;
    vch_group scope(c->pool);                  // save goes away on every path out
    if (nsave) {
        MEMCHK(c->pool.dev(&save, nsave * blk * sizeof(double)));
        size_t k = 0;
        for (double *o : outs)
            for (size_t i = 0; o && i < keep.size(); ++i, ++k)
                HIPCHK(hipMemcpyAsync(save + k * blk, o + keep[i] * hs, blk * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    const long syncs = c->n_sync, launches = c->n_launch;
    VCHCHK(reset_counters(c));
    VCHCHK(backward_pass(c, phi_hist_dev, M, t_hist, opt_tab, phiQ_dev, phiT_dev, r_out, p_out, q_out, true));
    if (save) {
        size_t k = 0;
        for (double *o : outs)
            for (size_t i = 0; o && i < keep.size(); ++i, ++k)
                HIPCHK(hipMemcpyAsync(o + keep[i] * hs, save + k * blk, blk * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    c->redo_iters = iters;                     // the first pass stays in the books (fill_stats, counters)
    c->n_sync += syncs;
    c->n_launch += launches;
    c->tot_sync -= syncs;
    c->tot_launch -= launches;
    return 0;
}

extern "C" int vch2d_backward(vch2d_ctx *c, const double *phi_hist, int M, const double *t_hist, double hx, double hy,
                              double b1, double b2, const double *phi_Q, const double *phi_T, double *p_out, double *q_out,
                              double *r_out, vch_stats *stats) {
    CTXCHK(c);
    ARGCHK(t_hist && M >= 1 && M <= c->Mmax, "NULL t_hist or M out of range");
    // the reference takes hx, hy from x[1]-x[0], y[1]-y[0] (B2:154-155): must agree with the context's grid
    ARGCHK(std::fabs(hx - c->hx) <= 1e-12 * c->hx && std::fabs(hy - c->hy) <= 1e-12 * c->hy,
           "grid spacing differs from the context's Lx/Nx, Ly/Ny");
    if (phi_hist) {
        VCHCHK(ensure_hist(c, &c->phi_hist));
        VCHCHK(h2d_hist(c, c->phi_hist, phi_hist, M + 1));
        c->M_res = M;
        c->res_pgd = false;
        c->shift_res = false;         // a history of the caller's: no march of this context stands behind it
    } else {
        if (c->M_res != M) return vch_fail(VCH_ERR_STATE, "vch2d_backward: no resident history with %d steps", M);
    }
    const double *pq = nullptr, *pt = nullptr;
    if (phi_Q == VCH_RESIDENT) {
        pq = c->phiQ;
    } else if (phi_Q) {
        VCHCHK(ensure_hist(c, &c->phiQ));
        VCHCHK(h2d_hist(c, c->phiQ, phi_Q, M + 1));
        pq = c->phiQ;
    }
    if (phi_T == VCH_RESIDENT) {
        pt = c->phiT;
    } else if (phi_T) {
        VCHCHK(h2d(c, c->phiT, phi_T, c->B));
        pt = c->phiT;
    }
    VCHCHK(ensure_hist(c, &c->r_hist));
    if (p_out) VCHCHK(ensure_hist(c, &c->p_hist));
    if (q_out) VCHCHK(ensure_hist(c, &c->q_hist));
    VCHCHK(reset_counters(c));
    {
        vch_opt_params o{};
        o.b1 = b1;
        o.b2 = b2;
        VCHCHK(write_opt_tab(c, c->seam_tab, &o, 1));
    }
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    VCHCHK(backward_core(c, c->phi_hist, M, t_hist, c->seam_tab, pq, pt, c->r_hist, p_out ? c->p_hist : nullptr,
                         q_out ? c->q_hist : nullptr));
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    VCHCHK(sync_state(c));
    if (r_out) VCHCHK(d2h_hist(c, r_out, c->r_hist, M + 1));
    if (p_out) VCHCHK(d2h_hist(c, p_out, c->p_hist, M + 1));
    if (q_out) VCHCHK(d2h_hist(c, q_out, c->q_hist, M + 1));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    fill_stats(c, stats, ms);
    return 0;
}

// ------------------------------------------------------------------------------------
// cost (C2:80-108), gradient + prox (C2:150, C2:191-198)
// ------------------------------------------------------------------------------------
// trapezoid weights with np.trapz's arithmetic on the caller's grid: w_i = (d_{i-1} + d_i)/2
static std::vector<double> trapz_w(const double *x, int n) {
    std::vector<double> w(n, 0.0);
    for (int i = 0; i + 1 < n; ++i) {
        double d = x[i + 1] - x[i];
        w[i] += 0.5 * d;
        w[i + 1] += 0.5 * d;
    }
    return w;
}

static int set_cost_weights(vch2d_ctx *c, const double *x, const double *y) {
    const Geom &G = c->G;
    const int nx1 = c->prm.Nx + 1, ny1 = c->prm.Ny + 1;
    std::vector<double> wx = trapz_w(x, nx1), wy = trapz_w(y, ny1), W((size_t)G.plane, 0.0);
    for (int i = 0; i < nx1; ++i)
        for (int j = 0; j < ny1; ++j) {
            long f = (long)i * ny1 + j;
            W[(f / G.nf) * G.pitch + (f % G.nf)] = wx[i] * wy[j];
        }
    HIPCHK(hipMemcpyAsync(c->W_cost, W.data(), W.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// workgroup partials [B][Mmax+1][nblk][4] and level sums [B][Mmax+1][4] (device and pinned) of the cost, the norms, the free
// energy and the prox step's change: all three or none
static int ensure_cost_bufs(vch2d_ctx *c) {
    if (c->cost_part) return 0;
    const size_t lv = (size_t)c->B * (c->Mmax + 1) * 4 * 8;
    vch_group g(c->pool);
    MEMCHK(c->pool.dev(&c->cost_part, lv * c->nblk));
    MEMCHK(c->pool.dev(&c->cost_lvl, lv));
    MEMCHK(c->pool.host(&c->cost_lvl_host, lv));
    return g.keep();
}

// ------------------------------------------------------------------------------------
// directional sparsity: the mode table and what the group kernels need
// ------------------------------------------------------------------------------------
static inline int gp2_nsb(const vch2d_ctx *c) { return (int)((c->G.plane + 63) / 64); }      // workgroups of a pencil kernel
static inline long gp2_ss(const vch2d_ctx *c) { return std::max<long>(c->Mmax + 1, (long)c->G.ns * c->G.nf); }
static bool gp2_any(const vch2d_ctx *c, int mode) { return std::find(c->modes.begin(), c->modes.end(), mode) != c->modes.end(); }
static bool gp2_group(const vch2d_ctx *c) { return gp2_any(c, VCH_SPARSITY_TIME) || gp2_any(c, VCH_SPARSITY_SPACE); }
static int gp2_mode(const vch2d_ctx *c, int b) { return c->modes.empty() ? VCH_SPARSITY_FULL : c->modes[b]; }
constexpr int GP2_RESIDENT = -1;          // cost_core: every trajectory by the resident problem's mode table

// the buffers of the group kernels, all or none, beside the cost buffers whose layout the TIME prox shares
static int gp2_ensure(vch2d_ctx *c) {
    VCHCHK(ensure_cost_bufs(c));
    if (!c->gp_s) {
        const size_t B = c->B, nsb = gp2_nsb(c);
        vch_group g(c->pool);
        MEMCHK(c->pool.dev(&c->mode_dev, sizeof(int) * B));
        MEMCHK(c->pool.dev(&c->gp_wt, sizeof(double) * (c->Mmax + 1)));
        MEMCHK(c->pool.dev(&c->gp_s, sizeof(double) * B * gp2_ss(c)));
        MEMCHK(c->pool.dev(&c->gp_tpart, sizeof(double) * B * (c->Mmax + 1) * c->nblk * 4));
        MEMCHK(c->pool.dev(&c->gp_chg, sizeof(double) * B * nsb * 2));
        MEMCHK(c->pool.dev(&c->gp_j4, sizeof(double) * B * nsb));
        MEMCHK(c->pool.dev(&c->gp_one, sizeof(double) * B));
        g.keep();
        const std::vector<double> one(B, 1.0);
        HIPCHK(hipMemcpyAsync(c->gp_one, one.data(), sizeof(double) * B, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));          // one is a local
    }
    c->gp_chg_host.resize((size_t)c->B * gp2_nsb(c) * 2);
    c->gp_j4_host.resize((size_t)c->B * gp2_nsb(c));
    return 0;
}

// the trapezoid weights of t_hist [rows] for the pencil norms
static int gp2_time_weights(vch2d_ctx *c, const double *t_hist, int rows) {
    const std::vector<double> wt = trapz_w(t_hist, rows);
    HIPCHK(hipMemcpyAsync(c->gp_wt, wt.data(), sizeof(double) * rows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));              // wt is a local
    return 0;
}

// The group prox of the trajectories of `mode` (mode_dev NULL: all of them): u, r -> uout (or NULL: the sums alone), s in
// gp_s.  TIME: three launches, the change partials in cost_part (the layout of k_grad_prox).  SPACE: one launch, the change
// partials in gp_chg.  W_cost (TIME) and gp_wt (SPACE) hold the group's weights.
static int gp2_launch(vch2d_ctx *c, int mode, const int *mode_dev, const double *u_dev, const double *r_dev, int rows,
                      const double *alpha_dev, const double *opt_tab, double *uout) {
    const Geom &G = c->G;
    if (mode == VCH_SPARSITY_TIME) {
        const dim3 g(c->nblk, rows, c->B);
        LAUNCHC(PC_PROX, k_gp_time_part, g, dim3(NTH), G, G.tiles_f, u_dev, r_dev, hist_stride(c), alpha_dev, opt_tab, mode_dev,
                (const double *)c->W_cost, c->gp_tpart);
        LAUNCHC(PC_PROX, k_gp_time_solve, dim3(rows, c->B), dim3(GT_T), G, c->nblk, u_dev, r_dev, hist_stride(c), alpha_dev, opt_tab,
                mode_dev, (const double *)c->W_cost, (const double *)c->gp_tpart, c->gp_s, gp2_ss(c));
        LAUNCHC(PC_PROX, k_gp_time_apply, g, dim3(NTH), G, G.tiles_f, u_dev, r_dev, hist_stride(c), alpha_dev, opt_tab, mode_dev,
                (const double *)c->gp_s, gp2_ss(c), uout, c->cost_part);
    } else {
        LAUNCHC(PC_PROX, k_gp_space, dim3(gp2_nsb(c), c->B), dim3(GT_T), G, rows, u_dev, r_dev, hist_stride(c), alpha_dev, opt_tab,
                mode_dev, (const double *)c->gp_wt, uout, c->gp_s, gp2_ss(c), c->gp_chg);
    }
    return 0;
}

// sum_ij W_ij ||u[:, i, j]||_wt of the SPACE trajectories (mode_dev NULL: all) into gp_j4_host [B][gp2_nsb], one look
static int gp2_pencil_cost(vch2d_ctx *c, const int *mode_dev, const double *u_dev, int rows) {
    LAUNCHC(PC_COST, k_gp_pencil, dim3(gp2_nsb(c), c->B), dim3(GT_T), c->G, rows, u_dev, hist_stride(c), mode_dev,
            (const double *)c->gp_wt, (const double *)c->W_cost, c->gp_j4);
    HIPCHK(hipMemcpyAsync(c->gp_j4_host.data(), c->gp_j4, sizeof(double) * c->gp_j4_host.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// J4 / kappa_s of a group mode for one trajectory: s [levels][4] the level sums of k_cost (TIME: column 2 = sum W u^2), or
// the pencil kernel's partials pen [gp2_nsb] (SPACE).  Host sums in index order.
static double gp2_j4(int mode, const double *s, const double *t, int M, const double *pen, int nsb) {
    double acc = 0;
    if (mode == VCH_SPARSITY_TIME)
        for (int n = 0; n < M; ++n) acc += (t[n + 1] - t[n]) * (std::sqrt(s[(n + 1) * 4 + 2]) + std::sqrt(s[n * 4 + 2])) / 2.0;
    else
        for (int j = 0; j < nsb; ++j) acc += pen[j];
    return acc;
}

// J_out [B][5]; arrays on the device in history layout; phiQ_dev NULL + ramp => on-the-fly ramp target
static int cost_core(vch2d_ctx *c, const double *phi_dev, const double *u_dev, const double *pq_dev, const double *pt_dev,
                     bool ramp, int M, const double *t_hist, const vch_opt_params *opts, double *J_out,
                     double *raw_out = nullptr /* [B][2] = {int int (phi - phi_Q)^2, int (phi_M - phi_T)^2} */,
                     int n_opts = 1 /* 1: opts[0] weighs every trajectory; B: trajectory b takes opts[b] */,
                     int mode_sel = VCH_SPARSITY_FULL /* J4 of this mode for the whole batch; GP2_RESIDENT: by the mode table */) {
    const Geom &G = c->G;
    const int levels = M + 1, ntiles = c->nblk;
    VCHCHK(ensure_cost_bufs(c));
    dim3 g(ntiles, levels, c->B);
    LAUNCHC(PC_COST, k_cost, g, dim3(NTH), G, G.tiles_f, phi_dev, u_dev, pq_dev, pt_dev, (const double *)c->phi0,
           (const double *)((ramp && !pq_dev) ? c->tfrac_dev : nullptr), hist_stride(c), M, (const double *)c->W_cost,
           c->cost_part);
    LAUNCH(k_cost_fin, dim3(c->B * levels), dim3(64), ntiles, (const double *)c->cost_part, c->cost_lvl);
    HIPCHK(hipMemcpyAsync(c->cost_lvl_host, c->cost_lvl, (size_t)c->B * levels * 4 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // the pencil norms of the SPACE trajectories (none: the launches and looks above are the call's)
    const bool resident = mode_sel == GP2_RESIDENT;
    if (u_dev && (resident ? gp2_any(c, VCH_SPARSITY_SPACE) : mode_sel == VCH_SPARSITY_SPACE))
        VCHCHK(gp2_pencil_cost(c, resident ? (const int *)c->mode_dev : nullptr, u_dev, levels));
    for (int b = 0; b < c->B; ++b) {
        const double *s = c->cost_lvl_host + (size_t)b * levels * 4;
        double i1 = 0.0, i3 = 0.0, i4 = 0.0;
        for (int n = 0; n < M; ++n) {          // np.trapz over t (C2:84,98,106)
            const double d = t_hist[n + 1] - t_hist[n];
            i1 += d * (s[(n + 1) * 4 + 0] + s[n * 4 + 0]) / 2.0;
            i3 += d * (s[(n + 1) * 4 + 2] + s[n * 4 + 2]) / 2.0;
            i4 += d * (s[(n + 1) * 4 + 3] + s[n * 4 + 3]) / 2.0;
        }
        const int mode = resident ? gp2_mode(c, b) : mode_sel;
        if (mode != VCH_SPARSITY_FULL)
            i4 = u_dev ? gp2_j4(mode, s, t_hist, M, c->gp_j4_host.data() + (size_t)b * gp2_nsb(c), gp2_nsb(c)) : 0.0;
        double *J = J_out + 5 * b;
        const vch_opt_params *o = opts + (n_opts == 1 ? 0 : b);
        J[0] = (o->b1 / 2.0) * i1;
        J[1] = (o->b2 / 2.0) * s[M * 4 + 1];
        J[2] = (o->b3 / 2.0) * i3;
        J[3] = o->kappa_sparsity * i4;
        J[4] = J[0] + J[1] + J[2] + J[3];
        if (raw_out) {
            raw_out[2 * b] = i1;
            raw_out[2 * b + 1] = s[M * 4 + 1];
        }
    }
    return 0;
}

// int_t int_Omega a^2 (levels > 1, trapezoid in t) or int_Omega a^2 (levels == 1) per trajectory, with the cost's weights
static int l2sq_core(vch2d_ctx *c, const double *arr, long stride, int levels, const double *t_hist, double *out) {
    const Geom &G = c->G;
    const int ntiles = c->nblk;
    VCHCHK(ensure_cost_bufs(c));
    LAUNCH(k_cost, dim3(ntiles, levels, c->B), dim3(NTH), G, G.tiles_f, arr, (const double *)nullptr, (const double *)nullptr,
           (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, stride, -1, (const double *)c->W_cost,
           c->cost_part);
    LAUNCH(k_cost_fin, dim3(c->B * levels), dim3(64), ntiles, (const double *)c->cost_part, c->cost_lvl);
    HIPCHK(hipMemcpyAsync(c->cost_lvl_host, c->cost_lvl, (size_t)c->B * levels * 4 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < c->B; ++b) {
        const double *s = c->cost_lvl_host + (size_t)b * levels * 4;
        if (levels == 1) { out[b] = s[0]; continue; }
        double acc = 0.0;
        for (int n = 0; n + 1 < levels; ++n) acc += (t_hist[n + 1] - t_hist[n]) * (s[(n + 1) * 4] + s[n * 4]) / 2.0;
        out[b] = acc;
    }
    return 0;
}

// vch2d_cost and vch2d_cost_g: J4 of `mode` for the whole batch
static int cost_seam(vch2d_ctx *c, const double *phi_hist, const double *u, const double *phi_Q, const double *phi_T, int M,
                     const double *x, const double *y, const double *t_hist, const vch_opt_params *opt, int mode, double *J_out) {
    if (mode == VCH_SPARSITY_SPACE) {
        VCHCHK(gp2_ensure(c));
        VCHCHK(gp2_time_weights(c, t_hist, M + 1));
    }
    VCHCHK(set_cost_weights(c, x, y));
    if (phi_hist) {
        VCHCHK(ensure_hist(c, &c->phi_hist));
        VCHCHK(h2d_hist(c, c->phi_hist, phi_hist, M + 1));
        c->M_res = M;
        c->res_pgd = false;
        c->shift_res = false;         // a history of the caller's: no march of this context stands behind it
    } else if (c->M_res != M) {
        return vch_fail(VCH_ERR_STATE, "vch2d_cost: no resident history with %d steps", M);
    }
    const double *ud = nullptr, *pq = nullptr, *pt = nullptr;
    if (u == VCH_RESIDENT) {
        ud = c->u_hist;
    } else if (u) {
        VCHCHK(ensure_hist(c, &c->u_hist));
        VCHCHK(h2d_hist(c, c->u_hist, u, M + 1));
        c->u_rows_res = M + 1;
        ud = c->u_hist;
    }
    if (phi_Q == VCH_RESIDENT) {
        pq = c->phiQ;
    } else if (phi_Q) {
        VCHCHK(ensure_hist(c, &c->phiQ));
        VCHCHK(h2d_hist(c, c->phiQ, phi_Q, M + 1));
        pq = c->phiQ;
    }
    if (phi_T == VCH_RESIDENT) {
        pt = c->phiT;
    } else if (phi_T) {
        VCHCHK(h2d(c, c->phiT, phi_T, c->B));
        pt = c->phiT;
    }
    return cost_core(c, c->phi_hist, ud, pq, pt, false, M, t_hist, opt, J_out, nullptr, 1, mode);
}

extern "C" int vch2d_cost(vch2d_ctx *c, const double *phi_hist, const double *u, const double *phi_Q, const double *phi_T,
                          int M, const double *x, const double *y, const double *t_hist, const vch_opt_params *opt,
                          double *J_out) {
    CTXCHK(c);
    ARGCHK(x && y && t_hist && opt && J_out && M >= 1 && M <= c->Mmax, "NULL argument or M out of range");
    return cost_seam(c, phi_hist, u, phi_Q, phi_T, M, x, y, t_hist, opt, VCH_SPARSITY_FULL, J_out);
}

extern "C" int vch2d_cost_g(vch2d_ctx *c, const double *phi_hist, const double *u, const double *phi_Q, const double *phi_T,
                            int M, const double *x, const double *y, const double *t_hist, const vch_opt_params *opt,
                            int sparsity, double *J_out) {
    CTXCHK(c);
    ARGCHK(x && y && t_hist && opt && J_out && M >= 1 && M <= c->Mmax, "NULL argument or M out of range");
    ARGCHK(sparsity >= VCH_SPARSITY_FULL && sparsity <= VCH_SPARSITY_SPACE, "sparsity is none of VCH_SPARSITY_FULL, _TIME, _SPACE");
    return cost_seam(c, phi_hist, u, phi_Q, phi_T, M, x, y, t_hist, opt, sparsity, J_out);
}

extern "C" int vch2d_free_energy(vch2d_ctx *c, const double *phi_hist, int rows, const double *w_hist, double hx, double hy,
                                 double eps, double *E_out) {
    CTXCHK(c);
    ARGCHK(phi_hist && E_out && rows >= 1 && rows <= c->Mmax + 1 && hx > 0 && hy > 0, "NULL argument, rows out of range or h <= 0");
    const double *pd = nullptr, *wd = nullptr;
    if (phi_hist == VCH_RESIDENT) {
        ARGCHK(c->phi_hist && c->M_res + 1 >= rows, "no resident state history with that many levels");
        pd = c->phi_hist;
    } else {
        VCHCHK(ensure_hist(c, &c->phi_hist));
        VCHCHK(h2d_hist(c, c->phi_hist, phi_hist, rows));
        c->M_res = rows - 1;
        c->res_pgd = false;
        c->shift_res = false;
        pd = c->phi_hist;
    }
    if (w_hist) {                      // the coupling field travels through the trial-state buffer
        VCHCHK(ensure_hist(c, &c->phi_trial));
        VCHCHK(h2d_hist(c, c->phi_trial, w_hist, rows));
        wd = c->phi_trial;
    }
    const int ntiles = c->nblk, A0 = c->prm.Nx + 1, A1 = c->prm.Ny + 1;
    VCHCHK(ensure_cost_bufs(c));
    const int nt = (A0 * A1 + 1023) / 1024;            // <= tiles_f * tiles_s
    LAUNCH(k_energy, dim3(nt, rows, c->B), dim3(NTH), c->G, A0, A1, c->P.c1, c->P.c2, eps > 0 ? eps : 1e-8, pd, wd,
           hist_stride(c), c->cost_part);
    LAUNCH(k_cost_fin, dim3(c->B * rows), dim3(64), nt, (const double *)c->cost_part, c->cost_lvl);
    HIPCHK(hipMemcpyAsync(c->cost_lvl_host, c->cost_lvl, (size_t)c->B * rows * 4 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (long k = 0; k < (long)c->B * rows; ++k) {
        const double *s = c->cost_lvl_host + 4 * k;
        // axis 0 carries hy and axis 1 carries hx, as the reference labels them (F2:293-302)
        double E = (c->P.kappa / (2.0 * hy)) * s[0] * hx + (c->P.kappa / (2.0 * hx)) * s[1] * hy + hx * hy * s[2];
        if (w_hist) E -= hx * hy * s[3];
        E_out[k] = E;
    }
    return 0;
}

// u_out = prox(u - alpha (r + b3 u)), trajectory b with row b of the device table opt_tab; change_out [B][2] =
// {sum (u+ - u)^2, sum u^2} or NULL.  mode_sel: the prox of this mode for the whole batch, or GP2_RESIDENT: every trajectory
// by the resident problem's mode table, k_grad_prox once per run of consecutive FULL trajectories (pointer offsets) and each
// group kernel once over the batch.  Without a group mode the launches, looks and bits are those of the one k_grad_prox
// launch over the batch.  uout_dev NULL (group modes only): the change sums alone.
static int grad_prox_core(vch2d_ctx *c, const double *u_dev, const double *r_dev, int rows, const double *alpha_host,
                          const double *opt_tab, double *uout_dev, double *change_out, int mode_sel = VCH_SPARSITY_FULL) {
    HIPCHK(hipMemcpyAsync(c->alpha_dev, alpha_host, sizeof(double) * c->B, hipMemcpyHostToDevice, c->stream));
    VCHCHK(ensure_cost_bufs(c));
    const int B = c->B;
    const bool resident = mode_sel == GP2_RESIDENT && gp2_group(c);
    const bool grouped = resident || (mode_sel != GP2_RESIDENT && mode_sel != VCH_SPARSITY_FULL);
    HIPCHK(hipMemsetAsync(c->cost_part, 0, (size_t)B * rows * c->nblk * 4 * 8, c->stream));
    if (!grouped) {
        dim3 g(c->nblk, rows, B);
        LAUNCHC(PC_PROX, k_grad_prox, g, dim3(NTH), c->G, c->G.tiles_f, u_dev, r_dev, hist_stride(c), (const double *)c->alpha_dev, opt_tab,
               uout_dev, c->cost_part);
    } else if (resident) {
        const long hs = hist_stride(c);
        for (int b0 = 0; b0 < B;) {
            if (gp2_mode(c, b0) != VCH_SPARSITY_FULL) { ++b0; continue; }
            int b1 = b0 + 1;
            while (b1 < B && gp2_mode(c, b1) == VCH_SPARSITY_FULL) ++b1;
            LAUNCHC(PC_PROX, k_grad_prox, dim3(c->nblk, rows, b1 - b0), dim3(NTH), c->G, c->G.tiles_f, u_dev + b0 * hs, r_dev + b0 * hs, hs,
                    (const double *)c->alpha_dev + b0, opt_tab + (size_t)b0 * OPT_STRIDE, uout_dev + b0 * hs,
                    c->cost_part + (size_t)b0 * rows * c->nblk * 4);
            b0 = b1;
        }
        for (int mode : {VCH_SPARSITY_TIME, VCH_SPARSITY_SPACE})
            if (gp2_any(c, mode))
                VCHCHK(gp2_launch(c, mode, c->mode_dev, u_dev, r_dev, rows, c->alpha_dev, opt_tab, uout_dev));
    } else {
        VCHCHK(gp2_launch(c, mode_sel, nullptr, u_dev, r_dev, rows, c->alpha_dev, opt_tab, uout_dev));
    }
    if (change_out) {
        LAUNCH(k_cost_fin, dim3(B * rows), dim3(64), c->nblk, (const double *)c->cost_part, c->cost_lvl);
        HIPCHK(hipMemcpyAsync(c->cost_lvl_host, c->cost_lvl, (size_t)B * rows * 4 * 8, hipMemcpyDeviceToHost, c->stream));
        const bool space = resident ? gp2_any(c, VCH_SPARSITY_SPACE) : (grouped && mode_sel == VCH_SPARSITY_SPACE);
        if (space)
            HIPCHK(hipMemcpyAsync(c->gp_chg_host.data(), c->gp_chg, sizeof(double) * c->gp_chg_host.size(), hipMemcpyDeviceToHost,
                                  c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int b = 0; b < B; ++b) {
            double d = 0.0, n = 0.0;
            if (space && (resident ? gp2_mode(c, b) : mode_sel) == VCH_SPARSITY_SPACE) {
                const double *q = c->gp_chg_host.data() + (size_t)b * gp2_nsb(c) * 2;      // the pencil kernel's workgroups, in index order
                for (int j = 0; j < gp2_nsb(c); ++j) { d += q[2 * j]; n += q[2 * j + 1]; }
            } else {
                for (int l = 0; l < rows; ++l) {
                    d += c->cost_lvl_host[((size_t)b * rows + l) * 4 + 0];
                    n += c->cost_lvl_host[((size_t)b * rows + l) * 4 + 1];
                }
            }
            change_out[2 * b] = d;
            change_out[2 * b + 1] = n;
        }
    }
    return 0;
}

extern "C" int vch2d_grad_prox(vch2d_ctx *c, const double *u, const double *r, int rows, const double *alpha,
                               const vch_opt_params *opt, double *u_out) {
    CTXCHK(c);
    ARGCHK(u && r && alpha && opt && u_out && rows >= 1 && rows <= c->Mmax + 1, "NULL argument or rows out of range");
    VCHCHK(ensure_hist(c, &c->u_hist));
    VCHCHK(ensure_hist(c, &c->r_hist));
    VCHCHK(ensure_hist(c, &c->u_trial));
    VCHCHK(h2d_hist(c, c->u_hist, u, rows));
    VCHCHK(h2d_hist(c, c->r_hist, r, rows));
    VCHCHK(write_opt_tab(c, c->seam_tab, opt, 1));
    VCHCHK(grad_prox_core(c, c->u_hist, c->r_hist, rows, alpha, c->seam_tab, c->u_trial, nullptr));
    return d2h_hist(c, u_out, c->u_trial, rows);
}

extern "C" int vch2d_grad_prox_g(vch2d_ctx *c, const double *u, const double *r, int rows, const double *x, const double *y,
                                 const double *t_hist, const double *alpha, const vch_opt_params *opt, int sparsity,
                                 double *u_out, double *scale_out) {
    CTXCHK(c);
    ARGCHK(sparsity >= VCH_SPARSITY_FULL && sparsity <= VCH_SPARSITY_SPACE, "sparsity is none of VCH_SPARSITY_FULL, _TIME, _SPACE");
    if (sparsity == VCH_SPARSITY_FULL) return vch2d_grad_prox(c, u, r, rows, alpha, opt, u_out);
    ARGCHK(u && r && alpha && opt && u_out && rows >= 1 && rows <= c->Mmax + 1, "NULL argument or rows out of range");
    ARGCHK(sparsity == VCH_SPARSITY_TIME ? (x && y) : (t_hist != nullptr), "NULL x, y (TIME) or t_hist (SPACE): the group's weights");
    ARGCHK(opt->u_min <= 0.0 && opt->u_max >= 0.0, "a group mode needs a box with u_min <= 0 <= u_max");
    ARGCHK(std::isfinite(opt->kappa_sparsity) && opt->kappa_sparsity >= 0, "kappa_sparsity must be finite and >= 0");
    VCHCHK(ensure_hist(c, &c->u_hist));
    VCHCHK(ensure_hist(c, &c->r_hist));
    VCHCHK(ensure_hist(c, &c->u_trial));
    VCHCHK(gp2_ensure(c));
    VCHCHK(h2d_hist(c, c->u_hist, u, rows));
    VCHCHK(h2d_hist(c, c->r_hist, r, rows));
    VCHCHK(write_opt_tab(c, c->seam_tab, opt, 1));
    if (sparsity == VCH_SPARSITY_TIME) VCHCHK(set_cost_weights(c, x, y));
    else VCHCHK(gp2_time_weights(c, t_hist, rows));
    VCHCHK(grad_prox_core(c, c->u_hist, c->r_hist, rows, alpha, c->seam_tab, c->u_trial, nullptr, sparsity));
    if (scale_out) {
        const size_t ng = sparsity == VCH_SPARSITY_TIME ? (size_t)rows : (size_t)c->G.ns * c->G.nf;
        for (int b = 0; b < c->B; ++b)
            HIPCHK(hipMemcpyAsync(scale_out + b * ng, c->gp_s + b * gp2_ss(c), sizeof(double) * ng, hipMemcpyDeviceToHost, c->stream));
    }
    return d2h_hist(c, u_out, c->u_trial, rows);
}

// ------------------------------------------------------------------------------------
// device-resident PGD loop (G2:291-382)
// ------------------------------------------------------------------------------------
// the shift record of an accepted trial follows its history (copy_traj(phi_hist, phi_trial))
static int copy_traj_shifts(vch2d_ctx *c, int b) {
    const size_t n = (size_t)c->Mmax * SHIFT_REC;
    HIPCHK(hipMemcpyAsync(c->shift_hist + b * n, c->shift_trial + b * n, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}
static int copy_traj(vch2d_ctx *c, double *dst, const double *src, int b, int rows) {
    const long hs = hist_stride(c);
    HIPCHK(hipMemcpyAsync(dst + b * hs, src + b * hs, sizeof(double) * rows * c->G.plane, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// vch2d_pgd_init_v and vch2d_pgd_init_g (fn: who the messages name).  sparsity NULL: every trajectory VCH_SPARSITY_FULL.
static int pgd_init2(vch2d_ctx *c, const char *fn, const double *phi0, const double *phi_T, const double *phi_Q, int ramp, double T,
                     const double *t_hist, int M, const double *x, const double *y, const vch_opt_params *opts, int n_opts,
                     const double *u0, const double *alpha0, const int32_t *sparsity, int n_sparsity, double *J0_out) {
    if (!(phi0 && phi_T && t_hist && x && y && opts && M >= 1 && M <= c->Mmax))
        return vch_fail(VCH_ERR_ARG, "%s: NULL argument or M out of range", fn);
    if (!(n_opts == 1 || n_opts == c->B)) return vch_fail(VCH_ERR_ARG, "%s: n_opts must be 1 or the context's batch", fn);
    // all of this before anything is enqueued or any resident state changes
    for (int b = 0; b < c->B; ++b)
        if (const char *bad = vch_pgd_check(opts, n_opts, alpha0, b))
            return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: %s", fn, b, bad);
    bool grouped = false;
    if (sparsity) {
        if (!(n_sparsity == 1 || n_sparsity == c->B)) return vch_fail(VCH_ERR_ARG, "%s: n_sparsity must be 1 or the context's batch", fn);
        for (int b = 0; b < c->B; ++b) {
            const int m = sparsity[n_sparsity == 1 ? 0 : b];
            const vch_opt_params &o = vch_pgd_opt(opts, n_opts, b);
            if (m < VCH_SPARSITY_FULL || m > VCH_SPARSITY_SPACE)
                return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: sparsity %d is none of VCH_SPARSITY_FULL, _TIME, _SPACE", fn, b, m);
            if (m != VCH_SPARSITY_FULL && !(o.u_min <= 0.0 && o.u_max >= 0.0))
                return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: a group mode needs a box with u_min <= 0 <= u_max", fn, b);
            grouped = grouped || m != VCH_SPARSITY_FULL;
        }
        for (int n = 0; n < M; ++n)
            if (!(t_hist[n + 1] - t_hist[n] > 0)) return vch_fail(VCH_ERR_ARG, "%s: t_hist must be strictly increasing", fn);
    }
    if (grouped) VCHCHK(gp2_ensure(c));      // before any resident state changes: a refused allocation leaves the problem as it was
    c->modes.assign(c->B, VCH_SPARSITY_FULL);
    if (sparsity)
        for (int b = 0; b < c->B; ++b) c->modes[b] = sparsity[n_sparsity == 1 ? 0 : b];
    if (grouped) {
        HIPCHK(hipMemcpyAsync(c->mode_dev, c->modes.data(), sizeof(int) * c->B, hipMemcpyHostToDevice, c->stream));
        VCHCHK(gp2_time_weights(c, t_hist, M + 1));
    }
    c->opts.resize(c->B);
    for (int b = 0; b < c->B; ++b) c->opts[b] = vch_pgd_opt(opts, n_opts, b);
    VCHCHK(write_opt_tab(c, c->opt_tab, c->opts.data(), c->B));
    c->pgd_r_valid = false;
    c->t_hist.assign(t_hist, t_hist + M + 1);
    c->dt.resize(M);
    for (int n = 0; n < M; ++n) {
        c->dt[n] = t_hist[n + 1] - t_hist[n];
        if (!(c->dt[n] > 0)) return vch_fail(VCH_ERR_ARG, "%s: t_hist must be strictly increasing", fn);
    }
    c->xg.assign(x, x + c->prm.Nx + 1);
    c->yg.assign(y, y + c->prm.Ny + 1);
    VCHCHK(set_cost_weights(c, x, y));
    VCHCHK(ensure_hist(c, &c->phi_hist));
    VCHCHK(ensure_hist(c, &c->phi_trial));
    VCHCHK(ensure_hist(c, &c->u_hist));
    VCHCHK(ensure_hist(c, &c->u_trial));
    VCHCHK(ensure_hist(c, &c->r_hist));
    VCHCHK(h2d(c, c->phi0, phi0, c->B));
    VCHCHK(h2d(c, c->phiT, phi_T, c->B));
    c->ramp = false;
    if (phi_Q) {
        VCHCHK(ensure_hist(c, &c->phiQ));
        VCHCHK(h2d_hist(c, c->phiQ, phi_Q, M + 1));
    } else if (ramp) {
        c->ramp = true;
        c->rampT = T;
        c->tfrac.resize(M + 1);
        for (int n = 0; n <= M; ++n) c->tfrac[n] = t_hist[n] / T;      // G2:221
        if (!c->tfrac_dev) MEMCHK(c->pool.dev(&c->tfrac_dev, sizeof(double) * (c->Mmax + 1)));
        HIPCHK(hipMemcpyAsync(c->tfrac_dev, c->tfrac.data(), sizeof(double) * (M + 1), hipMemcpyHostToDevice, c->stream));
        // materialise phi_Q once on the device (the adjoint source reads it every step)
        VCHCHK(ensure_hist(c, &c->phiQ));
        LAUNCH(k_ramp, dim3(c->nblk, M + 1, c->B), dim3(NTH), c->G, c->G.tiles_f, (const double *)c->phi0,
               (const double *)c->phiT, (const double *)c->tfrac_dev, hist_stride(c), c->phiQ);
    } else {
        if (c->phiQ) HIPCHK(hipMemsetAsync(c->phiQ, 0, sizeof(double) * c->B * hist_stride(c), c->stream));
    }
    // u^0 = 0 and the uncontrolled march (G2:255-258), or the caller's u^0 as given (not clipped) and the march under it;
    // then J(u^0) under every trajectory's own weights (G2:291)
    HIPCHK(hipMemsetAsync(c->u_hist, 0, sizeof(double) * c->B * hist_stride(c), c->stream));
    if (u0) VCHCHK(h2d_hist(c, c->u_hist, u0, M + 1));
    c->u_rows_res = M + 1;
    VCHCHK(reset_counters(c));
    HIPCHK(hipMemcpyAsync(c->phi_s, c->phi0, sizeof(double) * c->B * c->G.plane, hipMemcpyDeviceToDevice, c->stream));
    if (u0) VCHCHK(forward_core(c, c->u_hist, M + 1, c->dt.data(), M, c->phi_hist));
    else VCHCHK(forward_core(c, nullptr, 0, c->dt.data(), M, c->phi_hist));
    c->M_res = M;
    c->res_pgd = false;
    c->shift_res = true;
    c->J_host.assign(5 * c->B, 0.0);
    VCHCHK(cost_core(c, c->phi_hist, c->u_hist, (phi_Q || ramp) ? c->phiQ : nullptr, c->phiT, false, M, c->t_hist.data(),
                     c->opts.data(), c->J_host.data(), nullptr, c->B, GP2_RESIDENT));
    // target norms of the error metrics (G2:348-361)
    c->pgd.denQ2.assign(c->B, 0.0);
    c->pgd.denT2.assign(c->B, 0.0);
    if (phi_Q || ramp) VCHCHK(l2sq_core(c, c->phiQ, hist_stride(c), M + 1, c->t_hist.data(), c->pgd.denQ2.data()));
    VCHCHK(l2sq_core(c, c->phiT, c->G.plane, 1, nullptr, c->pgd.denT2.data()));
    {
        const double area = (x[c->prm.Nx] - x[0]) * (y[c->prm.Ny] - y[0]), tl = t_hist[M] - t_hist[0];
        c->pgd.rms = std::sqrt(std::max(area, 1e-30) * std::max(tl, 1e-30));
    }
    c->pgd.reset(c->B, c->J_host.data(), c->opts.data(), alpha0);
    HIPCHK(hipMemcpyAsync(c->J_dev, c->J_host.data(), sizeof(double) * 5 * c->B, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (J0_out) memcpy(J0_out, c->J_host.data(), sizeof(double) * 5 * c->B);
    c->pgd_iter_total = 0;
    c->pgd_ready = true;
    c->res_pgd = true;
    return 0;
}

extern "C" int vch2d_pgd_init_v(vch2d_ctx *c, const double *phi0, const double *phi_T, const double *phi_Q, int ramp, double T,
                                const double *t_hist, int M, const double *x, const double *y, const vch_opt_params *opts,
                                int n_opts, const double *u0, const double *alpha0, double *J0_out) {
    CTXCHK(c);
    return pgd_init2(c, "vch2d_pgd_init_v", phi0, phi_T, phi_Q, ramp, T, t_hist, M, x, y, opts, n_opts, u0, alpha0, nullptr, 0, J0_out);
}

extern "C" int vch2d_pgd_init_g(vch2d_ctx *c, const double *phi0, const double *phi_T, const double *phi_Q, int ramp, double T,
                                const double *t_hist, int M, const double *x, const double *y, const vch_opt_params *opts,
                                int n_opts, const double *u0, const double *alpha0, const int32_t *sparsity, int n_sparsity,
                                double *J0_out) {
    CTXCHK(c);
    if (!sparsity) return vch_fail(VCH_ERR_ARG, "vch2d_pgd_init_g: NULL sparsity");
    return pgd_init2(c, "vch2d_pgd_init_g", phi0, phi_T, phi_Q, ramp, T, t_hist, M, x, y, opts, n_opts, u0, alpha0, sparsity, n_sparsity,
                     J0_out);
}

extern "C" int vch2d_pgd_init(vch2d_ctx *c, const double *phi0, const double *phi_T, const double *phi_Q, int ramp, double T,
                              const double *t_hist, int M, const double *x, const double *y, const vch_opt_params *opt,
                              double *J0_out) {
    return vch2d_pgd_init_v(c, phi0, phi_T, phi_Q, ramp, T, t_hist, M, x, y, opt, 1, nullptr, nullptr, J0_out);
}

static double elapsed_s(vch2d_ctx *c, hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    hipEventSynchronize(b);
    hipEventElapsedTime(&ms, a, b);
    return ms * 1e-3;
}

extern "C" int vch2d_pgd_iterate(vch2d_ctx *c, int n_iters, double *cost_out, double *alpha_out, int32_t *attempts_out,
                                 double *change_out, double *seconds_out) {
    CTXCHK(c);
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch2d_pgd_iterate: call vch2d_pgd_init first");
    ARGCHK(n_iters >= 1, "n_iters must be >= 1");
    const int B = c->B, M = c->M_res, rows = M + 1;
    const double *pq = (c->phiQ) ? c->phiQ : nullptr;
    double sec[5] = {0, 0, 0, 0, 0};
    hipEvent_t e0 = c->ev0, e1 = c->ev1;
    constexpr vch_pgd_rule R = VCH_PGD_2D;
    static_assert(!R.stop_keeps_state, "an accepted trial is taken whole, also on a stop");
    vch_pgd_state &st = c->pgd;
    std::vector<double> Jt(5 * B), chg(2 * B), raw(2 * B);
    int done_iters = 0;
    st.begin_call(n_iters);
    for (int it = 0; it < n_iters; ++it) {
        if (!st.begin_iteration()) break;
        // --- adjoint sweep on the current state (G2:299)
        HIPCHK(hipEventRecord(e0, c->stream));
        {
            // Adjoint solves inside the PGD loop stop at pgd_adj_tol (relative residual 1e-12; the function-seam entry points
            // vch2d_backward / vch2d_adjoint_solve keep 1e-15, the accuracy class of the reference's direct solves).  What the
            // loop consumes is r in u+ = prox(u - alpha (r + b3 u)): a relative error of 1e-11 in r moves u by 1e-11 |alpha r|,
            // three orders below the tolerance of the PGD parity statement; 1.92 -> 1.38 sweeps per solve.
            const double keep = c->lin_tol;
            c->lin_tol = std::max(c->lin_tol, c->pgd_adj_tol);
            const int rc_ = backward_core(c, c->phi_hist, M, c->t_hist.data(), c->opt_tab, pq, c->phiT, c->r_hist, nullptr, nullptr);
            c->lin_tol = keep;
            VCHCHK(rc_);
            c->pgd_r_valid = true;
        }
        HIPCHK(hipEventRecord(e1, c->stream));
        sec[0] += elapsed_s(c, e0, e1);
        for (int round = 0; round < R.rounds; ++round) {
            // round 0 = optimistic step with alpha_prev (G2:304-313); later rounds = backtracking trials (G2:128-146)
            HIPCHK(hipEventRecord(e0, c->stream));
            VCHCHK(grad_prox_core(c, c->u_hist, c->r_hist, rows, st.alpha.data(), c->opt_tab, c->u_trial, chg.data(), GP2_RESIDENT));
            HIPCHK(hipEventRecord(e1, c->stream));
            sec[1] += elapsed_s(c, e0, e1);
            HIPCHK(hipEventRecord(e0, c->stream));
            HIPCHK(hipMemcpyAsync(c->phi_s, c->phi0, sizeof(double) * B * c->G.plane, hipMemcpyDeviceToDevice, c->stream));
            VCHCHK(reset_counters(c));
            // a trajectory whose step is already accepted (or that has stopped) sits the trial out
            if (std::any_of(st.accepted.begin(), st.accepted.end(), [](int a) { return a != 0; })) VCHCHK(freeze(c, st.accepted));
            VCHCHK(forward_core(c, c->u_trial, rows, c->dt.data(), M, c->phi_trial));
            HIPCHK(hipEventRecord(e1, c->stream));
            sec[round == 0 ? 2 : 4] += elapsed_s(c, e0, e1);
            HIPCHK(hipEventRecord(e0, c->stream));
            VCHCHK(cost_core(c, c->phi_trial, c->u_trial, pq, c->phiT, false, M, c->t_hist.data(), c->opts.data(), Jt.data(), raw.data(), B,
                             GP2_RESIDENT));
            HIPCHK(hipEventRecord(e1, c->stream));
            sec[round == 0 ? 3 : 4] += elapsed_s(c, e0, e1);
            bool pending = false;
            for (int b = 0; b < B; ++b) {
                if (st.accepted[b]) continue;
                vch_pgd_step s;     // the stop rule uses the relative control change (G2:375-381)
                if (st.judge(R, b, it, round, c->opts[b].alpha_max, Jt[5 * b + 4], chg[2 * b], chg[2 * b + 1], raw[2 * b],
                             raw[2 * b + 1], s) == VCH_PGD_PENDING) {
                    pending = true;
                    continue;
                }
                // accepted (or "return last try", G2:144-146)
                std::copy_n(&Jt[5 * b], 5, &c->J_host[5 * b]);
                VCHCHK(copy_traj(c, c->u_hist, c->u_trial, b, rows));
                VCHCHK(copy_traj(c, c->phi_hist, c->phi_trial, b, rows));
                VCHCHK(copy_traj_shifts(c, b));
                if (cost_out) cost_out[(long)b * n_iters + it] = Jt[5 * b + 4];
                if (alpha_out) alpha_out[(long)b * n_iters + it] = s.alpha_k;
                if (attempts_out) attempts_out[(long)b * n_iters + it] = s.count;
                if (change_out) change_out[(long)b * n_iters + it] = s.change;
            }
            if (!pending) break;
        }
        VCHCHK(reset_counters(c));
        done_iters = it + 1;
        {   // this iteration's cost scalars into the ring (read by the collective of this iteration)
            const size_t slot = (size_t)(c->pgd_iter_total.load(std::memory_order_relaxed) % J_RING) * 5 * B;
            memcpy(c->J_ring_host + slot, c->J_host.data(), sizeof(double) * 5 * B);
            HIPCHK(hipMemcpyAsync(c->J_ring_dev + slot, c->J_ring_host + slot, sizeof(double) * 5 * B, hipMemcpyHostToDevice, c->stream));
            c->pgd_iter_total.fetch_add(1, std::memory_order_release);
        }
    }
    HIPCHK(hipMemcpyAsync(c->J_dev, c->J_host.data(), sizeof(double) * 5 * B, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (seconds_out) memcpy(seconds_out, sec, sizeof(sec));
    return done_iters;
}

extern "C" int vch2d_pgd_errors(vch2d_ctx *c, int n_iters, double *tracking_out, double *terminal_out) {
    CTXCHK(c);
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch2d_pgd_errors: call vch2d_pgd_init first");
    ARGCHK(c->pgd.errors(n_iters, tracking_out, terminal_out), "n_iters differs from the last vch2d_pgd_iterate call");
    return 0;
}

extern "C" int vch2d_pgd_get(vch2d_ctx *c, int what, double *out) {
    CTXCHK(c);
    ARGCHK(out && what >= 0 && what <= 3, "NULL out or what not in 0..3");
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch2d_pgd_get: call vch2d_pgd_init first");
    const double *src = what == 0 ? c->u_hist : what == 1 ? c->phi_hist : what == 2 ? c->r_hist : c->phiQ;
    if (!src) return vch_fail(VCH_ERR_STATE, "vch2d_pgd_get: array %d is not resident", what);
    return d2h_hist(c, out, src, c->M_res + 1);
}

extern "C" int vch2d_pgd_kkt(vch2d_ctx *c, int refresh, double tol, int64_t *counts_out, double *stationarity_out) {
    CTXCHK(c);
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch2d_pgd_kkt: call vch2d_pgd_init first");
    ARGCHK(counts_out, "NULL counts_out");
    if (!refresh && !c->pgd_r_valid)
        return vch_fail(VCH_ERR_STATE, "vch2d_pgd_kkt: no adjoint sweep has run since vch2d_pgd_init (pass refresh != 0)");
    const int B = c->B, M = c->M_res, rows = M + 1;
    if (!(tol > 0)) tol = 1e-6;
    if (refresh) {
        // the adjoint of the resident iterate, every trajectory with its own b1, b2, at the accuracy of vch2d_backward
        VCHCHK(backward_core(c, c->phi_hist, M, c->t_hist.data(), c->opt_tab, c->phiQ ? c->phiQ : nullptr, c->phiT, c->r_hist,
                             nullptr, nullptr));
        VCHCHK(reset_counters(c));      // the records as the end of a PGD iteration leaves them
        c->pgd_r_valid = true;
    }
    unsigned long long *kpart = c->kkt_dev + 3 * (size_t)B;
    HIPCHK(hipMemsetAsync(kpart, 0, sizeof(unsigned long long) * 3 * B * rows, c->stream));
    LAUNCH(k_kkt_count, dim3(c->nblk, rows, B), dim3(NTH), c->G, c->G.tiles_f, (const double *)c->u_hist,
           (const double *)c->r_hist, hist_stride(c), (const double *)c->opt_tab, tol, kpart);
    LAUNCH(k_kkt_fin, dim3(B), dim3(64), rows, (const unsigned long long *)kpart, c->kkt_dev);
    std::vector<unsigned long long> cnt(3 * (size_t)B);
    HIPCHK(hipMemcpyAsync(cnt.data(), c->kkt_dev, sizeof(unsigned long long) * 3 * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int64_t total = (int64_t)rows * c->G.ns * c->G.nf;
    for (int b = 0; b < B; ++b) {
        for (int k = 0; k < 3; ++k) counts_out[4 * b + k] = (int64_t)cnt[3 * b + k];
        counts_out[4 * b + 3] = total;
    }
    if (gp2_group(c)) {     // the group modes count groups in the group's norm (the node counts above stand for the FULL members)
        std::vector<double> nu((size_t)B * rows), scratch(B);
        if (gp2_any(c, VCH_SPARSITY_TIME)) {      // sum W u^2 and sum W r^2 of every level by the cost kernel, counted on the host
            VCHCHK(l2sq_core(c, c->u_hist, hist_stride(c), rows, c->t_hist.data(), scratch.data()));
            for (size_t k = 0; k < nu.size(); ++k) nu[k] = c->cost_lvl_host[4 * k];
            VCHCHK(l2sq_core(c, c->r_hist, hist_stride(c), rows, c->t_hist.data(), scratch.data()));
        }
        if (gp2_any(c, VCH_SPARSITY_SPACE)) {
            HIPCHK(hipMemsetAsync(c->kkt_dev, 0, sizeof(unsigned long long) * 3 * B, c->stream));
            LAUNCH(k_gp_kkt_space, dim3(gp2_nsb(c), B), dim3(GT_T), c->G, rows, (const double *)c->u_hist, (const double *)c->r_hist,
                   hist_stride(c), (const double *)c->opt_tab, (const int *)c->mode_dev, (const double *)c->gp_wt, tol, c->kkt_dev);
            HIPCHK(hipMemcpyAsync(cnt.data(), c->kkt_dev, sizeof(unsigned long long) * 3 * B, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        for (int b = 0; b < B; ++b) {
            int64_t *q = counts_out + 4 * b;
            if (gp2_mode(c, b) == VCH_SPARSITY_TIME) {
                q[0] = q[1] = q[2] = 0;
                for (int l = 0; l < rows; ++l) {
                    const bool zero = std::sqrt(nu[(size_t)b * rows + l]) < tol;
                    const bool small = std::sqrt(c->cost_lvl_host[((size_t)b * rows + l) * 4]) <= c->opts[b].kappa_sparsity;
                    q[0] += zero; q[1] += small; q[2] += (zero == small);
                }
                q[3] = rows;
            } else if (gp2_mode(c, b) == VCH_SPARSITY_SPACE) {
                for (int k = 0; k < 3; ++k) q[k] = (int64_t)cnt[3 * b + k];
                q[3] = (int64_t)c->G.ns * c->G.nf;
            }
        }
    }
    if (stationarity_out) {
        // prox_1(u): the grad-prox step with alpha = 1 into the trial-control scratch, and that kernel's change sums
        std::vector<double> one(B, 1.0), chg(2 * (size_t)B);
        VCHCHK(grad_prox_core(c, c->u_hist, c->r_hist, rows, one.data(), c->opt_tab, c->u_trial, chg.data(), GP2_RESIDENT));
        for (int b = 0; b < B; ++b) stationarity_out[b] = std::sqrt(chg[2 * b]) / (std::sqrt(chg[2 * b + 1]) + 1e-9);
    }
    return 0;
}

// ------------------------------------------------------------------------------------
// exact second-order check: tangent marches about the resident control and state history (kernels: "Tangent march" in
// vch_kernels2d.h)
// ------------------------------------------------------------------------------------
// The refusal cells of a linearisation call (FixCheck in vch_kernels2d.h): cleared before the first kernel of the call, read
// with the look that closes it.  A step whose classified interior weight exceeds the weight the march recorded has a skipped
// node that passes for an interior one: the derivative would be that of another scheme, so the call returns an error.  The
// context stays as a successful call leaves it.
static int ensure_fix_bad(vch2d_ctx *c) {
    if (c->fix_bad) return 0;
    if (c->pool.dev(&c->fix_bad, sizeof(int) * c->B)) {
        (void)hipGetLastError();
        return vch_fail(VCH_ERR_NOMEM, "hipMalloc of the mass fix's refusal cells failed");
    }
    return 0;
}
static int fix_check_begin(vch2d_ctx *c) {
    HIPCHK(hipMemsetAsync(c->fix_bad, 0xff, sizeof(int) * c->B, c->stream));
    return 0;
}
static FixCheck fix_check_of(const vch2d_ctx *c, int step) {
    return FixCheck{c->fix_bad, step, (double)c->G.ns * c->G.nf * 2.220446049250313e-16};
}
static int fix_check_end(const char *fn, const std::vector<int> &bad) {
    for (size_t b = 0; b < bad.size(); ++b)
        if (bad[b] >= 0)
            return vch_fail(VCH_ERR_STATE,
                            "%s: trajectory %d, step %d: interior set of the mass fix not recoverable from the state history "
                            "(a node the fix skipped lies within its shift of the band's threshold); the linearisation is refused",
                            fn, (int)b, bad[b]);
    return 0;
}

// One tangent solve: the right-hand side is in slot 0 (k_tan_rhs); x = 0 start, the context's lin_tol, every trajectory
// gated by its own lin_active; on return dphi* is in c->xf and dmu' in c->dmu.  With a shift record (rec: the step's cell)
// the partials of the fix's weighted mean of dphi* follow in c->part_mass, for the kernel that reads c->xf next.
static int tangent_solve(vch2d_ctx *c, double dt, const double *phi1, const double *rec) {
    // a wide diagonal takes the right-scaled CG form by the march's rule (newton_level: the stencil-free path only)
    const bool spectral = c->use_fft && !c->half_f && !c->half_s;
    LAUNCH(k_fin_lin_begin, dim3(c->B), dim3(64), c->st, c->part, c->nblk, 2, c->P.tau, c->P.kappa, dt, c->lin_tol,
           spectral ? c->cg_scale_ratio : 0.0);
    LAUNCH(k_tan_arm, dim3((c->B + 63) / 64), dim3(64), c->st, c->B);
    VCHCHK(sync_state(c, false));
    VCHCHK(schur_solve(c, dt, cg_budget(c, false), true));
    VCHCHK(dmu_ceiling(c, 0));
    if (rec)
        LAUNCH(k_tan_mass, c->grid, dim3(NTH), c->G, (const double *)c->xf, phi1, hist_stride(c), rec, (long)c->Mmax * SHIFT_REC,
               (const double *)c->wts_mass, c->part_mass);
    return 0;
}

// one level of a [B][plane] work plane -> host history [B][M+1][ns][nf] (asynchronous; the caller synchronises)
static int tangent_level_out(vch2d_ctx *c, double *host, const double *dev, int M, int lvl) {
    const size_t lev = (size_t)c->G.nf * c->G.ns;
    for (int b = 0; b < c->B; ++b)
        HIPCHK(hipMemcpy2DAsync(host + ((size_t)b * (M + 1) + lvl) * lev, (size_t)c->G.nf * 8, dev + b * c->G.plane,
                                (size_t)c->G.pitch * 8, (size_t)c->G.nf * 8, (size_t)c->G.ns, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

static int second_order_core(vch2d_ctx *c, const double *h, int h_rows, const double *dt, int M, const double *t_hist,
                             const double *pq, const double *pt, const vch_opt_params *opts, int n_opts, int order, double *out,
                             double *dphi_hist_out, double *d2phi_hist_out, vch_stats *stats) {
    const Geom &G = c->G;
    const int B = c->B, levels = M + 1;
    const long hs = hist_stride(c);
    VCHCHK(ensure_fix_bad(c));
    if (!c->tan_out) {              // all four or none
        vch_group g(c->pool);
        MEMCHK(c->pool.dev(&c->tan_part, (size_t)B * (c->Mmax + 1) * c->nblk * TAN_NSUM * 8));
        MEMCHK(c->pool.dev(&c->tan_lvl, (size_t)B * (c->Mmax + 1) * TAN_NSUM * 8));
        MEMCHK(c->pool.dev(&c->tan_t, (size_t)(c->Mmax + 1) * 8));
        MEMCHK(c->pool.dev(&c->tan_out, (size_t)B * 6 * 8));
        g.keep();
    }
    VCHCHK(ensure_hist(c, &c->u_trial));            // the direction lives in the trial-control scratch
    VCHCHK(h2d_hist(c, c->u_trial, h, h_rows));
    VCHCHK(write_opt_tab(c, c->seam_tab, opts, n_opts));
    HIPCHK(hipMemcpyAsync(c->tan_t, t_hist, sizeof(double) * levels, hipMemcpyHostToDevice, c->stream));
    VCHCHK(reset_counters(c));
    VCHCHK(fix_check_begin(c));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    // planes: dphi, dmu, d2phi, d2mu, and dw in two copies
    double *dphi = c->tmp[0], *dmu = c->tmp[1], *d2phi = c->tmp[2], *d2mu = c->tmp[3], *dw[2] = {c->tmp[4], c->tmp[5]};
    for (int k = 0; k < 6; ++k) HIPCHK(hipMemsetAsync(c->tmp[k], 0, sizeof(double) * B * G.plane, c->stream));
    c->guess_wr = -1;          // the back substitution keeps no increment for a march's starting guesses
    c->cheb_enq = -1;
    const int u_rows = c->res_pgd ? levels : std::min(c->fwd_u_rows, levels);
    const long part_stride = (long)levels * c->nblk * TAN_NSUM;
    const long rec_stride = (long)c->Mmax * SHIFT_REC;
    // the cell of step n in the shift record of the resident history (none behind a history the caller uploaded)
    auto rec_of = [&](int n) { return c->shift_res ? (const double *)c->shift_hist + (long)n * SHIFT_REC : (const double *)nullptr; };
    auto level = [&](int lvl, const double *d1, const double *d2, double *dst_phi, double *dst_mu) -> int {
        TanLevelArgs a{c->phi_hist + (long)lvl * G.plane,
                       pq ? pq + (long)lvl * G.plane : (const double *)nullptr,
                       lvl < u_rows ? c->u_hist + (long)lvl * G.plane : (const double *)nullptr,
                       lvl < h_rows ? c->u_trial + (long)lvl * G.plane : (const double *)nullptr,
                       hs, pt, lvl == M ? 1 : 0, d1, d2, c->xf, c->dmu, dst_phi, dst_mu, c->W_cost,
                       lvl == 0 ? 0 : (d2 ? 2 : 1), lvl == 0 ? (const double *)nullptr : rec_of(lvl - 1), rec_stride,
                       (const double *)c->part_mass, c->P.LxLy, fix_check_of(c, lvl - 1)};
        LAUNCH(k_tan_level, c->grid, dim3(NTH), G, a, c->tan_part + (long)lvl * c->nblk * TAN_NSUM, part_stride);
        return 0;
    };
    VCHCHK(level(0, nullptr, nullptr, nullptr, nullptr));
    if (dphi_hist_out) VCHCHK(tangent_level_out(c, dphi_hist_out, dphi, M, 0));
    if (d2phi_hist_out) VCHCHK(tangent_level_out(c, d2phi_hist_out, d2phi, M, 0));
    for (int n = 0; n < M; ++n) {
        const double *phi1 = c->phi_hist + (long)(n + 1) * G.plane;
        const bool live = n < h_rows - 1;           // F2:545-548
        TanRhsArgs a1{dphi, dmu, dw[n & 1], dw[(n + 1) & 1], live ? c->u_trial + (long)n * G.plane : (const double *)nullptr,
                      live ? c->u_trial + (long)(n + 1) * G.plane : (const double *)nullptr, phi1, hs, nullptr, nullptr, nullptr,
                      nullptr, rec_of(n), rec_stride, nullptr};
        LAUNCH((k_tan_rhs<0>), c->grid, dim3(NTH), G, c->P, a1, dt[n], c->Rphi_s, c->rhs_s, c->D_s, c->part);
        VCHCHK(tangent_solve(c, dt[n], phi1, rec_of(n)));
        // the level's kernel takes the fix's mean out of the last solve's output on its way to the plane the next step reads
        // (k_tan_rhs<1> does that for dphi'), so the host copies come from those planes
        if (order == 2) {
            TanRhsArgs a2{d2phi, d2mu, nullptr, nullptr, nullptr, nullptr, phi1, hs, c->xf, c->dmu, dphi, dmu, rec_of(n), rec_stride,
                          (const double *)c->part_mass};
            LAUNCH((k_tan_rhs<1>), c->grid, dim3(NTH), G, c->P, a2, dt[n], c->Rphi_s, c->rhs_s, c->D_s, c->part);
            VCHCHK(tangent_solve(c, dt[n], phi1, rec_of(n)));
            VCHCHK(level(n + 1, dphi, c->xf, d2phi, d2mu));
            if (dphi_hist_out) VCHCHK(tangent_level_out(c, dphi_hist_out, dphi, M, n + 1));
            if (d2phi_hist_out) VCHCHK(tangent_level_out(c, d2phi_hist_out, d2phi, M, n + 1));
        } else {
            VCHCHK(level(n + 1, c->xf, nullptr, dphi, dmu));
            if (dphi_hist_out) VCHCHK(tangent_level_out(c, dphi_hist_out, dphi, M, n + 1));
        }
    }
    LAUNCH(k_tan_fin, dim3(B * levels), dim3(64), c->nblk, (const double *)c->tan_part, c->tan_lvl);
    LAUNCH(k_tan_scalars, dim3(B), dim3(64), M, (const double *)c->tan_lvl, (const double *)c->tan_t, (const double *)c->seam_tab,
           order, c->tan_out);
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    std::vector<int> bad(B, -1);
    HIPCHK(hipMemcpyAsync(out, c->tan_out, sizeof(double) * 6 * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(bad.data(), c->fix_bad, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
    VCHCHK(sync_state(c));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    fill_stats(c, stats, ms);
    VCHCHK(reset_counters(c));      // the records as the end of a PGD iteration leaves them
    return fix_check_end("vch2d_second_order", bad);
}

// The argument rules vch2d_second_order and vch2d_hessvec share, in the order their messages are pinned: checked before
// anything is enqueued or any resident state changes.  fn = the calling entry point's name.  With a resident PGD problem
// NULL dt / t_hist are replaced by the problem's.
#define TANCHK(cond, msg)                                                  \
    do {                                                                   \
        if (!(cond)) return vch_fail(VCH_ERR_ARG, "%s: %s", fn, msg);      \
    } while (0)
static int tan_check_state(const vch2d_ctx *c, const char *fn) {
    if (c->M_res < 1 || !c->phi_hist)
        return vch_fail(VCH_ERR_STATE, "%s: no resident state history (call vch2d_forward or vch2d_pgd_init first)", fn);
    return 0;
}
static int tan_check_args(const vch2d_ctx *c, const char *fn, int h_rows, const double **dt, int M, const double **t_hist,
                          const double *x, const double *y, const double *phi_Q, const double *phi_T,
                          const vch_opt_params *opts, int n_opts, int order, bool *pgd_out) {
    TANCHK(M == c->M_res, "M differs from the steps of the resident state history");
    TANCHK(n_opts == 1 || n_opts == c->B, "n_opts must be 1 or the context's batch");
    TANCHK(order == 1 || order == 2, "order must be 1 or 2");
    TANCHK(h_rows >= 1 && h_rows <= c->Mmax + 1, "direction rows out of range (1..max_steps+1)");
    for (int b = 0; b < c->B; ++b)
        if (const char *bad = vch_pgd_check_weights(opts, n_opts, b))
            return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: %s", fn, b, bad);
    const bool pgd = c->pgd_ready && c->res_pgd;
    if (pgd) {
        TANCHK(!phi_Q && !phi_T, "the resident problem's targets are used: pass phi_Q = phi_T = NULL");
        if (x) for (int i = 0; i <= c->prm.Nx; ++i) TANCHK(x[i] == c->xg[i], "x differs from the resident problem's grid");
        if (y) for (int j = 0; j <= c->prm.Ny; ++j) TANCHK(y[j] == c->yg[j], "y differs from the resident problem's grid");
        if (!*dt) *dt = c->dt.data();
        if (!*t_hist) *t_hist = c->t_hist.data();
    } else {
        TANCHK(*dt && *t_hist && x && y, "NULL dt, t_hist, x or y without a resident problem");
    }
    for (int k = 0; k < M; ++k) TANCHK((*dt)[k] > 0, "dt must be positive");
    *pgd_out = pgd;
    return 0;
}
// The targets and cost weights of the call on the device: the resident problem's, or the caller's (NULL = zeros).
static int tan_targets(vch2d_ctx *c, bool pgd, const double *x, const double *y, const double *phi_Q, const double *phi_T, int M,
                       const double **pq, const double **pt) {
    *pq = *pt = nullptr;
    if (pgd) {
        *pq = c->phiQ;
        *pt = c->phiT;
        return 0;
    }
    VCHCHK(set_cost_weights(c, x, y));
    if (phi_Q) {
        VCHCHK(ensure_hist(c, &c->phiQ));
        VCHCHK(h2d_hist(c, c->phiQ, phi_Q, M + 1));
        *pq = c->phiQ;
    }
    if (phi_T) {
        VCHCHK(h2d(c, c->phiT, phi_T, c->B));
        *pt = c->phiT;
    }
    return 0;
}

extern "C" int vch2d_second_order(vch2d_ctx *c, const double *h, int h_rows, const double *dt, int M, const double *t_hist,
                                  const double *x, const double *y, const double *phi_Q, const double *phi_T,
                                  const vch_opt_params *opts, int n_opts, int order, double rtol, double *out,
                                  double *dphi_hist_out, double *d2phi_hist_out, vch_stats *stats) {
    CTXCHK(c);
    // everything below is checked before anything is enqueued or any resident state changes
    VCHCHK(tan_check_state(c, __func__));
    ARGCHK(h && opts && out, "NULL h, opts or out");
    bool pgd = false;
    VCHCHK(tan_check_args(c, __func__, h_rows, &dt, M, &t_hist, x, y, phi_Q, phi_T, opts, n_opts, order, &pgd));
    const double *pq = nullptr, *pt = nullptr;
    VCHCHK(tan_targets(c, pgd, x, y, phi_Q, phi_T, M, &pq, &pt));
    // the solves stop at rtol (relative residual); the context's own tolerance comes back on every path out
    const double keep_tol = c->lin_tol;
    c->lin_tol = rtol > 0 ? rtol : 1e-12;
    const int rc = second_order_core(c, h, h_rows, dt, M, t_hist, pq, pt, opts, n_opts, order, out, dphi_hist_out, d2phi_hist_out,
                                     stats);
    c->lin_tol = keep_tol;
    return rc;
}

// ------------------------------------------------------------------------------------
// exact gradient field and Hessian-vector product: the transposed sweep of the tangent march (kernels: "Transposed
// (adjoint) sweep" in vch_kernels2d.h)
// ------------------------------------------------------------------------------------
// What the pieces of a transposed-sweep call share (vch2d_hessvec runs them in one order, vch2d_hess_lanczos in another).
struct HvRun {
    const double *dt;
    int M;
    const double *pq, *pt;
    int g_rows, h_rows;
    std::vector<double> wt;            // trapezoid weights in t; lives until the call's final synchronisation
};
// Tables, counters, refusal cells, the start of the timed span.
static int hv_begin(vch2d_ctx *c, HvRun &r, const double *t_hist, const vch_opt_params *opts, int n_opts) {
    r.wt = trapz_w(t_hist, r.M + 1);
    r.wt.resize((size_t)c->Mmax + 1, 0.0);                       // a direction's rows beyond the march carry no weight
    VCHCHK(write_opt_tab(c, c->seam_tab, opts, n_opts));
    HIPCHK(hipMemcpyAsync(c->hv_wt, r.wt.data(), sizeof(double) * r.wt.size(), hipMemcpyHostToDevice, c->stream));
    VCHCHK(reset_counters(c));
    VCHCHK(fix_check_begin(c));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    c->guess_wr = -1;          // the back substitution keeps no increment for a march's starting guesses
    c->cheb_enq = -1;
    return 0;
}
static const double *hv_rec_of(const vch2d_ctx *c, int n) {
    return c->shift_res ? (const double *)c->shift_hist + (long)n * SHIFT_REC : (const double *)nullptr;
}
// The start of the gradient field.
static int hv_grad_init(vch2d_ctx *c, const HvRun &r) {
    const int u_rows = c->res_pgd ? r.M + 1 : std::min(c->fwd_u_rows, r.M + 1);
    LAUNCH(k_hv_init, c->grid, dim3(NTH), c->G, r.g_rows, u_rows > 0 ? (const double *)c->u_hist : (const double *)nullptr, u_rows,
           (const double *)c->hv_wt, (const double *)c->seam_tab, (const double *)c->W_cost, hist_stride(c), c->hv_G);
    return 0;
}
// The start of H h and the order-1 tangent of the direction in the trial-control scratch, keeping every step's raw solve
// (v_k) and the field after the mean removal (dphi').
static int hv_tangent(vch2d_ctx *c, const HvRun &r) {
    const Geom &G = c->G;
    const int B = c->B, M = r.M, h_rows = r.h_rows;
    const long hs = hist_stride(c), rec_stride = (long)c->Mmax * SHIFT_REC;
    const double *dt = r.dt;
    auto rec_of = [&](int n) { return hv_rec_of(c, n); };
    LAUNCH(k_hv_init, c->grid, dim3(NTH), G, h_rows, (const double *)c->u_trial, h_rows, (const double *)c->hv_wt,
           (const double *)c->seam_tab, (const double *)c->W_cost, hs, c->hv_H);
    double *dphi = c->tmp[0], *dmu = c->tmp[1], *dw[2] = {c->tmp[4], c->tmp[5]};
    for (int k : {0, 1, 4, 5}) HIPCHK(hipMemsetAsync(c->tmp[k], 0, sizeof(double) * B * G.plane, c->stream));
    for (int n = 0; n < M; ++n) {
        const double *phi1 = c->phi_hist + (long)(n + 1) * G.plane;
        const bool live = n < h_rows - 1;           // F2:545-548
        TanRhsArgs a1{dphi, dmu, dw[n & 1], dw[(n + 1) & 1], live ? c->u_trial + (long)n * G.plane : (const double *)nullptr,
                      live ? c->u_trial + (long)(n + 1) * G.plane : (const double *)nullptr, phi1, hs, nullptr, nullptr,
                      nullptr, nullptr, rec_of(n), rec_stride, nullptr};
        LAUNCH((k_tan_rhs<0>), c->grid, dim3(NTH), G, c->P, a1, dt[n], c->Rphi_s, c->rhs_s, c->D_s, c->part);
        VCHCHK(tangent_solve(c, dt[n], phi1, rec_of(n)));
        LAUNCH(k_hv_keep, c->grid, dim3(NTH), G, (const double *)c->xf, (const double *)c->dmu, phi1, hs, rec_of(n), rec_stride,
               (const double *)c->part_mass, c->P.LxLy, fix_check_of(c, n), c->hv_V + (long)n * G.plane, c->hv_DP + (long)(n + 1) * G.plane, dphi,
               dmu);
    }
    return 0;
}
// The sweeps sw0 .. sw1 (0: the gradient, 1: H h) in lockstep: multipliers of the gradient in tmp[0..2], of H h in
// tmp[3..5]; partials of the transposed fix in the two halves of hv_part.  The second sweep needs the first one's xp of
// every step (y^p = -(2/dt) xp): beside the first it reads the solver's output plane; alone it reads xp_cached, the planes
// [M][B][plane] an earlier first sweep left through xp_keep.  The solves are deterministic, so either way gives the same bits.
static int hv_sweeps(vch2d_ctx *c, const HvRun &r, int sw0, int sw1, double *xp_keep, const double *xp_cached) {
    const Geom &G = c->G;
    const int B = c->B, M = r.M;
    const long hs = hist_stride(c), rec_stride = (long)c->Mmax * SHIFT_REC;
    const long pstride = (long)B * c->nblk * NPART;
    const double *dt = r.dt, *pq = r.pq, *pt = r.pt;
    const std::vector<double> &wt = r.wt;
    auto rec_of = [&](int n) { return hv_rec_of(c, n); };
    auto level_of = [&](const double *hist, int lvl) { return hist ? hist + (long)lvl * G.plane : (const double *)nullptr; };
    auto emit = [&](int sw, int k /* the step just solved, M = the start */) -> int {
        const int lvl = k;                                       // the level whose multipliers this launch leaves
        const bool start = k == M;
        const double dtk = start ? 1.0 : dt[k], gdt = c->P.gamma / dtk;
        const int rows = sw == 0 ? r.g_rows : r.h_rows;
        double *out = sw == 0 ? c->hv_G : c->hv_H;
        const bool live = !start && k < rows - 1;                // F2:545-548
        const double *src_a = lvl == 0 ? nullptr : (sw == 0 ? level_of(c->phi_hist, lvl) : level_of(c->hv_DP, lvl));
        HvEmitArgs a{start ? nullptr : (const double *)c->xf, start ? nullptr : (const double *)c->dmu,
                     c->tmp[3 * sw], c->tmp[3 * sw + 1], c->tmp[3 * sw + 2],
                     live ? out + (long)k * G.plane : nullptr, live ? out + (long)(k + 1) * G.plane : nullptr,
                     src_a, (sw == 0 && lvl > 0) ? level_of(pq, lvl) : nullptr, sw == 0 ? pt : nullptr, lvl == M ? 1 : 0, hs,
                     wt[lvl], (const double *)c->seam_tab, (const double *)c->W_cost, (const double *)c->wts_mass,
                     lvl > 0 ? level_of(c->phi_hist, lvl) : nullptr, lvl > 0 ? rec_of(lvl - 1) : nullptr, rec_stride,
                     c->hv_part + sw * pstride, dtk, c->P.tau / dtk + 2.0 * c->P.c2, 0.5 * c->P.kappa,
                     (gdt - 0.5) / (gdt + 0.5), 0.5 / (gdt + 0.5)};
        LAUNCH(k_hv_emit, c->grid, dim3(NTH), G, a);
        return 0;
    };
    for (int sw = sw0; sw <= sw1; ++sw) VCHCHK(emit(sw, M));
    for (int k = M - 1; k >= 0; --k) {
        const double *phi1 = c->phi_hist + (long)(k + 1) * G.plane;
        for (int sw = sw0; sw <= sw1; ++sw) {
            // beside the first sweep, the second's right-hand side reads y^p of the first from the solver's output plane
            // before its own solve reuses it (the emit kernel in between leaves that plane alone)
            const double *xp1 = xp_cached ? xp_cached + (long)k * B * G.plane : (const double *)c->xf;
            HvRhsArgs a{c->tmp[3 * sw], c->tmp[3 * sw + 1], phi1, hs, rec_of(k), rec_stride,
                        (const double *)(c->hv_part + sw * pstride), (const double *)c->wts_mass,
                        sw ? xp1 : nullptr, sw ? (const double *)(c->hv_V + (long)k * G.plane) : nullptr,
                        fix_check_of(c, k)};
            if (sw == 0) LAUNCH((k_hv_rhs<0>), c->grid, dim3(NTH), G, c->P, a, dt[k], c->Rphi_s, c->rhs_s, c->D_s, c->part);
            else LAUNCH((k_hv_rhs<1>), c->grid, dim3(NTH), G, c->P, a, dt[k], c->Rphi_s, c->rhs_s, c->D_s, c->part);
            VCHCHK(tangent_solve(c, dt[k], phi1, nullptr));
            if (sw == 0 && xp_keep)
                HIPCHK(hipMemcpyAsync(xp_keep + (long)k * B * G.plane, c->xf, sizeof(double) * B * G.plane, hipMemcpyDeviceToDevice,
                                      c->stream));
            VCHCHK(emit(sw, k));
        }
    }
    return 0;
}

static int hessvec_core(vch2d_ctx *c, const double *h, int h_rows, int g_rows, const double *dt, int M, const double *t_hist,
                        const double *pq, const double *pt, const vch_opt_params *opts, int n_opts, int order,
                        double *grad_out, double *hv_out, double *dots_out, vch_stats *stats) {
    const Geom &G = c->G;
    const int B = c->B;
    const long hs = hist_stride(c);
    HvRun r{dt, M, pq, pt, g_rows, h_rows, {}};
    if (h) VCHCHK(h2d_hist(c, c->u_trial, h, h_rows));           // the direction lives in the trial-control scratch
    VCHCHK(hv_begin(c, r, t_hist, opts, n_opts));
    VCHCHK(hv_grad_init(c, r));
    if (order == 2) VCHCHK(hv_tangent(c, r));
    VCHCHK(hv_sweeps(c, r, 0, order == 2 ? 1 : 0, nullptr, nullptr));
    if (dots_out) {
        if (h)
            LAUNCH(k_hv_dots, c->grid, dim3(NTH), G, (const double *)c->hv_G, g_rows, (const double *)c->u_trial, h_rows,
                   order == 2 ? (const double *)c->hv_H : (const double *)nullptr, hs, c->hv_part);
        LAUNCH(k_hv_dots_fin, dim3(B), dim3(64), (const double *)c->hv_part, c->nblk, h ? 1 : 0, order == 2 ? 1 : 0, c->hv_dots);
    }
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    std::vector<int> bad(B, -1);
    if (dots_out) HIPCHK(hipMemcpyAsync(dots_out, c->hv_dots, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(bad.data(), c->fix_bad, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
    VCHCHK(sync_state(c));
    if (grad_out) VCHCHK(d2h_hist(c, grad_out, c->hv_G, g_rows));
    if (order == 2) VCHCHK(d2h_hist(c, hv_out, c->hv_H, h_rows));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    fill_stats(c, stats, ms);
    VCHCHK(reset_counters(c));      // the records as the end of a PGD iteration leaves them
    return fix_check_end("vch2d_hessvec", bad);
}

// The block of vch2d_hessvec beside its histories: {partials [2][B][nblk][NPART], time weights [Mmax+1], dots [B][2]}.
static int ensure_hv_part(vch2d_ctx *c, const char *fn) {
    if (c->hv_part) return 0;
    const size_t n = (size_t)2 * c->B * c->nblk * NPART + (size_t)c->Mmax + 1 + 2 * (size_t)c->B;
    if (c->pool.dev(&c->hv_part, n * 8)) {
        (void)hipGetLastError();
        return vch_fail(VCH_ERR_NOMEM, "%s: hipMalloc of the partials failed", fn);
    }
    c->hv_wt = c->hv_part + (size_t)2 * c->B * c->nblk * NPART;
    c->hv_dots = c->hv_wt + c->Mmax + 1;
    return 0;
}

extern "C" int vch2d_hessvec(vch2d_ctx *c, const double *h, int h_rows, int g_rows, const double *dt, int M,
                             const double *t_hist, const double *x, const double *y, const double *phi_Q, const double *phi_T,
                             const vch_opt_params *opts, int n_opts, int order, double rtol, double *grad_out, double *hv_out,
                             double *dots_out, vch_stats *stats) {
    CTXCHK(c);
    // everything below is checked before anything is enqueued, copied or allocated
    VCHCHK(tan_check_state(c, __func__));
    ARGCHK(opts, "NULL opts");
    bool pgd = false;
    VCHCHK(tan_check_args(c, __func__, h ? h_rows : 1, &dt, M, &t_hist, x, y, phi_Q, phi_T, opts, n_opts, order, &pgd));
    ARGCHK(h || order == 1, "NULL h with order 2");
    ARGCHK(order == 1 || hv_out, "NULL hv_out with order 2");
    if (!c->shift_res)
        return vch_fail(VCH_ERR_STATE, "vch2d_hessvec: the resident state history is not one a march of this context wrote");
    if (c->res_pgd) ARGCHK(g_rows == M + 1, "g_rows must be M + 1 about a resident PGD iterate");
    else if (c->fwd_u_rows > 0) ARGCHK(g_rows == std::min(c->fwd_u_rows, M + 1), "g_rows differs from the rows of the march's control");
    else ARGCHK(g_rows >= 1 && g_rows <= M + 1, "g_rows out of range (1..M+1)");
    // lazy storage next: a failed allocation leaves the context as it was
    VCHCHK(ensure_hist(c, &c->u_trial));
    VCHCHK(ensure_hist(c, &c->hv_G));
    if (order == 2) {
        VCHCHK(ensure_hist(c, &c->hv_H));
        VCHCHK(ensure_hist(c, &c->hv_V));
        VCHCHK(ensure_hist(c, &c->hv_DP));
    }
    if (!pgd && phi_Q) VCHCHK(ensure_hist(c, &c->phiQ));
    VCHCHK(ensure_fix_bad(c));
    VCHCHK(ensure_hv_part(c, __func__));
    const double *pq = nullptr, *pt = nullptr;
    VCHCHK(tan_targets(c, pgd, x, y, phi_Q, phi_T, M, &pq, &pt));
    // the solves stop at rtol (relative residual); the context's own tolerance comes back on every path out
    const double keep_tol = c->lin_tol;
    c->lin_tol = rtol > 0 ? rtol : 1e-12;
    const int rc = hessvec_core(c, h, h_rows, g_rows, dt, M, t_hist, pq, pt, opts, n_opts, order, grad_out, hv_out, dots_out, stats);
    c->lin_tol = keep_tol;
    return rc;
}

// ------------------------------------------------------------------------------------
// Lanczos on the reduced Hessian P H P with the basis, the free set and the recurrence on the device (kernels: "Device-
// resident Lanczos" in vch_kernels2d.h)
// ------------------------------------------------------------------------------------
// The block of partials and scalars behind kr_sc, in doubles; S = basis slots (the stride of a partial and of a
// coefficient row), K = entries of alpha / beta per trajectory.
struct KrLayout {
    size_t part, coef1, coef2, ucoef, alpha, beta, look, scal, amax, nfree, lim, stop, total;
};
static KrLayout kr_layout(const vch2d_ctx *c, int S, int K) {
    const size_t B = c->B, nch = ((size_t)c->Mmax + c->kr_lchunk) / c->kr_lchunk;
    KrLayout L;
    size_t at = 0;
    auto take = [&](size_t n) { const size_t o = at; at += n; return o; };
    L.part = take(B * nch * c->nblk * S);
    L.coef1 = take(B * S);
    L.coef2 = take(B * S);
    L.ucoef = take(B * S);
    L.alpha = take(B * K);
    L.beta = take(B * K);
    L.look = take(2 * B);
    L.scal = take(B);
    L.amax = take(B);
    L.nfree = take(B);
    L.lim = take(B);
    L.stop = take(B);
    L.total = at;
    return L;
}
static KrCells kr_cells(const vch2d_ctx *c, const KrLayout &L) {
    double *p = c->kr_sc;
    return KrCells{p + L.coef1, p + L.coef2, p + L.alpha, p + L.beta, p + L.look, p + L.scal, p + L.amax,
                   (long long *)(p + L.nfree), (long long *)(p + L.lim), (long long *)(p + L.stop)};
}
// a look of the Krylov iteration: n doubles behind everything enqueued so far
static int kr_look(vch2d_ctx *c, void *host, const void *dev, size_t bytes) {
    c->n_sync++;
    HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
// The lazy storage of a Krylov call (fn: vch2d_hess_lanczos or vch2d_hess_cg), one group: a refused request gives back what
// this call got and leaves the context usable.  A request for more than the resident storage holds releases that storage
// first.  kr_valid / ncg_valid, in both engines: what an earlier call left resident stays valid until this call has released
// it or has all of its storage, so a refused request leaves the context as it was; then the caller overwrites it.
static int kr_storage(vch2d_ctx *c, const char *fn, int slots, int k, bool want_phiQ) {
    const size_t hist_bytes = (size_t)c->B * (c->Mmax + 1) * c->G.plane * 8;
    if (c->kr_Q && (slots > c->kr_slots || k > c->kr_kcap)) {       // a larger basis than the resident storage holds
        c->kr_valid = c->ncg_valid = false;
        c->pool.drop((void **)&c->kr_sc);
        c->pool.drop((void **)&c->kr_mask);
        c->pool.drop((void **)&c->kr_X);
        c->pool.drop((void **)&c->kr_Q);
        c->kr_slots = c->kr_kcap = 0;
    }
    vch_group g(c->pool);
    VCHCHK(ensure_hist(c, &c->u_trial));
    VCHCHK(ensure_hist(c, &c->hv_G));
    VCHCHK(ensure_hist(c, &c->hv_H));
    VCHCHK(ensure_hist(c, &c->hv_V));
    VCHCHK(ensure_hist(c, &c->hv_DP));
    if (want_phiQ) VCHCHK(ensure_hist(c, &c->phiQ));
    VCHCHK(ensure_fix_bad(c));
    VCHCHK(ensure_hv_part(c, fn));
    if (!c->kr_Q) {
        const KrLayout L = kr_layout(c, slots, k);
        const size_t need = (size_t)slots * hist_bytes + hist_bytes + hist_bytes / 8 + L.total * 8;
        const bool ok = c->pool.dev(&c->kr_Q, (size_t)slots * hist_bytes) == 0 && c->pool.dev(&c->kr_X, hist_bytes) == 0 &&
                        c->pool.dev(&c->kr_mask, hist_bytes / 8) == 0 && c->pool.dev(&c->kr_sc, L.total * 8) == 0;
        if (!ok) {
            (void)hipGetLastError();
            return vch_fail(VCH_ERR_NOMEM,
                            "%s: the Krylov storage needs %zu bytes (%d basis vectors of %zu bytes, one more "
                            "history for the cached sweep, %zu bytes of mask, %zu of partials) and was refused",
                            fn, need, slots, hist_bytes, hist_bytes / 8, L.total * 8);
        }
        c->kr_slots = slots;
        c->kr_kcap = k;
    }
    g.keep();
    c->kr_valid = c->ncg_valid = false;
    return 0;
}
// The arguments of the Krylov kernels over vectors of `levels` rows: vectors first .. first + nv - 1 of a ring of `slots`,
// partials of `pstride` cells per workgroup.
static KrArgs kr_args(const vch2d_ctx *c, int levels, int first, int nv, int slots, int pstride) {
    const long hs = hist_stride(c);
    return KrArgs{c->kr_Q, (long)c->B * hs, hs, levels, c->kr_lchunk, first, nv, slots, pstride, c->kr_mask,
                  kr_cells(c, kr_layout(c, c->kr_slots, c->kr_kcap)).stop};
}

// What vch2d_hess_lanczos and vch2d_hess_cg have in common between kr_open and kr_close.
struct KrCall {
    KrCells cells;
    double *part;                       // the partials: S cells per workgroup, nsum workgroups per trajectory; kgrid: the passes' grid
    long nsum;
    dim3 kgrid;
    int S, u_rows;                      // u_rows: rows of the resident control that bound the free set (u_dev NULL: none)
    const double *u_dev, *pq, *pt;
    std::vector<long long> nfree;
    std::vector<int> bad;               // the mass fix's refusals, read with the call's last look
    double keep_tol;                    // the context's lin_tol while the call runs at rtol
};
// After tan_check_state and the entry's own checks: the rest of the checks, before anything is enqueued, copied or allocated.
// Then the storage of `slots` vectors and k steps, the free set (mask NULL: built from the control and the box at tol; empty_ok:
// an empty one is no error) with its one mask launch, its sum and one look, the targets; the solves stop at rtol until kr_close.
static int kr_open(vch2d_ctx *c, const char *fn, KrCall &K, int slots, int k, bool empty_ok, const double **dt, int M,
                   const double **t_hist, const double *x, const double *y, const double *phi_Q, const double *phi_T,
                   const vch_opt_params *opts, int n_opts, double rtol, const uint8_t *mask, double tol) {
    bool pgd = false;
    VCHCHK(tan_check_args(c, fn, 1, dt, M, t_hist, x, y, phi_Q, phi_T, opts, n_opts, 2, &pgd));
    if (!c->shift_res)
        return vch_fail(VCH_ERR_STATE, "%s: the resident state history is not one a march of this context wrote", fn);
    // the direction has M + 1 rows: the g_rows the rule of vch2d_hessvec must allow
    if (!c->res_pgd && c->fwd_u_rows > 0)
        TANCHK(c->fwd_u_rows >= M + 1, "the march's control has fewer than M + 1 rows");
    const Geom &G = c->G;
    const int B = c->B, levels = M + 1, nch = (levels + c->kr_lchunk - 1) / c->kr_lchunk;
    const long hs = hist_stride(c);
    VCHCHK(kr_storage(c, fn, slots, k, !pgd && phi_Q));
    const KrLayout L = kr_layout(c, c->kr_slots, c->kr_kcap);
    K.cells = kr_cells(c, L);
    K.part = c->kr_sc + L.part;
    K.S = c->kr_slots;
    K.nsum = (long)nch * c->nblk;
    K.kgrid = dim3(c->nblk, nch, B);
    VCHCHK(write_opt_tab(c, c->seam_tab, opts, n_opts));
    if (mask)
        for (int b = 0; b < B; ++b)
            HIPCHK(hipMemcpy2DAsync(c->kr_mask + (size_t)b * hs, (size_t)G.pitch, mask + (size_t)b * levels * G.ns * G.nf, (size_t)G.nf,
                                    (size_t)G.nf, (size_t)G.ns * levels, hipMemcpyHostToDevice, c->stream));
    K.u_rows = c->res_pgd ? levels : std::min(c->fwd_u_rows, levels);
    K.u_dev = K.u_rows > 0 ? (const double *)c->u_hist : (const double *)nullptr;
    LAUNCHC(PC_KRYLOV, k_kr_mask, K.kgrid, dim3(NTH), G, kr_args(c, levels, 0, 0, slots, K.S), K.u_dev, K.u_rows,
            (const double *)c->seam_tab, tol > 0 ? tol : 1e-8, mask ? 0 : 1, c->kr_mask, K.part);
    LAUNCHC(PC_KRYLOV, k_kr_fin, dim3(B), dim3(NTH), K.cells, (const double *)K.part, K.nsum, K.S, 0, 0, 0, k);
    K.nfree.resize(B);
    VCHCHK(kr_look(c, K.nfree.data(), K.cells.nfree, sizeof(long long) * B));
    for (int b = 0; b < B; ++b)
        if (K.nfree[b] < 1 && !empty_ok) return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: the free set is empty", fn, b);
    VCHCHK(tan_targets(c, pgd, x, y, phi_Q, phi_T, M, &K.pq, &K.pt));
    K.bad.assign(B, -1);
    K.keep_tol = c->lin_tol;
    c->lin_tol = rtol > 0 ? rtol : 1e-12;
    return 0;
}
// One product H d into hv_H, d the direction in the trial-control scratch: with the gradient sweep's xp of every step from
// kr_X, or (kr_nocache) with that sweep run again.
static int kr_product(vch2d_ctx *c, const HvRun &r) {
    if (c->kr_nocache) VCHCHK(hv_grad_init(c, r));
    VCHCHK(hv_tangent(c, r));
    return c->kr_nocache ? hv_sweeps(c, r, 0, 1, nullptr, nullptr) : hv_sweeps(c, r, 1, 1, nullptr, c->kr_X);
}
// rc: what the call's own enqueues returned.  The context's own tolerance comes back on every path out.
static int kr_close(vch2d_ctx *c, const char *fn, const KrCall &K, int rc, vch_stats *stats) {
    c->lin_tol = K.keep_tol;
    if (rc < 0) {
        (void)reset_counters(c);    // the records as the end of a PGD iteration leaves them
        return rc;
    }
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev0, c->ev1);
    fill_stats(c, stats, ms);
    if (stats) {                    // the launches and the look of the free set, made before the counters were reset
        stats->launches += 2;
        stats->host_syncs += 1;
    }
    VCHCHK(reset_counters(c));      // the records as the end of a PGD iteration leaves them
    return fix_check_end(fn, K.bad);
}

extern "C" int vch2d_hess_lanczos(vch2d_ctx *c, const double *dt, int M, const double *t_hist, const double *x, const double *y,
                                  const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts, double rtol,
                                  const uint8_t *mask, double tol, const double *q0, int k, int reorth, double *alpha_out,
                                  double *beta_out, int32_t *steps_out, int64_t *n_free_out, vch_stats *stats) {
    CTXCHK(c);
    const char *fn = "vch2d_hess_lanczos";
    // everything below is checked before anything is enqueued, copied or allocated
    VCHCHK(tan_check_state(c, fn));
    TANCHK(opts, "NULL opts");
    TANCHK(q0, "NULL q0");
    TANCHK(alpha_out && beta_out && steps_out && n_free_out, "NULL alpha_out, beta_out, steps_out or n_free_out");
    TANCHK(k >= 1, "k must be >= 1");
    TANCHK(reorth == 0 || reorth == 1, "reorth must be 0 or 1");
    const Geom &G = c->G;
    const int B = c->B, levels = M + 1, slots = reorth ? k + 1 : 3;
    KrCall K;
    VCHCHK(kr_open(c, fn, K, slots, k, false, &dt, M, &t_hist, x, y, phi_Q, phi_T, opts, n_opts, rtol, mask, tol));
    const KrCells &cells = K.cells;
    const int S = K.S;
    auto kr_args = [&](int first, int nv) { return ::kr_args(c, levels, first, nv, slots, S); };
    auto slot_of = [&](int i) { return c->kr_Q + (long)(i % slots) * B * hist_stride(c); };
    std::vector<double> look(2 * (size_t)B);
    int hi = 0;                                     // the highest basis vector stored
    auto run = [&]() -> int {
        HvRun r{dt, M, K.pq, K.pt, levels, levels, {}};
        VCHCHK(h2d_hist(c, c->u_trial, q0, levels));            // the direction lives in the trial-control scratch
        VCHCHK(hv_begin(c, r, t_hist, opts, n_opts));
        // q_0 = P q0 / ||P q0||
        LAUNCHC(PC_KRYLOV, k_kr_start, K.kgrid, dim3(NTH), G, kr_args(0, 0), (const double *)c->u_trial, slot_of(0), K.part);
        LAUNCHC(PC_KRYLOV, k_kr_fin, dim3(B), dim3(NTH), cells, (const double *)K.part, K.nsum, S, 1, 0, 0, k);
        VCHCHK(kr_look(c, look.data(), cells.look, sizeof(double) * 2 * B));
        for (int b = 0; b < B; ++b)
            if (!(look[2 * b] > 0.0) || !std::isfinite(look[2 * b]))
                return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: the start vector vanishes on the free set (or is not finite)", fn, b);
        LAUNCHC(PC_KRYLOV, k_kr_next, K.kgrid, dim3(NTH), G, kr_args(0, 0), (const double *)slot_of(0), (const double *)cells.scal, slot_of(0),
               c->u_trial);
        HIPCHK(hipMemsetAsync(cells.alpha, 0xff, sizeof(double) * 2 * B * c->kr_kcap, c->stream));      // NaN: alpha, then beta
        if (!c->kr_nocache) {           // the gradient sweep once per base point: its xp of every step stays in kr_X
            VCHCHK(hv_grad_init(c, r));
            VCHCHK(hv_sweeps(c, r, 0, 0, c->kr_X, nullptr));
        }
        std::vector<char> active(B, 1);
        for (int b = 0; b < B; ++b) steps_out[b] = 0;
        for (int j = 0; j < k; ++j) {
            VCHCHK(kr_product(c, r));
            // w = P H q_j in hv_H; classical Gram-Schmidt twice against q_first .. q_j
            const int first = reorth ? 0 : std::max(j - 1, 0), nv = j + 1 - first;
            const KrArgs a = kr_args(first % slots, nv);
            LAUNCHC(PC_KRYLOV, (k_kr_pass<0>), K.kgrid, dim3(NTH), G, a, c->hv_H, (const double *)nullptr, K.part);
            LAUNCHC(PC_KRYLOV, k_kr_fin, dim3(B), dim3(NTH), cells, (const double *)K.part, K.nsum, S, 2, nv, j, k);
            LAUNCHC(PC_KRYLOV, (k_kr_pass<1>), K.kgrid, dim3(NTH), G, a, c->hv_H, (const double *)cells.coef1, K.part);
            LAUNCHC(PC_KRYLOV, k_kr_fin, dim3(B), dim3(NTH), cells, (const double *)K.part, K.nsum, S, 3, nv, j, k);
            LAUNCHC(PC_KRYLOV, (k_kr_pass<2>), K.kgrid, dim3(NTH), G, a, c->hv_H, (const double *)cells.coef2, K.part);
            LAUNCHC(PC_KRYLOV, k_kr_fin, dim3(B), dim3(NTH), cells, (const double *)K.part, K.nsum, S, 4, nv, j, k);
            LAUNCHC(PC_KRYLOV, k_kr_next, K.kgrid, dim3(NTH), G, a, (const double *)c->hv_H, (const double *)cells.scal, slot_of(j + 1), c->u_trial);
            hi = j + 1;
            // the one look of the step: beta_j and the stop cell of every trajectory
            VCHCHK(kr_look(c, look.data(), cells.look, sizeof(double) * 2 * B));
            bool any = false;
            for (int b = 0; b < B; ++b) {
                if (!active[b]) continue;
                steps_out[b] = j + 1;
                if (look[2 * b + 1] != 0.0) active[b] = 0;
                else any = true;
            }
            if (!any) break;
        }
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        for (int b = 0; b < B; ++b) {
            HIPCHK(hipMemcpyAsync(alpha_out + (size_t)b * k, cells.alpha + (size_t)b * k, sizeof(double) * k, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(beta_out + (size_t)b * k, cells.beta + (size_t)b * k, sizeof(double) * k, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(hipMemcpyAsync(K.bad.data(), c->fix_bad, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
        VCHCHK(sync_state(c));
        return 0;
    };
    VCHCHK(kr_close(c, fn, K, run(), stats));
    int smin = steps_out[0];
    for (int b = 0; b < B; ++b) {
        n_free_out[b] = K.nfree[b];
        smin = std::min(smin, (int)steps_out[b]);
    }
    c->kr_valid = true;
    c->kr_levels = levels;
    c->kr_run_slots = slots;
    c->kr_min_steps = smin;
    c->kr_window = reorth ? INT32_MAX : (hi <= 2 ? 3 : 0);   // three resident vectors: q_0 is gone once q_3 is stored
    return 0;
}

extern "C" int vch2d_krylov_vector(vch2d_ctx *c, const double *coef, int m, double *out) {
    CTXCHK(c);
    ARGCHK(coef && out, "NULL coef or out");
    ARGCHK(m >= 1, "m must be >= 1");
    if (!c->kr_valid || !c->kr_Q || !c->hv_H)
        return vch_fail(VCH_ERR_STATE, "vch2d_krylov_vector: no resident basis (call vch2d_hess_lanczos first)");
    if (m > c->kr_window)
        return vch_fail(VCH_ERR_STATE, "vch2d_krylov_vector: m = %d exceeds the %d vectors a run without reorthogonalisation still holds",
                        m, c->kr_window);
    ARGCHK(m <= c->kr_min_steps + 1, "m exceeds the smallest step count of the batch plus one");
    const int B = c->B, S = c->kr_slots, levels = c->kr_levels;
    double *ucoef = c->kr_sc + kr_layout(c, c->kr_slots, c->kr_kcap).ucoef;
    HIPCHK(hipMemcpy2DAsync(ucoef, sizeof(double) * S, coef, sizeof(double) * m, sizeof(double) * m, (size_t)B, hipMemcpyHostToDevice,
                            c->stream));
    const int nch = (levels + c->kr_lchunk - 1) / c->kr_lchunk;
    LAUNCH(k_kr_lincomb, dim3(c->nblk, nch, B), dim3(NTH), c->G, kr_args(c, levels, 0, m, c->kr_run_slots, S), (const double *)ucoef, c->hv_H);
    return d2h_hist(c, out, c->hv_H, levels);
}

// ------------------------------------------------------------------------------------
// Newton-CG on the free set: (preconditioned) conjugate gradients on P H P x = P b with x, r, p, the free set and the
// recurrence on the device (kernels: "Device-resident Newton-CG" in vch_kernels2d.h).  The storage, the
// mask launch and the sweeps are those of vch2d_hess_lanczos without reorthogonalisation.
// ------------------------------------------------------------------------------------
// The body of vch2d_hess_cg, shared with the rounds of vch2d_pgd_newton.  fn: the entry point the messages name.
// empty_ok (the Newton rounds): a trajectory with an empty free set is no error; with P b = 0 the start gives it zero steps,
// VCH_CG_CONVERGED and x = 0.
// radius (host [B], or NULL): the trust region of vch2d_hess_cg_tr, k_ncg_fin_tr in place of k_ncg_fin and xnorm_out [B] =
// ||x||_D by the recurrence (0 for P b = 0); NULL enqueues the launches, looks and copies of vch2d_hess_cg exactly.
// The right-hand side a Newton-CG call builds itself and its free set are those of the L1 functional: about the resident
// iterate of a problem that has a trajectory in a group mode they would belong to another cost.
static int gp2_refuse(const vch2d_ctx *c, const char *fn, bool resident) {
    if (resident && c->pgd_ready && gp2_group(c))
        return vch_fail(VCH_ERR_STATE, "%s: the resident problem has a trajectory in a directional-sparsity mode; the sign term and "
                        "the free set of this call are those of the L1 functional", fn);
    return 0;
}

static int hess_cg_core(vch2d_ctx *c, const char *fn, bool empty_ok, const double *dt, int M, const double *t_hist, const double *x,
                        const double *y, const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts,
                        double rtol, const uint8_t *mask, double tol, const double *rhs, int k, double cg_tol, int precond,
                        double *resid_out, double *curv_out, double *pred_out, double *rnorm0_out, int32_t *steps_out,
                        int32_t *status_out, int64_t *n_free_out, vch_stats *stats, const double *radius = nullptr,
                        double *xnorm_out = nullptr) {
    // everything below is checked before anything is enqueued, copied or allocated
    VCHCHK(gp2_refuse(c, fn, !rhs && c->res_pgd));
    VCHCHK(tan_check_state(c, fn));
    TANCHK(opts, "NULL opts");
    TANCHK(resid_out && curv_out && pred_out && rnorm0_out && steps_out && status_out && n_free_out,
           "NULL resid_out, curv_out, pred_out, rnorm0_out, steps_out, status_out or n_free_out");
    TANCHK(k >= 1, "k must be >= 1");
    TANCHK(precond == 0 || precond == 1, "precond must be 0 or 1");
    TANCHK(std::isfinite(cg_tol), "cg_tol must be finite");
    if (radius)
        for (int b = 0; b < c->B; ++b)
            if (!(radius[b] > 0.0))
                return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: radius %g must be > 0 (+inf allowed, NaN not)", fn, b, radius[b]);
    KrCall K;
    VCHCHK(kr_open(c, fn, K, 3, k, empty_ok, &dt, M, &t_hist, x, y, phi_Q, phi_T, opts, n_opts, rtol, mask, tol));
    const Geom &G = c->G;
    const int B = c->B, levels = M + 1, S = K.S;
    const KrCells &cells = K.cells;
    // the cells of the iteration in the block of the Lanczos scalars: resid, curv where alpha, beta live
    const NcgCells nc{cells.alpha, cells.beta, cells.look, cells.scal, cells.amax, cells.coef1, cells.coef1 + B, cells.coef1 + 2 * B,
                      cells.lim, cells.stop};
    // the six cells of the trust region where CG leaves the Lanczos block unused: three in coef2, three in ucoef, each
    // B * S doubles with S >= 3 (kr_open asked for three slots, and kr_storage keeps resident storage only if it holds at
    // least what is asked).  ucoef is otherwise written by vch2d_krylov_vector alone, whose basis this call invalidates.
    double *const ucoef = c->kr_sc + kr_layout(c, c->kr_slots, c->kr_kcap).ucoef;
    const NtrCells tc{cells.coef2, cells.coef2 + B, cells.coef2 + 2 * B, ucoef, ucoef + B, (long long *)(ucoef + 2 * B)};
    std::vector<double> xx(radius ? B : 0);
    const KrArgs a = kr_args(c, levels, 0, 0, 3, S);
    const double stop_at = cg_tol > 0 ? cg_tol : 1e-8;
    std::vector<double> look(2 * (size_t)B);
    std::vector<long long> steps(B), stop(B);
    auto run = [&]() -> int {
        HvRun r{dt, M, K.pq, K.pt, levels, levels, {}};
        if (radius) HIPCHK(hipMemcpyAsync(cells.coef2, radius, sizeof(double) * B, hipMemcpyHostToDevice, c->stream));
        if (rhs) VCHCHK(h2d_hist(c, c->u_trial, rhs, levels));   // through the trial-control scratch, which then holds p
        VCHCHK(hv_begin(c, r, t_hist, opts, n_opts));
        // the gradient sweep once per base point: its xp of every step stays in kr_X, its field is the Newton right-hand
        // side's; an uploaded right-hand side is looked at first
        auto grad_sweep = [&]() -> int {
            VCHCHK(hv_grad_init(c, r));
            VCHCHK(hv_sweeps(c, r, 0, 0, c->kr_nocache ? nullptr : c->kr_X, nullptr));
            return 0;
        };
        if (!rhs) {
            VCHCHK(grad_sweep());
            LAUNCHC(PC_KRYLOV, (k_ncg_start<1>), K.kgrid, dim3(NTH), G, a, (const double *)c->hv_G, K.u_dev, K.u_rows, (const double *)c->hv_wt,
                    (const double *)c->W_cost, (const double *)c->seam_tab, precond, c->u_trial, K.part);
        } else {
            LAUNCHC(PC_KRYLOV, (k_ncg_start<0>), K.kgrid, dim3(NTH), G, a, (const double *)c->u_trial, K.u_dev, K.u_rows,
                    (const double *)c->hv_wt, (const double *)c->W_cost, (const double *)c->seam_tab, precond, c->u_trial, K.part);
        }
        if (radius) LAUNCHC(PC_KRYLOV, k_ncg_fin_tr, dim3(B), dim3(NTH), nc, tc, (const double *)K.part, K.nsum, S, 1, 0, k, stop_at);
        else LAUNCHC(PC_KRYLOV, k_ncg_fin, dim3(B), dim3(NTH), nc, (const double *)K.part, K.nsum, S, 1, 0, k, stop_at);
        HIPCHK(hipMemsetAsync(nc.resid, 0xff, sizeof(double) * 2 * B * c->kr_kcap, c->stream));         // NaN: resid, then curv
        VCHCHK(kr_look(c, look.data(), nc.look, sizeof(double) * 2 * B));
        bool any = false;
        for (int b = 0; b < B; ++b) {
            if (!std::isfinite(look[2 * b]))
                return vch_fail(VCH_ERR_ARG, "%s: trajectory %d: the right-hand side is not finite on the free set", fn, b);
            any = any || look[2 * b + 1] == 0.0;
        }
        if (any && rhs && !c->kr_nocache) VCHCHK(grad_sweep());
        for (int j = 0; any && j < k; ++j) {
            VCHCHK(kr_product(c, r));
            // H p in hv_H
            LAUNCHC(PC_KRYLOV, k_ncg_curv, K.kgrid, dim3(NTH), G, a, (const double *)c->hv_H, (const double *)c->hv_wt,
                    (const double *)c->W_cost, precond, K.part);
            if (radius) LAUNCHC(PC_KRYLOV, k_ncg_fin_tr, dim3(B), dim3(NTH), nc, tc, (const double *)K.part, K.nsum, S, 2, j, k, stop_at);
            else LAUNCHC(PC_KRYLOV, k_ncg_fin, dim3(B), dim3(NTH), nc, (const double *)K.part, K.nsum, S, 2, j, k, stop_at);
            LAUNCHC(PC_KRYLOV, k_ncg_update, K.kgrid, dim3(NTH), G, a, (const double *)c->hv_H, (const double *)nc.alpha,
                    (const double *)c->hv_wt, (const double *)c->W_cost, precond, K.part);
            if (radius) LAUNCHC(PC_KRYLOV, k_ncg_fin_tr, dim3(B), dim3(NTH), nc, tc, (const double *)K.part, K.nsum, S, 3, j, k, stop_at);
            else LAUNCHC(PC_KRYLOV, k_ncg_fin, dim3(B), dim3(NTH), nc, (const double *)K.part, K.nsum, S, 3, j, k, stop_at);
            if (j + 1 < k)
                LAUNCHC(PC_KRYLOV, k_ncg_dir, K.kgrid, dim3(NTH), G, a, (const double *)nc.beta, (const double *)c->hv_wt,
                        (const double *)c->W_cost, precond, c->u_trial);
            // the one look of the step: the residual and the stop cell of every trajectory
            VCHCHK(kr_look(c, look.data(), nc.look, sizeof(double) * 2 * B));
            any = false;
            for (int b = 0; b < B; ++b) any = any || look[2 * b + 1] == 0.0;
        }
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        if (radius) HIPCHK(hipMemcpyAsync(xx.data(), tc.xx, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
        for (int b = 0; b < B; ++b) {
            HIPCHK(hipMemcpyAsync(resid_out + (size_t)b * k, nc.resid + (size_t)b * k, sizeof(double) * k, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(curv_out + (size_t)b * k, nc.curv + (size_t)b * k, sizeof(double) * k, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(hipMemcpyAsync(pred_out, nc.pred, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(rnorm0_out, nc.rnorm0, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(steps.data(), nc.steps, sizeof(long long) * B, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(stop.data(), nc.stop, sizeof(long long) * B, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(K.bad.data(), c->fix_bad, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
        VCHCHK(sync_state(c));
        return 0;
    };
    VCHCHK(kr_close(c, fn, K, run(), stats));
    for (int b = 0; b < B; ++b) {
        n_free_out[b] = K.nfree[b];
        steps_out[b] = (int32_t)steps[b];
        status_out[b] = (int32_t)stop[b];           // 0: still running after k steps, VCH_CG_LIMIT
        if (radius) xnorm_out[b] = std::sqrt(xx[b]);
    }
    c->ncg_valid = true;
    c->ncg_levels = levels;
    return 0;
}

extern "C" int vch2d_hess_cg(vch2d_ctx *c, const double *dt, int M, const double *t_hist, const double *x, const double *y,
                             const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts, double rtol,
                             const uint8_t *mask, double tol, const double *rhs, int k, double cg_tol, int precond,
                             double *resid_out, double *curv_out, double *pred_out, double *rnorm0_out, int32_t *steps_out,
                             int32_t *status_out, int64_t *n_free_out, vch_stats *stats) {
    CTXCHK(c);
    return hess_cg_core(c, __func__, false, dt, M, t_hist, x, y, phi_Q, phi_T, opts, n_opts, rtol, mask, tol, rhs, k, cg_tol, precond,
                        resid_out, curv_out, pred_out, rnorm0_out, steps_out, status_out, n_free_out, stats);
}

extern "C" int vch2d_hess_cg_tr(vch2d_ctx *c, const double *dt, int M, const double *t_hist, const double *x, const double *y,
                                const double *phi_Q, const double *phi_T, const vch_opt_params *opts, int n_opts, double rtol,
                                const uint8_t *mask, double tol, const double *rhs, int k, double cg_tol, int precond,
                                double *resid_out, double *curv_out, double *pred_out, double *rnorm0_out, int32_t *steps_out,
                                int32_t *status_out, int64_t *n_free_out, vch_stats *stats, const double *radius,
                                double *xnorm_out) {
    CTXCHK(c);
    if (!radius || !xnorm_out) return vch_fail(VCH_ERR_ARG, "%s: NULL radius or xnorm_out", __func__);
    return hess_cg_core(c, __func__, false, dt, M, t_hist, x, y, phi_Q, phi_T, opts, n_opts, rtol, mask, tol, rhs, k, cg_tol, precond,
                        resid_out, curv_out, pred_out, rnorm0_out, steps_out, status_out, n_free_out, stats, radius, xnorm_out);
}

extern "C" int vch2d_cg_vector(vch2d_ctx *c, int which, double *out) {
    CTXCHK(c);
    ARGCHK(out, "NULL out");
    ARGCHK(which >= 0 && which <= 2, "which must be 0 (x), 1 (r) or 2 (p)");
    if (!c->ncg_valid || !c->kr_Q)
        return vch_fail(VCH_ERR_STATE, "vch2d_cg_vector: no resident vectors (call vch2d_hess_cg first)");
    return d2h_hist(c, out, c->kr_Q + (long)which * c->B * hist_stride(c), c->ncg_levels);
}

// ------------------------------------------------------------------------------------
// Damped Newton rounds on the free set about the resident PGD iterate (kernels: "Damped Newton rounds" in vch_kernels2d.h,
// verdicts: vch_newton.h)
// ------------------------------------------------------------------------------------
// The trial control of the step lengths s_host [B] into the trial-control scratch, about the resident control, the x, the
// free set and the box table the last Newton-CG solve left; skip (device flags, or NULL) leaves a trajectory alone.  The
// partials and the sums go through the cost scratch; sums_out [B][4] = {sum (t - u)^2, sum u^2, pinned, clipped} after one
// look (the cells of a skipped trajectory are not written).
static int newton_trial_core(vch2d_ctx *c, const double *s_host, const int *skip, double *sums_out) {
    const int B = c->B, levels = c->ncg_levels;
    VCHCHK(ensure_cost_bufs(c));
    const int nch = (levels + c->kr_lchunk - 1) / c->kr_lchunk;
    const KrArgs a = kr_args(c, levels, 0, 0, 3, 4);        // partials of four sums, whatever the basis holds
    const int u_rows = c->res_pgd ? levels : std::min(c->fwd_u_rows, levels);
    HIPCHK(hipMemcpyAsync(c->alpha_dev, s_host, sizeof(double) * B, hipMemcpyHostToDevice, c->stream));
    LAUNCHC(PC_KRYLOV, k_nt_trial, dim3(c->nblk, nch, B), dim3(NTH), c->G, a, u_rows > 0 ? (const double *)c->u_hist : (const double *)nullptr,
            u_rows, (const double *)c->alpha_dev, (const double *)c->seam_tab, skip, c->u_trial, c->cost_part);
    LAUNCHC(PC_KRYLOV, k_nt_fin, dim3(B), dim3(NTH), (const double *)c->cost_part, (long)nch * c->nblk, skip, c->cost_lvl);
    VCHCHK(kr_look(c, c->cost_lvl_host, c->cost_lvl, sizeof(double) * 4 * B));
    memcpy(sums_out, c->cost_lvl_host, sizeof(double) * 4 * B);
    return 0;
}

extern "C" int vch2d_newton_trial(vch2d_ctx *c, const double *s, double *u_out, double *chg_out, int64_t *counts_out) {
    CTXCHK(c);
    ARGCHK(s && chg_out && counts_out, "NULL s, chg_out or counts_out");
    for (int b = 0; b < c->B; ++b) ARGCHK(std::isfinite(s[b]) && s[b] > 0, "s must be finite and > 0");
    VCHCHK(gp2_refuse(c, "vch2d_newton_trial", true));
    if (!c->ncg_valid || !c->kr_Q || !c->u_trial)
        return vch_fail(VCH_ERR_STATE, "vch2d_newton_trial: no resident vectors (call vch2d_hess_cg first)");
    std::vector<double> sums(4 * (size_t)c->B);
    VCHCHK(newton_trial_core(c, s, nullptr, sums.data()));
    for (int b = 0; b < c->B; ++b) {
        chg_out[2 * b] = sums[4 * b];
        chg_out[2 * b + 1] = sums[4 * b + 1];
        counts_out[2 * b] = (int64_t)sums[4 * b + 2];
        counts_out[2 * b + 1] = (int64_t)sums[4 * b + 3];
    }
    return u_out ? d2h_hist(c, u_out, c->u_trial, c->ncg_levels) : 0;
}

// The engine's side of the Newton and trust-region rounds (vch_newton.h) about the resident PGD iterate; sec = {solves, trial
// controls, marches, costs}.
struct PgdRounds {
    vch2d_ctx *c;
    const char *fn;
    int M, k, precond;
    double cg_tol, tol, rtol;
    std::vector<double> resid, curv, Jt;
    double sec[4];
    int solve(double *pred, double *rnorm0, int32_t *steps, int32_t *status, int64_t *n_free) {
        vch_stats st;
        VCHCHK(hess_cg_core(c, fn, true, nullptr, M, nullptr, nullptr, nullptr, nullptr, nullptr, c->opts.data(), c->B, rtol, nullptr,
                            tol, nullptr, k, cg_tol, precond, resid.data(), curv.data(), pred, rnorm0, steps, status, n_free, &st));
        sec[0] += st.seconds;
        return 0;
    }
    // the trust-region rounds: the Steihaug solve inside radius [B]
    int solve(const double *radius, double *pred, double *rnorm0, int32_t *steps, int32_t *status, int64_t *n_free, double *xnorm) {
        vch_stats st;
        VCHCHK(hess_cg_core(c, fn, true, nullptr, M, nullptr, nullptr, nullptr, nullptr, nullptr, c->opts.data(), c->B, rtol, nullptr,
                            tol, nullptr, k, cg_tol, precond, resid.data(), curv.data(), pred, rnorm0, steps, status, n_free, &st,
                            radius, xnorm));
        sec[0] += st.seconds;
        return 0;
    }
    // the trust-region rounds' one trial at s = 1
    int trial(const std::vector<int> &decided, double *sums, double *c_new) {
        return trial(decided, std::vector<double>(c->B, 1.0), sums, c_new);
    }
    double cost(int b) const { return c->J_host[5 * b + 4]; }
    int trial(const std::vector<int> &decided, const std::vector<double> &s, double *sums, double *c_new) {
        VCHCHK(reset_counters(c));
        VCHCHK(freeze(c, decided));
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        VCHCHK(newton_trial_core(c, s.data(), (const int *)c->frozen_dev, sums));
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        sec[1] += elapsed_s(c, c->ev0, c->ev1);
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        HIPCHK(hipMemcpyAsync(c->phi_s, c->phi0, sizeof(double) * c->B * c->G.plane, hipMemcpyDeviceToDevice, c->stream));
        VCHCHK(forward_core(c, c->u_trial, M + 1, c->dt.data(), M, c->phi_trial));
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        sec[2] += elapsed_s(c, c->ev0, c->ev1);
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        VCHCHK(cost_core(c, c->phi_trial, c->u_trial, c->phiQ, c->phiT, false, M, c->t_hist.data(), c->opts.data(), Jt.data(), nullptr, c->B));
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        sec[3] += elapsed_s(c, c->ev0, c->ev1);
        for (int b = 0; b < c->B; ++b) c_new[b] = Jt[5 * b + 4];
        return 0;
    }
    int accept(int b, double c_new) {
        std::copy_n(&Jt[5 * b], 5, &c->J_host[5 * b]);
        c->pgd.cost[b] = c_new;
        VCHCHK(copy_traj(c, c->u_hist, c->u_trial, b, M + 1));
        VCHCHK(copy_traj(c, c->phi_hist, c->phi_trial, b, M + 1));
        return copy_traj_shifts(c, b);
    }
    int after_trial() { return 0; }
    int after_round() { return reset_counters(c); }
};

extern "C" int vch2d_pgd_newton(vch2d_ctx *c, int n_rounds, int k, double cg_tol, int precond, double tol, double rtol,
                                int max_halvings, double *cost_out, double *cost_new_out, double *s_out, double *pred_out,
                                double *rnorm0_out, int32_t *halvings_out, int32_t *cg_steps_out, int32_t *cg_status_out,
                                int32_t *status_out, int64_t *counts_out, double *seconds_out) {
    CTXCHK(c);
    // everything below is checked before anything is enqueued, copied or allocated
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch2d_pgd_newton: call vch2d_pgd_init first");
    VCHCHK(gp2_refuse(c, "vch2d_pgd_newton", true));
    if (!c->res_pgd || !c->shift_res || c->M_res < 1)
        return vch_fail(VCH_ERR_STATE, "vch2d_pgd_newton: the resident state history is no longer the PGD iterate's (call vch2d_pgd_init again)");
    const char *fn = "vch2d_pgd_newton";
    const int B = c->B, M = c->M_res;
    const vch_newton_call call{B, n_rounds, k, cg_tol, precond, max_halvings, cost_out, cost_new_out, s_out, pred_out, rnorm0_out,
                               halvings_out, cg_steps_out, cg_status_out, status_out, counts_out};
    if (const char *bad = vch_newton_check(call)) return vch_fail(VCH_ERR_ARG, "%s: %s", fn, bad);
    // the engine's side of the rounds (vch_newton.h)
    PgdRounds eng{c, fn, M, k, precond, cg_tol, tol, rtol, std::vector<double>((size_t)B * k), std::vector<double>((size_t)B * k),
                  std::vector<double>(5 * (size_t)B), {0, 0, 0, 0}};
    bool moved = false;
    const int rc = vch_newton_rounds(eng, call, moved);
    if (moved) c->pgd_r_valid = false;      // r_hist is the adjoint of an iterate that has been replaced
    if (rc < 0) (void)reset_counters(c);
    HIPCHK(hipMemcpyAsync(c->J_dev, c->J_host.data(), sizeof(double) * 5 * B, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (rc >= 0 && seconds_out) memcpy(seconds_out, eng.sec, sizeof(eng.sec));
    return rc;
}

// ------------------------------------------------------------------------------------
// Trust-region (Steihaug) Newton-CG rounds on the free set about the resident PGD iterate (kernels: k_ncg_fin_tr in
// vch_kernels2d.h, verdicts: vch_trust_state in vch_newton.h)
// ------------------------------------------------------------------------------------
extern "C" int vch2d_pgd_trust(vch2d_ctx *c, int n_rounds, int k, double cg_tol, int precond, double tol, double rtol,
                               const double *radius0, double radius_max, double radius_min, double *cost_out, double *cost_new_out,
                               double *pred_out, double *rnorm0_out, double *radius_out, double *ratio_out, double *xnorm_out,
                               int32_t *cg_steps_out, int32_t *cg_status_out, int32_t *status_out, int64_t *counts_out,
                               double *seconds_out) {
    CTXCHK(c);
    // everything below is checked before anything is enqueued, copied or allocated
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch2d_pgd_trust: call vch2d_pgd_init first");
    VCHCHK(gp2_refuse(c, "vch2d_pgd_trust", true));
    if (!c->res_pgd || !c->shift_res || c->M_res < 1)
        return vch_fail(VCH_ERR_STATE, "vch2d_pgd_trust: the resident state history is no longer the PGD iterate's (call vch2d_pgd_init again)");
    const char *fn = "vch2d_pgd_trust";
    const int B = c->B, M = c->M_res;
    const vch_trust_call call{B, n_rounds, k, cg_tol, precond, radius0, radius_max, radius_min, cost_out, cost_new_out, pred_out,
                              rnorm0_out, radius_out, ratio_out, xnorm_out, cg_steps_out, cg_status_out, status_out, counts_out};
    if (const char *bad = vch_trust_check(call)) return vch_fail(VCH_ERR_ARG, "%s: %s", fn, bad);
    PgdRounds eng{c, fn, M, k, precond, cg_tol, tol, rtol, std::vector<double>((size_t)B * k), std::vector<double>((size_t)B * k),
                  std::vector<double>(5 * (size_t)B), {0, 0, 0, 0}};
    bool moved = false;
    const int rc = vch_trust_rounds(eng, call, moved);
    if (moved) c->pgd_r_valid = false;      // r_hist is the adjoint of an iterate that has been replaced
    if (rc < 0) (void)reset_counters(c);
    HIPCHK(hipMemcpyAsync(c->J_dev, c->J_host.data(), sizeof(double) * 5 * B, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (rc >= 0 && seconds_out) memcpy(seconds_out, eng.sec, sizeof(eng.sec));
    return rc;
}

extern "C" int vch2d_mass_shifts(vch2d_ctx *c, double *out) {
    CTXCHK(c);
    ARGCHK(out, "NULL out");
    if (c->M_res < 1 || !c->phi_hist || !c->shift_res)
        return vch_fail(VCH_ERR_STATE, "vch2d_mass_shifts: no resident state history that a march of this context wrote");
    const int B = c->B, M = c->M_res;
    std::vector<double> rec((size_t)B * c->Mmax * SHIFT_REC);
    HIPCHK(hipMemcpyAsync(rec.data(), c->shift_hist, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < B; ++b)
        for (int n = 0; n < M; ++n) out[(size_t)b * M + n] = rec[((size_t)b * c->Mmax + n) * SHIFT_REC];
    return M;
}

extern "C" int vch2d_pgd_cost_dev(vch2d_ctx *c, double **ptr_dev) {
    CTXCHK(c);
    ARGCHK(ptr_dev, "NULL ptr_dev");
    if (!c->pgd_ready) return vch_fail(VCH_ERR_STATE, "vch2d_pgd_cost_dev: call vch2d_pgd_init first");
    *ptr_dev = c->J_dev;
    return 0;
}

// ------------------------------------------------------------------------------------
// in-situ kernel timing (HIP events on the engine stream) for bench.py's roofline leg
// ------------------------------------------------------------------------------------
extern "C" int vch2d_prof_begin(vch2d_ctx *c, int max_launches) {
    CTXCHK(c);
    ARGCHK(max_launches >= 1, "max_launches must be >= 1");
    while (c->prof_ev.size() < (size_t)2 * max_launches) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        c->prof_ev.push_back(e);
    }
    c->prof_used = 0;
    c->prof_cls.clear();
    c->prof_on = true;
    // calibration: event pairs around an empty kernel (class 14), so that the caller can take the pair's own cost off
    for (int k = 0; k < 256; ++k) LAUNCHC(PC_NOOP, k_noop, dim3(1), dim3(64));
    return 0;
}

extern "C" int vch2d_prof_end(vch2d_ctx *c, double *ms_out, int64_t *count_out, int ncls) {
    CTXCHK(c);
    ARGCHK(ms_out && count_out && ncls >= 1, "NULL output");
    c->prof_on = false;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < ncls; ++k) { ms_out[k] = 0.0; count_out[k] = 0; }
    for (size_t i = 0; i < c->prof_cls.size(); ++i) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
        int k = c->prof_cls[i];
        if (k < ncls) { ms_out[k] += ms; count_out[k]++; }
    }
    return (int)c->prof_cls.size();
}

extern "C" int vch2d_prof_spans(vch2d_ctx *c, int32_t *cls_out, float *ms_out, int cap) {
    CTXCHK(c);
    ARGCHK(cls_out && ms_out && cap >= 0, "NULL output");
    if (c->prof_on) return vch_fail(VCH_ERR_STATE, "vch2d_prof_spans: call vch2d_prof_end first");
    const int n = (int)std::min<size_t>(c->prof_cls.size(), (size_t)cap);
    for (int i = 0; i < n; ++i) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
        cls_out[i] = c->prof_cls[i];
        ms_out[i] = ms;
    }
    return (int)c->prof_cls.size();
}

extern "C" int vch2d_counters(vch2d_ctx *c, int64_t *out) {
    CTXCHK(c);
    ARGCHK(out, "NULL out");
    out[0] = c->tot_launch + c->n_launch;
    out[1] = c->tot_sync + c->n_sync;
    return 0;
}

extern "C" int vch2d_uses_fft(const vch2d_ctx *c) { return c ? (c->use_fft ? 1 : 0) : VCH_ERR_ARG; }


