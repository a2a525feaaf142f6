// vch_pgd.h — the line-search state machine of the device-resident PGD loops (G1:74-113, 365-465; G2:71-146, 295-382).
// Host arithmetic only (no HIP, no I/O): both engines act on its verdicts, tests/pgd_replay_main.cpp replays it on the CPU.
#pragma once
#include "../../include/vch.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

struct vch_pgd_rule {
    int rounds;                 // trial marches per iteration at most; the last one is taken whether it descends or not
    int count0;                 // an accept in round r is reported as r + count0 (1D `trials`, 2D `attempts`)
    double beta;                // alpha *= beta after a rejected round, and once more when the last round is taken without descent
    double grow;                // alpha_prev = min(alpha_max, alpha_k * grow) ...
    double plateau_tol;         // ... or * plateau_boost once |J_k - J_{k-1}| < plateau_tol plateau_len times in a row
    int plateau_len;
    double plateau_boost;
    double stop_change;         // stop: relative control change < stop_change and k > stop_k
    int stop_k;
    bool stop_keeps_state;      // on a stop u is taken, the state history and the stored cost keep the previous iterate (G1:462-465)
};
constexpr vch_pgd_rule VCH_PGD_1D = {5, 1, 0.8, 1.2, 1e-7, 10, 2.0, 1e-5, 10, true};     // round 0 is trial 1 (G1:74, 383)
constexpr vch_pgd_rule VCH_PGD_2D = {11, 0, 0.8, 1.2, 1e-5, 5, 1.5, 1e-5, 20, false};    // round 0 optimistic, 1..10 backtracking

inline const vch_opt_params &vch_pgd_opt(const vch_opt_params *opts, int n_opts, int b) { return opts[n_opts == 1 ? 0 : b]; }
// nullptr, or what is wrong with trajectory b's weights (all that *_second_order reads) / with its parameters and alpha0
inline const char *vch_pgd_check_weights(const vch_opt_params *opts, int n_opts, int b) {
    const vch_opt_params &o = vch_pgd_opt(opts, n_opts, b);
    return std::isfinite(o.b1) && std::isfinite(o.b2) && std::isfinite(o.b3) ? nullptr : "b1, b2, b3 must be finite";
}
inline const char *vch_pgd_check(const vch_opt_params *opts, int n_opts, const double *alpha0, int b) {
    const vch_opt_params &o = vch_pgd_opt(opts, n_opts, b);
    if (const char *bad = vch_pgd_check_weights(opts, n_opts, b)) return bad;
    if (!std::isfinite(o.kappa_sparsity) || o.kappa_sparsity < 0) return "kappa_sparsity must be finite and >= 0";
    if (!(o.alpha_max > 0)) return "alpha_max must be > 0";
    if (std::isnan(o.u_min) || std::isnan(o.u_max) || o.u_min > o.u_max) return "u_min must be <= u_max";
    if (alpha0 && !(std::isfinite(alpha0[b]) && alpha0[b] > 0)) return "alpha0 must be finite and > 0";
    return nullptr;
}

enum vch_pgd_verdict { VCH_PGD_PENDING, VCH_PGD_ACCEPT, VCH_PGD_STOP };
struct vch_pgd_step { double alpha_k, change; int count; };     // of an accepted trial

struct vch_pgd_state {
    std::vector<double> cost, alpha_prev;       // per trajectory: the accepted cost, the next iteration's first step
    std::vector<int> plateau, k, done;
    std::vector<double> alpha;                  // this iteration's current trial step, and who sits the trial marches out
    std::vector<int> accepted;
    // error metrics (G1:425-450, G2:336-363): squared target norms and the RMS fallback scale, set by the engine once per
    // problem, and the per-iteration histories [B][err_n] of the last iterate call
    std::vector<double> denQ2, denT2, trk, trm;
    double rms = 1.0;
    int err_n = 0;

    // J0 [B][5]; the first alpha_prev is alpha_max (the references' start) or the caller's, capped at alpha_max
    void reset(int B, const double *J0, const vch_opt_params *opts, const double *alpha0) {
        cost.resize(B);
        alpha_prev.resize(B);
        for (int b = 0; b < B; ++b) {
            cost[b] = J0[5 * b + 4];
            alpha_prev[b] = alpha0 ? std::min(alpha0[b], opts[b].alpha_max) : opts[b].alpha_max;
        }
        plateau.assign(B, 0);
        k.assign(B, 0);
        done.assign(B, 0);
        alpha.assign(B, 0.0);
        accepted.assign(B, 0);
        err_n = 0;
    }
    void begin_call(int n_iters) {
        err_n = n_iters;
        trk.assign(cost.size() * n_iters, std::nan(""));
        trm.assign(cost.size() * n_iters, std::nan(""));
    }
    bool begin_iteration() {                    // false: every trajectory has stopped
        alpha = alpha_prev;
        accepted = done;
        return std::find(done.begin(), done.end(), 0) != done.end();
    }
    // Trajectory b's trial of `round` in iteration `it` of this call: its cost, the change sums |u+ - u|^2 and |u|^2, the
    // raw squared tracking / terminal errors.  PENDING: alpha[b] is reduced for the next round.  Otherwise `s` is filled
    // and the books are updated; what is copied on the device is the engine's part.
    vch_pgd_verdict judge(const vch_pgd_rule &R, int b, int it, int round, double alpha_max, double c_new, double d2, double n2,
                          double rawQ, double rawT, vch_pgd_step &s) {
        const bool ok = c_new < cost[b];
        if (!ok && round < R.rounds - 1) {
            alpha[b] *= R.beta;
            return VCH_PGD_PENDING;
        }
        accepted[b] = 1;
        s.alpha_k = ok ? alpha[b] : alpha[b] * R.beta;         // "return last try": reduced once more (G1:112-113, G2:144-146)
        s.count = round + R.count0;
        s.change = std::sqrt(d2) / (std::sqrt(n2) + 1e-9);
        double denQ = std::sqrt(std::max(denQ2[b], 0.0));
        if (denQ < 1e-9 * rms) denQ = rms;
        trk[(size_t)b * err_n + it] = std::sqrt(std::max(rawQ, 0.0)) / (denQ + 1e-12);
        trm[(size_t)b * err_n + it] = std::sqrt(std::max(rawT, 0.0)) / (std::sqrt(std::max(denT2[b], 0.0)) + 1e-12);
        // cost[b] is the previous accepted cost here: only a stop leaves it behind, and a stopped trajectory is never judged
        if (k[b] > 0 && std::fabs(c_new - cost[b]) < R.plateau_tol) plateau[b]++;
        else plateau[b] = 0;
        const bool boost = plateau[b] >= R.plateau_len;
        alpha_prev[b] = std::min(alpha_max, s.alpha_k * (boost ? R.plateau_boost : R.grow));
        if (boost) plateau[b] = 0;
        const bool stop = s.change < R.stop_change && k[b] > R.stop_k;
        if (stop) done[b] = 1;
        if (!(stop && R.stop_keeps_state)) cost[b] = c_new;
        k[b]++;
        return stop ? VCH_PGD_STOP : VCH_PGD_ACCEPT;
    }
    bool errors(int n_iters, double *tracking_out, double *terminal_out) const {     // false: not the last call's n_iters
        if (n_iters != err_n || n_iters < 1) return false;
        if (tracking_out) std::memcpy(tracking_out, trk.data(), trk.size() * sizeof(double));
        if (terminal_out) std::memcpy(terminal_out, trm.data(), trm.size() * sizeof(double));
        return true;
    }
};
