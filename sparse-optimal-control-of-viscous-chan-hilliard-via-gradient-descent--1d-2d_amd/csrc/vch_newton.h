// vch_newton.h — the device-resident damped Newton rounds of both engines (vch2d_pgd_newton; vch1d_pgd_newton,
// DESIGN.md 10j).  vch_newton_state holds the verdicts: who ends after the solve, the Armijo test and the halving of the
// trials, who sits a trial or a round out.  vch_newton_check and vch_newton_rounds are the shared argument checks and the round
// loop that applies the verdicts and keeps the call's record, over an adapter for what an engine does.  Host arithmetic only
// (no HIP, no I/O): the engines and tests/newton_replay_main.cpp (scripted solves and costs, on the CPU) are its adapters.
#pragma once
#include "../../include/vch.h"
#include <algorithm>
#include <cmath>
#include <vector>

constexpr double VCH_NEWTON_ARMIJO = 1e-4;      // a trial is accepted when J(trial) <= cost - 1e-4 s pred

enum vch_newton_verdict { VCH_NT_PENDING, VCH_NT_ACCEPT, VCH_NT_STALL };

struct vch_newton_state {
    std::vector<int> ended;         // per trajectory: ended in an earlier round or in this one, sits out all later rounds
    std::vector<int> decided;       // this round: the verdict is in, the trajectory sits the trial marches out
    std::vector<double> s;          // this round's current trial step, a power of two
    std::vector<int> halvings;      // halvings behind s

    void reset(int B) {
        ended.assign(B, 0);
        decided.assign(B, 0);
        s.assign(B, 1.0);
        halvings.assign(B, 0);
    }
    bool begin_round() {            // false: every trajectory has ended
        decided = ended;
        std::fill(s.begin(), s.end(), 1.0);
        std::fill(halvings.begin(), halvings.end(), 0);
        return std::find(ended.begin(), ended.end(), 0) != ended.end();
    }
    bool idle(int b) const { return ended[b] != 0; }
    bool all_decided() const { return std::find(decided.begin(), decided.end(), 0) == decided.end(); }
    // Trajectory b after the round's solve: the end state that needs no trial, or VCH_NEWTON_ACCEPTED when x is a step to
    // try (after VCH_CG_CONVERGED, VCH_CG_LIMIT, or VCH_CG_NEGCURV with steps > 0: the iterate before that direction).  A
    // breakdown ends the trajectory: a march under a control that may not be finite is never started.
    int after_solve(int b, long long n_free, double rnorm0, int cg_status, int cg_steps) {
        int st = VCH_NEWTON_ACCEPTED;
        if (n_free < 1 || rnorm0 == 0.0) st = VCH_NEWTON_STATIONARY;
        else if (cg_status == VCH_CG_BREAKDOWN) st = VCH_NEWTON_BREAKDOWN;
        else if (cg_status == VCH_CG_NEGCURV && cg_steps == 0) st = VCH_NEWTON_NEGCURV;
        if (st != VCH_NEWTON_ACCEPTED) ended[b] = decided[b] = 1;
        return st;
    }
    // Trajectory b's trial at s[b]: `cost` the iterate's, `pred` the decrease the quadratic model predicts for the full
    // step, `c_new` the trial's.  PENDING: s[b] is halved for the next trial.  STALL: no s was accepted within max_halvings
    // halvings, the trajectory ends unmoved.  A cost that is not finite is never accepted.
    vch_newton_verdict judge(int b, double cost, double pred, double c_new, int max_halvings) {
        if (c_new <= cost - VCH_NEWTON_ARMIJO * s[b] * pred) {
            decided[b] = 1;
            return VCH_NT_ACCEPT;
        }
        if (halvings[b] >= max_halvings) {
            ended[b] = decided[b] = 1;
            return VCH_NT_STALL;
        }
        s[b] *= 0.5;
        halvings[b]++;
        return VCH_NT_PENDING;
    }
};

// What a call of vch?d_pgd_newton shares between the engines: the arguments the rounds are run with and the record they
// write, [B][n_rounds] per array (counts: [B][n_rounds][3] = {n_free, pinned, clipped}).
struct vch_newton_call {
    int B, n_rounds, k;
    double cg_tol;
    int precond, max_halvings;
    double *cost, *cost_new, *s, *pred, *rnorm0;
    int32_t *halvings, *cg_steps, *cg_status, *status;
    int64_t *counts;
};
// The first of these arguments the call must refuse with VCH_ERR_ARG, as the text that follows the entry point's name in
// the message, or NULL.  An entry point checks this before anything is enqueued, copied or allocated.
inline const char *vch_newton_check(const vch_newton_call &a) {
    if (a.n_rounds < 1) return "n_rounds must be >= 1";
    if (a.k < 1) return "k must be >= 1";
    if (a.max_halvings < 0) return "max_halvings must be >= 0";
    if (a.precond != 0 && a.precond != 1) return "precond must be 0 or 1";
    if (!std::isfinite(a.cg_tol)) return "cg_tol must be finite";
    if (!(a.cost && a.cost_new && a.s && a.pred && a.rnorm0 && a.halvings && a.cg_steps && a.cg_status && a.status && a.counts))
        return "NULL cost_out, cost_new_out, s_out, pred_out, rnorm0_out, halvings_out, cg_steps_out, cg_status_out, status_out or "
               "counts_out";
    return nullptr;
}

// The rounds of a call that passed vch_newton_check: the record is initialised, then written round by round.  Returns the
// rounds run (fewer than n_rounds once every trajectory has ended) or the first negative code a hook returned; `moved`: a
// step was accepted, on either way out.  The hooks of E, every int one returning < 0 to fail the call:
//   int solve(pred, rnorm0, steps, status, n_free)   the Newton-CG solve of every trajectory about its iterate into these [B]
//                                        arrays (an idle trajectory's solve is not gated)
//   double cost(b)                       the cost of b's iterate
//   int trial(decided, s, sums, c_new)   the trial control of the steps s, its march and its cost for who is not decided: sums
//                                        [B][4] = {.., .., pinned, clipped}, c_new [B] (NaN: a march that must not be accepted)
//   int accept(b, c_new)                 b's trial becomes its iterate
//   int after_trial(), int after_round()
template <class E>
int vch_newton_rounds(E &eng, const vch_newton_call &a, bool &moved) {
    const int B = a.B;
    moved = false;
    for (size_t i = 0; i < (size_t)B * a.n_rounds; ++i) {
        a.cost[i] = a.cost_new[i] = a.s[i] = a.pred[i] = a.rnorm0[i] = std::nan("");
        a.halvings[i] = a.cg_steps[i] = a.cg_status[i] = 0;
        a.status[i] = VCH_NEWTON_IDLE;
        a.counts[3 * i] = a.counts[3 * i + 1] = a.counts[3 * i + 2] = 0;
    }
    vch_newton_state nt;
    nt.reset(B);
    std::vector<double> pred(B), rn0(B), sums(4 * (size_t)B), c_new(B);
    std::vector<int32_t> steps(B), cgst(B);
    std::vector<int64_t> nfree(B);
    int rc, done_rounds = 0;
    for (int r = 0; r < a.n_rounds && nt.begin_round(); ++r) {
        // --- the Newton step of every trajectory on its free set
        if ((rc = eng.solve(pred.data(), rn0.data(), steps.data(), cgst.data(), nfree.data())) < 0) return rc;
        for (int b = 0; b < B; ++b) {
            if (nt.idle(b)) continue;
            const size_t i = (size_t)b * a.n_rounds + r;
            a.cost[i] = a.cost_new[i] = eng.cost(b);
            a.pred[i] = pred[b];
            a.rnorm0[i] = rn0[b];
            a.cg_steps[i] = steps[b];
            a.cg_status[i] = cgst[b];
            a.counts[3 * i] = nfree[b];
            a.status[i] = nt.after_solve(b, nfree[b], rn0[b], cgst[b], steps[b]);
        }
        // --- trials s = 1, 1/2, ...: a trajectory whose verdict is in sits the trial out
        while (!nt.all_decided()) {
            if ((rc = eng.trial(nt.decided, nt.s, sums.data(), c_new.data())) < 0) return rc;
            for (int b = 0; b < B; ++b) {
                if (nt.decided[b]) continue;
                const size_t i = (size_t)b * a.n_rounds + r;
                a.halvings[i] = nt.halvings[b];
                a.counts[3 * i + 1] = (int64_t)sums[4 * b + 2];
                a.counts[3 * i + 2] = (int64_t)sums[4 * b + 3];
                const double s = nt.s[b];
                const vch_newton_verdict v = nt.judge(b, eng.cost(b), pred[b], c_new[b], a.max_halvings);
                if (v == VCH_NT_STALL) a.status[i] = VCH_NEWTON_STALLED;
                if (v != VCH_NT_ACCEPT) continue;
                // accepted: the trial becomes the iterate, as in the PGD loop
                if ((rc = eng.accept(b, c_new[b])) < 0) return rc;
                moved = true;
                a.cost_new[i] = c_new[b];
                a.s[i] = s;
            }
            if ((rc = eng.after_trial()) < 0) return rc;
        }
        if ((rc = eng.after_round()) < 0) return rc;
        done_rounds = r + 1;
    }
    return done_rounds;
}

// ---------------------------------------------------------------------------------------------------------------------
// Trust-region rounds (vch1d_pgd_trust): one trial per round at s = 1 of the Steihaug step inside the radius,
// the damped rounds' Armijo test at s = 1 for acceptance, the ratio rho = (J(u) - J(t)) / pred for the radius.
// ---------------------------------------------------------------------------------------------------------------------
constexpr double VCH_TRUST_SHRINK_BELOW = 0.25;     // rho below (or not finite): radius = 1/4 min(radius, ||x||_D)
constexpr double VCH_TRUST_GROW_ABOVE = 0.75;       // rho above and the step ended on the boundary: radius = min(2 radius, max)

struct vch_trust_state {
    std::vector<int> ended;         // per trajectory: ended in an earlier round or in this one, sits out all later rounds
    std::vector<double> radius;     // the radius of the next solve
    std::vector<double> radius0;

    void reset(const double *r0, int B) {
        ended.assign(B, 0);
        radius0.assign(r0, r0 + B);
        radius = radius0;
    }
    bool any_live() const { return std::find(ended.begin(), ended.end(), 0) != ended.end(); }
    bool idle(int b) const { return ended[b] != 0; }
    // the radius b's solve runs with: an ended trajectory's solve is not gated and gets its first radius, which passes the
    // solve's check whatever the rounds did to its own
    double solve_radius(int b) const { return ended[b] ? radius0[b] : radius[b]; }
    // Trajectory b after the round's solve: VCH_NEWTON_STATIONARY (empty free set or ||P b|| == 0) or VCH_NEWTON_BREAKDOWN
    // end it without a trial; otherwise VCH_NEWTON_ACCEPTED, pending: x is the step to try, whatever the CG exit.
    int after_solve(int b, long long n_free, double rnorm0, int cg_status) {
        int st = VCH_NEWTON_ACCEPTED;
        if (n_free < 1 || rnorm0 == 0.0) st = VCH_NEWTON_STATIONARY;
        else if (cg_status == VCH_CG_BREAKDOWN) st = VCH_NEWTON_BREAKDOWN;
        if (st != VCH_NEWTON_ACCEPTED) ended[b] = 1;
        return st;
    }
    // b's trial: `cost` the iterate's, `pred` the model's decrease, `c_new` the trial's, `xnorm` ||x||_D, `cg_status` the CG
    // exit.  Accepted iff c_new is finite and c_new <= cost - 1e-4 pred.  The radius: rho < 1/4 or not finite: 1/4 min(radius,
    // xnorm); else rho > 3/4 after VCH_CG_BOUNDARY or VCH_CG_NEGCURV: min(2 radius, radius_max).  A radius below radius_min
    // ends the trajectory: VCH_NEWTON_STALLED after a rejection (unmoved), VCH_NEWTON_ACCEPTED after an acceptance.
    // Otherwise a rejected trajectory is VCH_NEWTON_REJECTED, unmoved, and goes on.  ratio: rho.
    int judge(int b, double cost, double pred, double c_new, double xnorm, int cg_status, double radius_max, double radius_min,
              double &ratio) {
        ratio = (cost - c_new) / pred;
        const bool accept = std::isfinite(c_new) && c_new <= cost - VCH_NEWTON_ARMIJO * pred;
        double &rad = radius[b];
        if (!std::isfinite(ratio) || ratio < VCH_TRUST_SHRINK_BELOW)
            rad = 0.25 * std::min(rad, xnorm);
        else if (ratio > VCH_TRUST_GROW_ABOVE && (cg_status == VCH_CG_BOUNDARY || cg_status == VCH_CG_NEGCURV))
            rad = std::min(2.0 * rad, radius_max);
        const bool small = rad < radius_min;
        if (small) ended[b] = 1;
        if (accept) return VCH_NEWTON_ACCEPTED;
        return small ? VCH_NEWTON_STALLED : VCH_NEWTON_REJECTED;
    }
};

// What a call of vch1d_pgd_trust passes the rounds: the arguments and the record, [B][n_rounds] per array (counts:
// [B][n_rounds][3] = {n_free, pinned, clipped}).
struct vch_trust_call {
    int B, n_rounds, k;
    double cg_tol;
    int precond;
    const double *radius0;
    double radius_max, radius_min;
    double *cost, *cost_new, *pred, *rnorm0, *radius, *ratio, *xnorm;
    int32_t *cg_steps, *cg_status, *status;
    int64_t *counts;
};
// The first of these arguments the call must refuse with VCH_ERR_ARG (the text that follows the entry point's name in the
// message), or NULL.  An entry point checks this before anything is enqueued, copied or allocated.
inline const char *vch_trust_check(const vch_trust_call &a) {
    if (a.n_rounds < 1) return "n_rounds must be >= 1";
    if (a.k < 1) return "k must be >= 1";
    if (a.precond != 0 && a.precond != 1) return "precond must be 0 or 1";
    if (!std::isfinite(a.cg_tol)) return "cg_tol must be finite";
    if (!a.radius0) return "NULL radius0";
    for (int b = 0; b < a.B; ++b)
        if (!(std::isfinite(a.radius0[b]) && a.radius0[b] > 0.0)) return "every radius0 must be finite and > 0";
    if (!(std::isfinite(a.radius_max) && a.radius_max > 0.0)) return "radius_max must be finite and > 0";
    if (!(std::isfinite(a.radius_min) && a.radius_min > 0.0)) return "radius_min must be finite and > 0";
    if (!(a.cost && a.cost_new && a.pred && a.rnorm0 && a.radius && a.ratio && a.xnorm && a.cg_steps && a.cg_status && a.status &&
          a.counts))
        return "NULL cost_out, cost_new_out, pred_out, rnorm0_out, radius_out, ratio_out, xnorm_out, cg_steps_out, cg_status_out, "
               "status_out or counts_out";
    return nullptr;
}

// The rounds of a call that passed vch_trust_check, as vch_newton_rounds: the record is initialised (NaN, 0, IDLE), then
// written round by round.  Returns the rounds run (fewer than n_rounds once every trajectory has ended) or the first negative
// code a hook returned; `moved`: a trial was accepted.  The hooks of E, every int one returning < 0 to fail the call:
//   int solve(radius, pred, rnorm0, steps, status, n_free, xnorm)   the Steihaug solve of every trajectory about its iterate
//                                        inside radius [B] into these [B] arrays (an idle trajectory's solve is not gated)
//   double cost(b)                       the cost of b's iterate
//   int trial(decided, sums, c_new)      the trial control at s = 1, its march and its cost for who is not decided: sums [B][4]
//                                        = {.., .., pinned, clipped}, c_new [B] (NaN: a march that must not be accepted)
//   int accept(b, c_new)                 b's trial becomes its iterate
//   int after_trial(), int after_round()
template <class E>
int vch_trust_rounds(E &eng, const vch_trust_call &a, bool &moved) {
    const int B = a.B;
    moved = false;
    for (size_t i = 0; i < (size_t)B * a.n_rounds; ++i) {
        a.cost[i] = a.cost_new[i] = a.pred[i] = a.rnorm0[i] = a.radius[i] = a.ratio[i] = a.xnorm[i] = std::nan("");
        a.cg_steps[i] = a.cg_status[i] = 0;
        a.status[i] = VCH_NEWTON_IDLE;
        a.counts[3 * i] = a.counts[3 * i + 1] = a.counts[3 * i + 2] = 0;
    }
    vch_trust_state tr;
    tr.reset(a.radius0, B);
    std::vector<double> rad(B), pred(B), rn0(B), xn(B), sums(4 * (size_t)B), c_new(B);
    std::vector<int32_t> steps(B), cgst(B);
    std::vector<int64_t> nfree(B);
    std::vector<int> decided(B);
    int rc, done_rounds = 0;
    for (int r = 0; r < a.n_rounds && tr.any_live(); ++r) {
        for (int b = 0; b < B; ++b) rad[b] = tr.solve_radius(b);
        if ((rc = eng.solve(rad.data(), pred.data(), rn0.data(), steps.data(), cgst.data(), nfree.data(), xn.data())) < 0) return rc;
        for (int b = 0; b < B; ++b) {
            decided[b] = tr.idle(b);
            if (decided[b]) continue;
            const size_t i = (size_t)b * a.n_rounds + r;
            a.cost[i] = a.cost_new[i] = eng.cost(b);
            a.pred[i] = pred[b];
            a.rnorm0[i] = rn0[b];
            a.radius[i] = rad[b];
            a.xnorm[i] = xn[b];
            a.cg_steps[i] = steps[b];
            a.cg_status[i] = cgst[b];
            a.counts[3 * i] = nfree[b];
            a.status[i] = tr.after_solve(b, nfree[b], rn0[b], cgst[b]);
            decided[b] = a.status[i] != VCH_NEWTON_ACCEPTED;
        }
        // one trial at s = 1 for whoever has a step; a trajectory whose verdict is in sits it out
        if (std::find(decided.begin(), decided.end(), 0) != decided.end()) {
            if ((rc = eng.trial(decided, sums.data(), c_new.data())) < 0) return rc;
            for (int b = 0; b < B; ++b) {
                if (decided[b]) continue;
                const size_t i = (size_t)b * a.n_rounds + r;
                a.counts[3 * i + 1] = (int64_t)sums[4 * b + 2];
                a.counts[3 * i + 2] = (int64_t)sums[4 * b + 3];
                const int st = tr.judge(b, eng.cost(b), pred[b], c_new[b], xn[b], cgst[b], a.radius_max, a.radius_min, a.ratio[i]);
                a.status[i] = st;
                if (st != VCH_NEWTON_ACCEPTED) continue;
                if ((rc = eng.accept(b, c_new[b])) < 0) return rc;
                moved = true;
                a.cost_new[i] = c_new[b];
            }
            if ((rc = eng.after_trial()) < 0) return rc;
        }
        if ((rc = eng.after_round()) < 0) return rc;
        done_rounds = r + 1;
    }
    return done_rounds;
}
