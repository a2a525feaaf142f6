// vch_newton.h — the verdicts of the device-resident damped Newton rounds of both engines (vch2d_pgd_newton, DESIGN.md 10i;
// vch1d_pgd_newton): who ends after the solve, the Armijo test and the halving of the trials, who sits a trial
// or a round out.  Host arithmetic only (no HIP, no I/O): the engines act on its verdicts, tests/newton_replay_main.cpp
// replays it on the CPU.
#pragma once
#include "../../include/vch.h"
#include <algorithm>
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
