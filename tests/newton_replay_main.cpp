// newton_replay_main.cpp — drives the verdict logic of csrc/vch_newton.h the way vch2d_pgd_newton does, without a device: the
// solves' outcomes and the trial costs come from a script instead of a device.  Built and run by tests/test_newton_rule_cpu.py.
//
// stdin, whitespace-separated (doubles in any strtod form):
//   B n_rounds max_halvings, then per trajectory: J0 L and L entries {n_free rnorm0 cg_status cg_steps pred accept_at cost_new}
// Entry k of a script is the trajectory's k-th live round.  A trial after h halvings is offered cost_new when h == accept_at
// and the iterate's own cost otherwise (never a sufficient decrease for pred > 0); accept_at < 0 never accepts.
//   -> per round "round r", per trial march "trial r <the B flags of who sits it out> <the B step lengths>", and per
//      trajectory "row b r status s halvings cost cost_new" (status VCH_NEWTON_*, s = nan when nothing moved);
//      at the end "rounds <n>".
#include "vch_newton.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

static double num() {
    std::string s;
    if (!(std::cin >> s)) { fprintf(stderr, "unexpected end of input\n"); exit(2); }
    return strtod(s.c_str(), nullptr);
}
struct Entry { long long n_free; double rnorm0; int cg_status, cg_steps; double pred; int accept_at; double cost_new; };

int main() {
    const int B = (int)num(), n_rounds = (int)num(), max_halvings = (int)num();
    std::vector<double> cost(B);
    std::vector<std::vector<Entry>> script(B);
    std::vector<size_t> live(B, 0);
    for (int b = 0; b < B; ++b) {
        cost[b] = num();
        script[b].resize((size_t)num());
        for (Entry &e : script[b]) {
            e.n_free = (long long)num(); e.rnorm0 = num(); e.cg_status = (int)num(); e.cg_steps = (int)num();
            e.pred = num(); e.accept_at = (int)num(); e.cost_new = num();
        }
    }
    vch_newton_state nt;
    nt.reset(B);
    int done = 0;
    for (int r = 0; r < n_rounds; ++r) {
        if (!nt.begin_round()) break;
        printf("round %d\n", r);
        std::vector<int> status(B, VCH_NEWTON_IDLE), halv(B, 0);
        std::vector<double> s_acc(B, std::nan("")), c_old(cost), c_new(cost);
        std::vector<const Entry *> cur(B, nullptr);
        for (int b = 0; b < B; ++b) {
            if (nt.idle(b)) continue;
            if (live[b] >= script[b].size()) { fprintf(stderr, "script of trajectory %d is too short\n", b); return 2; }
            cur[b] = &script[b][live[b]++];
            status[b] = nt.after_solve(b, cur[b]->n_free, cur[b]->rnorm0, cur[b]->cg_status, cur[b]->cg_steps);
        }
        while (!nt.all_decided()) {
            printf("trial %d", r);
            for (int b = 0; b < B; ++b) printf(" %d", nt.decided[b]);
            for (int b = 0; b < B; ++b) printf(" %.17g", nt.s[b]);
            printf("\n");
            for (int b = 0; b < B; ++b) {
                if (nt.decided[b]) continue;
                halv[b] = nt.halvings[b];
                const double s = nt.s[b];
                const double offered = nt.halvings[b] == cur[b]->accept_at ? cur[b]->cost_new : cost[b];
                const vch_newton_verdict v = nt.judge(b, cost[b], cur[b]->pred, offered, max_halvings);
                if (v == VCH_NT_STALL) status[b] = VCH_NEWTON_STALLED;
                if (v != VCH_NT_ACCEPT) continue;
                cost[b] = c_new[b] = offered;
                s_acc[b] = s;
            }
        }
        for (int b = 0; b < B; ++b)
            printf("row %d %d %d %.17g %d %.17g %.17g\n", b, r, status[b], s_acc[b], halv[b], c_old[b], c_new[b]);
        done = r + 1;
    }
    printf("rounds %d\n", done);
    return 0;
}
