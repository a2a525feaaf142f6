// newton_replay_main.cpp — runs the argument checks and the round loop of csrc/vch_newton.h (vch_newton_check and
// vch_newton_rounds, the ones both engines run) without a device: its adapter takes the solves' outcomes and the trial costs
// from a script.  Built and run by tests/test_newton_rule_cpu.py.
//
// stdin, whitespace-separated (doubles in any strtod form):
//   B n_rounds max_halvings, then per trajectory: J0 L and L entries {n_free rnorm0 cg_status cg_steps pred accept_at cost_new}
// Entry k of a script is the trajectory's k-th live round.  A trial after h halvings is offered cost_new when h == accept_at
// and the iterate's own cost otherwise (never a sufficient decrease for pred > 0); accept_at < 0 never accepts.
//   -> per round "round r", per trial march "trial r <the B flags of who sits it out> <the B step lengths>", and per
//      trajectory "row b r status s halvings cost cost_new" (status VCH_NEWTON_*, s = nan when nothing moved; an idle
//      trajectory's row shows the cost it rests on); at the end "rounds <n>".
// Options: --k N, --precond N, --cg-tol X set the shared arguments the script does not carry (default 1, 0, 0), --null-s
// passes s_out as NULL, --record prints after "rounds" every cell of the driver's record: "rec b r cost cost_new s pred rnorm0
// halvings cg_steps cg_status status n_free pinned clipped".  A refused call prints "error <code> hooks <hook calls made>
// <message>" and exits with 3.
#include "vch_newton.h"
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

struct Replay {
    const vch_newton_call &a;
    std::vector<double> J;              // the cost of every trajectory's iterate
    std::vector<std::vector<Entry>> script;
    std::vector<size_t> live;
    std::vector<const Entry *> cur;
    std::vector<int> sat;               // this round: the trials a trajectory has sat = the halvings behind its step
    int round = -1, hooks = 0;

    int solve(double *pred, double *rnorm0, int32_t *steps, int32_t *status, int64_t *n_free) {
        hooks++;
        printf("round %d\n", ++round);
        for (int b = 0; b < a.B; ++b) {
            sat[b] = 0;
            // the record says who is idle: whoever did not end the round before with an accepted step
            if (round > 0 && a.status[(size_t)b * a.n_rounds + round - 1] != VCH_NEWTON_ACCEPTED) continue;
            if (live[b] >= script[b].size()) { fprintf(stderr, "script of trajectory %d is too short\n", b); return -1; }
            const Entry &e = *(cur[b] = &script[b][live[b]++]);
            n_free[b] = e.n_free; rnorm0[b] = e.rnorm0; status[b] = e.cg_status; steps[b] = e.cg_steps; pred[b] = e.pred;
        }
        return 0;
    }
    double cost(int b) { hooks++; return J[b]; }
    int trial(const std::vector<int> &decided, const std::vector<double> &s, double *sums, double *c_new) {
        hooks++;
        printf("trial %d", round);
        for (int b = 0; b < a.B; ++b) printf(" %d", decided[b]);
        for (int b = 0; b < a.B; ++b) printf(" %.17g", s[b]);
        printf("\n");
        for (int b = 0; b < a.B; ++b)
            if (!decided[b]) {
                c_new[b] = sat[b]++ == cur[b]->accept_at ? cur[b]->cost_new : J[b];
                sums[4 * b + 2] = sums[4 * b + 3] = 0.0;
            }
        return 0;
    }
    int accept(int b, double c_new) { hooks++; J[b] = c_new; return 0; }
    int after_trial() { hooks++; return 0; }
    int after_round() {
        hooks++;
        for (int b = 0; b < a.B; ++b) {
            const size_t i = (size_t)b * a.n_rounds + round;
            const bool rests = a.status[i] == VCH_NEWTON_IDLE;
            printf("row %d %d %d %.17g %d %.17g %.17g\n", b, round, a.status[i], a.s[i], a.halvings[i], rests ? J[b] : a.cost[i],
                   rests ? J[b] : a.cost_new[i]);
        }
        return 0;
    }
};

int main(int argc, char **argv) {
    vch_newton_call a{};
    a.k = 1;
    bool record = false, null_s = false;
    for (int i = 1; i < argc; ++i) {
        const std::string o = argv[i];
        if (o == "--record") record = true;
        else if (o == "--null-s") null_s = true;
        else if (o == "--k" && i + 1 < argc) a.k = atoi(argv[++i]);
        else if (o == "--precond" && i + 1 < argc) a.precond = atoi(argv[++i]);
        else if (o == "--cg-tol" && i + 1 < argc) a.cg_tol = strtod(argv[++i], nullptr);
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    const int B = a.B = (int)num(), n_rounds = a.n_rounds = (int)num();
    a.max_halvings = (int)num();
    Replay eng{a, std::vector<double>(B), std::vector<std::vector<Entry>>(B), std::vector<size_t>(B, 0),
               std::vector<const Entry *>(B, nullptr), std::vector<int>(B, 0)};
    for (int b = 0; b < B; ++b) {
        eng.J[b] = num();
        eng.script[b].resize((size_t)num());
        for (Entry &e : eng.script[b]) {
            e.n_free = (long long)num(); e.rnorm0 = num(); e.cg_status = (int)num(); e.cg_steps = (int)num();
            e.pred = num(); e.accept_at = (int)num(); e.cost_new = num();
        }
    }
    // the record, filled with what the driver writes nowhere: it must overwrite every cell
    const size_t cells = (size_t)B * (n_rounds > 0 ? n_rounds : 0);
    std::vector<double> d(5 * cells, -7.0);
    std::vector<int32_t> n(4 * cells, -7);
    std::vector<int64_t> counts(3 * cells, -7);
    a.cost = d.data(); a.cost_new = a.cost + cells; a.s = null_s ? nullptr : a.cost + 2 * cells; a.pred = a.cost + 3 * cells;
    a.rnorm0 = a.cost + 4 * cells;
    a.halvings = n.data(); a.cg_steps = a.halvings + cells; a.cg_status = a.halvings + 2 * cells; a.status = a.halvings + 3 * cells;
    a.counts = counts.data();
    bool moved = false;
    const char *bad = vch_newton_check(a);
    const int rc = bad ? VCH_ERR_ARG : vch_newton_rounds(eng, a, moved);
    if (bad) printf("error %d hooks %d newton_replay: %s\n", rc, eng.hooks, bad);
    if (rc < 0) return bad ? 3 : 2;
    printf("rounds %d\n", rc);
    for (size_t i = 0; record && i < cells; ++i)
        printf("rec %zu %zu %.17g %.17g %.17g %.17g %.17g %d %d %d %d %lld %lld %lld\n", i / a.n_rounds, i % a.n_rounds, a.cost[i],
               a.cost_new[i], a.s[i], a.pred[i], a.rnorm0[i], a.halvings[i], a.cg_steps[i], a.cg_status[i], a.status[i],
               (long long)a.counts[3 * i], (long long)a.counts[3 * i + 1], (long long)a.counts[3 * i + 2]);
    return 0;
}
