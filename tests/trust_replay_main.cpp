// trust_replay_main.cpp — runs the argument checks and the round loop of the trust-region rounds of csrc/vch_newton.h
// (vch_trust_check and vch_trust_rounds, the ones vch1d_pgd_trust runs) without a device: its adapter takes the solves'
// outcomes and the trial costs from a script.  Built and run by tests/test_trust_rule_cpu.py.
//
// stdin, whitespace-separated (doubles in any strtod form):
//   B n_rounds radius_max radius_min, then per trajectory: J0 radius0 L and L entries
//   {n_free rnorm0 cg_status cg_steps pred xnorm cost_new}
// Entry k of a script is the trajectory's k-th live round; its trial is offered cost_new.
//   -> per round "round r <the B radii the solve was given>", per trial "trial r <the B flags of who sits it out>", at the end
//      "rounds <n>" and every cell of the record: "rec b r cost cost_new pred rnorm0 radius ratio xnorm cg_steps cg_status status
//      n_free pinned clipped", then "J <the B final costs>".
// Options: --k N, --precond N, --cg-tol X set the shared arguments the script does not carry (default 1, 0, 0), --null-ratio
// passes ratio_out as NULL.  A refused call prints "error <code> hooks <hook calls made> <message>" and exits with 3.
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
struct Entry { long long n_free; double rnorm0; int cg_status, cg_steps; double pred, xnorm, cost_new; };

struct Replay {
    const vch_trust_call &a;
    std::vector<double> J;              // the cost of every trajectory's iterate
    std::vector<std::vector<Entry>> script;
    std::vector<size_t> live;
    std::vector<const Entry *> cur;
    int round = -1, hooks = 0;

    // the record says who is idle: whoever ended in an earlier round
    bool ended_before(int b) const {
        for (int r = 0; r < round; ++r) {
            const int st = a.status[(size_t)b * a.n_rounds + r];
            if (st != VCH_NEWTON_ACCEPTED && st != VCH_NEWTON_REJECTED) return true;
        }
        return false;
    }
    int solve(const double *radius, double *pred, double *rnorm0, int32_t *steps, int32_t *status, int64_t *n_free, double *xnorm) {
        hooks++;
        printf("round %d", ++round);
        for (int b = 0; b < a.B; ++b) printf(" %.17g", radius[b]);
        printf("\n");
        for (int b = 0; b < a.B; ++b) {
            if (ended_before(b) || live[b] >= script[b].size()) {
                cur[b] = nullptr;
                n_free[b] = 1; rnorm0[b] = 1.0; status[b] = VCH_CG_CONVERGED; steps[b] = 1; pred[b] = 1.0; xnorm[b] = 1.0;
                continue;
            }
            const Entry &e = *(cur[b] = &script[b][live[b]++]);
            n_free[b] = e.n_free; rnorm0[b] = e.rnorm0; status[b] = e.cg_status; steps[b] = e.cg_steps; pred[b] = e.pred;
            xnorm[b] = e.xnorm;
        }
        return 0;
    }
    double cost(int b) { hooks++; return J[b]; }
    int trial(const std::vector<int> &decided, double *sums, double *c_new) {
        hooks++;
        printf("trial %d", round);
        for (int b = 0; b < a.B; ++b) printf(" %d", decided[b]);
        printf("\n");
        for (int b = 0; b < a.B; ++b)
            if (!decided[b]) {
                if (!cur[b]) { fprintf(stderr, "script of trajectory %d is too short\n", b); return -1; }
                c_new[b] = cur[b]->cost_new;
                sums[4 * b + 2] = sums[4 * b + 3] = 0.0;
            }
        return 0;
    }
    int accept(int b, double c_new) { hooks++; J[b] = c_new; return 0; }
    int after_trial() { hooks++; return 0; }
    int after_round() { hooks++; return 0; }
};

int main(int argc, char **argv) {
    vch_trust_call a{};
    a.k = 1;
    bool null_ratio = false;
    for (int i = 1; i < argc; ++i) {
        const std::string o = argv[i];
        if (o == "--null-ratio") null_ratio = true;
        else if (o == "--k" && i + 1 < argc) a.k = atoi(argv[++i]);
        else if (o == "--precond" && i + 1 < argc) a.precond = atoi(argv[++i]);
        else if (o == "--cg-tol" && i + 1 < argc) a.cg_tol = strtod(argv[++i], nullptr);
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    const int B = a.B = (int)num(), n_rounds = a.n_rounds = (int)num();
    a.radius_max = num();
    a.radius_min = num();
    Replay eng{a, std::vector<double>(B), std::vector<std::vector<Entry>>(B), std::vector<size_t>(B, 0),
               std::vector<const Entry *>(B, nullptr)};
    std::vector<double> radius0(B);
    for (int b = 0; b < B; ++b) {
        eng.J[b] = num();
        radius0[b] = num();
        eng.script[b].resize((size_t)num());
        for (Entry &e : eng.script[b]) {
            e.n_free = (long long)num(); e.rnorm0 = num(); e.cg_status = (int)num(); e.cg_steps = (int)num();
            e.pred = num(); e.xnorm = num(); e.cost_new = num();
        }
    }
    a.radius0 = radius0.data();
    // the record, filled with what the driver writes nowhere: it must overwrite every cell
    const size_t cells = (size_t)B * (n_rounds > 0 ? n_rounds : 0);
    std::vector<double> d(7 * cells, -7.0);
    std::vector<int32_t> n(3 * cells, -7);
    std::vector<int64_t> counts(3 * cells, -7);
    a.cost = d.data(); a.cost_new = a.cost + cells; a.pred = a.cost + 2 * cells; a.rnorm0 = a.cost + 3 * cells;
    a.radius = a.cost + 4 * cells; a.ratio = null_ratio ? nullptr : a.cost + 5 * cells; a.xnorm = a.cost + 6 * cells;
    a.cg_steps = n.data(); a.cg_status = a.cg_steps + cells; a.status = a.cg_steps + 2 * cells;
    a.counts = counts.data();
    bool moved = false;
    const char *bad = vch_trust_check(a);
    const int rc = bad ? VCH_ERR_ARG : vch_trust_rounds(eng, a, moved);
    if (bad) printf("error %d hooks %d trust_replay: %s\n", rc, eng.hooks, bad);
    if (rc < 0) return bad ? 3 : 2;
    printf("rounds %d moved %d\n", rc, (int)moved);
    for (size_t i = 0; i < cells; ++i)
        printf("rec %zu %zu %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d %d %lld %lld %lld\n", i / a.n_rounds, i % a.n_rounds,
               a.cost[i], a.cost_new[i], a.pred[i], a.rnorm0[i], a.radius[i], a.ratio[i], a.xnorm[i], a.cg_steps[i], a.cg_status[i],
               a.status[i], (long long)a.counts[3 * i], (long long)a.counts[3 * i + 1], (long long)a.counts[3 * i + 2]);
    printf("J");
    for (int b = 0; b < B; ++b) printf(" %.17g", eng.J[b]);
    printf("\n");
    return 0;
}
