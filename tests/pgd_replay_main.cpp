// pgd_replay_main.cpp — drives the PGD line-search state machine of csrc/vch_pgd.h the way the engines do, without a device:
// the trial costs come from a script instead of a march.  Built and run by tests/test_pgd_rule_cpu.py.
//
// stdin, whitespace-separated (doubles in any strtod form):
//   check b1 b2 b3 kappa_sparsity alpha_max u_min u_max has_alpha0 alpha0
//       -> "check <message or ok>" and "weights <message or ok>"
//   <1d|2d> B n_iters n_calls has_alpha0, then per trajectory: alpha_max alpha0 J0 L and L entries {round cost change}
//       -> per call a line "row b it alpha_k count cost done alpha_prev" for every accepted trial
//          (cost, done, alpha_prev as stored after it), then "call <c> iters <n> errors <1> <0>" (what the error histories
//          answer to this call's n_iters and to another) and "err b it tracking terminal" for every slot of the histories.
// Entry k of a script is the trajectory's k-th iteration: the rounds before `round` are offered the stored cost (never a
// descent, so they are rejected), round `round` is offered `cost`; the change sums are change^2 and 1.
#include "vch_pgd.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

static double num() {
    std::string s;
    if (!(std::cin >> s)) { fprintf(stderr, "unexpected end of input\n"); exit(2); }
    return strtod(s.c_str(), nullptr);
}
struct Entry { int round; double cost, change; };

int main() {
    std::string mode;
    std::cin >> mode;
    if (mode == "check") {
        vch_opt_params o = {};
        o.b1 = num(); o.b2 = num(); o.b3 = num(); o.kappa_sparsity = num(); o.alpha_max = num(); o.u_min = num(); o.u_max = num();
        const bool has_alpha0 = num() != 0;
        const double alpha0 = num();
        const char *bad = vch_pgd_check(&o, 1, has_alpha0 ? &alpha0 : nullptr, 0), *w = vch_pgd_check_weights(&o, 1, 0);
        printf("check %s\nweights %s\n", bad ? bad : "ok", w ? w : "ok");
        return 0;
    }
    if (mode != "1d" && mode != "2d") { fprintf(stderr, "unknown rule %s\n", mode.c_str()); return 2; }
    const vch_pgd_rule R = mode == "1d" ? VCH_PGD_1D : VCH_PGD_2D;
    const int B = (int)num(), n_iters = (int)num(), n_calls = (int)num();
    const bool has_alpha0 = num() != 0;
    std::vector<vch_opt_params> opts(B);
    std::vector<double> alpha0(B), J0(5 * B, 0.0);
    std::vector<std::vector<Entry>> script(B);
    for (int b = 0; b < B; ++b) {
        opts[b] = {};
        opts[b].alpha_max = num();
        alpha0[b] = num();
        J0[5 * b + 4] = num();
        script[b].resize((size_t)num());
        for (Entry &e : script[b]) { e.round = (int)num(); e.cost = num(); e.change = num(); }
    }
    vch_pgd_state st;
    st.denQ2.assign(B, 1.0);
    st.denT2.assign(B, 1.0);
    st.reset(B, J0.data(), opts.data(), has_alpha0 ? alpha0.data() : nullptr);
    for (int call = 0; call < n_calls; ++call) {
        st.begin_call(n_iters);
        int done_iters = 0;
        for (int it = 0; it < n_iters; ++it) {
            if (!st.begin_iteration()) break;
            for (int round = 0; round < R.rounds; ++round) {
                bool pending = false;
                for (int b = 0; b < B; ++b) {
                    if (st.accepted[b]) continue;
                    if ((size_t)st.k[b] >= script[b].size()) { fprintf(stderr, "script of trajectory %d is too short\n", b); return 2; }
                    const Entry &e = script[b][st.k[b]];
                    vch_pgd_step s;
                    if (st.judge(R, b, it, round, opts[b].alpha_max, round == e.round ? e.cost : st.cost[b], e.change * e.change, 1.0,
                                 4.0, 9.0, s) == VCH_PGD_PENDING) {
                        pending = true;
                        continue;
                    }
                    printf("row %d %d %.17g %d %.17g %d %.17g\n", b, it, s.alpha_k, s.count, st.cost[b], st.done[b], st.alpha_prev[b]);
                }
                if (!pending) break;
            }
            done_iters = it + 1;
        }
        std::vector<double> trk((size_t)B * n_iters), trm((size_t)B * n_iters);
        const bool got = st.errors(n_iters, trk.data(), trm.data()), other = st.errors(n_iters + 1, nullptr, nullptr);
        printf("call %d iters %d errors %d %d\n", call, done_iters, (int)got, (int)other);
        for (size_t i = 0; i < trk.size(); ++i) printf("err %d %d %.17g %.17g\n", (int)(i / n_iters), (int)(i % n_iters), trk[i], trm[i]);
    }
    return 0;
}
