// Per-launch time of the group prox kernels of the 1D engine beside k1d_grad_prox: event pairs around single
// launches, medians of 21 after 3 warm-up launches.  Shapes: N = 4096 x 1000 steps at batch 1 and N = 256 x 100 steps at
// batch 256; inputs: one with an infinite box (every group takes the closed form or vanishes) and one whose box (-1, 1) holds
// about a third of the groups, which then run the safeguarded iteration.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -I <package>/csrc scripts/dirsparse_1d_timing.hip -o dirsparse_1d_timing
#include "vch_kernels1d.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#define CHK(call)                                                                            \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));       \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

static double rnd(unsigned long long &s) {          // uniform in (-1, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(s >> 11) / 9007199254740992.0) * 2.0 - 1.0;
}

template <class F>
static int median_ms(F launch, double *out) {
    hipEvent_t a, b;
    CHK(hipEventCreate(&a));
    CHK(hipEventCreate(&b));
    for (int i = 0; i < 3; ++i) launch();
    CHK(hipDeviceSynchronize());
    std::vector<float> ms(21);
    for (auto &m : ms) {
        CHK(hipEventRecord(a, 0));
        launch();
        CHK(hipEventRecord(b, 0));
        CHK(hipEventSynchronize(b));
        CHK(hipEventElapsedTime(&m, a, b));
    }
    CHK(hipGetLastError());
    std::sort(ms.begin(), ms.end());
    *out = ms[ms.size() / 2];
    hipEventDestroy(a);
    hipEventDestroy(b);
    return 0;
}

static int run(int N, int steps, int B, bool active) {
    const int n = N + 1, rows = steps + 2, nblk = (n + 63) / 64;
    const long hs = (long)rows * n;
    const double inf = std::numeric_limits<double>::infinity();
    const double alpha = 0.5, ks = 0.04, lo = active ? -1.0 : -inf, hi = active ? 1.0 : inf;
    std::vector<double> u((size_t)B * hs), r((size_t)B * hs), tab((size_t)B * OPT1_STRIDE), al(B, alpha), wx(n, 1.0 / N), wt(rows, 1.0 / steps);
    wx[0] = wx[n - 1] = 0.5 / N;
    wt[0] = 0.0; wt[1] = wt[rows - 1] = 0.5 / steps;
    unsigned long long seed = 12345;
    // v = u - alpha r with a block pattern of amplitudes in both directions: 0.005 (||v|| < lam = 0.02), 0.05, 3
    const double amp[3] = {0.005, 0.05, 3.0};
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < rows; ++k)
            for (int i = 0; i < n; ++i) {
                const double a = std::min(amp[(k + b) % 3], amp[(i / 7 + b) % 3]);
                const double v = a * rnd(seed) * 1.7, rr = rnd(seed);
                r[(size_t)b * hs + (long)k * n + i] = rr;
                u[(size_t)b * hs + (long)k * n + i] = v + alpha * rr;
            }
    for (int b = 0; b < B; ++b) {
        double *q = tab.data() + (size_t)b * OPT1_STRIDE;
        q[OPT1_B3] = 0.0; q[OPT1_KS] = ks; q[OPT1_UMIN] = lo; q[OPT1_UMAX] = hi;
    }
    double *du, *dr, *dout, *dtab, *dal, *dwx, *dwt, *ds, *dchg, *dchg2;
    CHK(hipMalloc(&du, u.size() * 8)); CHK(hipMalloc(&dr, r.size() * 8)); CHK(hipMalloc(&dout, u.size() * 8));
    CHK(hipMalloc(&dtab, tab.size() * 8)); CHK(hipMalloc(&dal, B * 8)); CHK(hipMalloc(&dwx, n * 8)); CHK(hipMalloc(&dwt, rows * 8));
    CHK(hipMalloc(&ds, (size_t)B * std::max(rows, n) * 8)); CHK(hipMalloc(&dchg, (size_t)B * rows * 16));
    CHK(hipMalloc(&dchg2, (size_t)B * nblk * 16));
    CHK(hipMemcpy(du, u.data(), u.size() * 8, hipMemcpyHostToDevice)); CHK(hipMemcpy(dr, r.data(), r.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(dtab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice)); CHK(hipMemcpy(dal, al.data(), B * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(dwx, wx.data(), n * 8, hipMemcpyHostToDevice)); CHK(hipMemcpy(dwt, wt.data(), rows * 8, hipMemcpyHostToDevice));
    const long ss = std::max(rows, n);
    double t_full, t_rows, t_cols;
    if (median_ms([&] { hipLaunchKernelGGL(k1d_grad_prox, dim3(rows, B), dim3(T1), 0, 0, n, (const double *)du, (const double *)dr, hs,
                                           (const double *)dal, (const double *)dtab, OPT1_STRIDE, dout, dchg); }, &t_full)) return 1;
    auto rows_kernel = k1d_group_prox_rows<GP_NV>;       // the instance the engine picks for n (gp_rows_nv)
    if (gp_rows_nv(n) == 1) rows_kernel = k1d_group_prox_rows<1>;
    else if (gp_rows_nv(n) == 2) rows_kernel = k1d_group_prox_rows<2>;
    else if (gp_rows_nv(n) == 4) rows_kernel = k1d_group_prox_rows<4>;
    if (median_ms([&] { hipLaunchKernelGGL(rows_kernel, dim3(rows, B), dim3(T1), 0, 0, n, (const double *)du, (const double *)dr,
                                           hs, (const double *)dal, (const double *)dtab, OPT1_STRIDE, (const int *)nullptr,
                                           (const double *)dwx, dout, ds, ss, dchg); }, &t_rows)) return 1;
    std::vector<double> s((size_t)B * ss);
    CHK(hipMemcpy(s.data(), ds, s.size() * 8, hipMemcpyDeviceToHost));
    long zr = 0; for (int b = 0; b < B; ++b) for (int k = 0; k < rows; ++k) zr += s[b * ss + k] == 0.0;
    if (median_ms([&] { hipLaunchKernelGGL(k1d_group_prox_cols, dim3(nblk, B), dim3(GC_T), 0, 0, n, rows, (const double *)du,
                                           (const double *)dr, hs, (const double *)dal, (const double *)dtab, OPT1_STRIDE,
                                           (const int *)nullptr, (const double *)dwt, dout, ds, ss, dchg2); }, &t_cols)) return 1;
    CHK(hipMemcpy(s.data(), ds, s.size() * 8, hipMemcpyDeviceToHost));
    long zc = 0; for (int b = 0; b < B; ++b) for (int i = 0; i < n; ++i) zc += s[b * ss + i] == 0.0;
    const double gb = 3.0 * B * hs * 8 / 1e9;        // u and r read, u+ written
    printf("N=%d steps=%d B=%d box=%s  bytes=%.3f GB\n", N, steps, B, active ? "(-1,1)" : "infinite", gb);
    printf("  k1d_grad_prox        %9.3f ms  %7.1f GB/s\n", t_full, gb / (t_full * 1e-3));
    printf("  k1d_group_prox_rows  %9.3f ms  %7.1f GB/s  x%.2f of k1d_grad_prox   zero rows %ld of %ld\n", t_rows, gb / (t_rows * 1e-3),
           t_rows / t_full, zr, (long)B * rows);
    printf("  k1d_group_prox_cols  %9.3f ms  %7.1f GB/s  x%.2f of k1d_grad_prox   zero columns %ld of %ld\n", t_cols,
           gb / (t_cols * 1e-3), t_cols / t_full, zc, (long)B * n);
    for (double *p : {du, dr, dout, dtab, dal, dwx, dwt, ds, dchg, dchg2}) hipFree(p);
    return 0;
}

int main() {
    for (int active = 0; active < 2; ++active) {
        if (run(4096, 1000, 1, active != 0)) return 1;
        if (run(256, 100, 256, active != 0)) return 1;
    }
    return 0;
}
