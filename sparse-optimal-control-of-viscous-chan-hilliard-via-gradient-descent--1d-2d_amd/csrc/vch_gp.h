// vch_gp.h — the prox of one group of the directional sparsity functionals, shared by the kernels of
// the 1D engine (vch_kernels1d.h) and of the 2D engine (vch_kernels2d.h).
//
// With v = u - alpha (r + b3 u) and lam = alpha kappa_s:  c = ||cone(v)|| <= lam gives u+ = 0, s = 0; otherwise
// u+ = clip(s v) with s the root of h(s) = ||clip(s v)|| (1 - s) - lam s, which is s0 = 1 - lam / ||v|| where clip(s0 v) = s0 v.
// The norm is the group's own (a row or a column in 1D, a plane or a pencil in 2D); what is here does not know which.
#pragma once
#include "vch_common.h"

constexpr int GP_FULL = 0, GP_TIME = 1, GP_SPACE = 2;      // VCH_SPARSITY_* of vch.h
// A cap, not the usual end: the bracket ends the iteration after at most 54 steps on 32 000 groups of the regimes of
// tests/test_gpu_dirsparse_edges_1d.py (a CPU port of gp_step; |c / lam - 1| >= 1e-9).  A group at the threshold itself
// (lam = c (1 - 2^-52) under a one-sided box, root at s ~ 1e-16) can run into the cap, about one group in 300 of that kind;
// the s it then holds is within 6e-16 of the bisection's.
constexpr int GP_MAXIT = 100;

// the gradient step, with its two roundings written out: every pass of a kernel recomputes the same bits
__device__ __forceinline__ double gp_v(double uu, double rr, double al, double b3) { return fma(-al, fma(b3, uu, rr), uu); }
__device__ __forceinline__ double gp_cone(double v, double umin, double umax) {
    return (umax == 0.0 && v > 0.0) || (umin == 0.0 && v < 0.0) ? 0.0 : v;
}
__device__ __forceinline__ double gp_out(double s, double v, double umin, double umax) {
    return s == 0.0 ? 0.0 : fmin(fmax(s * v, umin), umax);
}
// One step of the safeguarded iteration at s, where Q = ||clip(s v)||^2 and A = the sum of w v^2 over the nodes the box does
// not hold (d/ds ||clip(s v)|| = A s / ||clip(s v)||).  The bracket keeps h(lo) > 0 >= h(hi).  The candidate is Newton's,
// doubled while Newton closes in from one side (so that the other end of the bracket follows), else the midpoint.
// true: h vanishes or lo, hi are adjacent doubles; s is the answer.
__device__ __forceinline__ bool gp_step(double Q, double A, double lam, double &s, double &lo, double &hi) {
    const double rho = sqrt(Q);
    const double h = rho * (1.0 - s) - lam * s;
    if (h == 0.0) return true;
    if (h > 0.0) lo = s; else hi = s;
    const double dh = (rho > 0.0 ? A * s / rho : 0.0) * (1.0 - s) - rho - lam;
    const double step = -h / dh;
    double sn = fabs(step) < 0.25 * (hi - lo) ? s + 2.0 * step : s + step;
    if (!(sn > lo && sn < hi)) sn = s + step;
    if (!(sn > lo && sn < hi)) sn = lo + 0.5 * (hi - lo);
    if (!(sn > lo && sn < hi)) return true;
    s = sn;
    return false;
}
