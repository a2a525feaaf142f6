// vch_common.h — shared host/device definitions of the HIP engine (gfx950 / MI355X).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <math.h>
#include <string>
#include <vector>
#include "../../include/vch.h"
#include "vch_mem.h"

// ----------------------------------------------------------------------------------
// error plumbing
// ----------------------------------------------------------------------------------
extern thread_local char g_vch_err[512];
static inline int vch_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_vch_err, sizeof(g_vch_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIPCHK(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            (void)hipGetLastError();     /* reset the sticky error for later launch checks */ \
            return vch_fail(VCH_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                            \
        }                                                                                   \
    } while (0)
// A request to a context's pool (vch_mem.h), checked like the HIP call behind it: the pool hands the runtime's status through,
// and a refused request (vch_mem_refuse_after) reads as hipErrorOutOfMemory.  vch_hip_mem() is the runtime table of every pool.
static_assert(VCH_MEM_REFUSED == (int)hipErrorOutOfMemory, "a refused request must read as out of memory");
const vch_mem_fns *vch_hip_mem();
#define MEMCHK(call) HIPCHK((hipError_t)(call))
#define VCHCHK(call)                   \
    do {                               \
        int r_ = (call);               \
        if (r_ < 0) return r_;         \
    } while (0)
#define CTXCHK(c)                                                             \
    do {                                                                      \
        if (!(c)) return vch_fail(VCH_ERR_ARG, "%s: NULL context", __func__); \
        HIPCHK(hipSetDevice((c)->device));                                    \
    } while (0)
#define ARGCHK(cond, msg)                                                   \
    do {                                                                    \
        if (!(cond)) return vch_fail(VCH_ERR_ARG, "%s: %s", __func__, msg); \
    } while (0)
// Launch on the stream of the context `c` in scope, `lds` bytes of dynamic LDS; a failed launch fails the calling function.
// launch_begin / launch_end are the engine's bookkeeping around it (profiling class cls, -1 = none).
#define LAUNCH_LDS(cls, kern, grid, block, lds, ...)                                         \
    do {                                                                                    \
        const bool rec_ = launch_begin(c, cls);                                             \
        hipLaunchKernelGGL(kern, grid, block, lds, c->stream, __VA_ARGS__);                 \
        launch_end(c, cls, rec_);                                                           \
        hipError_t e_ = hipGetLastError();                                                  \
        if (e_ != hipSuccess)                                                               \
            return vch_fail(VCH_ERR_HIP, "launch %s: %s", #kern, hipGetErrorString(e_));    \
    } while (0)
#define LAUNCH(kern, grid, block, ...) LAUNCH_LDS(-1, kern, grid, block, 0, __VA_ARGS__)

// ----------------------------------------------------------------------------------
// geometry of one padded plane in HBM
//
// A field of the reference is an (Nx+1, Ny+1) row-major array.  Its Laplacian matrix is
// kron(I_{Ny+1}, Lx) + kron(Ly, I_{Nx+1}) applied to the y-fastest ravel (F2:125-152), i.e.
// the operator acts on the flat memory reinterpreted as `ns = Ny+1` rows of `nf = Nx+1`
// entries: hx-stencil along the fast axis, hy-stencil along the slow axis.  The engine stores
// exactly that reinterpretation, rows padded to `pitch` doubles (multiple of 8 => every row
// starts on a 64-byte boundary).
// ----------------------------------------------------------------------------------
struct Geom {
    int nf, ns;        // fast / slow extents
    int pitch;         // padded fast extent (doubles)
    int tiles_f, tiles_s;
    long plane;        // ns * pitch (doubles)
    double ax, ay;     // 1/hx^2 (fast axis), 1/hy^2 (slow axis)
};

constexpr int TX = 64;      // tile extent along the fast axis (one wavefront wide)
#ifndef VCH_TY
#define VCH_TY 16
#endif
constexpr int TY = VCH_TY;  // tile extent along the slow axis (A/B knob: 8 or 16; every thread owns TY / 4 rows)
constexpr int NTH = 256;    // threads per workgroup = 4 wavefronts
constexpr int NPART = 6;    // partial-reduction slots per workgroup

constexpr double DELTA_SEP = 1e-2;   // F2:510
