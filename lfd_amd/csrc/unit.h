// unit.h -- what a measurement unit (defocus.hip, sky/, inject/, radon/, stack/) shares with lfdmi.hip and with the other units:
// the context as a unit sees it, the check macros, the stream-ordered allocator of a call, the device guard of a destroy, the
// argument checks with their codes and messages, and (rho, theta) of a line.  Host side only: no kernel header includes it, so
// no unit's code object depends on it.  lfdmi.hip includes it too, which holds the ctx_* definitions to these declarations.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lfdmi.h"

// ---- the context's internals (defined in lfdmi.hip, not exported) ----------------------------------------------------------------
#define LFD_HIDDEN __attribute__((visibility("hidden")))
LFD_HIDDEN int ctx_begin(lfdmi_ctx *ctx);   // an entry point's start: not while calls are in flight; the ctx's device, no stale error
LFD_HIDDEN int ctx_fail(lfdmi_ctx *ctx, int code, const std::string &msg);   // sets lfdmi_last_error, returns code
LFD_HIDDEN hipStream_t ctx_stream(lfdmi_ctx *ctx);
LFD_HIDDEN int ctx_device(lfdmi_ctx *ctx);
LFD_HIDDEN void **ctx_defocus(lfdmi_ctx *ctx, void (*release)(lfdmi_ctx *));   // the defocus workspace's slot; release: called by lfdmi_ctx_destroy

// ---- checks of a HIP call and of a launch, in a function that has `ctx` and returns a status ----------------------------------------
#define UHIP(expr)                                                                                      \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return ctx_fail(ctx, LFDMI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define ULAUNCH(name)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = hipGetLastError();                                                              \
        if (e_ != hipSuccess) return ctx_fail(ctx, LFDMI_ERR_HIP, std::string("launch ") + name + ": " + hipGetErrorString(e_)); \
    } while (0)

// stream-ordered allocations of one call: whatever path leaves the call, they are queued for release behind its work
struct LFD_HIDDEN Pool {
    hipStream_t st;
    std::vector<void *> mem;
    explicit Pool(hipStream_t s) : st(s) {}
    ~Pool() {   // (a call that fails leaves here: the queued copies still read the call's host arrays, so it waits)
        if (!mem.empty()) { release(); (void)hipStreamSynchronize(st); }
    }
    void release() {
        for (void *m : mem) (void)hipFreeAsync(m, st);
        mem.clear();
    }
    template <class T> hipError_t get(T **out, size_t count) {
        void *m = nullptr;
        hipError_t e = hipMallocAsync(&m, std::max<size_t>(count, 1) * sizeof(T), st);
        if (e == hipSuccess) mem.push_back(m);
        *out = (T *)m;
        return e;
    }
};

// a handle's device is current while this lives; afterwards the caller's is again, if it was another
struct LFD_HIDDEN DeviceGuard {
    int cur = -1, dev;
    explicit DeviceGuard(int device) : dev(device) {
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (cur >= 0 && cur != dev) hipSetDevice(cur);
    }
};

// ---- argument checks of the entry point `fn`: 0, or the code ctx_fail returned (static: a copy per unit, none exported) -------------
static inline int unit_dtype(lfdmi_ctx *ctx, const char *fn, int dtype) {
    if (dtype != LFDMI_F32 && dtype != LFDMI_F32_BE) return ctx_fail(ctx, LFDMI_ERR_ARG, std::string(fn) + " takes LFDMI_F32 / LFDMI_F32_BE frames");
    return 0;
}
static inline int unit_loc(lfdmi_ctx *ctx, int loc) {
    if (loc != LFDMI_HOST && loc != LFDMI_DEVICE && loc != LFDMI_HOST_PINNED) return ctx_fail(ctx, LFDMI_ERR_ARG, "bad loc");
    return 0;
}
// sigma: NULL (0.025f for every frame) or n positive finite values; copied into *out where the caller wants them
static inline int unit_sigma(lfdmi_ctx *ctx, const char *fn, const float *sigma, int n, std::vector<float> *out) {
    if (out) out->assign(n, 0.025f);
    if (sigma)
        for (int i = 0; i < n; i++) {
            if (!std::isfinite(sigma[i]) || !(sigma[i] > 0)) return ctx_fail(ctx, LFDMI_ERR_ARG, std::string(fn) + ": sigma must be positive");
            if (out) (*out)[i] = sigma[i];
        }
    return 0;
}

// (rho, theta) of the line through (x, y) with the unit direction (dx, dy): its normal turned into theta in [0, pi]
static inline void line_rho_theta(double x, double y, double dx, double dy, double *rho, double *theta) {
    double nx = dy, ny = -dx;
    if (ny < 0.0 || (ny == 0.0 && nx < 0.0)) { nx = -nx; ny = -ny; }
    *theta = atan2(ny, nx);
    *rho = x * nx + y * ny;
}
