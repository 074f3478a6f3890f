// Shared internals of the chunkflow_amd extension (every csrc/*.hip
// is compiled into one shared object).
#ifndef CFX_INTERNAL_H
#define CFX_INTERNAL_H

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/chunkflow_amd.h"

struct ProfEntry {
    hipEvent_t e0, e1;
    int kid;
    double bytes;
};

struct cfx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  // legacy default stream unless adopted
    bool profile = false;
    std::vector<ProfEntry> pending;
    unsigned long long prof_count[CFX_K_COUNT] = {};
    double prof_ms[CFX_K_COUNT] = {};
    double prof_bytes[CFX_K_COUNT] = {};
    unsigned int* dev_max = nullptr;   // scratch for cfx_max
    unsigned int* cc_counts = nullptr;  // per-chunk root counts (cc.hip)
    int cc_counts_cap = 0;
    // run-start total + status flags (labels.hip)
    unsigned long long* label_words = nullptr;
};

extern thread_local std::string g_err;

#define CFX_CHECK(expr)                                                      \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) {                                              \
            g_err = std::string(#expr) + ": " + hipGetErrorString(_e);       \
            return -1;                                                       \
        }                                                                    \
    } while (0)

// the event half of cfx_timed (cfx.hip): an event created and recorded on
// ctx->stream, and the end of a region, which owns e0 whatever happens
int timed_open(cfx_ctx* ctx, hipEvent_t* e);
int timed_close(cfx_ctx* ctx, hipEvent_t e0, int rc, int kid, double work);

// One timed region: enqueue() launches on ctx->stream and returns 0, or
// sets g_err and returns non-zero, which is passed on. A launch error
// (hipGetLastError) fails the region too. With profiling on, a region that
// succeeds pushes one ledger row {kid, work}; one that fails on any path
// pushes none and leaves no event behind. With profiling off nothing but
// enqueue() and the error check runs.
template <typename F>
int cfx_timed(cfx_ctx* ctx, int kid, double work, F&& enqueue) {
    if (!ctx->profile) {
        if (int rc = enqueue()) return rc;
        CFX_CHECK(hipGetLastError());
        return 0;
    }
    hipEvent_t e0;
    if (timed_open(ctx, &e0)) return -1;
    return timed_close(ctx, e0, enqueue(), kid, work);
}

#endif  // CFX_INTERNAL_H
