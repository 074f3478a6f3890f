// The atomic union-find shared by the labellers (cc.hip: voxel predicates;
// watershed.hip: affinity edges). Device helpers only; the rank passes that
// turn roots into labels 1..N stay in cc.hip behind cc_rank_roots().
#ifndef CFX_CC_UNIONFIND_H
#define CFX_CC_UNIONFIND_H

#include <hip/hip_runtime.h>

#include "cfx_internal.h"

// parent value of a voxel that belongs to no component (volumes hold fewer
// than 2^32-1 voxels, so it is no index)
constexpr unsigned int CC_NONE = 0xFFFFFFFFu;

// Every parent access is an agent-scope relaxed atomic (lowered to an
// sc1 load/store that bypasses the per-CU L1): a mid-chain node j can only
// ever READ as "p[j]==j" from a stale init-era L1 line — plain loads
// produced exactly that (~0.7% of voxels compressed to a non-root on real
// volumes; MI355X_MICROARCH.md §inter-workgroup visibility).
__device__ inline unsigned int cc_ld(const unsigned int* p, unsigned int x) {
    return __hip_atomic_load(&p[x], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void cc_st(unsigned int* p, unsigned int x,
                             unsigned int v) {
    __hip_atomic_store(&p[x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// read-only find: used where a halving store could overwrite another
// thread's already-compressed root (the compress kernels: thread T2
// shortcutting THROUGH node i with a stale-read mid-chain ancestor would
// clobber T1's final parent[i]=root store — observed as ~1e-4 of voxels
// labeled from unwritten scratch)
__device__ inline unsigned int cc_find_ro(const unsigned int* p,
                                          unsigned int x) {
    unsigned int px = cc_ld(p, x);
    while (px != x) {
        x = px;
        px = cc_ld(p, x);
    }
    return x;
}

__device__ inline unsigned int cc_find(unsigned int* __restrict__ p,
                                       unsigned int x) {
    unsigned int px = cc_ld(p, x);
    while (px != x) {
        unsigned int ppx = cc_ld(p, px);
        cc_st(p, x, ppx);  // path halving (ancestor store, benign race)
        x = ppx;
        px = cc_ld(p, x);
    }
    return x;
}

__device__ inline void cc_union(unsigned int* __restrict__ p,
                                unsigned int a, unsigned int b) {
    while (true) {
        a = cc_find(p, a);
        b = cc_find(p, b);
        if (a == b) return;
        unsigned int lo = a < b ? a : b;
        unsigned int hi = a ^ b ^ lo;
        unsigned int old = atomicCAS(&p[hi], hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

// Defined in cc.hip. parent[0..n) is a compressed forest (every voxel
// holds its root or CC_NONE): counts the roots per rank chunk, scans the
// counts on the host (one sync), and writes newlabel[root] = 1 + the number
// of roots before it in flat order. *total is the number of roots.
int cc_rank_roots(cfx_ctx* ctx, const unsigned int* parent, long long n,
                  unsigned int* newlabel, long long* total);

#endif  // CFX_CC_UNIONFIND_H
