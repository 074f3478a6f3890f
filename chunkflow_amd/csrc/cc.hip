// Connected-components labeling on gfx950 (threshold + 6/18/26-connectivity
// union-find) — the cc3d replacement for the config-4 operator chain
// (reference flow/flow.py:1803-1829 + chunk/base.py:128-137; cc3d's labels
// are unpinned by any reference test, SURVEY.md §8c, so parity is defined
// against scipy.ndimage.label's partition AND numbering: labels are
// assigned 1..N in raster-scan first-encounter order).
//
// Algorithm: one merge pass of atomic union-find over the backward neighbor
// set (min-index root wins, so each component's root IS its first raster
// voxel), a path-compression pass, then a three-step rank assignment
// (per-chunk root counts -> host exclusive scan of the small count array ->
// wave-ballot local ranks), and a final gather. All buffers are
// caller-owned except the small per-chunk count array (context scratch).
//
// Which neighbours belong together is a predicate the kernels are templated
// on: BinaryFg (a u8 foreground mask; any two foreground neighbours unite)
// or EqualValue<T> (a label volume; non-zero neighbours unite iff their raw
// bit patterns are equal — cc3d's multi-label semantics).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

// shared context/error plumbing lives in cfx.hip; this file is compiled
// into the same shared object (see csrc/Makefile and build.py)
#include "cfx_internal.h"
// cc_ld / cc_st / cc_find_ro / cc_find / cc_union: every access to the
// parent array goes through them (the reasons are written there)
#include "cc_unionfind.h"

namespace {

constexpr int SCAN_CHUNK = 16384;  // elements ranked per workgroup

// backward (already-scanned) neighbor offsets per connectivity
// 6-conn: 3 face neighbors; 18: +6 edge; 26: +4 corner (13 total)
__device__ __constant__ int BWD[13][3] = {
    {0, 0, -1}, {0, -1, 0}, {-1, 0, 0},                    // 6
    {0, -1, -1}, {0, -1, 1}, {-1, 0, -1}, {-1, 0, 1},      // 18 (edges)
    {-1, -1, 0}, {-1, 1, 0},
    {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1},    // 26 (corners)
};

// "same component?" predicates: v is the voxel array, fg() tells foreground
// from a voxel's value, same() whether a FOREGROUND voxel of value a unites
// with a neighbour of value b
struct BinaryFg {
    const unsigned char* __restrict__ v;
    __device__ static bool fg(unsigned char a) { return a != 0; }
    __device__ static bool same(unsigned char, unsigned char b) {
        return b != 0;
    }
};

template <typename T>
struct EqualValue {
    const T* __restrict__ v;
    __device__ static bool fg(T a) { return a != 0; }
    // a != 0 here, so a == b also makes the neighbour foreground
    __device__ static bool same(T a, T b) { return a == b; }
};

template <typename P>
__global__ void k_cc_init(P pred, unsigned int* __restrict__ parent,
                          long long n) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    long long stride = gridDim.x * (long long)blockDim.x;
    for (; i < n; i += stride)
        cc_st(parent, (unsigned int)i,
              P::fg(pred.v[i]) ? (unsigned int)i : 0xFFFFFFFFu);
}

template <typename P>
__global__ void k_cc_merge(P pred, unsigned int* __restrict__ parent, int D,
                           int H, int W, int ndirs) {
    long long n = (long long)D * H * W;
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    long long stride = gridDim.x * (long long)blockDim.x;
    for (; i < n; i += stride) {
        const auto vi = pred.v[i];
        if (!P::fg(vi)) continue;
        int x = (int)(i % W);
        long long t = i / W;
        int y = (int)(t % H);
        int z = (int)(t / H);
        for (int d = 0; d < ndirs; ++d) {
            int nz = z + BWD[d][0];
            int ny = y + BWD[d][1];
            int nx = x + BWD[d][2];
            if (nz < 0 || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
            long long j = ((long long)nz * H + ny) * W + nx;
            if (P::same(vi, pred.v[j]))
                cc_union(parent, (unsigned int)i, (unsigned int)j);
        }
    }
}

template <typename P>
__global__ void k_cc_compress(P pred, unsigned int* __restrict__ parent,
                              long long n) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    long long stride = gridDim.x * (long long)blockDim.x;
    for (; i < n; i += stride)
        if (P::fg(pred.v[i]))
            cc_st(parent, (unsigned int)i,
                  cc_find_ro(parent, (unsigned int)i));
}

// one 64-lane wave per SCAN_CHUNK: count roots (parent[i] == i)
__global__ void k_cc_count(const unsigned int* __restrict__ parent,
                           long long n,
                           unsigned int* __restrict__ counts) {
    long long c0 = (long long)blockIdx.x * SCAN_CHUNK;
    if (c0 >= n) return;
    long long c1 = c0 + SCAN_CHUNK < n ? c0 + SCAN_CHUNK : n;
    unsigned int cnt = 0;
    for (long long i = c0 + threadIdx.x; i < c1; i += 64)
        if (cc_ld(parent, (unsigned int)i) == (unsigned int)i) ++cnt;
    for (int off = 32; off > 0; off >>= 1)
        cnt += __shfl_down(cnt, off, 64);
    if (threadIdx.x == 0)
        __hip_atomic_store(&counts[blockIdx.x], cnt, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// assign newlabel[root] = chunk_offset + local_rank + 1 via wave ballots
__global__ void k_cc_rank(const unsigned int* __restrict__ parent,
                          long long n,
                          const unsigned int* __restrict__ offsets,
                          unsigned int* __restrict__ newlabel) {
    long long c0 = (long long)blockIdx.x * SCAN_CHUNK;
    if (c0 >= n) return;
    long long c1 = c0 + SCAN_CHUNK < n ? c0 + SCAN_CHUNK : n;
    unsigned int base = __hip_atomic_load(
        &offsets[blockIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (long long i0 = c0; i0 < c1; i0 += 64) {
        long long i = i0 + threadIdx.x;
        bool is_root =
            i < c1 &&
            cc_ld(parent, (unsigned int)i) == (unsigned int)i;
        unsigned long long ballot = __ballot(is_root);
        if (is_root) {
            unsigned int before = (unsigned int)__popcll(
                ballot & ((1ull << threadIdx.x) - 1ull));
            __hip_atomic_store(&newlabel[i], base + before + 1,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        base += (unsigned int)__popcll(ballot);
    }
}

template <typename P>
__global__ void k_cc_final(P pred,
                           const unsigned int* __restrict__ parent,
                           const unsigned int* __restrict__ newlabel,
                           unsigned int* __restrict__ labels, long long n) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    long long stride = gridDim.x * (long long)blockDim.x;
    for (; i < n; i += stride)
        labels[i] =
            P::fg(pred.v[i])
                ? cc_ld(newlabel, cc_ld(parent, (unsigned int)i)) : 0u;
}

__global__ void k_threshold(const float* __restrict__ in,
                            unsigned char* __restrict__ fg, long long n,
                            float threshold) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    long long stride = gridDim.x * (long long)blockDim.x;
    for (; i < n; i += stride) fg[i] = in[i] > threshold ? 1 : 0;
}

__global__ void k_nonzero_u8(const unsigned char* __restrict__ in,
                             unsigned char* __restrict__ fg, long long n) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    long long stride = gridDim.x * (long long)blockDim.x;
    for (; i < n; i += stride) fg[i] = in[i] != 0 ? 1 : 0;
}

}  // namespace

// count / host scan / rank: shared with watershed.hip (cc_unionfind.h)
int cc_rank_roots(cfx_ctx* ctx, const unsigned int* parent, long long n,
                  unsigned int* newlabel, long long* total_out) {
    int nchunks = (int)((n + SCAN_CHUNK - 1) / SCAN_CHUNK);
    if (ctx->cc_counts_cap < nchunks) {
        if (ctx->cc_counts) (void)hipFree(ctx->cc_counts);
        ctx->cc_counts = nullptr;
        ctx->cc_counts_cap = 0;
        CFX_CHECK(hipMalloc(&ctx->cc_counts,
                            (size_t)nchunks * sizeof(unsigned int)));
        ctx->cc_counts_cap = nchunks;
    }
    hipLaunchKernelGGL(k_cc_count, dim3(nchunks), dim3(64), 0, ctx->stream,
                       parent, n, ctx->cc_counts);
    // exclusive scan of the (small) per-chunk counts on the host
    std::vector<unsigned int> counts(nchunks);
    CFX_CHECK(hipMemcpyAsync(counts.data(), ctx->cc_counts,
                             (size_t)nchunks * sizeof(unsigned int),
                             hipMemcpyDeviceToHost, ctx->stream));
    CFX_CHECK(hipStreamSynchronize(ctx->stream));
    unsigned long long total = 0;
    for (int i = 0; i < nchunks; ++i) {
        unsigned int c = counts[i];
        counts[i] = (unsigned int)total;
        total += c;
    }
    *total_out = (long long)total;
    CFX_CHECK(hipMemcpyAsync(ctx->cc_counts, counts.data(),
                             (size_t)nchunks * sizeof(unsigned int),
                             hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_cc_rank, dim3(nchunks), dim3(64), 0, ctx->stream,
                       parent, n, ctx->cc_counts, newlabel);
    CFX_CHECK(hipGetLastError());
    return 0;
}

namespace {

inline int grid_for(long long work, int threads) {
    long long want = (work + threads - 1) / threads;
    return (int)(want < 8192 ? want : 8192);
}

// init / merge / compress / count / rank / final over one predicate;
// elem_bytes is sizeof(P's voxel type), for the profile's byte count only
template <typename P>
int run_cc(cfx_ctx* ctx, P pred, int elem_bytes, const int dims[3],
           int connectivity, unsigned int* labels, unsigned int* scratch,
           long long* n_components) {
    int D = dims[0], H = dims[1], W = dims[2];
    if (D <= 0 || H <= 0 || W <= 0) {
        g_err = "connected_components: empty volume";
        return -1;
    }
    long long n = (long long)D * H * W;
    if (n >= 0xFFFFFFFFll) {
        g_err = "connected_components: volume exceeds u32 indexing";
        return -1;
    }
    int ndirs = connectivity == 6 ? 3 : connectivity == 18 ? 9
                : connectivity == 26 ? 13 : -1;
    if (ndirs < 0) {
        g_err = "connectivity must be 6, 18 or 26";
        return -1;
    }
    // algorithmic bytes: voxel reads x3 + parent RMW passes + final gather
    double bytes = (double)n * (3.0 * elem_bytes + 4.0 * 6.0);
    return cfx_timed(ctx, CFX_K_CC, bytes, [&] {
        hipLaunchKernelGGL(k_cc_init<P>, dim3(grid_for(n, 256)), dim3(256),
                           0, ctx->stream, pred, labels, n);
        hipLaunchKernelGGL(k_cc_merge<P>, dim3(grid_for(n, 256)), dim3(256),
                           0, ctx->stream, pred, labels, D, H, W, ndirs);
        hipLaunchKernelGGL(k_cc_compress<P>, dim3(grid_for(n, 256)),
                           dim3(256), 0, ctx->stream, pred, labels, n);
        if (cc_rank_roots(ctx, labels, n, scratch, n_components)) return -1;
        hipLaunchKernelGGL(k_cc_final<P>, dim3(grid_for(n, 256)), dim3(256),
                           0, ctx->stream, pred, labels, scratch, labels, n);
        return 0;
    });
}

}  // namespace

extern "C" int cfx_threshold(cfx_ctx* ctx, const float* in,
                             unsigned char* fg, long long n,
                             float threshold) {
    hipLaunchKernelGGL(k_threshold, dim3(grid_for(n, 256)), dim3(256), 0,
                       ctx->stream, in, fg, n, threshold);
    CFX_CHECK(hipGetLastError());
    return 0;
}

extern "C" int cfx_nonzero_u8(cfx_ctx* ctx, const unsigned char* in,
                              unsigned char* fg, long long n) {
    hipLaunchKernelGGL(k_nonzero_u8, dim3(grid_for(n, 256)), dim3(256), 0,
                       ctx->stream, in, fg, n);
    CFX_CHECK(hipGetLastError());
    return 0;
}

/* fg: device u8 foreground mask; labels: device u32 out (also used as the
 * union-find parent array); scratch: device u32, same length (root->label
 * table); n_components written on the host after a sync. */
extern "C" int cfx_connected_components(cfx_ctx* ctx,
                                        const unsigned char* fg,
                                        const int dims[3], int connectivity,
                                        unsigned int* labels,
                                        unsigned int* scratch,
                                        long long* n_components) {
    return run_cc(ctx, BinaryFg{fg}, 1, dims, connectivity, labels, scratch,
                  n_components);
}

/* seg: device label volume of 1-, 4- or 8-byte elements; one component per
 * connected region of equal non-zero value. Buffers as above. */
extern "C" int cfx_connected_components_labels(
    cfx_ctx* ctx, const void* seg, int elem_bytes, const int dims[3],
    int connectivity, unsigned int* labels, unsigned int* scratch,
    long long* n_components) {
    if (elem_bytes == 1)
        return run_cc(
            ctx, EqualValue<unsigned char>{
                     static_cast<const unsigned char*>(seg)},
            1, dims, connectivity, labels, scratch, n_components);
    if (elem_bytes == 4)
        return run_cc(
            ctx, EqualValue<unsigned int>{
                     static_cast<const unsigned int*>(seg)},
            4, dims, connectivity, labels, scratch, n_components);
    if (elem_bytes == 8)
        return run_cc(
            ctx, EqualValue<unsigned long long>{
                     static_cast<const unsigned long long*>(seg)},
            8, dims, connectivity, labels, scratch, n_components);
    g_err = "connected_components_labels: elem_bytes must be 1, 4 or 8";
    return -1;
}
