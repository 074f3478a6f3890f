// Affinity maps to segments on gfx950: watershed fragments and the region
// graph between them — the device half of the reference's `agglomerate`
// plugin (chunkflow/plugins/agglomerate.py, which hands both steps to the
// waterz C++ wheel). waterz's labels are pinned by no reference test, so the
// semantics are defined here, order-independent and exact, and pinned to the
// numpy/scipy oracle of chunkflow_amd/watershed.py ("Watershed
// and agglomeration", lists where they knowingly differ from waterz).
//
// Input. aff is f32 (3, D, H, W), contiguous, channels x, y, z: aff[c][v]
// is the weight of the edge between voxel v and its predecessor along that
// axis. The values on the leading face of each axis belong to no edge and
// are never loaded.
//
// Fragments: a steepest-ascent forest. An edge is live iff w >= low, strong
// iff live and w >= high (NaN fails both). A voxel with a live incident edge
// picks the first one, in the order -x +x -y +y -z +z, whose weight equals
// the maximum over its live incident edges. Fragments are the components of
// the voxels under the strong and the picked edges, numbered 1..N by first
// voxel in raster order; a voxel with no live incident edge is 0. This is
// cc.hip's union-find (cc_unionfind.h) with its own init and merge:
//   init      parent = self, or CC_NONE without a live edge; the decisions
//             (pick direction, which backward edges are strong) go into the
//             scratch buffer as one code word, so the affinities are read
//             once
//   merge     union with the pick and over the strong backward edges (a
//             strong forward edge is its other end's backward edge)
//   compress / cc_rank_roots / final as in cc.hip; foreground is
//             parent != CC_NONE
//
// Region graph: every in-volume edge whose ends carry different non-zero
// fragment ids a != b adds 1 to the count and q(w) to the sum of the row
// keyed (min(a,b) << 32) | max(a,b), in a table of label_table.h's kind.
// q(w) = floor(c * 2^24), c = w > 0 ? min(w, 1) : 0 (NaN and negatives: 0).
// The product is exact in f32 and integer adds commute, so the rows are
// bit-exact whatever the order. One lane walks SEG consecutive voxels and
// keeps a running (key, count, sum) per channel: one table operation per run
// of equal keys (voxels without an edge on that channel do not end a run).
// Inside a large fragment no edge qualifies and nothing is sent. The same
// walk with a counter in place of the table (k_region_edges<true>) gives the
// number of table operations, which bounds the number of distinct keys: the
// table is sized from it.
#include <hip/hip_runtime.h>

#include <string>

#include "cfx_internal.h"
#include "cc_unionfind.h"
#include "label_table.h"

namespace {

using namespace label_table;

constexpr int kBlock = 256;
constexpr int kGridCap = 8192;
constexpr int SEG = 16;  // voxels per lane of the region-graph walk
// the region-graph walk: 8 workgroups per CU on 256 CUs, every lane
// resident at once, as for the count passes of labels.hip (the sizing pass
// ends in one add per wave to a single word: keep the waves few)
constexpr int kRegionGrid = 2048;

inline int grid_for(long long work, int cap = kGridCap) {
    long long want = (work + kBlock - 1) / kBlock;
    if (want < 1) want = 1;
    return (int)(want < cap ? want : cap);
}

// code word of a voxel: bits 0..2 the picked direction (NO_PICK: no live
// edge), bits 3..5 set where the backward edge along x, y, z is strong
constexpr unsigned int NO_PICK = 7u;

__global__ void k_ws_init(const float* __restrict__ aff, int D, int H, int W,
                          float low, float high, unsigned int* parent,
                          unsigned int* __restrict__ code) {
    const long long HW = (long long)H * W;
    const long long n = (long long)D * HW;
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long stride = gridDim.x * (long long)blockDim.x;
    for (; i < n; i += stride) {
        const int x = (int)(i % W);
        const long long t = i / W;
        const int y = (int)(t % H);
        const int z = (int)(t / H);
        // -x +x -y +y -z +z; an edge that leaves the volume does not exist
        const bool inside[6] = {x > 0, x < W - 1, y > 0,
                                y < H - 1, z > 0, z < D - 1};
        const long long at[6] = {i, i + 1, n + i, n + i + W,
                                 2 * n + i, 2 * n + i + HW};
        unsigned int pick = NO_PICK, strong = 0;
        float best = 0.0f;
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            if (!inside[d]) continue;
            const float w = aff[at[d]];
            if (!(w >= low)) continue;
            if (pick == NO_PICK || w > best) {
                pick = (unsigned int)d;
                best = w;
            }
            if ((d & 1) == 0 && w >= high) strong |= 8u << (d >> 1);
        }
        cc_st(parent, (unsigned int)i,
              pick == NO_PICK ? CC_NONE : (unsigned int)i);
        code[i] = pick | strong;
    }
}

__global__ void k_ws_merge(const unsigned int* __restrict__ code, int D,
                           int H, int W, unsigned int* parent) {
    const long long HW = (long long)H * W;
    const long long n = (long long)D * HW;
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long stride = gridDim.x * (long long)blockDim.x;
    for (; i < n; i += stride) {
        const unsigned int c = code[i];
        const unsigned int pick = c & 7u;
        if (pick == NO_PICK) continue;
        // the edge was live, so it exists and its other end has a live
        // edge too: the target is inside the volume and is foreground
        const long long step = pick < 2 ? 1 : pick < 4 ? W : HW;
        const long long j = (pick & 1u) ? i + step : i - step;
        cc_union(parent, (unsigned int)i, (unsigned int)j);
        if (c & 8u) cc_union(parent, (unsigned int)i, (unsigned int)(i - 1));
        if (c & 16u) cc_union(parent, (unsigned int)i, (unsigned int)(i - W));
        if (c & 32u)
            cc_union(parent, (unsigned int)i, (unsigned int)(i - HW));
    }
}

__global__ void k_ws_compress(unsigned int* parent, long long n) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long stride = gridDim.x * (long long)blockDim.x;
    for (; i < n; i += stride)
        if (cc_ld(parent, (unsigned int)i) != CC_NONE)
            cc_st(parent, (unsigned int)i,
                  cc_find_ro(parent, (unsigned int)i));
}

// labels is the parent array: each lane replaces its own word
__global__ void k_ws_final(const unsigned int* newlabel,
                           unsigned int* labels, long long n) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long stride = gridDim.x * (long long)blockDim.x;
    for (; i < n; i += stride) {
        const unsigned int root = cc_ld(labels, (unsigned int)i);
        labels[i] = root == CC_NONE ? 0u : cc_ld(newlabel, root);
    }
}

// ---------------------------------------------------------------------------
// region graph
// ---------------------------------------------------------------------------
__global__ void k_region_clear(unsigned long long* __restrict__ keys,
                               unsigned int* __restrict__ counts,
                               unsigned long long* __restrict__ sums,
                               long long capacity) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < capacity; i += stride) {
        keys[i] = EMPTY;
        counts[i] = 0u;
        sums[i] = 0ull;
    }
}

__device__ inline unsigned long long quantise(float w) {
    const float c = w > 0.0f ? (w < 1.0f ? w : 1.0f) : 0.0f;
    return (unsigned long long)(c * 16777216.0f);  // exact product, floor
}

// a < b never both 2^32-1, so a key is never EMPTY
struct Run {
    unsigned long long key = EMPTY;
    unsigned long long sum = 0;
    unsigned int count = 0;
};

// COUNT: `total` receives the number of runs and the table is not touched
// (aff, t, sums and status are unused); otherwise each run goes to the
// table. blockDim is a multiple of 64.
template <bool COUNT>
__global__ void k_region_edges(const unsigned int* __restrict__ frag,
                               const float* __restrict__ aff, int D, int H,
                               int W, Table t,
                               unsigned long long* __restrict__ sums,
                               unsigned long long* __restrict__ total,
                               unsigned int* __restrict__ status) {
    const long long HW = (long long)H * W;
    const long long n = (long long)D * HW;
    const long long n_items = (n + SEG - 1) / SEG;
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned int runs = 0;

    auto flush = [&](Run& r) {
        if (r.count == 0) return;
        if (COUNT) {
            ++runs;
        } else {
            const long long slot = table_insert(t, r.key, status);
            if (slot >= 0) {
                atomicAdd(&t.vals[slot], r.count);
                atomicAdd(&sums[slot], r.sum);
            }
        }
        r.count = 0;
        r.sum = 0;
    };
    auto edge = [&](Run& r, unsigned int a, unsigned int b, long long at) {
        if (b == 0u || b == a) return;
        const unsigned int lo = a < b ? a : b;
        const unsigned long long key =
            ((unsigned long long)lo << 32) | (a ^ b ^ lo);
        if (key != r.key) {
            flush(r);
            r.key = key;
        }
        ++r.count;
        if (!COUNT) r.sum += quantise(aff[at]);
    };

    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         item < n_items; item += stride) {
        const long long s = item * SEG;
        const int len = (int)(n - s < SEG ? n - s : SEG);
        int x = (int)(s % W);
        const long long row = s / W;
        int y = (int)(row % H);
        int z = (int)(row / H);
        unsigned int left = s > 0 ? frag[s - 1] : 0u;
        Run rx, ry, rz;
#pragma unroll 1
        for (int j = 0; j < len; ++j) {
            const long long v = s + j;
            const unsigned int a = frag[v];
            if (a != 0u) {
                if (x > 0) edge(rx, a, left, v);
                if (y > 0) edge(ry, a, frag[v - W], n + v);
                if (z > 0) edge(rz, a, frag[v - HW], 2 * n + v);
            }
            left = a;
            if (++x == W) {
                x = 0;
                if (++y == H) {
                    y = 0;
                    ++z;
                }
            }
        }
        flush(rx);
        flush(ry);
        flush(rz);
    }
    if (COUNT) {
        for (int off = 32; off > 0; off >>= 1)
            runs += __shfl_down(runs, off, 64);
        if ((threadIdx.x & 63) == 0 && runs)
            atomicAdd(total, (unsigned long long)runs);
    }
}

int check_dims(const int dims[3], long long limit, const char* who,
               long long* n) {
    if (dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0) {
        g_err = std::string(who) + ": empty volume";
        return -1;
    }
    *n = (long long)dims[0] * dims[1] * dims[2];
    if (*n > limit) {
        g_err = std::string(who) + ": volume exceeds u32 indexing";
        return -1;
    }
    return 0;
}

// three edges per voxel at most, and a row's count is a u32
constexpr long long REGION_MAX_VOXELS = 0xFFFFFFFFll / 3;

}  // namespace

/* aff: device f32 (3, D, H, W); labels: device u32 out (also the union-find
 * parent array); scratch: device u32, same length (the code words, then the
 * root->label table); n_components written on the host after a sync. */
extern "C" int cfx_affinity_fragments(cfx_ctx* ctx, const float* aff,
                                      const int dims[3], float low,
                                      float high, unsigned int* labels,
                                      unsigned int* scratch,
                                      long long* n_components) {
    const char* who = "affinity_fragments";
    long long n;
    if (check_dims(dims, 0xFFFFFFFEll, who, &n)) return -1;
    if (!aff || !labels || !scratch || !n_components) {
        g_err = std::string(who) + ": null argument";
        return -1;
    }
    const int D = dims[0], H = dims[1], W = dims[2];
    // algorithmic bytes: the map once, the code word written and read, the
    // parent passes and the final gather as in cc.hip
    double bytes = (double)n * (12.0 + 8.0 + 4.0 * 6.0);
    return cfx_timed(ctx, CFX_K_CC, bytes, [&] {
        hipLaunchKernelGGL(k_ws_init, dim3(grid_for(n)), dim3(kBlock), 0,
                           ctx->stream, aff, D, H, W, low, high, labels,
                           scratch);
        hipLaunchKernelGGL(k_ws_merge, dim3(grid_for(n)), dim3(kBlock), 0,
                           ctx->stream, scratch, D, H, W, labels);
        hipLaunchKernelGGL(k_ws_compress, dim3(grid_for(n)), dim3(kBlock), 0,
                           ctx->stream, labels, n);
        if (cc_rank_roots(ctx, labels, n, scratch, n_components)) return -1;
        hipLaunchKernelGGL(k_ws_final, dim3(grid_for(n)), dim3(kBlock), 0,
                           ctx->stream, scratch, labels, n);
        return 0;
    });
}

/* number of table operations cfx_region_graph will make on this volume: an
 * upper bound on its number of rows. Synchronous. */
extern "C" int cfx_region_graph_runs(cfx_ctx* ctx, const unsigned int* frag,
                                     const int dims[3], long long* n_runs) {
    const char* who = "region_graph_runs";
    long long n;
    if (check_dims(dims, REGION_MAX_VOXELS, who, &n)) return -1;
    if (!frag || !n_runs) {
        g_err = std::string(who) + ": null argument";
        return -1;
    }
    unsigned long long* words;
    if (status_words(ctx, &words)) return -1;
    int rc = cfx_timed(ctx, CFX_K_LABELS, 4.0 * (double)n, [&] {
        CFX_CHECK(hipMemsetAsync(words, 0, sizeof(unsigned long long),
                                 ctx->stream));
        hipLaunchKernelGGL(k_region_edges<true>,
                           dim3(grid_for((n + SEG - 1) / SEG, kRegionGrid)),
                           dim3(kBlock), 0, ctx->stream, frag, nullptr,
                           dims[0], dims[1], dims[2],
                           Table{nullptr, nullptr, 0}, nullptr, words,
                           nullptr);
        return 0;
    });
    if (rc) return rc;
    unsigned long long total = 0;
    CFX_CHECK(hipMemcpyAsync(&total, words, sizeof(total),
                             hipMemcpyDeviceToHost, ctx->stream));
    CFX_CHECK(hipStreamSynchronize(ctx->stream));
    *n_runs = (long long)total;
    return 0;
}

/* keys u64 / counts u32 / sums u64 [capacity]: cleared here, then filled.
 * Synchronous (reads the status flags back). */
extern "C" int cfx_region_graph(cfx_ctx* ctx, const unsigned int* frag,
                                const float* aff, const int dims[3],
                                unsigned long long* keys,
                                unsigned int* counts,
                                unsigned long long* sums,
                                long long capacity) {
    const char* who = "region_graph";
    long long n;
    if (check_dims(dims, REGION_MAX_VOXELS, who, &n)) return -1;
    if (!frag || !aff || !sums) {
        g_err = std::string(who) + ": null argument";
        return -1;
    }
    if (check_table(keys, counts, capacity, who)) return -1;
    unsigned long long* words;
    if (status_words(ctx, &words)) return -1;
    unsigned int* status = reinterpret_cast<unsigned int*>(words + 1);
    Table t{keys, counts, (unsigned long long)capacity - 1};
    int rc = cfx_timed(ctx, CFX_K_LABELS, 4.0 * (double)n, [&] {
        CFX_CHECK(hipMemsetAsync(words + 1, 0, sizeof(unsigned long long),
                                 ctx->stream));
        hipLaunchKernelGGL(k_region_clear, dim3(grid_for(capacity)),
                           dim3(kBlock), 0, ctx->stream, keys, counts, sums,
                           capacity);
        hipLaunchKernelGGL(k_region_edges<false>,
                           dim3(grid_for((n + SEG - 1) / SEG, kRegionGrid)),
                           dim3(kBlock), 0, ctx->stream, frag, aff, dims[0],
                           dims[1], dims[2], t, sums, nullptr, status);
        return 0;
    });
    if (rc) return rc;
    return read_status(ctx, words + 1, who);
}
