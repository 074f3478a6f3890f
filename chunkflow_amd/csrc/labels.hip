// Per-label voxel counts, label masking and the contingency table of two
// label volumes on gfx950: the device primitives under
// chunkflow_amd/segmentation.py (unique_counts, mask_fragments, mask_except —
// the reference's mask-out-objects operator, flow/flow.py:2015-2050 +
// chunk/segmentation.py:86-109; contingency — its evaluate-segmentation
// operator, flow/flow.py:1519-1542, see the pair count pass below).
//
// Label table: open addressing with linear probing in caller-owned HBM.
//   keys  u64[capacity]  32-bit labels are zero-extended; all-ones = empty,
//                        so the label 2^64-1 is out of contract (the count
//                        and insert kernels flag it as an error)
//   vals  u32[capacity]  a voxel count, or a keep flag for mask_except
// capacity is a power of two. The slot of a key is a 64-bit mix of ALL its
// bits masked to the capacity, so label sets that agree in their low bits
// (multiples of the capacity, ids differing only above bit 32) still spread.
// Keys are only ever claimed (empty -> key, by CAS), never released, so a
// probe sequence that meets its key or an empty slot is final. Every probe
// loop runs at most `capacity` steps: on a table that is too small the
// kernel raises a status flag and moves on, and the entry point returns an
// error after the launch instead of spinning.
//
// The label stream is walked in flat (z,y,x) order. One lane owns SEG_BYTES
// contiguous bytes (16 u32 / 8 u64 labels, four 16-byte loads) and keeps a
// running (label, length): the table sees one insert + one atomicAdd (count
// pass) or one lookup (apply pass) per RUN of equal labels in the segment,
// not per voxel. A wave whose 64 segments all hold one and the same label —
// background, the inside of a large object — combines them into a single
// add, and a workgroup collects its runs in a small LDS table that it
// flushes to HBM once at its end. Integer adds commute, so counts are exact
// whatever the order.
//
// Alignment: the vector body starts at the first 16-byte-aligned element;
// the elements before it and the partial segment after the last whole one
// go through the scalar kernel (same code, element loads). An input and
// output whose addresses differ modulo 16 take the scalar kernel throughout,
// as the downsample kernels do for a misaligned start.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <type_traits>

#include "cfx_internal.h"
// Table, table_insert / table_find, the status flags and their read-back
#include "label_table.h"

namespace {

using namespace label_table;

constexpr int kBlock = 256;
constexpr int SEG_BYTES = 64;  // per lane: half a 128-byte line
constexpr int kCountGrid = 2048;  // 8 workgroups per CU on 256 CUs

inline int grid_for(long long items) {
    long long want = (items + kBlock - 1) / kBlock;
    if (want < 1) want = 1;
    return (int)(want < 16384 ? want : 16384);
}

template <typename T, int N>
union Vec {
    uint4 q;
    T e[N];
};

// Walk the lane's segment p[0..len) and call f(value, position, e) per
// element, in order; e is the element's compile-time index within its
// 16-byte vector (0 on the scalar path). VEC: len == SEG and p is 16-byte
// aligned.
template <typename T, bool VEC, typename F>
__device__ inline void walk_segment(const T* __restrict__ p, int len, F&& f) {
    constexpr int E = 16 / (int)sizeof(T);
    constexpr int SEG = SEG_BYTES / (int)sizeof(T);
    if (VEC) {
#pragma unroll 1
        for (int c = 0; c < SEG / E; ++c) {
            Vec<T, E> v;
            v.q = *reinterpret_cast<const uint4*>(p + c * E);
#pragma unroll
            for (int e = 0; e < E; ++e) f(v.e[e], c * E + e, e);
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < len; ++j) f(p[j], j, 0);
    }
}

// ---------------------------------------------------------------------------
// table maintenance
// ---------------------------------------------------------------------------
__global__ void k_table_clear(unsigned long long* __restrict__ keys,
                              unsigned int* __restrict__ vals,
                              long long capacity) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < capacity; i += stride) {
        keys[i] = EMPTY;
        vals[i] = 0u;
    }
}

__global__ void k_table_insert(Table t, const unsigned long long* ids,
                               long long n_ids, unsigned int value,
                               unsigned int* status) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < n_ids; i += stride) {
        unsigned long long key = ids[i];
        if (key == EMPTY) {
            atomicOr(status, ST_RESERVED);
            continue;
        }
        long long slot = table_insert(t, key, status);
        // every writer of a slot stores the same value
        if (slot >= 0)
            __hip_atomic_store(&t.vals[slot], value, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------
// run starts: voxels that differ from their flat predecessor, plus voxel 0
// ---------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ void k_run_starts(const T* __restrict__ in, long long begin,
                             long long end,
                             unsigned long long* __restrict__ total) {
    constexpr int SEG = SEG_BYTES / (int)sizeof(T);
    const long long n_items = (end - begin + SEG - 1) / SEG;
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned int starts = 0;
    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         item < n_items; item += stride) {
        long long s = begin + item * SEG;
        int len = (int)(end - s < SEG ? end - s : SEG);
        bool have_prev = s > 0;
        T prev = have_prev ? in[s - 1] : T(0);
        walk_segment<T, VEC>(in + s, len, [&](T v, int, int) {
            starts += (!have_prev || v != prev) ? 1u : 0u;
            have_prev = true;
            prev = v;
        });
    }
    for (int off = 32; off > 0; off >>= 1)
        starts += __shfl_down(starts, off, 64);
    if ((threadIdx.x & 63) == 0 && starts) atomicAdd(total, (unsigned long long)starts);
}

// ---------------------------------------------------------------------------
// count pass
// ---------------------------------------------------------------------------
__device__ inline void count_run(const Table& t, unsigned long long key,
                                 unsigned int len, unsigned int* status) {
    if (key == EMPTY) {
        atomicOr(status, ST_RESERVED);
        return;
    }
    long long slot = table_insert(t, key, status);
    if (slot >= 0) atomicAdd(&t.vals[slot], len);
}

// A small table of the same kind in LDS collects a workgroup's runs first:
// a volume with few labels (background, large objects) would otherwise send
// every run's add to the same few HBM words. A key that finds no LDS slot
// within LDS_PROBES steps goes straight to the HBM table, so a workgroup
// that meets more labels than the LDS table holds loses nothing.
constexpr int LDS_SLOTS = 512;
constexpr int LDS_PROBES = 4;

__device__ inline void count_run_lds(unsigned long long* lkeys,
                                     unsigned int* lvals, const Table& t,
                                     unsigned long long key,
                                     unsigned int len,
                                     unsigned int* status) {
    if (key == EMPTY) {
        atomicOr(status, ST_RESERVED);
        return;
    }
    unsigned int slot = (unsigned int)(mix64(key) >> 40) & (LDS_SLOTS - 1);
    for (int probe = 0; probe < LDS_PROBES; ++probe) {
        unsigned long long k = __hip_atomic_load(
            &lkeys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == EMPTY) k = atomicCAS(&lkeys[slot], EMPTY, key);
        if (k == EMPTY || k == key) {
            atomicAdd(&lvals[slot], len);
            return;
        }
        slot = (slot + 1) & (LDS_SLOTS - 1);
    }
    count_run(t, key, len, status);
}

// blockDim is a multiple of 64 and the loop bound depends on the wave's
// first item only, so all 64 lanes of a wave make the same number of trips
// and the cross-lane operations below are convergent
template <typename T, bool VEC>
__global__ void k_count(const T* __restrict__ in, long long begin,
                        long long end, Table t, unsigned int* status) {
    constexpr int SEG = SEG_BYTES / (int)sizeof(T);
    __shared__ unsigned long long lkeys[LDS_SLOTS];
    __shared__ unsigned int lvals[LDS_SLOTS];
    for (int i = threadIdx.x; i < LDS_SLOTS; i += blockDim.x) {
        lkeys[i] = EMPTY;
        lvals[i] = 0u;
    }
    __syncthreads();
    const long long n_items = (end - begin + SEG - 1) / SEG;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (long long item0 = (long long)blockIdx.x * blockDim.x
                           + (threadIdx.x - lane);
         item0 < n_items; item0 += stride) {
        const long long item = item0 + lane;
        const bool active = item < n_items;
        T cur = T(0);
        unsigned int runlen = 0, flushed = 0;
        if (active) {
            long long s = begin + item * SEG;
            int len = (int)(end - s < SEG ? end - s : SEG);
            walk_segment<T, VEC>(in + s, len, [&](T v, int, int) {
                if (runlen != 0 && v != cur) {
                    count_run_lds(lkeys, lvals, t, (unsigned long long)cur,
                                  runlen, status);
                    ++flushed;
                    runlen = 0;
                }
                cur = v;
                ++runlen;
            });
        }
        // a wave whose 64 segments hold one label adds once; lane 0 of a
        // wave with any active lane is active (items ascend)
        const T first = __shfl(cur, 0, 64);
        const bool uniform =
            __all(!active || (flushed == 0 && cur == first));
        if (uniform) {
            unsigned int sum = active ? runlen : 0u;
            for (int off = 32; off > 0; off >>= 1)
                sum += __shfl_down(sum, off, 64);
            if (lane == 0 && active)
                count_run_lds(lkeys, lvals, t, (unsigned long long)cur, sum,
                              status);
        } else if (active) {
            count_run_lds(lkeys, lvals, t, (unsigned long long)cur, runlen,
                          status);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LDS_SLOTS; i += blockDim.x)
        if (lkeys[i] != EMPTY) count_run(t, lkeys[i], lvals[i], status);
}

// ---------------------------------------------------------------------------
// pair count pass: the contingency table of two volumes walked in lockstep.
// Both volumes were counted into tables of their own first, so every label
// has a slot there; the key of a (seg, gt) pair is (slot_seg << 32) | slot_gt,
// a u64 that goes through the same Table code as a label. Single tables are
// at most 2^31 slots, so a pair key never has its top bit set and cannot
// equal EMPTY. The single tables are read-only here: table_find is safe.
//
// One lane owns PSEG = SEG_BYTES / max(element size) voxels of each volume
// and keeps a running (seg, gt, length): one table operation per run of equal
// PAIRS, and a slot is looked up again only for the side that changed.
// ---------------------------------------------------------------------------
constexpr unsigned int NO_SLOT = 0xFFFFFFFFu;  // above any slot of a 2^31 table

template <typename T, int N>
struct alignas(sizeof(T) * N) Pack {
    T e[N];
};

template <typename TS, typename TG>
struct PairGeom {
    static constexpr int WIDE =
        (int)(sizeof(TS) > sizeof(TG) ? sizeof(TS) : sizeof(TG));
    static constexpr int E = 16 / WIDE;          // voxels per load step
    static constexpr int SEG = SEG_BYTES / WIDE;  // voxels per lane
};

// f(seg value, gt value) per voxel of the lane's segment, in order. VEC:
// len == SEG and both pointers are aligned to their E-element load (16 bytes
// for the wider type, 8 for a u32 stream beside a u64 one).
template <typename TS, typename TG, bool VEC, typename F>
__device__ inline void walk_pair_segment(const TS* __restrict__ ps,
                                         const TG* __restrict__ pg, int len,
                                         F&& f) {
    constexpr int E = PairGeom<TS, TG>::E;
    constexpr int SEG = PairGeom<TS, TG>::SEG;
    if (VEC) {
#pragma unroll 1
        for (int c = 0; c < SEG / E; ++c) {
            Pack<TS, E> a = *reinterpret_cast<const Pack<TS, E>*>(ps + c * E);
            Pack<TG, E> b = *reinterpret_cast<const Pack<TG, E>*>(pg + c * E);
#pragma unroll
            for (int e = 0; e < E; ++e) f(a.e[e], b.e[e]);
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < len; ++j) f(ps[j], pg[j]);
    }
}

// slot of a label in its own (finished) table; NO_SLOT with a status flag
// for the reserved label and for one the table does not hold
__device__ inline unsigned int pair_slot(const Table& t,
                                         unsigned long long key,
                                         unsigned int* status) {
    if (key == EMPTY) {
        atomicOr(status, ST_RESERVED);
        return NO_SLOT;
    }
    long long slot = table_find(t, key);
    if (slot < 0) {
        atomicOr(status, ST_MISSING);
        return NO_SLOT;
    }
    return (unsigned int)slot;
}

__device__ inline void count_pair_lds(unsigned long long* lkeys,
                                      unsigned int* lvals, const Table& t,
                                      unsigned int ss, unsigned int sg,
                                      unsigned int len,
                                      unsigned int* status) {
    if (ss == NO_SLOT || sg == NO_SLOT) return;  // already flagged
    count_run_lds(lkeys, lvals, t, ((unsigned long long)ss << 32) | sg, len,
                  status);
}

// same convergence argument as k_count
template <typename TS, typename TG, bool VEC>
__global__ void k_pair_count(const TS* __restrict__ seg,
                             const TG* __restrict__ gt, long long begin,
                             long long end, Table ts, Table tg, Table t,
                             unsigned int* status) {
    constexpr int SEG = PairGeom<TS, TG>::SEG;
    __shared__ unsigned long long lkeys[LDS_SLOTS];
    __shared__ unsigned int lvals[LDS_SLOTS];
    for (int i = threadIdx.x; i < LDS_SLOTS; i += blockDim.x) {
        lkeys[i] = EMPTY;
        lvals[i] = 0u;
    }
    __syncthreads();
    const long long n_items = (end - begin + SEG - 1) / SEG;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (long long item0 = (long long)blockIdx.x * blockDim.x
                           + (threadIdx.x - lane);
         item0 < n_items; item0 += stride) {
        const long long item = item0 + lane;
        const bool active = item < n_items;
        TS cs = TS(0);
        TG cg = TG(0);
        unsigned int ss = NO_SLOT, sg = NO_SLOT;
        unsigned int runlen = 0, flushed = 0;
        if (active) {
            long long s = begin + item * SEG;
            int len = (int)(end - s < SEG ? end - s : SEG);
            walk_pair_segment<TS, TG, VEC>(
                seg + s, gt + s, len, [&](TS vs, TG vg) {
                    const bool first = runlen == 0;
                    const bool ds = first || vs != cs;
                    const bool dg = first || vg != cg;
                    if (ds || dg) {
                        if (!first) {
                            count_pair_lds(lkeys, lvals, t, ss, sg, runlen,
                                           status);
                            ++flushed;
                            runlen = 0;
                        }
                        if (ds) {
                            cs = vs;
                            ss = pair_slot(ts, (unsigned long long)vs,
                                           status);
                        }
                        if (dg) {
                            cg = vg;
                            sg = pair_slot(tg, (unsigned long long)vg,
                                           status);
                        }
                    }
                    ++runlen;
                });
        }
        // slots are one-to-one with labels: equal slot pairs, equal pairs
        const unsigned long long key = ((unsigned long long)ss << 32) | sg;
        const unsigned long long first = __shfl(key, 0, 64);
        const bool uniform =
            __all(!active || (flushed == 0 && key == first));
        if (uniform) {
            unsigned int sum = active ? runlen : 0u;
            for (int off = 32; off > 0; off >>= 1)
                sum += __shfl_down(sum, off, 64);
            if (lane == 0 && active)
                count_pair_lds(lkeys, lvals, t, ss, sg, sum, status);
        } else if (active) {
            count_pair_lds(lkeys, lvals, t, ss, sg, runlen, status);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LDS_SLOTS; i += blockDim.x)
        if (lkeys[i] != EMPTY) count_run(t, lkeys[i], lvals[i], status);
}

// ---------------------------------------------------------------------------
// apply pass: out = keep(label) ? label : 0, one lookup per run
//   MODE 0 (fragments): keep iff the label's count exceeds `threshold`
//   MODE 1 (except):    keep iff the label is in the table with a set flag
// Zero is written as zero without a lookup.
// ---------------------------------------------------------------------------
template <int MODE>
__device__ inline bool keep_label(const Table& t, unsigned long long key,
                                  long long threshold) {
    long long slot = table_find(t, key);
    if (slot < 0) return false;
    unsigned int val = t.vals[slot];
    return MODE == 0 ? (long long)val > threshold : val != 0u;
}

template <typename T, bool VEC, int MODE>
__global__ void k_apply(const T* __restrict__ in, T* __restrict__ out,
                        long long begin, long long end, Table t,
                        long long threshold) {
    constexpr int E = 16 / (int)sizeof(T);
    constexpr int SEG = SEG_BYTES / (int)sizeof(T);
    const long long n_items = (end - begin + SEG - 1) / SEG;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         item < n_items; item += stride) {
        long long s = begin + item * SEG;
        int len = (int)(end - s < SEG ? end - s : SEG);
        T cur = T(0);       // zero is never kept: the right initial state
        bool keep = false;
        Vec<T, E> o;
        walk_segment<T, VEC>(in + s, len, [&](T v, int j, int e) {
            if (v != cur) {
                cur = v;
                keep = v != T(0)
                       && keep_label<MODE>(t, (unsigned long long)v,
                                           threshold);
            }
            T r = keep ? v : T(0);
            if (VEC) {
                o.e[e] = r;
                if (e == E - 1)
                    *reinterpret_cast<uint4*>(out + s + (j - (E - 1))) = o.q;
            } else {
                out[s + j] = r;
            }
        });
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
inline unsigned int misalign16(const void* p) {
    return (unsigned int)(reinterpret_cast<uintptr_t>(p) & 15);
}

// [0, head) scalar, [head, head + body) vector, [head + body, n) scalar;
// `same_phase` is false when a second stream (the output) does not share
// the input's address modulo 16 — then everything is scalar
template <typename T>
void split_range(const T* in, long long n, bool same_phase, long long* head,
                 long long* body) {
    constexpr int SEG = SEG_BYTES / (int)sizeof(T);
    unsigned int mis = misalign16(in);
    if (!same_phase || mis % sizeof(T) != 0) {
        *head = n;
        *body = 0;
        return;
    }
    long long h = mis ? (16 - mis) / (long long)sizeof(T) : 0;
    if (h > n) h = n;
    *head = h;
    *body = (n - h) / SEG * SEG;
}

int check_volume(const int dims[3], int elem_bytes, const char* who,
                 long long* n) {
    if (dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0) {
        g_err = std::string(who) + ": empty input";
        return -1;
    }
    if (elem_bytes != 4 && elem_bytes != 8) {
        g_err = std::string(who) + ": elem_bytes must be 4 or 8";
        return -1;
    }
    *n = (long long)dims[0] * dims[1] * dims[2];
    if (*n > 0xFFFFFFFFll) {
        g_err = std::string(who) + ": more voxels than a u32 count holds";
        return -1;
    }
    return 0;
}

// The three parts of split_range in stream order: launch(vec, grid, begin,
// end) is called for each non-empty one, `vec` a std::bool_constant that
// picks the kernel. Head and body get one lane per `seg` voxels on at most
// `cap` workgroups, the tail (less than one body segment) one workgroup.
template <typename F>
void launch_parts(long long head, long long body, long long n, int seg,
                  int cap, F&& launch) {
    if (head > 0)
        launch(std::false_type{},
               std::min(grid_for((head + seg - 1) / seg), cap), 0ll, head);
    if (body > 0)
        launch(std::true_type{}, std::min(grid_for(body / seg), cap), head,
               head + body);
    if (head + body < n) launch(std::false_type{}, 1, head + body, n);
}

template <typename T>
void launch_run_starts(cfx_ctx* ctx, const T* in, long long n,
                       unsigned long long* total) {
    long long head, body;
    split_range(in, n, true, &head, &body);
    // one add per wave to a single word: keep the waves few
    launch_parts(head, body, n, SEG_BYTES / (int)sizeof(T), kCountGrid,
                 [&](auto vec, int grid, long long begin, long long end) {
        hipLaunchKernelGGL((k_run_starts<T, decltype(vec)::value>),
                           dim3(grid), dim3(kBlock), 0, ctx->stream, in,
                           begin, end, total);
    });
}

template <typename T>
void launch_count(cfx_ctx* ctx, const T* in, long long n, Table t,
                  unsigned int* status) {
    long long head, body;
    split_range(in, n, true, &head, &body);
    // few, long-lived workgroups: each flushes its LDS table once
    launch_parts(head, body, n, SEG_BYTES / (int)sizeof(T), kCountGrid,
                 [&](auto vec, int grid, long long begin, long long end) {
        hipLaunchKernelGGL((k_count<T, decltype(vec)::value>), dim3(grid),
                           dim3(kBlock), 0, ctx->stream, in, begin, end, t,
                           status);
    });
}

// the first h in [0, 4) at which seg + h and gt + h are both 16-byte aligned
// starts the vector body; a pair of views with no such h is all scalar
template <typename TS, typename TG>
void launch_pair_count(cfx_ctx* ctx, const TS* seg, const TG* gt,
                       long long n, Table ts, Table tg, Table t,
                       unsigned int* status) {
    constexpr int SEG = PairGeom<TS, TG>::SEG;
    long long head = n, body = 0;
    for (long long h = 0; h < 4; ++h)
        if (misalign16(seg + h) == 0 && misalign16(gt + h) == 0) {
            head = std::min(h, n);
            body = (n - head) / SEG * SEG;
            break;
        }
    launch_parts(head, body, n, SEG, kCountGrid,
                 [&](auto vec, int grid, long long begin, long long end) {
        hipLaunchKernelGGL((k_pair_count<TS, TG, decltype(vec)::value>),
                           dim3(grid), dim3(kBlock), 0, ctx->stream, seg, gt,
                           begin, end, ts, tg, t, status);
    });
}

template <typename T, int MODE>
void launch_apply(cfx_ctx* ctx, const T* in, T* out, long long n, Table t,
                  long long threshold) {
    long long head, body;
    split_range(in, n, misalign16(in) == misalign16(out), &head, &body);
    // no cap beyond grid_for's own
    launch_parts(head, body, n, SEG_BYTES / (int)sizeof(T), INT_MAX,
                 [&](auto vec, int grid, long long begin, long long end) {
        hipLaunchKernelGGL((k_apply<T, decltype(vec)::value, MODE>),
                           dim3(grid), dim3(kBlock), 0, ctx->stream, in, out,
                           begin, end, t, threshold);
    });
}

}  // namespace

extern "C" int cfx_label_run_starts(cfx_ctx* ctx, const void* labels,
                                    int elem_bytes, const int dims[3],
                                    long long* n_runs) {
    long long n;
    if (check_volume(dims, elem_bytes, "label_run_starts", &n)) return -1;
    unsigned long long* words;
    if (status_words(ctx, &words)) return -1;
    int rc = cfx_timed(ctx, CFX_K_LABELS, (double)n * elem_bytes, [&] {
        CFX_CHECK(hipMemsetAsync(words, 0, sizeof(unsigned long long),
                                 ctx->stream));
        if (elem_bytes == 4)
            launch_run_starts(ctx, static_cast<const unsigned int*>(labels),
                              n, words);
        else
            launch_run_starts(
                ctx, static_cast<const unsigned long long*>(labels), n,
                words);
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

extern "C" int cfx_label_table_clear(cfx_ctx* ctx, unsigned long long* keys,
                                     unsigned int* vals,
                                     long long capacity) {
    if (check_table(keys, vals, capacity, "label_table_clear")) return -1;
    hipLaunchKernelGGL(k_table_clear, dim3(grid_for(capacity)), dim3(kBlock),
                       0, ctx->stream, keys, vals, capacity);
    CFX_CHECK(hipGetLastError());
    return 0;
}

extern "C" int cfx_label_table_insert(cfx_ctx* ctx,
                                      const unsigned long long* ids,
                                      long long n_ids, unsigned int value,
                                      unsigned long long* keys,
                                      unsigned int* vals,
                                      long long capacity) {
    if (check_table(keys, vals, capacity, "label_table_insert")) return -1;
    if (n_ids < 0 || (n_ids > 0 && !ids)) {
        g_err = "label_table_insert: bad id list";
        return -1;
    }
    if (n_ids == 0) return 0;
    unsigned long long* words;
    if (status_words(ctx, &words)) return -1;
    unsigned int* status = reinterpret_cast<unsigned int*>(words + 1);
    CFX_CHECK(hipMemsetAsync(words + 1, 0, sizeof(unsigned long long),
                             ctx->stream));
    Table t{keys, vals, (unsigned long long)capacity - 1};
    hipLaunchKernelGGL(k_table_insert, dim3(grid_for(n_ids)), dim3(kBlock),
                       0, ctx->stream, t, ids, n_ids, value, status);
    CFX_CHECK(hipGetLastError());
    return read_status(ctx, words + 1, "label_table_insert");
}

extern "C" int cfx_label_count(cfx_ctx* ctx, const void* labels,
                               int elem_bytes, const int dims[3],
                               unsigned long long* keys, unsigned int* vals,
                               long long capacity) {
    long long n;
    if (check_volume(dims, elem_bytes, "label_count", &n)) return -1;
    if (check_table(keys, vals, capacity, "label_count")) return -1;
    unsigned long long* words;
    if (status_words(ctx, &words)) return -1;
    unsigned int* status = reinterpret_cast<unsigned int*>(words + 1);
    Table t{keys, vals, (unsigned long long)capacity - 1};
    int rc = cfx_timed(ctx, CFX_K_LABELS, (double)n * elem_bytes, [&] {
        CFX_CHECK(hipMemsetAsync(words + 1, 0, sizeof(unsigned long long),
                                 ctx->stream));
        if (elem_bytes == 4)
            launch_count(ctx, static_cast<const unsigned int*>(labels), n, t,
                         status);
        else
            launch_count(ctx, static_cast<const unsigned long long*>(labels),
                         n, t, status);
        return 0;
    });
    if (rc) return rc;
    return read_status(ctx, words + 1, "label_count");
}

extern "C" int cfx_label_pair_count(
    cfx_ctx* ctx, const void* seg, int seg_bytes, const int seg_dims[3],
    const unsigned long long* seg_keys, long long seg_capacity,
    const void* gt, int gt_bytes, const int gt_dims[3],
    const unsigned long long* gt_keys, long long gt_capacity,
    unsigned long long* keys, unsigned int* vals, long long capacity) {
    const char* who = "label_pair_count";
    long long n, n_gt;
    if (check_volume(seg_dims, seg_bytes, who, &n)) return -1;
    if (check_volume(gt_dims, gt_bytes, who, &n_gt)) return -1;
    if (seg_dims[0] != gt_dims[0] || seg_dims[1] != gt_dims[1]
        || seg_dims[2] != gt_dims[2]) {
        g_err = std::string(who) + ": the two volumes differ in shape";
        return -1;
    }
    if (!seg || !gt) {
        g_err = std::string(who) + ": null volume";
        return -1;
    }
    if (check_table(keys, vals, capacity, who)) return -1;
    // only the keys of the single tables are read
    if (check_table(seg_keys, seg_keys, seg_capacity, who)) return -1;
    if (check_table(gt_keys, gt_keys, gt_capacity, who)) return -1;
    if (seg_capacity > (1ll << 31) || gt_capacity > (1ll << 31)) {
        g_err = std::string(who)
                + ": a single table above 2^31 slots has no 31-bit slot index";
        return -1;
    }
    unsigned long long* words;
    if (status_words(ctx, &words)) return -1;
    unsigned int* status = reinterpret_cast<unsigned int*>(words + 1);
    Table ts{const_cast<unsigned long long*>(seg_keys), nullptr,
             (unsigned long long)seg_capacity - 1};
    Table tg{const_cast<unsigned long long*>(gt_keys), nullptr,
             (unsigned long long)gt_capacity - 1};
    Table t{keys, vals, (unsigned long long)capacity - 1};
    typedef unsigned int u32;
    typedef unsigned long long u64;
    double bytes = (double)n * (seg_bytes + gt_bytes);
    int rc = cfx_timed(ctx, CFX_K_LABELS, bytes, [&] {
        CFX_CHECK(hipMemsetAsync(words + 1, 0, sizeof(unsigned long long),
                                 ctx->stream));
        if (seg_bytes == 4 && gt_bytes == 4)
            launch_pair_count(ctx, static_cast<const u32*>(seg),
                              static_cast<const u32*>(gt), n, ts, tg, t,
                              status);
        else if (seg_bytes == 4)
            launch_pair_count(ctx, static_cast<const u32*>(seg),
                              static_cast<const u64*>(gt), n, ts, tg, t,
                              status);
        else if (gt_bytes == 4)
            launch_pair_count(ctx, static_cast<const u64*>(seg),
                              static_cast<const u32*>(gt), n, ts, tg, t,
                              status);
        else
            launch_pair_count(ctx, static_cast<const u64*>(seg),
                              static_cast<const u64*>(gt), n, ts, tg, t,
                              status);
        return 0;
    });
    if (rc) return rc;
    return read_status(ctx, words + 1, who);
}

extern "C" int cfx_label_mask(cfx_ctx* ctx, const void* in, void* out,
                              int elem_bytes, const int dims[3],
                              const unsigned long long* keys,
                              const unsigned int* vals, long long capacity,
                              int mode, long long threshold) {
    long long n;
    if (check_volume(dims, elem_bytes, "label_mask", &n)) return -1;
    if (check_table(keys, vals, capacity, "label_mask")) return -1;
    if (mode != 0 && mode != 1) {
        g_err = "label_mask: mode must be 0 (count > threshold) or 1 (flag)";
        return -1;
    }
    if (!in || !out) {
        g_err = "label_mask: null volume";
        return -1;
    }
    Table t{const_cast<unsigned long long*>(keys),
            const_cast<unsigned int*>(vals),
            (unsigned long long)capacity - 1};
    return cfx_timed(ctx, CFX_K_LABELS, 2.0 * (double)n * elem_bytes, [&] {
        if (elem_bytes == 4) {
            auto* i4 = static_cast<const unsigned int*>(in);
            auto* o4 = static_cast<unsigned int*>(out);
            if (mode == 0)
                launch_apply<unsigned int, 0>(ctx, i4, o4, n, t, threshold);
            else
                launch_apply<unsigned int, 1>(ctx, i4, o4, n, t, threshold);
        } else {
            auto* i8 = static_cast<const unsigned long long*>(in);
            auto* o8 = static_cast<unsigned long long*>(out);
            if (mode == 0)
                launch_apply<unsigned long long, 0>(ctx, i8, o8, n, t,
                                                    threshold);
            else
                launch_apply<unsigned long long, 1>(ctx, i8, o8, n, t,
                                                    threshold);
        }
        return 0;
    });
}
