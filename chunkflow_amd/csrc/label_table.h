// The open-addressing table in caller-owned HBM shared by labels.hip (label
// counts, contingency pairs) and watershed.hip (region-graph edges): the
// probing rules, the status flags and their host-side read-back. The layout
// and the contract are described at the top of labels.hip.
#ifndef CFX_LABEL_TABLE_H
#define CFX_LABEL_TABLE_H

#include <hip/hip_runtime.h>

#include <string>

#include "cfx_internal.h"

namespace label_table {

constexpr unsigned long long EMPTY = ~0ull;

enum : unsigned int { ST_FULL = 1u, ST_RESERVED = 2u, ST_MISSING = 4u };

// murmur3's 64-bit finalizer: every input bit reaches every output bit
__device__ inline unsigned long long mix64(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

struct Table {
    unsigned long long* keys;
    unsigned int* vals;
    unsigned long long mask;  // capacity - 1
};

// slot of `key`, claiming an empty one if needed; -1 (and ST_FULL raised)
// after `capacity` probes without success. Keys are read and claimed with
// agent-scope atomics: the claiming CAS of another CU must be seen.
__device__ inline long long table_insert(const Table& t,
                                         unsigned long long key,
                                         unsigned int* status) {
    unsigned long long slot = mix64(key) & t.mask;
    for (unsigned long long probe = 0; probe <= t.mask; ++probe) {
        unsigned long long k = __hip_atomic_load(
            &t.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == EMPTY) k = atomicCAS(&t.keys[slot], EMPTY, key);
        if (k == EMPTY || k == key) return (long long)slot;
        slot = (slot + 1) & t.mask;
    }
    atomicOr(status, ST_FULL);
    return -1;
}

// slot of `key` in a table no kernel is writing, or -1 if absent
__device__ inline long long table_find(const Table& t,
                                       unsigned long long key) {
    unsigned long long slot = mix64(key) & t.mask;
    for (unsigned long long probe = 0; probe <= t.mask; ++probe) {
        unsigned long long k = t.keys[slot];
        if (k == key) return (long long)slot;
        if (k == EMPTY) return -1;
        slot = (slot + 1) & t.mask;
    }
    return -1;
}

inline int check_table(const void* keys, const void* vals, long long capacity,
                       const char* who) {
    if (!keys || !vals) {
        g_err = std::string(who) + ": null table";
        return -1;
    }
    if (capacity < 1 || (capacity & (capacity - 1)) != 0) {
        g_err = std::string(who) + ": table capacity must be a power of two";
        return -1;
    }
    return 0;
}

// two u64 words of context scratch: [0] run-start total, [1] status flags
inline int status_words(cfx_ctx* ctx, unsigned long long** words) {
    if (!ctx->label_words)
        CFX_CHECK(hipMalloc(&ctx->label_words,
                            2 * sizeof(unsigned long long)));
    *words = ctx->label_words;
    return 0;
}

inline int read_status(cfx_ctx* ctx, unsigned long long* word,
                       const char* who) {
    unsigned long long st = 0;
    CFX_CHECK(hipMemcpyAsync(&st, word, sizeof(st), hipMemcpyDeviceToHost,
                             ctx->stream));
    CFX_CHECK(hipStreamSynchronize(ctx->stream));
    if (st & ST_RESERVED) {
        g_err = std::string(who)
                + ": the label 2^64-1 is reserved (empty-slot key)";
        return -1;
    }
    if (st & ST_MISSING) {
        g_err = std::string(who)
                + ": a label is missing from its table (count each volume "
                  "into its table first)";
        return -1;
    }
    if (st & ST_FULL) {
        g_err = std::string(who)
                + ": label table full (more distinct labels than capacity)";
        return -1;
    }
    return 0;
}

}  // namespace label_table

#endif  // CFX_LABEL_TABLE_H
