/* mpix — the pull kernels of the native transport and their launch dispatch.
 * HIP only; included by native.cpp alone.  The host plans a batch
 * (pull_plan.h, strided_plan.h); what runs on the device is in here. */
#ifndef MPIX_TRANSPORT_PULL_KERNELS_H
#define MPIX_TRANSPORT_PULL_KERNELS_H

#include <hip/hip_runtime.h>

#include "pull_plan.h"
#include "strided_plan.h"

namespace mpix {

/* Batched pull: one launch copies every partition/message that became
 * ready in the same progress pass (a 64 x 4 MiB partitioned step was
 * latency-bound at ~9 us per serialized launch+event).  The host plans the
 * batch (pull_plan.h): contiguous entries merge into one copy and every copy
 * is cut into tiles of 256 threads x U x 16 B.  Blocks grid-stride over the
 * TOTAL tile count, so they finish together whatever the size mix.  The
 * table travels by value in the kernel argument: no block reads host memory,
 * and there is no argument ring to recycle.  Per full tile a thread issues
 * its U 16-byte loads into independent registers before the first store
 * (U x 4 KiB in flight per block), through global-address-space pointers so
 * the accesses are global_*, not flat_*, and nontemporal by default: the
 * payload is touched once, and keeping it out of the caches is what
 * measured faster than the one-vector-per-thread kernel this replaces
 * (profiles/pull_stream_copy.md).  The partial last tile of a copy
 * and its n % 16 tail bytes take the slow branch.  No spin-wait in here, in
 * either variant (see maybe_switch_prio for why nothing may park on a
 * queue).  k_pull_multi carries no completion signal: its completion is the
 * event recorded behind the launch.  k_pull_multi_done (MPIX_PULL_DONE=word)
 * is the same copy followed by pull_signal_done, which nothing waits for
 * on the device either. */
#define PULL_THREADS 256
typedef unsigned int pull_v4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) pull_v4 *pull_gsrc;
typedef __attribute__((address_space(1))) pull_v4 *pull_gdst;

template <bool NT>
static __device__ __forceinline__ pull_v4 pull_ld(pull_gsrc p)
{
    return NT ? __builtin_nontemporal_load(p) : *p;
}

template <bool NT>
static __device__ __forceinline__ void pull_st(pull_gdst p, pull_v4 v)
{
    if (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

/* Completion word (done_ring.h), device side.  Every block arrives at the
 * slot's counter once its own stores are out of the XCD's L2; the block
 * whose add is the last of the grid zeroes the counter for the slot's next
 * user and publishes the sequence number to the host word.  Nothing waits
 * and nothing spins.
 *  - each wave drains its own stores (vmcnt counts stores on gfx9), then the
 *    block barrier: thread 0 signals for all waves of the block;
 *  - agent-scope release before the add: nontemporal stores stay in the L2
 *    of the XCD, and the host word must not overtake them.  The wait behind
 *    the fence is written as asm so that it cannot be dropped;
 *  - the last arriver's add returned gridDim.x - 1, so every other block's
 *    release happened before it; its system-scope release store orders the
 *    counter reset and the word behind all of that. */
struct PullDone {
    uint32_t *counter; /* device memory, 0 between uses */
    uint64_t *word;    /* pinned host memory */
    uint64_t seq;
};

static __device__ __forceinline__ void pull_signal_done(const PullDone &d)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t before = __hip_atomic_fetch_add(
            d.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before == gridDim.x - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(d.counter, 0u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(d.word, d.seq, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <int U, bool NT>
static __device__ __forceinline__ void pull_multi_body(const PullTable &t)
{
    constexpr uint64_t TILE = (uint64_t)PULL_THREADS * U * 16;
    const uint64_t total = t.tile_end[t.ncopies - 1];
    /* copy c holds global tiles [first, end); the table sits in the kernel
     * argument and is re-read only when a block crosses into another copy */
    uint32_t c = 0;
    uint64_t first = 0, end = t.tile_end[0];
    PullCopy cur = t.copy[0];
    for (uint64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        if (tile >= end) {
            do {
                first = end;
                end = t.tile_end[++c];
            } while (tile >= end);
            cur = t.copy[c];
        }
        const uint64_t off = (tile - first) * TILE;
        const uint64_t left = cur.bytes - off;
        pull_gsrc s = (pull_gsrc)(cur.src + off);
        pull_gdst d = (pull_gdst)(cur.dst + off);
        if (left >= TILE) {
            pull_v4 r[U];
#pragma unroll
            for (int k = 0; k < U; k++)
                r[k] = pull_ld<NT>(s + threadIdx.x + k * PULL_THREADS);
#pragma unroll
            for (int k = 0; k < U; k++)
                pull_st<NT>(d + threadIdx.x + k * PULL_THREADS, r[k]);
        } else {
            const uint32_t nv = (uint32_t)(left / 16);
            for (uint32_t v = threadIdx.x; v < nv; v += PULL_THREADS)
                d[v] = s[v];
            if (threadIdx.x < (uint32_t)(left & 15)) {
                const uint64_t b = (uint64_t)nv * 16 + threadIdx.x;
                ((__attribute__((address_space(1))) char *)d)[b] =
                    ((const __attribute__((address_space(1))) char *)s)[b];
            }
        }
    }
}

template <int U, bool NT>
__global__ __launch_bounds__(PULL_THREADS) void k_pull_multi(const PullTable t)
{
    pull_multi_body<U, NT>(t);
}

template <int U, bool NT>
__global__ __launch_bounds__(PULL_THREADS) void k_pull_multi_done(
    const PullTable t, const PullDone d)
{
    pull_multi_body<U, NT>(t);
    pull_signal_done(d);
}

/* Strided pull: the same launch shape for messages that are strided on
 * either side (strided_plan.h).  Work is indexed in message space in units
 * of the entry's granule, so a strided source lands straight in a strided
 * destination: no pack, no unpack, no staging buffer.  Consecutive lanes take
 * consecutive units, so lanes inside one run coalesce; a wave access made of
 * 128-byte segments streams at full rate, 64 lanes in 64 different rows do
 * not (4-byte runs are served correctly, not fast).  Per side a unit index
 * decomposes into (plane, run, offset) by two divisions whose reciprocals
 * the host prepared (a multiply and a shift each).  Granule 16 is the
 * vector path: one global_load_dwordx4 / global_store_dwordx4 per unit,
 * nontemporal, the U loads of a tile issued before its first store.  The
 * element path is the same walk with 8/4/2/1-byte accesses, 16/granule
 * rounds of it per tile.  Every unit is bounds-checked against the entry
 * (the partial last tile takes the same code).  WIDE is the variant with
 * 64-bit division, launched only when an entry has 2^31 units or more: it
 * is many times the code, so the common kernel does not carry it.  PARTS is
 * the variant for runs of partitions (an entry of k partitions, part strides
 * apart on each side): one more division per unit splits off the partition
 * number, shared by both sides since partitions have one size.  It is right
 * for every entry (one without a partition level has a quotient of 0), and
 * launched only when a batch holds a run entry, so plain strided messages
 * do not pay the third division. */
template <typename T, int ROUNDS, bool WIDE, bool PARTS>
static __device__ __forceinline__ void strided_tile(const StridedEntry &e,
                                                    uint64_t unit0)
{
    typedef const __attribute__((address_space(1))) T *gsrc;
    typedef __attribute__((address_space(1))) T *gdst;
    constexpr int U = MPIX_STRIDED_UNROLL;
    constexpr bool wide = WIDE;
    constexpr bool parts = PARTS;
#pragma unroll 1
    for (int j = 0; j < ROUNDS; j++) {
        T r[U];
        int64_t doff[U];
        bool ok[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            const uint64_t u = unit0 +
                (uint64_t)(j * U + k) * PULL_THREADS + threadIdx.x;
            ok[k] = u < e.units;
            if (ok[k]) {
                int64_t soff;
                strided_entry_offsets(e, u, wide, parts, &soff, &doff[k]);
                r[k] = __builtin_nontemporal_load((gsrc)(e.src + soff));
            }
        }
#pragma unroll
        for (int k = 0; k < U; k++)
            if (ok[k])
                __builtin_nontemporal_store(r[k], (gdst)(e.dst + doff[k]));
    }
}

template <bool WIDE, bool PARTS>
static __device__ __forceinline__ void pull_strided_body(const StridedTable &t)
{
    const uint64_t total = t.tile_end[t.n - 1];
    uint32_t c = 0;
    uint64_t first = 0, end = t.tile_end[0];
    StridedEntry cur = t.e[0];
    for (uint64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        if (tile >= end) {
            do {
                first = end;
                end = t.tile_end[++c];
            } while (tile >= end);
            cur = t.e[c];
        }
        /* units of this tile start at (tile bytes) >> glog */
        const uint64_t unit0 = ((tile - first) * MPIX_STRIDED_TILE) >> cur.glog;
        switch (cur.glog) {
        case 4: strided_tile<pull_v4, 1, WIDE, PARTS>(cur, unit0); break;
        case 3: strided_tile<uint64_t, 2, WIDE, PARTS>(cur, unit0); break;
        case 2: strided_tile<uint32_t, 4, WIDE, PARTS>(cur, unit0); break;
        case 1: strided_tile<uint16_t, 8, WIDE, PARTS>(cur, unit0); break;
        default: strided_tile<uint8_t, 16, WIDE, PARTS>(cur, unit0); break;
        }
    }
}

template <bool WIDE, bool PARTS>
__global__ __launch_bounds__(PULL_THREADS) void k_pull_strided(
    const StridedTable t)
{
    pull_strided_body<WIDE, PARTS>(t);
}

/* MPIX_PULL_DONE=word: see pull_signal_done */
template <bool WIDE, bool PARTS>
__global__ __launch_bounds__(PULL_THREADS) void k_pull_strided_done(
    const StridedTable t, const PullDone d)
{
    pull_strided_body<WIDE, PARTS>(t);
    pull_signal_done(d);
}

/* Launch dispatch.  Each variant comes as a pair: the kernel that signals
 * the completion word, launched when `done` is given, and the plain one
 * whose completion is an event.  unroll is 1, 8 or (anything else) 4. */
struct PullKernel { /* of one unroll; [0] nontemporal, [1] cached accesses */
    void (*by_word[2])(const PullTable, const PullDone);
    void (*by_event[2])(const PullTable);
};
struct StridedKernel {
    void (*by_word)(const StridedTable, const PullDone);
    void (*by_event)(const StridedTable);
};

static inline void launch_pull(const PullTable &t, int unroll, bool nt,
                               unsigned blocks, hipStream_t cs,
                               const PullDone *done)
{
    static const PullKernel variants[3] = {
        {{k_pull_multi_done<1, true>, k_pull_multi_done<1, false>},
         {k_pull_multi<1, true>, k_pull_multi<1, false>}},
        {{k_pull_multi_done<8, true>, k_pull_multi_done<8, false>},
         {k_pull_multi<8, true>, k_pull_multi<8, false>}},
        {{k_pull_multi_done<4, true>, k_pull_multi_done<4, false>},
         {k_pull_multi<4, true>, k_pull_multi<4, false>}}};
    const PullKernel &k = variants[unroll == 1 ? 0 : unroll == 8 ? 1 : 2];
    if (done != nullptr)
        hipLaunchKernelGGL(k.by_word[nt ? 0 : 1], dim3(blocks),
                           dim3(PULL_THREADS), 0, cs, t, *done);
    else
        hipLaunchKernelGGL(k.by_event[nt ? 0 : 1], dim3(blocks),
                           dim3(PULL_THREADS), 0, cs, t);
}

static inline void launch_strided(const StridedTable &t, bool wide, bool parts,
                                  unsigned blocks, hipStream_t cs,
                                  const PullDone *done)
{
    static const StridedKernel variants[2][2] = {
        {{k_pull_strided_done<true, true>, k_pull_strided<true, true>},
         {k_pull_strided_done<true, false>, k_pull_strided<true, false>}},
        {{k_pull_strided_done<false, true>, k_pull_strided<false, true>},
         {k_pull_strided_done<false, false>, k_pull_strided<false, false>}}};
    const StridedKernel &k = variants[wide ? 0 : 1][parts ? 0 : 1];
    if (done != nullptr)
        hipLaunchKernelGGL(k.by_word, dim3(blocks), dim3(PULL_THREADS), 0, cs,
                           t, *done);
    else
        hipLaunchKernelGGL(k.by_event, dim3(blocks), dim3(PULL_THREADS), 0, cs,
                           t);
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_PULL_KERNELS_H */
