/* mpix — the pull kernels of the native transport and their launch dispatch.
 * HIP only; included by native.cpp, and by
 * tests/native/pull_kernels_check.hip, which launches every variant in here
 * directly (tests/native/reduce_kernels_check.hip for the reduce kernels,
 * tests/native/strided_reduce_kernels_check.hip for the strided reduce
 * kernels).  The host plans a batch (pull_plan.h, strided_plan.h,
 * reduce_plan.h, strided_reduce_plan.h); what runs on the device is in
 * here. */
#ifndef MPIX_TRANSPORT_PULL_KERNELS_H
#define MPIX_TRANSPORT_PULL_KERNELS_H

#include <hip/hip_runtime.h>

#include "pull_plan.h"
#include "reduce_plan.h"
#include "strided_plan.h"
#include "strided_reduce_plan.h"

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
 * event recorded behind the launch, or k_pull_tail behind it on the stream
 * (MPIX_PULL_DONE=tail).  k_pull_multi_done (MPIX_PULL_DONE=word) is the
 * same copy with every payload store written through, followed by
 * pull_signal_done, which nothing waits for on the device either. */
#define PULL_THREADS 256
typedef unsigned int pull_v4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) pull_v4 *pull_gsrc;
typedef __attribute__((address_space(1))) pull_v4 *pull_gdst;

/* How a kernel stores the payload (its loads are nontemporal unless the
 * policy is PULL_ST_PLAIN):
 *   PULL_ST_NT     nontemporal stores: the event and tail kernels.  The lines
 *                  stay dirty in the L2 of the block's XCD until the end of
 *                  the kernel writes them back.
 *   PULL_ST_PLAIN  cached loads and stores (MPIX_PULL_NT=0).
 *   PULL_ST_WT     write-through stores (sc1): the bytes are in memory once
 *                  the storing wave's vmcnt has drained, so the completion
 *                  word needs no release fence (pull_signal_done).  It
 *                  covers EVERY payload store of the kernel: the partial
 *                  last tile and the n % 16 tail bytes too.  (sc1 nt was
 *                  measured and lost: profiles/pull_done_modes.md.)
 */
enum PullStore { PULL_ST_NT, PULL_ST_PLAIN, PULL_ST_WT };

static constexpr bool pull_write_through(PullStore S)
{
    return S == PULL_ST_WT;
}

template <PullStore S>
static __device__ __forceinline__ pull_v4 pull_ld(pull_gsrc p)
{
    return S != PULL_ST_PLAIN ? __builtin_nontemporal_load(p) : *p;
}

/* The 16-byte store of a full tile.  The write-through form is written
 * as asm: the compiler has no 16-byte atomic store to lower to it.  The
 * s_nop covers the wait states between a store of more than 64 bits and an
 * overwrite of its data registers, which the compiler does not count for
 * asm. */
template <PullStore S>
static __device__ __forceinline__ void pull_st(pull_gdst p, pull_v4 v)
{
    if (S == PULL_ST_WT)
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1"
                     :: "v"(p), "v"(v) : "memory");
    else if (S == PULL_ST_NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

/* Stores of the slow branches (partial tiles, tail bytes, the element path
 * of the strided kernel): T is 16, 8, 4, 2 or 1 bytes.  Write-through: the
 * 16-byte form above, and a relaxed agent-scope atomic store below that,
 * which is the same store with sc1.  Otherwise NT says which. */
template <PullStore S, typename T, bool NT>
static __device__ __forceinline__ void pull_st_any(
    __attribute__((address_space(1))) T *p, T v)
{
    if constexpr (pull_write_through(S)) {
        if constexpr (sizeof(T) == 16)
            pull_st<S>((pull_gdst)p, v);
        else
            __hip_atomic_store(p, v, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    } else {
        if constexpr (NT)
            __builtin_nontemporal_store(v, p);
        else
            *p = v;
    }
}

/* Completion word (done_ring.h), device side, for kernels whose payload
 * stores are all write-through.  Every block arrives at the slot's counter
 * once its own stores are in memory; the block whose arrival is the last of
 * the grid publishes the sequence number to the host word.  Nothing waits
 * and nothing spins, and there is no fence: a release at agent scope is a
 * write-back of the XCD's whole L2 (buffer_wbl2), and 1024 of them at the
 * end of a 256 MiB copy cost 50 us (profiles/batch_handoffs.md section 5).
 *  - each wave drains its own stores (vmcnt counts stores on gfx9; written
 *    as asm so that it cannot be dropped or moved), then the block barrier:
 *    thread 0 signals for all waves of the block;
 *  - the arrival is an atomic increment that wraps at gridDim.x - 1
 *    (relaxed, agent scope): the last arriver's own atomic leaves the
 *    counter at 0 for the slot's next user, so there is no reset store that
 *    the word could overtake;
 *  - why that is enough: every payload byte was written through and its
 *    store acknowledged before its block's increment was issued, and the
 *    increment that returned gridDim.x - 1 came after all the others.  The
 *    word is a relaxed system-scope store; a release there would bring one
 *    buffer_wbl2 back. */
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
        const uint32_t before = atomicInc(d.counter, gridDim.x - 1);
        if (before == gridDim.x - 1)
            __hip_atomic_store(d.word, d.seq, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

/* MPIX_PULL_DONE=tail: one thread, launched on the copy's stream straight
 * behind the copy kernel or the hipMemcpyAsync.  Ordering and visibility are
 * those of two kernels on one stream. */
__global__ void k_pull_tail(uint64_t *word, uint64_t seq)
{
    __hip_atomic_store(word, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int U, PullStore S>
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
                r[k] = pull_ld<S>(s + threadIdx.x + k * PULL_THREADS);
#pragma unroll
            for (int k = 0; k < U; k++)
                pull_st<S>(d + threadIdx.x + k * PULL_THREADS, r[k]);
        } else {
            typedef __attribute__((address_space(1))) char *gchar;
            const uint32_t nv = (uint32_t)(left / 16);
            for (uint32_t v = threadIdx.x; v < nv; v += PULL_THREADS) {
                if constexpr (pull_write_through(S))
                    pull_st<S>(d + v, s[v]);
                else
                    d[v] = s[v];
            }
            if (threadIdx.x < (uint32_t)(left & 15)) {
                const uint64_t b = (uint64_t)nv * 16 + threadIdx.x;
                pull_st_any<S, char, false>(
                    (gchar)d + b,
                    ((const __attribute__((address_space(1))) char *)s)[b]);
            }
        }
    }
}

template <int U, PullStore S>
__global__ __launch_bounds__(PULL_THREADS) void k_pull_multi(const PullTable t)
{
    pull_multi_body<U, S>(t);
}

template <int U, PullStore S>
__global__ __launch_bounds__(PULL_THREADS) void k_pull_multi_done(
    const PullTable t, const PullDone d)
{
    static_assert(pull_write_through(S), "the word needs write-through stores");
    pull_multi_body<U, S>(t);
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
 * do not pay the third division.  S is the store policy, as in the
 * contiguous kernel: nontemporal, or write-through in the kernels that
 * signal the completion word. */
template <typename T, int ROUNDS, bool WIDE, bool PARTS, PullStore S>
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
                pull_st_any<S, T, true>((gdst)(e.dst + doff[k]), r[k]);
    }
}

template <bool WIDE, bool PARTS, PullStore S>
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
        case 4: strided_tile<pull_v4, 1, WIDE, PARTS, S>(cur, unit0); break;
        case 3: strided_tile<uint64_t, 2, WIDE, PARTS, S>(cur, unit0); break;
        case 2: strided_tile<uint32_t, 4, WIDE, PARTS, S>(cur, unit0); break;
        case 1: strided_tile<uint16_t, 8, WIDE, PARTS, S>(cur, unit0); break;
        default: strided_tile<uint8_t, 16, WIDE, PARTS, S>(cur, unit0); break;
        }
    }
}

template <bool WIDE, bool PARTS>
__global__ __launch_bounds__(PULL_THREADS) void k_pull_strided(
    const StridedTable t)
{
    pull_strided_body<WIDE, PARTS, PULL_ST_NT>(t);
}

/* MPIX_PULL_DONE=word: write-through stores, then pull_signal_done */
template <bool WIDE, bool PARTS, PullStore S>
__global__ __launch_bounds__(PULL_THREADS) void k_pull_strided_done(
    const StridedTable t, const PullDone d)
{
    static_assert(pull_write_through(S), "the word needs write-through stores");
    pull_strided_body<WIDE, PARTS, S>(t);
    pull_signal_done(d);
}

/* Reducing pull: dst[i] = dst[i] op src[i], the combine of reduce.h, inside
 * the pull (MPIX_Irecv_reduce_enqueue, MPIX_Precv_init_reduce).  The launch
 * shape is k_pull_multi's: the table (reduce_plan.h) travels by value, every
 * entry is cut into tiles of 256 threads x 4 x 16 B and blocks grid-stride
 * over the total tile count.  Per payload byte it moves 3 bytes (remote
 * load, local load, store) where a pull into a staging buffer and an add
 * kernel behind it move 5.  Per full tile a thread issues its 4 remote
 * loads (nontemporal: the message is touched once) and its 4 local loads
 * before the first store.  Element type and op are per entry and switched
 * on once per tile, so one kernel serves all 18 combinations and a batch
 * may mix them.
 *  - vector path: both addresses of the entry 16-byte aligned; the entry's
 *    bytes % 16 tail takes element-sized accesses;
 *  - element path: the same walk with element-sized accesses, 16 / size
 *    rounds per tile, for an entry with a side that is element-aligned only.
 * Elements are loaded and stored as their bit patterns (uint16/32/64_t).
 *
 * Why the load of dst sees the user's data: the per-XCD L2s are not coherent
 * with each other, so a line the user wrote on one XCD could be stale in the
 * L2 of the XCD this block runs on.  But the user's writes finished in an
 * EARLIER kernel (or copy) on the stream that triggered the receive, or
 * before MPIX_Start: the end of that kernel wrote its dirty lines back to
 * memory, and the start of this kernel invalidates what the L2s hold of
 * them, so a plain load here is served from memory or from a line loaded
 * after that.  The same argument covers two reducing launches behind each
 * other on the copy stream (overlapping destinations, reduce_plan.h): the
 * first one's end writes back (its write-through stores are in memory even
 * sooner), the second one's start invalidates.  Inside one launch no
 * element is touched by two blocks: plan_reduce ends the batch first.
 *
 * k_pull_reduce stores nontemporal and signals nothing (event and tail
 * modes).  k_pull_reduce_done stores EVERY payload byte write-through (sc1):
 * the full tiles, the partial tile, the tail elements and the whole element
 * path, then pull_signal_done, with no fence, like the other _done kernels. */
template <int BYTES> struct RedBits;
template <> struct RedBits<2> { typedef uint16_t U; };
template <> struct RedBits<4> { typedef uint32_t U; };
template <> struct RedBits<8> { typedef uint64_t U; };

template <int TYPE>
using RedB = typename RedBits<sizeof(typename Red<TYPE>::T)>::U;

template <int TYPE, int OP>
static __device__ __forceinline__ RedB<TYPE> reduce_bits(RedB<TYPE> a,
                                                         RedB<TYPE> b)
{
    typedef typename Red<TYPE>::T T;
    T ta, tb;
    __builtin_memcpy(&ta, &a, sizeof(T));
    __builtin_memcpy(&tb, &b, sizeof(T));
    ta = Red<TYPE>::combine(OP, ta, tb);
    __builtin_memcpy(&a, &ta, sizeof(T));
    return a;
}

template <int TYPE, int OP>
static __device__ __forceinline__ pull_v4 reduce_v4(pull_v4 a, pull_v4 b)
{
    typedef typename Red<TYPE>::T T;
    constexpr int PER = 16 / (int)sizeof(T);
    T ta[PER], tb[PER];
    __builtin_memcpy(ta, &a, 16);
    __builtin_memcpy(tb, &b, 16);
#pragma unroll
    for (int i = 0; i < PER; i++) ta[i] = Red<TYPE>::combine(OP, ta[i], tb[i]);
    __builtin_memcpy(&a, ta, 16);
    return a;
}

/* the tile of entry `cur` that starts `off` bytes into it */
template <int TYPE, int OP, PullStore S>
static __device__ __forceinline__ void reduce_tile(const ReduceEntry &cur,
                                                   uint64_t off)
{
    typedef RedB<TYPE> B;
    typedef const __attribute__((address_space(1))) B *gbsrc;
    typedef __attribute__((address_space(1))) B *gbdst;
    constexpr int U = MPIX_REDUCE_UNROLL;
    constexpr uint64_t TILE = MPIX_REDUCE_TILE;
    static_assert(TILE == (uint64_t)PULL_THREADS * U * 16, "tile of the plan");
    const uint64_t left = cur.bytes - off;
    if (((((uintptr_t)cur.src) | ((uintptr_t)cur.dst)) & 15) == 0) {
        pull_gsrc s = (pull_gsrc)(cur.src + off);
        pull_gdst d = (pull_gdst)(cur.dst + off);
        if (left >= TILE) {
            pull_v4 a[U], b[U];
#pragma unroll
            for (int k = 0; k < U; k++)
                b[k] = __builtin_nontemporal_load(s + threadIdx.x +
                                                  k * PULL_THREADS);
#pragma unroll
            for (int k = 0; k < U; k++)
                a[k] = d[threadIdx.x + k * PULL_THREADS];
#pragma unroll
            for (int k = 0; k < U; k++)
                pull_st<S>(d + threadIdx.x + k * PULL_THREADS,
                           reduce_v4<TYPE, OP>(a[k], b[k]));
            return;
        }
        const uint32_t nv = (uint32_t)(left / 16);
        for (uint32_t v = threadIdx.x; v < nv; v += PULL_THREADS)
            pull_st<S>(d + v, reduce_v4<TYPE, OP>(
                                  d[v], __builtin_nontemporal_load(s + v)));
        /* bytes % 16 of the entry: whole elements, fewer than 16 / size */
        if (threadIdx.x < (uint32_t)(left & 15) / sizeof(B)) {
            gbsrc ts = (gbsrc)(s + nv) + threadIdx.x;
            gbdst td = (gbdst)(d + nv) + threadIdx.x;
            pull_st_any<S, B, true>(
                td, reduce_bits<TYPE, OP>(*td,
                                          __builtin_nontemporal_load(ts)));
        }
        return;
    }
    /* element path: the elements of this tile, in rounds of U x 256 */
    gbsrc s = (gbsrc)(cur.src + off);
    gbdst d = (gbdst)(cur.dst + off);
    const uint32_t cnt =
        (uint32_t)((left < TILE ? left : TILE) / sizeof(B));
#pragma unroll 1
    for (uint32_t j = 0; j < 16 / sizeof(B); j++) {
        B a[U], b[U];
        bool ok[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            const uint32_t i = (j * U + k) * PULL_THREADS + threadIdx.x;
            ok[k] = i < cnt;
            if (ok[k]) b[k] = __builtin_nontemporal_load(s + i);
        }
#pragma unroll
        for (int k = 0; k < U; k++) {
            const uint32_t i = (j * U + k) * PULL_THREADS + threadIdx.x;
            if (ok[k]) a[k] = d[i];
        }
#pragma unroll
        for (int k = 0; k < U; k++) {
            const uint32_t i = (j * U + k) * PULL_THREADS + threadIdx.x;
            if (ok[k])
                pull_st_any<S, B, true>(d + i,
                                        reduce_bits<TYPE, OP>(a[k], b[k]));
        }
    }
}

template <PullStore S>
static __device__ __forceinline__ void pull_reduce_body(const ReduceTable &t)
{
    const uint64_t total = t.tile_end[t.n - 1];
    uint32_t c = 0;
    uint64_t first = 0, end = t.tile_end[0];
    ReduceEntry cur = t.e[0];
    for (uint64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        if (tile >= end) {
            do {
                first = end;
                end = t.tile_end[++c];
            } while (tile >= end);
            cur = t.e[c];
        }
        const uint64_t off = (tile - first) * MPIX_REDUCE_TILE;
#define REDUCE_CASE(TY)                                                      \
    case TY * RED_NOPS + RED_SUM: reduce_tile<TY, RED_SUM, S>(cur, off); break; \
    case TY * RED_NOPS + RED_MAX: reduce_tile<TY, RED_MAX, S>(cur, off); break; \
    case TY * RED_NOPS + RED_MIN: reduce_tile<TY, RED_MIN, S>(cur, off); break;
        switch (cur.type * RED_NOPS + cur.op) {
            REDUCE_CASE(RED_F32)
            REDUCE_CASE(RED_F64)
            REDUCE_CASE(RED_BF16)
            REDUCE_CASE(RED_F16)
            REDUCE_CASE(RED_I32)
            REDUCE_CASE(RED_I64)
        default: break; /* the host validated type and op */
        }
#undef REDUCE_CASE
    }
}

__global__ __launch_bounds__(PULL_THREADS) void k_pull_reduce(
    const ReduceTable t)
{
    pull_reduce_body<PULL_ST_NT>(t);
}

/* MPIX_PULL_DONE=word: write-through stores, then pull_signal_done */
__global__ __launch_bounds__(PULL_THREADS) void k_pull_reduce_done(
    const ReduceTable t, const PullDone d)
{
    pull_reduce_body<PULL_ST_WT>(t);
    pull_signal_done(d);
}

/* Strided reducing pull: the walk of k_pull_strided with the combine of
 * k_pull_reduce (MPIX_Irecv_reduce_strided_enqueue,
 * MPIX_Precv_init_reduce_strided).  Units are indexed in message space and
 * decomposed per side by strided_entry_offsets, always with the partition
 * level (an entry without one has a quotient of 0;
 * profiles/strided_partitions.md measured no cost for it), every unit
 * bounds-checked, blocks grid-striding over tile_end[].  Two unit sizes
 * (strided_reduce_plan.h): 16 bytes, combined by reduce_v4, or one element,
 * combined by reduce_bits, 16 / size rounds of it per tile.  Per round a
 * thread issues its U nontemporal loads of the (remote) source, then its U
 * plain loads of the destination, then combines in registers, then stores.
 * The plain load of dst sees the user's data by the argument above
 * k_pull_reduce; no element is touched by two blocks of one launch because
 * plan_strided_reduce ends the batch before overlapping extents.  Type and
 * op are per entry and switched on once per tile.  WIDE as in
 * k_pull_strided.  k_pull_strided_reduce stores nontemporal and signals
 * nothing; k_pull_strided_reduce_done stores every byte write-through, then
 * pull_signal_done, with no fence. */
template <int TYPE, bool VEC> struct StridedRedUnit { typedef RedB<TYPE> U; };
template <int TYPE> struct StridedRedUnit<TYPE, true> { typedef pull_v4 U; };

template <int TYPE, int OP, bool VEC, bool WIDE, PullStore S>
static __device__ __forceinline__ void strided_reduce_tile(
    const StridedEntry &e, uint64_t unit0)
{
    typedef typename StridedRedUnit<TYPE, VEC>::U T;
    typedef const __attribute__((address_space(1))) T *gsrc;
    typedef __attribute__((address_space(1))) T *gdst;
    constexpr int U = MPIX_STRIDED_UNROLL;
    constexpr int ROUNDS = 16 / (int)sizeof(T);
    constexpr bool wide = WIDE;
#pragma unroll 1
    for (int j = 0; j < ROUNDS; j++) {
        T a[U], b[U];
        int64_t doff[U];
        bool ok[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            const uint64_t u = unit0 +
                (uint64_t)(j * U + k) * PULL_THREADS + threadIdx.x;
            ok[k] = u < e.units;
            if (ok[k]) {
                int64_t soff;
                strided_entry_offsets(e, u, wide, true, &soff, &doff[k]);
                b[k] = __builtin_nontemporal_load((gsrc)(e.src + soff));
            }
        }
#pragma unroll
        for (int k = 0; k < U; k++)
            if (ok[k]) a[k] = *(gdst)(e.dst + doff[k]);
#pragma unroll
        for (int k = 0; k < U; k++)
            if (ok[k]) {
                if constexpr (VEC)
                    a[k] = reduce_v4<TYPE, OP>(a[k], b[k]);
                else
                    a[k] = reduce_bits<TYPE, OP>(a[k], b[k]);
                pull_st_any<S, T, true>((gdst)(e.dst + doff[k]), a[k]);
            }
    }
}

template <bool WIDE, PullStore S>
static __device__ __forceinline__ void pull_strided_reduce_body(
    const StridedReduceTable &t)
{
    const uint64_t total = t.tile_end[t.n - 1];
    uint32_t c = 0;
    uint64_t first = 0, end = t.tile_end[0];
    StridedEntry cur = t.e[0];
    uint32_t sel = t.type[0] * RED_NOPS + t.op[0];
    for (uint64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        if (tile >= end) {
            do {
                first = end;
                end = t.tile_end[++c];
            } while (tile >= end);
            cur = t.e[c];
            sel = t.type[c] * RED_NOPS + t.op[c];
        }
        const uint64_t unit0 = ((tile - first) * MPIX_STRIDED_TILE) >> cur.glog;
        const bool vec = cur.glog == 4;
#define STRIDED_REDUCE_OP(TY, OP)                                        \
    case TY * RED_NOPS + OP:                                             \
        if (vec)                                                         \
            strided_reduce_tile<TY, OP, true, WIDE, S>(cur, unit0);      \
        else                                                             \
            strided_reduce_tile<TY, OP, false, WIDE, S>(cur, unit0);     \
        break;
#define STRIDED_REDUCE_CASE(TY)    \
    STRIDED_REDUCE_OP(TY, RED_SUM) \
    STRIDED_REDUCE_OP(TY, RED_MAX) \
    STRIDED_REDUCE_OP(TY, RED_MIN)
        switch (sel) {
            STRIDED_REDUCE_CASE(RED_F32)
            STRIDED_REDUCE_CASE(RED_F64)
            STRIDED_REDUCE_CASE(RED_BF16)
            STRIDED_REDUCE_CASE(RED_F16)
            STRIDED_REDUCE_CASE(RED_I32)
            STRIDED_REDUCE_CASE(RED_I64)
        default: break; /* the host validated type and op */
        }
#undef STRIDED_REDUCE_CASE
#undef STRIDED_REDUCE_OP
    }
}

template <bool WIDE>
__global__ __launch_bounds__(PULL_THREADS) void k_pull_strided_reduce(
    const StridedReduceTable t)
{
    pull_strided_reduce_body<WIDE, PULL_ST_NT>(t);
}

/* MPIX_PULL_DONE=word: write-through stores, then pull_signal_done */
template <bool WIDE>
__global__ __launch_bounds__(PULL_THREADS) void k_pull_strided_reduce_done(
    const StridedReduceTable t, const PullDone d)
{
    pull_strided_reduce_body<WIDE, PULL_ST_WT>(t);
    pull_signal_done(d);
}

/* Launch dispatch.  Each variant comes as a pair: the kernel that stores
 * write-through and signals the completion word, launched when `done` is
 * given, and the plain one whose completion is an event or a tail kernel
 * (`nt`: its loads and stores nontemporal, or cached).  unroll is 1, 8 or
 * (anything else) 4. */
struct PullKernel { /* of one unroll */
    void (*by_word)(const PullTable, const PullDone);
    void (*by_event[2])(const PullTable); /* [0] nontemporal, [1] cached */
};
struct StridedKernel {
    void (*by_word)(const StridedTable, const PullDone);
    void (*by_event)(const StridedTable);
};

#define PULL_KERNELS(U)                  \
    {k_pull_multi_done<U, PULL_ST_WT>,   \
     {k_pull_multi<U, PULL_ST_NT>, k_pull_multi<U, PULL_ST_PLAIN>}}
#define STRIDED_KERNELS(W, P) \
    {k_pull_strided_done<W, P, PULL_ST_WT>, k_pull_strided<W, P>}

static inline void launch_pull(const PullTable &t, int unroll, bool nt,
                               unsigned blocks, hipStream_t cs,
                               const PullDone *done)
{
    static const PullKernel variants[3] = {PULL_KERNELS(1), PULL_KERNELS(8),
                                           PULL_KERNELS(4)};
    const PullKernel &k = variants[unroll == 1 ? 0 : unroll == 8 ? 1 : 2];
    if (done != nullptr)
        hipLaunchKernelGGL(k.by_word, dim3(blocks), dim3(PULL_THREADS), 0, cs,
                           t, *done);
    else
        hipLaunchKernelGGL(k.by_event[nt ? 0 : 1], dim3(blocks),
                           dim3(PULL_THREADS), 0, cs, t);
}

static inline void launch_strided(const StridedTable &t, bool wide, bool parts,
                                  unsigned blocks, hipStream_t cs,
                                  const PullDone *done)
{
    static const StridedKernel variants[2][2] = {
        {STRIDED_KERNELS(true, true), STRIDED_KERNELS(true, false)},
        {STRIDED_KERNELS(false, true), STRIDED_KERNELS(false, false)}};
    const StridedKernel &k = variants[wide ? 0 : 1][parts ? 0 : 1];
    if (done != nullptr)
        hipLaunchKernelGGL(k.by_word, dim3(blocks), dim3(PULL_THREADS), 0, cs,
                           t, *done);
    else
        hipLaunchKernelGGL(k.by_event, dim3(blocks), dim3(PULL_THREADS), 0, cs,
                           t);
}

/* the reducing pull: k_pull_reduce_done when `done` is given, else
 * k_pull_reduce */
static inline void launch_reduce(const ReduceTable &t, unsigned blocks,
                                 hipStream_t cs, const PullDone *done)
{
    if (done != nullptr)
        hipLaunchKernelGGL(k_pull_reduce_done, dim3(blocks),
                           dim3(PULL_THREADS), 0, cs, t, *done);
    else
        hipLaunchKernelGGL(k_pull_reduce, dim3(blocks), dim3(PULL_THREADS), 0,
                           cs, t);
}

/* the strided reducing pull: k_pull_strided_reduce_done when `done` is
 * given, else k_pull_strided_reduce; `wide`: the 64-bit-division pair.  A
 * template only so that the four kernels (1.6 MB of code, a minute to
 * compile) are emitted by the files that launch them, not by every file
 * that includes this header. */
template <typename Table = StridedReduceTable>
static inline void launch_strided_reduce(const Table &t,
                                         bool wide, unsigned blocks,
                                         hipStream_t cs, const PullDone *done)
{
    if (done != nullptr)
        hipLaunchKernelGGL(wide ? k_pull_strided_reduce_done<true>
                                : k_pull_strided_reduce_done<false>,
                           dim3(blocks), dim3(PULL_THREADS), 0, cs, t, *done);
    else
        hipLaunchKernelGGL(wide ? k_pull_strided_reduce<true>
                                : k_pull_strided_reduce<false>,
                           dim3(blocks), dim3(PULL_THREADS), 0, cs, t);
}

#undef PULL_KERNELS
#undef STRIDED_KERNELS

static inline void launch_tail(uint64_t *word, uint64_t seq, hipStream_t cs)
{
    hipLaunchKernelGGL(k_pull_tail, dim3(1), dim3(1), 0, cs, word, seq);
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_PULL_KERNELS_H */
