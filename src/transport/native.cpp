/* mpix — native intra-node data plane: shared-memory control + xGMI data.
 *
 * The reference delegates all data movement to a CUDA-aware host MPI
 * (SURVEY.md §2b).  On an MI355X node the fast path between GPUs is direct
 * peer-to-peer over xGMI, so this transport implements tag-matched
 * point-to-point natively:
 *
 *  control plane  per ordered rank pair (s -> r), an SPSC descriptor ring in
 *                 a POSIX shm segment owned by r, plus a chunked staging
 *                 buffer for host payloads.
 *  device data    sender publishes {hipIpcMemHandle, offset}; the RECEIVER
 *                 pulls with hipMemcpyAsync over xGMI (SDMA) on a private
 *                 stream and acks with a DONE descriptor.  Same-process /
 *                 same-rank transfers skip IPC and use the raw pointer.
 *                 Consecutive partitions of one request go out as a RUN:
 *                 one descriptor, one pull, one DONE per acked range
 *                 (part_run.h); an ack to ourselves skips the ring.
 *  host data      sender stages through the shm chunk ring (64 KiB chunks,
 *                 credit-based flow control); the receiver copies chunks
 *                 straight into the posted buffer (or an unexpected-message
 *                 heap buffer).  Send completes when fully staged (buffered-
 *                 send semantics), so no ack round-trip.
 *
 * Matching: (comm_id, src rank, tag, partitioned?, partition) with
 * MPI_ANY_SOURCE / MPI_ANY_TAG wildcards; descriptor rings are FIFO per
 * sender, posted receives match in post order — this preserves MPI
 * non-overtaking per (src, tag, comm) pair, which the reference explicitly
 * does not (README.md:173-176).
 *
 * Single-threaded by construction: only the proxy thread touches this object
 * after construction.
 */
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <hip/hip_runtime.h>

#include <deque>
#include <list>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../internal.h"
#include "bootstrap.h"
#include "done_ring.h"
#include "layout.h"
#include "part_run.h"
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

/* Sender-push threshold for small DEVICE payloads: stage D2H into the shm
 * chunk ring like a host message (receiver H2D's it out), skipping the
 * NOTIFY/pull/ACK round trip.  Measured WORSE (74-97 us vs ~38 us half-RTT:
 * the two proxy-synchronous staging copies cost more than the round trip
 * they remove — profiles/r02_pingpong_devpush.json); kept off, tunable for
 * experiments with MPIX_DEV_PUSH_MAX=<bytes>. */
static bool env_flag(const char *name)
{
    const char *e = getenv(name);
    return e && atoi(e);
}

/* MPIX_TRACE=1, read once (as in proxy.cpp) */
static bool trace_on()
{
    static const bool v = env_flag("MPIX_TRACE");
    return v;
}

static uint64_t dev_push_max()
{
    static const uint64_t v = [] {
        const char *e = getenv("MPIX_DEV_PUSH_MAX");
        return e ? (uint64_t)atoll(e) : (uint64_t)0;
    }();
    return v;
}

/* MPIX_PART_RUNS=0, read once: the sender announces every partition with a
 * descriptor of its own (runs of length 1 only), as before part_run.h.
 * An A/B inside one build, and the way tests drive both protocols. */
static bool part_runs_on()
{
    static const bool v = [] {
        const char *e = getenv("MPIX_PART_RUNS");
        return e ? atoi(e) != 0 : true;
    }();
    return v;
}

/* MPIX_PULL_DONE=word|event, read once: how a pull kernel's completion
 * reaches the proxy.  event (default): an event recorded behind the launch
 * and tested with hipEventQuery in every pass.  word: the kernel's last
 * block stores a sequence number to pinned host memory (done_ring.h,
 * pull_signal_done); no event, no runtime call per pass.  The A/B is in
 * profiles/batch_handoffs.md. */
static bool pull_done_word()
{
    static const bool v = [] {
        const char *e = getenv("MPIX_PULL_DONE");
        if (e != nullptr && strcmp(e, "word") != 0 && strcmp(e, "event") != 0)
            MPIX_ERR("MPIX_PULL_DONE=%s is neither word nor event: event", e);
        return e != nullptr && strcmp(e, "word") == 0;
    }();
    return v;
}

/* ------------------------------------------------------------- shm layout */

static constexpr uint32_t RING_SLOTS_DEFAULT = 1024;
static constexpr uint64_t CHUNK_BYTES = 64 * 1024;
static constexpr uint32_t STAGE_CHUNKS_DEFAULT = 64; /* 4 MiB per pair */

enum DescType : uint32_t {
    DESC_HOST_CHUNK = 1, /* one staged chunk of a host-buffer message */
    DESC_DEV_NOTIFY = 2, /* device-buffer message advertisement, or a run of
                            partitions (count > 1) */
    DESC_DONE       = 3, /* receiver ack for DESC_DEV_NOTIFY: all of it, or
                            the range {partition, count} of a run */
};

enum DescFlags : uint32_t {
    DESCF_PARTITIONED = 1u << 0,
    DESCF_SELF_PTR    = 1u << 1, /* ipc field holds a raw pointer (same proc) */
    DESCF_STRIDED     = 1u << 2, /* layout field holds the sender's layout */
};

struct alignas(64) Desc {
    uint32_t type = 0;
    uint32_t flags = 0;
    uint64_t token = 0;       /* sender-side slot index */
    int32_t src_world = -1;
    int32_t tag = 0;
    uint32_t comm_id = 0;
    int32_t partition = -1;   /* a run (count > 1): its first partition */
    uint64_t msg_bytes = 0;   /* a run: the size of ONE partition */
    union {
        uint64_t chunk_off = 0; /* HOST_CHUNK: offset of this chunk in the
                                   msg */
        int64_t part_stride;  /* DEV_NOTIFY of a partition: bytes between
                                 partition p and p+1 at the SENDER (the
                                 request's; not msg_bytes when there are
                                 gaps).  Shares the word: a notify has no
                                 chunks. */
    };
    uint64_t chunk_bytes = 0;
    uint64_t stage_chunk = 0; /* HOST_CHUNK: chunk index in the stage ring */
    uint8_t ipc[64] = {};     /* DEV_NOTIFY: hipIpcMemHandle_t (or raw ptr) */
    uint64_t ipc_off = 0;
    int32_t src_dev = -1;
    uint32_t count = 0;       /* DEV_NOTIFY: partitions partition ..
                                 partition+count-1 of one request, laid out
                                 alike, part_stride apart (part_run.h);
                                 DONE: that many partitions from `partition`
                                 on are finished.  0 reads as 1. */
    uint64_t t_seen_ns = 0;   /* DEV_NOTIFY: sender saw PENDING (MPIX_STATS=1;
                                 steady clock, comparable across the node) */
    MPIX_Layout layout = {};  /* DEV_NOTIFY / first HOST_CHUNK of a message
                                 with DESCF_STRIDED: the sender's normalised
                                 layout (both ends are the same build) */
};
static_assert(sizeof(Desc) == 192, "Desc layout"); /* layout took the pad */

struct alignas(64) InboxHdr {
    alignas(64) std::atomic<uint64_t> head;       /* producer (peer proxy) */
    alignas(64) std::atomic<uint64_t> tail;       /* consumer (my proxy) */
    alignas(64) std::atomic<uint64_t> stage_tail; /* chunks released by me */
};

struct ShmGeom {
    uint32_t ring_slots;
    uint32_t stage_chunks;
    size_t inbox_bytes;   /* hdr + ring + stage, 64-aligned */
    size_t segment_bytes; /* nranks inboxes */
};

static ShmGeom shm_geometry(int nranks)
{
    ShmGeom g;
    g.ring_slots = RING_SLOTS_DEFAULT;
    if (const char *p = getenv("MPIX_SHM_RING")) g.ring_slots = atoi(p);
    g.stage_chunks = STAGE_CHUNKS_DEFAULT;
    if (const char *p = getenv("MPIX_SHM_STAGE_CHUNKS")) g.stage_chunks = atoi(p);
    size_t b = sizeof(InboxHdr) + (size_t)g.ring_slots * sizeof(Desc) +
               (size_t)g.stage_chunks * CHUNK_BYTES;
    g.inbox_bytes = (b + 63) & ~(size_t)63;
    g.segment_bytes = g.inbox_bytes * (size_t)nranks;
    return g;
}

/* views into one inbox */
struct InboxView {
    InboxHdr *hdr;
    Desc *ring;
    char *stage;
};

static InboxView inbox_view(void *seg_base, const ShmGeom &g, int src)
{
    char *p = (char *)seg_base + (size_t)src * g.inbox_bytes;
    InboxView v;
    v.hdr = (InboxHdr *)p;
    v.ring = (Desc *)(p + sizeof(InboxHdr));
    v.stage = (char *)(v.ring + g.ring_slots);
    return v;
}

/* -------------------------------------------------------------- transport */

class NativeTransport : public Transport {
public:
    NativeTransport(int rank, int size, bool mpi_mode, bool have_gpu, int dev)
        : rank_(rank), size_(size), have_gpu_(have_gpu), dev_(dev),
          mpi_mode_(mpi_mode) {}

    int init();
    void shutdown(); /* called from MPIX_Finalize before dtor */
    ~NativeTransport() override;

    int start(Op *op) override;
    void progress() override;
    const char *name() const override { return "native-shm-xgmi"; }

private:
    /* ---- send side ---- */
    struct SendState {
        Op *op;
        uint64_t staged = 0;   /* bytes staged so far (host path) */
        bool notified = false; /* DEV_NOTIFY emitted */
    };
    /* per-destination FIFO queues (preserves non-overtaking) */
    std::map<int, std::deque<SendState>> sendq_;
    /* device sends awaiting DONE: token (slot of the first op) -> the op,
     * or the run of partitions announced under that token */
    struct AwaitDone {
        Op *op;       /* first (or only) op */
        Request *req; /* owner of a run (k > 1), else unused */
        RunAwait run;
    };
    std::unordered_map<uint64_t, AwaitDone> await_done_;
    /* pending DONE descriptors we could not emit (ring full) */
    struct PendingDone {
        int dst;
        uint64_t token;
        int32_t first;
        uint32_t count;
    };
    std::deque<PendingDone> pending_done_;

    /* ---- recv side ---- */
    struct InboundMsg {
        Desc d;                 /* first descriptor (header info) */
        int src;                /* sending world rank */
        Op *op = nullptr;       /* matched recv, or null */
        std::vector<char> heap; /* unexpected host payload buffer */
        uint64_t got = 0;       /* host bytes received so far */
        bool dev_copy_started = false;
        bool kind_mismatch = false; /* strided msg between host and device */
    };
    std::list<InboundMsg> inbound_;                 /* arrival order */
    std::unordered_map<uint64_t, InboundMsg *> inbound_by_token_;
    std::vector<Op *> posted_recvs_;                /* post order */

    struct CopyInflight {
        Op *op;
        hipEvent_t ev;
        int src;
        uint64_t token;
        int32_t partition;
        ChStatus st;
    };
    std::list<CopyInflight> copies_;

    /* pulls collected this progress pass, flushed as ONE kernel launch */
    struct PendingPull {
        Op *op;             /* first (or only) receive */
        int src;
        uint64_t token;
        ChStatus st;        /* of each of its receives */
        void *dst;
        const void *csrc;
        uint64_t n;         /* all k receives together */
        uint64_t t_seen_ns; /* both sides seen PENDING (MPIX_STATS=1) */
        int32_t partition;  /* of the first receive (for the ack) */
        uint32_t k;         /* receives it completes: 1, or the partitions
                               partition .. partition+k-1 of op->req, taken
                               as one copy (the fast path of a run) */
    };
    /* receive j of a pull */
    static Op *pull_op(const PendingPull &pp, uint32_t j) {
        return j == 0 ? pp.op
                      : &g_state->ops[pp.op->req->part_idx[pp.partition + j]];
    }
    static size_t pull_ops(const std::vector<PendingPull> &v, size_t n) {
        size_t ops = 0;
        for (size_t i = 0; i < n; i++) ops += v[i].k;
        return ops;
    }
    void finish_pull(const PendingPull &pp, BatchStat *bs);
    std::vector<PendingPull> pend_pulls_;
    struct PullBatch {
        hipEvent_t ev = nullptr; /* event path; word path: only MPIX_STATS=1 */
        int done_slot = -1;   /* word path: slot of done_ring_, else -1 */
        hipStream_t cs = nullptr;
        uint64_t t_born_ns = 0;  /* word path: for the lost-signal guard */
        uint32_t passes = 0;     /* word path: passes that found no word */
        uint64_t t_launch_ns = 0; /* MPIX_STATS=1 */
        bool first = false;   /* MPIX_STATS=1: first batch of the process */
        std::vector<PendingPull> items;
    };
    std::list<PullBatch> batches_;
    /* MPIX_PULL_DONE=word: completion words in pinned host memory, one per
     * 64 bytes, and arrival counters in device memory, one per 128 bytes
     * (done_ring.h has the bookkeeping) */
    static constexpr size_t DONE_WORD_STRIDE = 8;     /* in uint64_t */
    static constexpr size_t DONE_COUNTER_STRIDE = 32; /* in uint32_t */
    bool done_word_ = false;
    DoneRing done_ring_;
    std::atomic<uint64_t> *done_words_ = nullptr; /* host view */
    uint64_t *done_words_d_ = nullptr;            /* device view */
    uint32_t *done_counters_ = nullptr;
    /* a batch on the word path: slot and kernel argument, or -1 (event
     * path: MPIX_PULL_DONE=event, or the ring is full) */
    int done_begin(PullDone *d);
    /* MPIX_STATS=1 with word: the event recorded all the same, kept after
     * the word was seen to measure word seen -> event seen */
    struct WordEvent {
        hipEvent_t ev;
        uint64_t t_word_ns;
    };
    std::list<WordEvent> word_events_;
    bool batch_done(PullBatch &b, hipError_t *err);
    void close_batch(PullBatch &b, hipStream_t cs, int slot, bool stats);
    PullTable plan_{}; /* scratch of flush_pulls; passed by value */
    void launch_pull(unsigned blocks, hipStream_t cs, const PullDone *done);

    /* strided pulls collected this progress pass: ONE k_pull_strided launch
     * per MPIX_STRIDED_BATCH of them, completed through batches_ like the
     * contiguous ones */
    struct PendingStrided {
        PendingPull pp;
        MPIX_Layout sl, dl; /* normalised source / destination layouts */
        /* a run that did not fold: pp.k partitions laid out as sl / dl,
         * these many bytes apart (parts false: one message, or a folded
         * run whose sl / dl already span all of pp.n) */
        bool parts = false;
        int64_t s_part_stride = 0, d_part_stride = 0;
    };
    std::vector<PendingStrided> pend_strided_;
    StridedTable splan_{}; /* scratch of flush_strided; passed by value */
    bool strided_div64_ = false; /* MPIX_STRIDED_DIV64=1: see plan_strided */

    /* ---- shm ---- */
    ShmGeom geom_{};
    std::string my_seg_name_;
    std::vector<void *> seg_;       /* seg_[r] = rank r's segment base */
    std::vector<uint64_t> out_head_; /* producer-local head per dst */
    std::vector<uint64_t> out_stage_head_; /* producer-local chunk cursor */
    std::vector<uint64_t> in_tail_;  /* consumer-local tail per src */

    /* ---- hip ---- */
    /* Copy-stream POOL.  Stream 0 is PLAIN and carries small pulls plus
     * synchronous staging (lowest latency: a priority queue costs ~17 us
     * extra half-RTT, ci_full2); streams 1..3 are created at GREATEST
     * PRIORITY and carry large pulls concurrently — large partitioned
     * transfers were latency-bound at ~9 us/partition serialized on one
     * stream.  The high-priority set can never share a hardware queue
     * with user streams (different priority = different queue), which
     * matters beyond spin kernels: an unsatisfied hipStreamWaitValue32 is
     * a queue-parking packet, so a SAME-priority copy stream that aliases
     * a user stream's queue deadlocks exactly like the graph spin-kernel
     * case (observed when a 4-plain-stream pool pushed total streams past
     * the 4-queue pool: every transfer hung).  Stream 0 carries the same
     * small residual aliasing risk as the original single-stream design
     * (mitigated by the lazy priority upgrade below). */
    static constexpr int N_COPY_STREAMS = 4;
    hipStream_t copy_streams_[N_COPY_STREAMS] = {};
    hipStream_t copy_plain0_ = nullptr; /* pre-upgrade stream 0 (kept) */
    bool prio_switched_ = false;
    static uint64_t pool_min_bytes() {
        static const uint64_t v = [] {
            const char *e = getenv("MPIX_COPY_POOL_MIN");
            return e ? (uint64_t)atoll(e) : (uint64_t)(256 << 10);
        }();
        return v;
    }

    /* The copy stream must never share a hardware queue with a stream that
     * holds a SPIN-WAIT kernel: HIP muxes same-priority streams onto a
     * small HSA queue pool, and GRAPH execution orders its queue with AQL
     * barrier packets — a k_wait_flag graph node parked in front of our
     * pull/blit packet blocks it forever, while that wait needs this very
     * copy to finish (deterministic after stream churn rotated the
     * mapping: gpurun_out/diag5_loop5.log).  Streams of different
     * priorities never share a queue, but an always-priority copy stream
     * costs ~17 us extra half-RTT with two processes on one GPU
     * (gpurun_out/ci_full2: 54 us vs 37.9), so the switch is LAZY: plain
     * stream until the library emits its first spin-wait kernel
     * (mark_spin_wait in enqueue.cpp — ordered before any graph launch
     * that could contain one), then migrate to a greatest-priority stream.
     * In-flight copies on the plain stream finish normally (events). */
    void maybe_switch_prio() {
        if (prio_switched_ || g_state == nullptr ||
            !g_state->spin_wait_kernels.load(std::memory_order_acquire))
            return;
        prio_switched_ = true;
        int lo = 0, hi = 0;
        hipStream_t ps = nullptr;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess &&
            hi != lo &&
            hipStreamCreateWithPriority(&ps, hipStreamNonBlocking, hi) ==
                hipSuccess) {
            copy_plain0_ = copy_streams_[0];
            copy_streams_[0] = ps;
        } else {
            (void)hipGetLastError();
        }
    }
    /* stream for an independent pull: small payloads ride the plain
     * stream 0 (latency), large ones rotate over the priority set 1..3
     * (bandwidth; per-message ordering is by the event recorded on the
     * same stream as the copy) */
    hipStream_t copy_stream(uint64_t bytes) {
        maybe_switch_prio();
        if (bytes <= pool_min_bytes() || copy_streams_[1] == nullptr)
            return copy_streams_[0];
        return copy_streams_[1];
    }
    /* fixed stream for synchronous staging (memcpy_auto) */
    hipStream_t copy_stream0() {
        maybe_switch_prio();
        return copy_streams_[0];
    }
    std::vector<hipEvent_t> event_pool_;
    std::unordered_map<std::string, void *> ipc_open_;   /* handle -> ptr */
    std::unordered_map<const void *, std::pair<void *, hipIpcMemHandle_t>>
        ipc_get_;                                        /* buf base -> handle */

    Bootstrap *boot_ = nullptr;

    int rank_, size_;
    bool have_gpu_;
    int dev_;
    bool mpi_mode_;
    bool shut_ = false;

    /* helpers */
    InboxView my_inbox(int src) { return inbox_view(seg_[rank_], geom_, src); }
    InboxView out_box(int dst) { return inbox_view(seg_[dst], geom_, rank_); }

    bool ring_has_space(int dst, uint64_t need) {
        InboxView v = out_box(dst);
        uint64_t tail = v.hdr->tail.load(std::memory_order_acquire);
        return out_head_[dst] + need - tail <= geom_.ring_slots;
    }
    void emit_desc(int dst, const Desc &d) {
        InboxView v = out_box(dst);
        uint64_t h = out_head_[dst];
        v.ring[h % geom_.ring_slots] = d;
        v.hdr->head.store(h + 1, std::memory_order_release);
        out_head_[dst] = h + 1;
    }
    uint64_t stage_free_chunks(int dst) {
        InboxView v = out_box(dst);
        uint64_t st = v.hdr->stage_tail.load(std::memory_order_acquire);
        return geom_.stage_chunks - (out_stage_head_[dst] - st);
    }

    hipEvent_t get_event();
    void put_event(hipEvent_t ev);

    int progress_sends();
    int drain_inbox(int src);
    int progress_copies();
    void flush_pulls();
    void flush_strided();
    void fail_kind_mismatch(InboundMsg &m);
    void handle_desc(int src, const Desc &d, const char *stage_base);
    bool try_run_fast_path(int src, const Desc &d, uint32_t k);
    void ack(int src, uint64_t token, int32_t first, uint32_t count);
    void handle_done(uint64_t token, int32_t first, uint32_t count);
    void try_match_new_inbound(InboundMsg &m);
    void attach(InboundMsg &m, Op *op);
    void start_dev_copy(InboundMsg &m);
    void finish_host_recv(InboundMsg &m);
    void deliver_chunk(InboundMsg &m, const Desc &d, const char *src_chunk);
    void erase_inbound(InboundMsg *m);
    int memcpy_auto(void *dst, const void *src, size_t n);
    void *map_remote(const Desc &d);
    bool match(const Op *op, const Desc &d, int src) const;
    void complete_send_buffered(Op *op);
};

/* ------------------------------------------------------------------- init */

int NativeTransport::init()
{
    boot_ = make_bootstrap(rank_, size_, mpi_mode_);
    if (!boot_) return -1;

    geom_ = shm_geometry(size_);

    /* create my segment */
    char name[96];
    unsigned seed = (unsigned)getpid() * 2654435761u + (unsigned)rank_;
    snprintf(name, sizeof(name), "/mpix-r%d-%d-%x", rank_, (int)getpid(),
             rand_r(&seed));
    my_seg_name_ = name;
    int fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0) {
        MPIX_ERR("shm_open(%s) failed", name);
        return -1;
    }
    if (ftruncate(fd, (off_t)geom_.segment_bytes) != 0) {
        MPIX_ERR("ftruncate(%zu) failed", geom_.segment_bytes);
        close(fd);
        return -1;
    }
    void *base = mmap(nullptr, geom_.segment_bytes, PROT_READ | PROT_WRITE,
                      MAP_SHARED, fd, 0);
    close(fd);
    if (base == MAP_FAILED) {
        MPIX_ERR("mmap own segment failed");
        return -1;
    }
    memset(base, 0, geom_.segment_bytes);

    /* exchange names, open peers */
    struct Blob { char name[96]; };
    Blob mine{};
    snprintf(mine.name, sizeof(mine.name), "%s", name);
    std::vector<Blob> all(size_);
    if (boot_->allgather(&mine, all.data(), sizeof(Blob)) != 0) {
        MPIX_ERR("bootstrap allgather failed");
        return -1;
    }
    seg_.assign(size_, nullptr);
    seg_[rank_] = base;
    for (int r = 0; r < size_; r++) {
        if (r == rank_) continue;
        int pfd = shm_open(all[r].name, O_RDWR, 0600);
        if (pfd < 0) {
            MPIX_ERR("shm_open(peer %s) failed", all[r].name);
            return -1;
        }
        void *pb = mmap(nullptr, geom_.segment_bytes, PROT_READ | PROT_WRITE,
                        MAP_SHARED, pfd, 0);
        close(pfd);
        if (pb == MAP_FAILED) {
            MPIX_ERR("mmap peer segment failed");
            return -1;
        }
        seg_[r] = pb;
    }
    /* everyone mapped everything -> segments can be unlinked */
    boot_->barrier();
    shm_unlink(my_seg_name_.c_str());

    out_head_.assign(size_, 0);
    out_stage_head_.assign(size_, 0);
    in_tail_.assign(size_, 0);

    strided_div64_ = env_flag("MPIX_STRIDED_DIV64");

    if (have_gpu_) {
        if (hipStreamCreateWithFlags(&copy_streams_[0],
                                     hipStreamNonBlocking) != hipSuccess) {
            MPIX_ERR("copy stream create failed");
            return -1;
        }
        /* NO standing second stream: every additional hardware queue
         * (even per another process) oversubscribes the device's HW
         * scheduler and adds tens of us to every wait — a standing
         * priority stream alone pushed the 2-process 8-B half-RTT from
         * 36.5 to ~55 us.  Batched pulls serialize on stream 0 at HBM
         * rate, so extra streams buy nothing; MPIX_COPY_PRIO_STREAM=1
         * opts a standing priority stream back in for experiments. */
        if (pull_done_word()) {
            void *w = nullptr, *wd = nullptr, *c = nullptr;
            const size_t wbytes =
                MPIX_DONE_SLOTS * DONE_WORD_STRIDE * sizeof(uint64_t);
            const size_t cbytes =
                MPIX_DONE_SLOTS * DONE_COUNTER_STRIDE * sizeof(uint32_t);
            if (hipHostMalloc(&w, wbytes, hipHostMallocMapped) != hipSuccess ||
                hipHostGetDevicePointer(&wd, w, 0) != hipSuccess ||
                hipMalloc(&c, cbytes) != hipSuccess ||
                hipMemset(c, 0, cbytes) != hipSuccess) {
                MPIX_ERR("MPIX_PULL_DONE=word: completion words not allocated");
                return -1;
            }
            memset(w, 0, wbytes);
            done_words_ = reinterpret_cast<std::atomic<uint64_t> *>(w);
            done_words_d_ = (uint64_t *)wd;
            done_counters_ = (uint32_t *)c;
            done_word_ = true;
        }
        if (env_flag("MPIX_COPY_PRIO_STREAM")) {
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess &&
                hi != lo) {
                if (hipStreamCreateWithPriority(&copy_streams_[1],
                                                hipStreamNonBlocking, hi) !=
                    hipSuccess) {
                    (void)hipGetLastError();
                    copy_streams_[1] = nullptr;
                }
            } else {
                (void)hipGetLastError();
            }
        }
    }
    return 0;
}

void NativeTransport::shutdown()
{
    if (shut_) return;
    shut_ = true;
    /* make sure no peer is still reading our segment */
    if (boot_) boot_->barrier();
    for (auto &kv : ipc_open_) (void)hipIpcCloseMemHandle(kv.second);
    ipc_open_.clear();
    for (WordEvent &we : word_events_) event_pool_.push_back(we.ev);
    word_events_.clear();
    for (hipEvent_t ev : event_pool_) (void)hipEventDestroy(ev);
    event_pool_.clear();
    if (done_words_) (void)hipHostFree((void *)done_words_);
    if (done_counters_) (void)hipFree(done_counters_);
    done_words_ = nullptr;
    done_words_d_ = nullptr;
    done_counters_ = nullptr;
    done_word_ = false;
    for (int i = 0; i < N_COPY_STREAMS; i++) {
        if (copy_streams_[i]) (void)hipStreamDestroy(copy_streams_[i]);
        copy_streams_[i] = nullptr;
    }
    if (copy_plain0_) (void)hipStreamDestroy(copy_plain0_);
    copy_plain0_ = nullptr;
    for (int r = 0; r < (int)seg_.size(); r++)
        if (seg_[r]) munmap(seg_[r], geom_.segment_bytes);
    seg_.clear();
    delete boot_;
    boot_ = nullptr;
}

NativeTransport::~NativeTransport() { shutdown(); }

/* ------------------------------------------------------------------ events */

hipEvent_t NativeTransport::get_event()
{
    if (!event_pool_.empty()) {
        hipEvent_t ev = event_pool_.back();
        event_pool_.pop_back();
        return ev;
    }
    hipEvent_t ev = nullptr;
    (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    return ev;
}

void NativeTransport::put_event(hipEvent_t ev) { event_pool_.push_back(ev); }

/* ------------------------------------------------------------------- start */

int NativeTransport::start(Op *op)
{
    /* the proxy stamps this again after start() returns; the batch legs
     * need it already while the op is matched in here */
    if (g_state->stats) op->t_issue_ns = now_ns();
    switch (op->kind) {
    case OpKind::ISEND:
    case OpKind::PSEND_PART:
        sendq_[op->peer_world].push_back(SendState{op});
        return 0;
    case OpKind::IRECV:
    case OpKind::PRECV_PART: {
        /* match against already-arrived messages first (FIFO arrival order) */
        for (auto &m : inbound_) {
            if (m.op == nullptr && match(op, m.d, m.src)) {
                attach(m, op);
                return 0;
            }
        }
        posted_recvs_.push_back(op);
        return 0;
    }
    default:
        return -1;
    }
}

bool NativeTransport::match(const Op *op, const Desc &d, int src) const
{
    if (op->comm_id != d.comm_id) return false;
    bool want_part = (op->kind == OpKind::PRECV_PART);
    bool is_part = (d.flags & DESCF_PARTITIONED) != 0;
    if (want_part != is_part) return false;
    if (want_part && op->partition != d.partition) return false;
    if (op->peer_world != MPI_ANY_SOURCE && op->peer_world != src) return false;
    if (op->tag != MPI_ANY_TAG && op->tag != d.tag) return false;
    return true;
}

/* ---------------------------------------------------------------- progress */

void NativeTransport::progress()
{
    progress_sends();
    for (int s = 0; s < size_; s++) drain_inbox(s);
    flush_pulls();
    flush_strided();
    progress_copies();

    /* retry queued DONE acks */
    for (size_t i = 0; i < pending_done_.size();) {
        const PendingDone pd = pending_done_[i];
        if (ring_has_space(pd.dst, 1)) {
            Desc d;
            d.type = DESC_DONE;
            d.token = pd.token;
            d.src_world = rank_;
            d.partition = pd.first;
            d.count = pd.count;
            emit_desc(pd.dst, d);
            pending_done_.erase(pending_done_.begin() + i);
        } else {
            i++;
        }
    }
}

void NativeTransport::complete_send_buffered(Op *op)
{
    op->ch_status.src = (op->comm_id == 1) ? 0 : rank_;
    op->ch_status.tag = op->tag;
    op->ch_status.bytes = op->bytes;
    op->ch_status.err = MPI_SUCCESS;
    op->ch_done.store(1, std::memory_order_release);
}

int NativeTransport::progress_sends()
{
    for (auto &kv : sendq_) {
        int dst = kv.first;
        auto &q = kv.second;
        while (!q.empty()) {
            SendState &ss = q.front();
            Op *op = ss.op;
            /* strided device sends always take the notify/pull path */
            if (op->buf_is_device &&
                (op->strided || op->bytes > dev_push_max())) {
                if (!ring_has_space(dst, 1)) break;
                /* the run of partitions at the head of the queue goes out
                 * as ONE descriptor (part_run.h); anything else is a run
                 * of 1, today's descriptor */
                size_t k = 1;
                if (op->kind == OpKind::PSEND_PART && part_runs_on())
                    k = part_run_length(q.size(), [&q](size_t i) {
                        const Op *o = q[i].op;
                        return RunSend{o->req, o->pseq, o->partition,
                                       o->bytes,
                                       o->kind == OpKind::PSEND_PART,
                                       o->buf_is_device, o->strided};
                    }, dev_push_max());
                Desc d;
                d.type = DESC_DEV_NOTIFY;
                d.count = (uint32_t)k;
                d.flags = (op->kind == OpKind::PSEND_PART) ? DESCF_PARTITIONED : 0;
                d.token = (uint64_t)(op - g_state->ops);
                d.src_world = rank_;
                d.tag = op->tag;
                d.comm_id = op->comm_id;
                d.partition = op->partition;
                d.msg_bytes = op->bytes;
                d.src_dev = dev_;
                d.t_seen_ns = op->t_issue_ns;
                /* the request's, never inferred from msg_bytes: contiguous
                 * partitions may have gaps between them */
                if (op->kind == OpKind::PSEND_PART && op->req != nullptr)
                    d.part_stride = op->req->part_stride;
                if (op->strided) {
                    d.flags |= DESCF_STRIDED;
                    d.layout = op->layout;
                }
                if (dst == rank_) {
                    d.flags |= DESCF_SELF_PTR;
                    uint64_t p = (uint64_t)(uintptr_t)op->buf;
                    memcpy(d.ipc, &p, 8);
                    d.ipc_off = 0;
                } else {
                    /* IPC handle of the allocation base + offset */
                    void *base = nullptr;
                    hipError_t e = hipPointerGetAttribute(
                        &base, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR,
                        (hipDeviceptr_t)op->buf);
                    if (e != hipSuccess || base == nullptr) base = op->buf;
                    auto it = ipc_get_.find(base);
                    if (it == ipc_get_.end()) {
                        hipIpcMemHandle_t h;
                        if (hipIpcGetMemHandle(&h, base) != hipSuccess) {
                            MPIX_ERR("hipIpcGetMemHandle failed (buf %p)", base);
                            /* the rest of a run fails the same way, op by
                             * op, on the next turns of this loop */
                            op->ch_status.err = MPI_ERR_OTHER;
                            op->ch_done.store(1, std::memory_order_release);
                            q.pop_front();
                            continue;
                        }
                        it = ipc_get_.emplace(base, std::make_pair(base, h)).first;
                    }
                    memcpy(d.ipc, &it->second.second, sizeof(hipIpcMemHandle_t));
                    d.ipc_off = (uint64_t)((char *)op->buf - (char *)base);
                }
                /* before the descriptor is visible: a self-loopback ack
                 * comes back on this thread, another rank's through the
                 * ring, both after this */
                await_done_[d.token] = AwaitDone{
                    op, op->req,
                    RunAwait{op->partition, (uint32_t)k, (uint32_t)k}};
                emit_desc(dst, d);
                g_state->notify_descs++;
                g_state->notify_msgs += k;
                q.erase(q.begin(), q.begin() + (long)k);
                continue;
            }
            /* host-staged path */
            bool stalled = false;
            while (ss.staged < op->bytes || op->bytes == 0) {
                if (!ring_has_space(dst, 1) || stage_free_chunks(dst) == 0) {
                    stalled = true;
                    break;
                }
                uint64_t chunk_idx = out_stage_head_[dst] % geom_.stage_chunks;
                uint64_t n = op->bytes - ss.staged;
                if (n > CHUNK_BYTES) n = CHUNK_BYTES;
                InboxView v = out_box(dst);
                if (n > 0) {
                    char *stage_dst = v.stage + chunk_idx * CHUNK_BYTES;
                    const char *payload = (const char *)op->buf + ss.staged;
                    if (op->strided) /* host buffer: device ones notify */
                        layout_copy_out(stage_dst, op->buf, op->layout,
                                        ss.staged, n);
                    else if (op->buf_is_device)
                        memcpy_auto(stage_dst, payload, n); /* D2H */
                    else
                        memcpy(stage_dst, payload, n);
                }
                Desc d;
                d.type = DESC_HOST_CHUNK;
                d.flags = (op->kind == OpKind::PSEND_PART) ? DESCF_PARTITIONED : 0;
                d.token = (uint64_t)(op - g_state->ops);
                d.src_world = rank_;
                d.tag = op->tag;
                d.comm_id = op->comm_id;
                d.partition = op->partition;
                d.msg_bytes = op->bytes;
                d.chunk_off = ss.staged;
                d.chunk_bytes = n;
                if (op->strided && ss.staged == 0) {
                    d.flags |= DESCF_STRIDED;
                    d.layout = op->layout;
                }
                d.stage_chunk = chunk_idx;
                out_stage_head_[dst]++;
                emit_desc(dst, d);
                ss.staged += n;
                if (op->bytes == 0) break; /* zero-byte message: one desc */
            }
            if (stalled) break; /* preserve FIFO: don't start next send */
            complete_send_buffered(op);
            q.pop_front();
        }
    }
    return 0;
}

int NativeTransport::drain_inbox(int src)
{
    InboxView v = my_inbox(src);
    uint64_t head = v.hdr->head.load(std::memory_order_acquire);
    uint64_t tail = in_tail_[src];
    int budget = 64;
    while (tail < head && budget-- > 0) {
        const Desc &d = v.ring[tail % geom_.ring_slots];
        handle_desc(src, d, v.stage);
        tail++;
        v.hdr->tail.store(tail, std::memory_order_release);
        in_tail_[src] = tail;
    }
    return 0;
}

void NativeTransport::handle_desc(int src, const Desc &d, const char *stage_base)
{
    switch (d.type) {
    case DESC_DONE:
        handle_done(d.token, d.partition, d.count ? d.count : 1);
        return;
    case DESC_DEV_NOTIFY: {
        const uint32_t k = d.count ? d.count : 1;
        if (k > 1 && try_run_fast_path(src, d, k)) return;
        /* one message, or a run expanded in partition order exactly as if k
         * descriptors had arrived: the ring position is the run's, so FIFO
         * order per sender holds.  inbound_by_token_ is not written: only
         * HOST_CHUNK descriptors look messages up by token. */
        for (uint32_t j = 0; j < k; j++) {
            inbound_.emplace_back();
            InboundMsg &m = inbound_.back();
            m.d = d; /* the ring slot is ours until drain_inbox moves tail */
            m.src = src;
            if (k > 1) {
                /* slice j starts j * (the sender's part_stride) further on;
                 * layout and DESCF_STRIDED stay as the run had them */
                const RunSlice sl = part_run_slice(
                    d.partition, d.ipc_off, (uint64_t)d.part_stride, d.token,
                    j);
                m.d.partition = sl.partition;
                m.d.ipc_off = sl.ipc_off;
                m.d.count = sl.count;
            }
            try_match_new_inbound(m);
        }
        return;
    }
    case DESC_HOST_CHUNK: {
        uint64_t key = ((uint64_t)src << 32) ^ d.token;
        InboundMsg *m = nullptr;
        if (d.chunk_off == 0) {
            inbound_.emplace_back();
            m = &inbound_.back();
            m->d = d;
            m->src = src;
            inbound_by_token_[key] = m; /* overwrite OK: FIFO => the previous
                                           msg with this token needs no more
                                           chunks (see erase_inbound) */
            try_match_new_inbound(*m);
        } else {
            auto it = inbound_by_token_.find(key);
            if (it != inbound_by_token_.end()) m = it->second;
        }
        if (m != nullptr)
            deliver_chunk(*m, d, stage_base + d.stage_chunk * CHUNK_BYTES);
        else
            MPIX_ERR("chunk for unknown msg token %lu", (unsigned long)d.token);
        /* release the stage credit unconditionally (no credit leaks) */
        InboxView v = my_inbox(src);
        v.hdr->stage_tail.fetch_add(1, std::memory_order_release);
        if (m != nullptr && m->got >= m->d.msg_bytes) finish_host_recv(*m);
        return;
    }
    default:
        MPIX_ERR("bad descriptor type %u from %d", d.type, src);
    }
}

/* The sender's end of an ack: partitions [first, first+count) of the run
 * announced under `token` (or the single message) are finished. */
void NativeTransport::handle_done(uint64_t token, int32_t first,
                                  uint32_t count)
{
    auto it = await_done_.find(token);
    if (it == await_done_.end()) {
        MPIX_ERR("DONE for unknown token %lu", (unsigned long)token);
        return;
    }
    AwaitDone &a = it->second;
    const RunAck r = part_run_ack(&a.run, first, count);
    if (r == RUN_ACK_BAD) {
        MPIX_ERR("DONE for partitions %d..+%u outside run %d..+%u (%u left) "
                 "of token %lu", first, count, a.run.p0, a.run.k,
                 a.run.remaining, (unsigned long)token);
        return;
    }
    if (a.run.k == 1) {
        complete_send_buffered(a.op);
    } else {
        for (uint32_t j = 0; j < count; j++)
            complete_send_buffered(
                &g_state->ops[a.req->part_idx[first + (int32_t)j]]);
    }
    if (r == RUN_ACK_LAST) await_done_.erase(it);
}

/* The receiver's end: tell rank `src` that partitions [first, first+count)
 * under `token` are finished.  For ourselves the send ops complete right
 * here: through the ring the DONE would be drained one proxy pass later
 * (drain_inbox runs before progress_copies), and a wait on the send
 * request that follows the wait on the receive sits through that pass. */
void NativeTransport::ack(int src, uint64_t token, int32_t first,
                          uint32_t count)
{
    if (src == rank_) {
        handle_done(token, first, count);
        return;
    }
    if (ring_has_space(src, 1)) {
        Desc d;
        d.type = DESC_DONE;
        d.token = token;
        d.src_world = rank_;
        d.partition = first;
        d.count = count;
        emit_desc(src, d);
    } else {
        pending_done_.push_back(PendingDone{src, token, first, count});
    }
}

/* A run of k partitions whose receives are all posted, in order, as the
 * partitions of one request in device memory (part_run_fast_range) is ONE
 * pending pull: no InboundMsg, one erase from posted_recvs_, one entry of a
 * batch.  Which pull is decided by the shape of both sides:
 *  - contiguous partitions msg_bytes apart on both sides, both bases
 *    16-byte aligned: one copy of k * msg_bytes (k_pull_multi);
 *  - the run folds into a layout on each side (part_layout_fold: rows with
 *    a gap, a face split along its outer dimension): one ordinary strided
 *    entry, as if the k partitions were one strided message;
 *  - anything else: a strided entry with a partition level.
 * The last two go by the granule; only the first asks for alignment.
 * false: nothing was touched, the caller expands the run. */
bool NativeTransport::try_run_fast_path(int src, const Desc &d, uint32_t k)
{
    if (!(d.flags & DESCF_PARTITIONED)) return false;
    void *sp = map_remote(d);
    if (sp == nullptr) return false; /* the expansion fails op by op */
    const long first = part_run_fast_range(
        posted_recvs_.size(),
        [&](size_t i) {
            const Op *o = posted_recvs_[i];
            const bool env =
                o->kind == OpKind::PRECV_PART && o->comm_id == d.comm_id &&
                (o->peer_world == MPI_ANY_SOURCE || o->peer_world == src) &&
                (o->tag == MPI_ANY_TAG || o->tag == d.tag);
            RunRecv r{o->req, o->partition, o->bytes, (uintptr_t)o->buf, env,
                      o->buf_is_device, o->strided};
            /* the receiver's own distance between partitions */
            r.part_stride = o->req != nullptr ? o->req->part_stride
                                              : (int64_t)o->bytes;
            return r;
        },
        d.partition, k, d.msg_bytes);
    if (first < 0) return false;
    Op *op = posted_recvs_[(size_t)first];
    /* the receives must be the request's own partitions: finish_pull finds
     * receive j through op->req->part_idx */
    const Request *rq = op->req;
    if (rq == nullptr || d.partition < 0 ||
        (uint64_t)d.partition + k > (uint64_t)rq->n_partitions)
        return false;
    const bool s_strided = (d.flags & DESCF_STRIDED) != 0;
    const bool plain = !s_strided && !op->strided &&
                       d.part_stride == (int64_t)d.msg_bytes &&
                       rq->part_stride == (int64_t)d.msg_bytes;
    /* today's run, and today's rule for it: a misaligned one expands into
     * k hipMemcpyAsync */
    if (plain && ((((uintptr_t)op->buf) | ((uintptr_t)sp)) & 15) != 0)
        return false;
    posted_recvs_.erase(posted_recvs_.begin() + first,
                        posted_recvs_.begin() + first + (long)k);
    ChStatus st;
    st.src = (op->comm_id == 1) ? 0 : src;
    st.tag = d.tag;
    st.bytes = d.msg_bytes;
    st.err = MPI_SUCCESS;
    uint64_t seen = op->t_issue_ns > d.t_seen_ns ? op->t_issue_ns
                                                 : d.t_seen_ns;
    const PendingPull pp{op, src, d.token, st, op->buf, sp,
                         (uint64_t)k * d.msg_bytes, seen, d.partition, k};
    g_state->run_fast_msgs += k;
    if (plain) {
        pend_pulls_.push_back(pp);
        g_state->run_copy++;
        return true;
    }
    PendingStrided ps;
    ps.pp = pp;
    const MPIX_Layout sl =
        s_strided ? d.layout : layout_contiguous(d.msg_bytes);
    const MPIX_Layout dl =
        op->strided ? op->layout : layout_contiguous(op->bytes);
    if (!part_layout_fold(sl, k, d.part_stride, &ps.sl) ||
        !part_layout_fold(dl, k, rq->part_stride, &ps.dl)) {
        ps.sl = sl;
        ps.dl = dl;
        ps.parts = true;
        ps.s_part_stride = d.part_stride;
        ps.d_part_stride = rq->part_stride;
    }
    (ps.parts ? g_state->run_parts : g_state->run_folded)++;
    pend_strided_.push_back(ps);
    return true;
}

/* Every receive of a pull gets its status and ch_done (the per-partition
 * flag transitions stay with the proxy walk); the sender gets ONE ack. */
void NativeTransport::finish_pull(const PendingPull &pp, BatchStat *bs)
{
    if (bs != nullptr && pp.src == rank_) {
        /* MPIX_STATS=1, loopback: the send ops this ack completes belong to
         * the batch's event -> last-send leg (before the ack: it erases the
         * entry) */
        auto it = await_done_.find(pp.token);
        if (it != await_done_.end()) {
            const AwaitDone &a = it->second;
            for (uint32_t j = 0; j < pp.k; j++) {
                Op *so = a.run.k == 1
                    ? a.op
                    : &g_state->ops[a.req->part_idx[pp.partition + (int32_t)j]];
                so->stat_batch = bs;
                bs->left_send++;
            }
        }
    }
    ack(pp.src, pp.token, pp.partition, pp.k);
    for (uint32_t j = 0; j < pp.k; j++) {
        Op *op = pull_op(pp, j);
        op->stat_batch = bs;
        op->ch_status = pp.st;
        op->ch_done.store(1, std::memory_order_release);
    }
}

void NativeTransport::try_match_new_inbound(InboundMsg &m)
{
    for (size_t i = 0; i < posted_recvs_.size(); i++) {
        Op *op = posted_recvs_[i];
        if (match(op, m.d, m.src)) {
            posted_recvs_.erase(posted_recvs_.begin() + i);
            attach(m, op);
            return;
        }
    }
    /* unexpected: host messages buffer into heap as chunks arrive */
    if (m.d.type == DESC_HOST_CHUNK) m.heap.resize(m.d.msg_bytes);
}

void NativeTransport::attach(InboundMsg &m, Op *op)
{
    op->ch_priv = &m;
    m.op = op;
    if (m.d.type == DESC_DEV_NOTIFY) {
        start_dev_copy(m);
        return;
    }
    if ((op->strided || (m.d.flags & DESCF_STRIDED)) && op->buf_is_device) {
        fail_kind_mismatch(m);
    } else if (m.got > 0 && !m.heap.empty()) {
        /* host message: move already-buffered bytes (message order) into
         * the user buffer */
        uint64_t n = m.got;
        if (n > op->bytes) n = op->bytes;
        if (n > 0 && op->strided)
            layout_copy_in(op->buf, op->layout, 0, m.heap.data(), n);
        else if (n > 0)
            memcpy_auto(op->buf, m.heap.data(), n);
    }
    m.heap.clear();
    m.heap.shrink_to_fit();
    if (m.got >= m.d.msg_bytes) finish_host_recv(m);
}

void NativeTransport::deliver_chunk(InboundMsg &m, const Desc &d,
                                    const char *src_chunk)
{
    if (m.op != nullptr) {
        uint64_t room = (m.op->bytes > d.chunk_off)
                            ? m.op->bytes - d.chunk_off : 0;
        uint64_t n = d.chunk_bytes < room ? d.chunk_bytes : room;
        /* kind_mismatch: payload dropped, the receive completes with
         * MPI_ERR_TYPE */
        if (m.kind_mismatch)
            n = 0;
        if (n > 0 && m.op->strided)
            layout_copy_in(m.op->buf, m.op->layout, d.chunk_off, src_chunk, n);
        else if (n > 0)
            memcpy_auto((char *)m.op->buf + d.chunk_off, src_chunk, n);
    } else {
        if (m.heap.size() < d.chunk_off + d.chunk_bytes)
            m.heap.resize(m.d.msg_bytes);
        if (d.chunk_bytes > 0)
            memcpy(m.heap.data() + d.chunk_off, src_chunk, d.chunk_bytes);
    }
    m.got += d.chunk_bytes;
    if (m.d.msg_bytes == 0) m.got = 0; /* zero-byte msg: single empty chunk */
}

void NativeTransport::finish_host_recv(InboundMsg &m)
{
    if (m.op == nullptr) return; /* stays buffered until a recv posts */
    Op *op = m.op;
    op->ch_status.src = (op->comm_id == 1) ? 0 : m.src;
    op->ch_status.tag = m.d.tag;
    op->ch_status.bytes =
        m.d.msg_bytes <= op->bytes ? m.d.msg_bytes : op->bytes;
    op->ch_status.err =
        m.d.msg_bytes > op->bytes ? MPI_ERR_TRUNCATE : MPI_SUCCESS;
    if (m.kind_mismatch) {
        op->ch_status.bytes = 0;
        op->ch_status.err = MPI_ERR_TYPE;
    }
    op->ch_done.store(1, std::memory_order_release);
    erase_inbound(&m);
}

/* A strided message is served device-to-device (k_pull_strided) or
 * host-to-host (layout_copy_out/in).  Between the two kinds it would take a
 * synchronous copy per run or a kernel dereferencing pageable host memory;
 * instead the receive completes with MPI_ERR_TYPE (and the sender completes:
 * host sends are buffered, device sends are acked by the caller). */
void NativeTransport::fail_kind_mismatch(InboundMsg &m)
{
    if (!m.kind_mismatch)
        MPIX_ERR("strided transfers need both buffers in the same kind of "
                 "memory (device or host): message from rank %d, tag %d "
                 "fails with MPI_ERR_TYPE", m.src, m.d.tag);
    m.kind_mismatch = true;
}

void *NativeTransport::map_remote(const Desc &d)
{
    if (d.flags & DESCF_SELF_PTR) {
        uint64_t p;
        memcpy(&p, d.ipc, 8);
        /* the sender writes offset 0; slice j of an expanded run is at
         * j * part_stride (part_run_slice) */
        return (char *)(uintptr_t)p + d.ipc_off;
    }
    std::string key((const char *)d.ipc, sizeof(hipIpcMemHandle_t));
    auto it = ipc_open_.find(key);
    void *base = nullptr;
    if (it != ipc_open_.end()) {
        base = it->second;
    } else {
        hipIpcMemHandle_t h;
        memcpy(&h, d.ipc, sizeof(h));
        if (hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess) !=
            hipSuccess) {
            MPIX_ERR("hipIpcOpenMemHandle failed (src %d)", d.src_world);
            return nullptr;
        }
        ipc_open_.emplace(std::move(key), base);
    }
    return (char *)base + d.ipc_off;
}

void NativeTransport::start_dev_copy(InboundMsg &m)
{
    Op *op = m.op;
    void *src = map_remote(m.d);
    ChStatus st;
    st.src = (op->comm_id == 1) ? 0 : m.src;
    st.tag = m.d.tag;
    st.bytes = m.d.msg_bytes <= op->bytes ? m.d.msg_bytes : op->bytes;
    st.err = m.d.msg_bytes > op->bytes ? MPI_ERR_TRUNCATE : MPI_SUCCESS;
    if (src == nullptr) {
        st.err = MPI_ERR_OTHER;
        op->ch_status = st;
        op->ch_done.store(1, std::memory_order_release);
        /* still ack so the sender does not hang */
        ack(m.src, m.d.token, m.d.partition, 1);
        erase_inbound(&m);
        return;
    }
    uint64_t n = st.bytes;
    hipError_t e = hipSuccess;
    const bool strided = op->strided || (m.d.flags & DESCF_STRIDED) != 0;
    if (strided && !op->buf_is_device) {
        fail_kind_mismatch(m);
        st.bytes = 0;
        st.err = MPI_ERR_TYPE;
        op->ch_status = st;
        op->ch_done.store(1, std::memory_order_release);
        ack(m.src, m.d.token, m.d.partition, 1);
        erase_inbound(&m);
        return;
    }
    if (strided && n > 0) {
        /* defer: every strided pull that matched in this progress pass goes
         * out in ONE k_pull_strided launch (flush_strided).  n is a multiple
         * of the granule: it is the length of one of the two layouts, and the
         * granule divides the runs of both. */
        uint64_t seen = op->t_issue_ns > m.d.t_seen_ns ? op->t_issue_ns
                                                       : m.d.t_seen_ns;
        PendingStrided ps;
        ps.pp = PendingPull{op, m.src, m.d.token, st, op->buf, src, n, seen,
                            m.d.partition, 1};
        ps.sl = (m.d.flags & DESCF_STRIDED) ? m.d.layout
                                            : layout_contiguous(m.d.msg_bytes);
        ps.dl = op->strided ? op->layout : layout_contiguous(op->bytes);
        pend_strided_.push_back(ps);
        m.dev_copy_started = true;
        erase_inbound(&m);
        return;
    }
    /* The shader pull path requires (a) a device destination — dereferencing
     * a pageable host pointer from a kernel faults on non-XNACK systems —
     * and (b) 16-byte alignment on both sides (user buffers can be
     * arbitrarily offset, e.g. partitioned slices).  Everything else rides
     * hipMemcpyAsync (SDMA / runtime blit). */
    /* pull kernel is deadlock-safe in both copy-stream phases: before the
     * priority switch no spin-wait kernel exists anywhere; after it the
     * copy stream owns its hardware queue (see copy_stream()) */
    bool kernel_ok = op->buf_is_device &&
                     ((((uintptr_t)op->buf) | ((uintptr_t)src)) & 15) == 0;
    if (n > 0 && kernel_ok) {
        /* defer: every pull that matched in this progress pass goes out in
         * ONE k_pull_multi launch (flush_pulls) */
        uint64_t seen = op->t_issue_ns > m.d.t_seen_ns ? op->t_issue_ns
                                                       : m.d.t_seen_ns;
        pend_pulls_.push_back(PendingPull{op, m.src, m.d.token, st,
                                          op->buf, src, n, seen,
                                          m.d.partition, 1});
        m.dev_copy_started = true;
        erase_inbound(&m);
        return;
    }
    hipStream_t cs = copy_stream(n);
    if (n > 0) {
        e = hipMemcpyAsync(op->buf, src, n, hipMemcpyDefault, cs);
    }
    if (e != hipSuccess) {
        MPIX_ERR("hipMemcpyAsync(pull %lu B) failed: %s", (unsigned long)n,
                 hipGetErrorString(e));
        st.err = MPI_ERR_OTHER;
        op->ch_status = st;
        op->ch_done.store(1, std::memory_order_release);
        ack(m.src, m.d.token, m.d.partition, 1);
        erase_inbound(&m);
        return;
    }
    if (trace_on())
        fprintf(stderr, "[mpix trace] pull start %lu B via memcpyAsync "
                "(dst=%p src=%p)\n", (unsigned long)n, op->buf, src);
    hipEvent_t ev = get_event();
    hipError_t erec = hipEventRecord(ev, cs);
    if (erec != hipSuccess)
        MPIX_ERR("hipEventRecord(pull) failed: %s", hipGetErrorString(erec));
    copies_.push_back(CopyInflight{op, ev, m.src, m.d.token, m.d.partition,
                                   st});
    m.dev_copy_started = true;
    erase_inbound(&m);
}

/* Kernel variant knobs, read once; the defaults are the measured winners
 * (profiles/pull_stream_copy.md).  MPIX_PULL_UNROLL = 4 (default) or 8
 * vectors per thread and tile, or 1, which is the access pattern of the
 * earlier kernel.  MPIX_PULL_NT=0 turns the nontemporal loads and stores
 * off: the payload is touched once and is far larger than L2, and keeping
 * it out of the caches is where the gain over the earlier kernel comes
 * from (with plain accesses the tiled kernel is slower than that one). */
static int pull_unroll()
{
    static const int v = [] {
        const char *e = getenv("MPIX_PULL_UNROLL");
        int u = e ? atoi(e) : 4;
        return u == 1 || u == 8 ? u : 4;
    }();
    return v;
}

static bool pull_nontemporal()
{
    static const bool v = [] {
        const char *e = getenv("MPIX_PULL_NT");
        return e ? atoi(e) != 0 : true;
    }();
    return v;
}

template <int U>
static void launch_pull_u(bool nt, unsigned blocks, hipStream_t cs,
                          const PullTable &t, const PullDone *done)
{
    if (done != nullptr) {
        if (nt)
            hipLaunchKernelGGL((k_pull_multi_done<U, true>), dim3(blocks),
                               dim3(PULL_THREADS), 0, cs, t, *done);
        else
            hipLaunchKernelGGL((k_pull_multi_done<U, false>), dim3(blocks),
                               dim3(PULL_THREADS), 0, cs, t, *done);
        return;
    }
    if (nt)
        hipLaunchKernelGGL((k_pull_multi<U, true>), dim3(blocks),
                           dim3(PULL_THREADS), 0, cs, t);
    else
        hipLaunchKernelGGL((k_pull_multi<U, false>), dim3(blocks),
                           dim3(PULL_THREADS), 0, cs, t);
}

void NativeTransport::launch_pull(unsigned blocks, hipStream_t cs,
                                  const PullDone *done)
{
    const bool nt = pull_nontemporal();
    switch (pull_unroll()) {
    case 1: launch_pull_u<1>(nt, blocks, cs, plan_, done); break;
    case 8: launch_pull_u<8>(nt, blocks, cs, plan_, done); break;
    default: launch_pull_u<4>(nt, blocks, cs, plan_, done); break;
    }
}

int NativeTransport::done_begin(PullDone *d)
{
    if (!done_word_) return -1;
    uint64_t seq = 0;
    const int slot = done_acquire(&done_ring_, &seq);
    if (slot < 0) return -1; /* ring full: this batch takes the event path */
    d->counter = done_counters_ + (size_t)slot * DONE_COUNTER_STRIDE;
    d->word = done_words_d_ + (size_t)slot * DONE_WORD_STRIDE;
    d->seq = seq;
    return slot;
}

/* What follows a successful launch: the word path records no event (with
 * MPIX_STATS=1 it does, to measure what the event would have cost). */
void NativeTransport::close_batch(PullBatch &b, hipStream_t cs, int slot,
                                  bool stats)
{
    b.done_slot = slot;
    b.cs = cs;
    if (slot >= 0) b.t_born_ns = now_ns();
    if (slot < 0 || stats) {
        b.ev = get_event();
        (void)hipEventRecord(b.ev, cs);
    }
}

void NativeTransport::flush_pulls()
{
    const bool stats = g_state != nullptr && g_state->stats;
    const uint64_t tile_bytes = (uint64_t)PULL_THREADS * pull_unroll() * 16;
    while (!pend_pulls_.empty()) {
        PullSeg segs[MPIX_PULL_BATCH];
        size_t n = pend_pulls_.size();
        if (n > MPIX_PULL_BATCH) n = MPIX_PULL_BATCH;
        uint64_t total = 0;
        uint64_t t_first = UINT64_MAX;
        for (size_t i = 0; i < n; i++) {
            const PendingPull &pp = pend_pulls_[i];
            segs[i] = PullSeg{pp.dst, pp.csrc, pp.n};
            total += pp.n;
            if (pp.t_seen_ns < t_first) t_first = pp.t_seen_ns;
        }
        plan_pulls(segs, n, tile_bytes, &plan_);
        hipStream_t cs = copy_stream(total);
        static const unsigned max_blocks = [] {
            const char *e = getenv("MPIX_PULL_BLOCKS");
            /* cap on blocks; A/B in profiles/pull_stream_copy.md */
            return e && atoi(e) > 0 ? (unsigned)atoi(e) : 1024u;
        }();
        uint64_t tiles = pull_total_tiles(plan_);
        unsigned blocks = tiles < max_blocks ? (unsigned)tiles : max_blocks;
        PullDone done;
        const int slot = done_begin(&done);
        const uint64_t t_call = stats ? now_ns() : 0;
        launch_pull(blocks, cs, slot >= 0 ? &done : nullptr);
        hipError_t e = hipGetLastError();
        const uint64_t t_rec = stats ? now_ns() : 0;
        if (e != hipSuccess) {
            MPIX_ERR("k_pull_multi launch failed: %s", hipGetErrorString(e));
            if (slot >= 0) done_release(&done_ring_, slot);
            for (size_t i = 0; i < n; i++) {
                pend_pulls_[i].st.err = MPI_ERR_OTHER;
                finish_pull(pend_pulls_[i], nullptr);
            }
            pend_pulls_.erase(pend_pulls_.begin(), pend_pulls_.begin() + n);
            continue;
        }
        PullBatch b;
        close_batch(b, cs, slot, stats);
        if (stats) {
            State *s = g_state;
            b.t_launch_ns = now_ns();
            const uint64_t call = t_rec - t_call;
            if (!s->bleg_first_seen) {
                /* loads the code object: reported apart from the means */
                s->bleg_first_seen = b.first = true;
                s->bleg_first_wait_ns = b.t_launch_ns - t_first;
                s->bleg_first_call_ns = call;
                s->bleg_first_rec_ns = b.t_launch_ns - t_rec;
                s->bleg_first_items = pull_ops(pend_pulls_, n);
            } else {
                s->bleg_wait_ns += b.t_launch_ns - t_first;
                s->bleg_call_ns += call;
                if (call < s->bleg_call_min_ns) s->bleg_call_min_ns = call;
                if (call > s->bleg_call_max_ns) s->bleg_call_max_ns = call;
                s->bleg_rec_ns += b.t_launch_ns - t_rec;
                s->bleg_n++;
                s->bleg_items += pull_ops(pend_pulls_, n);
                s->bleg_copies += plan_.ncopies;
            }
        }
        b.items.assign(pend_pulls_.begin(), pend_pulls_.begin() + n);
        pend_pulls_.erase(pend_pulls_.begin(), pend_pulls_.begin() + n);
        batches_.push_back(std::move(b));
        if (trace_on())
            fprintf(stderr, "[mpix trace] pull batch n=%zu copies=%u "
                    "tiles=%lu total=%lu B\n", n, plan_.ncopies,
                    (unsigned long)tiles, (unsigned long)total);
    }
}

void NativeTransport::flush_strided()
{
    while (!pend_strided_.empty()) {
        StridedSeg segs[MPIX_STRIDED_BATCH];
        size_t n = pend_strided_.size();
        if (n > MPIX_STRIDED_BATCH) n = MPIX_STRIDED_BATCH;
        uint64_t total = 0;
        for (size_t i = 0; i < n; i++) {
            const PendingStrided &ps = pend_strided_[i];
            segs[i] = StridedSeg{ps.pp.dst, ps.pp.csrc, ps.pp.n, ps.sl, ps.dl};
            if (ps.parts) {
                segs[i].parts = ps.pp.k;
                segs[i].s_part_stride = ps.s_part_stride;
                segs[i].d_part_stride = ps.d_part_stride;
            }
            total += ps.pp.n;
        }
        plan_strided(segs, n, strided_div64_, &splan_);
        /* same stream choice as flush_pulls: a contiguous batch of this
         * pass and this launch go back to back on the copy stream */
        hipStream_t cs = copy_stream(total);
        uint64_t tiles = strided_total_tiles(splan_);
        unsigned blocks = tiles < 1024 ? (unsigned)tiles : 1024u;
        const bool wide = strided_plan_wide(splan_);
        const bool parts = strided_plan_parts(splan_);
        PullDone done;
        const int slot = done_begin(&done);
#define MPIX_LAUNCH_STRIDED(W, P)                                            \
        do {                                                                  \
            if (slot >= 0)                                                    \
                hipLaunchKernelGGL((k_pull_strided_done<W, P>), dim3(blocks), \
                                   dim3(PULL_THREADS), 0, cs, splan_, done);  \
            else                                                              \
                hipLaunchKernelGGL((k_pull_strided<W, P>), dim3(blocks),      \
                                   dim3(PULL_THREADS), 0, cs, splan_);        \
        } while (0)
        if (wide && parts)
            MPIX_LAUNCH_STRIDED(true, true);
        else if (wide)
            MPIX_LAUNCH_STRIDED(true, false);
        else if (parts)
            MPIX_LAUNCH_STRIDED(false, true);
        else
            MPIX_LAUNCH_STRIDED(false, false);
#undef MPIX_LAUNCH_STRIDED
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            MPIX_ERR("k_pull_strided launch failed: %s", hipGetErrorString(e));
            if (slot >= 0) done_release(&done_ring_, slot);
            for (size_t i = 0; i < n; i++) {
                pend_strided_[i].pp.st.err = MPI_ERR_OTHER;
                finish_pull(pend_strided_[i].pp, nullptr);
            }
            pend_strided_.erase(pend_strided_.begin(),
                                pend_strided_.begin() + n);
            continue;
        }
        PullBatch b; /* t_launch_ns stays 0: the batch legs of MPIX_STATS
                        count plain pulls */
        close_batch(b, cs, slot, g_state != nullptr && g_state->stats);
        for (size_t i = 0; i < n; i++) b.items.push_back(pend_strided_[i].pp);
        pend_strided_.erase(pend_strided_.begin(), pend_strided_.begin() + n);
        batches_.push_back(std::move(b));
        if (trace_on())
            fprintf(stderr, "[mpix trace] strided pull batch n=%zu tiles=%lu "
                    "total=%lu B wide=%d parts=%d\n", n, (unsigned long)tiles,
                    (unsigned long)total, (int)wide, (int)parts);
    }
}

/* Is the batch's kernel finished?  *err: hipSuccess, or why its ops fail.
 * Event path: hipEventQuery.  Word path: a plain acquire load of the slot's
 * host word, no runtime call.  A kernel that dies never stores its word, so
 * for a batch older than a second the stream is asked, once per 4096 passes
 * that found no word: an error there fails the batch (reasoned, not
 * exercised: nothing in the tests makes a kernel fail). */
bool NativeTransport::batch_done(PullBatch &b, hipError_t *err)
{
    *err = hipSuccess;
    if (b.done_slot < 0) {
        hipError_t e = hipEventQuery(b.ev);
        if (e == hipErrorNotReady) return false;
        *err = e;
        put_event(b.ev);
        b.ev = nullptr;
        return true;
    }
    const uint64_t w =
        done_words_[(size_t)b.done_slot * DONE_WORD_STRIDE].load(
            std::memory_order_acquire);
    if (!done_seen(&done_ring_, b.done_slot, w)) {
        if ((++b.passes & 4095u) != 0 ||
            now_ns() - b.t_born_ns < 1000000000ull)
            return false;
        hipError_t e = hipStreamQuery(b.cs);
        if (e == hipSuccess || e == hipErrorNotReady) return false;
        MPIX_ERR("pull kernel lost (no completion word after %.1f s): %s",
                 (double)(now_ns() - b.t_born_ns) / 1e9, hipGetErrorString(e));
        *err = e;
    }
    done_release(&done_ring_, b.done_slot);
    b.done_slot = -1;
    if (b.ev != nullptr) {
        /* MPIX_STATS=1: how long after the word does the event follow? */
        word_events_.push_back(WordEvent{b.ev, now_ns()});
        b.ev = nullptr;
    }
    return true;
}

int NativeTransport::progress_copies()
{
    for (auto it = word_events_.begin(); it != word_events_.end();) {
        if (hipEventQuery(it->ev) == hipErrorNotReady) {
            ++it;
            continue;
        }
        g_state->word_event_ns += now_ns() - it->t_word_ns;
        g_state->word_event_n++;
        put_event(it->ev);
        it = word_events_.erase(it);
    }
    for (auto it = batches_.begin(); it != batches_.end();) {
        hipError_t e;
        if (!batch_done(*it, &e)) {
            ++it;
            continue;
        }
        BatchStat *bs = nullptr;
        if (it->t_launch_ns) {
            bs = new BatchStat{now_ns(),
                               (int)pull_ops(it->items, it->items.size()),
                               it->first};
            if (it->first)
                g_state->bleg_first_kernel_ns = bs->t_ev_ns - it->t_launch_ns;
            else
                g_state->bleg_kernel_ns += bs->t_ev_ns - it->t_launch_ns;
            /* a batch that is one whole request: its launch -> event is
             * comparable with the kernel's traced duration */
            const PendingPull &p0 = it->items.front();
            if (!it->first && it->items.size() == 1 && p0.k > 1 &&
                p0.op->req != nullptr &&
                (int)p0.k == p0.op->req->n_partitions)
                g_state->bleg_whole_ns.push_back(
                    (uint32_t)(bs->t_ev_ns - it->t_launch_ns));
        }
        for (PendingPull &pp : it->items) {
            if (e != hipSuccess) pp.st.err = MPI_ERR_OTHER;
            finish_pull(pp, bs);
        }
        it = batches_.erase(it);
    }
    for (auto it = copies_.begin(); it != copies_.end();) {
        hipError_t e = hipEventQuery(it->ev);
        if (e == hipErrorNotReady) {
            ++it;
            continue;
        }
        if (e != hipSuccess) it->st.err = MPI_ERR_OTHER;
        if (trace_on())
            fprintf(stderr, "[mpix trace] pull done (e=%d)\n", (int)e);
        put_event(it->ev);
        /* ack the sender, then complete the recv */
        ack(it->src, it->token, it->partition, 1);
        it->op->ch_status = it->st;
        it->op->ch_done.store(1, std::memory_order_release);
        it = copies_.erase(it);
    }
    return 0;
}

void NativeTransport::erase_inbound(InboundMsg *m)
{
    /* erase the token mapping only if it still points at THIS message — a
     * later message may have legitimately reused the slot-index token */
    auto it = inbound_by_token_.find(((uint64_t)m->src << 32) ^ m->d.token);
    if (it != inbound_by_token_.end() && it->second == m)
        inbound_by_token_.erase(it);
    for (auto it = inbound_.begin(); it != inbound_.end(); ++it) {
        if (&*it == m) {
            inbound_.erase(it);
            return;
        }
    }
}

int NativeTransport::memcpy_auto(void *dst, const void *src, size_t n)
{
    if (!have_gpu_) {
        memcpy(dst, src, n);
        return 0;
    }
    /* hipMemcpyDefault resolves host/device direction via unified addressing;
     * plain memcpy when both sides are host saves the runtime call.
     * Device copies MUST ride the proxy-private non-blocking stream: a
     * synchronous hipMemcpy runs on the legacy NULL stream, which
     * serializes against every blocking user stream — including one parked
     * on hipStreamWaitValue32 waiting for THIS proxy to make progress
     * (deadlock observed with MPIX_DEV_PUSH_MAX; the reference documents
     * the same hazard class, README.md:140-150). */
    bool dd = ptr_is_device(dst);
    if (!dd && !ptr_is_device(src)) {
        memcpy(dst, src, n);
        return 0;
    }
    hipStream_t cs = copy_stream0();
    if (hipMemcpyAsync(dst, src, n, hipMemcpyDefault, cs) != hipSuccess)
        return -1;
    return hipStreamSynchronize(cs) == hipSuccess ? 0 : -1;
}

/* ----------------------------------------------------------------- factory */

Transport *make_native_transport(int world_rank, int world_size, bool mpi_mode,
                                 bool have_gpu, int device_id)
{
    auto *t = new NativeTransport(world_rank, world_size, mpi_mode, have_gpu,
                                  device_id);
    if (t->init() != 0) {
        delete t;
        return nullptr;
    }
    return t;
}

void native_transport_shutdown(Transport *t)
{
    static_cast<NativeTransport *>(t)->shutdown();
}

} /* namespace mpix */
