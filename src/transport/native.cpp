/* mpix — native intra-node data plane: shared-memory control + xGMI data.
 *
 * The reference delegates all data movement to a CUDA-aware host MPI
 * (SURVEY.md §2b).  On an MI355X node the fast path between GPUs is direct
 * peer-to-peer over xGMI, so this transport implements tag-matched
 * point-to-point natively:
 *
 *  control plane  per ordered rank pair (s -> r), an SPSC descriptor ring in
 *                 a POSIX shm segment owned by r, plus a chunked staging
 *                 buffer for host payloads (shm_ring.h).
 *  device data    sender publishes {hipIpcMemHandle, offset}; the RECEIVER
 *                 pulls over xGMI on its one private copy stream and acks
 *                 with a DONE descriptor: one copy kernel per progress pass
 *                 (pull_kernels.h), or hipMemcpyAsync as a batch of one for
 *                 a misaligned side or a host destination.  Same-process /
 *                 same-rank transfers skip IPC and use the raw pointer.
 *                 Consecutive partitions of one request go out as a RUN:
 *                 one descriptor, one pull, one DONE per acked range
 *                 (part_run.h); an ack to ourselves skips the ring.
 *                 A REDUCING receive (Op::reduce) combines the message into
 *                 its buffer inside the pull: k_pull_reduce, planned by
 *                 reduce_plan.h, the combine defined by reduce.h; host
 *                 buffers combine chunk by chunk (reduce_host).  One that is
 *                 strided on either side (the strided reducing calls) is an
 *                 entry of k_pull_strided_reduce, planned by
 *                 strided_reduce_plan.h; host buffers combine run by run
 *                 (layout_reduce_in).
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
#include "pull_kernels.h"
#include "pull_plan.h"
#include "reduce.h"
#include "reduce_plan.h"
#include "shm_ring.h"
#include "strided_plan.h"
#include "strided_reduce_plan.h"

namespace mpix {

/* ------------------------------------------------- knobs, each read once */

/* a number; unset reads as `dflt` */
static uint64_t env_u64(const char *name, uint64_t dflt)
{
    const char *e = getenv(name);
    return e ? (uint64_t)atoll(e) : dflt;
}

static bool env_flag(const char *name) { return env_u64(name, 0) != 0; }

/* MPIX_TRACE=1 (as in proxy.cpp) */
static bool trace_on()
{
    static const bool v = env_flag("MPIX_TRACE");
    return v;
}

/* Sender-push threshold for small DEVICE payloads: stage D2H into the shm
 * chunk ring like a host message (receiver H2D's it out), skipping the
 * NOTIFY/pull/ACK round trip.  Measured WORSE (74-97 us vs ~38 us half-RTT:
 * the two proxy-synchronous staging copies cost more than the round trip
 * they remove — profiles/r02_pingpong_devpush.json); kept off, tunable for
 * experiments with MPIX_DEV_PUSH_MAX=<bytes>. */
static uint64_t dev_push_max()
{
    static const uint64_t v = env_u64("MPIX_DEV_PUSH_MAX", 0);
    return v;
}

/* MPIX_PART_RUNS=0: the sender announces every partition with a descriptor
 * of its own (runs of length 1 only), as before part_run.h.  An A/B inside
 * one build, and the way tests drive both protocols. */
static bool part_runs_on()
{
    static const bool v = env_u64("MPIX_PART_RUNS", 1) != 0;
    return v;
}

/* MPIX_PULL_DONE=word|tail|event: how a pull batch's completion reaches
 * the proxy.
 *  word   (default) the copy kernel stores its payload write-through (sc1)
 *         and its last block stores a sequence number to pinned host memory
 *         (done_ring.h, pull_signal_done); no event, no runtime call per
 *         pass.  hipMemcpyAsync pulls complete by event.
 *  tail   the event path's kernel (or the hipMemcpyAsync), and a one-thread
 *         kernel behind it on the stream that stores the sequence number.
 *  event  an event recorded behind the launch and tested with hipEventQuery
 *         in every pass.
 * None of them waits on the device.  A/B: profiles/pull_done_modes.md. */
enum class PullDoneMode { EVENT, WORD, TAIL };
static const char *const PULL_DONE_DEFAULT = "word";

static PullDoneMode pull_done_mode()
{
    static const PullDoneMode v = [] {
        const char *e = getenv("MPIX_PULL_DONE");
        if (e == nullptr) e = PULL_DONE_DEFAULT;
        if (strcmp(e, "word") == 0) return PullDoneMode::WORD;
        if (strcmp(e, "tail") == 0) return PullDoneMode::TAIL;
        if (strcmp(e, "event") != 0)
            MPIX_ERR("MPIX_PULL_DONE=%s is none of word, tail, event: event",
                     e);
        return PullDoneMode::EVENT;
    }();
    return v;
}

/* Kernel variant knobs; the defaults are the measured winners
 * (profiles/pull_stream_copy.md).  MPIX_PULL_UNROLL = 4 (default) or 8
 * vectors per thread and tile, or 1, which is the access pattern of the
 * earlier kernel.  MPIX_PULL_NT=0 turns the nontemporal loads and stores
 * off: the payload is touched once and is far larger than L2, and keeping
 * it out of the caches is where the gain over the earlier kernel comes
 * from (with plain accesses the tiled kernel is slower than that one); it
 * applies to the kernels of MPIX_PULL_DONE=event and tail, the word kernels
 * always load nontemporal and store write-through.
 * MPIX_PULL_BLOCKS caps the blocks of a launch (A/B in the same profile). */
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
    static const bool v = env_u64("MPIX_PULL_NT", 1) != 0;
    return v;
}

static unsigned pull_max_blocks()
{
    static const int v = (int)env_u64("MPIX_PULL_BLOCKS", 1024);
    return v > 0 ? (unsigned)v : 1024u;
}

/* ---------------------------------------------- receive-side completion */

/* everything of the envelope but the partitioned kind and number */
static bool envelope_match(const Op *op, uint32_t comm_id, int src, int tag)
{
    return op->comm_id == comm_id &&
           (op->peer_world == MPI_ANY_SOURCE || op->peer_world == src) &&
           (op->tag == MPI_ANY_TAG || op->tag == tag);
}

/* What receive `op` reports for a message of msg_bytes from world rank `src`:
 * on SELF the source is rank 0; a longer message is cut and truncated. */
static ChStatus recv_status(const Op *op, int src, int tag, uint64_t msg_bytes)
{
    ChStatus st;
    st.src = (op->comm_id == 1) ? 0 : src;
    st.tag = tag;
    st.bytes = msg_bytes <= op->bytes ? msg_bytes : op->bytes;
    st.err = msg_bytes > op->bytes ? MPI_ERR_TRUNCATE : MPI_SUCCESS;
    return st;
}

static void complete_recv(Op *op, const ChStatus &st)
{
    op->ch_status = st;
    op->ch_done.store(1, std::memory_order_release);
}

/* MPIX_STATS=1: the moment both sides of a pull had been seen PENDING */
static uint64_t seen_ns(const Op *op, const Desc &d)
{
    return op->t_issue_ns > d.t_seen_ns ? op->t_issue_ns : d.t_seen_ns;
}

/* -------------------------------------------------------------- transport */

class NativeTransport : public Transport {
public:
    NativeTransport(int rank, int size, bool mpi_mode, bool have_gpu, int dev)
        : rank_(rank), size_(size), have_gpu_(have_gpu), dev_(dev),
          mpi_mode_(mpi_mode) {}

    int init();
    void shutdown(); /* called from MPIX_Finalize before dtor */
    ~NativeTransport() override { shutdown(); }

    int start(Op *op) override;
    void progress() override;
    const char *name() const override { return "native-shm-xgmi"; }

private:
    /* ---- send side ---- */
    struct SendState {
        Op *op;
        uint64_t staged = 0;   /* bytes staged so far (host path) */
    };
    /* per-destination FIFO queues (preserves non-overtaking) */
    std::map<int, std::deque<SendState>> sendq_;
    /* device sends awaiting DONE: token (slot of the first op) -> the op,
     * or the run of partitions announced under that token */
    struct AwaitDone {
        Op *op;       /* first (or only) op */
        Request *req; /* owner of a run (k > 1), else unused */
        RunAwait run;
        Op *send_op(int32_t partition) const { /* the send of a partition */
            return run.k == 1 ? op : &g_state->ops[req->part_idx[partition]];
        }
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
        bool kind_mismatch = false; /* payload dropped, MPI_ERR_TYPE: strided
                                       msg between host and device, or one
                                       a reducing receive cannot combine */
    };
    std::list<InboundMsg> inbound_;                 /* arrival order */
    std::unordered_map<uint64_t, InboundMsg *> inbound_by_token_;
    std::vector<Op *> posted_recvs_;                /* post order */

    /* One pull.  Kernel pulls are collected over a progress pass and flushed
     * as ONE launch; a hipMemcpyAsync pull is a batch of its own. */
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
    static size_t pull_ops(const std::vector<PendingPull> &v) {
        size_t ops = 0;
        for (const PendingPull &pp : v) ops += pp.k;
        return ops;
    }
    void finish_pull(const PendingPull &pp, BatchStat *bs);
    std::vector<PendingPull> pend_pulls_;
    /* what is in flight on a copy stream, in submission order */
    struct PullBatch {
        hipEvent_t ev = nullptr; /* event path; word paths: only MPIX_STATS=1 */
        int done_slot = -1;   /* word paths: slot of done_ring_, else -1 */
        hipStream_t cs = nullptr;
        uint64_t t_born_ns = 0;  /* word paths: for the lost-signal guard */
        uint32_t passes = 0;     /* word paths: passes that found no word */
        uint64_t t_launch_ns = 0; /* MPIX_STATS=1, contiguous kernel batches */
        bool first = false;   /* MPIX_STATS=1: first batch of the process */
        bool memcpy_pull = false; /* hipMemcpyAsync, not a kernel */
        std::vector<PendingPull> items;
    };
    std::list<PullBatch> batches_;
    /* MPIX_PULL_DONE=word, tail (the word paths): completion words
     * in pinned host memory, one per 64 bytes, and arrival counters in
     * device memory, one per 128 bytes, which tail leaves alone (done_ring.h
     * has the bookkeeping) */
    static constexpr size_t DONE_WORD_STRIDE = 8;     /* in uint64_t */
    static constexpr size_t DONE_COUNTER_STRIDE = 32; /* in uint32_t */
    PullDoneMode done_mode_ = PullDoneMode::EVENT; /* EVENT: no words */
    DoneRing done_ring_;
    std::atomic<uint64_t> *done_words_ = nullptr; /* host view */
    uint64_t *done_words_d_ = nullptr;            /* device view */
    uint32_t *done_counters_ = nullptr;
    /* MPIX_STATS=1 on a word path: the event recorded all the same, kept
     * after the word was seen to measure word seen -> event seen */
    struct WordEvent {
        hipEvent_t ev;
        uint64_t t_word_ns;
    };
    std::list<WordEvent> word_events_;
    bool batch_done(PullBatch &b, hipError_t *err);
    PullBatch &push_batch(std::vector<PendingPull> items, hipStream_t cs,
                          int slot);
    int acquire_done(PullDone *done);
    int signal_by_tail(int slot, const PullDone &done, hipStream_t cs);
    template <typename Launch>
    PullBatch *submit_batch(std::vector<PendingPull> items, hipStream_t cs,
                            const char *kernel, Launch launch);
    PullTable plan_{}; /* scratch of flush_pulls; passed by value */

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

    /* reducing pulls (Op::reduce) collected this progress pass: k_pull_reduce
     * launches of up to MPIX_PULL_BATCH of them, cut where destinations
     * overlap (reduce_plan.h), completed through batches_ like the others.
     * They all go to the copy stream itself, so launches with overlapping
     * destinations run one after the other. */
    struct PendingReduce {
        PendingPull pp;
        uint32_t type, op;
    };
    std::vector<PendingReduce> pend_reduce_;
    ReduceTable rplan_{}; /* scratch of flush_reduce; passed by value */
    hipStream_t reduce_cs_ = nullptr; /* stream of the last reduce launch */
    hipStream_t reduce_stream();

    /* reducing pulls that are strided on either side (receives made by the
     * strided reducing calls): k_pull_strided_reduce launches of up to
     * MPIX_STRIDED_BATCH of them, cut where destination extents overlap
     * (strided_reduce_plan.h), on the stream of the contiguous reducing
     * launches and behind them */
    struct PendingStridedReduce {
        PendingStrided ps;
        uint32_t type, op;
    };
    std::vector<PendingStridedReduce> pend_sreduce_;
    StridedReduceTable srplan_{}; /* scratch of flush_strided_reduce */

    /* ---- shm ---- */
    ShmGeom geom_{};
    void *map_segment(const char *name, bool create);
    std::vector<void *> seg_;       /* seg_[r] = rank r's segment base */
    std::vector<uint64_t> out_head_; /* producer-local head per dst */
    std::vector<uint64_t> out_stage_head_; /* producer-local chunk cursor */
    std::vector<uint64_t> in_tail_;  /* consumer-local tail per src */

    /* ---- hip ---- */
    /* ONE plain copy stream carries every pull and the synchronous staging
     * copies (memcpy_auto); it is upgraded to greatest priority, lazily, once
     * a spin-wait kernel was ever emitted (maybe_switch_prio).  Batched
     * pulls serialize on it at HBM rate, and there are NO standing extra
     * streams: each extra hardware queue, even another process's, adds tens
     * of us to every wait on the device (36.5 -> ~55 us 2-process half-RTT).
     * copy_big_ (MPIX_COPY_PRIO_STREAM=1) is the experiment that opts one
     * back in, for batches above MPIX_COPY_POOL_MIN bytes. */
    hipStream_t copy_stream_ = nullptr;
    hipStream_t copy_retired_ = nullptr; /* the plain stream after the switch,
                                            kept alive for what is on it */
    hipStream_t copy_big_ = nullptr;
    bool prio_switched_ = false;
    /* a new greatest-priority stream, or nullptr */
    static hipStream_t prio_stream() {
        int lo = 0, hi = 0;
        hipStream_t ps = nullptr;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess &&
            hi != lo &&
            hipStreamCreateWithPriority(&ps, hipStreamNonBlocking, hi) ==
                hipSuccess)
            return ps;
        (void)hipGetLastError();
        return nullptr;
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
        if (hipStream_t ps = prio_stream()) {
            copy_retired_ = copy_stream_;
            copy_stream_ = ps;
        }
    }
    /* stream for `bytes` of copy: the copy stream (ordering per message is
     * by what is recorded on the same stream as its copy) */
    hipStream_t copy_stream(uint64_t bytes) {
        static const uint64_t pool_min =
            env_u64("MPIX_COPY_POOL_MIN", 256 << 10);
        maybe_switch_prio();
        return bytes > pool_min && copy_big_ ? copy_big_ : copy_stream_;
    }
    std::vector<hipEvent_t> event_pool_;
    std::unordered_map<std::string, void *> ipc_open_;   /* handle -> ptr */
    std::unordered_map<const void *, hipIpcMemHandle_t> ipc_get_; /* by base */

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
        return mpix::ring_has_space(out_box(dst), geom_, out_head_[dst], need);
    }
    void emit_desc(int dst, const Desc &d) {
        ring_emit(out_box(dst), geom_, &out_head_[dst], d);
    }

    hipEvent_t get_event() {
        hipEvent_t ev = nullptr;
        if (event_pool_.empty()) {
            (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        } else {
            ev = event_pool_.back();
            event_pool_.pop_back();
        }
        return ev;
    }
    void put_event(hipEvent_t ev) { event_pool_.push_back(ev); }

    void progress_sends();
    void drain_inbox(int src);
    void progress_copies();
    void flush_pulls();
    void flush_strided();
    void flush_reduce();
    void flush_strided_reduce();
    void fail_kind_mismatch(InboundMsg &m);
    const char *reduce_reject(const InboundMsg &m, const void *src) const;
    void handle_desc(int src, const Desc &d, const char *stage_base);
    bool try_run_fast_path(int src, const Desc &d, uint32_t k);
    Desc desc_for(const Op *op, DescType type) const;
    bool emit_done(int dst, uint64_t token, int32_t first, uint32_t count);
    void ack(int src, uint64_t token, int32_t first, uint32_t count);
    void handle_done(uint64_t token, int32_t first, uint32_t count);
    void try_match_new_inbound(InboundMsg &m);
    void attach(InboundMsg &m, Op *op);
    void start_dev_copy(InboundMsg &m);
    void fail_dev_recv(InboundMsg &m, const ChStatus &st);
    void finish_host_recv(InboundMsg &m);
    void deliver_chunk(InboundMsg &m, const Desc &d, const char *src_chunk);
    void erase_inbound(InboundMsg *m);
    int memcpy_auto(void *dst, const void *src, size_t n);
    void *map_remote(const Desc &d);
    bool match(const Op *op, const Desc &d, int src) const;
    void complete_send_buffered(Op *op);
};

/* ------------------------------------------------------------------- init */

/* Map segment `name`; create: make it first (ours), and zero it. */
void *NativeTransport::map_segment(const char *name, bool create)
{
    int fd = shm_open(name, create ? O_CREAT | O_EXCL | O_RDWR : O_RDWR, 0600);
    if (fd < 0) {
        MPIX_ERR("shm_open(%s) failed", name);
        return nullptr;
    }
    if (create && ftruncate(fd, (off_t)geom_.segment_bytes) != 0) {
        MPIX_ERR("ftruncate(%zu) failed", geom_.segment_bytes);
        close(fd);
        return nullptr;
    }
    void *base = mmap(nullptr, geom_.segment_bytes, PROT_READ | PROT_WRITE,
                      MAP_SHARED, fd, 0);
    close(fd);
    if (base == MAP_FAILED) {
        MPIX_ERR("mmap(%s) failed", name);
        return nullptr;
    }
    if (create) memset(base, 0, geom_.segment_bytes);
    return base;
}

int NativeTransport::init()
{
    boot_ = make_bootstrap(rank_, size_, mpi_mode_);
    if (!boot_) return -1;

    geom_ = shm_geometry(
        size_, (uint32_t)env_u64("MPIX_SHM_RING", RING_SLOTS_DEFAULT),
        (uint32_t)env_u64("MPIX_SHM_STAGE_CHUNKS", STAGE_CHUNKS_DEFAULT));

    /* create my segment */
    struct Blob { char name[96]; };
    Blob mine{};
    unsigned seed = (unsigned)getpid() * 2654435761u + (unsigned)rank_;
    snprintf(mine.name, sizeof(mine.name), "/mpix-r%d-%d-%x", rank_,
             (int)getpid(), rand_r(&seed));
    void *base = map_segment(mine.name, true);
    if (base == nullptr) return -1;

    /* exchange names, open peers */
    std::vector<Blob> all(size_);
    if (boot_->allgather(&mine, all.data(), sizeof(Blob)) != 0) {
        MPIX_ERR("bootstrap allgather failed");
        return -1;
    }
    seg_.assign(size_, nullptr);
    seg_[rank_] = base;
    for (int r = 0; r < size_; r++) {
        if (r == rank_) continue;
        seg_[r] = map_segment(all[r].name, false);
        if (seg_[r] == nullptr) return -1;
    }
    /* everyone mapped everything -> segments can be unlinked */
    boot_->barrier();
    shm_unlink(mine.name);

    out_head_.assign(size_, 0);
    out_stage_head_.assign(size_, 0);
    in_tail_.assign(size_, 0);

    strided_div64_ = env_flag("MPIX_STRIDED_DIV64");

    if (have_gpu_) {
        if (hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking) !=
            hipSuccess) {
            MPIX_ERR("copy stream create failed");
            return -1;
        }
        if (pull_done_mode() != PullDoneMode::EVENT) {
            void *w = nullptr, *wd = nullptr, *c = nullptr;
            const size_t wbytes =
                MPIX_DONE_SLOTS * DONE_WORD_STRIDE * sizeof(uint64_t);
            const size_t cbytes =
                MPIX_DONE_SLOTS * DONE_COUNTER_STRIDE * sizeof(uint32_t);
            if (hipHostMalloc(&w, wbytes, hipHostMallocMapped) != hipSuccess ||
                hipHostGetDevicePointer(&wd, w, 0) != hipSuccess ||
                hipMalloc(&c, cbytes) != hipSuccess ||
                hipMemset(c, 0, cbytes) != hipSuccess) {
                MPIX_ERR("MPIX_PULL_DONE: completion words not allocated");
                return -1;
            }
            memset(w, 0, wbytes);
            done_words_ = reinterpret_cast<std::atomic<uint64_t> *>(w);
            done_words_d_ = (uint64_t *)wd;
            done_counters_ = (uint32_t *)c;
            done_mode_ = pull_done_mode();
            if (g_state != nullptr) {
                const char *e = getenv("MPIX_PULL_DONE");
                snprintf(g_state->pull_done_name,
                         sizeof(g_state->pull_done_name), "%s",
                         e ? e : PULL_DONE_DEFAULT);
            }
        }
        /* the standing priority stream, for experiments only */
        if (env_flag("MPIX_COPY_PRIO_STREAM")) copy_big_ = prio_stream();
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
    done_mode_ = PullDoneMode::EVENT;
    reduce_cs_ = nullptr;
    for (hipStream_t *s : {&copy_stream_, &copy_big_, &copy_retired_}) {
        if (*s) (void)hipStreamDestroy(*s);
        *s = nullptr;
    }
    for (int r = 0; r < (int)seg_.size(); r++)
        if (seg_[r]) munmap(seg_[r], geom_.segment_bytes);
    seg_.clear();
    delete boot_;
    boot_ = nullptr;
}

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
    const bool want_part = (op->kind == OpKind::PRECV_PART);
    const bool is_part = (d.flags & DESCF_PARTITIONED) != 0;
    return want_part == is_part &&
           (!want_part || op->partition == d.partition) &&
           envelope_match(op, d.comm_id, src, d.tag);
}

/* ---------------------------------------------------------------- progress */

void NativeTransport::progress()
{
    progress_sends();
    for (int s = 0; s < size_; s++) drain_inbox(s);
    flush_pulls();
    flush_strided();
    flush_reduce();
    flush_strided_reduce();
    progress_copies();

    /* retry queued DONE acks */
    for (size_t i = 0; i < pending_done_.size();) {
        const PendingDone pd = pending_done_[i];
        if (emit_done(pd.dst, pd.token, pd.first, pd.count))
            pending_done_.erase(pending_done_.begin() + i);
        else
            i++;
    }
}

void NativeTransport::complete_send_buffered(Op *op)
{
    op->ch_status = ChStatus{(op->comm_id == 1) ? 0 : rank_, op->tag,
                             op->bytes, MPI_SUCCESS};
    op->ch_done.store(1, std::memory_order_release);
}

/* what a DEV_NOTIFY and a HOST_CHUNK of `op` have in common */
Desc NativeTransport::desc_for(const Op *op, DescType type) const
{
    Desc d;
    d.type = type;
    d.flags = (op->kind == OpKind::PSEND_PART) ? DESCF_PARTITIONED : 0;
    d.token = (uint64_t)(op - g_state->ops);
    d.src_world = rank_;
    d.tag = op->tag;
    d.comm_id = op->comm_id;
    d.partition = op->partition;
    d.msg_bytes = op->bytes;
    return d;
}

void NativeTransport::progress_sends()
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
                Desc d = desc_for(op, DESC_DEV_NOTIFY);
                d.count = (uint32_t)k;
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
                        it = ipc_get_.emplace(base, h).first;
                    }
                    memcpy(d.ipc, &it->second, sizeof(hipIpcMemHandle_t));
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
                InboxView v = out_box(dst);
                if (!ring_has_space(dst, 1) ||
                    stage_free_chunks(v, geom_, out_stage_head_[dst]) == 0) {
                    stalled = true;
                    break;
                }
                uint64_t chunk_idx = out_stage_head_[dst] % geom_.stage_chunks;
                uint64_t n = op->bytes - ss.staged;
                if (n > CHUNK_BYTES) n = CHUNK_BYTES;
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
                Desc d = desc_for(op, DESC_HOST_CHUNK);
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
}

void NativeTransport::drain_inbox(int src)
{
    InboxView v = my_inbox(src);
    const uint64_t head = ring_head(v);
    int budget = 64;
    while (in_tail_[src] < head && budget-- > 0) {
        handle_desc(src, ring_front(v, geom_, in_tail_[src]), v.stage);
        ring_pop(v, &in_tail_[src]);
    }
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
        stage_release(my_inbox(src));
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
    for (uint32_t j = 0; j < count; j++) /* a single message: count is 1 */
        complete_send_buffered(a.send_op(first + (int32_t)j));
    if (r == RUN_ACK_LAST) await_done_.erase(it);
}

/* A DONE for rank `dst` through the ring; false: no slot free, nothing sent */
bool NativeTransport::emit_done(int dst, uint64_t token, int32_t first,
                                uint32_t count)
{
    if (!ring_has_space(dst, 1)) return false;
    Desc d;
    d.type = DESC_DONE;
    d.token = token;
    d.src_world = rank_;
    d.partition = first;
    d.count = count;
    emit_desc(dst, d);
    return true;
}

/* The receiver's end: tell rank `src` that partitions [first, first+count)
 * under `token` are finished.  For ourselves the send ops complete right
 * here: through the ring the DONE would be drained one proxy pass later
 * (drain_inbox runs before progress_copies), and a wait on the send
 * request that follows the wait on the receive sits through that pass. */
void NativeTransport::ack(int src, uint64_t token, int32_t first,
                          uint32_t count)
{
    if (src == rank_)
        handle_done(token, first, count);
    else if (!emit_done(src, token, first, count))
        pending_done_.push_back(PendingDone{src, token, first, count});
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
            const bool env = o->kind == OpKind::PRECV_PART &&
                             envelope_match(o, d.comm_id, src, d.tag);
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
    /* Reducing partitions (one request: all of the range or none) are taken
     * in the plain shape as ONE reduce entry of k * msg_bytes.  In any other
     * shape those of the strided reducing call are ONE strided reduce entry
     * (folded, or with the partition level, as below), provided the
     * sender's side steps in whole elements; those of the plain reducing
     * call expand, and so does everything start_dev_copy would reject: it
     * gives every partition its status. */
    if (op->reduce) {
        const uint32_t esize = reduce_elem_size(op->red_type);
        if (d.msg_bytes % esize != 0) return false;
        if (!plain) {
            uint64_t bits = (uint64_t)(uintptr_t)sp | (uint64_t)d.part_stride;
            if (s_strided) bits |= layout_align_bits(d.layout, 0);
            if (!op->reduce_any_sender || bits % esize != 0) return false;
        }
    }
    /* today's run, and today's rule for it: a misaligned one expands into
     * k hipMemcpyAsync (reducing: k entries on the element path) */
    if (plain && ((((uintptr_t)op->buf) | ((uintptr_t)sp)) & 15) != 0)
        return false;
    posted_recvs_.erase(posted_recvs_.begin() + first,
                        posted_recvs_.begin() + first + (long)k);
    /* every receive of the range is msg_bytes long: nothing is truncated */
    const PendingPull pp{op, src, d.token,
                         recv_status(op, src, d.tag, d.msg_bytes), op->buf, sp,
                         (uint64_t)k * d.msg_bytes, seen_ns(op, d),
                         d.partition, k};
    g_state->run_fast_msgs += k;
    if (op->reduce && plain) {
        pend_reduce_.push_back(PendingReduce{pp, op->red_type, op->red_op});
        g_state->run_reduce++;
        return true;
    }
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
    if (op->reduce) {
        pend_sreduce_.push_back(
            PendingStridedReduce{ps, op->red_type, op->red_op});
        g_state->run_sreduce++;
        return true;
    }
    (ps.parts ? g_state->run_parts : g_state->run_folded)++;
    pend_strided_.push_back(ps);
    return true;
}

/* The sender gets ONE ack, then every receive of the pull gets its status
 * and ch_done (the per-partition flag transitions stay with the proxy
 * walk). */
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
                a.send_op(pp.partition + (int32_t)j)->stat_batch = bs;
                bs->left_send++;
            }
        }
    }
    ack(pp.src, pp.token, pp.partition, pp.k);
    for (uint32_t j = 0; j < pp.k; j++) {
        Op *op = pull_op(pp, j);
        op->stat_batch = bs;
        complete_recv(op, pp.st);
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
    m.op = op;
    if (m.d.type == DESC_DEV_NOTIFY) {
        start_dev_copy(m);
        return;
    }
    /* a zero-byte message touches no memory of either kind: a strided
     * reducing receive takes it whatever its own buffer (a zero-byte send
     * always travels as one empty host chunk) */
    const bool empty_ok = op->reduce_any_sender && m.d.msg_bytes == 0;
    const char *why =
        op->reduce && !empty_ok ? reduce_reject(m, nullptr) : nullptr;
    if (why != nullptr) {
        MPIX_ERR("reducing receive from rank %d, tag %d fails with "
                 "MPI_ERR_TYPE: %s", m.src, m.d.tag, why);
        m.kind_mismatch = true;
    } else if ((op->strided || (m.d.flags & DESCF_STRIDED)) &&
               op->buf_is_device && !empty_ok) {
        fail_kind_mismatch(m);
    } else if (m.got > 0 && !m.heap.empty()) {
        /* host message: move already-buffered bytes (message order) into
         * the user buffer */
        uint64_t n = m.got;
        if (n > op->bytes) n = op->bytes;
        if (n > 0 && op->reduce && op->strided)
            layout_reduce_in(op->buf, op->layout, 0, m.heap.data(), n,
                             op->red_type, op->red_op);
        else if (n > 0 && op->reduce)
            /* whole elements: see deliver_chunk */
            reduce_host(op->buf, m.heap.data(),
                        n / reduce_elem_size(op->red_type), op->red_type,
                        op->red_op);
        else if (n > 0 && op->strided)
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
        /* A reducing receive combines the chunk where a plain one copies
         * it.  No element straddles two chunks: a chunk starts at a
         * multiple of CHUNK_BYTES, which every element size divides, so it
         * holds whole elements except possibly at the message's end, and a
         * message that ends inside an element was rejected in attach.  The
         * receive's own length is a multiple of the element size too, so a
         * truncated chunk still ends on an element.  Into a strided buffer
         * the chunk is combined run by run; the runs are whole elements. */
        static_assert(CHUNK_BYTES % 8 == 0, "chunks hold whole elements");
        if (n > 0 && m.op->reduce && m.op->strided)
            layout_reduce_in(m.op->buf, m.op->layout, d.chunk_off, src_chunk,
                             n, m.op->red_type, m.op->red_op);
        else if (n > 0 && m.op->reduce)
            reduce_host((char *)m.op->buf + d.chunk_off, src_chunk,
                        n / reduce_elem_size(m.op->red_type), m.op->red_type,
                        m.op->red_op);
        else if (n > 0 && m.op->strided)
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
    ChStatus st = recv_status(m.op, m.src, m.d.tag, m.d.msg_bytes);
    if (m.kind_mismatch) {
        st.bytes = 0;
        st.err = MPI_ERR_TYPE;
    } else if (m.op->reduce && m.op->strided && st.bytes > 0) {
        g_state->sreduce_host++;
    }
    complete_recv(m.op, st);
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

/* Why the reducing receive matched to `m` cannot combine the message (it
 * then completes with MPI_ERR_TYPE, its buffer untouched), or nullptr.
 * `src`: the sender's mapped address, for a device message. */
const char *NativeTransport::reduce_reject(const InboundMsg &m,
                                           const void *src) const
{
    const Op *op = m.op;
    const uint32_t esize = reduce_elem_size(op->red_type);
    const bool dev_msg = m.d.type == DESC_DEV_NOTIFY;
    if ((m.d.flags & DESCF_STRIDED) && !op->reduce_any_sender)
        return "the sender's message is strided";
    if (m.d.msg_bytes % esize != 0)
        return "the message length is not a multiple of the element size";
    if (dev_msg != op->buf_is_device)
        return "one side is in host memory and the other in device memory";
    if (dev_msg && ((uintptr_t)src % esize) != 0)
        return "the sender's address is not aligned to the element size";
    /* a strided device sender is walked in place: an element must not
     * straddle two of its runs (host chunks come in message order) */
    if (dev_msg && (m.d.flags & DESCF_STRIDED) &&
        layout_align_bits(m.d.layout, 0) % esize != 0)
        return "the sender's run or strides are not multiples of the element "
               "size";
    return nullptr;
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

/* A matched device message that will move no data: the receive completes
 * with `st`, and the sender is still acked so that it does not hang. */
void NativeTransport::fail_dev_recv(InboundMsg &m, const ChStatus &st)
{
    complete_recv(m.op, st);
    ack(m.src, m.d.token, m.d.partition, 1);
    erase_inbound(&m);
}

void NativeTransport::start_dev_copy(InboundMsg &m)
{
    Op *op = m.op;
    void *src = map_remote(m.d);
    ChStatus st = recv_status(op, m.src, m.d.tag, m.d.msg_bytes);
    if (src == nullptr) {
        st.err = MPI_ERR_OTHER;
        fail_dev_recv(m, st);
        return;
    }
    const bool strided = op->strided || (m.d.flags & DESCF_STRIDED) != 0;
    if (strided && !op->buf_is_device) {
        fail_kind_mismatch(m);
        st.bytes = 0;
        st.err = MPI_ERR_TYPE;
        fail_dev_recv(m, st);
        return;
    }
    if (op->reduce) {
        if (const char *why = reduce_reject(m, src)) {
            MPIX_ERR("reducing receive from rank %d, tag %d fails with "
                     "MPI_ERR_TYPE: %s", m.src, m.d.tag, why);
            st.bytes = 0;
            st.err = MPI_ERR_TYPE;
            fail_dev_recv(m, st);
            return;
        }
    }
    const uint64_t n = st.bytes;
    const PendingPull pp{op, m.src, m.d.token, st, op->buf, src, n,
                         seen_ns(op, m.d), m.d.partition, 1};
    /* A reducing receive is always an entry of a reduce kernel, by the
     * vector or the element path: never hipMemcpyAsync, never a plain
     * strided entry.  Strided on either side (reduce_reject let a strided
     * sender through for the strided reducing calls only) it is an entry of
     * the strided reduce kernel, layouts as for a plain strided pull.  n is
     * a multiple of the element size (the message's length is, and a
     * truncated one is cut to the receive's).  A zero-byte message falls
     * through to the batch of one that copies nothing. */
    if (op->reduce && n > 0) {
        if (strided) {
            PendingStridedReduce pr{{}, op->red_type, op->red_op};
            pr.ps.pp = pp;
            pr.ps.sl = (m.d.flags & DESCF_STRIDED)
                           ? m.d.layout : layout_contiguous(m.d.msg_bytes);
            pr.ps.dl = op->strided ? op->layout : layout_contiguous(op->bytes);
            pend_sreduce_.push_back(pr);
        } else {
            pend_reduce_.push_back(
                PendingReduce{pp, op->red_type, op->red_op});
        }
        erase_inbound(&m);
        return;
    }
    /* The shader pull path requires (a) a device destination — dereferencing
     * a pageable host pointer from a kernel faults on non-XNACK systems —
     * and (b) 16-byte alignment on both sides (user buffers can be
     * arbitrarily offset, e.g. partitioned slices); a strided pull goes by
     * its granule instead.  Everything else rides hipMemcpyAsync (SDMA /
     * runtime blit).  A pull kernel is deadlock-safe in both copy-stream
     * phases: before the priority switch no spin-wait kernel exists; after
     * it the copy stream owns its hardware queue (see maybe_switch_prio) */
    const bool kernel_ok = op->buf_is_device &&
        ((((uintptr_t)op->buf) | ((uintptr_t)src)) & 15) == 0;
    if (n > 0 && (strided || kernel_ok)) {
        /* defer: every pull that matched in this progress pass goes out in
         * ONE k_pull_multi launch (flush_pulls), every strided one in ONE
         * k_pull_strided launch (flush_strided).  There n is a multiple of
         * the granule: it is the length of one of the two layouts, and the
         * granule divides the runs of both. */
        if (strided) {
            PendingStrided ps;
            ps.pp = pp;
            ps.sl = (m.d.flags & DESCF_STRIDED)
                        ? m.d.layout : layout_contiguous(m.d.msg_bytes);
            ps.dl = op->strided ? op->layout : layout_contiguous(op->bytes);
            pend_strided_.push_back(ps);
        } else {
            pend_pulls_.push_back(pp);
        }
        erase_inbound(&m);
        return;
    }
    /* a batch of one.  A runtime copy cannot store a completion word, so it
     * completes by event, or by the tail kernel behind it in that mode.
     * t_launch_ns stays 0 */
    hipStream_t cs = copy_stream(n);
    hipError_t e = hipSuccess;
    if (n > 0) e = hipMemcpyAsync(op->buf, src, n, hipMemcpyDefault, cs);
    if (e != hipSuccess) {
        MPIX_ERR("hipMemcpyAsync(pull %lu B) failed: %s", (unsigned long)n,
                 hipGetErrorString(e));
        st.err = MPI_ERR_OTHER;
        fail_dev_recv(m, st);
        return;
    }
    if (trace_on())
        fprintf(stderr, "[mpix trace] pull start %lu B via memcpyAsync "
                "(dst=%p src=%p)\n", (unsigned long)n, op->buf, src);
    int slot = -1;
    if (done_mode_ == PullDoneMode::TAIL) {
        PullDone done{nullptr, nullptr, 0};
        slot = signal_by_tail(acquire_done(&done), done, cs);
    }
    push_batch({pp}, cs, slot).memcpy_pull = true;
    erase_inbound(&m);
}

/* What follows a successful launch or copy on `cs`: its batch, the last of
 * batches_.  The word path (slot >= 0) records no event (with MPIX_STATS=1
 * it does, to measure what the event would have cost). */
NativeTransport::PullBatch &NativeTransport::push_batch(
    std::vector<PendingPull> items, hipStream_t cs, int slot)
{
    batches_.emplace_back();
    PullBatch &b = batches_.back();
    b.items = std::move(items);
    b.done_slot = slot;
    b.cs = cs;
    if (slot >= 0) b.t_born_ns = now_ns();
    if (slot < 0 || (g_state != nullptr && g_state->stats)) {
        b.ev = get_event();
        hipError_t e = hipEventRecord(b.ev, cs);
        if (e != hipSuccess)
            MPIX_ERR("hipEventRecord(pull) failed: %s", hipGetErrorString(e));
    }
    return b;
}

/* A slot of the ring and the kernel argument for it, on a word path; -1:
 * the event path (MPIX_PULL_DONE=event, or the ring is full). */
int NativeTransport::acquire_done(PullDone *done)
{
    if (done_mode_ == PullDoneMode::EVENT) return -1;
    const int slot = done_acquire(&done_ring_, &done->seq);
    if (slot >= 0) {
        done->counter = done_counters_ + (size_t)slot * DONE_COUNTER_STRIDE;
        done->word = done_words_d_ + (size_t)slot * DONE_WORD_STRIDE;
    }
    return slot;
}

/* Tail mode: the kernel that stores the word of `slot`, behind what was just
 * put on `cs`.  Returns the slot; or -1 (the slot was -1, or the launch
 * failed and the slot was given back): the copy is on the stream all the
 * same, and its batch completes by event. */
int NativeTransport::signal_by_tail(int slot, const PullDone &done,
                                    hipStream_t cs)
{
    if (slot < 0) return -1;
    launch_tail(done.word, done.seq, cs);
    if (hipGetLastError() == hipSuccess) return slot;
    done_release(&done_ring_, slot);
    return -1;
}

/* The second half of a flush: `items` go out as one launch on `cs`.
 * launch(done) issues the kernel (done: the argument of the completion
 * word, or nullptr for the kernel that signals nothing) and returns the
 * launch's error.  In tail mode the signal is a launch of its own behind
 * that kernel.  Returns the batch; or nullptr: the launch failed, and every
 * item was finished with MPI_ERR_OTHER. */
template <typename Launch>
NativeTransport::PullBatch *NativeTransport::submit_batch(
    std::vector<PendingPull> items, hipStream_t cs, const char *kernel,
    Launch launch)
{
    PullDone done{nullptr, nullptr, 0};
    int slot = acquire_done(&done);
    const bool tail = done_mode_ == PullDoneMode::TAIL;
    const hipError_t e = launch(slot >= 0 && !tail ? &done : nullptr);
    if (e == hipSuccess && tail) slot = signal_by_tail(slot, done, cs);
    if (e != hipSuccess) {
        MPIX_ERR("%s launch failed: %s", kernel, hipGetErrorString(e));
        if (slot >= 0) done_release(&done_ring_, slot);
        for (PendingPull &pp : items) {
            pp.st.err = MPI_ERR_OTHER;
            finish_pull(pp, nullptr);
        }
        return nullptr;
    }
    return &push_batch(std::move(items), cs, slot);
}

void NativeTransport::flush_pulls()
{
    const bool stats = g_state != nullptr && g_state->stats;
    const uint64_t tile_bytes = (uint64_t)PULL_THREADS * pull_unroll() * 16;
    while (!pend_pulls_.empty()) {
        PullSeg segs[MPIX_PULL_BATCH];
        size_t n = pend_pulls_.size();
        if (n > MPIX_PULL_BATCH) n = MPIX_PULL_BATCH;
        uint64_t total = 0, t_first = UINT64_MAX;
        for (size_t i = 0; i < n; i++) {
            const PendingPull &pp = pend_pulls_[i];
            segs[i] = PullSeg{pp.dst, pp.csrc, pp.n};
            total += pp.n;
            if (pp.t_seen_ns < t_first) t_first = pp.t_seen_ns;
        }
        plan_pulls(segs, n, tile_bytes, &plan_);
        hipStream_t cs = copy_stream(total);
        uint64_t tiles = pull_total_tiles(plan_);
        unsigned blocks = tiles < pull_max_blocks() ? (unsigned)tiles
                                                    : pull_max_blocks();
        std::vector<PendingPull> items(pend_pulls_.begin(),
                                       pend_pulls_.begin() + n);
        pend_pulls_.erase(pend_pulls_.begin(), pend_pulls_.begin() + n);
        uint64_t t_call = 0, t_rec = 0;
        PullBatch *b = submit_batch(
            std::move(items), cs, "k_pull_multi", [&](const PullDone *done) {
                t_call = stats ? now_ns() : 0;
                launch_pull(plan_, pull_unroll(), pull_nontemporal(), blocks,
                            cs, done);
                const hipError_t e = hipGetLastError();
                t_rec = stats ? now_ns() : 0;
                return e;
            });
        if (b == nullptr) continue;
        if (stats) {
            State *s = g_state;
            b->t_launch_ns = now_ns();
            const uint64_t call = t_rec - t_call;
            if (!s->bleg_first_seen) {
                /* loads the code object: reported apart from the means */
                s->bleg_first_seen = b->first = true;
                s->bleg_first_wait_ns = b->t_launch_ns - t_first;
                s->bleg_first_call_ns = call;
                s->bleg_first_rec_ns = b->t_launch_ns - t_rec;
                s->bleg_first_items = pull_ops(b->items);
            } else {
                s->bleg_wait_ns += b->t_launch_ns - t_first;
                s->bleg_call_ns += call;
                if (call < s->bleg_call_min_ns) s->bleg_call_min_ns = call;
                if (call > s->bleg_call_max_ns) s->bleg_call_max_ns = call;
                s->bleg_rec_ns += b->t_launch_ns - t_rec;
                s->bleg_n++;
                s->bleg_items += pull_ops(b->items);
                s->bleg_copies += plan_.ncopies;
            }
        }
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
        std::vector<PendingPull> items;
        for (size_t i = 0; i < n; i++) {
            const PendingStrided &ps = pend_strided_[i];
            segs[i] = StridedSeg{ps.pp.dst, ps.pp.csrc, ps.pp.n, ps.sl, ps.dl};
            if (ps.parts) {
                segs[i].parts = ps.pp.k;
                segs[i].s_part_stride = ps.s_part_stride;
                segs[i].d_part_stride = ps.d_part_stride;
            }
            total += ps.pp.n;
            items.push_back(ps.pp);
        }
        pend_strided_.erase(pend_strided_.begin(), pend_strided_.begin() + n);
        plan_strided(segs, n, strided_div64_, &splan_);
        /* same stream choice as flush_pulls: a contiguous batch of this
         * pass and this launch go back to back on the copy stream */
        hipStream_t cs = copy_stream(total);
        uint64_t tiles = strided_total_tiles(splan_);
        unsigned blocks = tiles < 1024 ? (unsigned)tiles : 1024u;
        const bool wide = strided_plan_wide(splan_);
        const bool parts = strided_plan_parts(splan_);
        /* t_launch_ns stays 0: the batch legs of MPIX_STATS count plain
         * pulls */
        if (submit_batch(std::move(items), cs, "k_pull_strided",
                         [&](const PullDone *done) {
                             launch_strided(splan_, wide, parts, blocks, cs,
                                            done);
                             return hipGetLastError();
                         }) == nullptr)
            continue;
        if (trace_on())
            fprintf(stderr, "[mpix trace] strided pull batch n=%zu tiles=%lu "
                    "total=%lu B wide=%d parts=%d\n", n, (unsigned long)tiles,
                    (unsigned long)total, (int)wide, (int)parts);
    }
}

/* The stream of every reducing launch, contiguous or strided: the copy
 * stream itself, whatever the size.  Should it have been replaced since the
 * last reducing launch (maybe_switch_prio), the new one waits for the old
 * one once. */
hipStream_t NativeTransport::reduce_stream()
{
    hipStream_t cs = copy_stream(0);
    if (reduce_cs_ != nullptr && reduce_cs_ != cs) {
        hipEvent_t ev = get_event();
        if (hipEventRecord(ev, reduce_cs_) != hipSuccess ||
            hipStreamWaitEvent(cs, ev, 0) != hipSuccess)
            MPIX_ERR("reduce: ordering behind the retired copy stream "
                     "failed: %s", hipGetErrorString(hipGetLastError()));
        put_event(ev);
    }
    reduce_cs_ = cs;
    return cs;
}

/* The reducing pulls of this pass: one k_pull_reduce launch, and another
 * for every entry whose destination overlaps one already planned and for
 * every MPIX_PULL_BATCH entries.  All of them go to reduce_stream(): a later
 * launch must run behind an earlier one that combined into the same bytes
 * (pull_kernels.h on why it then sees them). */
void NativeTransport::flush_reduce()
{
    while (!pend_reduce_.empty()) {
        ReduceSeg segs[MPIX_PULL_BATCH];
        size_t n = pend_reduce_.size();
        if (n > MPIX_PULL_BATCH) n = MPIX_PULL_BATCH;
        for (size_t i = 0; i < n; i++) {
            const PendingReduce &pr = pend_reduce_[i];
            segs[i] = ReduceSeg{pr.pp.dst, pr.pp.csrc, pr.pp.n, pr.type,
                                pr.op};
        }
        n = plan_reduce(segs, n, MPIX_REDUCE_TILE, &rplan_);
        uint64_t total = 0;
        std::vector<PendingPull> items;
        for (size_t i = 0; i < n; i++) {
            total += pend_reduce_[i].pp.n;
            items.push_back(pend_reduce_[i].pp);
        }
        pend_reduce_.erase(pend_reduce_.begin(), pend_reduce_.begin() + n);
        hipStream_t cs = reduce_stream();
        const uint64_t tiles = reduce_total_tiles(rplan_);
        const unsigned blocks = tiles < pull_max_blocks() ? (unsigned)tiles
                                                          : pull_max_blocks();
        g_state->reduce_launches++;
        g_state->reduce_msgs += pull_ops(items);
        g_state->reduce_entries += rplan_.n;
        /* t_launch_ns stays 0: the batch legs of MPIX_STATS count plain
         * pulls */
        if (submit_batch(std::move(items), cs, "k_pull_reduce",
                         [&](const PullDone *done) {
                             launch_reduce(rplan_, blocks, cs, done);
                             return hipGetLastError();
                         }) == nullptr)
            continue;
        if (trace_on())
            fprintf(stderr, "[mpix trace] reduce pull batch n=%zu entries=%u "
                    "tiles=%lu total=%lu B\n", n, rplan_.n,
                    (unsigned long)tiles, (unsigned long)total);
    }
}

/* The strided reducing pulls of this pass, behind the contiguous ones on
 * the same stream (reduce_stream), so that reducing launches into
 * overlapping memory always follow each other: one k_pull_strided_reduce
 * launch, and another for every entry whose destination extent overlaps one
 * already planned and for every MPIX_STRIDED_BATCH entries. */
void NativeTransport::flush_strided_reduce()
{
    while (!pend_sreduce_.empty()) {
        StridedReduceSeg segs[MPIX_STRIDED_BATCH];
        size_t n = pend_sreduce_.size();
        if (n > MPIX_STRIDED_BATCH) n = MPIX_STRIDED_BATCH;
        for (size_t i = 0; i < n; i++) {
            const PendingStridedReduce &pr = pend_sreduce_[i];
            const PendingStrided &ps = pr.ps;
            StridedReduceSeg &g = segs[i];
            g.dst = ps.pp.dst;
            g.src = ps.pp.csrc;
            g.bytes = ps.pp.n;
            g.sl = ps.sl;
            g.dl = ps.dl;
            if (ps.parts) {
                g.parts = ps.pp.k;
                g.s_part_stride = ps.s_part_stride;
                g.d_part_stride = ps.d_part_stride;
            }
            g.type = pr.type;
            g.op = pr.op;
        }
        n = plan_strided_reduce(segs, n, strided_div64_, &srplan_);
        if (n == 0) {
            /* reduce_reject and try_run_fast_path let nothing through that
             * the planner refuses */
            MPIX_ERR("strided reduce: a pull that steps in fractions of an "
                     "element reached the planner");
            PendingPull pp = pend_sreduce_.front().ps.pp;
            pend_sreduce_.erase(pend_sreduce_.begin());
            pp.st.err = MPI_ERR_OTHER;
            finish_pull(pp, nullptr);
            continue;
        }
        uint64_t total = 0;
        std::vector<PendingPull> items;
        for (size_t i = 0; i < n; i++) {
            total += pend_sreduce_[i].ps.pp.n;
            items.push_back(pend_sreduce_[i].ps.pp);
        }
        pend_sreduce_.erase(pend_sreduce_.begin(), pend_sreduce_.begin() + n);
        hipStream_t cs = reduce_stream();
        const uint64_t tiles = strided_reduce_total_tiles(srplan_);
        /* the limit of the contiguous reducing launches it shares the
         * stream with (MPIX_PULL_BLOCKS) */
        const unsigned blocks = tiles < pull_max_blocks() ? (unsigned)tiles
                                                          : pull_max_blocks();
        const bool wide = strided_reduce_plan_wide(srplan_);
        g_state->sreduce_launches++;
        g_state->sreduce_msgs += pull_ops(items);
        g_state->sreduce_entries += srplan_.n;
        /* t_launch_ns stays 0: the batch legs of MPIX_STATS count plain
         * pulls */
        if (submit_batch(std::move(items), cs, "k_pull_strided_reduce",
                         [&](const PullDone *done) {
                             launch_strided_reduce(srplan_, wide, blocks, cs,
                                                   done);
                             return hipGetLastError();
                         }) == nullptr)
            continue;
        if (trace_on()) {
            unsigned vec = 0; /* entries on the vector path */
            for (uint32_t i = 0; i < srplan_.n; i++)
                vec += srplan_.e[i].glog == 4;
            fprintf(stderr, "[mpix trace] strided reduce pull batch n=%zu "
                    "entries=%u vec=%u tiles=%lu total=%lu B wide=%d\n", n,
                    srplan_.n, vec, (unsigned long)tiles,
                    (unsigned long)total, (int)wide);
        }
    }
}

/* Is the batch's work finished?  *err: hipSuccess, or why its ops fail.
 * Event path: hipEventQuery.  Word paths (the tail kernel's word too): a
 * plain acquire load of the slot's host word, no runtime call.  A kernel
 * that dies never stores its word, nor does one behind it on the stream, so
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

void NativeTransport::progress_copies()
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
        if (it->memcpy_pull && trace_on())
            fprintf(stderr, "[mpix trace] pull done (e=%d)\n", (int)e);
        BatchStat *bs = nullptr;
        if (it->t_launch_ns) {
            bs = new BatchStat{now_ns(), (int)pull_ops(it->items), it->first};
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
        /* ack the sender, then complete the receives */
        for (PendingPull &pp : it->items) {
            if (e != hipSuccess) pp.st.err = MPI_ERR_OTHER;
            finish_pull(pp, bs);
        }
        it = batches_.erase(it);
    }
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
    if (!ptr_is_device(dst) && !ptr_is_device(src)) {
        memcpy(dst, src, n);
        return 0;
    }
    hipStream_t cs = copy_stream(0); /* always the copy stream itself */
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
