/* mpix — control plane of the native transport: the descriptor and the
 * per-pair inbox in shared memory (no HIP dependency, checked on its own by
 * tests/native/shm_ring_check.cpp, under ASan/UBSan and under TSan).
 *
 * Rank r owns one segment of `nranks` inboxes; inbox s of it is written by
 * rank s alone and read by r alone: an SPSC ring of `ring_slots` descriptors
 * plus `stage_chunks` staging chunks for host payloads.  Cursors only grow;
 * each side keeps its own privately, passes it in, and publishes it with a
 * release store (`head`, `tail`, `stage_tail`) that the other side acquires.
 * Chunks are credits: taken at cursor % stage_chunks, returned in order. */
#ifndef MPIX_TRANSPORT_SHM_RING_H
#define MPIX_TRANSPORT_SHM_RING_H

#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "../../include/mpix/mpix_layout.h"

namespace mpix {

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

static inline ShmGeom shm_geometry(int nranks, uint32_t ring_slots,
                                   uint32_t stage_chunks)
{
    ShmGeom g;
    g.ring_slots = ring_slots;
    g.stage_chunks = stage_chunks;
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

static inline InboxView inbox_view(void *seg_base, const ShmGeom &g, int src)
{
    char *p = (char *)seg_base + (size_t)src * g.inbox_bytes;
    InboxView v;
    v.hdr = (InboxHdr *)p;
    v.ring = (Desc *)(p + sizeof(InboxHdr));
    v.stage = (char *)(v.ring + g.ring_slots);
    return v;
}

/* ---- producer: `head` / `stage_head` are its own cursors for this inbox */

static inline bool ring_has_space(const InboxView &v, const ShmGeom &g,
                                  uint64_t head, uint64_t need)
{
    uint64_t tail = v.hdr->tail.load(std::memory_order_acquire);
    return head + need - tail <= g.ring_slots;
}

static inline void ring_emit(const InboxView &v, const ShmGeom &g,
                             uint64_t *head, const Desc &d)
{
    uint64_t h = *head;
    v.ring[h % g.ring_slots] = d;
    v.hdr->head.store(h + 1, std::memory_order_release);
    *head = h + 1;
}

static inline uint64_t stage_free_chunks(const InboxView &v, const ShmGeom &g,
                                         uint64_t stage_head)
{
    uint64_t st = v.hdr->stage_tail.load(std::memory_order_acquire);
    return g.stage_chunks - (stage_head - st);
}

/* ---- consumer: `tail` is its own cursor for this inbox.  Descriptors
 * [tail, ring_head) may be read in place (ring_front); a slot stays the
 * consumer's until ring_pop, the oldest chunk until stage_release. */

static inline uint64_t ring_head(const InboxView &v)
{
    return v.hdr->head.load(std::memory_order_acquire);
}

static inline const Desc &ring_front(const InboxView &v, const ShmGeom &g,
                                     uint64_t tail)
{
    return v.ring[tail % g.ring_slots];
}

static inline void ring_pop(const InboxView &v, uint64_t *tail)
{
    v.hdr->tail.store(++*tail, std::memory_order_release);
}

static inline void stage_release(const InboxView &v)
{
    v.hdr->stage_tail.fetch_add(1, std::memory_order_release);
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_SHM_RING_H */
