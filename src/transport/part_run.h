/* mpix — partition runs on the native control plane (no HIP dependency).
 *
 * The partitions of one partitioned request are pieces of one buffer, the
 * request's part_stride apart (buf + p * part_stride: part_bytes for the
 * plain init calls, anything not smaller than a partition's extent for the
 * strided ones), all laid out alike, and everything a DEV_NOTIFY descriptor
 * says about them except the partition number is the same.  The distance is
 * ALWAYS the request's part_stride, never inferred from the message size:
 * contiguous rows of a pitched buffer are msg_bytes long and further apart.
 * So the sender announces a
 * RUN of them, partitions p0 .. p0+k-1, with ONE descriptor (partition = p0,
 * count = k), and the receiver answers with one DONE per range it finished.
 *
 * This header holds the pure decisions, so they can be checked on a CPU
 * build (tests/native/part_run_check.cpp):
 *
 *  - part_run_length: how long the run at the head of a send queue is;
 *  - part_run_fast_range: whether the posted receives take a run as ONE pull
 *    (the fast path), and if not,
 *  - part_run_slice: how the descriptor expands into k single-partition
 *    messages, exactly as if k descriptors had arrived in partition order;
 *  - RunAwait / part_run_ack: the sender's bookkeeping of the ranges acked so
 *    far; ranges may arrive in any order and must sum to the run.
 */
#ifndef MPIX_TRANSPORT_PART_RUN_H
#define MPIX_TRANSPORT_PART_RUN_H

#include <stddef.h>
#include <stdint.h>

namespace mpix {

/* what part_run_length needs to know about one queued send */
struct RunSend {
    const void *req;   /* owning request */
    uint32_t pseq;     /* partitioned iteration number */
    int32_t partition;
    uint64_t bytes;
    bool part_send;    /* a PSEND_PART op */
    bool device;
    bool strided;
};

/* Length (>= 1) of the run at the head of a queue of `n` > 0 sends;
 * get(i) describes queue entry i.  A run is a maximal sequence of
 * queue-adjacent partition sends of one request and one iteration with
 * partition numbers p0, p0+1, ..., from a device buffer, all strided or
 * all contiguous (one request has one layout), and announced by DEV_NOTIFY:
 * strided, or larger than the sender-push threshold `push_max`.  Gaps
 * between the partitions do not matter here: the descriptor carries the
 * request's part_stride.  A head that does not qualify is a run of 1:
 * today's descriptor. */
template <class Get>
static inline size_t part_run_length(size_t n, Get get, uint64_t push_max)
{
    const RunSend h = get(0);
    if (!h.part_send || !h.device || (!h.strided && h.bytes <= push_max))
        return 1;
    size_t k = 1;
    while (k < n && k < (size_t)INT32_MAX) {
        const RunSend s = get(k);
        if (!s.part_send || !s.device || s.strided != h.strided ||
            s.req != h.req ||
            s.pseq != h.pseq || s.bytes != h.bytes ||
            (int64_t)s.partition != (int64_t)h.partition + (int64_t)k)
            break;
        k++;
    }
    return k;
}

/* what part_run_fast_range needs to know about one posted receive */
struct RunRecv {
    const void *req;
    int32_t partition;
    uint64_t bytes;
    uintptr_t buf;
    bool envelope; /* matches the descriptor in everything but the partition
                      number (comm, partitioned kind, source, tag) */
    bool device;
    bool strided;
    int64_t part_stride = 0; /* of the owning request (its receives are that
                                far apart); read by the 5-argument
                                part_run_fast_range only */
};

/* The fast path: index of the first of k posted receives that take the run
 * {p0, k, msg_bytes} as ONE pull, or -1 when the run has to be expanded.
 * get(i) describes posted receive i of n_posted, in post order.  It applies
 * when the first posted receive that matches partition p0 is followed by the
 * receives for p0+1 .. p0+k-1 of the same request, each of exactly
 * msg_bytes, in device memory, all strided or all contiguous, and sitting at
 * h.buf + j * (the receiver's part_stride), where h is the first of them.  A
 * receive posted BEFORE that range which would take one of the later
 * partitions (another request with the same envelope) also sends the run to
 * the expansion: matching is first-posted-first, partition by partition.
 * Which pull it becomes (a contiguous copy, a folded layout, an entry with a
 * partition level) is the caller's decision, by the shape of both sides. */
template <class Get>
static inline long part_run_fast_range(size_t n_posted, Get get, int32_t p0,
                                       uint32_t k, uint64_t msg_bytes)
{
    if (k < 2 || msg_bytes == 0) return -1;
    size_t first = n_posted;
    for (size_t i = 0; i < n_posted; i++) {
        const RunRecv r = get(i);
        if (!r.envelope) continue;
        if (r.partition == p0) {
            first = i;
            break;
        }
        if ((int64_t)r.partition > (int64_t)p0 &&
            (int64_t)r.partition < (int64_t)p0 + (int64_t)k)
            return -1;
    }
    if (first == n_posted || n_posted - first < (size_t)k) return -1;
    const RunRecv h = get(first);
    for (uint32_t j = 0; j < k; j++) {
        const RunRecv r = get(first + j);
        if (!r.envelope || r.req != h.req ||
            (int64_t)r.partition != (int64_t)p0 + (int64_t)j ||
            r.bytes != msg_bytes || !r.device || r.strided != h.strided ||
            r.buf != h.buf + (uintptr_t)j * (uintptr_t)h.part_stride)
            return -1;
    }
    return (long)first;
}

/* The plain shape of the fast path: the range above for contiguous
 * receives msg_bytes apart (slices of one buffer), with both base addresses
 * 16-byte aligned; `src` is the sender's.  This is the run that becomes one
 * contiguous copy of k * msg_bytes. */
template <class Get>
static inline long part_run_fast_range(size_t n_posted, Get get, int32_t p0,
                                       uint32_t k, uint64_t msg_bytes,
                                       uintptr_t src)
{
    if ((src & 15) != 0) return -1;
    const long first = part_run_fast_range(
        n_posted,
        [&](size_t i) {
            RunRecv r = get(i);
            r.part_stride = (int64_t)msg_bytes;
            return r;
        },
        p0, k, msg_bytes);
    if (first < 0) return -1;
    const RunRecv h = get((size_t)first);
    if (h.strided || (h.buf & 15) != 0) return -1;
    return first;
}

/* Message j (0 <= j < k) of the expansion of a run descriptor: what a
 * single-partition descriptor for partition p0+j would have carried; the
 * partitions are the SENDER's part_stride apart.  The token stays the run
 * token; its ack is the range {partition, 1}. */
struct RunSlice {
    int32_t partition;
    uint64_t ipc_off;
    uint64_t token;
    uint32_t count; /* always 1 */
};

static inline RunSlice part_run_slice(int32_t p0, uint64_t ipc_off,
                                      uint64_t part_stride, uint64_t token,
                                      uint32_t j)
{
    RunSlice s;
    s.partition = (int32_t)((int64_t)p0 + (int64_t)j);
    s.ipc_off = ipc_off + (uint64_t)j * part_stride;
    s.token = token;
    s.count = 1;
    return s;
}

/* Sender side: one announced run waiting for its acks. */
struct RunAwait {
    int32_t p0;
    uint32_t k;
    uint32_t remaining; /* partitions not acked yet */
};

enum RunAck {
    RUN_ACK_BAD = -1, /* range outside the run, or more than was left */
    RUN_ACK_MORE = 0, /* accepted, the run is still waiting */
    RUN_ACK_LAST = 1, /* accepted, every partition of the run is acked */
};

/* Account the ack of partitions [first, first+count).  A bad range changes
 * nothing. */
static inline RunAck part_run_ack(RunAwait *a, int32_t first, uint32_t count)
{
    if (count == 0 || count > a->remaining ||
        (int64_t)first < (int64_t)a->p0 ||
        (int64_t)first + (int64_t)count > (int64_t)a->p0 + (int64_t)a->k)
        return RUN_ACK_BAD;
    a->remaining -= count;
    return a->remaining == 0 ? RUN_ACK_LAST : RUN_ACK_MORE;
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_PART_RUN_H */
