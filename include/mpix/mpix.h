/* mpix — accelerator-triggered MPI extensions for AMD Instinct MI355X (gfx950)
 *
 * Public C API. Provides the same 17-entry-point MPIX_* surface as NVIDIA's
 * MPI-ACX prototype (reference: /root/reference/include/mpi-acx.h:48-104),
 * re-designed for ROCm/HIP on CDNA4:
 *
 *   - Stream/graph-triggered point-to-point: MPIX_Isend_enqueue /
 *     MPIX_Irecv_enqueue / MPIX_Wait[all]_enqueue ordered by a HIP stream or
 *     HIP graph instead of the host.
 *   - Kernel-triggered partitioned communication: MPIX_Psend_init /
 *     MPIX_Precv_init plus __device__ MPIX_Pready / MPIX_Parrived
 *     (see mpix_device.h) so a GPU kernel can publish / poll individual
 *     partitions of a large message.
 *
 * Core mechanism (same protocol family as the reference, new implementation):
 * a CPU proxy thread polls 32-bit flag words in host-pinned, device-mapped
 * memory.  The GPU (via hipStream memOps or tiny gfx950 kernels) flips a flag
 * to PENDING; the proxy issues the communication on the GPU's behalf and
 * flips the flag to COMPLETED, which the GPU (or host) is waiting on.
 *
 * Unlike the reference, the data plane is NOT required to be a GPU-aware MPI:
 * intra-node transfers between GPUs use a native xGMI path (HIP IPC +
 * peer-to-peer SDMA copies) and host transfers use a shared-memory channel,
 * with host-MPI passthrough available when the library is initialized inside
 * an MPI program.  See README.md / ARCHITECTURE.md.
 */
#ifndef MPIX_H
#define MPIX_H

#include <mpi.h>

#include "mpix_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef void *MPIX_Request;
typedef void *MPIX_Prequest;

#define MPIX_REQUEST_NULL  NULL
#define MPIX_PREQUEST_NULL NULL

/* Library init / teardown.  May be called either
 *  (a) after MPI_Init_thread(MPI_THREAD_MULTIPLE)  — "MPI mode": rank/size
 *      come from MPI_COMM_WORLD and host-buffer traffic may ride MPI, or
 *  (b) without MPI, with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the
 *      environment (torchrun-style)                — "env mode": the native
 *      shared-memory + xGMI data plane carries everything.
 * Both modes work with zero GPUs (host-buffer, proxy-only path). */
int MPIX_Init(void);
int MPIX_Finalize(void);

/* Runtime introspection (not in the reference API): how MPIX_Init resolved
 * this process — GPU presence, hipStream memOps probe results, bootstrap
 * mode.  Any pointer may be NULL. */
int MPIX_Query_config(int *have_gpu, int *use_memops, int *use_batch_memops,
                      int *mpi_mode, int *nflags);

/* ENQUEUED OPERATIONS ******************************************************/

enum {
    MPIX_QUEUE_HIP_STREAM, /* queue is a hipStream_t*  */
    MPIX_QUEUE_HIP_GRAPH   /* queue is a hipGraph_t*: the call RETURNS a
                              single-node graph the caller composes */
};

int MPIX_Isend_enqueue(const void *buf, int count, MPI_Datatype datatype,
                       int dest, int tag, MPI_Comm comm, MPIX_Request *request,
                       int qtype, void *queue);

int MPIX_Irecv_enqueue(void *buf, int count, MPI_Datatype datatype,
                       int source, int tag, MPI_Comm comm, MPIX_Request *request,
                       int qtype, void *queue);

/* Strided variants: `buf` is laid out as *layout (mpix_layout.h: a
 * contiguous run plus up to two strided levels) and the message is its bytes
 * in (plane, run, byte) order, layout->run_bytes * count[0] * count[1] of
 * them.  As with MPI datatypes only that byte sequence has to agree between
 * the two sides: either side may be strided, contiguous (the plain calls) or
 * strided differently.  Device buffers are moved by one kernel that walks
 * both layouts (no pack, no unpack, no staging); host buffers are staged run
 * by run.  Requests behave exactly like those of the plain calls (stream and
 * graph queues, captures, MPIX_Wait*_enqueue, status byte count, truncation).
 * Errors: MPI_ERR_ARG for a layout with a stride that is zero, negative or
 * smaller than what it steps over (overlap), or whose size overflows;
 * MPI_ERR_TYPE at enqueue for a communicator served by the MPI passthrough
 * transport, and as the completion status when one buffer is in device and
 * the other in host memory (plain messages between the two kinds work).
 * Partitioned requests with layouts: MPIX_Psend/Precv_init_strided below.
 * Not supported: decoding MPI_Type_vector / subarray handles, more than two
 * strided levels. */
int MPIX_Isend_strided_enqueue(const void *buf, const MPIX_Layout *layout,
                               int dest, int tag, MPI_Comm comm,
                               MPIX_Request *request, int qtype, void *queue);

int MPIX_Irecv_strided_enqueue(void *buf, const MPIX_Layout *layout,
                               int source, int tag, MPI_Comm comm,
                               MPIX_Request *request, int qtype, void *queue);

/* Reducing receives: the message is COMBINED into the buffer instead of
 * overwriting it.  On completion buf[i] = buf[i] op msg[i] for every whole
 * element of the message; exactly one combine happens per element per
 * receive, so the result is bit-defined.  Nothing changes for the sender: a
 * message is still its bytes, and MPIX_Isend_enqueue or MPIX_Psend_init
 * match.  Device buffers are combined inside the receiver's pull kernel (no
 * staging buffer, no add kernel behind the wait), host buffers as the chunks
 * arrive.  mpix has its own element types because MPI 3.1 has no bf16 or
 * f16 datatype.
 *
 * Numeric definition, for host and device buffers alike:
 *   MPIX_F32, MPIX_F64  IEEE add
 *   MPIX_F16            the correctly rounded half sum, rounded once
 *   MPIX_BF16           round-to-nearest-even to bf16 of the f32 sum of the
 *                       two widened values (what torch computes on the CPU)
 *   MPIX_I32, MPIX_I64  two's-complement wrap
 *   MPIX_MAX, MPIX_MIN  the larger / smaller value
 * NaNs and the sign of a zero result under MAX/MIN are unspecified; subnormal
 * f32 and bf16 results follow the compiler's default denormal mode.
 *
 * Requests behave like those of the plain receives: stream and graph queues,
 * captures, fast-wait, MPIX_Wait*_enqueue, MPIX_Wait[all], MPIX_Request_free,
 * the status byte count, unexpected messages; a zero-byte message leaves the
 * buffer untouched.  For partitions: MPIX_Start, MPIX_Parrived on host and
 * device, MPIX_Prequest_create and reuse across iterations are the same
 * calls.  Reuse ACCUMULATES AGAIN on every iteration: a replayed capture or
 * a restarted partitioned request adds to what the buffer holds, so the user
 * resets the buffer between iterations, with work that finished before the
 * receive is triggered (before MPIX_Start for partitions).
 *
 * Several pending reducing receives into the same or overlapping device
 * memory are allowed, provided all of them are reducing (one receive per
 * peer accumulating into one buffer): the library serialises them, and the
 * result depends on arrival order only through float rounding.
 *
 * Errors at the call: MPI_ERR_ARG for an unknown type or op, a buf that is
 * not aligned to the element size, a negative count; MPI_ERR_TYPE for a
 * communicator served by the MPI passthrough and under
 * MPIX_MPI_PARTITIONED=1.  As the completion status, with the sender still
 * acked and completing: MPI_ERR_TRUNCATE for a message longer than the
 * buffer (the elements that fit are combined); MPI_ERR_TYPE, the buffer
 * untouched, when the message length is not a multiple of the element size,
 * a device sender's source address is not element-aligned, the sender's
 * message is strided (for MPIX_Irecv_reduce_enqueue and
 * MPIX_Precv_init_reduce; the strided reducing calls below accept one), or
 * one side is in host memory and the other in device memory (a device
 * receive that gets host chunks included).
 * Not supported: user-defined ops.  Reducing into a strided buffer, or from
 * a strided sender: MPIX_Irecv_reduce_strided_enqueue and
 * MPIX_Precv_init_reduce_strided below. */
enum { MPIX_F32, MPIX_F64, MPIX_BF16, MPIX_F16, MPIX_I32, MPIX_I64 };
enum { MPIX_SUM, MPIX_MAX, MPIX_MIN };

int MPIX_Irecv_reduce_enqueue(void *buf, int count, int type, int op,
                              int source, int tag, MPI_Comm comm,
                              MPIX_Request *request, int qtype, void *queue);

/* Strided reducing receive: the message is combined into a buffer laid out
 * as *layout (mpix_layout.h): the boundary face of a grid, a sub-block of a
 * pitched matrix.  On completion every whole element i of the message, in
 * the layout's (plane, run, byte) order, has been combined once into the
 * buffer at the layout's offset of its position; bytes in the gaps between
 * runs are neither read into the result nor written.  ANY sender matches,
 * whatever the receive's own layout: contiguous or strided, the plain or the
 * strided send calls (only the byte sequence has to agree).  Device buffers
 * are combined inside one strided pull kernel (no staging buffer, no
 * unpack-add kernel behind the wait), host buffers run by run as the chunks
 * arrive.  Numeric definition, request behaviour, reuse (it accumulates
 * again) and overlapping receives are those of MPIX_Irecv_reduce_enqueue.
 * A zero-byte message completes with 0 bytes and no error whatever memory
 * the two sides are in: it touches none.
 * Errors at the call: MPI_ERR_ARG for a null or illegal layout (the rules of
 * the strided calls), an unknown type or op, a buf not aligned to the
 * element size, a run_bytes or a stride in use that is not a multiple of the
 * element size; MPI_ERR_TYPE for a communicator served by the MPI
 * passthrough.  As the completion status, with the sender still acked and
 * completing: MPI_ERR_TRUNCATE for a longer message (the whole elements that
 * fit are combined); MPI_ERR_TYPE, the buffer untouched, when the message
 * length is not a multiple of the element size, when a device sender's
 * address, run or strides in use are not multiples of the element size (an
 * element would straddle two runs), or when one side is in host memory and
 * the other in device memory. */
int MPIX_Irecv_reduce_strided_enqueue(void *buf, const MPIX_Layout *layout,
                                      int type, int op, int source, int tag,
                                      MPI_Comm comm, MPIX_Request *request,
                                      int qtype, void *queue);

int MPIX_Wait_enqueue(MPIX_Request *req, MPI_Status *status, int qtype,
                      void *queue);
int MPIX_Waitall_enqueue(int count, MPIX_Request *reqs, MPI_Status *statuses,
                         int qtype, void *queue);

/* PARTITIONED OPERATIONS ***************************************************/

int MPIX_Psend_init(const void *buf, int partitions, MPI_Count count,
                    MPI_Datatype datatype, int dest, int tag, MPI_Comm comm,
                    MPI_Info info, MPIX_Request *request);

int MPIX_Precv_init(void *buf, int partitions, MPI_Count count,
                    MPI_Datatype datatype, int source, int tag, MPI_Comm comm,
                    MPI_Info info, MPIX_Request *request);

/* Strided variants: partition p is the buffer at buf + p * part_stride laid
 * out as *part_layout (mpix_layout.h), and its message is that layout's
 * bytes in (plane, run, byte) order: a y-face of a grid split along z, a
 * column block of a matrix, rows of a pitched allocation, published slab by
 * slab without a pack kernel.  As with the strided enqueue calls only the
 * byte sequence of a partition has to agree between the two sides: each may
 * use the plain init call, a strided one, or a differently strided one.
 * Everything that takes the request (MPIX_Start, MPIX_Pready, MPIX_Parrived,
 * MPIX_Wait, MPIX_Prequest_create and the __device__ functions, reuse across
 * iterations, MPIX_Request_free) is the same call and behaves the same.  A
 * contiguous layout with part_stride equal to its bytes IS the plain call.
 * Device partitions made ready together are announced as a run and moved by
 * one kernel entry: as one strided message when the run folds into a layout
 * on both sides, by the kernel's partition level otherwise; host partitions
 * are staged one by one.
 * Errors, all at init: MPI_ERR_ARG for a null or illegal layout (as for the
 * enqueue calls) and, with more than one partition, a part_stride that is
 * zero, negative, smaller than the layout's extent (partitions would
 * overlap) or so large that the whole buffer overflows 63 bits;
 * MPI_ERR_TYPE for a communicator or peer served by the MPI passthrough
 * transport and under MPIX_MPI_PARTITIONED=1.  A strided partition between
 * device and host memory completes with MPI_ERR_TYPE, as a strided message.
 * Not supported: partitions of unequal size, a layout per partition, more
 * than two strided levels inside a partition. */
int MPIX_Psend_init_strided(const void *buf, int partitions,
                            const MPIX_Layout *part_layout,
                            int64_t part_stride, int dest, int tag,
                            MPI_Comm comm, MPI_Info info,
                            MPIX_Request *request);

int MPIX_Precv_init_strided(void *buf, int partitions,
                            const MPIX_Layout *part_layout,
                            int64_t part_stride, int source, int tag,
                            MPI_Comm comm, MPI_Info info,
                            MPIX_Request *request);

/* Reducing variant of MPIX_Precv_init: `count` elements of `type` per
 * partition, each arriving partition combined into its slice with `op`
 * (semantics, numeric definition and errors: MPIX_Irecv_reduce_enqueue
 * above).  The sender uses MPIX_Psend_init with the same bytes per partition.
 * Device partitions made ready together are combined by one kernel entry. */
int MPIX_Precv_init_reduce(void *buf, int partitions, MPI_Count count,
                           int type, int op, int source, int tag,
                           MPI_Comm comm, MPI_Info info, MPIX_Request *request);

/* Strided reducing variant: partition p is the buffer at
 * buf + p * part_stride laid out as *part_layout, and each arriving
 * partition is combined into it (semantics and errors:
 * MPIX_Irecv_reduce_strided_enqueue and MPIX_Precv_init_strided; with more
 * than one partition part_stride must be a multiple of the element size
 * too; MPI_ERR_TYPE also under MPIX_MPI_PARTITIONED=1).  The sender uses
 * MPIX_Psend_init or MPIX_Psend_init_strided with the same bytes per
 * partition.  Device partitions made ready together are combined by one
 * kernel entry, folded into one layout where both sides fold and by the
 * kernel's partition level otherwise. */
int MPIX_Precv_init_reduce_strided(void *buf, int partitions,
                                   const MPIX_Layout *part_layout,
                                   int64_t part_stride, int type, int op,
                                   int source, int tag, MPI_Comm comm,
                                   MPI_Info info, MPIX_Request *request);

/* Build a device-resident handle for __device__ MPIX_Pready/Parrived. */
int MPIX_Prequest_create(MPIX_Request request, MPIX_Prequest *prequest);
int MPIX_Prequest_free(MPIX_Prequest *prequest);

/* HELPERS FOR PARTITIONED OPERATIONS ***************************************/

int MPIX_Start(MPIX_Request *request);
int MPIX_Startall(int count, MPIX_Request *request);

int MPIX_Wait(MPIX_Request *req, MPI_Status *status);
int MPIX_Waitall(int count, MPIX_Request *reqs, MPI_Status *statuses);

int MPIX_Request_free(MPIX_Request *request);

/* Host-side partitioned publish / poll (device versions in mpix_device.h).
 * The request argument is void* so one signature serves host (MPIX_Request*)
 * and device (MPIX_Prequest*) — reference parity: mpi-acx.h:96-103. */
int MPIX_Pready(int partition, void *request);
int MPIX_Parrived(void *request, int partition, int *flag);

#ifdef __cplusplus
}
#endif

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
/* device overloads live in mpix_device.h; include it from HIP TUs */
#endif

#endif /* MPIX_H */
