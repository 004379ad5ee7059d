/* mpix — strided buffer layout (part of the public API; mpix.h includes this).
 *
 * Kept free of <mpi.h> and of HIP so that host-only tools can use it.
 *
 * A layout is a contiguous innermost run plus up to two strided outer
 * levels.  The message is the byte sequence in (plane, run, byte) order:
 *
 *     for p in [0, count[1])  for r in [0, count[0])  for b in [0, run_bytes)
 *         buffer[p * stride[1] + r * stride[0] + b]
 *
 * and its length is run_bytes * count[0] * count[1].  A level of count 1 is
 * unused; its stride is ignored.  Strides of used levels are positive and no
 * byte may be addressed twice: stride[0] >= run_bytes and stride[1] >=
 * stride[0] * (count[0] - 1) + run_bytes.
 */
#ifndef MPIX_LAYOUT_H
#define MPIX_LAYOUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint64_t run_bytes;   /* contiguous innermost run                    */
    uint64_t count[2];    /* count[0] runs per plane, count[1] planes    */
    int64_t  stride[2];   /* bytes between run starts / plane starts     */
} MPIX_Layout;

#ifdef __cplusplus
}
#endif

#endif /* MPIX_LAYOUT_H */
