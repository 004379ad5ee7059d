/* mpix — host-side planning of one strided reducing pull (no HIP dependency).
 *
 * flush_strided_reduce() hands the reducing receives that are strided on
 * either side (MPIX_Irecv_reduce_strided_enqueue,
 * MPIX_Precv_init_reduce_strided) to plan_strided_reduce(), which turns them
 * into the table k_pull_strided_reduce walks.  It is plan_strided
 * (strided_plan.h: message-space units, multiply-shift division, the
 * partition level) with three differences:
 *
 *  - an entry carries its element type and op;
 *  - TWO unit sizes only.  When layout_granule of the segment is 16 the unit
 *    is 16 bytes (the vector path: 16 / size elements per unit); in every
 *    other case it is ONE ELEMENT.  The element size always divides the
 *    granule (an element never straddles two runs: the transport rejects
 *    such a message), so granules between the two (8 with 4-byte elements,
 *    4 or 8 with 2-byte ones) are walked element by element;
 *  - the kernel reads the destination, so two entries of one launch must not
 *    share a destination byte: the batch ends BEFORE the first entry whose
 *    destination EXTENT, [dst, dst + (parts - 1) * d_part_stride +
 *    extent(dl)), overlaps the extent of an earlier entry of the batch.  That
 *    entry opens the next launch on the same stream, so the two combines
 *    happen one after the other.  The test is conservative: two interleaved
 *    faces share no byte, but their extents intersect, so they go into
 *    consecutive launches; that is correct and only costs a launch.  Extents
 *    that merely touch do not overlap.
 */
#ifndef MPIX_TRANSPORT_STRIDED_REDUCE_PLAN_H
#define MPIX_TRANSPORT_STRIDED_REDUCE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "reduce.h"
#include "reduce_plan.h"
#include "strided_plan.h"

namespace mpix {

/* one ready strided reducing pull: a StridedSeg whose bytes, runs, strides
 * in use, part strides and addresses are multiples of the element size */
struct StridedReduceSeg : StridedSeg {
    uint32_t type = 0; /* RedType */
    uint32_t op = 0;   /* RedOp */
};

/* Passed BY VALUE as the kernel argument. */
struct StridedReduceTable {
    uint32_t n;
    uint32_t _pad;
    uint64_t tile_end[MPIX_STRIDED_BATCH]; /* tiles in entries 0..i */
    StridedEntry e[MPIX_STRIDED_BATCH];
    uint8_t type[MPIX_STRIDED_BATCH];
    uint8_t op[MPIX_STRIDED_BATCH];
};
static_assert(sizeof(StridedReduceTable) <= 4096,
              "StridedReduceTable travels as the kernel argument (4096-byte "
              "limit)");
static_assert(RED_NTYPES <= 256 && RED_NOPS <= 256, "type and op fit a byte");

static inline uint64_t strided_reduce_total_tiles(const StridedReduceTable &t)
{
    return t.n ? t.tile_end[t.n - 1] : 0;
}

/* bytes from the first to one past the last destination byte of a segment */
static inline uint64_t strided_reduce_dst_extent(const StridedSeg &g)
{
    uint64_t ext = 0;
    (void)layout_validate(g.dl, &ext); /* the transport validated it */
    if (g.parts > 1) ext += (uint64_t)(g.parts - 1) * (uint64_t)g.d_part_stride;
    return ext;
}

/* log2 of the unit the segment is walked in: 4, or log2(element size).
 * -1: the element size does not divide the segment's granule or its length
 * (or the type is unknown): such a segment must not be planned. */
static inline int strided_reduce_glog(const StridedReduceSeg &g)
{
    const uint32_t es = reduce_elem_size((int)g.type);
    if (es == 0 || g.bytes == 0 || g.bytes % es != 0) return -1;
    const uint32_t gran = strided_seg_granule(g);
    if (gran % es != 0) return -1;
    if (gran == 16 && g.bytes % 16 == 0) return 4;
    int glog = 0;
    while ((1u << glog) < es) glog++;
    return glog;
}

/* Plan a prefix of `in` (at most MPIX_STRIDED_BATCH entries) into `out`.
 * Returns how many entries were consumed: at least 1 for n > 0, fewer than
 * min(n, MPIX_STRIDED_BATCH) when the next entry's destination extent
 * overlaps one already in the table.  Precondition, checked: every segment
 * has strided_reduce_glog() >= 0; the plan stops before one that has not
 * (0 when it is the first: out->n is 0 and nothing may be launched).
 * force_wide and the wide rule are plan_strided's. */
static inline size_t plan_strided_reduce(const StridedReduceSeg *in, size_t n,
                                         bool force_wide,
                                         StridedReduceTable *out)
{
    if (n > MPIX_STRIDED_BATCH) n = MPIX_STRIDED_BATCH;
    uint64_t tiles = 0;
    uint64_t ext[MPIX_STRIDED_BATCH];
    size_t used = 0;
    for (; used < n; used++) {
        const StridedReduceSeg &g = in[used];
        const int glog = strided_reduce_glog(g);
        if (glog < 0) break;
        ext[used] = strided_reduce_dst_extent(g);
        bool overlap = false;
        for (size_t c = 0; c < used && !overlap; c++)
            overlap = reduce_ranges_overlap(
                (uint64_t)(uintptr_t)g.dst, ext[used],
                (uint64_t)(uintptr_t)in[c].dst, ext[c]);
        if (overlap) break;
        strided_entry_prepare(g, (uint32_t)glog, force_wide, &out->e[used]);
        out->type[used] = (uint8_t)g.type;
        out->op[used] = (uint8_t)g.op;
        tiles += g.bytes / MPIX_STRIDED_TILE + (g.bytes % MPIX_STRIDED_TILE != 0);
        out->tile_end[used] = tiles;
    }
    out->n = (uint32_t)used;
    out->_pad = 0;
    return used;
}

/* does this launch need the 64-bit-division kernel? */
static inline bool strided_reduce_plan_wide(const StridedReduceTable &t)
{
    for (uint32_t i = 0; i < t.n; i++)
        if (t.e[i].wide) return true;
    return false;
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_STRIDED_REDUCE_PLAN_H */
