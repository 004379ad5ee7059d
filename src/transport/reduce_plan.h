/* mpix — host-side planning of one reducing pull (no HIP dependency).
 *
 * flush_reduce() hands the reducing receives that became ready to
 * plan_reduce(), which turns them into the table k_pull_reduce streams over.
 * It is plan_pulls (pull_plan.h) with two differences:
 *
 *  - an entry carries its element type and op, and consecutive entries merge
 *    only when they continue each other on both sides (the 16-byte rule of
 *    plan_pulls included) AND share type and op;
 *  - the kernel reads the destination, so two entries of one launch must not
 *    share a destination byte: the batch ends BEFORE the first entry whose
 *    destination range overlaps an earlier entry of the batch.  That entry
 *    opens the next launch, on the same stream, so the two combines happen
 *    one after the other and no two blocks ever read-modify-write the same
 *    element.  Ranges that merely touch do not overlap.
 *
 * Every entry is cut into tiles of `tile_bytes`; tile_end[] is the running
 * tile count, as in PullTable.  All arithmetic is 64-bit.
 */
#ifndef MPIX_TRANSPORT_REDUCE_PLAN_H
#define MPIX_TRANSPORT_REDUCE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "pull_plan.h"
#include "reduce.h"

namespace mpix {

/* the tile of the reduce kernels: 256 threads x 4 x 16 B */
#define MPIX_REDUCE_UNROLL 4
#define MPIX_REDUCE_TILE (256ull * MPIX_REDUCE_UNROLL * 16ull)

/* one ready reducing pull, as collected by the transport: bytes > 0 and a
 * multiple of the element size, both addresses element-aligned */
struct ReduceSeg {
    void *dst;
    const void *src;
    uint64_t bytes;
    uint32_t type; /* RedType */
    uint32_t op;   /* RedOp */
};

struct ReduceEntry {
    char *dst;
    const char *src;
    uint64_t bytes;
    uint32_t type;
    uint32_t op;
};

/* Passed BY VALUE as the kernel argument (2568 bytes). */
struct ReduceTable {
    uint32_t n;
    uint32_t _pad;
    uint64_t tile_end[MPIX_PULL_BATCH]; /* tiles in entries 0..i, inclusive */
    ReduceEntry e[MPIX_PULL_BATCH];
};

static inline uint64_t reduce_total_tiles(const ReduceTable &t)
{
    return t.n ? t.tile_end[t.n - 1] : 0;
}

/* do [a, a + an) and [b, b + bn) share a byte?  (an, bn > 0) */
static inline bool reduce_ranges_overlap(uint64_t a, uint64_t an, uint64_t b,
                                         uint64_t bn)
{
    return a < b + bn && b < a + an;
}

/* Plan a prefix of `in` (at most MPIX_PULL_BATCH entries) into `out`.
 * Returns how many entries were consumed: at least 1 for n > 0; fewer than
 * min(n, MPIX_PULL_BATCH) when the next entry's destination overlaps one
 * already in the table. */
static inline size_t plan_reduce(const ReduceSeg *in, size_t n,
                                 uint64_t tile_bytes, ReduceTable *out)
{
    if (n > MPIX_PULL_BATCH) n = MPIX_PULL_BATCH;
    uint32_t nc = 0;
    size_t used = 0;
    for (; used < n; used++) {
        const ReduceSeg &g = in[used];
        char *d = (char *)g.dst;
        const char *s = (const char *)g.src;
        bool overlap = false;
        for (uint32_t c = 0; c < nc && !overlap; c++)
            overlap = reduce_ranges_overlap(
                (uint64_t)(uintptr_t)d, g.bytes,
                (uint64_t)(uintptr_t)out->e[c].dst, out->e[c].bytes);
        if (overlap) break;
        if (nc > 0) {
            ReduceEntry &cur = out->e[nc - 1];
            if ((cur.bytes & 15) == 0 && d == cur.dst + cur.bytes &&
                s == cur.src + cur.bytes && g.type == cur.type &&
                g.op == cur.op) {
                cur.bytes += g.bytes;
                continue;
            }
        }
        out->e[nc] = ReduceEntry{d, s, g.bytes, g.type, g.op};
        nc++;
    }
    uint64_t tiles = 0;
    for (uint32_t c = 0; c < nc; c++) {
        const uint64_t b = out->e[c].bytes;
        tiles += b / tile_bytes + (b % tile_bytes != 0);
        out->tile_end[c] = tiles;
    }
    out->n = nc;
    out->_pad = 0;
    return used;
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_REDUCE_PLAN_H */
