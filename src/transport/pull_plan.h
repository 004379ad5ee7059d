/* mpix — host-side planning of one batched pull (no HIP dependency).
 *
 * flush_pulls() hands the pulls that became ready in one progress pass to
 * plan_pulls(), which turns them into the copy table k_pull_multi streams
 * over:
 *
 *  - consecutive entries whose source AND destination continue exactly where
 *    the previous entry ended are merged into one copy (partitions are slices
 *    of one buffer, so a pass that sees several of them sees one long run).
 *    A run ends at an entry whose length is not a multiple of 16: the next
 *    entry would start off the 16-byte vector grid of the merged copy.
 *    Merging only ever looks forward, so entries arriving in descending
 *    address order stay separate copies in arrival order;
 *  - every copy is cut into tiles of `tile_bytes`; tile_end[] is the running
 *    (inclusive) tile count, so a block maps a global tile index to
 *    (copy, offset) without touching memory outside the table.  The last
 *    tile of a copy may be partial and carries the n % 16 tail bytes.
 *
 * Only the copy table is merged: status, DONE and ch_done stay per op in
 * the caller.  All arithmetic is 64-bit (device buffers reach 288 GB).
 */
#ifndef MPIX_TRANSPORT_PULL_PLAN_H
#define MPIX_TRANSPORT_PULL_PLAN_H

#include <stddef.h>
#include <stdint.h>

namespace mpix {

/* most entries one launch takes; a larger flush splits into several */
#define MPIX_PULL_BATCH 64

/* one ready pull, as collected by the transport */
struct PullSeg {
    void *dst;
    const void *src;
    uint64_t bytes; /* > 0 */
};

struct PullCopy {
    char *dst;
    const char *src;
    uint64_t bytes;
};

/* Passed BY VALUE as the kernel argument (2056 bytes). */
struct PullTable {
    uint32_t ncopies;
    uint32_t _pad;
    uint64_t tile_end[MPIX_PULL_BATCH]; /* tiles in copies 0..i, inclusive */
    PullCopy copy[MPIX_PULL_BATCH];
};

static inline uint64_t pull_total_tiles(const PullTable &t)
{
    return t.ncopies ? t.tile_end[t.ncopies - 1] : 0;
}

/* What global tile `tile` (< pull_total_tiles) stands for: bytes
 * [*off, *off + *len) of copy *c.  k_pull_multi walks the same mapping
 * incrementally; this form is the definition the plan is checked against. */
static inline void pull_tile_lookup(const PullTable &t, uint64_t tile,
                                    uint64_t tile_bytes, uint32_t *c,
                                    uint64_t *off, uint64_t *len)
{
    uint32_t i = 0;
    while (tile >= t.tile_end[i]) i++;
    uint64_t first = i ? t.tile_end[i - 1] : 0;
    uint64_t o = (tile - first) * tile_bytes;
    uint64_t left = t.copy[i].bytes - o;
    *c = i;
    *off = o;
    *len = left < tile_bytes ? left : tile_bytes;
}

/* Plan the first min(n, MPIX_PULL_BATCH) entries of `in` into `out`.
 * Returns how many entries were consumed (0 for an empty batch, in which
 * case out->ncopies is 0 and nothing may be launched). */
static inline size_t plan_pulls(const PullSeg *in, size_t n,
                                uint64_t tile_bytes, PullTable *out)
{
    if (n > MPIX_PULL_BATCH) n = MPIX_PULL_BATCH;
    uint32_t nc = 0;
    for (size_t i = 0; i < n; i++) {
        char *d = (char *)in[i].dst;
        const char *s = (const char *)in[i].src;
        if (nc > 0) {
            PullCopy &cur = out->copy[nc - 1];
            if ((cur.bytes & 15) == 0 && d == cur.dst + cur.bytes &&
                s == cur.src + cur.bytes) {
                cur.bytes += in[i].bytes;
                continue;
            }
        }
        out->copy[nc].dst = d;
        out->copy[nc].src = s;
        out->copy[nc].bytes = in[i].bytes;
        nc++;
    }
    uint64_t tiles = 0;
    for (uint32_t c = 0; c < nc; c++) {
        uint64_t b = out->copy[c].bytes;
        tiles += b / tile_bytes + (b % tile_bytes != 0);
        out->tile_end[c] = tiles;
    }
    out->ncopies = nc;
    out->_pad = 0;
    return n;
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_PULL_PLAN_H */
