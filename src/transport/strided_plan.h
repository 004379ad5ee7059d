/* mpix — host-side planning of one strided pull launch (no HIP dependency).
 *
 * The companion of pull_plan.h for messages that are strided on either side.
 * Work is indexed in MESSAGE space, in units of the entry's granule
 * (layout_granule: 16, 8, 4, 2 or 1 bytes), so both sides are walked in the
 * same order whatever their shapes.  A tile is MPIX_STRIDED_TILE message
 * bytes; tile_end[] is the running (inclusive) tile count, as in PullTable.
 *
 * Per side the kernel turns a unit index u into
 *     r = u / run_units, o = u % run_units, p = r / count0, rr = r % count0
 *     offset = p * stride1 + rr * stride0 + o * granule
 * which is layout_offset(l, u * granule).  The two divisors are prepared
 * here: while the unit count of an entry fits 31 bits the kernel divides by
 * a 32-bit multiply and shift (StridedDiv); beyond that (`wide`) it uses
 * 64-bit division.  Counts and run lengths larger than the entry are clamped
 * to it, which changes no quotient and makes them fit.
 *
 * An entry may be a RUN of k partitions (part_run.h) of part_units granules
 * each, part strides apart on each side.  Partitions have the same size on
 * both sides, so the split q = u / part_units, u' = u - q * part_units is
 * shared: one more division per unit, then per side
 *     offset = q * part_stride + (the walk above on u')
 * which is part_layout_offset(l, part_stride, u * granule).  Runs and counts
 * are then clamped to part_units.  An entry without a partition level has
 * part_units == units (q is always 0); the kernel variant that carries the
 * third division is launched only when a batch holds a run entry.
 */
#ifndef MPIX_TRANSPORT_STRIDED_PLAN_H
#define MPIX_TRANSPORT_STRIDED_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "layout.h"

namespace mpix {

/* most entries one launch takes; a larger flush splits into several */
#define MPIX_STRIDED_BATCH 16
/* vectors per thread and tile, and the tile: 256 threads x U x 16 B */
#define MPIX_STRIDED_UNROLL 4
#define MPIX_STRIDED_TILE ((uint64_t)256 * MPIX_STRIDED_UNROLL * 16)

/* n / d for 0 <= n < 2^31, 1 <= d < 2^31 as (n * mul) >> shift.
 * With l = ceil(log2 d) and mul = ceil(2^(31+l) / d):
 * 2^(31+l) <= mul * d < 2^(31+l) + 2^l, which makes the quotient exact for
 * every n below 2^31; mul <= 2^32 - 1 and n * mul < 2^63. */
struct StridedDiv {
    uint32_t mul;
    uint32_t shift;
};

static inline StridedDiv strided_div_prepare(uint32_t d)
{
    uint32_t l = 0;
    while (((uint64_t)1 << l) < d) l++;
    StridedDiv f;
    f.shift = 31 + l;
    f.mul = (uint32_t)((((uint64_t)1 << f.shift) + d - 1) / d);
    return f;
}

#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t strided_div(uint32_t n, StridedDiv f)
{
    return (uint32_t)(((uint64_t)n * f.mul) >> f.shift);
}

/* one side of an entry, in units of the granule where it says units */
struct StridedSide {
    uint64_t run_units; /* run_bytes / granule (clamped to the entry) */
    uint64_t count0;    /* runs per plane (clamped to the entry) */
    int64_t stride0;    /* bytes; 0 when the level is unused */
    int64_t stride1;
    StridedDiv d_run;   /* valid when !wide */
    StridedDiv d_cnt;
};

struct StridedEntry {
    char *dst;
    const char *src;
    uint64_t units; /* message length in granules, > 0 */
    StridedSide s;  /* source walk */
    StridedSide d;  /* destination walk */
    uint32_t glog;  /* log2(granule): 4 = vector path, 3..0 = element path */
    uint32_t wide;  /* units >= 2^31: 64-bit division in the kernel */
    /* partition level: units == k * part_units; part_units == units (and the
     * part strides 0) when the entry is one message */
    uint64_t part_units;
    StridedDiv d_part; /* valid when !wide */
    int64_t s_part_stride; /* bytes between partitions at the source */
    int64_t d_part_stride; /* ... at the destination */
};

/* Passed BY VALUE as the kernel argument (2696 bytes). */
struct StridedTable {
    uint32_t n;
    uint32_t _pad;
    uint64_t tile_end[MPIX_STRIDED_BATCH]; /* tiles in entries 0..i */
    StridedEntry e[MPIX_STRIDED_BATCH];
};
static_assert(sizeof(StridedTable) <= 4096,
              "StridedTable travels as the kernel argument (4096-byte limit)");

/* one ready strided pull, as collected by the transport: the first `bytes`
 * message bytes go from `src` (laid out as sl) to `dst` (laid out as dl);
 * both layouts normalised, bytes > 0 and a multiple of `granule`.
 * parts > 1: a run of that many whole partitions, each laid out as sl / dl,
 * s_part_stride / d_part_stride bytes apart; `bytes` is all of them. */
struct StridedSeg {
    void *dst;
    const void *src;
    uint64_t bytes;
    MPIX_Layout sl;
    MPIX_Layout dl;
    uint32_t parts = 1;
    int64_t s_part_stride = 0;
    int64_t d_part_stride = 0;
};

static inline uint64_t strided_total_tiles(const StridedTable &t)
{
    return t.n ? t.tile_end[t.n - 1] : 0;
}

/* buffer offset of unit u on one side: what the kernel computes */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline int64_t strided_side_offset(const StridedSide &s, uint64_t u,
                                          uint32_t glog, bool wide)
{
    uint64_t o, p, rr;
    if (wide) {
        uint64_t r = u / s.run_units;
        o = u - r * s.run_units;
        p = r / s.count0;
        rr = r - p * s.count0;
    } else {
        uint32_t u32 = (uint32_t)u;
        uint32_t r = strided_div(u32, s.d_run);
        o = u32 - r * (uint32_t)s.run_units;
        uint32_t p32 = strided_div(r, s.d_cnt);
        rr = r - p32 * (uint32_t)s.count0;
        p = p32;
    }
    return (int64_t)p * s.stride1 + (int64_t)rr * s.stride0 +
           (int64_t)(o << glog);
}

/* does the entry have a partition level? */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline bool strided_entry_parts(const StridedEntry &e)
{
    return e.part_units < e.units;
}

/* source and destination offsets of unit u of an entry: what the kernel
 * computes.  `parts` false skips the partition split (right only for
 * entries without a partition level). */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline void strided_entry_offsets(const StridedEntry &e, uint64_t u,
                                         bool wide, bool parts,
                                         int64_t *soff, int64_t *doff)
{
    int64_t sb = 0, db = 0;
    if (parts) {
        uint64_t q;
        if (wide)
            q = u / e.part_units;
        else
            q = strided_div((uint32_t)u, e.d_part);
        u -= q * e.part_units;
        sb = (int64_t)q * e.s_part_stride;
        db = (int64_t)q * e.d_part_stride;
    }
    *soff = sb + strided_side_offset(e.s, u, e.glog, wide);
    *doff = db + strided_side_offset(e.d, u, e.glog, wide);
}

static inline void strided_side_prepare(const MPIX_Layout &l, uint64_t units,
                                        uint32_t glog, bool wide,
                                        StridedSide *out)
{
    uint64_t run = l.run_bytes >> glog;
    uint64_t cnt = l.count[0];
    /* every index is below `units`, so a divisor above it acts like it */
    if (run > units) run = units;
    if (cnt > units) cnt = units;
    out->run_units = run;
    out->count0 = cnt;
    out->stride0 = l.count[0] > 1 ? l.stride[0] : 0;
    out->stride1 = l.count[1] > 1 ? l.stride[1] : 0;
    out->d_run = StridedDiv{0, 0};
    out->d_cnt = StridedDiv{0, 0};
    if (!wide) {
        out->d_run = strided_div_prepare((uint32_t)run);
        out->d_cnt = strided_div_prepare((uint32_t)cnt);
    }
}

/* One entry from one segment, walked in units of 1 << glog bytes; the caller
 * chose glog so that the unit divides layout_granule of the segment. */
static inline void strided_entry_prepare(const StridedSeg &g, uint32_t glog,
                                         bool force_wide, StridedEntry *out)
{
    StridedEntry &e = *out;
    const bool parts = g.parts > 1;
    e.dst = (char *)g.dst;
    e.src = (const char *)g.src;
    e.units = g.bytes >> glog;
    e.glog = glog;
    e.wide = (force_wide || e.units >= ((uint64_t)1 << 31)) ? 1 : 0;
    e.part_units = parts ? e.units / g.parts : e.units;
    e.s_part_stride = parts ? g.s_part_stride : 0;
    e.d_part_stride = parts ? g.d_part_stride : 0;
    e.d_part = StridedDiv{0, 0};
    if (!e.wide) e.d_part = strided_div_prepare((uint32_t)e.part_units);
    strided_side_prepare(g.sl, e.part_units, glog, e.wide != 0, &e.s);
    strided_side_prepare(g.dl, e.part_units, glog, e.wide != 0, &e.d);
}

/* layout_granule of a segment: its part strides count only for a run */
static inline uint32_t strided_seg_granule(const StridedSeg &g)
{
    const bool parts = g.parts > 1;
    return layout_granule(g.sl, (uint64_t)(uintptr_t)g.src, g.dl,
                          (uint64_t)(uintptr_t)g.dst,
                          parts ? g.s_part_stride : 0,
                          parts ? g.d_part_stride : 0);
}

/* Plan the first min(n, MPIX_STRIDED_BATCH) entries of `in` into `out`.
 * Returns how many entries were consumed (0 for an empty batch, in which
 * case out->n is 0 and nothing may be launched).  force_wide makes every
 * entry use 64-bit division (a test knob for the path that otherwise needs
 * a message of 2^31 units).  One wide entry makes the whole launch wide
 * (strided_plan_wide): 64-bit division is right for every entry, since
 * run_units and count0 are always filled in. */
static inline size_t plan_strided(const StridedSeg *in, size_t n,
                                  bool force_wide, StridedTable *out)
{
    if (n > MPIX_STRIDED_BATCH) n = MPIX_STRIDED_BATCH;
    uint64_t tiles = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t g = strided_seg_granule(in[i]);
        uint32_t glog = 0;
        while ((1u << glog) < g) glog++;
        strided_entry_prepare(in[i], glog, force_wide, &out->e[i]);
        uint64_t b = in[i].bytes;
        tiles += b / MPIX_STRIDED_TILE + (b % MPIX_STRIDED_TILE != 0);
        out->tile_end[i] = tiles;
    }
    out->n = (uint32_t)n;
    out->_pad = 0;
    return n;
}

/* does this launch need the kernel with the partition level? */
static inline bool strided_plan_parts(const StridedTable &t)
{
    for (uint32_t i = 0; i < t.n; i++)
        if (strided_entry_parts(t.e[i])) return true;
    return false;
}

/* does this launch need the 64-bit-division kernel? */
static inline bool strided_plan_wide(const StridedTable &t)
{
    for (uint32_t i = 0; i < t.n; i++)
        if (t.e[i].wide) return true;
    return false;
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_STRIDED_PLAN_H */
