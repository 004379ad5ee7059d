/* Byte-exact reference for the pull kernels (src/transport/pull_kernels.h),
 * and the tables they are run on.  Host only, no HIP: shared by
 * pull_ref_check.cpp (CPU, sanitized: shows that the comparison catches a
 * subtly wrong walk) and pull_kernels_check.hip (the kernels themselves).
 *
 * The reference never goes through a planned table.  A contiguous batch is
 * one plain byte copy per PullSeg; a strided one is, byte by byte,
 *     dst[part_layout_offset(dl, d_part_stride, pos)] =
 *         src[part_layout_offset(sl, s_part_stride, pos)]
 * with layout.h, THE definition of the addressing.  strided_entry_offsets,
 * which is what the kernel computes, is not used in here.
 *
 * An arena stands for the addresses [base, base + size): the tables hold
 * addresses (device pointers in the GPU harness, the host bytes themselves
 * in the CPU check), the reference works on host copies by offset.  Source
 * arenas hold pattern(i) = (i * 7 + 3) % 251 <= 250, destination arenas the
 * sentinel 0xFD, which the pattern never takes: a payload byte that was not
 * written and a sentinel byte that was are both seen.
 */
#ifndef MPIX_TESTS_PULL_REF_H
#define MPIX_TESTS_PULL_REF_H

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../src/transport/pull_plan.h"
#include "../../src/transport/strided_plan.h"

namespace pullref {

using namespace mpix;

static const uint8_t SENTINEL = 0xFD;
static const uint64_t GAP = 64; /* sentinel bytes between destinations */

static inline uint8_t pattern(uint64_t i)
{
    return (uint8_t)((i * 7 + 3) % 251);
}

static inline void fill_src(uint8_t *p, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) p[i] = pattern(i);
}

static inline void fill_dst(uint8_t *p, uint64_t n)
{
    memset(p, SENTINEL, n);
}

struct Arena {
    uint64_t base; /* the address the tables use for byte 0 */
    uint8_t *host;
    uint64_t size;
};

static inline bool arena_holds(const Arena &a, uint64_t addr, uint64_t n)
{
    return addr >= a.base && n <= a.size && addr - a.base <= a.size - n;
}

/* ------------------------------------------------------------ reference */

/* dst.host (sentinel-filled) becomes what the batch must leave behind.
 * owner (optional, dst.size entries of -1) gets the segment each payload
 * byte belongs to.  false: a segment leaves its arena (nothing may be
 * launched then). */
static inline bool ref_contig(const PullSeg *segs, size_t n, const Arena &src,
                              const Arena &dst, std::vector<int32_t> *owner)
{
    for (size_t i = 0; i < n; i++) {
        const uint64_t s = (uint64_t)(uintptr_t)segs[i].src;
        const uint64_t d = (uint64_t)(uintptr_t)segs[i].dst;
        if (!arena_holds(src, s, segs[i].bytes) ||
            !arena_holds(dst, d, segs[i].bytes))
            return false;
        memcpy(dst.host + (d - dst.base), src.host + (s - src.base),
               segs[i].bytes);
        if (owner != nullptr)
            for (uint64_t b = 0; b < segs[i].bytes; b++)
                (*owner)[d - dst.base + b] = (int32_t)i;
    }
    return true;
}

static inline bool ref_strided(const StridedSeg *segs, size_t n,
                               const Arena &src, const Arena &dst,
                               std::vector<int32_t> *owner)
{
    for (size_t i = 0; i < n; i++) {
        const StridedSeg &g = segs[i];
        const int64_t sps = g.parts > 1 ? g.s_part_stride : 0;
        const int64_t dps = g.parts > 1 ? g.d_part_stride : 0;
        for (uint64_t pos = 0; pos < g.bytes; pos++) {
            const uint64_t s = (uint64_t)(uintptr_t)g.src +
                               (uint64_t)part_layout_offset(g.sl, sps, pos);
            const uint64_t d = (uint64_t)(uintptr_t)g.dst +
                               (uint64_t)part_layout_offset(g.dl, dps, pos);
            if (!arena_holds(src, s, 1) || !arena_holds(dst, d, 1))
                return false;
            dst.host[d - dst.base] = src.host[s - src.base];
            if (owner != nullptr) (*owner)[d - dst.base] = (int32_t)i;
        }
    }
    return true;
}

/* -------------------------------------------------------------- compare */

struct Diff {
    uint64_t bad;   /* differing bytes */
    uint64_t first; /* offset of the first one; valid when bad > 0 */
};

static inline Diff compare(const uint8_t *got, const uint8_t *want, uint64_t n)
{
    Diff d{0, 0};
    for (uint64_t i = 0; i < n; i++)
        if (got[i] != want[i] && d.bad++ == 0) d.first = i;
    return d;
}

/* where in the destination arena offset `off` lies */
static inline std::string classify(const std::vector<int32_t> &owner,
                                   uint64_t off)
{
    char buf[96];
    if (owner[off] >= 0) {
        snprintf(buf, sizeof buf, "payload of segment %d", owner[off]);
        return buf;
    }
    int32_t before = -1, after = -1;
    for (uint64_t i = off; i-- > 0;)
        if (owner[i] >= 0) { before = owner[i]; break; }
    for (uint64_t i = off + 1; i < owner.size(); i++)
        if (owner[i] >= 0) { after = owner[i]; break; }
    if (before < 0 && after < 0)
        return "sentinel, no payload";
    if (before < 0)
        snprintf(buf, sizeof buf, "sentinel before segment %d", after);
    else if (after < 0)
        snprintf(buf, sizeof buf, "sentinel after segment %d", before);
    else
        snprintf(buf, sizeof buf, "sentinel between segments %d and %d",
                 before, after);
    return buf;
}

/* ----------------------------------------------------- contiguous tables */

struct ContigSeg {
    uint64_t dst_off, src_off, bytes;
};

struct ContigCase {
    std::string name;
    std::vector<ContigSeg> segs;
    std::vector<unsigned> blocks; /* 0 stands for "as many as tiles" */
    uint64_t src_size, dst_size;
    uint32_t want_copies; /* what the plan has to come to */
    bool stepping;        /* blocks 3 and 7 must step over whole copies */
};

static inline uint64_t up16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

/* segments placed one after the other: destinations GAP sentinel bytes
 * apart on the 16-byte grid, sources 16 bytes apart, in the order `order`
 * gives (order[i] = rank of segment i among the source addresses) */
static inline void contig_place(ContigCase *c,
                                const std::vector<uint64_t> &lens,
                                const std::vector<size_t> &order)
{
    const size_t n = lens.size();
    std::vector<uint64_t> src_at(n);
    uint64_t s = GAP;
    for (size_t r = 0; r < n; r++)
        for (size_t i = 0; i < n; i++)
            if (order[i] == r) {
                src_at[i] = s;
                s += up16(lens[i]) + 16;
            }
    uint64_t d = GAP;
    for (size_t i = 0; i < n; i++) {
        c->segs.push_back(ContigSeg{d, src_at[i], lens[i]});
        d += up16(lens[i]) + GAP;
    }
    c->src_size = s + GAP;
    c->dst_size = d;
}

static inline std::vector<size_t> ascending(size_t n)
{
    std::vector<size_t> o(n);
    for (size_t i = 0; i < n; i++) o[i] = i;
    return o;
}

/* lengths of full_table: the cycle 16, T, 5, T+16, 2T, T-9, 48, with the
 * entries 24..31 all of one tile; `last` (if not 0) replaces entry 63 */
static inline std::vector<uint64_t> full_table_lens(uint64_t T, uint64_t last)
{
    const uint64_t cyc[7] = {16, T, 5, T + 16, 2 * T, T - 9, 48};
    const uint64_t one[5] = {16, T, 5, T - 9, 48};
    std::vector<uint64_t> lens;
    for (size_t i = 0; i < MPIX_PULL_BATCH; i++)
        lens.push_back(i >= 24 && i < 32 ? one[i % 5] : cyc[i % 7]);
    if (last) lens.back() = last;
    return lens;
}

/* The contiguous tables for unroll U (tile T = 4096 * U).  with_1024 adds
 * full_table_1024: full_table with its last copy replaced by one of 1024
 * tiles, run with the production cap of 1024 blocks. */
static inline std::vector<ContigCase> contig_cases(int U, bool with_1024)
{
    const uint64_t T = 4096ull * (uint64_t)U;
    std::vector<ContigCase> out;
    const struct { const char *name; uint64_t len; } edges[] = {
        {"edges/3", 3},          {"edges/16", 16},
        {"edges/19", 19},        {"edges/T-16", T - 16},
        {"edges/T", T},          {"edges/T+16", T + 16},
        {"edges/T+21", T + 21},  {"edges/3T+21", 3 * T + 21}};
    for (const auto &e : edges) {
        ContigCase c;
        c.name = e.name;
        c.blocks = {1, 2, 0};
        c.want_copies = 1;
        c.stepping = false;
        contig_place(&c, {e.len}, ascending(1));
        out.push_back(c);
    }
    for (int big = 0; big < (with_1024 ? 2 : 1); big++) {
        ContigCase c;
        c.name = big ? "full_table_1024" : "full_table";
        if (big)
            c.blocks = {1024};
        else
            c.blocks = {1, 2, 3, 7, 65, 0};
        c.want_copies = MPIX_PULL_BATCH;
        c.stepping = !big;
        std::vector<size_t> order = ascending(MPIX_PULL_BATCH);
        for (size_t i = 40; i < 48; i++) order[i] = 87 - i; /* descending */
        contig_place(&c, full_table_lens(T, big ? 1024 * T : 0), order);
        out.push_back(c);
    }
    {
        /* eight segments that continue each other on both sides, then one
         * whose destination does not */
        ContigCase c;
        c.name = "merged_run";
        c.blocks = {1, 2, 0};
        c.want_copies = 2;
        c.stepping = false;
        for (uint64_t i = 0; i < 8; i++)
            c.segs.push_back(ContigSeg{GAP + i * 4112, GAP + i * 4112, 4112});
        c.segs.push_back(ContigSeg{GAP + 8 * 4112 + GAP, GAP + 8 * 4112, 4112});
        c.src_size = GAP + 9 * 4112 + GAP;
        c.dst_size = GAP + 9 * 4112 + 2 * GAP;
        out.push_back(c);
    }
    return out;
}

static inline std::vector<PullSeg> contig_segs(const ContigCase &c,
                                               uint64_t src_base,
                                               uint64_t dst_base)
{
    std::vector<PullSeg> v;
    for (const ContigSeg &s : c.segs)
        v.push_back(PullSeg{(void *)(uintptr_t)(dst_base + s.dst_off),
                            (const void *)(uintptr_t)(src_base + s.src_off),
                            s.bytes});
    return v;
}

/* the block counts a case is launched with: 0 becomes `tiles`, nothing
 * exceeds the tiles (as in production) or 1024, each count once */
static inline std::vector<unsigned> resolve_blocks(
    const std::vector<unsigned> &want, uint64_t tiles)
{
    std::vector<unsigned> out;
    for (unsigned b : want) {
        uint64_t v = b == 0 ? tiles : b;
        if (v > tiles) v = tiles;
        if (v > 1024) v = 1024;
        bool seen = false;
        for (unsigned o : out) seen = seen || o == (unsigned)v;
        if (!seen) out.push_back((unsigned)v);
    }
    return out;
}

/* most whole copies any of G blocks steps over between two of its tiles */
static inline uint32_t max_copies_stepped_over(const PullTable &t,
                                               uint64_t tile_bytes, unsigned G)
{
    const uint64_t total = pull_total_tiles(t);
    uint32_t most = 0;
    for (uint64_t b = 0; b < G && b < total; b++) {
        uint32_t prev = 0;
        for (uint64_t tile = b; tile < total; tile += G) {
            uint32_t c;
            uint64_t off, len;
            pull_tile_lookup(t, tile, tile_bytes, &c, &off, &len);
            if (tile != b && c > prev + 1 && c - prev - 1 > most)
                most = c - prev - 1;
            prev = c;
        }
    }
    return most;
}

/* -------------------------------------------------------- strided tables */

struct StridedCaseSeg {
    uint64_t dst_off, src_off;
    MPIX_Layout sl, dl;
    uint32_t parts;
    int64_t s_part_stride, d_part_stride;
    uint32_t want_glog;
};

struct StridedCase {
    std::string name;
    std::vector<StridedCaseSeg> segs;
    uint64_t src_size, dst_size;
    bool has_parts;
    bool ok; /* every layout valid and the two sides of equal length */
};

static inline MPIX_Layout L0(uint64_t bytes) { return layout_contiguous(bytes); }

static inline MPIX_Layout L1(uint64_t run, uint64_t c0, int64_t s0)
{
    MPIX_Layout l;
    l.run_bytes = run;
    l.count[0] = c0;
    l.stride[0] = s0;
    l.count[1] = 1;
    l.stride[1] = s0 * (int64_t)c0;
    return l;
}

static inline MPIX_Layout L2(uint64_t run, uint64_t c0, int64_t s0,
                             uint64_t c1, int64_t s1)
{
    MPIX_Layout l = L1(run, c0, s0);
    l.count[1] = c1;
    l.stride[1] = s1;
    return l;
}

/* place one entry behind the ones already there; s_mis misaligns its source
 * base (for a granule that only the address forces) */
static inline void strided_add(StridedCase *c, uint32_t want_g, MPIX_Layout sl,
                               MPIX_Layout dl, uint32_t parts = 1,
                               int64_t sps = 0, int64_t dps = 0,
                               uint64_t s_mis = 0)
{
    uint64_t sext = 0, dext = 0;
    if (layout_validate(sl, &sext) != 0 || layout_validate(dl, &dext) != 0 ||
        layout_bytes(sl) != layout_bytes(dl) || layout_bytes(sl) == 0)
        c->ok = false;
    if (parts > 1 && ((uint64_t)sps <= sext || (uint64_t)dps <= dext))
        c->ok = false; /* part strides larger than the partition's extent */
    StridedCaseSeg s;
    s.sl = layout_normalize(sl);
    s.dl = layout_normalize(dl);
    s.parts = parts;
    s.s_part_stride = sps;
    s.d_part_stride = dps;
    s.want_glog = 0;
    while ((1u << s.want_glog) < want_g) s.want_glog++;
    s.src_off = up16(c->src_size) + s_mis;
    s.dst_off = up16(c->dst_size);
    c->src_size = s.src_off + (uint64_t)(parts - 1) * (uint64_t)sps + sext + GAP;
    c->dst_size = s.dst_off + (uint64_t)(parts - 1) * (uint64_t)dps + dext + GAP;
    if (parts > 1) c->has_parts = true;
    c->segs.push_back(s);
}

static inline StridedCase strided_begin(const char *name)
{
    StridedCase c;
    c.name = name;
    c.src_size = c.dst_size = GAP;
    c.has_parts = false;
    c.ok = true;
    return c;
}

/* 16 entries without a partition level.  Granules 16 8 4 2 1 16 8 4 2 1 16
 * 2 16 1 8 4: neighbours differ.  The tile is 16384 message bytes. */
static inline StridedCase strided_mixed_granules()
{
    StridedCase c = strided_begin("mixed_granules");
    /* 0: 4112-byte runs straddle the tile end on the vector path; strided
     * to contiguous; one tile + 64 B */
    strided_add(&c, 16, L1(4112, 4, 4128), L0(16448));
    /* 1: contiguous to strided, exactly one tile, 8 from the stride */
    strided_add(&c, 8, L0(16384), L1(64, 256, 72));
    /* 2: 4-byte runs into two levels, below a tile */
    strided_add(&c, 4, L1(4, 1000, 12), L2(20, 10, 28, 20, 300));
    /* 3: one tile + one granule of 2 */
    strided_add(&c, 2, L0(16386), L1(2, 8193, 6));
    /* 4: 7-byte runs over about 2.5 tiles */
    strided_add(&c, 1, L1(7, 5851, 9), L0(40957));
    /* 5: two levels of 4112-byte runs to 8224-byte runs, 2.5 tiles */
    strided_add(&c, 16, L2(4112, 5, 4128, 2, 20640), L1(8224, 5, 8240));
    /* 6: two levels of 8-byte runs, below a tile */
    strided_add(&c, 8, L2(8, 16, 24, 8, 400), L1(128, 8, 136));
    /* 7: one tile + one granule of 4, into 4-byte runs */
    strided_add(&c, 4, L0(16388), L1(4, 4097, 8));
    /* 8: 14-byte runs, about 2.5 tiles */
    strided_add(&c, 2, L1(14, 2926, 18), L0(40964));
    /* 9: exactly one tile, 1 from the source address alone */
    strided_add(&c, 1, L0(16384), L1(64, 256, 67), 1, 0, 0, 1);
    /* 10: exactly one tile, one level to two levels */
    strided_add(&c, 16, L1(256, 64, 512), L2(128, 8, 256, 16, 4096));
    /* 11: 200 B */
    strided_add(&c, 2, L1(2, 100, 4), L1(10, 20, 12));
    /* 12: one tile + one granule of 16 */
    strided_add(&c, 16, L0(16400), L1(16, 1025, 32));
    /* 13: one tile + one byte, 5-byte runs to 3277-byte runs */
    strided_add(&c, 1, L1(5, 3277, 7), L1(3277, 5, 3280));
    /* 14: 4104-byte runs straddle the tile ends, 2.5 tiles */
    strided_add(&c, 8, L1(4104, 10, 4112), L0(41040));
    /* 15: two levels on both sides */
    strided_add(&c, 4, L2(12, 3, 16, 50, 64), L2(36, 5, 40, 10, 256));
    return c;
}

/* 16 entries: the even ones runs of 3 and 5 partitions whose part strides
 * exceed the partition's extent and differ on the two sides, the odd ones
 * plain.  Granules 16 4 8 16 8 1 16 2 16 8 2 16 1 8 4 1. */
static inline StridedCase strided_with_partitions()
{
    StridedCase c = strided_begin("with_partitions");
    strided_add(&c, 16, L1(64, 8, 128), L0(512), 3, 1024, 528);
    strided_add(&c, 4, L0(1000), L1(4, 250, 8));
    /* 20560 B: the partitions end off the tile grid */
    strided_add(&c, 8, L0(4112), L1(2056, 2, 2064), 5, 4128, 4144);
    strided_add(&c, 16, L1(4112, 4, 4128), L0(16448));
    /* 8 only because the source part stride is 1000 */
    strided_add(&c, 8, L1(32, 16, 64), L0(512), 3, 1000, 1024);
    strided_add(&c, 1, L1(7, 100, 9), L0(700));
    strided_add(&c, 16, L2(16, 4, 32, 4, 256), L1(128, 2, 160), 5, 896, 304);
    strided_add(&c, 2, L0(16386), L1(2, 8193, 4));
    /* 1.5 tiles, a partition boundary inside a tile */
    strided_add(&c, 16, L1(4112, 2, 4128), L0(8224), 3, 8256, 8240);
    strided_add(&c, 8, L1(8, 128, 24), L0(1024));
    /* 2 only because the source part stride is 102 */
    strided_add(&c, 2, L0(100), L1(20, 5, 24), 5, 102, 120);
    strided_add(&c, 16, L0(16384), L1(256, 64, 512));
    strided_add(&c, 1, L1(7, 9, 8), L0(63), 3, 75, 64);
    strided_add(&c, 8, L2(24, 3, 32, 25, 128), L2(40, 5, 48, 9, 256));
    /* 1.25 tiles of 4-byte runs */
    strided_add(&c, 4, L1(4, 1024, 8), L1(4, 1024, 12), 5, 8192, 12284);
    strided_add(&c, 1, L0(16385), L1(5, 3277, 7));
    return c;
}

static inline std::vector<StridedSeg> strided_segs(const StridedCase &c,
                                                   uint64_t src_base,
                                                   uint64_t dst_base)
{
    std::vector<StridedSeg> v;
    for (const StridedCaseSeg &s : c.segs) {
        StridedSeg g;
        g.dst = (void *)(uintptr_t)(dst_base + s.dst_off);
        g.src = (const void *)(uintptr_t)(src_base + s.src_off);
        g.bytes = layout_bytes(s.sl) * s.parts;
        g.sl = s.sl;
        g.dl = s.dl;
        g.parts = s.parts;
        g.s_part_stride = s.parts > 1 ? s.s_part_stride : 0;
        g.d_part_stride = s.parts > 1 ? s.d_part_stride : 0;
        v.push_back(g);
    }
    return v;
}

/* Is the plan what the case intends (so that a case cannot degrade into an
 * easier path)?  Empty string: yes. */
static inline std::string strided_plan_mismatch(const StridedCase &c,
                                                const StridedTable &t,
                                                bool force_wide)
{
    char buf[160];
    if (!c.ok) return "case " + c.name + " holds an invalid entry";
    if (t.n != c.segs.size() || t.n != MPIX_STRIDED_BATCH)
        return "case " + c.name + " is not a full table";
    for (uint32_t i = 0; i < t.n; i++) {
        const StridedEntry &e = t.e[i];
        if (e.glog != c.segs[i].want_glog || (e.wide != 0) != force_wide ||
            strided_entry_parts(e) != (c.segs[i].parts > 1)) {
            snprintf(buf, sizeof buf,
                     "%s entry %u: glog %u (want %u) wide %u (want %d) "
                     "parts %d (want %d)", c.name.c_str(), i, e.glog,
                     c.segs[i].want_glog, e.wide, (int)force_wide,
                     (int)strided_entry_parts(e), (int)(c.segs[i].parts > 1));
            return buf;
        }
        if (i > 0 && e.glog == t.e[i - 1].glog) {
            snprintf(buf, sizeof buf, "%s entries %u and %u share a granule",
                     c.name.c_str(), i - 1, i);
            return buf;
        }
    }
    if (strided_plan_parts(t) != c.has_parts)
        return "case " + c.name + ": partition level";
    return "";
}

} /* namespace pullref */

#endif /* MPIX_TESTS_PULL_REF_H */
