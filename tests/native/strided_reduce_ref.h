/* Byte-exact reference for the strided reduce kernels
 * (k_pull_strided_reduce* of src/transport/pull_kernels.h) and for
 * layout_reduce_in, and the tables they are run on.  Host only, no HIP:
 * shared by strided_reduce_check.cpp (CPU, sanitized: the planner, the host
 * combine, and that the comparison catches a subtly wrong walk) and
 * strided_reduce_kernels_check.hip (the kernels themselves).
 *
 * The reference never goes through a planned table.  Element by element,
 *     d = dst + part_layout_offset(dl, d_part_stride, pos)
 *     s = src + part_layout_offset(sl, s_part_stride, pos)
 *     *d = Red<TYPE>::combine(op, *d, *s)
 * with layout.h, THE definition of the addressing, and reduce.h, THE
 * definition of the combine.  strided_entry_offsets, which is what the kernel
 * computes, is not used in here.  Segments are applied in order, so two that
 * overlap give the sequential result.
 *
 * Arenas as in pull_ref.h.  The source arena holds random bytes and, where a
 * segment reads, finite values of its type; the destination arena holds the
 * sentinel 0xA5 and, where a segment combines, finite values: a gap between
 * two runs that was written is seen, and strided_reduce_check.cpp shows that
 * the comparison also sees an operand that was dropped, an element combined
 * twice and a wrong offset.
 */
#ifndef MPIX_TESTS_STRIDED_REDUCE_REF_H
#define MPIX_TESTS_STRIDED_REDUCE_REF_H

#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../src/transport/strided_reduce_plan.h"
#include "pull_ref.h"

namespace sredref {

using namespace mpix;
using pullref::Arena;
using pullref::arena_holds;
using pullref::L0;
using pullref::L1;
using pullref::L2;
using pullref::up16;

static const uint8_t SENTINEL = 0xA5;
static const uint64_t GAP = 64;     /* sentinel bytes between destinations */
static const uint64_t T = MPIX_STRIDED_TILE;

static const char *const TYPE_NAME[] = {"f32", "f64", "bf16", "f16", "i32",
                                        "i64"};
static const char *const OP_NAME[] = {"sum", "max", "min"};

struct Rng {
    uint64_t s = 0x2545f4914f6cdd1dull;
    uint64_t next()
    {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
};

/* one finite element of `type` at p: sums of any three stay finite and, for
 * f32 and bf16, normal or zero */
static inline void put_value(uint8_t *p, uint32_t type, Rng *rng)
{
    const uint64_t r = rng->next();
    switch (type) {
    case RED_F32: {
        const float v = (float)((int64_t)(r & 0xffffff) - 0x800000) /
                        (float)(1 << (8 + (r >> 60)));
        memcpy(p, &v, 4);
        break;
    }
    case RED_F64: {
        const double v = (double)((int64_t)(r & 0xffffffffffffull) -
                                  0x800000000000ll) /
                         (double)(1ull << (20 + (r >> 59)));
        memcpy(p, &v, 8);
        break;
    }
    case RED_BF16: { /* exponent field 120 .. 135 */
        const uint16_t v = (uint16_t)((r & 0x8000) |
                                      ((120 + ((r >> 16) & 15)) << 7) |
                                      ((r >> 24) & 0x7f));
        memcpy(p, &v, 2);
        break;
    }
    case RED_F16: { /* exponent field 0 (subnormal) .. 28 */
        const uint16_t v = (uint16_t)((r & 0x8000) | (((r >> 16) % 29) << 10) |
                                      ((r >> 24) & 0x3ff));
        memcpy(p, &v, 2);
        break;
    }
    case RED_I32: {
        const uint32_t v = (uint32_t)r;
        memcpy(p, &v, 4);
        break;
    }
    default:
        memcpy(p, &r, 8);
    }
}

template <int TYPE>
static inline void combine_at(uint8_t *d, const uint8_t *s, int op)
{
    typedef typename Red<TYPE>::T E;
    E a, b;
    memcpy(&a, d, sizeof(E));
    memcpy(&b, s, sizeof(E));
    a = Red<TYPE>::combine(op, a, b);
    memcpy(d, &a, sizeof(E));
}

/* *d = *d op *s for one element of `type` */
static inline void combine_one(uint8_t *d, const uint8_t *s, uint32_t type,
                               uint32_t op)
{
    switch (type) {
    case RED_F32: combine_at<RED_F32>(d, s, (int)op); break;
    case RED_F64: combine_at<RED_F64>(d, s, (int)op); break;
    case RED_BF16: combine_at<RED_BF16>(d, s, (int)op); break;
    case RED_F16: combine_at<RED_F16>(d, s, (int)op); break;
    case RED_I32: combine_at<RED_I32>(d, s, (int)op); break;
    default: combine_at<RED_I64>(d, s, (int)op); break;
    }
}

/* ------------------------------------------------------------ reference */

/* calls f(source address, destination address) for every element of the
 * segment, in message order; false: the segment is not made of elements */
template <typename F>
static inline bool for_elements(const StridedReduceSeg &g, F f)
{
    const uint64_t es = reduce_elem_size((int)g.type);
    if (es == 0 || g.bytes % es != 0) return false;
    const int64_t sps = g.parts > 1 ? g.s_part_stride : 0;
    const int64_t dps = g.parts > 1 ? g.d_part_stride : 0;
    for (uint64_t pos = 0; pos < g.bytes; pos += es) {
        const uint64_t s = (uint64_t)(uintptr_t)g.src +
                           (uint64_t)part_layout_offset(g.sl, sps, pos);
        const uint64_t d = (uint64_t)(uintptr_t)g.dst +
                           (uint64_t)part_layout_offset(g.dl, dps, pos);
        /* an element lies inside one run on both sides */
        if (part_layout_offset(g.sl, sps, pos + es - 1) !=
                part_layout_offset(g.sl, sps, pos) + (int64_t)(es - 1) ||
            part_layout_offset(g.dl, dps, pos + es - 1) !=
                part_layout_offset(g.dl, dps, pos) + (int64_t)(es - 1))
            return false;
        if (!f(s, d)) return false;
    }
    return true;
}

/* finite values where the segments read and combine (before ref_apply) */
static inline bool fill_values(const StridedReduceSeg *segs, size_t n,
                               const Arena &src, const Arena &dst, Rng *rng)
{
    for (size_t i = 0; i < n; i++) {
        const uint64_t es = reduce_elem_size((int)segs[i].type);
        const bool ok = for_elements(segs[i], [&](uint64_t s, uint64_t d) {
            if (!arena_holds(src, s, es) || !arena_holds(dst, d, es))
                return false;
            put_value(src.host + (s - src.base), segs[i].type, rng);
            put_value(dst.host + (d - dst.base), segs[i].type, rng);
            return true;
        });
        if (!ok) return false;
    }
    return true;
}

/* dst.host becomes what the segments, applied in order, must leave behind.
 * owner (optional, dst.size entries of -1) gets the segment each combined
 * byte belongs to.  false: a segment leaves its arena or is not made of
 * whole elements (nothing may be launched then). */
static inline bool ref_apply(const StridedReduceSeg *segs, size_t n,
                             const Arena &src, const Arena &dst,
                             std::vector<int32_t> *owner)
{
    for (size_t i = 0; i < n; i++) {
        const uint64_t es = reduce_elem_size((int)segs[i].type);
        const bool ok = for_elements(segs[i], [&](uint64_t s, uint64_t d) {
            if (!arena_holds(src, s, es) || !arena_holds(dst, d, es))
                return false;
            combine_one(dst.host + (d - dst.base), src.host + (s - src.base),
                        segs[i].type, segs[i].op);
            if (owner != nullptr)
                for (uint64_t b = 0; b < es; b++)
                    (*owner)[d - dst.base + b] = (int32_t)i;
            return true;
        });
        if (!ok) return false;
    }
    return true;
}

/* ---------------------------------------------------------------- tables */

struct CaseSeg {
    uint64_t dst_off, src_off, bytes;
    MPIX_Layout sl, dl; /* normalised */
    uint32_t parts;
    int64_t s_part_stride, d_part_stride;
    uint32_t type, op;
    bool fold; /* handed to the planner folded into one layout per side */
};

struct Case {
    std::string name;
    std::vector<CaseSeg> segs;
    uint64_t src_size = GAP, dst_size = GAP;
    std::vector<unsigned> blocks; /* 0 stands for `tiles` */
    uint32_t want_launches = 1;
    uint32_t want_vec = 0; /* entries on the vector path, all launches */
    bool ok = true;        /* every layout valid, lengths fit */
};

/* Place one segment of `bytes` message bytes behind the ones already there
 * (16-byte aligned plus s_mis / d_mis).  bytes may be shorter than the
 * layouts (a short or a truncated message), never longer.  dst_at != 0 puts
 * the destination at that offset instead (overlapping cases). */
static inline void add(Case *c, uint32_t type, uint32_t op, uint64_t bytes,
                       MPIX_Layout sl, MPIX_Layout dl, uint32_t parts = 1,
                       int64_t sps = 0, int64_t dps = 0, uint64_t s_mis = 0,
                       uint64_t d_mis = 0, bool fold = false,
                       uint64_t dst_at = 0)
{
    uint64_t sext = 0, dext = 0;
    if (layout_validate(sl, &sext) != 0 || layout_validate(dl, &dext) != 0 ||
        bytes == 0 || bytes > layout_bytes(sl) * parts ||
        bytes > layout_bytes(dl) * parts)
        c->ok = false;
    if (parts > 1 && ((uint64_t)sps < sext || (uint64_t)dps < dext ||
                      layout_bytes(sl) != layout_bytes(dl)))
        c->ok = false;
    CaseSeg s;
    s.bytes = bytes;
    s.sl = layout_normalize(sl);
    s.dl = layout_normalize(dl);
    s.parts = parts;
    s.s_part_stride = sps;
    s.d_part_stride = dps;
    s.type = type;
    s.op = op;
    s.fold = fold;
    s.src_off = up16(c->src_size) + s_mis;
    s.dst_off = dst_at ? dst_at : up16(c->dst_size) + d_mis;
    const uint64_t send =
        s.src_off + (uint64_t)(parts - 1) * (uint64_t)sps + sext + GAP;
    const uint64_t dend =
        s.dst_off + (uint64_t)(parts - 1) * (uint64_t)dps + dext + GAP;
    if (send > c->src_size) c->src_size = send;
    if (dend > c->dst_size) c->dst_size = dend;
    c->segs.push_back(s);
}

/* the segments as the reference takes them */
static inline std::vector<StridedReduceSeg> ref_segs(const Case &c,
                                                     uint64_t src_base,
                                                     uint64_t dst_base)
{
    std::vector<StridedReduceSeg> v;
    for (const CaseSeg &s : c.segs) {
        StridedReduceSeg g;
        g.dst = (void *)(uintptr_t)(dst_base + s.dst_off);
        g.src = (const void *)(uintptr_t)(src_base + s.src_off);
        g.bytes = s.bytes;
        g.sl = s.sl;
        g.dl = s.dl;
        g.parts = s.parts;
        g.s_part_stride = s.parts > 1 ? s.s_part_stride : 0;
        g.d_part_stride = s.parts > 1 ? s.d_part_stride : 0;
        g.type = s.type;
        g.op = s.op;
        v.push_back(g);
    }
    return v;
}

/* the segments as the planner takes them: a `fold` one as the transport
 * hands over a run that folds (part_layout_fold on both sides); *ok false
 * when one that should fold does not */
static inline std::vector<StridedReduceSeg> plan_segs(const Case &c,
                                                      uint64_t src_base,
                                                      uint64_t dst_base,
                                                      bool *ok)
{
    std::vector<StridedReduceSeg> v = ref_segs(c, src_base, dst_base);
    *ok = true;
    for (size_t i = 0; i < v.size(); i++) {
        if (!c.segs[i].fold) continue;
        StridedReduceSeg &g = v[i];
        if (!part_layout_fold(c.segs[i].sl, g.parts, g.s_part_stride, &g.sl) ||
            !part_layout_fold(c.segs[i].dl, g.parts, g.d_part_stride, &g.dl))
            *ok = false;
        g.parts = 1;
        g.s_part_stride = g.d_part_stride = 0;
    }
    return v;
}

/* is the segment, as planned, on the vector path? */
static inline bool seg_is_vec(const StridedReduceSeg &g)
{
    return strided_reduce_glog(g) == 4;
}

/* `edges`: one entry per table, contiguous source, strided on the
 * destination only, runs of 1 element and of 48 bytes; for all 18 type/op
 * pairs; 1 element, one 16-byte unit, T - 16, T, T + 16 + 1 element and
 * 3T + an odd number of elements. */
static inline std::vector<Case> edges_cases()
{
    std::vector<Case> out;
    for (uint32_t type = 0; type < RED_NTYPES; type++)
        for (uint32_t op = 0; op < RED_NOPS; op++) {
            const uint64_t es = reduce_elem_size((int)type);
            const struct { const char *name; uint64_t bytes; } sizes[] = {
                {"1el", es}, {"16", 16}, {"T-16", T - 16}, {"T", T},
                {"T+16+1el", T + 16 + es}, {"3T+odd", 3 * T + 1237 * es}};
            for (const auto &z : sizes)
                for (int wide_run = 0; wide_run < 2; wide_run++) {
                    Case c;
                    const uint64_t run = wide_run ? 48 : es;
                    const uint64_t runs = (z.bytes + run - 1) / run;
                    c.name = std::string("edges/") + TYPE_NAME[type] + "/" +
                             OP_NAME[op] + "/" + z.name +
                             (wide_run ? "/run48" : "/run1el");
                    add(&c, type, op, z.bytes, L0(z.bytes),
                        L1(run, runs, wide_run ? 64 : (int64_t)(3 * es)));
                    c.blocks = {1, 2, 0};
                    c.want_vec = wide_run && z.bytes % 16 == 0 ? 1 : 0;
                    out.push_back(c);
                }
        }
    return out;
}

/* `shapes`: ten entries, vector and element path alternating where they can */
static inline Case shapes_case()
{
    Case c;
    c.name = "shapes";
    /* 0: 48-byte runs to contiguous, over a tile (vector) */
    add(&c, RED_F32, RED_SUM, 19200, L1(48, 400, 64), L0(19200));
    /* 1: runs of 3 elements to contiguous (element) */
    add(&c, RED_I32, RED_MIN, 18000, L1(12, 1500, 20), L0(18000));
    /* 2: contiguous to 48-byte runs (vector) */
    add(&c, RED_F64, RED_MAX, 16800, L0(16800), L1(48, 350, 80));
    /* 3: contiguous to two levels, count0 = 3, count1 = 5, runs of 3
     * elements (element) */
    add(&c, RED_F16, RED_SUM, 90, L0(90), L2(6, 3, 8, 5, 40));
    /* 4: runs of T + 16 B to 48-byte runs: runs and tiles straddle each
     * other on both sides (vector) */
    add(&c, RED_BF16, RED_SUM, 3 * (T + 16), L1(T + 16, 3, T + 32),
        L1(48, 1025, 64));
    /* 5: one level against two levels (element: 44 and 24 are no multiples
     * of 16) */
    add(&c, RED_F32, RED_MAX, 6000, L1(20, 300, 24), L2(40, 3, 44, 50, 200));
    /* 6: two levels against one level (vector) */
    add(&c, RED_I64, RED_SUM, 720, L2(48, 3, 64, 5, 256), L1(240, 3, 256));
    /* 7: a destination base offset by one element, everything else on the
     * 16-byte grid (element) */
    add(&c, RED_F64, RED_SUM, 16400, L0(16400), L1(16, 1025, 32), 1, 0, 0, 0,
        8);
    /* 8: contiguous to runs of T + 16 B (vector) */
    add(&c, RED_I32, RED_SUM, 2 * (T + 16), L0(2 * (T + 16)),
        L1(T + 16, 2, T + 48));
    /* 9: a source base offset by one element (element) */
    add(&c, RED_BF16, RED_MIN, 19200, L1(64, 300, 128), L0(19200), 1, 0, 0, 2,
        0);
    c.blocks = {1, 2, 3, 0};
    c.want_vec = 5;
    return c;
}

/* `parts`: run entries of k = 4 with unrelated part strides per side, a
 * folded run, and single messages between them */
static inline Case parts_case()
{
    Case c;
    c.name = "parts";
    /* 0: k = 4, part strides unrelated to the layouts and to each other
     * (vector) */
    add(&c, RED_F32, RED_SUM, 4 * 512, L1(64, 8, 128), L0(512), 4, 1040, 528);
    /* 1: a single message (element) */
    add(&c, RED_I32, RED_MAX, 1000, L0(1000), L1(4, 250, 8));
    /* 2: k = 4 over 1.25 tiles, the partitions end off the tile grid; the
     * source part stride 5144 makes it the element path */
    add(&c, RED_F64, RED_MIN, 4 * 5136, L0(5136), L1(2568, 2, 2576), 4, 5144,
        5168);
    /* 3: a run that folds on both sides: a y-face split along z against
     * rows with a gap (vector) */
    add(&c, RED_BF16, RED_SUM, 4 * 2 * 96, L1(96, 2, 256), L0(192), 4, 512,
        208, 0, 0, true);
    /* 4: a single message (vector) */
    add(&c, RED_I64, RED_SUM, 16448, L1(4112, 4, 4128), L0(16448));
    /* 5: k = 4 of two levels, 2-byte elements (element) */
    add(&c, RED_F16, RED_MAX, 4 * 60, L2(6, 2, 8, 5, 20), L1(30, 2, 34), 4,
        102, 70);
    c.blocks = {1, 2, 3, 0};
    c.want_vec = 3;
    return c;
}

/* `batch`: 16 entries mixing all six types, three ops and both unit sizes */
static inline Case batch16_case()
{
    Case c;
    c.name = "batch16";
    for (uint32_t i = 0; i < MPIX_STRIDED_BATCH; i++) {
        const uint32_t type = i % RED_NTYPES, op = (i / 2) % RED_NOPS;
        const uint64_t es = reduce_elem_size((int)type);
        if (i % 2 == 0) { /* vector: 48-byte runs, a tile and a bit every 6th */
            const uint64_t runs = i % 6 == 0 ? 345 : 7 + i;
            add(&c, type, op, 48 * runs, L0(48 * runs), L1(48, runs, 64));
        } else { /* element: runs of 3 elements */
            const uint64_t runs = i % 5 == 0 ? T / (3 * es) + 5 : 11 * i;
            add(&c, type, op, 3 * es * runs, L1(3 * es, runs, 5 * (int64_t)es),
                L1(3 * es, runs, 4 * (int64_t)es));
        }
    }
    c.blocks = {1, 2, 3, 7, 0};
    c.want_vec = 8;
    return c;
}

/* 17 segments: the 17th goes into a second launch */
static inline Case batch17_case()
{
    Case c;
    c.name = "batch17";
    for (uint32_t i = 0; i < MPIX_STRIDED_BATCH + 1; i++) {
        const uint32_t type = (i + 1) % RED_NTYPES, op = i % RED_NOPS;
        const uint64_t es = reduce_elem_size((int)type);
        add(&c, type, op, 6 * es * (20 + i), L0(6 * es * (20 + i)),
            L1(2 * es, 3 * (20 + i), 3 * (int64_t)es));
    }
    c.blocks = {1, 0};
    c.want_launches = 2;
    c.want_vec = 0;
    return c;
}

/* two faces into overlapping extents: the second reads what the first
 * left, so they must plan to two launches, and the result is the sequential
 * one; then a third whose extent only touches the second's */
static inline Case overlap_case()
{
    Case c;
    c.name = "overlap";
    add(&c, RED_F32, RED_SUM, 48 * 40, L0(48 * 40), L1(48, 40, 64));
    const uint64_t first = c.segs[0].dst_off;
    /* the same face again, shifted by half its length: shares bytes */
    add(&c, RED_F32, RED_SUM, 48 * 40, L0(48 * 40), L1(48, 40, 64), 1, 0, 0,
        0, 0, false, first + 20 * 64);
    /* starts exactly where the extent of the second ends */
    add(&c, RED_F32, RED_MAX, 48 * 10, L0(48 * 10), L1(48, 10, 64), 1, 0, 0,
        0, 0, false, first + 20 * 64 + 39 * 64 + 48);
    c.blocks = {1, 0};
    c.want_launches = 2;
    c.want_vec = 3;
    return c;
}

/* two faces that interleave (the second in the gaps of the first): they
 * share no byte, their extents intersect, and that is a cut all the same */
static inline Case interleaved_case()
{
    Case c;
    c.name = "interleaved";
    add(&c, RED_I32, RED_SUM, 16 * 50, L0(16 * 50), L1(16, 50, 64));
    add(&c, RED_I32, RED_MIN, 16 * 50, L0(16 * 50), L1(16, 50, 64), 1, 0, 0,
        0, 0, false, c.segs[0].dst_off + 32);
    c.blocks = {1, 0};
    c.want_launches = 2;
    c.want_vec = 2;
    return c;
}

/* the tables of a group of the GPU harness; *wide: with 64-bit division */
static inline std::vector<Case> cases_of(const std::string &group, bool *wide)
{
    *wide = group == "wide";
    if (group == "edges") return edges_cases();
    if (group == "shapes") return {shapes_case()};
    if (group == "parts") return {parts_case()};
    if (group == "wide") return {shapes_case(), parts_case()};
    if (group == "batch")
        return {batch16_case(), batch17_case(), overlap_case(),
                interleaved_case()};
    return {};
}

using pullref::resolve_blocks;

} /* namespace sredref */

#endif /* MPIX_TESTS_STRIDED_REDUCE_REF_H */
