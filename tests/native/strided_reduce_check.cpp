/* Stand-alone CPU check of the strided reducing receive: its planner
 * (src/transport/strided_reduce_plan.h), the host combine (layout_reduce_in
 * of src/transport/layout.h) and the reference the GPU harness compares the
 * kernels with (strided_reduce_ref.h).  Built with AddressSanitizer + UBSan
 * by tests/test_strided_reduce_ref.py and run as a program.
 *
 *  - every table of the GPU harness (strided_reduce_kernels_check.hip) is
 *    planned, narrow and wide, and walked on the host exactly as the kernel
 *    walks it (strided_entry_offsets per unit, the combine of reduce.h per
 *    element of the unit): strided_entry_offsets must equal
 *    part_layout_offset for every unit, the unit is 16 bytes or one element
 *    and never between, the tile counts are right, and the walk must leave
 *    the reference's bytes behind, gaps included;
 *  - the batch cut: at overlapping extents, not at touching ones, and at
 *    interleaved ones, with the sequential result;
 *  - which segments the planner refuses (a fraction of an element anywhere);
 *  - layout_reduce_in against the reference for chunk positions that split a
 *    run;
 *  - the comparison itself: five wrong walks must each be flagged.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "strided_reduce_ref.h"

using namespace sredref;

static int g_failed = 0;

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            g_failed++;                                                   \
        }                                                                 \
    } while (0)

enum Mutation {
    MUT_NONE,
    MUT_GAP_WRITTEN,    /* an element stored behind the first run */
    MUT_DROP_LAST_TILE, /* the partial last tile stores dst unchanged */
    MUT_SWAP_OFFSETS,   /* source and destination offsets swapped */
    MUT_NO_QUOTIENT,    /* the partition quotient ignored */
    MUT_TWICE           /* the first element combined twice */
};

/* What the kernel does with one table, on the host.  Returns the number of
 * accesses that left an arena (they are skipped). */
static uint64_t walk_table(const StridedReduceTable &t, bool wide,
                           const Arena &src, const Arena &dst, Mutation mut)
{
    uint64_t outside = 0;
    for (uint32_t c = 0; c < t.n; c++) {
        const StridedEntry &e = t.e[c];
        const uint32_t type = t.type[c], op = t.op[c];
        const uint64_t es = reduce_elem_size((int)type);
        const uint64_t unit = 1ull << e.glog;
        const uint64_t tile_units = T >> e.glog;
        const uint64_t tiles = t.tile_end[c] - (c ? t.tile_end[c - 1] : 0);
        const bool partial = (e.units % tile_units) != 0;
        for (uint64_t u = 0; u < e.units; u++) {
            int64_t soff, doff;
            strided_entry_offsets(e, u, wide, mut != MUT_NO_QUOTIENT, &soff,
                                  &doff);
            if (mut == MUT_SWAP_OFFSETS) {
                const int64_t x = soff;
                soff = doff;
                doff = x;
            }
            const uint64_t s = (uint64_t)(uintptr_t)e.src + (uint64_t)soff;
            const uint64_t d = (uint64_t)(uintptr_t)e.dst + (uint64_t)doff;
            if (!arena_holds(src, s, unit) || !arena_holds(dst, d, unit)) {
                outside++;
                continue;
            }
            if (mut == MUT_DROP_LAST_TILE && partial &&
                u >= (tiles - 1) * tile_units)
                continue;
            for (uint64_t b = 0; b < unit; b += es)
                combine_one(dst.host + (d - dst.base) + b,
                            src.host + (s - src.base) + b, type, op);
            if (mut == MUT_TWICE && u == 0)
                combine_one(dst.host + (d - dst.base),
                            src.host + (s - src.base), type, op);
            if (mut == MUT_GAP_WRITTEN && u == 0 && e.d.stride0 != 0) {
                const uint64_t behind = d + (e.d.run_units << e.glog);
                if (arena_holds(dst, behind, es))
                    memset(dst.host + (behind - dst.base), 0, es);
            }
        }
    }
    return outside;
}

/* 64-byte aligned arena of `size` bytes inside `store` */
static Arena arena_in(std::vector<uint8_t> *store, uint64_t size)
{
    store->assign(size + 64, 0);
    uint8_t *p = store->data();
    p += (64 - ((uintptr_t)p & 63)) & 63;
    return Arena{(uint64_t)(uintptr_t)p, p, size};
}

struct Prepared {
    std::vector<uint8_t> src_store, init_store, want_store, got_store;
    Arena src, init, want, got; /* the last three share `got`'s addresses */
    std::vector<StridedReduceSeg> plan;
};

/* arenas, values and the reference's result for a case; the tables hold the
 * addresses of `got`, which starts as a copy of `init` */
static bool prepare(const Case &c, Prepared *p)
{
    Rng rng;
    p->src = arena_in(&p->src_store, c.src_size);
    p->got = arena_in(&p->got_store, c.dst_size);
    for (uint64_t i = 0; i < c.src_size; i++)
        p->src.host[i] = (uint8_t)(rng.next() >> 32);
    memset(p->got.host, SENTINEL, c.dst_size);
    const std::vector<StridedReduceSeg> ref =
        ref_segs(c, p->src.base, p->got.base);
    if (!c.ok || !fill_values(ref.data(), ref.size(), p->src, p->got, &rng))
        return false;
    p->init = arena_in(&p->init_store, c.dst_size);
    memcpy(p->init.host, p->got.host, c.dst_size);
    p->want = arena_in(&p->want_store, c.dst_size);
    memcpy(p->want.host, p->got.host, c.dst_size);
    /* the reference works on `want` under the addresses of `got` */
    const Arena want_as_got{p->got.base, p->want.host, c.dst_size};
    if (!ref_apply(ref.data(), ref.size(), p->src, want_as_got, nullptr))
        return false;
    bool ok = true;
    p->plan = plan_segs(c, p->src.base, p->got.base, &ok);
    return ok;
}

static uint64_t differing(const Arena &a, const Arena &b)
{
    return pullref::compare(a.host, b.host, a.size).bad;
}

/* plan the case launch by launch and walk every launch */
static void check_case(const Case &c, bool force_wide)
{
    Prepared p;
    if (!prepare(c, &p)) {
        printf("FAILED case %s is not as meant\n", c.name.c_str());
        g_failed++;
        return;
    }
    const std::vector<uint8_t> src_before(p.src.host, p.src.host + p.src.size);
    const std::vector<StridedReduceSeg> ref =
        ref_segs(c, p.src.base, p.got.base);
    uint32_t launches = 0, vec = 0;
    size_t at = 0;
    while (at < p.plan.size()) {
        StridedReduceTable t;
        const size_t n = plan_strided_reduce(p.plan.data() + at,
                                             p.plan.size() - at, force_wide,
                                             &t);
        EXPECT(n > 0 && n == t.n);
        if (n == 0) return;
        launches++;
        uint64_t tiles = 0;
        for (uint32_t i = 0; i < t.n; i++) {
            const StridedEntry &e = t.e[i];
            const StridedReduceSeg &g = ref[at + i];
            const uint64_t es = reduce_elem_size((int)g.type);
            /* the unit rule: 16 bytes, or one element */
            EXPECT(e.glog == 4 || (1ull << e.glog) == es);
            EXPECT((e.glog == 4) == seg_is_vec(p.plan[at + i]));
            vec += e.glog == 4;
            EXPECT((e.units << e.glog) == g.bytes);
            EXPECT((e.wide != 0) == force_wide);
            EXPECT(t.type[i] == g.type && t.op[i] == g.op);
            tiles += (g.bytes + T - 1) / T;
            EXPECT(t.tile_end[i] == tiles);
            /* what the kernel computes against THE definition, for the
             * unfolded segment */
            const int64_t sps = g.parts > 1 ? g.s_part_stride : 0;
            const int64_t dps = g.parts > 1 ? g.d_part_stride : 0;
            uint64_t wrong = 0;
            for (uint64_t u = 0; u < e.units; u++) {
                int64_t soff, doff;
                strided_entry_offsets(e, u, e.wide != 0, true, &soff, &doff);
                wrong += soff != part_layout_offset(g.sl, sps, u << e.glog) ||
                         doff != part_layout_offset(g.dl, dps, u << e.glog);
            }
            EXPECT(wrong == 0);
        }
        EXPECT(strided_reduce_total_tiles(t) == tiles);
        EXPECT(strided_reduce_plan_wide(t) == force_wide);
        EXPECT(walk_table(t, force_wide, p.src, p.got, MUT_NONE) == 0);
        at += n;
    }
    EXPECT(launches == c.want_launches);
    EXPECT(vec == c.want_vec);
    const uint64_t bad = differing(p.got, p.want);
    if (bad) printf("FAILED %s: %lu bytes differ\n", c.name.c_str(),
                    (unsigned long)bad);
    EXPECT(bad == 0);
    EXPECT(memcmp(src_before.data(), p.src.host, p.src.size) == 0);
    /* and something was combined at all (a single element may combine to
     * itself: a maximum that is already there, a sum that rounds back) */
    if (c.segs[0].bytes >= 64) EXPECT(differing(p.got, p.init) > 0);
}

/* ------------------------------------------------------------- batch cut */

static std::vector<size_t> launch_sizes(const Case &c)
{
    Prepared p;
    std::vector<size_t> out;
    if (!prepare(c, &p)) return out;
    size_t at = 0;
    while (at < p.plan.size()) {
        StridedReduceTable t;
        const size_t n = plan_strided_reduce(p.plan.data() + at,
                                             p.plan.size() - at, false, &t);
        if (n == 0) break;
        out.push_back(n);
        at += n;
    }
    return out;
}

static void check_cuts()
{
    /* overlapping extents: a cut; the third only touches the second: none */
    EXPECT((launch_sizes(overlap_case()) == std::vector<size_t>{1, 2}));
    /* interleaved: no shared byte, a cut all the same */
    EXPECT((launch_sizes(interleaved_case()) == std::vector<size_t>{1, 1}));
    EXPECT((launch_sizes(batch17_case()) ==
            std::vector<size_t>{MPIX_STRIDED_BATCH, 1}));
    EXPECT((launch_sizes(batch16_case()) ==
            std::vector<size_t>{MPIX_STRIDED_BATCH}));
    /* the extent of a run of partitions reaches to its last partition */
    StridedReduceSeg g;
    g.dst = (void *)(uintptr_t)0x1000;
    g.src = (const void *)(uintptr_t)0x100000;
    g.sl = L0(512);
    g.dl = L1(64, 8, 128);
    g.bytes = 4 * 512;
    g.parts = 4;
    g.s_part_stride = 512;
    g.d_part_stride = 2048;
    g.type = RED_F32;
    g.op = RED_SUM;
    EXPECT(strided_reduce_dst_extent(g) == 3 * 2048 + 7 * 128 + 64);
    StridedReduceSeg two[2] = {g, g};
    two[1].parts = 1;
    two[1].bytes = 512;
    two[1].s_part_stride = two[1].d_part_stride = 0;
    StridedReduceTable t;
    two[1].dst = (char *)g.dst + 3 * 2048 + 7 * 128 + 62; /* its last bytes */
    two[1].type = RED_BF16; /* aligned for its elements: not the reason */
    EXPECT(plan_strided_reduce(two, 2, false, &t) == 1);
    two[1].dst = (char *)g.dst + 3 * 2048 + 7 * 128 + 64; /* touching */
    EXPECT(plan_strided_reduce(two, 2, false, &t) == 2);
}

/* ---------------------------------------------------- what the plan refuses */

static void check_refusals()
{
    StridedReduceSeg g;
    g.dst = (void *)(uintptr_t)0x1000;
    g.src = (const void *)(uintptr_t)0x2000;
    g.sl = L0(960);
    g.dl = L1(48, 20, 64);
    g.bytes = 960;
    g.type = RED_F32;
    g.op = RED_SUM;
    EXPECT(strided_reduce_glog(g) == 4);
    StridedReduceSeg b = g;
    b.dl = L1(8, 120, 24); /* granule 8, 4-byte elements: the element path */
    EXPECT(strided_reduce_glog(b) == 2);
    b.type = RED_F64;
    EXPECT(strided_reduce_glog(b) == 3);
    b.type = RED_BF16;
    EXPECT(strided_reduce_glog(b) == 1);
    b = g;
    b.bytes = 48 * 3 + 4; /* a truncated message off the 16-byte grid */
    EXPECT(strided_reduce_glog(b) == 2);
    b = g;
    b.dl = L1(6, 160, 8); /* a run that is no multiple of the element */
    EXPECT(strided_reduce_glog(b) == -1);
    b.type = RED_F16;
    EXPECT(strided_reduce_glog(b) == 1);
    b = g;
    b.dl = L1(48, 20, 66); /* a stride */
    EXPECT(strided_reduce_glog(b) == -1);
    b = g;
    b.src = (const void *)(uintptr_t)0x2002; /* an address */
    EXPECT(strided_reduce_glog(b) == -1);
    b = g;
    b.bytes = 958; /* a length */
    EXPECT(strided_reduce_glog(b) == -1);
    b = g;
    b.type = RED_NTYPES;
    EXPECT(strided_reduce_glog(b) == -1);
    b = g;
    b.sl = L0(240);
    b.dl = L1(48, 5, 64);
    b.parts = 4;
    b.s_part_stride = 242; /* a part stride */
    b.d_part_stride = 320;
    EXPECT(strided_reduce_glog(b) == -1);
    b.s_part_stride = 248;
    EXPECT(strided_reduce_glog(b) == 2);
    b.parts = 1; /* part strides count only for a run */
    b.s_part_stride = 242;
    b.bytes = 240;
    EXPECT(strided_reduce_glog(b) == 4);
    /* the plan stops before a segment it refuses */
    StridedReduceSeg two[2] = {g, g};
    two[1].dst = (void *)(uintptr_t)0x8002;
    StridedReduceTable t;
    EXPECT(plan_strided_reduce(two, 2, false, &t) == 1 && t.n == 1);
    EXPECT(plan_strided_reduce(two + 1, 1, false, &t) == 0 && t.n == 0);
}

/* ---------------------------------------------------------- host combine */

/* a message of `bytes` combined into a host buffer laid out as dl, chunk by
 * chunk, against the reference */
static void check_host(uint32_t type, uint32_t op, MPIX_Layout dl,
                       uint64_t bytes, uint64_t chunk)
{
    Case c;
    add(&c, type, op, bytes, L0(bytes), dl);
    Prepared p;
    if (!prepare(c, &p)) {
        printf("FAILED host case is not as meant\n");
        g_failed++;
        return;
    }
    const CaseSeg &s = c.segs[0];
    bool split = false;
    for (uint64_t pos = 0; pos < bytes; pos += chunk) {
        const uint64_t n = bytes - pos < chunk ? bytes - pos : chunk;
        split = split || pos % s.dl.run_bytes != 0;
        layout_reduce_in(p.got.host + s.dst_off, s.dl, pos,
                         p.src.host + s.src_off + pos, n, (int)type, (int)op);
    }
    EXPECT(split); /* a chunk started inside a run */
    EXPECT(differing(p.got, p.want) == 0);
    EXPECT(differing(p.got, p.init) > 0);
}

static void check_host_combine()
{
    check_host(RED_F64, RED_SUM, L1(24, 3000, 40), 72000, 65536);
    check_host(RED_F32, RED_MAX, L1(12, 50, 20), 600, 40);
    check_host(RED_BF16, RED_SUM, L2(6, 3, 8, 5, 40), 90, 16);
    check_host(RED_I64, RED_MIN, L1(48, 10, 64), 480, 104);
    check_host(RED_F16, RED_SUM, L1(6, 50, 10), 150, 64); /* a short message */
    check_host(RED_I32, RED_SUM, L2(20, 4, 24, 6, 128), 480, 28);
}

/* ------------------------------------------------- the check of the check */

static void check_mutation(const char *name, const Case &c, Mutation mut)
{
    Prepared p;
    if (!prepare(c, &p)) {
        printf("FAILED case %s is not as meant\n", c.name.c_str());
        g_failed++;
        return;
    }
    size_t at = 0;
    while (at < p.plan.size()) {
        StridedReduceTable t;
        const size_t n = plan_strided_reduce(p.plan.data() + at,
                                             p.plan.size() - at, false, &t);
        if (n == 0) break;
        (void)walk_table(t, false, p.src, p.got, mut);
        at += n;
    }
    const uint64_t flagged = differing(p.got, p.want);
    printf("%s: %lu bytes flagged\n", name, (unsigned long)flagged);
    EXPECT(flagged > 0);
}

static void check_the_check()
{
    check_mutation("destination gap written", shapes_case(), MUT_GAP_WRITTEN);
    check_mutation("operand dropped in the last partial tile", shapes_case(),
                   MUT_DROP_LAST_TILE);
    check_mutation("source and destination offsets swapped", shapes_case(),
                   MUT_SWAP_OFFSETS);
    check_mutation("partition quotient ignored", parts_case(),
                   MUT_NO_QUOTIENT);
    check_mutation("one element combined twice", shapes_case(), MUT_TWICE);
    /* one wrong element of one entry is enough */
    Case one;
    add(&one, RED_F32, RED_SUM, 48, L0(48), L1(4, 12, 12));
    check_mutation("one element combined twice, one entry", one, MUT_TWICE);
}

int main()
{
    const char *const groups[] = {"edges", "shapes", "parts", "wide", "batch"};
    unsigned long cases = 0;
    for (const char *g : groups) {
        bool wide = false;
        for (const Case &c : cases_of(g, &wide)) {
            check_case(c, wide);
            /* every table also with the other division */
            if (strcmp(g, "edges") != 0) check_case(c, !wide);
            cases++;
        }
    }
    printf("%lu tables planned and walked\n", cases);
    check_cuts();
    check_refusals();
    check_host_combine();
    check_the_check();
    if (g_failed) {
        printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
