/* Stand-alone check of tests/native/pull_ref.h (host only, no HIP): does the
 * byte-exact comparison that tests/native/pull_kernels_check.hip applies to
 * the pull kernels catch a subtly wrong kernel?  Built with
 * -fsanitize=address,undefined and run as a program by
 * tests/test_pull_ref.py.  Exit status 0 = every case passed.
 *
 * emu_contig and emu_strided are host emulations of pull_multi_body and
 * pull_strided_body (src/transport/pull_kernels.h), written to mirror the
 * kernel loops: block b of G takes the tiles b, b + G, ..., the c / first /
 * end walk is incremental, a full tile is U vectors per thread and the slow
 * branch is nv vectors plus left & 15 tail bytes; the strided walk calls
 * strided_entry_offsets per unit in the rounds of strided_tile.  Every
 * access goes through Mem, which refuses what leaves the arenas.
 *
 *  1. The unmutated emulation matches the reference for every table of the
 *     GPU harness and every block count used there.
 *  2. Each mutation is flagged by the compare, and nothing outside the
 *     mutated bytes is flagged.  "The mutated bytes" of a run are, for every
 *     tile in which the mutation took effect, the bytes that tile should
 *     have written (by pull_tile_lookup / part_layout_offset) and the bytes
 *     it did write.
 *
 * One line per mutation goes to stdout (profiles/pull_kernels_check.md). */
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "pull_ref.h"

using namespace pullref;

static int g_fail = 0;

#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                  \
            fprintf(stderr, "\n");                                         \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

enum Mut {
    M_NONE,
    M_FIRST_STALE,  /* first not updated when a block steps over a copy */
    M_CUR_STALE,    /* cur not reloaded after the crossing */
    M_NV_ROUNDUP,   /* the partial tile's nv rounded up */
    M_TAIL_DROPPED, /* the left & 15 bytes dropped */
    M_TAIL_SHIFT,   /* the tail written at nv * 16 + threadIdx.x + 1 */
    M_VEC_SHIFT,    /* one vector of a full tile stored 16 B further */
    M_TILE_SKIP,    /* one tile skipped */
    M_GLOG_STALE,   /* unit0 computed with the previous entry's glog */
    M_PART_SRC,     /* the partition quotient applied to the source only */
    M_STRIDE_SWAP,  /* rr * stride0 and p * stride1 exchanged */
    M_BOUND_LE      /* u <= e.units */
};

/* host arenas that the tables address directly */
struct Mem {
    Arena src, dst;
    std::vector<uint8_t> allowed; /* per dst byte: a mutated tile's */
    bool mutated_tile = false;
    uint64_t refused = 0; /* accesses outside the arenas (not carried out) */

    Mem(uint64_t ssize, uint64_t dsize)
    {
        src.size = ssize;
        dst.size = dsize;
        src.host = (uint8_t *)aligned_alloc(256, (ssize + 255) & ~255ull);
        dst.host = (uint8_t *)aligned_alloc(256, (dsize + 255) & ~255ull);
        src.base = (uint64_t)(uintptr_t)src.host;
        dst.base = (uint64_t)(uintptr_t)dst.host;
        fill_src(src.host, ssize);
        fill_dst(dst.host, dsize);
        allowed.assign(dsize, 0);
    }
    ~Mem()
    {
        free(src.host);
        free(dst.host);
    }
    Mem(const Mem &) = delete;
    Mem &operator=(const Mem &) = delete;

    void copy(uint64_t d, uint64_t s, unsigned n)
    {
        if (!arena_holds(src, s, n) || !arena_holds(dst, d, n)) {
            refused++;
            return;
        }
        memcpy(dst.host + (d - dst.base), src.host + (s - src.base), n);
        if (mutated_tile) allow(d, n);
    }
    void allow(uint64_t d, uint64_t n)
    {
        for (uint64_t i = 0; i < n; i++)
            if (arena_holds(dst, d + i, 1)) allowed[d + i - dst.base] = 1;
    }
};

static const int THREADS = 256;

/* pull_multi_body<U, S> for all blocks of a grid of G.  mut_tile: the tile
 * M_VEC_SHIFT and M_TILE_SKIP apply to. */
static void emu_contig(const PullTable &t, int U, unsigned G, Mut m,
                       uint64_t mut_tile, Mem &mem)
{
    const uint64_t TILE = (uint64_t)THREADS * (uint64_t)U * 16;
    const uint64_t total = t.tile_end[t.ncopies - 1];
    for (unsigned block = 0; block < G; block++) {
        uint32_t c = 0;
        uint64_t first = 0, end = t.tile_end[0];
        PullCopy cur = t.copy[0];
        for (uint64_t tile = block; tile < total; tile += G) {
            if (tile >= end) {
                bool stepped = false;
                do {
                    if (m != M_FIRST_STALE || !stepped) first = end;
                    stepped = true;
                    end = t.tile_end[++c];
                } while (tile >= end);
                if (m != M_CUR_STALE) cur = t.copy[c];
            }
            /* what this tile stands for, by the plan's own definition */
            uint32_t rc;
            uint64_t roff, rlen;
            pull_tile_lookup(t, tile, TILE, &rc, &roff, &rlen);
            const uint64_t off = (tile - first) * TILE;
            const uint64_t left = cur.bytes - off;
            const uint64_t s = (uint64_t)(uintptr_t)cur.src + off;
            const uint64_t d = (uint64_t)(uintptr_t)cur.dst + off;
            const bool full = left >= TILE;
            bool hit = cur.dst != t.copy[rc].dst || off != roff;
            if ((m == M_VEC_SHIFT || m == M_TILE_SKIP) && tile == mut_tile)
                hit = true;
            if ((m == M_NV_ROUNDUP || m == M_TAIL_DROPPED ||
                 m == M_TAIL_SHIFT) && !full && (left & 15) != 0)
                hit = true;
            mem.mutated_tile = hit;
            if (hit)
                mem.allow((uint64_t)(uintptr_t)t.copy[rc].dst + roff, rlen);
            if (m == M_TILE_SKIP && tile == mut_tile) continue;
            for (uint32_t tid = 0; tid < (uint32_t)THREADS; tid++) {
                if (full) {
                    for (int k = 0; k < U; k++) {
                        const uint64_t v = tid + (uint64_t)k * THREADS;
                        uint64_t dv = v;
                        if (m == M_VEC_SHIFT && tile == mut_tile &&
                            tid == (uint32_t)THREADS - 1 && k == U - 1)
                            dv = v + 1;
                        mem.copy(d + dv * 16, s + v * 16, 16);
                    }
                } else {
                    uint32_t nv = (uint32_t)(left / 16);
                    if (m == M_NV_ROUNDUP) nv = (uint32_t)((left + 15) / 16);
                    for (uint32_t v = tid; v < nv; v += THREADS)
                        mem.copy(d + (uint64_t)v * 16, s + (uint64_t)v * 16,
                                 16);
                    if (m != M_TAIL_DROPPED && tid < (uint32_t)(left & 15)) {
                        uint64_t b = (uint64_t)nv * 16 + tid;
                        if (m == M_TAIL_SHIFT) b++;
                        mem.copy(d + b, s + b, 1);
                    }
                }
            }
        }
    }
    mem.mutated_tile = false;
}

/* strided_side_offset with the two stride products exchanged */
static int64_t side_offset_swapped(const StridedSide &s, uint64_t u,
                                   uint32_t glog)
{
    const uint64_t r = u / s.run_units, o = u - r * s.run_units;
    const uint64_t p = r / s.count0, rr = r - p * s.count0;
    return (int64_t)rr * s.stride1 + (int64_t)p * s.stride0 +
           (int64_t)(o << glog);
}

/* pull_strided_body<WIDE, PARTS, S> for all blocks of a grid of G */
static void emu_strided(const StridedTable &t, bool wide, bool parts,
                        unsigned G, Mut m, const std::vector<StridedSeg> &segs,
                        Mem &mem)
{
    const int U = MPIX_STRIDED_UNROLL;
    const uint64_t total = t.tile_end[t.n - 1];
    for (unsigned block = 0; block < G; block++) {
        uint32_t c = 0;
        uint64_t first = 0, end = t.tile_end[0];
        StridedEntry cur = t.e[0];
        uint32_t glog_before = cur.glog;
        for (uint64_t tile = block; tile < total; tile += G) {
            if (tile >= end) {
                glog_before = cur.glog;
                do {
                    first = end;
                    end = t.tile_end[++c];
                } while (tile >= end);
                cur = t.e[c];
            }
            uint32_t g0 = cur.glog;
            if (m == M_GLOG_STALE) {
                g0 = glog_before;
                glog_before = cur.glog; /* right from the entry's next tile */
            }
            const uint64_t unit0 = ((tile - first) * MPIX_STRIDED_TILE) >> g0;
            const uint64_t tile_pos = (tile - first) * MPIX_STRIDED_TILE;
            bool hit = unit0 != tile_pos >> cur.glog;
            if (m == M_PART_SRC && strided_entry_parts(cur) &&
                tile_pos + MPIX_STRIDED_TILE > (cur.part_units << cur.glog))
                hit = true;
            /* a one-level side loses its stride0 to the unused stride1 */
            if (m == M_STRIDE_SWAP &&
                (cur.s.stride0 != 0 || cur.s.stride1 != 0 ||
                 cur.d.stride0 != 0 || cur.d.stride1 != 0))
                hit = true;
            if (m == M_BOUND_LE &&
                cur.units < unit0 + (MPIX_STRIDED_TILE >> cur.glog))
                hit = true;
            mem.mutated_tile = hit;
            if (hit) {
                /* the bytes this tile should have written, by layout.h */
                const StridedSeg &g = segs[c];
                for (uint64_t pos = tile_pos;
                     pos < tile_pos + MPIX_STRIDED_TILE && pos < g.bytes;
                     pos++)
                    mem.allow((uint64_t)(uintptr_t)g.dst +
                                  (uint64_t)part_layout_offset(
                                      g.dl, g.d_part_stride, pos), 1);
            }
            const unsigned gran = 1u << cur.glog;
            const int rounds = 16 / (int)gran;
            for (int j = 0; j < rounds; j++)
                for (uint32_t tid = 0; tid < (uint32_t)THREADS; tid++)
                    for (int k = 0; k < U; k++) {
                        const uint64_t u = unit0 +
                            (uint64_t)(j * U + k) * THREADS + tid;
                        const bool ok = m == M_BOUND_LE ? u <= cur.units
                                                        : u < cur.units;
                        if (!ok) continue;
                        int64_t soff, doff;
                        if (m == M_STRIDE_SWAP) {
                            const uint64_t q = u / cur.part_units;
                            const uint64_t ur = u - q * cur.part_units;
                            soff = (int64_t)q * cur.s_part_stride +
                                   side_offset_swapped(cur.s, ur, cur.glog);
                            doff = (int64_t)q * cur.d_part_stride +
                                   side_offset_swapped(cur.d, ur, cur.glog);
                        } else {
                            strided_entry_offsets(cur, u, wide, parts, &soff,
                                                  &doff);
                            if (m == M_PART_SRC && parts) {
                                const uint64_t q = u / cur.part_units;
                                const uint64_t ur = u - q * cur.part_units;
                                doff = strided_side_offset(cur.d, ur, cur.glog,
                                                           true);
                            }
                        }
                        mem.copy((uint64_t)(uintptr_t)cur.dst + (uint64_t)doff,
                                 (uint64_t)(uintptr_t)cur.src + (uint64_t)soff,
                                 gran);
                    }
        }
    }
    mem.mutated_tile = false;
}

/* ------------------------------------------------------------- the runs */

struct Verdict {
    Diff diff;
    uint64_t outside; /* differing bytes that no mutated tile accounts for */
    std::string where;
};

static Verdict judge(const Mem &mem, const Arena &want,
                     const std::vector<int32_t> &owner)
{
    Verdict v;
    v.diff = compare(mem.dst.host, want.host, mem.dst.size);
    v.outside = 0;
    for (uint64_t i = 0; i < mem.dst.size; i++)
        if (mem.dst.host[i] != want.host[i] && !mem.allowed[i]) v.outside++;
    v.where = v.diff.bad ? classify(owner, v.diff.first) : "";
    return v;
}

static void report(const char *mut, const std::string &table, int U,
                   unsigned G, const Verdict &v, uint64_t refused)
{
    printf("MUTATION %-14s table %-16s U %d blocks %-3u flagged %-6lu first "
           "%-7lu (%s) outside %lu refused %lu\n", mut, table.c_str(), U, G,
           (unsigned long)v.diff.bad, (unsigned long)v.diff.first,
           v.where.c_str(), (unsigned long)v.outside, (unsigned long)refused);
}

static const ContigCase *find_case(const std::vector<ContigCase> &cases,
                                   const char *name)
{
    for (const ContigCase &c : cases)
        if (c.name == name) return &c;
    fprintf(stderr, "no table %s\n", name);
    exit(2);
}

/* one contiguous table under one walk; returns the verdict */
static Verdict run_contig(const ContigCase &cc, int U, unsigned G, Mut m,
                          uint64_t mut_tile, uint64_t *refused)
{
    const uint64_t TILE = 4096ull * (uint64_t)U;
    Mem mem(cc.src_size, cc.dst_size);
    std::vector<PullSeg> segs = contig_segs(cc, mem.src.base, mem.dst.base);
    std::vector<uint8_t> want_bytes(cc.dst_size, SENTINEL);
    std::vector<int32_t> owner(cc.dst_size, -1);
    Arena want{mem.dst.base, want_bytes.data(), cc.dst_size};
    CHECK(ref_contig(segs.data(), segs.size(), mem.src, want, &owner),
          "%s leaves its arenas", cc.name.c_str());
    PullTable t;
    CHECK(plan_pulls(segs.data(), segs.size(), TILE, &t) == segs.size(),
          "%s", cc.name.c_str());
    CHECK(t.ncopies == cc.want_copies, "%s: %u copies", cc.name.c_str(),
          t.ncopies);
    emu_contig(t, U, G, m, mut_tile, mem);
    /* the source arena is never written */
    for (uint64_t i = 0; i < cc.src_size; i++)
        if (mem.src.host[i] != pattern(i)) {
            CHECK(false, "%s: source byte %lu changed", cc.name.c_str(),
                  (unsigned long)i);
            break;
        }
    *refused = mem.refused;
    return judge(mem, want, owner);
}

static Verdict run_strided(const StridedCase &sc, bool wide, bool parts,
                           unsigned G, Mut m, uint64_t *refused)
{
    Mem mem(sc.src_size, sc.dst_size);
    std::vector<StridedSeg> segs = strided_segs(sc, mem.src.base, mem.dst.base);
    std::vector<uint8_t> want_bytes(sc.dst_size, SENTINEL);
    std::vector<int32_t> owner(sc.dst_size, -1);
    Arena want{mem.dst.base, want_bytes.data(), sc.dst_size};
    CHECK(ref_strided(segs.data(), segs.size(), mem.src, want, &owner),
          "%s leaves its arenas", sc.name.c_str());
    StridedTable t;
    CHECK(plan_strided(segs.data(), segs.size(), wide, &t) == segs.size(),
          "%s", sc.name.c_str());
    const std::string why = strided_plan_mismatch(sc, t, wide);
    CHECK(why.empty(), "%s", why.c_str());
    emu_strided(t, wide, parts, G, m, segs, mem);
    *refused = mem.refused;
    return judge(mem, want, owner);
}

static uint64_t contig_tiles(const ContigCase &cc, int U)
{
    std::vector<PullSeg> segs = contig_segs(cc, 1 << 20, 1 << 30);
    PullTable t;
    plan_pulls(segs.data(), segs.size(), 4096ull * (uint64_t)U, &t);
    return pull_total_tiles(t);
}

static uint64_t strided_tiles(const StridedCase &sc)
{
    uint64_t tiles = 0;
    for (const StridedCaseSeg &s : sc.segs) {
        const uint64_t b = layout_bytes(s.sl) * s.parts;
        tiles += (b + MPIX_STRIDED_TILE - 1) / MPIX_STRIDED_TILE;
    }
    return tiles;
}

static void unmutated_matches()
{
    unsigned long runs = 0;
    for (int U : {1, 4, 8}) {
        for (const ContigCase &cc : contig_cases(U, U == 1)) {
            const uint64_t tiles = contig_tiles(cc, U);
            for (unsigned G : resolve_blocks(cc.blocks, tiles)) {
                uint64_t refused;
                Verdict v = run_contig(cc, U, G, M_NONE, 0, &refused);
                CHECK(v.diff.bad == 0 && refused == 0,
                      "%s U %d blocks %u: %lu bad, first %lu (%s)",
                      cc.name.c_str(), U, G, (unsigned long)v.diff.bad,
                      (unsigned long)v.diff.first, v.where.c_str());
                runs++;
            }
            if (cc.stepping) {
                std::vector<PullSeg> segs = contig_segs(cc, 1 << 20, 1 << 30);
                PullTable t;
                plan_pulls(segs.data(), segs.size(), 4096ull * U, &t);
                for (unsigned G : {3u, 7u})
                    CHECK(max_copies_stepped_over(t, 4096ull * U, G) >= G - 1,
                          "%s U %d: %u blocks step over %u copies",
                          cc.name.c_str(), U, G,
                          max_copies_stepped_over(t, 4096ull * U, G));
            }
        }
    }
    const StridedCase tables[2] = {strided_mixed_granules(),
                                   strided_with_partitions()};
    for (const StridedCase &sc : tables)
        for (int wide = 0; wide < 2; wide++)
            for (int parts = sc.has_parts ? 1 : 0; parts < 2; parts++) {
                const uint64_t tiles = strided_tiles(sc);
                for (unsigned G : resolve_blocks({1, 2, 3, 0}, tiles)) {
                    uint64_t refused;
                    Verdict v = run_strided(sc, wide != 0, parts != 0, G,
                                            M_NONE, &refused);
                    CHECK(v.diff.bad == 0 && refused == 0,
                          "%s wide %d parts %d blocks %u: %lu bad, first %lu "
                          "(%s)", sc.name.c_str(), wide, parts, G,
                          (unsigned long)v.diff.bad,
                          (unsigned long)v.diff.first, v.where.c_str());
                    runs++;
                }
            }
    printf("unmutated emulation == reference in %lu runs\n", runs);
}

static void flagged(const char *mut, const std::string &table, int U,
                    unsigned G, const Verdict &v, uint64_t refused)
{
    report(mut, table, U, G, v, refused);
    CHECK(v.diff.bad > 0, "%s on %s is not flagged", mut, table.c_str());
    CHECK(v.outside == 0, "%s on %s: %lu bytes flagged outside the mutation",
          mut, table.c_str(), (unsigned long)v.outside);
}

static void mutations_are_flagged()
{
    /* each on the smallest table of the harness where it applies, at U = 1 */
    const std::vector<ContigCase> cases = contig_cases(1, false);
    const struct {
        Mut m;
        const char *name, *table;
        unsigned G;
        uint64_t tile;
    } contig[] = {
        /* 3 blocks over full_table: a block steps over 2 whole copies */
        {M_FIRST_STALE, "first_stale", "full_table", 3, 0},
        /* two copies, one block: the crossing into the second */
        {M_CUR_STALE, "cur_stale", "merged_run", 1, 0},
        {M_NV_ROUNDUP, "nv_roundup", "edges/19", 1, 0},
        {M_TAIL_DROPPED, "tail_dropped", "edges/3", 1, 0},
        {M_TAIL_SHIFT, "tail_shift", "edges/19", 1, 0},
        /* the last vector of the one full tile lands in the sentinel */
        {M_VEC_SHIFT, "vec_shift", "edges/T", 1, 0},
        {M_VEC_SHIFT, "vec_shift", "edges/T+16", 2, 0},
        {M_TILE_SKIP, "tile_skipped", "edges/3T+21", 2, 1},
    };
    for (const auto &x : contig) {
        uint64_t refused;
        Verdict v = run_contig(*find_case(cases, x.table), 1, x.G, x.m, x.tile,
                               &refused);
        flagged(x.name, x.table, 1, x.G, v, refused);
    }
    /* a stale first needs a step over whole copies: with 2 blocks over
     * merged_run there is none, and the mutation must then change nothing
     * (the harness asserts that full_table has such steps) */
    {
        uint64_t refused;
        Verdict v = run_contig(*find_case(cases, "merged_run"), 1, 2,
                               M_FIRST_STALE, 0, &refused);
        CHECK(v.diff.bad == 0, "first_stale without a step over a copy");
    }
    const StridedCase mixed = strided_mixed_granules();
    const StridedCase withp = strided_with_partitions();
    const struct {
        Mut m;
        const char *name;
        const StridedCase *sc;
        bool parts;
        unsigned G;
    } strided[] = {
        /* 3 blocks: a block enters an entry of another granule at a tile
         * that is not its first */
        {M_GLOG_STALE, "glog_stale", &mixed, false, 3},
        {M_PART_SRC, "part_src_only", &withp, true, 1},
        {M_STRIDE_SWAP, "stride_swap", &mixed, false, 1},
        {M_BOUND_LE, "bound_le", &mixed, false, 1},
    };
    for (const auto &x : strided) {
        uint64_t refused;
        Verdict v = run_strided(*x.sc, false, x.parts, x.G, x.m, &refused);
        flagged(x.name, x.sc->name, MPIX_STRIDED_UNROLL, x.G, v, refused);
    }
    /* with one block every entry is entered at its first tile: a stale
     * glog changes nothing there, which is why the harness runs 2 and 3 */
    {
        uint64_t refused;
        Verdict v = run_strided(mixed, false, false, 1, M_GLOG_STALE, &refused);
        CHECK(v.diff.bad == 0, "glog_stale with one block");
    }
}

static void compare_and_classify()
{
    uint8_t a[8] = {1, 2, 3, 4, 5, 6, 7, 8}, b[8] = {1, 2, 9, 4, 5, 0, 7, 8};
    Diff d = compare(a, b, 8);
    CHECK(d.bad == 2 && d.first == 2, "compare");
    CHECK(compare(a, a, 8).bad == 0, "compare equal");
    std::vector<int32_t> owner = {-1, -1, 0, 0, -1, 1, 1, -1};
    CHECK(classify(owner, 0) == "sentinel before segment 0", "classify 0");
    CHECK(classify(owner, 3) == "payload of segment 0", "classify 3");
    CHECK(classify(owner, 4) == "sentinel between segments 0 and 1",
          "classify 4");
    CHECK(classify(owner, 7) == "sentinel after segment 1", "classify 7");
}

int main()
{
    compare_and_classify();
    unmutated_matches();
    mutations_are_flagged();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
