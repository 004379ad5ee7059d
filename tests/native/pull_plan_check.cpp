/* Stand-alone check of src/transport/pull_plan.h (host only, no HIP).
 * Built with -fsanitize=address,undefined and run as a program by
 * tests/test_pull_plan.py.  Exit status 0 = every case passed.
 *
 * verify() holds for every case: the copies, read in order, are exactly the
 * consumed entries in arrival order (so every byte keeps its source and its
 * destination and appears once), and the tiles of the prefix, walked in
 * order, cover each copy from byte 0 to its end without gap or overlap. */
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../src/transport/pull_plan.h"

using namespace mpix;

static int g_fail = 0;
static const char *g_case = "";

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "FAIL [%s] %s:%d: %s\n", g_case, __FILE__,     \
                    __LINE__, #cond);                                      \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

/* addresses are only ever compared and offset, never dereferenced */
static char *A(uint64_t a) { return (char *)(uintptr_t)a; }

static const uint64_t SRC = 0x7f0000000000ull; /* 16-aligned bases */
static const uint64_t DST = 0x7e0000000000ull;

static PullSeg seg(uint64_t dst, uint64_t src, uint64_t bytes)
{
    return PullSeg{A(dst), A(src), bytes};
}

static void verify(const std::vector<PullSeg> &in, uint64_t tile,
                   const PullTable &t, size_t used)
{
    size_t want = in.size() < MPIX_PULL_BATCH ? in.size() : MPIX_PULL_BATCH;
    CHECK(used == want);
    CHECK(t.ncopies <= used);
    CHECK((used == 0) == (t.ncopies == 0));
    /* entries -> copies, in order */
    uint32_t c = 0;
    uint64_t o = 0;
    for (size_t i = 0; i < used; i++) {
        CHECK(c < t.ncopies);
        if (c >= t.ncopies) return;
        CHECK((char *)in[i].dst == t.copy[c].dst + o);
        CHECK((const char *)in[i].src == t.copy[c].src + o);
        CHECK(o + in[i].bytes <= t.copy[c].bytes);
        /* an entry may only follow another inside a copy on the 16 B grid */
        CHECK(o % 16 == 0);
        o += in[i].bytes;
        if (o == t.copy[c].bytes) {
            c++;
            o = 0;
        }
    }
    CHECK(c == t.ncopies && o == 0);
    /* tiles -> copies */
    uint64_t total = pull_total_tiles(t);
    uint64_t prev_end = 0;
    for (uint32_t i = 0; i < t.ncopies; i++) {
        CHECK(t.tile_end[i] > prev_end); /* no empty copy */
        prev_end = t.tile_end[i];
    }
    uint32_t cc = 0;
    uint64_t cursor = 0;
    for (uint64_t k = 0; k < total; k++) {
        uint32_t kc;
        uint64_t off, len;
        pull_tile_lookup(t, k, tile, &kc, &off, &len);
        if (kc != cc) {
            CHECK(kc == cc + 1);
            CHECK(cursor == t.copy[cc].bytes);
            cc = kc;
            cursor = 0;
        }
        CHECK(off == cursor);
        CHECK(len > 0 && len <= tile);
        CHECK(off + len <= t.copy[kc].bytes);
        /* only the last tile of a copy may be partial */
        CHECK(len == tile || off + len == t.copy[kc].bytes);
        cursor += len;
        if (g_fail) return;
    }
    if (t.ncopies) {
        CHECK(cc == t.ncopies - 1);
        CHECK(cursor == t.copy[cc].bytes);
    }
}

static PullTable run(const std::vector<PullSeg> &in, uint64_t tile,
                     size_t *used_out = nullptr)
{
    PullTable t;
    size_t used = plan_pulls(in.data(), in.size(), tile, &t);
    verify(in, tile, t, used);
    if (used_out) *used_out = used;
    return t;
}

static void cases(uint64_t tile)
{
    const uint64_t P = 4ull << 20;

    g_case = "empty batch";
    {
        PullTable t = run({}, tile);
        CHECK(t.ncopies == 0 && pull_total_tiles(t) == 0);
    }
    g_case = "one entry";
    {
        PullTable t = run({seg(DST, SRC, 8)}, tile);
        CHECK(t.ncopies == 1 && pull_total_tiles(t) == 1);
        CHECK(t.copy[0].bytes == 8);
    }
    g_case = "64 contiguous entries";
    {
        std::vector<PullSeg> in;
        for (uint64_t i = 0; i < 64; i++)
            in.push_back(seg(DST + i * P, SRC + i * P, P));
        PullTable t = run(in, tile);
        CHECK(t.ncopies == 1);
        CHECK(t.copy[0].bytes == 64 * P);
        CHECK(pull_total_tiles(t) == 64 * P / tile);
    }
    g_case = "gap in source only";
    {
        PullTable t = run({seg(DST, SRC, P), seg(DST + P, SRC + P + 16, P)},
                          tile);
        CHECK(t.ncopies == 2);
    }
    g_case = "gap in destination only";
    {
        PullTable t = run({seg(DST, SRC, P), seg(DST + P + 16, SRC + P, P)},
                          tile);
        CHECK(t.ncopies == 2);
    }
    g_case = "gap in both";
    {
        PullTable t = run({seg(DST, SRC, P),
                           seg(DST + P + 16, SRC + P + 16, P),
                           seg(DST + 2 * P + 16, SRC + 2 * P + 16, P)},
                          tile);
        CHECK(t.ncopies == 2);
        CHECK(t.copy[1].bytes == 2 * P);
    }
    g_case = "length not a multiple of 16 ends its run";
    {
        /* the second entry continues the first exactly, byte for byte, and
         * so does the third the second: only the first pair may merge */
        PullTable t = run({seg(DST, SRC, 4096), seg(DST + 4096, SRC + 4096,
                                                    4100),
                           seg(DST + 8196, SRC + 8196, 4096)},
                          tile);
        CHECK(t.ncopies == 2);
        CHECK(t.copy[0].bytes == 8196);
        CHECK(t.copy[1].bytes == 4096);
    }
    g_case = "reverse address order";
    {
        std::vector<PullSeg> in;
        for (int i = 7; i >= 0; i--)
            in.push_back(seg(DST + (uint64_t)i * 4112,
                             SRC + (uint64_t)i * 4112, 4112));
        PullTable t = run(in, tile);
        CHECK(t.ncopies == 8);
        CHECK(t.copy[0].dst == A(DST + 7 * 4112));
        CHECK(t.copy[7].dst == A(DST));
    }
    g_case = "more than MPIX_PULL_BATCH entries";
    {
        std::vector<PullSeg> in;
        for (uint64_t i = 0; i < MPIX_PULL_BATCH + 7; i++)
            in.push_back(seg(DST + i * 64, SRC + i * 128, 32)); /* no merge */
        size_t used = 0;
        PullTable t = run(in, tile, &used);
        CHECK(used == MPIX_PULL_BATCH);
        CHECK(t.ncopies == MPIX_PULL_BATCH);
        std::vector<PullSeg> rest(in.begin() + used, in.end());
        PullTable t2 = run(rest, tile, &used);
        CHECK(used == 7 && t2.ncopies == 7);
        /* contiguous ones split too, and the run restarts in the next */
        in.clear();
        for (uint64_t i = 0; i < MPIX_PULL_BATCH + 7; i++)
            in.push_back(seg(DST + i * 32, SRC + i * 32, 32));
        PullTable t3 = run(in, tile, &used);
        CHECK(used == MPIX_PULL_BATCH && t3.ncopies == 1);
        CHECK(t3.copy[0].bytes == MPIX_PULL_BATCH * 32);
    }
    g_case = "one tile minus 16, one tile, one tile plus 16";
    {
        PullTable t = run({seg(DST, SRC, tile - 16)}, tile);
        CHECK(pull_total_tiles(t) == 1);
        t = run({seg(DST, SRC, tile)}, tile);
        CHECK(pull_total_tiles(t) == 1);
        t = run({seg(DST, SRC, tile + 16)}, tile);
        CHECK(pull_total_tiles(t) == 2);
        /* the three as separate copies of one batch */
        t = run({seg(DST, SRC, tile - 16),
                 seg(DST + (1ull << 30), SRC + (1ull << 30), tile),
                 seg(DST + (2ull << 30), SRC + (2ull << 30), tile + 16)},
                tile);
        CHECK(t.ncopies == 3);
        CHECK(t.tile_end[0] == 1 && t.tile_end[1] == 2 && t.tile_end[2] == 4);
    }
    g_case = "single 200 GiB entry";
    {
        const uint64_t big = 200ull << 30;
        PullTable t = run({seg(DST, SRC, big + 5)}, tile);
        CHECK(t.ncopies == 1);
        CHECK(pull_total_tiles(t) == big / tile + 1);
        CHECK(pull_total_tiles(t) > (1ull << 22));
        uint32_t c;
        uint64_t off, len;
        pull_tile_lookup(t, big / tile, tile, &c, &off, &len);
        CHECK(c == 0 && off == big && len == 5); /* off is past 2^32 */
    }
}

int main()
{
    cases(256 * 4 * 16);
    cases(256 * 8 * 16);
    if (g_fail) {
        fprintf(stderr, "pull_plan_check: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("pull_plan_check: all cases passed\n");
    return 0;
}
