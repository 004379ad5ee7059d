/* Stand-alone check of src/transport/layout.h and strided_plan.h (host only,
 * no HIP).  Built with -fsanitize=address,undefined and run as a program by
 * tests/test_layout.py.  Exit status 0 = every case passed.
 *
 * brute() is the reference for addressing: it enumerates the layout with
 * three nested loops, straight from its definition. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../src/transport/strided_plan.h"

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

static MPIX_Layout L(uint64_t run, uint64_t c0, uint64_t c1, int64_t s0,
                     int64_t s1)
{
    MPIX_Layout l;
    l.run_bytes = run;
    l.count[0] = c0;
    l.count[1] = c1;
    l.stride[0] = s0;
    l.stride[1] = s1;
    return l;
}

static bool same(const MPIX_Layout &a, const MPIX_Layout &b)
{
    return a.run_bytes == b.run_bytes && a.count[0] == b.count[0] &&
           a.count[1] == b.count[1] && a.stride[0] == b.stride[0] &&
           a.stride[1] == b.stride[1];
}

/* buffer offset of every message byte, by definition */
static std::vector<int64_t> brute(const MPIX_Layout &l)
{
    std::vector<int64_t> v;
    for (uint64_t p = 0; p < l.count[1]; p++)
        for (uint64_t r = 0; r < l.count[0]; r++)
            for (uint64_t b = 0; b < l.run_bytes; b++)
                v.push_back((int64_t)p * l.stride[1] +
                            (int64_t)r * l.stride[0] + (int64_t)b);
    return v;
}

static void test_validate()
{
    g_case = "validate";
    uint64_t ext = 0;
    CHECK(layout_validate(L(4, 5, 6, 32, 160), &ext) == 0);
    CHECK(ext == 5 * 160 + 4 * 32 + 4);
    CHECK(layout_validate(L(16, 1, 1, 0, 0), &ext) == 0 && ext == 16);
    /* unused levels: strides are ignored, whatever they hold */
    CHECK(layout_validate(L(16, 1, 1, -5, -7)) == 0);
    CHECK(layout_validate(L(16, 1, 3, 0, 16), &ext) == 0 && ext == 48);
    /* zero-length */
    CHECK(layout_validate(L(0, 3, 3, 0, 0), &ext) == 0 && ext == 0);
    CHECK(layout_validate(L(8, 0, 3, 8, 8)) == 0);
    /* zero / negative strides of used levels */
    CHECK(layout_validate(L(4, 2, 1, 0, 0)) != 0);
    CHECK(layout_validate(L(4, 2, 1, -8, 0)) != 0);
    CHECK(layout_validate(L(4, 2, 2, 8, 0)) != 0);
    CHECK(layout_validate(L(4, 2, 2, 8, -64)) != 0);
    /* overlap: run level */
    CHECK(layout_validate(L(4, 2, 1, 3, 0)) != 0);
    CHECK(layout_validate(L(4, 2, 1, 4, 0)) == 0);
    /* overlap: plane level must clear stride0*(count0-1)+run = 20 */
    CHECK(layout_validate(L(4, 3, 2, 8, 19)) != 0);
    CHECK(layout_validate(L(4, 3, 2, 8, 20)) == 0);
    /* plane level over an unused run level clears just the run */
    CHECK(layout_validate(L(4, 1, 2, 1000, 4)) == 0);
    CHECK(layout_validate(L(4, 1, 2, 1000, 3)) != 0);
    /* overflowing products */
    CHECK(layout_validate(L(1ull << 32, 1ull << 32, 1, 1ll << 32, 0)) != 0);
    CHECK(layout_validate(L(1ull << 21, 1ull << 21, 1ull << 22, 1ll << 21,
                            1ll << 42)) != 0);
    CHECK(layout_validate(L(1, 1ull << 40, 1, 1ll << 40, 0)) != 0);
    CHECK(layout_validate(L(1, 2, 1ull << 40, 2, 1ll << 40)) != 0);
    CHECK(layout_validate(L(1ull << 63, 1, 1, 0, 0)) != 0);
    CHECK(layout_validate(L(1, 1ull << 62, 1, 1, 0)) == 0);
}

static void test_normalize()
{
    g_case = "normalize";
    /* contiguous in disguise */
    CHECK(same(layout_normalize(L(4, 5, 6, 4, 20)), layout_contiguous(120)));
    CHECK(same(layout_normalize(L(4, 5, 1, 4, 999)), layout_contiguous(20)));
    CHECK(same(layout_normalize(L(4, 1, 6, -3, 4)), layout_contiguous(24)));
    CHECK(same(layout_normalize(L(7, 1, 1, 0, 0)), layout_contiguous(7)));
    CHECK(same(layout_normalize(L(0, 3, 2, 1, 1)), layout_contiguous(0)));
    CHECK(same(layout_normalize(L(8, 0, 2, 8, 64)), layout_contiguous(0)));
    CHECK(layout_is_contiguous(layout_contiguous(0)));
    /* run level merges into the run, plane level moves down */
    CHECK(same(layout_normalize(L(4, 5, 6, 4, 32)), L(20, 6, 1, 32, 192)));
    /* unused run level: plane level moves down */
    CHECK(same(layout_normalize(L(4, 1, 6, 0, 32)), L(4, 6, 1, 32, 192)));
    /* plane level continues the run level at the same pitch */
    CHECK(same(layout_normalize(L(4, 5, 6, 32, 160)), L(4, 30, 1, 32, 960)));
    /* nothing to merge */
    CHECK(same(layout_normalize(L(4, 5, 6, 32, 200)), L(4, 5, 6, 32, 200)));
    /* idempotence and unchanged addressing over a sweep */
    const uint64_t runs[] = {1, 4, 16};
    for (uint64_t run : runs)
        for (uint64_t c0 = 1; c0 <= 3; c0++)
            for (uint64_t c1 = 1; c1 <= 3; c1++)
                for (int64_t p0 = 0; p0 <= 4; p0 += 4)
                    for (int64_t p1 = 0; p1 <= 8; p1 += 8) {
                        int64_t s0 = (int64_t)run + p0;
                        int64_t s1 = s0 * (int64_t)c0 + p1;
                        MPIX_Layout l = L(run, c0, c1, s0, s1);
                        CHECK(layout_validate(l) == 0);
                        MPIX_Layout n = layout_normalize(l);
                        CHECK(layout_validate(n) == 0);
                        CHECK(same(layout_normalize(n), n));
                        CHECK(layout_bytes(n) == layout_bytes(l));
                        CHECK(brute(n) == brute(l));
                        if (p0 == 0 && p1 == 0)
                            CHECK(layout_is_contiguous(n));
                    }
}

static void test_offset()
{
    g_case = "offset";
    const uint64_t runs[] = {1, 4, 7, 16, 48, 4112};
    for (uint64_t run : runs)
        for (uint64_t c0 = 1; c0 <= 5; c0++)
            for (uint64_t c1 = 1; c1 <= 5; c1++)
                for (int pad = 0; pad < 3; pad++) {
                    /* pad 0: dense, 1: padded runs, 2: padded runs + planes */
                    if (run == 4112 && (c0 > 3 || c1 > 2)) continue;
                    int64_t s0 = (int64_t)run + (pad >= 1 ? 5 : 0);
                    int64_t s1 = s0 * (int64_t)c0 + (pad >= 2 ? 11 : 0);
                    MPIX_Layout l = L(run, c0, c1, s0, s1);
                    CHECK(layout_validate(l) == 0);
                    std::vector<int64_t> want = brute(l);
                    CHECK(want.size() == layout_bytes(l));
                    MPIX_Layout n = layout_normalize(l);
                    bool ok = true;
                    for (uint64_t pos = 0; pos < want.size(); pos++) {
                        ok = ok && layout_offset(l, pos) == want[pos];
                        ok = ok && layout_offset(n, pos) == want[pos];
                    }
                    CHECK(ok);
                }
}

static void test_copy()
{
    g_case = "copy";
    /* every (pos, n) of a small two-level layout with padded strides */
    MPIX_Layout l = L(7, 3, 2, 10, 40);
    uint64_t ext = 0;
    CHECK(layout_validate(l, &ext) == 0);
    const uint64_t total = layout_bytes(l);
    std::vector<int64_t> off = brute(l);
    std::vector<unsigned char> buf(ext);
    for (size_t i = 0; i < buf.size(); i++) buf[i] = (unsigned char)(i * 7 + 3);
    for (uint64_t pos = 0; pos <= total; pos++)
        for (uint64_t n = 0; pos + n <= total; n++) {
            /* out: exactly-sized heap block, so ASan sees an overrun */
            std::vector<unsigned char> out(n);
            layout_copy_out(out.data(), buf.data(), l, pos, n);
            bool ok = true;
            for (uint64_t i = 0; i < n; i++)
                ok = ok && out[i] == buf[(size_t)off[pos + i]];
            CHECK(ok);
            /* in: into a sentinel-filled buffer; gaps and the message bytes
             * outside [pos, pos+n) must keep the sentinel */
            std::vector<unsigned char> dst(ext, 0xA5);
            std::vector<unsigned char> src(n);
            for (uint64_t i = 0; i < n; i++) src[i] = (unsigned char)(i + 1);
            layout_copy_in(dst.data(), l, pos, src.data(), n);
            std::vector<int> want(ext, -1);
            for (uint64_t i = 0; i < n; i++)
                want[(size_t)off[pos + i]] = (unsigned char)(i + 1);
            for (size_t b = 0; b < dst.size(); b++)
                ok = ok && dst[b] == (want[b] < 0 ? 0xA5 : want[b]);
            CHECK(ok);
        }
    /* 64 KiB chunks over runs that straddle chunk ends */
    g_case = "copy-chunks";
    MPIX_Layout big = L(400, 300, 1, 512, 0);
    CHECK(layout_validate(big, &ext) == 0);
    std::vector<unsigned char> src(ext), dst(ext, 0xA5), stage(65536);
    for (size_t i = 0; i < src.size(); i++) src[i] = (unsigned char)(i % 251);
    for (uint64_t pos = 0; pos < layout_bytes(big); pos += 65536) {
        uint64_t n = layout_bytes(big) - pos;
        if (n > 65536) n = 65536;
        layout_copy_out(stage.data(), src.data(), big, pos, n);
        layout_copy_in(dst.data(), big, pos, stage.data(), n);
    }
    bool ok = true;
    for (size_t i = 0; i < dst.size(); i++)
        ok = ok && dst[i] == (i % 512 < 400 ? src[i] : 0xA5);
    CHECK(ok);
}

static void test_granule()
{
    g_case = "granule";
    MPIX_Layout v = L(48, 4, 1, 64, 0);
    MPIX_Layout c = layout_contiguous(192);
    CHECK(layout_granule(v, 0x1000, c, 0x2000) == 16);
    CHECK(layout_granule(v, 0x1000, v, 0x2000) == 16);
    /* base misaligned by 8, 4, 2, 1 — on either side */
    CHECK(layout_granule(v, 0x1008, c, 0x2000) == 8);
    CHECK(layout_granule(v, 0x1004, c, 0x2000) == 4);
    CHECK(layout_granule(v, 0x1000, c, 0x2004) == 4);
    CHECK(layout_granule(v, 0x1002, c, 0x2000) == 2);
    CHECK(layout_granule(v, 0x1001, c, 0x2000) == 1);
    CHECK(layout_granule(v, 0x1000, c, 0x2001) == 1);
    /* runs and strides */
    CHECK(layout_granule(L(8, 4, 1, 16, 0), 0, layout_contiguous(32), 0) == 8);
    CHECK(layout_granule(L(4, 30, 1, 32, 0), 0, layout_contiguous(120), 0) == 4);
    CHECK(layout_granule(L(6, 4, 1, 8, 0), 0, layout_contiguous(24), 0) == 2);
    CHECK(layout_granule(L(7, 4, 1, 8, 0), 0, layout_contiguous(28), 0) == 1);
    CHECK(layout_granule(L(16, 4, 1, 20, 0), 0, layout_contiguous(64), 0) == 4);
    CHECK(layout_granule(L(16, 4, 2, 32, 136), 0, layout_contiguous(128), 0) == 8);
    /* strides of unused levels do not count */
    CHECK(layout_granule(L(16, 1, 1, 3, 5), 0, layout_contiguous(16), 0) == 16);
}

static void test_div()
{
    g_case = "div";
    const uint32_t ds[] = {1, 2, 3, 5, 7, 10, 12, 16, 257, 1000, 4112, 65535,
                           65536, 65537, 1u << 30, (1u << 30) + 1,
                           0x7ffffffeu, 0x7fffffffu};
    for (uint32_t d : ds) {
        StridedDiv f = strided_div_prepare(d);
        bool ok = true;
        for (uint32_t n = 0; n < 70000; n++)
            ok = ok && strided_div(n, f) == n / d;
        for (uint32_t k = 1; k < 4000; k++) {
            /* around multiples of d and at the top of the range */
            uint64_t m = (uint64_t)d * (0x7fffffffu / d / 4000 * k);
            for (int e = -2; e <= 2; e++) {
                uint64_t n = m + (uint64_t)(int64_t)e;
                if (n < (1ull << 31))
                    ok = ok && strided_div((uint32_t)n, f) == (uint32_t)n / d;
            }
            uint32_t top = 0x7fffffffu - k;
            ok = ok && strided_div(top, f) == top / d;
        }
        ok = ok && strided_div(0x7fffffffu, f) == 0x7fffffffu / d;
        CHECK(ok);
    }
}

/* every message byte of every entry is covered by exactly one tile, and the
 * kernel's address arithmetic agrees with layout_offset on both sides */
static void verify_plan(const std::vector<StridedSeg> &in, bool force_wide)
{
    StridedTable t;
    memset(&t, 0, sizeof(t));
    size_t used = plan_strided(in.data(), in.size(), force_wide, &t);
    size_t want = in.size() < MPIX_STRIDED_BATCH ? in.size()
                                                 : MPIX_STRIDED_BATCH;
    CHECK(used == want);
    CHECK(t.n == used);
    CHECK(strided_plan_wide(t) == (force_wide && used > 0));
    uint64_t tile = 0;
    for (size_t i = 0; i < used; i++) {
        const StridedEntry &e = t.e[i];
        const uint32_t g = 1u << e.glog;
        CHECK(e.dst == (char *)in[i].dst && e.src == (const char *)in[i].src);
        CHECK(g == layout_granule(in[i].sl, (uintptr_t)in[i].src, in[i].dl,
                                  (uintptr_t)in[i].dst));
        CHECK(e.units * g == in[i].bytes);
        std::vector<unsigned char> hits(in[i].bytes, 0);
        uint64_t first = i ? t.tile_end[i - 1] : 0;
        CHECK(t.tile_end[i] > first);
        bool ok = true;
        for (; tile < t.tile_end[i]; tile++) {
            /* the kernel's walk of one tile */
            uint64_t unit0 = ((tile - first) * MPIX_STRIDED_TILE) >> e.glog;
            uint64_t per_tile = MPIX_STRIDED_TILE >> e.glog;
            CHECK(unit0 < e.units); /* no empty tile */
            for (uint64_t u = unit0; u < unit0 + per_tile && u < e.units; u++) {
                for (uint32_t b = 0; b < g; b++) hits[u * g + b]++;
                bool wide = e.wide != 0;
                ok = ok && strided_side_offset(e.s, u, e.glog, wide) ==
                               layout_offset(in[i].sl, u * g);
                ok = ok && strided_side_offset(e.d, u, e.glog, wide) ==
                               layout_offset(in[i].dl, u * g);
                /* the wide kernel serves narrow entries too */
                ok = ok && strided_side_offset(e.s, u, e.glog, true) ==
                               layout_offset(in[i].sl, u * g);
                /* a unit never leaves its run */
                ok = ok && (u * g) % in[i].sl.run_bytes + g <=
                               in[i].sl.run_bytes;
                ok = ok && (u * g) % in[i].dl.run_bytes + g <=
                               in[i].dl.run_bytes;
            }
        }
        for (unsigned char h : hits) ok = ok && h == 1;
        CHECK(ok);
    }
    CHECK(tile == strided_total_tiles(t));
}

static StridedSeg sseg(uint64_t dst, uint64_t src, uint64_t bytes,
                       MPIX_Layout sl, MPIX_Layout dl)
{
    StridedSeg s;
    s.dst = (void *)(uintptr_t)dst;
    s.src = (const void *)(uintptr_t)src;
    s.bytes = bytes;
    s.sl = layout_normalize(sl);
    s.dl = layout_normalize(dl);
    return s;
}

static void test_plan()
{
    g_case = "plan";
    const uint64_t S = 0x7f0000000000ull, D = 0x7e0000000000ull;
    std::vector<StridedSeg> in;
    verify_plan(in, false); /* empty */
    /* vector path, runs straddling the 16 KiB tile ends */
    in.push_back(sseg(D, S, 4112 * 8, L(4112, 8, 1, 4128, 0),
                      layout_contiguous(4112 * 8)));
    /* two levels on the source, one on the destination */
    in.push_back(sseg(D, S, 3 * 5 * 64, L(64, 5, 3, 96, 768),
                      L(48, 20, 1, 64, 0)));
    /* element paths: 8, 4, 2, 1 */
    in.push_back(sseg(D, S, 8 * 100, L(8, 100, 1, 24, 0),
                      layout_contiguous(800)));
    in.push_back(sseg(D, S, 4 * 30, L(4, 30, 1, 32, 0),
                      layout_contiguous(120)));
    in.push_back(sseg(D, S, 6 * 5000, L(6, 5000, 1, 10, 0),
                      layout_contiguous(30000)));
    in.push_back(sseg(D, S, 7 * 3000, L(7, 3000, 1, 9, 0),
                      L(3, 7000, 1, 5, 0)));
    /* vector-eligible shape, base + 4 */
    in.push_back(sseg(D + 4, S, 48 * 4, L(48, 4, 1, 64, 0),
                      layout_contiguous(192)));
    /* truncated: the first 96 of 160 message bytes; a contiguous side whose
     * run is longer than the entry */
    in.push_back(sseg(D, S, 96, L(16, 10, 1, 32, 0), L(32, 3, 1, 48, 0)));
    in.push_back(sseg(D, S, 64, layout_contiguous(1ull << 40),
                      L(16, 4, 1, 32, 0)));
    /* exactly one tile, one tile + one unit */
    in.push_back(sseg(D, S, 16384, L(128, 128, 1, 256, 0),
                      layout_contiguous(16384)));
    in.push_back(sseg(D, S, 16400, L(16, 1025, 1, 32, 0),
                      layout_contiguous(16400)));
    verify_plan(in, false);
    verify_plan(in, true);
    /* more than one launch's worth: only the first BATCH are consumed */
    while (in.size() < MPIX_STRIDED_BATCH + 3) in.push_back(in[1]);
    verify_plan(in, false);
    /* an entry of 2^31 units is wide without being forced (planned only) */
    g_case = "plan-wide";
    StridedSeg w = sseg(D, S, 1ull << 31, L(1, 1ull << 31, 1, 2, 0),
                        layout_contiguous(1ull << 31));
    StridedTable t;
    memset(&t, 0, sizeof(t));
    CHECK(plan_strided(&w, 1, false, &t) == 1);
    CHECK(t.e[0].glog == 0 && t.e[0].wide == 1 && strided_plan_wide(t));
    CHECK(t.tile_end[0] == (1ull << 31) / MPIX_STRIDED_TILE);
    const uint64_t us[] = {0, 1, (1ull << 31) - 1, 1ull << 30};
    for (uint64_t u : us)
        CHECK(strided_side_offset(t.e[0].s, u, 0, true) ==
              layout_offset(w.sl, u));
    w.bytes = (1ull << 31) - 1;
    CHECK(plan_strided(&w, 1, false, &t) == 1);
    CHECK(t.e[0].wide == 0 && !strided_plan_wide(t));
    for (uint64_t u : us)
        if (u < w.bytes)
            CHECK(strided_side_offset(t.e[0].s, u, 0, false) ==
                  layout_offset(w.sl, u));
}

int main()
{
    test_validate();
    test_normalize();
    test_offset();
    test_copy();
    test_granule();
    test_div();
    test_plan();
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
