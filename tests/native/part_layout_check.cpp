/* Stand-alone check of what treats a RUN of partitions as one transfer
 * (host only, no HIP): part_layout_fold (layout.h), the partition level of
 * the strided plan (strided_plan.h) and the run decisions for strided and
 * gapped partitions (part_run.h).  Built with -fsanitize=address,undefined
 * and run as a program by tests/test_part_layout.py.  Exit status 0 = every
 * case passed.
 *
 * Everything is compared with part_layout_offset(), the one definition of
 * where message byte `pos` of a run of partitions lives. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../src/transport/layout.h"
#include "../../src/transport/part_run.h"
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
    return layout_normalize(l);
}

/* ------------------------------------------------------------------ fold */

/* the folded layout addresses every byte as the definition does */
static bool fold_matches(const MPIX_Layout &l, uint64_t k, int64_t ps,
                         const MPIX_Layout &f)
{
    const uint64_t total = k * layout_bytes(l);
    if (layout_bytes(f) != total) return false;
    if (layout_validate(f) != 0) return false;
    for (uint64_t pos = 0; pos < total; pos++)
        if (layout_offset(f, pos) != part_layout_offset(l, ps, pos))
            return false;
    return true;
}

static void test_offset()
{
    g_case = "part_layout_offset";
    /* by hand: run 48 x 5 @ 80, 2 planes @ 1024, partitions 4096 apart */
    const MPIX_Layout l = L(48, 5, 2, 80, 1024);
    CHECK(layout_bytes(l) == 480);
    CHECK(part_layout_offset(l, 4096, 0) == 0);
    CHECK(part_layout_offset(l, 4096, 47) == 47);
    CHECK(part_layout_offset(l, 4096, 48) == 80);
    CHECK(part_layout_offset(l, 4096, 240) == 1024);
    CHECK(part_layout_offset(l, 4096, 479) == 1024 + 4 * 80 + 47);
    CHECK(part_layout_offset(l, 4096, 480) == 4096);
    CHECK(part_layout_offset(l, 4096, 4 * 480 + 250) ==
          4 * 4096 + 1024 + 10);
    /* one partition: the layout's own addressing */
    for (uint64_t pos = 0; pos < 480; pos++)
        CHECK(part_layout_offset(l, 12345, pos) == layout_offset(l, pos));
}

static void test_fold()
{
    MPIX_Layout f;
    g_case = "fold rows with a gap";
    for (uint64_t k = 1; k <= 8; k++) {
        const MPIX_Layout row = layout_contiguous(4112);
        CHECK(part_layout_fold(row, k, 4352, &f));
        CHECK(fold_matches(row, k, 4352, f));
        if (k > 1)
            CHECK(f.run_bytes == 4112 && f.count[0] == k &&
                  f.stride[0] == 4352 && f.count[1] == 1);
        else
            CHECK(layout_is_contiguous(f));
    }
    g_case = "fold rows without a gap";
    {
        CHECK(part_layout_fold(layout_contiguous(4112), 8, 4112, &f));
        CHECK(layout_is_contiguous(f) && f.run_bytes == 8 * 4112);
        /* overlapping partitions are nobody's layout */
        CHECK(!part_layout_fold(layout_contiguous(4112), 8, 4111, &f));
        CHECK(!part_layout_fold(layout_contiguous(4112), 8, 0, &f));
        CHECK(!part_layout_fold(layout_contiguous(4112), 8, -4352, &f));
    }
    g_case = "fold one level at its pitch";
    {
        /* a y-face split along z: 15 runs of 272 B, 400 apart */
        const MPIX_Layout l = L(272, 15, 1, 400, 0);
        CHECK(part_layout_fold(l, 8, 15 * 400, &f));
        CHECK(fold_matches(l, 8, 15 * 400, f));
        CHECK(f.run_bytes == 272 && f.count[0] == 120 && f.count[1] == 1);
        /* 64 bytes more between partitions: no fold */
        CHECK(!part_layout_fold(l, 8, 15 * 400 + 64, &f));
        CHECK(!part_layout_fold(l, 2, 15 * 400 - 16, &f));
        /* one partition always folds, to itself */
        CHECK(part_layout_fold(l, 1, 15 * 400 + 64, &f));
        CHECK(memcmp(&f, &l, sizeof(f)) == 0);
    }
    g_case = "fold two levels";
    {
        const MPIX_Layout l = L(48, 5, 2, 80, 1024);
        CHECK(l.count[1] == 2); /* really two levels */
        CHECK(part_layout_fold(l, 5, 2 * 1024, &f));
        CHECK(fold_matches(l, 5, 2 * 1024, f));
        CHECK(f.count[1] == 10 && f.count[0] == 5);
        /* any other part stride is refused */
        const int64_t others[] = {2 * 1024 + 16, 4096, 1024 + 5 * 80,
                                  2 * 1024 - 16, 1 << 20};
        for (int64_t ps : others) CHECK(!part_layout_fold(l, 5, ps, &f));
        /* another two-level shape with non-power-of-two numbers */
        const MPIX_Layout m = L(6, 7, 3, 10, 100);
        CHECK(part_layout_fold(m, 4, 300, &f));
        CHECK(fold_matches(m, 4, 300, f));
        CHECK(!part_layout_fold(m, 4, 301, &f));
        CHECK(!part_layout_fold(m, 4, 600, &f));
    }
    g_case = "fold degenerate";
    {
        CHECK(!part_layout_fold(layout_contiguous(0), 4, 64, &f));
        CHECK(!part_layout_fold(layout_contiguous(64), 0, 64, &f));
    }
}

/* ------------------------------------------------------------------ plan */

static StridedSeg rseg(uint64_t dst, uint64_t src, MPIX_Layout sl,
                       int64_t sps, MPIX_Layout dl, int64_t dps, uint32_t k)
{
    StridedSeg s;
    s.dst = (void *)(uintptr_t)dst;
    s.src = (const void *)(uintptr_t)src;
    s.bytes = (uint64_t)k * layout_bytes(sl);
    s.sl = sl;
    s.dl = dl;
    s.parts = k;
    s.s_part_stride = sps;
    s.d_part_stride = dps;
    return s;
}

/* every unit of every entry lands where part_layout_offset says, on both
 * sides, and never leaves its run; returns the granule of entry 0 */
static uint32_t verify_runs(const std::vector<StridedSeg> &in, bool force_wide)
{
    StridedTable t;
    memset(&t, 0, sizeof(t));
    const size_t n = plan_strided(in.data(), in.size(), force_wide, &t);
    CHECK(n == in.size() && t.n == n);
    bool any_parts = false;
    uint64_t tiles = 0;
    for (size_t i = 0; i < n; i++) {
        const StridedEntry &e = t.e[i];
        const StridedSeg &sg = in[i];
        const uint64_t g = 1ull << e.glog;
        const bool parts = sg.parts > 1;
        any_parts = any_parts || parts;
        CHECK(e.units * g == sg.bytes);
        CHECK(strided_entry_parts(e) == parts);
        CHECK(e.wide == (force_wide ? 1u : 0u));
        if (parts) {
            CHECK(e.part_units * sg.parts == e.units);
            CHECK(e.s.run_units <= e.part_units && e.s.count0 <= e.part_units);
            CHECK(e.d.run_units <= e.part_units && e.d.count0 <= e.part_units);
            CHECK((uint64_t)sg.s_part_stride % g == 0);
            CHECK((uint64_t)sg.d_part_stride % g == 0);
        } else {
            CHECK(e.part_units == e.units);
        }
        tiles += sg.bytes / MPIX_STRIDED_TILE +
                 (sg.bytes % MPIX_STRIDED_TILE != 0);
        CHECK(t.tile_end[i] == tiles);
        bool ok = true;
        for (uint64_t u = 0; u < e.units; u++) {
            const int64_t ws = parts
                ? part_layout_offset(sg.sl, sg.s_part_stride, u * g)
                : layout_offset(sg.sl, u * g);
            const int64_t wd = parts
                ? part_layout_offset(sg.dl, sg.d_part_stride, u * g)
                : layout_offset(sg.dl, u * g);
            int64_t so, dof;
            /* the variant with the partition level serves every entry */
            strided_entry_offsets(e, u, e.wide != 0, true, &so, &dof);
            ok = ok && so == ws && dof == wd;
            /* 64-bit division serves narrow entries too */
            strided_entry_offsets(e, u, true, true, &so, &dof);
            ok = ok && so == ws && dof == wd;
            if (!parts) {
                strided_entry_offsets(e, u, e.wide != 0, false, &so, &dof);
                ok = ok && so == ws && dof == wd;
            }
            const uint64_t pb = layout_bytes(sg.sl);
            const uint64_t in_part = (u * g) % (parts ? pb : sg.bytes);
            ok = ok && in_part % sg.sl.run_bytes + g <= sg.sl.run_bytes;
            ok = ok && in_part % sg.dl.run_bytes + g <= sg.dl.run_bytes;
        }
        CHECK(ok);
    }
    CHECK(strided_plan_parts(t) == any_parts);
    CHECK(strided_plan_wide(t) == (force_wide && n > 0));
    return n ? 1u << t.e[0].glog : 0;
}

static void test_plan()
{
    const uint64_t S = 0x7f0000000000ull, D = 0x7e0000000000ull;
    g_case = "plan granule 16";
    {
        std::vector<StridedSeg> in;
        /* two levels with non-power-of-two divisors against contiguous */
        const MPIX_Layout two = L(48, 5, 2, 80, 1024);
        in.push_back(rseg(D, S, two, 4096, layout_contiguous(480), 480, 5));
        /* the other way round */
        in.push_back(rseg(D, S, layout_contiguous(480), 480, two, 4096, 5));
        /* both sides strided differently */
        in.push_back(rseg(D, S, two, 4096, L(96, 5, 1, 128, 0), 1024, 5));
        /* a face whose partitions sit 64 B further apart than its pitch; one
         * run entry crosses a 16 KiB tile end */
        const MPIX_Layout face = L(272, 15, 1, 400, 0);
        in.push_back(rseg(D, S, face, 6064, layout_contiguous(4080), 4080,
                          8));
        /* an entry without a partition level next to them */
        StridedSeg plain;
        plain.dst = (void *)(uintptr_t)D;
        plain.src = (const void *)(uintptr_t)S;
        plain.bytes = 4080;
        plain.sl = face;
        plain.dl = layout_contiguous(4080);
        in.push_back(plain);
        CHECK(verify_runs(in, false) == 16);
        CHECK(verify_runs(in, true) == 16);
        /* alone it does not ask for the partition-level kernel */
        std::vector<StridedSeg> one{plain};
        verify_runs(one, false);
    }
    g_case = "plan granule 4";
    {
        std::vector<StridedSeg> in;
        in.push_back(rseg(D, S, L(4, 7, 1, 12, 0), 100,
                          layout_contiguous(28), 28, 8));
        /* 16-byte runs, but the part stride only divides by 4 */
        in.push_back(rseg(D, S, L(16, 3, 1, 32, 0), 100,
                          layout_contiguous(48), 48, 3));
        CHECK(verify_runs(in, false) == 4);
        CHECK(verify_runs(in, true) == 4);
        StridedTable t;
        memset(&t, 0, sizeof(t));
        plan_strided(&in[1], 1, false, &t);
        CHECK(t.e[0].glog == 2);
    }
    g_case = "plan granule 1";
    {
        std::vector<StridedSeg> in;
        in.push_back(rseg(D + 1, S, L(3, 5, 1, 7, 0), 41,
                          layout_contiguous(15), 15, 8));
        in.push_back(rseg(D, S, L(3, 5, 2, 7, 50), 101, L(5, 6, 1, 9, 0), 77,
                          7));
        CHECK(verify_runs(in, false) == 1);
        CHECK(verify_runs(in, true) == 1);
    }
    g_case = "plan wide by size";
    {
        /* k * part_units reaches 2^31: wide without being forced (planned
         * only, then spot-checked) */
        const MPIX_Layout big = L(1, 1ull << 27, 1, 2, 0);
        StridedSeg w = rseg(D, S, big, 3ll << 28, layout_contiguous(1ull << 27),
                            1ll << 27, 16);
        StridedTable t;
        memset(&t, 0, sizeof(t));
        CHECK(plan_strided(&w, 1, false, &t) == 1);
        CHECK(t.e[0].glog == 0 && t.e[0].wide == 1 && strided_plan_wide(t));
        CHECK(strided_plan_parts(t));
        CHECK(t.tile_end[0] == (1ull << 31) / MPIX_STRIDED_TILE);
        const uint64_t us[] = {0, 1, (1ull << 27) - 1, 1ull << 27,
                               (1ull << 31) - 1, (5ull << 27) + 12345};
        for (uint64_t u : us) {
            int64_t so, dof;
            strided_entry_offsets(t.e[0], u, true, true, &so, &dof);
            CHECK(so == part_layout_offset(w.sl, w.s_part_stride, u));
            CHECK(dof == part_layout_offset(w.dl, w.d_part_stride, u));
        }
        w.parts = 15;
        w.bytes = 15ull << 27;
        CHECK(plan_strided(&w, 1, false, &t) == 1);
        CHECK(t.e[0].wide == 0 && strided_plan_parts(t));
    }
}

/* -------------------------------------------------------------- run code */

static const void *REQ_A = (const void *)(uintptr_t)0x1000;
static const void *REQ_B = (const void *)(uintptr_t)0x2000;
static const uint64_t PART = 4080;
static const uintptr_t DST = 0x7e0000000000ull;

static RunSend snd(int p, bool strided, uint64_t bytes = PART)
{
    return RunSend{REQ_A, 1, p, bytes, true, true, strided};
}

static size_t run_len(const std::vector<RunSend> &q, uint64_t push_max = 0)
{
    return part_run_length(q.size(), [&](size_t i) { return q[i]; },
                           push_max);
}

static RunRecv rcv(int p, int64_t stride, bool strided,
                   const void *req = REQ_A, uintptr_t base = DST)
{
    RunRecv r{req, p, PART, base + (uintptr_t)p * (uintptr_t)stride, true,
              true, strided};
    r.part_stride = stride;
    return r;
}

static long fast(const std::vector<RunRecv> &posted, int p0, uint32_t k,
                 uint64_t bytes = PART)
{
    return part_run_fast_range(posted.size(),
                               [&](size_t i) { return posted[i]; }, p0, k,
                               bytes);
}

static void test_run_code()
{
    g_case = "run length, strided";
    {
        std::vector<RunSend> q;
        for (int p = 0; p < 8; p++) q.push_back(snd(p, true));
        CHECK(run_len(q) == 8);
        /* strided sends are always announced, whatever the push threshold */
        CHECK(run_len(q, PART) == 8);
        CHECK(run_len(q, 1ull << 40) == 8);
        q[5].partition = 6; /* no continuation */
        CHECK(run_len(q) == 5);
        q[5].partition = 5;
        q[3].req = REQ_B;
        CHECK(run_len(q) == 3);
        q[3].req = REQ_A;
        q[2].device = false;
        CHECK(run_len(q) == 2);
    }
    g_case = "run length, gapped";
    {
        /* contiguous partitions with gaps look like any contiguous ones to
         * the sender: the part stride travels in the descriptor */
        std::vector<RunSend> q;
        for (int p = 0; p < 8; p++) q.push_back(snd(p, false));
        CHECK(run_len(q) == 8);
        CHECK(run_len(q, PART) == 1); /* pushed, not announced */
    }
    g_case = "fast range follows the receiver's part stride";
    {
        const int64_t strides[] = {(int64_t)PART, 4352, 6064, 1 << 20};
        for (int64_t st : strides) {
            for (int strided = 0; strided < 2; strided++) {
                std::vector<RunRecv> all;
                for (int p = 0; p < 8; p++)
                    all.push_back(rcv(p, st, strided != 0));
                CHECK(fast(all, 0, 8) == 0);
                CHECK(fast(all, 3, 4) == 3);
                CHECK(fast(all, 3, 1) == -1);
                CHECK(fast(all, 0, 8, PART + 16) == -1);
                /* one receive off by one byte, either way */
                std::vector<RunRecv> v = all;
                v[5].buf += 1;
                CHECK(fast(v, 0, 8) == -1);
                CHECK(fast(v, 0, 5) == 0);
                v[5].buf -= 2;
                CHECK(fast(v, 0, 8) == -1);
                /* receives that are msg_bytes apart while the request says
                 * otherwise are no range */
                if (st != (int64_t)PART) {
                    std::vector<RunRecv> w;
                    for (int p = 0; p < 8; p++) {
                        RunRecv r = rcv(p, (int64_t)PART, strided != 0);
                        r.part_stride = st;
                        w.push_back(r);
                    }
                    CHECK(fast(w, 0, 8) == -1);
                }
                v = all;
                v[2].device = false;
                CHECK(fast(v, 0, 8) == -1);
                v = all;
                v[6].strided = !v[6].strided;
                CHECK(fast(v, 0, 8) == -1);
                v = all;
                std::swap(v[1], v[2]);
                CHECK(fast(v, 0, 8) == -1);
                v = all;
                v[4].req = REQ_B;
                CHECK(fast(v, 0, 8) == -1);
            }
        }
        /* no alignment demand here: base + 1 is a range */
        std::vector<RunRecv> odd;
        for (int p = 0; p < 8; p++)
            odd.push_back(rcv(p, 41, false, REQ_A, DST + 1));
        CHECK(fast(odd, 0, 8) == 0);
        /* an earlier receive of another request that takes a later
         * partition sends the run to the expansion */
        std::vector<RunRecv> two;
        for (int p = 4; p < 8; p++) two.push_back(rcv(p, 6064, true));
        for (int p = 0; p < 8; p++)
            two.push_back(rcv(p, 6064, true, REQ_B, DST + (1 << 24)));
        CHECK(fast(two, 0, 8) == -1);
        CHECK(fast(two, 0, 4) == 4);
        CHECK(fast(two, 4, 4) == 0);
    }
    g_case = "the plain range is the aligned, contiguous special case";
    {
        std::vector<RunRecv> all;
        for (int p = 0; p < 8; p++) all.push_back(rcv(p, (int64_t)PART, false));
        auto plain = [&](const std::vector<RunRecv> &v, uintptr_t src) {
            return part_run_fast_range(v.size(),
                                       [&](size_t i) { return v[i]; }, 0, 8,
                                       PART, src);
        };
        CHECK(plain(all, 0x7f0000000000ull) == 0);
        CHECK(plain(all, 0x7f0000000004ull) == -1);
        std::vector<RunRecv> gap;
        for (int p = 0; p < 8; p++) gap.push_back(rcv(p, 4352, false));
        CHECK(plain(gap, 0x7f0000000000ull) == -1); /* not msg_bytes apart */
        CHECK(fast(gap, 0, 8) == 0);
    }
    g_case = "expansion";
    {
        const uint64_t token = 9, ipc_off = 0x4000;
        const uint64_t strides[] = {PART, 4352, 6064, 5ull << 30};
        for (uint64_t st : strides)
            for (uint32_t j = 0; j < 8; j++) {
                RunSlice s = part_run_slice(2, ipc_off, st, token, j);
                CHECK(s.partition == 2 + (int)j);
                CHECK(s.ipc_off == ipc_off + j * st);
                CHECK(s.token == token && s.count == 1);
                /* which is where the definition puts the partition */
                CHECK((int64_t)(s.ipc_off - ipc_off) ==
                      part_layout_offset(layout_contiguous(PART), (int64_t)st,
                                         j * PART));
            }
    }
}

int main()
{
    test_offset();
    test_fold();
    test_plan();
    test_run_code();
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
