/* Stand-alone check of src/transport/part_run.h (host only, no HIP).
 * Built with -fsanitize=address,undefined and run as a program by
 * tests/test_part_run.py.  Exit status 0 = every case passed.
 *
 * Three things are checked: how long the run at the head of a send queue is,
 * whether a range of posted receives takes a run as one copy, and, when it
 * does not, what the expansion and the acks look like. */
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../src/transport/part_run.h"

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

/* requests are only ever compared */
static const void *REQ_A = (const void *)(uintptr_t)0x1000;
static const void *REQ_B = (const void *)(uintptr_t)0x2000;

static const uint64_t PART = 4112; /* a multiple of 16, not of a tile */
static const uintptr_t SRC = 0x7f0000000000ull; /* 16-aligned bases */
static const uintptr_t DST = 0x7e0000000000ull;

/* ------------------------------------------------------------ run length */

static RunSend snd(int p, const void *req = REQ_A, uint32_t pseq = 1)
{
    return RunSend{req, pseq, p, PART, true, true, false};
}

static size_t run_len(const std::vector<RunSend> &q, size_t from = 0,
                      uint64_t push_max = 0)
{
    return part_run_length(q.size() - from,
                           [&](size_t i) { return q[from + i]; }, push_max);
}

/* the runs a whole queue splits into, head after head */
static std::vector<size_t> split(const std::vector<RunSend> &q,
                                 uint64_t push_max = 0)
{
    std::vector<size_t> out;
    for (size_t at = 0; at < q.size();) {
        size_t k = run_len(q, at, push_max);
        CHECK(k >= 1 && at + k <= q.size());
        if (k < 1) break;
        out.push_back(k);
        at += k;
    }
    return out;
}

static void run_length_cases()
{
    typedef std::vector<size_t> L;
    g_case = "ascending";
    {
        std::vector<RunSend> q;
        for (int p = 0; p < 8; p++) q.push_back(snd(p));
        CHECK(split(q) == L({8}));
        /* a run need not start at partition 0 */
        CHECK(run_len(q, 3) == 5);
    }
    g_case = "descending";
    {
        std::vector<RunSend> q;
        for (int p = 7; p >= 0; p--) q.push_back(snd(p));
        CHECK(split(q) == L({1, 1, 1, 1, 1, 1, 1, 1}));
    }
    g_case = "interleaved";
    {
        std::vector<RunSend> q;
        for (int p : {0, 2, 4, 6, 1, 3, 5, 7}) q.push_back(snd(p));
        CHECK(split(q) == L({1, 1, 1, 1, 1, 1, 1, 1}));
    }
    g_case = "mixed";
    {
        std::vector<RunSend> q;
        for (int p : {4, 5, 6, 0, 1, 7, 2, 3}) q.push_back(snd(p));
        CHECK(split(q) == L({3, 2, 1, 2}));
    }
    g_case = "single";
    {
        std::vector<RunSend> q{snd(5)};
        CHECK(split(q) == L({1}));
    }
    g_case = "repeat";
    {
        /* the same partition twice is no continuation */
        std::vector<RunSend> q{snd(0), snd(1), snd(1), snd(2)};
        CHECK(split(q) == L({2, 2}));
    }
    g_case = "other request";
    {
        std::vector<RunSend> q{snd(0), snd(1), snd(2, REQ_B), snd(3, REQ_B),
                               snd(2), snd(3)};
        CHECK(split(q) == L({2, 2, 2}));
    }
    g_case = "other pseq";
    {
        std::vector<RunSend> q{snd(0), snd(1), snd(2, REQ_A, 2),
                               snd(3, REQ_A, 2)};
        CHECK(split(q) == L({2, 2}));
    }
    g_case = "strided op";
    {
        std::vector<RunSend> q{snd(0), snd(1), snd(2), snd(3)};
        q[2].strided = true;
        CHECK(split(q) == L({2, 1, 1}));
        q[2].strided = false;
        q[0].strided = true; /* a strided head is a run of 1 */
        CHECK(split(q) == L({1, 3}));
    }
    g_case = "host op";
    {
        std::vector<RunSend> q{snd(0), snd(1), snd(2), snd(3)};
        q[1].device = false;
        CHECK(split(q) == L({1, 1, 2}));
    }
    g_case = "plain send between";
    {
        std::vector<RunSend> q{snd(0), snd(1), snd(2)};
        q[1].part_send = false; /* an ISEND between two partitions */
        q[1].partition = -1;
        CHECK(split(q) == L({1, 1, 1}));
    }
    g_case = "other size";
    {
        std::vector<RunSend> q{snd(0), snd(1), snd(2)};
        q[2].bytes = PART - 16;
        CHECK(split(q) == L({2, 1}));
    }
    g_case = "push threshold";
    {
        /* at or under the sender-push threshold nothing is announced */
        std::vector<RunSend> q{snd(0), snd(1), snd(2)};
        CHECK(split(q, PART) == L({1, 1, 1}));
        CHECK(split(q, PART - 1) == L({3}));
    }
}

/* ------------------------------------------------------------- fast path */

static RunRecv rcv(int p, const void *req = REQ_A, uintptr_t base = DST)
{
    return RunRecv{req, p, PART, base + (uintptr_t)p * PART, true, true,
                   false};
}

static long fast(const std::vector<RunRecv> &posted, int p0, uint32_t k,
                 uint64_t bytes = PART, uintptr_t src = SRC)
{
    return part_run_fast_range(posted.size(),
                               [&](size_t i) { return posted[i]; }, p0, k,
                               bytes, src);
}

static void fast_path_cases()
{
    std::vector<RunRecv> all;
    for (int p = 0; p < 8; p++) all.push_back(rcv(p));

    g_case = "exactly k in order";
    CHECK(fast(all, 0, 8) == 0);
    CHECK(fast(all, 2, 4) == 2);
    CHECK(fast(all, 6, 2) == 6);
    {
        /* receives of another envelope in front do not matter */
        std::vector<RunRecv> v;
        RunRecv other = rcv(0, REQ_B);
        other.envelope = false;
        v.push_back(other);
        v.insert(v.end(), all.begin(), all.end());
        CHECK(fast(v, 0, 8) == 1);
    }
    g_case = "runs of 1 never";
    CHECK(fast(all, 3, 1) == -1);

    g_case = "one missing";
    {
        std::vector<RunRecv> v(all.begin(), all.begin() + 7); /* no 7 */
        CHECK(fast(v, 0, 8) == -1);
        CHECK(fast(v, 0, 7) == 0);
        v.erase(v.begin() + 3); /* 0 1 2 4 5 6 */
        CHECK(fast(v, 0, 7) == -1);
        CHECK(fast(v, 0, 3) == 0);
        CHECK(fast(v, 4, 3) == 3);
        std::vector<RunRecv> none;
        CHECK(fast(none, 0, 8) == -1);
        std::vector<RunRecv> late(all.begin() + 1, all.end()); /* no 0 */
        CHECK(fast(late, 0, 8) == -1);
    }
    g_case = "out of order";
    {
        std::vector<RunRecv> v = all;
        std::swap(v[4], v[5]);
        CHECK(fast(v, 0, 8) == -1);
        CHECK(fast(v, 0, 4) == 0);
        std::vector<RunRecv> rev(all.rbegin(), all.rend());
        CHECK(fast(rev, 0, 8) == -1);
    }
    g_case = "different size";
    {
        std::vector<RunRecv> v = all;
        v[5].bytes = PART - 16; /* a truncating receive */
        CHECK(fast(v, 0, 8) == -1);
        CHECK(fast(v, 0, 5) == 0);
        CHECK(fast(all, 0, 8, PART + 16) == -1); /* sender's are larger */
        CHECK(fast(all, 0, 8, 0) == -1);
    }
    g_case = "host or strided or misaligned";
    {
        std::vector<RunRecv> v = all;
        v[2].device = false;
        CHECK(fast(v, 0, 8) == -1);
        v = all;
        v[7].strided = true;
        CHECK(fast(v, 0, 8) == -1);
        std::vector<RunRecv> off;
        for (int p = 0; p < 8; p++) off.push_back(rcv(p, REQ_A, DST + 4));
        CHECK(fast(off, 0, 8) == -1);
        CHECK(fast(all, 0, 8, PART, SRC + 4) == -1);
    }
    g_case = "not slices of one buffer";
    {
        std::vector<RunRecv> v = all;
        v[3].buf += 16;
        CHECK(fast(v, 0, 8) == -1);
    }
    g_case = "two requests, one envelope";
    {
        /* A's receives 4..7 are still posted, then all of B's.  Single
         * descriptors for 0..7 would give 0..3 to B and 4..7 to A: no one
         * range, so the run expands */
        std::vector<RunRecv> v(all.begin() + 4, all.end());
        for (int p = 0; p < 8; p++) v.push_back(rcv(p, REQ_B, DST + 0x100000));
        CHECK(fast(v, 0, 8) == -1);
        CHECK(fast(v, 0, 4) == 4);  /* B's 0..3: nothing in front takes them */
        CHECK(fast(v, 4, 4) == 0);  /* A's 4..7 */
        /* a range must not run from one request into the other */
        std::vector<RunRecv> w(all.begin(), all.begin() + 4);
        for (int p = 4; p < 8; p++) w.push_back(rcv(p, REQ_B, DST));
        CHECK(fast(w, 0, 8) == -1);
    }
}

/* --------------------------------------------------- expansion and acks */

static void expansion_cases()
{
    g_case = "slices";
    const uint64_t token = 77, ipc_off = 0x4000;
    for (uint32_t j = 0; j < 8; j++) {
        RunSlice s = part_run_slice(3, ipc_off, PART, token, j);
        CHECK(s.partition == 3 + (int)j);
        CHECK(s.ipc_off == ipc_off + j * PART);
        CHECK(s.token == token);
        CHECK(s.count == 1);
    }
    {
        /* partitions of 4 GiB and more: offsets are 64-bit */
        RunSlice s = part_run_slice(0, 16, 5ull << 30, token, 63);
        CHECK(s.ipc_off == 16 + 63 * (5ull << 30));
    }

    g_case = "acks in order";
    {
        RunAwait a{3, 8, 8};
        for (int p = 3; p < 10; p++) CHECK(part_run_ack(&a, p, 1) == RUN_ACK_MORE);
        CHECK(a.remaining == 1);
        CHECK(part_run_ack(&a, 10, 1) == RUN_ACK_LAST);
        CHECK(a.remaining == 0);
    }
    g_case = "acks in any order";
    {
        RunAwait a{3, 8, 8};
        CHECK(part_run_ack(&a, 9, 2) == RUN_ACK_MORE);
        CHECK(part_run_ack(&a, 3, 1) == RUN_ACK_MORE);
        CHECK(part_run_ack(&a, 6, 3) == RUN_ACK_MORE);
        CHECK(part_run_ack(&a, 4, 2) == RUN_ACK_LAST);
    }
    g_case = "one ack";
    {
        RunAwait a{0, 64, 64};
        CHECK(part_run_ack(&a, 0, 64) == RUN_ACK_LAST);
        RunAwait one{-1, 1, 1}; /* a plain message: partition -1 */
        CHECK(part_run_ack(&one, -1, 1) == RUN_ACK_LAST);
    }
    g_case = "bad acks";
    {
        RunAwait a{3, 8, 8};
        CHECK(part_run_ack(&a, 2, 1) == RUN_ACK_BAD);
        CHECK(part_run_ack(&a, 11, 1) == RUN_ACK_BAD);
        CHECK(part_run_ack(&a, 10, 2) == RUN_ACK_BAD);
        CHECK(part_run_ack(&a, 3, 0) == RUN_ACK_BAD);
        CHECK(part_run_ack(&a, 3, 9) == RUN_ACK_BAD);
        CHECK(a.remaining == 8); /* a bad range changes nothing */
        CHECK(part_run_ack(&a, 3, 8) == RUN_ACK_LAST);
        CHECK(part_run_ack(&a, 3, 1) == RUN_ACK_BAD); /* nothing left */
    }
}

int main()
{
    run_length_cases();
    fast_path_cases();
    expansion_cases();
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
