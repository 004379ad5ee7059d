/* Stand-alone check of the reduce kernels (src/transport/pull_kernels.h):
 * k_pull_reduce and k_pull_reduce_done are launched directly through
 * launch_reduce, from tables made by the production planner (plan_reduce),
 * with block counts the runtime never chooses, and the whole destination
 * arena is compared byte for byte with reduce_host (src/transport/reduce.h)
 * applied to a host copy.  No libmpix, no MPI.
 *
 *     reduce_kernels_check GROUP          GROUP = edges | paths | full
 *     reduce_kernels_check --list GROUP   the launches, without a GPU
 *
 *   edges  one entry per table, for all 18 type/op pairs: 1 element,
 *          16 B - 1 element, 16 B, T - 16, T, T + 16 + 1 element and
 *          3T + an odd number of elements (T = 16 KiB), with 1, 2 and
 *          `tiles` blocks;
 *   paths  one table that mixes all six types and three ops, and one whose
 *          entries have the source, the destination or both offset by one
 *          element (the element path);
 *   full   64 segments, the most one launch takes, 8 of them one merged
 *          run, with 1, 2, 3, 7 and `tiles` blocks.
 *
 * Per launch: the destination arena (sentinel bytes, the entries' initial
 * values, a guard page behind it) is written afresh, the kernel runs, the
 * stream is synchronised, both arenas come back; the destination must equal
 * the reference exactly and the source must be unchanged.  The arenas hold
 * finite values of each entry's type (no NaNs: their payload is
 * unspecified).  One counter and one word serve every by-word launch of the
 * program, as in pull_kernels_check: after each the counter reads 0 and the
 * word the launch's number; an event launch leaves the word alone.  One
 * JSON line per launch; the first HIP error ends the program (exit 2); exit
 * 1 if any launch had a bad byte or a wrong counter or word; exit 3 if a
 * case is not what it is meant to be.  Everything is read after
 * hipStreamSynchronize: that the word implies the payload without one is
 * not shown here.  tests/native/reduce_check.cpp shows on the CPU that a
 * byte-exact comparison with this reference flags a subtly wrong combine. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../src/transport/pull_kernels.h"

using namespace mpix;

#define HIP_OK(call)                                                       \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) {                                            \
            fflush(stdout);                                                \
            fprintf(stderr, "HIP error at %s:%d: %s: %s\n", __FILE__,      \
                    __LINE__, #call, hipGetErrorString(e_));               \
            exit(2);                                                       \
        }                                                                  \
    } while (0)

static const uint64_t T = MPIX_REDUCE_TILE;
static const uint64_t GUARD = 4096; /* sentinel behind every destination */
static const uint8_t SENTINEL = 0xA5;
static const uint64_t MAX_ARENA = 1ull << 20; /* no case is over 1 MiB */

static bool g_dry = false;
static hipStream_t g_stream;
static uint32_t *g_counter;  /* device */
static uint64_t *g_word;     /* host, mapped */
static uint64_t *g_word_dev; /* its device address */
static uint64_t g_seq = 0;
static unsigned long g_launches = 0, g_failed = 0;

[[noreturn]] static void not_as_meant(const std::string &why)
{
    fflush(stdout);
    fprintf(stderr, "case not as meant: %s\n", why.c_str());
    exit(3);
}

static uint64_t g_rng = 0x2545f4914f6cdd1dull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

/* n finite elements of `type` at p: sums of any two stay finite and, for
 * f32 and bf16, normal or zero */
static void fill_values(uint8_t *p, uint64_t n, uint32_t type)
{
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t r = rnd();
        switch (type) {
        case RED_F32: {
            const float v = (float)((int64_t)(r & 0xffffff) - 0x800000) /
                            (float)(1 << (8 + (r >> 60)));
            memcpy(p + 4 * i, &v, 4);
            break;
        }
        case RED_F64: {
            const double v = (double)((int64_t)(r & 0xffffffffffffull) -
                                      0x800000000000ll) /
                             (double)(1ull << (20 + (r >> 59)));
            memcpy(p + 8 * i, &v, 8);
            break;
        }
        case RED_BF16: { /* exponent field 120 .. 135 */
            const uint16_t v = (uint16_t)((r & 0x8000) |
                                          ((120 + ((r >> 16) & 15)) << 7) |
                                          ((r >> 24) & 0x7f));
            memcpy(p + 2 * i, &v, 2);
            break;
        }
        case RED_F16: { /* exponent field 0 (subnormal) .. 28 */
            const uint16_t v = (uint16_t)((r & 0x8000) |
                                          (((r >> 16) % 29) << 10) |
                                          ((r >> 24) & 0x3ff));
            memcpy(p + 2 * i, &v, 2);
            break;
        }
        case RED_I32: {
            const uint32_t v = (uint32_t)r;
            memcpy(p + 4 * i, &v, 4);
            break;
        }
        default:
            memcpy(p + 8 * i, &r, 8);
        }
    }
}

/* one segment of a case, by its offsets into the two arenas */
struct SegAt {
    uint64_t soff, doff, bytes;
    uint32_t type, op;
};

struct Case {
    std::string name;
    std::vector<SegAt> segs;
    uint64_t ssize = 0, dsize = 0;
    uint32_t want_entries = 0;
    std::vector<unsigned> blocks; /* 0 stands for `tiles` */

    /* the next segment 256-aligned plus (s_extra, d_extra) bytes in each
     * arena; follow: straight behind the previous one on both sides */
    void add(uint64_t bytes, uint32_t type, uint32_t op, uint64_t s_extra = 0,
             uint64_t d_extra = 0, bool follow = false)
    {
        SegAt g;
        if (follow) {
            g.soff = segs.back().soff + segs.back().bytes;
            g.doff = segs.back().doff + segs.back().bytes;
        } else {
            g.soff = ((ssize + 255) & ~255ull) + 256 + s_extra;
            g.doff = ((dsize + 255) & ~255ull) + 256 + d_extra;
        }
        g.bytes = bytes;
        g.type = type;
        g.op = op;
        ssize = g.soff + bytes;
        dsize = g.doff + bytes;
        segs.push_back(g);
    }
};

static const char *const TYPE_NAME[] = {"f32", "f64", "bf16", "f16", "i32",
                                        "i64"};
static const char *const OP_NAME[] = {"sum", "max", "min"};

static std::vector<Case> cases_of(const std::string &group)
{
    std::vector<Case> out;
    if (group == "edges") {
        for (uint32_t type = 0; type < RED_NTYPES; type++)
            for (uint32_t op = 0; op < RED_NOPS; op++) {
                const uint64_t es = reduce_elem_size((int)type);
                const struct { const char *name; uint64_t bytes; } sizes[] = {
                    {"1el", es}, {"16-1el", 16 - es}, {"16", 16},
                    {"T-16", T - 16}, {"T", T}, {"T+16+1el", T + 16 + es},
                    {"3T+odd", 3 * T + 1237 * es}};
                for (const auto &z : sizes) {
                    Case c;
                    c.name = std::string("edges/") + TYPE_NAME[type] + "/" +
                             OP_NAME[op] + "/" + z.name;
                    c.add(z.bytes, type, op);
                    c.want_entries = 1;
                    c.blocks = {1, 2, 0};
                    out.push_back(c);
                }
            }
    } else if (group == "paths") {
        Case m;
        m.name = "mixed_types";
        const uint64_t elems[] = {1, 7, 4096, 1031, 5000, 9};
        for (uint32_t type = 0; type < RED_NTYPES; type++)
            for (uint32_t op = 0; op < RED_NOPS; op++)
                m.add(elems[(type + 2 * op) % 6] *
                          reduce_elem_size((int)type), type, op);
        m.want_entries = 18;
        m.blocks = {1, 2, 3, 0};
        out.push_back(m);
        Case o;
        o.name = "offset_by_one_element";
        for (uint32_t type = 0; type < RED_NTYPES; type++) {
            const uint64_t es = reduce_elem_size((int)type);
            o.add(T + 16 + es, type, RED_SUM, es, 0);
            o.add(3 * es, type, RED_MAX, 0, es);
            o.add(T - es, type, RED_MIN, es, es);
            o.add(2 * T + 5 * es, type, RED_SUM, 16 - es, es);
        }
        o.want_entries = 24;
        o.blocks = {1, 2, 3, 0};
        out.push_back(o);
    } else if (group == "full") {
        Case f;
        f.name = "full_table";
        for (int i = 0; i < 8; i++) /* one run: 8 x 4112 B */
            f.add(4112, RED_F32, RED_SUM, 0, 0, i > 0);
        for (uint32_t i = 8; i < MPIX_PULL_BATCH; i++) {
            const uint32_t type = i % RED_NTYPES, op = (i / 6) % RED_NOPS;
            const uint64_t es = reduce_elem_size((int)type);
            const uint64_t elems = i % 9 == 0 ? T / es + 3 : 1 + (i * 37) % 300;
            /* every fifth entry off the 16-byte grid on one side */
            f.add(elems * es, type, op, i % 5 == 0 ? es : 0, 0);
        }
        f.want_entries = MPIX_PULL_BATCH - 7;
        f.blocks = {1, 2, 3, 7, 0};
        out.push_back(f);
    }
    return out;
}

static std::vector<unsigned> resolve_blocks(const std::vector<unsigned> &want,
                                            uint64_t tiles)
{
    std::vector<unsigned> out;
    for (unsigned b : want) {
        uint64_t v = b == 0 ? tiles : b;
        if (v > tiles) v = tiles;
        if (v > 1024) v = 1024;
        bool seen = false;
        for (unsigned o : out) seen = seen || o == v;
        if (!seen) out.push_back((unsigned)v);
    }
    return out;
}

static void run_case(const Case &c)
{
    const uint64_t ssize = c.ssize + 256, dsize = c.dsize + 256 + GUARD;
    if (ssize > MAX_ARENA || dsize > MAX_ARENA)
        not_as_meant(c.name + ": an arena over 1 MiB");
    std::vector<uint8_t> src(ssize), init(dsize, SENTINEL), want, got_src(ssize),
        got_dst(dsize);
    for (uint64_t i = 0; i < ssize; i++) src[i] = (uint8_t)(rnd() >> 32);
    for (const SegAt &g : c.segs) {
        const uint64_t es = reduce_elem_size((int)g.type);
        if (g.bytes == 0 || g.bytes % es || g.soff % es || g.doff % es ||
            g.soff + g.bytes > c.ssize || g.doff + g.bytes > c.dsize)
            not_as_meant(c.name + ": a segment off its element grid or "
                         "outside its arena");
        fill_values(src.data() + g.soff, g.bytes / es, g.type);
        fill_values(init.data() + g.doff, g.bytes / es, g.type);
    }
    want = init;
    for (const SegAt &g : c.segs)
        reduce_host(want.data() + g.doff, src.data() + g.soff,
                    g.bytes / reduce_elem_size((int)g.type), (int)g.type,
                    (int)g.op);

    uint8_t *dsrc = (uint8_t *)(uintptr_t)0x10000000;
    uint8_t *ddst = (uint8_t *)(uintptr_t)0x20000000;
    if (!g_dry) {
        HIP_OK(hipMalloc(&dsrc, ssize));
        HIP_OK(hipMalloc(&ddst, dsize));
        if (((uintptr_t)dsrc | (uintptr_t)ddst) & 255)
            not_as_meant("device arenas are not 256-byte aligned");
        HIP_OK(hipMemcpyAsync(dsrc, src.data(), ssize, hipMemcpyHostToDevice,
                              g_stream));
        HIP_OK(hipStreamSynchronize(g_stream));
    }
    std::vector<ReduceSeg> segs;
    for (const SegAt &g : c.segs)
        segs.push_back(ReduceSeg{ddst + g.doff, dsrc + g.soff, g.bytes, g.type,
                                 g.op});
    ReduceTable t;
    if (plan_reduce(segs.data(), segs.size(), T, &t) != segs.size())
        not_as_meant(c.name + ": the planner cut the batch");
    if (t.n != c.want_entries)
        not_as_meant(c.name + ": number of entries");
    /* every table address inside its arena: nothing here may write, or
     * read, out of bounds */
    for (uint32_t i = 0; i < t.n; i++) {
        const ReduceEntry &e = t.e[i];
        if ((uint8_t *)e.dst < ddst ||
            (uint8_t *)e.dst + e.bytes > ddst + c.dsize ||
            (const uint8_t *)e.src < dsrc ||
            (const uint8_t *)e.src + e.bytes > dsrc + c.ssize)
            not_as_meant(c.name + ": an entry leaves its arena");
    }
    const uint64_t tiles = reduce_total_tiles(t);
    for (int by_word = 1; by_word >= 0; by_word--)
        for (unsigned blocks : resolve_blocks(c.blocks, tiles)) {
            const char *variant = by_word ? "k_pull_reduce_done"
                                          : "k_pull_reduce";
            if (blocks < 1 || blocks > 1024 || tiles == 0)
                not_as_meant(c.name + ": blocks or tiles out of range");
            g_launches++;
            if (g_dry) {
                printf("{\"variant\": \"%s\", \"table\": \"%s\", \"blocks\": "
                       "%u, \"tiles\": %lu, \"entries\": %u}\n", variant,
                       c.name.c_str(), blocks, (unsigned long)tiles, t.n);
                continue;
            }
            const uint64_t word_before = *(volatile uint64_t *)g_word;
            PullDone done{g_counter, g_word_dev, 0};
            if (by_word) done.seq = ++g_seq;
            HIP_OK(hipMemcpyAsync(ddst, init.data(), dsize,
                                  hipMemcpyHostToDevice, g_stream));
            HIP_OK(hipStreamSynchronize(g_stream));
            launch_reduce(t, blocks, g_stream, by_word ? &done : nullptr);
            HIP_OK(hipGetLastError());
            HIP_OK(hipStreamSynchronize(g_stream));
            uint32_t counter = 0;
            HIP_OK(hipMemcpyAsync(&counter, g_counter, sizeof counter,
                                  hipMemcpyDeviceToHost, g_stream));
            HIP_OK(hipMemcpyAsync(got_dst.data(), ddst, dsize,
                                  hipMemcpyDeviceToHost, g_stream));
            HIP_OK(hipMemcpyAsync(got_src.data(), dsrc, ssize,
                                  hipMemcpyDeviceToHost, g_stream));
            HIP_OK(hipStreamSynchronize(g_stream));
            const uint64_t word = *(volatile uint64_t *)g_word;
            uint64_t bad = 0, first_bad = 0, src_bad = 0;
            for (uint64_t i = 0; i < dsize; i++)
                if (got_dst[i] != want[i] && bad++ == 0) first_bad = i;
            for (uint64_t i = 0; i < ssize; i++) src_bad += got_src[i] != src[i];
            const bool signal_ok =
                counter == 0 && word == (by_word ? done.seq : word_before);
            char first[32] = "null", seq[32] = "null";
            if (bad)
                snprintf(first, sizeof first, "%lu", (unsigned long)first_bad);
            if (by_word)
                snprintf(seq, sizeof seq, "%lu", (unsigned long)done.seq);
            printf("{\"variant\": \"%s\", \"table\": \"%s\", \"blocks\": %u, "
                   "\"tiles\": %lu, \"entries\": %u, \"bad\": %lu, "
                   "\"first_bad\": %s, \"src_bad\": %lu, \"seq\": %s, "
                   "\"word_before\": %lu, \"word\": %lu, \"counter\": %u}\n",
                   variant, c.name.c_str(), blocks, (unsigned long)tiles, t.n,
                   (unsigned long)bad, first, (unsigned long)src_bad, seq,
                   (unsigned long)word_before, (unsigned long)word, counter);
            fflush(stdout);
            if (bad || src_bad || !signal_ok) g_failed++;
        }
    if (!g_dry) {
        HIP_OK(hipFree(dsrc));
        HIP_OK(hipFree(ddst));
    }
}

int main(int argc, char **argv)
{
    int at = 1;
    if (argc > at && strcmp(argv[at], "--list") == 0) {
        g_dry = true;
        at++;
    }
    const std::string group = argc > at ? argv[at] : "";
    const std::vector<Case> cases = cases_of(group);
    if (cases.empty()) {
        fprintf(stderr, "usage: %s [--list] edges|paths|full\n", argv[0]);
        return 64;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (!g_dry) {
        HIP_OK(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
        HIP_OK(hipMalloc(&g_counter, sizeof *g_counter));
        HIP_OK(hipMemset(g_counter, 0, sizeof *g_counter));
        HIP_OK(hipHostMalloc(&g_word, sizeof *g_word, hipHostMallocMapped));
        *g_word = 0;
        HIP_OK(hipHostGetDevicePointer((void **)&g_word_dev, g_word, 0));
        HIP_OK(hipDeviceSynchronize());
    }
    for (const Case &c : cases) run_case(c);
    if (!g_dry) {
        HIP_OK(hipStreamSynchronize(g_stream));
        HIP_OK(hipHostFree(g_word));
        HIP_OK(hipFree(g_counter));
        HIP_OK(hipStreamDestroy(g_stream));
    }
    const double secs = std::chrono::duration<double>(
        std::chrono::steady_clock::now() - t0).count();
    printf("{\"group\": \"%s\", \"launches\": %lu, \"failed\": %lu, "
           "\"seconds\": %.3f}\n", group.c_str(), g_launches, g_failed, secs);
    return g_failed ? 1 : 0;
}
