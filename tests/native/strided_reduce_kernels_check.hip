/* Stand-alone check of the strided reduce kernels
 * (src/transport/pull_kernels.h): k_pull_strided_reduce<WIDE> and
 * k_pull_strided_reduce_done<WIDE>, all four, are launched directly through
 * launch_strided_reduce, from tables made by the production planner
 * (plan_strided_reduce), with block counts the runtime never chooses, and
 * the whole destination arena, gaps between the runs included, is compared
 * byte for byte with the reference of strided_reduce_ref.h (element by
 * element through part_layout_offset and Red<TYPE>::combine).  No libmpix,
 * no MPI.
 *
 *     strided_reduce_kernels_check GROUP
 *     strided_reduce_kernels_check --list GROUP   the launches, without a GPU
 *
 * GROUP (T = 16 KiB tile; the tables are those of strided_reduce_ref.h):
 *   edges   one entry per table, for all 18 type/op pairs: 1 element, one
 *           16-byte unit, T - 16, T, T + 16 + 1 element and 3T + an odd
 *           number of elements, each strided on the destination only, in
 *           runs of 1 element and of 48 bytes, with 1, 2 and `tiles` blocks;
 *   shapes  strided to contiguous, contiguous to strided, one level against
 *           two, a base offset by one element, runs of 3 elements, of 48 B
 *           and of T + 16 B, on the vector and the element path;
 *   parts   run entries of k = 4 with unrelated part strides, a folded run,
 *           single messages between them;
 *   wide    the tables of shapes and parts on the WIDE kernels;
 *   batch   16 entries mixing all six types, three ops and both unit sizes
 *           with 1, 2, 3, 7 and `tiles` blocks; 17 segments (two launches);
 *           overlapping and interleaved extents (two launches each, the
 *           sequential result).
 *
 * Per case and block count: the destination arena (sentinel bytes, the
 * entries' initial values, a guard page behind it) is written afresh, the
 * case's launches run one after the other on one stream, the stream is
 * synchronised, both arenas come back; the destination must equal the
 * reference exactly and the source must be unchanged.  A case of several
 * launches is compared once, behind its last launch (bad and src_bad are
 * null on the lines of the earlier ones).  One counter and one word serve
 * every by-word launch of the program: after each the counter reads 0 and
 * the word the launch's number; an event launch leaves the word alone.  One
 * JSON line per launch; the first HIP error ends the program (exit 2); exit
 * 1 if any launch had a bad byte or a wrong counter or word; exit 3 if a
 * case is not what it is meant to be, which includes every table address
 * that would leave its arena: nothing is launched then.  Everything is read
 * after hipStreamSynchronize: that the word implies the payload without one
 * is not shown here. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../src/transport/pull_kernels.h"
#include "strided_reduce_ref.h"

using namespace sredref;

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

static const uint64_t GUARD = 4096; /* sentinel behind every destination */
static const uint64_t MAX_ARENA = 1ull << 20; /* no case is over 1 MiB */

static bool g_dry = false;
static hipStream_t g_stream;
static uint8_t *g_dsrc = (uint8_t *)(uintptr_t)0x10000000; /* --list: any */
static uint8_t *g_ddst = (uint8_t *)(uintptr_t)0x20000000;
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

struct Launch {
    StridedReduceTable t;
    uint64_t tiles;
    uint32_t vec;
};

static void run_case(const Case &c, bool wide)
{
    const uint64_t ssize = c.src_size, dsize = c.dst_size + GUARD;
    if (!c.ok) not_as_meant(c.name + ": an invalid entry");
    if (ssize > MAX_ARENA || dsize > MAX_ARENA)
        not_as_meant(c.name + ": an arena over 1 MiB");
    std::vector<uint8_t> src(ssize), init(dsize, SENTINEL), want,
        got_src(ssize), got_dst(dsize);
    Rng rng;
    for (uint64_t i = 0; i < ssize; i++) src[i] = (uint8_t)(rng.next() >> 32);
    const uint64_t sbase = (uint64_t)(uintptr_t)g_dsrc;
    const uint64_t dbase = (uint64_t)(uintptr_t)g_ddst;
    /* the arenas the entries may touch: the guard page is not part of them,
     * so a reference (and with it every table address, checked below) that
     * reaches into it is refused */
    const Arena asrc{sbase, src.data(), c.src_size};
    const std::vector<StridedReduceSeg> ref = ref_segs(c, sbase, dbase);
    if (!fill_values(ref.data(), ref.size(), asrc,
                     Arena{dbase, init.data(), c.dst_size}, &rng))
        not_as_meant(c.name + ": a segment leaves its arena or is not made "
                     "of whole elements");
    want = init;
    if (!ref_apply(ref.data(), ref.size(), asrc,
                   Arena{dbase, want.data(), c.dst_size}, nullptr))
        not_as_meant(c.name + ": the reference leaves an arena");

    bool folds = true;
    const std::vector<StridedReduceSeg> segs = plan_segs(c, sbase, dbase,
                                                         &folds);
    if (!folds) not_as_meant(c.name + ": a run that should fold does not");
    std::vector<Launch> launches;
    uint32_t vec = 0;
    for (size_t at = 0; at < segs.size();) {
        Launch l;
        const size_t n = plan_strided_reduce(segs.data() + at,
                                             segs.size() - at, wide, &l.t);
        if (n == 0) not_as_meant(c.name + ": the planner refuses a segment");
        /* every unit of every entry inside the arenas, by the offsets the
         * kernel computes: nothing here may write, or read, out of bounds */
        l.vec = 0;
        for (uint32_t i = 0; i < l.t.n; i++) {
            const StridedEntry &e = l.t.e[i];
            l.vec += e.glog == 4;
            if ((e.wide != 0) != wide)
                not_as_meant(c.name + ": division width");
            for (uint64_t u = 0; u < e.units; u++) {
                int64_t soff, doff;
                strided_entry_offsets(e, u, wide, true, &soff, &doff);
                if (!arena_holds(asrc, (uint64_t)(uintptr_t)e.src +
                                           (uint64_t)soff, 1ull << e.glog) ||
                    !arena_holds(Arena{dbase, nullptr, c.dst_size},
                                 (uint64_t)(uintptr_t)e.dst + (uint64_t)doff,
                                 1ull << e.glog))
                    not_as_meant(c.name + ": a unit leaves its arena");
            }
        }
        l.tiles = strided_reduce_total_tiles(l.t);
        if (l.tiles == 0) not_as_meant(c.name + ": no tiles");
        vec += l.vec;
        launches.push_back(l);
        at += n;
    }
    if (launches.size() != c.want_launches)
        not_as_meant(c.name + ": number of launches");
    if (vec != c.want_vec)
        not_as_meant(c.name + ": entries on the vector path");

    if (!g_dry) {
        HIP_OK(hipMemcpyAsync(g_dsrc, src.data(), ssize, hipMemcpyHostToDevice,
                              g_stream));
        HIP_OK(hipStreamSynchronize(g_stream));
    }
    /* block counts are resolved against the case's first launch */
    for (int by_word = 1; by_word >= 0; by_word--)
        for (unsigned want_blocks : resolve_blocks(c.blocks,
                                                   launches[0].tiles)) {
            char variant[64];
            snprintf(variant, sizeof variant, "k_pull_strided_reduce%s<%s>",
                     by_word ? "_done" : "", wide ? "wide" : "narrow");
            if (!g_dry) {
                HIP_OK(hipMemcpyAsync(g_ddst, init.data(), dsize,
                                      hipMemcpyHostToDevice, g_stream));
                HIP_OK(hipStreamSynchronize(g_stream));
            }
            for (size_t li = 0; li < launches.size(); li++) {
                const Launch &l = launches[li];
                const bool last = li + 1 == launches.size();
                const unsigned blocks = want_blocks < l.tiles
                                            ? want_blocks : (unsigned)l.tiles;
                if (blocks < 1 || blocks > 1024)
                    not_as_meant(c.name + ": blocks out of range");
                g_launches++;
                if (g_dry) {
                    printf("{\"variant\": \"%s\", \"table\": \"%s\", "
                           "\"blocks\": %u, \"launch\": %zu, \"tiles\": %lu, "
                           "\"entries\": %u, \"vec\": %u}\n", variant,
                           c.name.c_str(), want_blocks, li,
                           (unsigned long)l.tiles, l.t.n, l.vec);
                    continue;
                }
                const uint64_t word_before = *(volatile uint64_t *)g_word;
                PullDone done{g_counter, g_word_dev, 0};
                if (by_word) done.seq = ++g_seq;
                launch_strided_reduce(l.t, wide, blocks, g_stream,
                                      by_word ? &done : nullptr);
                HIP_OK(hipGetLastError());
                HIP_OK(hipStreamSynchronize(g_stream));
                uint32_t counter = 0;
                HIP_OK(hipMemcpyAsync(&counter, g_counter, sizeof counter,
                                      hipMemcpyDeviceToHost, g_stream));
                if (last) {
                    HIP_OK(hipMemcpyAsync(got_dst.data(), g_ddst, dsize,
                                          hipMemcpyDeviceToHost, g_stream));
                    HIP_OK(hipMemcpyAsync(got_src.data(), g_dsrc, ssize,
                                          hipMemcpyDeviceToHost, g_stream));
                }
                HIP_OK(hipStreamSynchronize(g_stream));
                const uint64_t word = *(volatile uint64_t *)g_word;
                uint64_t bad = 0, first_bad = 0, src_bad = 0;
                if (last) {
                    for (uint64_t i = 0; i < dsize; i++)
                        if (got_dst[i] != want[i] && bad++ == 0) first_bad = i;
                    for (uint64_t i = 0; i < ssize; i++)
                        src_bad += got_src[i] != src[i];
                }
                const bool signal_ok =
                    counter == 0 && word == (by_word ? done.seq : word_before);
                char sbad[32] = "null", ssrc[32] = "null", first[32] = "null",
                     seq[32] = "null";
                if (last) {
                    snprintf(sbad, sizeof sbad, "%lu", (unsigned long)bad);
                    snprintf(ssrc, sizeof ssrc, "%lu", (unsigned long)src_bad);
                }
                if (bad)
                    snprintf(first, sizeof first, "%lu",
                             (unsigned long)first_bad);
                if (by_word)
                    snprintf(seq, sizeof seq, "%lu", (unsigned long)done.seq);
                printf("{\"variant\": \"%s\", \"table\": \"%s\", \"blocks\": "
                       "%u, \"launch\": %zu, \"tiles\": %lu, \"entries\": %u, "
                       "\"vec\": %u, \"bad\": %s, \"first_bad\": %s, "
                       "\"src_bad\": %s, \"seq\": %s, \"word_before\": %lu, "
                       "\"word\": %lu, \"counter\": %u}\n", variant,
                       c.name.c_str(), want_blocks, li, (unsigned long)l.tiles,
                       l.t.n, l.vec, sbad, first, ssrc, seq,
                       (unsigned long)word_before, (unsigned long)word,
                       counter);
                fflush(stdout);
                if (bad || src_bad || !signal_ok) g_failed++;
            }
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
    bool wide = false;
    const std::vector<Case> cases = cases_of(group, &wide);
    if (cases.empty()) {
        fprintf(stderr, "usage: %s [--list] edges|shapes|parts|wide|batch\n",
                argv[0]);
        return 64;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (!g_dry) {
        HIP_OK(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
        HIP_OK(hipMalloc(&g_dsrc, MAX_ARENA));
        HIP_OK(hipMalloc(&g_ddst, MAX_ARENA));
        if (((uintptr_t)g_dsrc | (uintptr_t)g_ddst) & 255)
            not_as_meant("device arenas are not 256-byte aligned");
        HIP_OK(hipMalloc(&g_counter, sizeof *g_counter));
        HIP_OK(hipMemset(g_counter, 0, sizeof *g_counter));
        HIP_OK(hipHostMalloc(&g_word, sizeof *g_word, hipHostMallocMapped));
        *g_word = 0;
        HIP_OK(hipHostGetDevicePointer((void **)&g_word_dev, g_word, 0));
        HIP_OK(hipDeviceSynchronize());
    }
    for (const Case &c : cases) run_case(c, wide);
    if (!g_dry) {
        HIP_OK(hipStreamSynchronize(g_stream));
        HIP_OK(hipHostFree(g_word));
        HIP_OK(hipFree(g_counter));
        HIP_OK(hipFree(g_ddst));
        HIP_OK(hipFree(g_dsrc));
        HIP_OK(hipStreamDestroy(g_stream));
    }
    const double secs = std::chrono::duration<double>(
        std::chrono::steady_clock::now() - t0).count();
    printf("{\"group\": \"%s\", \"launches\": %lu, \"failed\": %lu, "
           "\"seconds\": %.3f}\n", group.c_str(), g_launches, g_failed, secs);
    return g_failed ? 1 : 0;
}
