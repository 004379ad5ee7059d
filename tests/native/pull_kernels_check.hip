/* Stand-alone check of the pull kernels (src/transport/pull_kernels.h): every
 * variant the header instantiates is launched directly, with block counts
 * the runtime never chooses, and the whole destination arena is compared
 * with the byte-exact reference of pull_ref.h.  No libmpix, no MPI.
 *
 *     pull_kernels_check GROUP     GROUP = contig-u1 | contig-u4 | contig-u8 |
 *                                          strided-narrow | strided-wide
 *     pull_kernels_check --list GROUP      the launches, without a GPU
 *
 * The tables come from the production planners (plan_pulls, plan_strided
 * with force_wide) and the launches from launch_pull, launch_strided and
 * launch_tail on one non-blocking stream.  Per launch: the destination
 * arena (plus a guard page behind it) is filled with the sentinel, the
 * kernel runs, the stream is synchronised, both arenas come back; the
 * destination must equal the reference exactly and the source must be
 * unchanged.  One JSON line per launch; the first HIP error ends the
 * program (exit 2) and nothing more is launched; exit 1 if any launch had a
 * bad byte or a wrong counter or word; exit 3 if a case is not what it is
 * meant to be (nothing of it is launched then).
 *
 * Completion signal: ONE counter (device memory, zeroed once) and ONE word
 * (mapped host memory) serve every by-word launch of the program, with
 * sequence numbers that grow from launch to launch.  After each by-word
 * launch the counter must read 0 and the word the launch's number, whatever
 * grid sizes came before; after each event launch the word is unchanged.
 *
 * What this cannot show: that the word, once seen, implies the payload is in
 * memory WITHOUT a fence or a synchronise.  Everything here is read after
 * hipStreamSynchronize.  tests/test_pull_done_modes_gpu.py reads from a
 * second stream for that.
 *
 * tests/native/pull_ref_check.cpp shows on the CPU that this comparison
 * flags a subtly wrong walk.  No wrong kernel is ever built for the GPU. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../src/transport/pull_kernels.h"
#include "pull_ref.h"

using namespace pullref;

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

/* device arenas of one case, and the host side of the comparison */
struct Run {
    std::string table;
    uint64_t ssize, dsize;
    uint8_t *dsrc = nullptr, *ddst = nullptr;
    std::vector<uint8_t> src, want, got_src, got_dst;
    std::vector<int32_t> owner;

    Run(const std::string &name, uint64_t src_size, uint64_t dst_size)
        : table(name), ssize(src_size), dsize(dst_size + GUARD)
    {
        src.resize(ssize);
        fill_src(src.data(), ssize);
        want.assign(dsize, SENTINEL);
        owner.assign(dsize, -1);
        got_src.resize(ssize);
        got_dst.resize(dsize);
        if (g_dry) {
            dsrc = (uint8_t *)(uintptr_t)0x10000000;
            ddst = (uint8_t *)(uintptr_t)0x20000000;
            return;
        }
        HIP_OK(hipMalloc(&dsrc, ssize));
        HIP_OK(hipMalloc(&ddst, dsize));
        if (((uintptr_t)dsrc | (uintptr_t)ddst) & 255)
            not_as_meant("device arenas are not 256-byte aligned");
        HIP_OK(hipMemcpyAsync(dsrc, src.data(), ssize, hipMemcpyHostToDevice,
                              g_stream));
        HIP_OK(hipStreamSynchronize(g_stream));
    }
    ~Run()
    {
        if (g_dry) return;
        HIP_OK(hipFree(dsrc));
        HIP_OK(hipFree(ddst));
    }
    Run(const Run &) = delete;
    Run &operator=(const Run &) = delete;

    Arena src_arena() { return Arena{(uint64_t)(uintptr_t)dsrc, src.data(), ssize}; }
    Arena want_arena() { return Arena{(uint64_t)(uintptr_t)ddst, want.data(), dsize}; }

    /* fill, launch, synchronise, fetch, compare, report */
    template <typename Launch>
    void launch(const std::string &variant, unsigned blocks, uint64_t tiles,
                bool by_word, Launch fn)
    {
        if (blocks < 1 || blocks > 1024 || tiles == 0)
            not_as_meant(table + ": blocks or tiles out of range");
        g_launches++;
        if (g_dry) {
            printf("{\"variant\": \"%s\", \"table\": \"%s\", \"blocks\": %u, "
                   "\"tiles\": %lu}\n", variant.c_str(), table.c_str(), blocks,
                   (unsigned long)tiles);
            return;
        }
        const uint64_t word_before = *(volatile uint64_t *)g_word;
        PullDone done{g_counter, g_word_dev, 0};
        if (by_word) done.seq = ++g_seq;
        HIP_OK(hipMemsetAsync(ddst, SENTINEL, dsize, g_stream));
        fn(by_word ? &done : nullptr);
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
        const Diff d = compare(got_dst.data(), want.data(), dsize);
        const Diff s = compare(got_src.data(), src.data(), ssize);
        const bool signal_ok = counter == 0 &&
                               word == (by_word ? done.seq : word_before);
        char first[32] = "null";
        std::string where = "";
        if (d.bad) {
            snprintf(first, sizeof first, "%lu", (unsigned long)d.first);
            where = classify(owner, d.first);
        }
        char seq[32] = "null";
        if (by_word) snprintf(seq, sizeof seq, "%lu", (unsigned long)done.seq);
        printf("{\"variant\": \"%s\", \"table\": \"%s\", \"blocks\": %u, "
               "\"tiles\": %lu, \"bad\": %lu, \"first_bad\": %s, \"where\": "
               "\"%s\", \"src_bad\": %lu, \"seq\": %s, \"word_before\": %lu, "
               "\"word\": %lu, \"counter\": %u}\n", variant.c_str(),
               table.c_str(), blocks, (unsigned long)tiles,
               (unsigned long)d.bad, first, where.c_str(),
               (unsigned long)s.bad, seq, (unsigned long)word_before,
               (unsigned long)word, counter);
        fflush(stdout);
        if (d.bad || s.bad || !signal_ok) g_failed++;
    }
};

static void run_contig(int U)
{
    const uint64_t T = 4096ull * (uint64_t)U;
    static const char *store[3] = {"WT", "NT", "PLAIN"};
    for (const ContigCase &cc : contig_cases(U, U == 1)) {
        Run run(cc.name, cc.src_size, cc.dst_size);
        std::vector<PullSeg> segs = contig_segs(
            cc, (uint64_t)(uintptr_t)run.dsrc, (uint64_t)(uintptr_t)run.ddst);
        for (const PullSeg &g : segs)
            if ((((uintptr_t)g.src | (uintptr_t)g.dst) & 15) != 0)
                not_as_meant(cc.name + ": a base is off the 16-byte grid");
        if (!ref_contig(segs.data(), segs.size(), run.src_arena(),
                        run.want_arena(), &run.owner))
            not_as_meant(cc.name + " leaves its arenas");
        PullTable t;
        if (plan_pulls(segs.data(), segs.size(), T, &t) != segs.size() ||
            t.ncopies != cc.want_copies || t.ncopies == 0)
            not_as_meant(cc.name + ": number of copies");
        const uint64_t tiles = pull_total_tiles(t);
        /* blocks 3 and 7 over full_table must step over 2 and 6 whole
         * copies in one trip of the do ... while of pull_multi_body */
        if (cc.stepping)
            for (unsigned G : {3u, 7u})
                if (max_copies_stepped_over(t, T, G) < G - 1)
                    not_as_meant(cc.name + ": no block steps over copies");
        for (int v = 0; v < 3; v++) {
            char variant[64];
            snprintf(variant, sizeof variant, "k_pull_multi%s<%d,%s>",
                     v == 0 ? "_done" : "", U, store[v]);
            for (unsigned blocks : resolve_blocks(cc.blocks, tiles))
                run.launch(variant, blocks, tiles, v == 0,
                           [&](const PullDone *done) {
                               launch_pull(t, U, v == 1, blocks, g_stream,
                                           done);
                           });
        }
    }
}

static void run_strided(bool wide)
{
    const StridedCase tables[2] = {strided_mixed_granules(),
                                   strided_with_partitions()};
    for (const StridedCase &sc : tables) {
        Run run(sc.name, sc.src_size, sc.dst_size);
        std::vector<StridedSeg> segs = strided_segs(
            sc, (uint64_t)(uintptr_t)run.dsrc, (uint64_t)(uintptr_t)run.ddst);
        if (!ref_strided(segs.data(), segs.size(), run.src_arena(),
                         run.want_arena(), &run.owner))
            not_as_meant(sc.name + " leaves its arenas");
        StridedTable t;
        if (plan_strided(segs.data(), segs.size(), wide, &t) != segs.size() ||
            t.n == 0)
            not_as_meant(sc.name + ": entries consumed");
        const std::string why = strided_plan_mismatch(sc, t, wide);
        if (!why.empty()) not_as_meant(why);
        if (strided_plan_wide(t) != wide)
            not_as_meant(sc.name + ": wide");
        const uint64_t tiles = strided_total_tiles(t);
        /* the PARTS kernel is right for entries without a partition level
         * too: mixed_granules runs under both */
        for (int parts = sc.has_parts ? 1 : 0; parts < 2; parts++)
            for (int by_word = 1; by_word >= 0; by_word--) {
                char variant[64];
                snprintf(variant, sizeof variant,
                         "k_pull_strided%s<wide=%d,parts=%d>",
                         by_word ? "_done" : "", (int)wide, parts);
                for (unsigned blocks : resolve_blocks({1, 2, 3, 0}, tiles))
                    run.launch(variant, blocks, tiles, by_word != 0,
                               [&](const PullDone *done) {
                                   launch_strided(t, wide, parts != 0, blocks,
                                                  g_stream, done);
                               });
            }
    }
}

/* launch_tail: the word takes the number, the counter is not touched */
static void run_tail()
{
    g_launches++;
    if (g_dry) {
        printf("{\"variant\": \"k_pull_tail\", \"table\": \"-\", \"blocks\": "
               "1, \"tiles\": 0}\n");
        return;
    }
    const uint64_t word_before = *(volatile uint64_t *)g_word;
    const uint64_t seq = ++g_seq;
    launch_tail(g_word_dev, seq, g_stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g_stream));
    uint32_t counter = 0;
    HIP_OK(hipMemcpyAsync(&counter, g_counter, sizeof counter,
                          hipMemcpyDeviceToHost, g_stream));
    HIP_OK(hipStreamSynchronize(g_stream));
    const uint64_t word = *(volatile uint64_t *)g_word;
    printf("{\"variant\": \"k_pull_tail\", \"table\": \"-\", \"blocks\": 1, "
           "\"tiles\": 0, \"bad\": 0, \"first_bad\": null, \"where\": \"\", "
           "\"src_bad\": 0, \"seq\": %lu, \"word_before\": %lu, \"word\": %lu, "
           "\"counter\": %u}\n", (unsigned long)seq,
           (unsigned long)word_before, (unsigned long)word, counter);
    if (word != seq || counter != 0) g_failed++;
}

int main(int argc, char **argv)
{
    int at = 1;
    if (argc > at && strcmp(argv[at], "--list") == 0) {
        g_dry = true;
        at++;
    }
    const std::string group = argc > at ? argv[at] : "";
    const int U = group == "contig-u1" ? 1 : group == "contig-u4" ? 4
                : group == "contig-u8" ? 8 : 0;
    if (U == 0 && group != "strided-narrow" && group != "strided-wide") {
        fprintf(stderr, "usage: %s [--list] contig-u1|contig-u4|contig-u8|"
                "strided-narrow|strided-wide\n", argv[0]);
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
    if (U)
        run_contig(U);
    else
        run_strided(group == "strided-wide");
    run_tail();
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
