/* Stand-alone check of bench/gemm_check.h (no HIP, no GPU): an emulated
 * kernel (fp32 accumulation in 32-term chunks, round-to-nearest-even to bf16)
 * passes in both data modes at every shape that tests/test_gemm_gpu.py runs,
 * and each mutation of its output that a subtly wrong kernel would produce
 * is reported bad: in unit mode exactly at the elements the mutation changed.
 * Built with AddressSanitizer + UBSan by tests/test_gemm_check.py. */
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <utility>
#include <vector>

#include "../../bench/gemm_check.h"

using namespace gemm_check;

static int failures = 0;

#define EXPECT(cond, ...)                                                  \
    do {                                                                   \
        if (!(cond)) {                                                     \
            failures++;                                                    \
            printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);          \
            printf(__VA_ARGS__);                                           \
            printf("\n");                                                  \
        }                                                                  \
    } while (0)

static const int T = 256;  /* C tile of the default kernel */
static const int KT = 64;  /* its K-tile */

struct Problem {
    int M, N, K;
    Mode mode;
    std::vector<uint16_t> A, Bt;
    std::vector<float> fa, fb;
    Reference ref;
    std::vector<uint16_t> clean; /* the emulated kernel's C */
};

/* one C element as the emulated kernel computes it; the mutations that
 * change the K loop are arguments */
static float emu_acc(const Problem &p, int i, int j, int drop_k = -1,
                     int skip_tile = -1, int twice_tile = -1)
{
    const float *a = &p.fa[(size_t)i * p.K], *b = &p.fb[(size_t)j * p.K];
    float acc = 0.f;
    for (int k0 = 0; k0 < p.K; k0 += 32) {
        float part = 0.f;
        for (int k = k0; k < k0 + 32; k++)
            if (k != drop_k) part += a[k] * b[k];
        if (k0 / KT == skip_tile) continue;
        acc += part;
        if (k0 / KT == twice_tile) acc += part;
    }
    return acc;
}

static void make(Problem &p, int M, int N, int K, Mode mode, uint32_t seed)
{
    p.M = M; p.N = N; p.K = K; p.mode = mode;
    p.A.resize((size_t)M * K);
    p.Bt.resize((size_t)N * K);
    fill(mode, seed, OP_A, M, K, p.A.data());
    fill(mode, seed, OP_B, N, K, p.Bt.data());
    p.fa.resize(p.A.size());
    p.fb.resize(p.Bt.size());
    for (size_t i = 0; i < p.A.size(); i++) p.fa[i] = bf16_to_f32(p.A[i]);
    for (size_t i = 0; i < p.Bt.size(); i++) p.fb[i] = bf16_to_f32(p.Bt[i]);
    reference(p.A.data(), p.Bt.data(), M, N, K, p.ref);
    p.clean.resize((size_t)M * N);
    for (int i = 0; i < M; i++)
        for (int j = 0; j < N; j++)
            p.clean[(size_t)i * N + j] = f32_to_bf16(emu_acc(p, i, j));
}

/* ------------------------------------------------------------ conversions */

static void check_conversions()
{
    EXPECT(f32_to_bf16(1.0f) == 0x3F80, "1.0");
    EXPECT(f32_to_bf16(-1.0f) == 0xBF80, "-1.0");
    EXPECT(f32_to_bf16(256.0f) == 0x4380, "256");
    /* ties to even: 1 + 2^-8 is half way between 1 and 1 + 2^-7 */
    EXPECT(f32_to_bf16(1.0f + 0.00390625f) == 0x3F80, "tie down to even");
    EXPECT(f32_to_bf16(1.0f + 3 * 0.00390625f) == 0x3F82, "tie up to even");
    EXPECT(f32_to_bf16(1.00390625f + 0.000001f) == 0x3F81, "above the tie");
    EXPECT(bf16_is_nan(f32_to_bf16(NAN)), "NaN stays NaN");
    EXPECT(bf16_is_nan(BF16_POISON), "poison is a NaN");
    EXPECT(!bf16_is_nan(0x7F80), "inf is no NaN");
    for (int v = -256; v <= 256; v++)
        EXPECT(bf16_to_f32(f32_to_bf16((float)v)) == (float)v,
               "integer %d not exact", v);
}

static void check_generators()
{
    const int R = 64, C = 96;
    std::vector<uint16_t> u((size_t)R * C), a(u.size()), b(u.size());
    fill(UNIT, 7, OP_A, R, C, u.data());
    size_t plus = 0;
    for (uint16_t x : u) {
        EXPECT(x == 0x3F80 || x == 0xBF80, "unit element 0x%04x", x);
        plus += x == 0x3F80;
    }
    EXPECT(plus > u.size() / 3 && plus < u.size() * 2 / 3, "%zu of %zu +1",
           plus, u.size());
    fill(UNIFORM, 7, OP_A, R, C, a.data());
    fill(UNIFORM, 7, OP_B, R, C, b.data());
    size_t same = 0, distinct_rows = 0;
    for (size_t i = 0; i < a.size(); i++) {
        float v = bf16_to_f32(a[i]);
        EXPECT(v >= -1.f && v < 1.f, "uniform element %g", v);
        same += a[i] == b[i];
    }
    EXPECT(same < a.size() / 16, "A and B agree in %zu elements", same);
    /* a value depends on the row and on the column */
    for (int r = 1; r < R; r++)
        distinct_rows += memcmp(&a[0], &a[(size_t)r * C], C * 2) != 0;
    EXPECT(distinct_rows == (size_t)R - 1, "rows repeat");
    std::vector<uint16_t> a2(a.size());
    fill(UNIFORM, 8, OP_A, R, C, a2.data());
    EXPECT(a2 != a, "seed ignored");
    /* a sub-matrix is generated from its own (row, col), not the global */
    EXPECT(element(UNIFORM, 7, OP_A, 5, 9) == a[5 * C + 9], "element/fill");
}

/* ------------------------------------------------- the emulation passes */

static const int SHAPES[][3] = {
    /* default binary */
    {256, 256, 64}, {256, 256, 128}, {256, 256, 192}, {256, 256, 512},
    {512, 768, 128}, {512, 1280, 128}, {768, 1536, 64}, {768, 1024, 64},
    {1024, 256, 64},
    /* v2, v3 */
    {128, 128, 32}, {128, 128, 96}, {256, 384, 64}, {128, 128, 64},
    {128, 128, 192}, {256, 384, 128},
    /* v5 (256 x 256 x 64 and x 128 are above) */
    {256, 256, 32}, {256, 256, 96}, {256, 256, 160}, {512, 768, 96},
    /* v6 */
    {256, 256, 256}, {256, 256, 384}, {512, 768, 256},
};

static void check_emulation_passes()
{
    double worst_all = 0.0;
    for (auto &s : SHAPES) {
        for (Mode mode : {UNIT, UNIFORM}) {
            if (mode == UNIT && s[2] > 256) continue;
            Problem p;
            make(p, s[0], s[1], s[2], mode, 12345);
            Result r = compare(mode, p.clean.data(), p.ref);
            EXPECT(r.ok(), "%dx%dx%d %s: %zu bad, worst %g, first %s", s[0],
                   s[1], s[2], mode_name(mode), r.bad, r.worst,
                   address(r).c_str());
            if (mode == UNIT)
                EXPECT(r.worst == 0.0 && p.ref.max_abs <= s[2], "unit worst");
            else if (r.worst > worst_all)
                worst_all = r.worst;
        }
    }
    printf("emulated kernel: worst err/tol %.3f in uniform mode\n",
           worst_all);
    EXPECT(worst_all > 0.05, "tolerance far wider than the emulation needs");
}

static void check_unit_refused()
{
    /* all +1: every C element is K = 512 > 256 */
    const int M = 16, N = 16, K = 512;
    std::vector<uint16_t> A((size_t)M * K, 0x3F80), B((size_t)N * K, 0x3F80);
    Reference ref;
    reference(A.data(), B.data(), M, N, K, ref);
    EXPECT(ref.max_abs == 512.0, "max_abs %g", ref.max_abs);
    std::vector<uint16_t> got((size_t)M * N, f32_to_bf16(512.f));
    Result r = compare(UNIT, got.data(), ref);
    EXPECT(r.refused && !r.ok(), "unit mode with |ref| = 512 not refused");
    EXPECT(compare(UNIFORM, got.data(), ref).ok(), "uniform refused");
}

/* -------------------------------------------------------------- mutations */

typedef std::vector<uint8_t> Mask;

/* `touched` marks the elements the mutation wrote.  Outside of it nothing
 * may be flagged.  In unit mode the flagged elements are exactly the touched
 * ones whose bits changed, and at least `min_share` of the touched. */
static void expect_caught(const char *name, const Problem &p,
                          const std::vector<uint16_t> &out,
                          const Mask &touched, double min_share)
{
    Mask mask;
    Result r = compare(p.mode, out.data(), p.ref, &mask);
    size_t n_touched = 0, n_changed = 0, outside = 0, missed = 0, flagged = 0;
    for (size_t i = 0; i < mask.size(); i++) {
        bool changed = touched[i] && out[i] != p.clean[i];
        n_touched += touched[i];
        n_changed += changed;
        flagged += mask[i];
        outside += mask[i] && !touched[i];
        missed += changed && !mask[i];
    }
    printf("%-22s %-7s touched %7zu changed %7zu flagged %7zu worst %.3g\n",
           name, mode_name(p.mode), n_touched, n_changed, flagged, r.worst);
    EXPECT(r.bad == flagged, "%s: bad %zu, mask %zu", name, r.bad, flagged);
    EXPECT(r.bad > 0 && !r.ok(), "%s (%s) not reported", name,
           mode_name(p.mode));
    EXPECT(outside == 0, "%s (%s): %zu flagged outside the mutation", name,
           mode_name(p.mode), outside);
    EXPECT(r.first_row >= 0 && mask[(size_t)r.first_row * p.N + r.first_col],
           "%s: first bad element", name);
    if (p.mode == UNIT) {
        EXPECT(missed == 0 && flagged == n_changed,
               "%s: %zu changed elements not flagged", name, missed);
        EXPECT((double)flagged >= min_share * (double)n_touched,
               "%s: %zu of %zu flagged, want a share of %.2f", name, flagged,
               n_touched, min_share);
    }
}

static void mark_tile(Mask &m, int N, int tm, int tn)
{
    for (int i = 0; i < T; i++)
        for (int j = 0; j < T; j++)
            m[(size_t)(tm * T + i) * N + tn * T + j] = 1;
}

static void check_mutations(Mode mode)
{
    /* 2 x 3 tiles of 256^2, two K-tiles of 64; K <= 256 for unit mode */
    Problem p;
    make(p, 512, 768, 128, mode, 4242);
    const int N = p.N, tiles_m = p.M / T, tiles_n = p.N / T;
    size_t n = p.clean.size();
    EXPECT(compare(mode, p.clean.data(), p.ref).ok(), "clean output bad");

    { /* one k-term dropped from one element: off by one product */
        std::vector<uint16_t> out = p.clean;
        Mask touched(n, 0);
        int i = 300, j = 517, drop = 77;
        /* uniform: a small product can stay below the bound (see the next
         * case), so drop this element's largest */
        for (int k = 0; mode == UNIFORM && k < p.K; k++)
            if (std::fabs(p.fa[(size_t)i * p.K + k] * p.fb[(size_t)j * p.K + k]) >
                std::fabs(p.fa[(size_t)i * p.K + drop] *
                          p.fb[(size_t)j * p.K + drop]))
                drop = k;
        out[(size_t)i * N + j] = f32_to_bf16(emu_acc(p, i, j, drop));
        touched[(size_t)i * N + j] = 1;
        expect_caught("drop one k-term", p, out, touched, 1.0);
    }
    if (mode == UNIFORM) {
        /* one k-term dropped from EVERY element: most are flagged */
        std::vector<uint16_t> out(n);
        Mask touched(n, 1);
        for (int i = 0; i < p.M; i++)
            for (int j = 0; j < N; j++)
                out[(size_t)i * N + j] =
                    f32_to_bf16(emu_acc(p, i, j, (i * 31 + j * 17) % p.K));
        Mask mask;
        Result r = compare(mode, out.data(), p.ref, &mask);
        printf("%-22s uniform flagged %zu of %zu\n", "drop one k-term each",
               r.bad, n);
        EXPECT((double)r.bad > 0.5 * (double)n,
               "one dropped product per element: only %zu of %zu flagged",
               r.bad, n);
    }
    { /* one K-tile skipped for one C tile.  The share: a sum of 64 values
       * of +-1 is zero with probability C(64,32) / 2^64 = 0.099 */
        std::vector<uint16_t> out = p.clean;
        Mask touched(n, 0);
        mark_tile(touched, N, 1, 2);
        for (int i = T; i < 2 * T; i++)
            for (int j = 2 * T; j < 3 * T; j++)
                out[(size_t)i * N + j] = f32_to_bf16(emu_acc(p, i, j, -1, 1));
        expect_caught("skip one K-tile", p, out, touched, 0.85);
    }
    { /* one K-tile accumulated twice */
        std::vector<uint16_t> out = p.clean;
        Mask touched(n, 0);
        mark_tile(touched, N, 0, 1);
        for (int i = 0; i < T; i++)
            for (int j = T; j < 2 * T; j++)
                out[(size_t)i * N + j] =
                    f32_to_bf16(emu_acc(p, i, j, -1, -1, 0));
        expect_caught("K-tile twice", p, out, touched, 0.85);
    }
    { /* two C tiles exchanged.  Two independent sums of 128 values of +-1
       * agree with probability C(256,128) / 2^256 = 0.050 */
        std::vector<uint16_t> out = p.clean;
        Mask touched(n, 0);
        mark_tile(touched, N, 0, 0);
        mark_tile(touched, N, 1, 1);
        for (int i = 0; i < T; i++)
            for (int j = 0; j < T; j++)
                std::swap(out[(size_t)i * N + j],
                          out[(size_t)(T + i) * N + T + j]);
        expect_caught("two tiles exchanged", p, out, touched, 0.90);
    }
    { /* tm and tn exchanged: workgroup w, which owns tile (w / tiles_n,
       * w % tiles_n), computes tile (w % tiles_m, w / tiles_m) there */
        std::vector<uint16_t> out = p.clean;
        Mask touched(n, 0);
        int moved = 0;
        for (int w = 0; w < tiles_m * tiles_n; w++) {
            int tm = w / tiles_n, tn = w % tiles_n;
            int sm = w % tiles_m, sn = w / tiles_m;
            if (sm == tm && sn == tn) continue;
            moved++;
            mark_tile(touched, N, tm, tn);
            for (int i = 0; i < T; i++)
                for (int j = 0; j < T; j++)
                    out[(size_t)(tm * T + i) * N + tn * T + j] =
                        p.clean[(size_t)(sm * T + i) * N + sn * T + j];
        }
        EXPECT(moved == 4, "moved %d tiles", moved);
        expect_caught("tm/tn exchanged", p, out, touched, 0.90);
    }
    { /* one 16 x 16 sub-block transposed: its diagonal stays */
        std::vector<uint16_t> out = p.clean;
        Mask touched(n, 0);
        int r0 = T + 5 * 16, c0 = 2 * T + 9 * 16;
        for (int i = 0; i < 16; i++)
            for (int j = 0; j < 16; j++) {
                out[(size_t)(r0 + i) * N + c0 + j] =
                    p.clean[(size_t)(r0 + j) * N + c0 + i];
                touched[(size_t)(r0 + i) * N + c0 + j] = 1;
            }
        expect_caught("sub-block transposed", p, out, touched, 0.80);
    }
    { /* one tile left at the poison value */
        std::vector<uint16_t> out = p.clean;
        Mask touched(n, 0);
        mark_tile(touched, N, 1, 0);
        for (int i = T; i < 2 * T; i++)
            for (int j = 0; j < T; j++)
                out[(size_t)i * N + j] = BF16_POISON;
        expect_caught("tile left at poison", p, out, touched, 1.0);
        Mask mask;
        Result r = compare(mode, out.data(), p.ref, &mask);
        EXPECT(r.bad == (size_t)T * T, "poison: %zu bad", r.bad);
        EXPECT(r.first_row == T && r.first_col == 0, "poison: first (%ld, "
               "%ld)", r.first_row, r.first_col);
        EXPECT(address(r).find("tile (1, 0)") != std::string::npos, "%s",
               address(r).c_str());
    }
    if (mode == UNIFORM) {
        /* truncation instead of round-to-nearest on the final conversion:
         * the error reaches 2^-7 |ref|, twice the first term of the bound */
        std::vector<uint16_t> out(n);
        Mask touched(n, 1);
        for (int i = 0; i < p.M; i++)
            for (int j = 0; j < N; j++) {
                float v = emu_acc(p, i, j);
                uint32_t u;
                memcpy(&u, &v, sizeof u);
                out[(size_t)i * N + j] = (uint16_t)(u >> 16);
            }
        expect_caught("truncated conversion", p, out, touched, 0.0);
        Result r = compare(mode, out.data(), p.ref);
        EXPECT((double)r.bad > 0.05 * (double)n,
               "truncation: only %zu of %zu flagged", r.bad, n);
    }
}

int main()
{
    check_conversions();
    check_generators();
    check_unit_refused();
    check_emulation_passes();
    check_mutations(UNIT);
    check_mutations(UNIFORM);
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
