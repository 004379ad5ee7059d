/* Stand-alone CPU check of the reducing receive's definition
 * (src/transport/reduce.h) and planner (src/transport/reduce_plan.h).
 * Built with AddressSanitizer + UBSan by tests/test_reduce_ref.py and run as
 * a program.
 *
 *  - combine and reduce_host for all 18 type/op pairs against references
 *    that share no code with reduce.h: float64 arithmetic rounded once
 *    (nearbyint on a scaled double) for f16, widen / add / pick the nearer
 *    neighbour, the even one on a tie, for bf16, the native types otherwise
 *    (integers through __builtin_add_overflow);
 *  - inputs: random normal values at several scales, exact ties of both
 *    parities for bf16 and f16, integer wrap at both ends;
 *  - the comparison itself: a bf16 sum that truncates instead of rounding,
 *    and a reduce that drops the operand in the tail, must both be flagged;
 *  - plan_reduce: merging, the cut at an overlapping destination, tile
 *    counts.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../src/transport/reduce_plan.h"

using namespace mpix;

static int g_failed = 0;

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            g_failed++;                                                   \
        }                                                                 \
    } while (0)

/* ------------------------------------------------------------- references */

static double ref_half_value(uint16_t h)
{
    const int exp = (h >> 10) & 31, man = h & 1023;
    double v;
    if (exp == 31) v = man ? NAN : INFINITY;
    else if (exp == 0) v = ldexp((double)man, -24);
    else v = ldexp((double)(1024 + man), exp - 25);
    return (h & 0x8000) ? -v : v;
}

/* v rounded ONCE to the nearest half (ties to even: the default rounding
 * mode of nearbyint), as a double */
static double ref_round_to_half(double v)
{
    if (v == 0.0 || isinf(v)) return v;
    const double a = fabs(v);
    double r;
    if (a < ldexp(1.0, -14)) {
        r = ldexp(nearbyint(ldexp(a, 24)), -24);
    } else {
        const int e = ilogb(a);
        r = ldexp(nearbyint(ldexp(a, 10 - e)), e - 10);
    }
    if (r >= 65520.0) r = INFINITY;
    return v < 0 ? -r : r;
}

/* bits of a double that is exactly a half */
static uint16_t ref_half_bits(double v)
{
    const uint16_t sign = signbit(v) ? 0x8000 : 0;
    const double a = fabs(v);
    if (a == 0.0) return sign;
    if (isinf(a)) return sign | 0x7c00;
    if (a < ldexp(1.0, -14)) return sign | (uint16_t)ldexp(a, 24);
    const int e = ilogb(a);
    const int man = (int)ldexp(a, 10 - e) - 1024;
    return sign | (uint16_t)(((e + 15) << 10) | man);
}

static float ref_bf16_value(uint16_t h)
{
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

/* the nearer of the two bf16 neighbours of s, the even one on a tie
 * (s finite and below the largest bf16) */
static uint16_t ref_bf16_round(float s)
{
    uint32_t u;
    memcpy(&u, &s, 4);
    const uint16_t lo = (uint16_t)(u >> 16), hi = (uint16_t)(lo + 1);
    const double dl = fabs((double)s - (double)ref_bf16_value(lo));
    const double dh = fabs((double)ref_bf16_value(hi) - (double)s);
    if (dl < dh) return lo;
    if (dh < dl) return hi;
    return (lo & 1) ? hi : lo;
}

template <int TYPE> struct Ref;
template <> struct Ref<RED_F32> {
    static float combine(int op, float a, float b)
    {
        return op == RED_SUM ? a + b : op == RED_MAX ? fmaxf(a, b)
                                                     : fminf(a, b);
    }
};
template <> struct Ref<RED_F64> {
    static double combine(int op, double a, double b)
    {
        return op == RED_SUM ? a + b : op == RED_MAX ? fmax(a, b) : fmin(a, b);
    }
};
template <> struct Ref<RED_BF16> {
    static uint16_t combine(int op, uint16_t a, uint16_t b)
    {
        const float fa = ref_bf16_value(a), fb = ref_bf16_value(b);
        if (op == RED_SUM) return ref_bf16_round(fa + fb);
        return ((op == RED_MAX) == (fa >= fb)) ? a : b;
    }
};
template <> struct Ref<RED_F16> {
    static uint16_t combine(int op, uint16_t a, uint16_t b)
    {
        const double da = ref_half_value(a), db = ref_half_value(b);
        if (op == RED_SUM) return ref_half_bits(ref_round_to_half(da + db));
        return ((op == RED_MAX) == (da >= db)) ? a : b;
    }
};
template <> struct Ref<RED_I32> {
    static int32_t combine(int op, int32_t a, int32_t b)
    {
        int32_t r;
        if (op == RED_SUM) {
            (void)__builtin_add_overflow(a, b, &r);
            return r;
        }
        return op == RED_MAX ? (a > b ? a : b) : (a < b ? a : b);
    }
};
template <> struct Ref<RED_I64> {
    static int64_t combine(int op, int64_t a, int64_t b)
    {
        int64_t r;
        if (op == RED_SUM) {
            (void)__builtin_add_overflow(a, b, &r);
            return r;
        }
        return op == RED_MAX ? (a > b ? a : b) : (a < b ? a : b);
    }
};

/* ----------------------------------------------------------------- inputs */

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static double uniform()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(g_rng >> 11) + 0.5) / 9007199254740992.0;
}
static double normal()
{
    return sqrt(-2.0 * log(uniform())) * cos(6.283185307179586 * uniform());
}

template <int TYPE> static typename Red<TYPE>::T from_double(double v);
template <> float from_double<RED_F32>(double v) { return (float)v; }
template <> double from_double<RED_F64>(double v) { return v; }
template <> uint16_t from_double<RED_BF16>(double v)
{
    const float f = (float)v;
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)(u >> 16);
}
template <> uint16_t from_double<RED_F16>(double v)
{
    return ref_half_bits(ref_round_to_half(v));
}
template <> int32_t from_double<RED_I32>(double v)
{
    return (int32_t)(int64_t)(v * 1e6); /* wraps for the large scales */
}
template <> int64_t from_double<RED_I64>(double v)
{
    return (int64_t)(v * 1e15);
}

template <int TYPE>
static bool both_zero(typename Red<TYPE>::T a, typename Red<TYPE>::T b)
{
    typedef typename Red<TYPE>::T T;
    if (TYPE == RED_BF16 || TYPE == RED_F16) {
        uint16_t x, y;
        memcpy(&x, &a, 2);
        memcpy(&y, &b, 2);
        return ((x | y) & 0x7fff) == 0;
    }
    return a == (T)0 && b == (T)0;
}

/* --------------------------------------------------------- the comparison */

/* How many of the n results in `got` differ, bit for bit, from the
 * reference combine of a[i] and b[i].  Pairs of two zeros are left out
 * under MAX/MIN: the sign of that result is unspecified. */
template <int TYPE>
static size_t mismatches(const std::vector<typename Red<TYPE>::T> &got,
                         const std::vector<typename Red<TYPE>::T> &a,
                         const std::vector<typename Red<TYPE>::T> &b, int op)
{
    typedef typename Red<TYPE>::T T;
    size_t bad = 0;
    for (size_t i = 0; i < a.size(); i++) {
        if (op != RED_SUM && both_zero<TYPE>(a[i], b[i])) continue;
        const T want = Ref<TYPE>::combine(op, a[i], b[i]);
        if (memcmp(&want, &got[i], sizeof(T)) != 0) bad++;
    }
    return bad;
}

template <int TYPE>
static void check_pairs(const char *what,
                        const std::vector<typename Red<TYPE>::T> &a,
                        const std::vector<typename Red<TYPE>::T> &b)
{
    typedef typename Red<TYPE>::T T;
    for (int op = 0; op < RED_NOPS; op++) {
        std::vector<T> one(a.size()), all(a);
        for (size_t i = 0; i < a.size(); i++)
            one[i] = Red<TYPE>::combine(op, a[i], b[i]);
        reduce_host(all.data(), b.data(), a.size(), TYPE, op);
        const size_t bad1 = mismatches<TYPE>(one, a, b, op);
        const size_t bad2 = mismatches<TYPE>(all, a, b, op);
        if (bad1 || bad2) {
            printf("FAILED %s type %d op %d: combine %zu, reduce_host %zu of "
                   "%zu differ from the reference\n", what, TYPE, op, bad1,
                   bad2, a.size());
            g_failed++;
        }
    }
}

template <int TYPE> static void check_random()
{
    typedef typename Red<TYPE>::T T;
    const double scales[] = {1.0, 1e-3, 1e3, 3e-6, 40.0};
    std::vector<T> a, b;
    for (double sa : scales)
        for (double sb : scales)
            for (int i = 0; i < 400; i++) {
                a.push_back(from_double<TYPE>(normal() * sa));
                b.push_back(from_double<TYPE>(normal() * sb));
            }
    /* cancellation, equal operands and zeros of both signs */
    for (int i = 0; i < 200; i++) {
        const T x = from_double<TYPE>(normal());
        a.push_back(x);
        b.push_back(x);
        a.push_back(x);
        b.push_back(from_double<TYPE>(-normal() * 1e-2));
        a.push_back(from_double<TYPE>(i & 1 ? 0.0 : -0.0));
        b.push_back(i & 2 ? x : from_double<TYPE>(0.0));
    }
    check_pairs<TYPE>("random", a, b);
}

/* Pairs whose exact sum lies halfway between two values of the format:
 * (1 + m * ulp) * 2^e plus half an ulp * 2^e, for every mantissa m (even and
 * odd: both parities), a few exponents, both signs.  The result must be the
 * neighbour with the even mantissa. */
static void check_ties()
{
    std::vector<uint16_t> a, b, even;
    for (int e = -6; e <= 6; e += 3)
        for (int m = 0; m < 128; m++)
            for (int neg = 0; neg < 2; neg++) {
                const uint16_t s = neg ? 0x8000 : 0;
                a.push_back(s | (uint16_t)(((127 + e) << 7) | m));
                b.push_back(s | (uint16_t)((127 + e - 8) << 7));
                const uint16_t hi = (uint16_t)((((127 + e) << 7) | m) + 1);
                even.push_back(s | ((m & 1) ? hi : (uint16_t)(hi - 1)));
            }
    check_pairs<RED_BF16>("bf16 ties", a, b);
    for (size_t i = 0; i < a.size(); i++)
        EXPECT(Red<RED_BF16>::combine(RED_SUM, a[i], b[i]) == even[i]);

    a.clear(), b.clear(), even.clear();
    for (int e = -3; e <= 6; e += 3)
        for (int m = 0; m < 1024; m++)
            for (int neg = 0; neg < 2; neg++) {
                const uint16_t s = neg ? 0x8000 : 0;
                a.push_back(s | (uint16_t)(((15 + e) << 10) | m));
                b.push_back(s | (uint16_t)((15 + e - 11) << 10));
                const uint16_t hi = (uint16_t)((((15 + e) << 10) | m) + 1);
                even.push_back(s | ((m & 1) ? hi : (uint16_t)(hi - 1)));
            }
    /* and in the subnormal range of f16, where the f32 sum is exact */
    for (int m = 1; m < 1024; m++) {
        a.push_back((uint16_t)m);
        b.push_back((uint16_t)(m ^ 0x155));
        even.push_back((uint16_t)(m + (m ^ 0x155)));
    }
    check_pairs<RED_F16>("f16 ties", a, b);
    for (size_t i = 0; i < a.size(); i++)
        EXPECT(Red<RED_F16>::combine(RED_SUM, a[i], b[i]) == even[i]);
    /* overflow: 65504 + 16 is the tie that rounds to infinity, + 8 stays */
    EXPECT(Red<RED_F16>::combine(RED_SUM, 0x7bff, 0x4c00) == 0x7c00);
    EXPECT(Red<RED_F16>::combine(RED_SUM, 0x7bff, 0x4800) == 0x7bff);
    EXPECT(Red<RED_F16>::combine(RED_SUM, 0xfbff, 0xcc00) == 0xfc00);
}

static void check_wrap()
{
    const std::vector<int32_t> a32 = {INT32_MAX, INT32_MIN, INT32_MAX,
                                      INT32_MIN, -1, 0x40000000},
                               b32 = {1, -1, INT32_MAX, INT32_MIN, 1,
                                      0x40000000};
    check_pairs<RED_I32>("i32 wrap", a32, b32);
    EXPECT(Red<RED_I32>::combine(RED_SUM, INT32_MAX, 1) == INT32_MIN);
    EXPECT(Red<RED_I32>::combine(RED_SUM, INT32_MIN, -1) == INT32_MAX);
    const std::vector<int64_t> a64 = {INT64_MAX, INT64_MIN, INT64_MAX,
                                      INT64_MIN, -1, 1ll << 62},
                               b64 = {1, -1, INT64_MAX, INT64_MIN, 1,
                                      1ll << 62};
    check_pairs<RED_I64>("i64 wrap", a64, b64);
    EXPECT(Red<RED_I64>::combine(RED_SUM, INT64_MAX, 1) == INT64_MIN);
    EXPECT(Red<RED_I64>::combine(RED_SUM, INT64_MIN, -1) == INT64_MAX);
    EXPECT(Red<RED_I64>::combine(RED_MAX, INT64_MIN, 3) == 3);
    EXPECT(Red<RED_I32>::combine(RED_MIN, INT32_MIN, 3) == INT32_MIN);
}

/* the comparison must flag a combine that is subtly wrong */
static void check_the_check()
{
    /* (a) a bf16 sum that truncates the f32 sum instead of rounding it */
    std::vector<uint16_t> a, b;
    for (int i = 0; i < 2000; i++) {
        a.push_back(from_double<RED_BF16>(normal()));
        b.push_back(from_double<RED_BF16>(normal()));
    }
    std::vector<uint16_t> wrong(a.size());
    for (size_t i = 0; i < a.size(); i++) {
        const float s = ref_bf16_value(a[i]) + ref_bf16_value(b[i]);
        uint32_t u;
        memcpy(&u, &s, 4);
        wrong[i] = (uint16_t)(u >> 16);
    }
    const size_t flagged = mismatches<RED_BF16>(wrong, a, b, RED_SUM);
    printf("truncating bf16 sum: %zu of %zu flagged\n", flagged, a.size());
    EXPECT(flagged > a.size() / 10);

    /* (b) a reduce that forgets the operand in the n % 4 tail */
    std::vector<float> fa, fb;
    for (int i = 0; i < 1027; i++) {
        fa.push_back((float)normal());
        fb.push_back((float)normal() + 3.0f);
    }
    std::vector<float> got(fa);
    reduce_host(got.data(), fb.data(), fa.size() & ~(size_t)3, RED_F32,
                RED_SUM);
    EXPECT(mismatches<RED_F32>(got, fa, fb, RED_SUM) == 3);
    reduce_host(got.data() + 1024, fb.data() + 1024, 3, RED_F32, RED_SUM);
    EXPECT(mismatches<RED_F32>(got, fa, fb, RED_SUM) == 0);
}

/* ------------------------------------------------------------ plan_reduce */

static ReduceSeg seg(uint64_t dst, uint64_t src, uint64_t bytes,
                     uint32_t type = RED_F32, uint32_t op = RED_SUM)
{
    return ReduceSeg{(void *)(uintptr_t)dst, (const void *)(uintptr_t)src,
                     bytes, type, op};
}

static void check_plan()
{
    const uint64_t T = MPIX_REDUCE_TILE, D = 0x10000000, S = 0x50000000;
    EXPECT(T == 16384);
    EXPECT(sizeof(ReduceTable) <= 4096);
    ReduceTable t;

    /* merging: both sides continue AND type and op agree */
    {
        const ReduceSeg in[] = {
            seg(D, S, 4096), seg(D + 4096, S + 4096, 4096),
            seg(D + 8192, S + 8192, 4096, RED_F32, RED_MAX),
            seg(D + 12288, S + 12288, 4096, RED_I32, RED_MAX),
            seg(D + 16384, S + 16384, 4096, RED_I32, RED_MAX),
            seg(D + 20480, S + 99999 * 16, 4096, RED_I32, RED_MAX)};
        EXPECT(plan_reduce(in, 6, T, &t) == 6);
        EXPECT(t.n == 4);
        EXPECT(t.e[0].bytes == 8192 && t.e[0].op == RED_SUM);
        EXPECT(t.e[1].bytes == 4096 && t.e[1].type == RED_F32 &&
               t.e[1].op == RED_MAX);
        EXPECT(t.e[2].bytes == 8192 && t.e[2].type == RED_I32);
        EXPECT(t.e[3].bytes == 4096);
        EXPECT(reduce_total_tiles(t) == 4);
    }
    /* a length off the 16-byte grid ends the run, as in plan_pulls */
    {
        const ReduceSeg in[] = {seg(D, S, 20), seg(D + 20, S + 20, 16)};
        EXPECT(plan_reduce(in, 2, T, &t) == 2);
        EXPECT(t.n == 2);
    }
    /* the cut: partial overlap, identical ranges; adjacent ranges do NOT */
    {
        const ReduceSeg part[] = {seg(D, S, 100), seg(D + 96, S + 4096, 100)};
        EXPECT(plan_reduce(part, 2, T, &t) == 1);
        EXPECT(t.n == 1 && t.e[0].bytes == 100);
        const ReduceSeg same[] = {seg(D, S, 4096), seg(D, S + 4096, 4096)};
        EXPECT(plan_reduce(same, 2, T, &t) == 1);
        EXPECT(t.n == 1);
        const ReduceSeg adj[] = {seg(D, S, 4096), seg(D + 4096, S + 8192, 4096),
                                 seg(D - 64, S + 16384, 64)};
        EXPECT(plan_reduce(adj, 3, T, &t) == 3);
        EXPECT(t.n == 3);
        /* inside an earlier, merged entry, behind a disjoint one */
        const ReduceSeg deep[] = {
            seg(D, S, 4096), seg(D + 4096, S + 4096, 4096),
            seg(D + 65536, S + 65536, 4096), seg(D + 4092, S + 32768, 8),
            seg(D + 131072, S + 131072, 8)};
        EXPECT(plan_reduce(deep, 5, T, &t) == 3);
        EXPECT(t.n == 2 && t.e[0].bytes == 8192);
        /* ... and that entry opens the next launch */
        EXPECT(plan_reduce(deep + 3, 2, T, &t) == 2);
        EXPECT(t.n == 2 && t.e[0].bytes == 8);
        /* contained, and containing */
        const ReduceSeg in1[] = {seg(D, S, 4096), seg(D + 8, S + 8192, 8)};
        EXPECT(plan_reduce(in1, 2, T, &t) == 1);
        const ReduceSeg in2[] = {seg(D + 8, S, 8), seg(D, S + 8192, 4096)};
        EXPECT(plan_reduce(in2, 2, T, &t) == 1);
    }
    /* tile counts */
    {
        const uint64_t odd = 3 * T + 4 * 1237 + 4;
        const ReduceSeg in[] = {seg(D, S, T - 16),
                                seg(D + 0x100000, S + 0x100000, T),
                                seg(D + 0x200000, S + 0x200000, T + 16),
                                seg(D + 0x300000, S + 0x300000, odd)};
        EXPECT(plan_reduce(in, 4, T, &t) == 4);
        EXPECT(t.n == 4);
        EXPECT(t.tile_end[0] == 1 && t.tile_end[1] == 2 &&
               t.tile_end[2] == 4 && t.tile_end[3] == 8);
        EXPECT(reduce_total_tiles(t) == 8);
    }
    /* capacity, the empty batch, 64-bit sizes */
    {
        std::vector<ReduceSeg> many;
        for (uint64_t i = 0; i < 70; i++)
            many.push_back(seg(D + i * 4096, S + i * 8192, 4096));
        EXPECT(plan_reduce(many.data(), many.size(), T, &t) ==
               MPIX_PULL_BATCH);
        EXPECT(t.n == MPIX_PULL_BATCH);
        EXPECT(plan_reduce(many.data(), 0, T, &t) == 0);
        EXPECT(t.n == 0 && reduce_total_tiles(t) == 0);
        const uint64_t big = 5ull << 32;
        const ReduceSeg in[] = {seg(1ull << 40, 1ull << 41, big),
                                seg((1ull << 40) + big - 4, 1ull << 42, 8)};
        EXPECT(plan_reduce(in, 2, T, &t) == 1);
        EXPECT(reduce_total_tiles(t) == big / T);
    }
}

int main()
{
    for (int t = 0; t < RED_NTYPES; t++)
        EXPECT(reduce_type_ok(t) && reduce_elem_size(t) != 0);
    EXPECT(!reduce_type_ok(-1) && !reduce_type_ok(RED_NTYPES));
    EXPECT(!reduce_op_ok(-1) && !reduce_op_ok(RED_NOPS));
    EXPECT(reduce_elem_size(RED_BF16) == 2 && reduce_elem_size(RED_F64) == 8 &&
           reduce_elem_size(RED_I32) == 4 && reduce_elem_size(99) == 0);
    check_random<RED_F32>();
    check_random<RED_F64>();
    check_random<RED_BF16>();
    check_random<RED_F16>();
    check_random<RED_I32>();
    check_random<RED_I64>();
    check_ties();
    check_wrap();
    check_the_check();
    check_plan();
    if (g_failed) {
        printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
