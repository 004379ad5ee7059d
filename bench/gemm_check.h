/* Checker for the bf16 GEMM of gemm_pready.hip: inputs, a float64 reference
 * and the comparison.  Plain C++17, no HIP and no MPI: gemm_pready.hip and
 * tests/native/gemm_check_check.cpp both include it.  bf16 is uint16_t bits.
 *
 * C = A x B with A as [M][K] and B as [N][K] (the caller transposes for the
 * variants that keep B as [K][N]).
 *
 * Inputs are a hash of (seed, operand, row, col) of the element in the WHOLE
 * matrix, so a tile computed from the wrong rows cannot match:
 *   UNIT     every element +1 or -1: C is an integer with |C| <= K, exact in
 *            fp32 and in bf16 while |C| <= 256.  Compared BIT-EXACT; the
 *            comparison refuses the mode when max|ref| > 256 (a condition on
 *            the inputs, not a tolerance).
 *   UNIFORM  bf16 values in [-1, 1).  |got - ref| <= 2^-8 |ref| + K 2^-23 S
 *            with S = sum_k |a_ik b_kj|: the first term is the final
 *            round-to-nearest of an fp32 value to bf16 (unit roundoff 2^-8);
 *            the second is twice the bound (K-1) 2^-24 S of an fp32
 *            accumulation in any order (bf16 x bf16 is exact in fp32), the
 *            factor two for an MFMA that chops inside its 32-term dot where
 *            software would round.
 * A NaN in the result is always bad. */
#ifndef MPIX_BENCH_GEMM_CHECK_H
#define MPIX_BENCH_GEMM_CHECK_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace gemm_check {

enum Mode { UNIT = 0, UNIFORM = 1 };
enum Operand { OP_A = 0, OP_B = 1 };

static const uint16_t BF16_POISON = 0xFFFFu; /* a NaN; memset(0xFF) makes it */
static const double UNIT_MAX_REF = 256.0;

inline const char *mode_name(Mode m) { return m == UNIT ? "unit" : "uniform"; }

inline float bf16_to_f32(uint16_t b)
{
    uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

/* round to nearest even; a NaN stays a NaN */
inline uint16_t f32_to_bf16(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu))
        return (uint16_t)((u >> 16) | 0x0040u);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

inline bool bf16_is_nan(uint16_t b)
{
    return (b & 0x7F80u) == 0x7F80u && (b & 0x007Fu);
}

inline uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

inline uint16_t element(Mode mode, uint32_t seed, Operand op, size_t row,
                        size_t col)
{
    uint32_t h = mix32(seed * 0x9E3779B9u + (uint32_t)op * 0x85EBCA6Bu + 1u);
    h = mix32(h ^ (uint32_t)row * 0xC2B2AE35u);
    h = mix32(h + (uint32_t)col * 0x27D4EB2Fu + 0x165667B1u);
    if (mode == UNIT) return (h >> 31) ? 0xBF80u : 0x3F80u; /* -1 : +1 */
    float v = (float)(h >> 8) / (float)(1 << 24) * 2.f - 1.f;
    uint16_t b = f32_to_bf16(v);
    if (b == 0x3F80u) b = 0x3F7Fu; /* rounded up to 1: largest value below */
    return b;
}

/* row-major [rows][cols]; A is filled as [M][K], B as [N][K] */
inline void fill(Mode mode, uint32_t seed, Operand op, size_t rows,
                 size_t cols, uint16_t *out)
{
    for (size_t r = 0; r < rows; r++)
        for (size_t c = 0; c < cols; c++)
            out[r * cols + c] = element(mode, seed, op, r, c);
}

struct Reference {
    int M = 0, N = 0, K = 0;
    std::vector<double> c; /* [M][N] sum_k a_ik b_jk */
    std::vector<double> s; /* [M][N] sum_k |a_ik b_jk| */
    double max_abs = 0.0;
};

inline void reference(const uint16_t *A, const uint16_t *Bt, int M, int N,
                      int K, Reference &ref)
{
    ref.M = M; ref.N = N; ref.K = K;
    ref.c.assign((size_t)M * N, 0.0);
    ref.s.assign((size_t)M * N, 0.0);
    ref.max_abs = 0.0;
    std::vector<double> a((size_t)M * K), b((size_t)N * K);
    for (size_t i = 0; i < a.size(); i++) a[i] = (double)bf16_to_f32(A[i]);
    for (size_t i = 0; i < b.size(); i++) b[i] = (double)bf16_to_f32(Bt[i]);
    for (int i = 0; i < M; i++)
        for (int j = 0; j < N; j++) {
            const double *ar = &a[(size_t)i * K], *br = &b[(size_t)j * K];
            double c = 0.0, s = 0.0;
            for (int k = 0; k < K; k++) {
                double p = ar[k] * br[k];
                c += p;
                s += std::fabs(p);
            }
            ref.c[(size_t)i * N + j] = c;
            ref.s[(size_t)i * N + j] = s;
            if (std::fabs(c) > ref.max_abs) ref.max_abs = std::fabs(c);
        }
}

inline double tolerance(const Reference &ref, size_t idx)
{
    return std::ldexp(std::fabs(ref.c[idx]), -8) +
           (double)ref.K * std::ldexp(ref.s[idx], -23);
}

struct Result {
    bool refused = false; /* UNIT asked for with max|ref| > 256 */
    size_t bad = 0;
    /* UNIFORM: worst err / tol.  UNIT: 0 when every element is bit-exact,
     * else the worst |got - ref| (the tolerance is zero) */
    double worst = 0.0;
    long first_row = -1, first_col = -1;
    uint16_t first_got = 0;
    double first_ref = 0.0, first_tol = 0.0;
    bool ok() const { return !refused && bad == 0; }
};

/* got is [M][N] bf16 bits.  mask, when given, gets one byte per element:
 * 1 = bad. */
inline Result compare(Mode mode, const uint16_t *got, const Reference &ref,
                      std::vector<uint8_t> *mask = nullptr)
{
    Result res;
    size_t n = (size_t)ref.M * ref.N;
    if (mask) mask->assign(n, 0);
    if (mode == UNIT && ref.max_abs > UNIT_MAX_REF) {
        res.refused = true;
        return res;
    }
    for (size_t idx = 0; idx < n; idx++) {
        uint16_t g = got[idx];
        double want = ref.c[idx], tol = 0.0, ratio;
        bool bad;
        if (bf16_is_nan(g)) {
            bad = true;
            ratio = INFINITY;
        } else if (mode == UNIT) {
            /* want is an integer of at most 256: exact as float and bf16 */
            bad = g != f32_to_bf16((float)want);
            ratio = bad ? std::fabs((double)bf16_to_f32(g) - want) : 0.0;
            if (bad && ratio == 0.0) ratio = INFINITY; /* -0 for +0 */
        } else {
            tol = tolerance(ref, idx);
            double err = std::fabs((double)bf16_to_f32(g) - want);
            bad = !(err <= tol);
            ratio = tol > 0.0 ? err / tol : (err > 0.0 ? INFINITY : 0.0);
        }
        if (ratio > res.worst) res.worst = ratio;
        if (!bad) continue;
        if (mask) (*mask)[idx] = 1;
        if (res.bad++ == 0) {
            res.first_row = (long)(idx / ref.N);
            res.first_col = (long)(idx % ref.N);
            res.first_got = g;
            res.first_ref = want;
            res.first_tol = tol;
        }
    }
    return res;
}

/* where the first bad element sits: its 256^2 tile and 16 x 16 sub-block */
inline std::string address(const Result &r)
{
    if (r.first_row < 0) return "none";
    char buf[256];
    snprintf(buf, sizeof buf,
             "C[%ld][%ld] got %g (0x%04x) want %.9g tol %.3g: 256^2 tile "
             "(%ld, %ld), 16x16 sub-block (%ld, %ld) of it, element (%ld, "
             "%ld) of that",
             r.first_row, r.first_col, (double)bf16_to_f32(r.first_got),
             (unsigned)r.first_got, r.first_ref, r.first_tol,
             r.first_row / 256, r.first_col / 256, r.first_row % 256 / 16,
             r.first_col % 256 / 16, r.first_row % 16, r.first_col % 16);
    return buf;
}

/* JSON: finite numbers only */
inline double json_num(double v) { return std::isfinite(v) ? v : 1e300; }

} // namespace gemm_check

#endif
