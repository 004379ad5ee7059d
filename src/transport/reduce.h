/* mpix — the combine of a reducing receive (no HIP, no MPI dependency).
 *
 * MPIX_Irecv_reduce_enqueue / MPIX_Precv_init_reduce leave
 * buf[i] = buf[i] op msg[i].  combine() in here is THE definition of that
 * one step, per element type: the pull kernels (pull_kernels.h,
 * k_pull_reduce*), the host path (reduce_host) and
 * tests/native/reduce_check.cpp all go through it, so host and device agree
 * bit for bit wherever the rule below defines the result.
 *
 *   f32, f64   IEEE add
 *   f16        the correctly rounded half sum: both halves widen exactly to
 *              f32, the f32 sum is correctly rounded to 24 bits, and
 *              24 >= 2 * 11 + 2 makes the second rounding (to half, nearest
 *              even) innocuous; sums below 2^-14 are exact in f32
 *   bf16       round-to-nearest-even to bf16 of the f32 sum of the two
 *              widened values
 *   i32, i64   two's-complement wrap (the arithmetic is unsigned)
 *   MAX, MIN   the larger / smaller value
 *
 * NaNs and the sign of a zero under MAX/MIN are unspecified; subnormal f32
 * and bf16 results follow the compiler's denormal mode.  The 16-bit types
 * travel as their bit patterns (uint16_t) and are converted by bit
 * arithmetic: no __half, no hardware conversion whose rounding could differ
 * between the two sides.
 */
#ifndef MPIX_TRANSPORT_REDUCE_H
#define MPIX_TRANSPORT_REDUCE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MPIX_RED_HD __host__ __device__
#else
#define MPIX_RED_HD
#endif

namespace mpix {

/* the values of MPIX_F32 .. and MPIX_SUM .. of mpix.h (asserted equal in
 * enqueue.cpp; this header does not pull in mpi.h) */
enum RedType { RED_F32 = 0, RED_F64, RED_BF16, RED_F16, RED_I32, RED_I64,
               RED_NTYPES };
enum RedOp { RED_SUM = 0, RED_MAX, RED_MIN, RED_NOPS };

/* bytes of one element; 0 for an unknown type */
MPIX_RED_HD static inline uint32_t reduce_elem_size(int type)
{
    switch (type) {
    case RED_F32: case RED_I32: return 4;
    case RED_F64: case RED_I64: return 8;
    case RED_BF16: case RED_F16: return 2;
    default: return 0;
    }
}

static inline bool reduce_type_ok(int type)
{
    return type >= 0 && type < RED_NTYPES;
}
static inline bool reduce_op_ok(int op) { return op >= 0 && op < RED_NOPS; }

/* ------------------------------------------------------- bit conversions */

MPIX_RED_HD static inline float red_bits_f32(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

MPIX_RED_HD static inline uint32_t red_f32_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

MPIX_RED_HD static inline float red_bf16_to_f32(uint16_t h)
{
    return red_bits_f32((uint32_t)h << 16);
}

/* round to nearest, ties to even; a NaN stays one */
MPIX_RED_HD static inline uint16_t red_f32_to_bf16(float f)
{
    const uint32_t u = red_f32_bits(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

/* exact */
MPIX_RED_HD static inline float red_f16_to_f32(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t exp = (h >> 10) & 0x1fu;
    uint32_t man = h & 0x3ffu;
    if (exp == 31) return red_bits_f32(sign | 0x7f800000u | (man << 13));
    if (exp != 0)
        return red_bits_f32(sign | ((exp + 112u) << 23) | (man << 13));
    if (man == 0) return red_bits_f32(sign);
    /* subnormal: man * 2^-24; shift its leading one up to bit 10 */
    const uint32_t lz = (uint32_t)__builtin_clz(man) - 21u;
    man <<= lz;
    return red_bits_f32(sign | ((113u - lz) << 23) | ((man & 0x3ffu) << 13));
}

/* round to nearest, ties to even: overflow to infinity from 65520 on,
 * subnormal halves below 2^-14, zero up to and including 2^-25 */
MPIX_RED_HD static inline uint16_t red_f32_to_f16(float f)
{
    const uint32_t u = red_f32_bits(f);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
    if (a < 0x38800000u) {
        const uint32_t shift = 126u - (a >> 23);
        if (shift > 24u) return sign;
        const uint32_t m = (a & 0x7fffffu) | 0x800000u;
        uint32_t q = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u);
        const uint32_t half = 1u << (shift - 1u);
        if (rem > half || (rem == half && (q & 1u))) q++;
        return (uint16_t)(sign | q);
    }
    uint32_t h = (a - 0x38000000u) >> 13;
    const uint32_t rem = a & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
    return (uint16_t)(sign | h);
}

/* ---------------------------------------------------------------- combine */

template <typename T>
MPIX_RED_HD static inline T red_pick(int op, T a, T b)
{
    return op == RED_MAX ? (b > a ? b : a) : (b < a ? b : a);
}

/* Red<TYPE>::T is how an element of TYPE sits in memory;
 * Red<TYPE>::combine(op, a, b) is a op b */
template <int TYPE> struct Red;

template <> struct Red<RED_F32> {
    typedef float T;
    MPIX_RED_HD static inline T combine(int op, T a, T b)
    {
        return op == RED_SUM ? a + b : red_pick(op, a, b);
    }
};

template <> struct Red<RED_F64> {
    typedef double T;
    MPIX_RED_HD static inline T combine(int op, T a, T b)
    {
        return op == RED_SUM ? a + b : red_pick(op, a, b);
    }
};

template <> struct Red<RED_BF16> {
    typedef uint16_t T;
    MPIX_RED_HD static inline T combine(int op, T a, T b)
    {
        const float fa = red_bf16_to_f32(a), fb = red_bf16_to_f32(b);
        if (op == RED_SUM) return red_f32_to_bf16(fa + fb);
        return red_pick(op, fa, fb) == fa ? a : b;
    }
};

template <> struct Red<RED_F16> {
    typedef uint16_t T;
    MPIX_RED_HD static inline T combine(int op, T a, T b)
    {
        const float fa = red_f16_to_f32(a), fb = red_f16_to_f32(b);
        if (op == RED_SUM) return red_f32_to_f16(fa + fb);
        return red_pick(op, fa, fb) == fa ? a : b;
    }
};

template <> struct Red<RED_I32> {
    typedef int32_t T;
    MPIX_RED_HD static inline T combine(int op, T a, T b)
    {
        if (op == RED_SUM) return (T)((uint32_t)a + (uint32_t)b);
        return red_pick(op, a, b);
    }
};

template <> struct Red<RED_I64> {
    typedef int64_t T;
    MPIX_RED_HD static inline T combine(int op, T a, T b)
    {
        if (op == RED_SUM) return (T)((uint64_t)a + (uint64_t)b);
        return red_pick(op, a, b);
    }
};

/* ------------------------------------------------------------ host buffers */

template <int TYPE>
static inline void reduce_host_typed(void *dst, const void *src, uint64_t n,
                                     int op)
{
    typedef typename Red<TYPE>::T T;
    char *d = (char *)dst;
    const char *s = (const char *)src;
    for (uint64_t i = 0; i < n; i++) {
        T a, b;
        memcpy(&a, d + i * sizeof(T), sizeof(T));
        memcpy(&b, s + i * sizeof(T), sizeof(T));
        a = Red<TYPE>::combine(op, a, b);
        memcpy(d + i * sizeof(T), &a, sizeof(T));
    }
}

/* dst[i] = dst[i] op src[i] for n_elems elements; type and op are valid */
static inline void reduce_host(void *dst, const void *src, uint64_t n_elems,
                               int type, int op)
{
    switch (type) {
    case RED_F32: reduce_host_typed<RED_F32>(dst, src, n_elems, op); break;
    case RED_F64: reduce_host_typed<RED_F64>(dst, src, n_elems, op); break;
    case RED_BF16: reduce_host_typed<RED_BF16>(dst, src, n_elems, op); break;
    case RED_F16: reduce_host_typed<RED_F16>(dst, src, n_elems, op); break;
    case RED_I32: reduce_host_typed<RED_I32>(dst, src, n_elems, op); break;
    case RED_I64: reduce_host_typed<RED_I64>(dst, src, n_elems, op); break;
    default: break;
    }
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_REDUCE_H */
