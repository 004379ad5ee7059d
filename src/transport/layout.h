/* mpix — strided buffer layouts: validation, normalisation, addressing and
 * host copies (no HIP, no MPI dependency).
 *
 * Used by the enqueue layer (validate + normalise what the user passed), by
 * the native transport (host staging copies, granule selection for the
 * strided pull kernel) and by tests/native/layout_check.cpp.
 *
 * layout_offset() is THE definition of where message byte `pos` lives in a
 * laid-out buffer; k_pull_strided and layout_copy_out/in are checked
 * against it.  See include/mpix/mpix_layout.h for the layout itself.
 */
#ifndef MPIX_TRANSPORT_LAYOUT_H
#define MPIX_TRANSPORT_LAYOUT_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mpix/mpix_layout.h"
#include "reduce.h"

namespace mpix {

static inline MPIX_Layout layout_contiguous(uint64_t bytes)
{
    MPIX_Layout l;
    l.run_bytes = bytes;
    l.count[0] = l.count[1] = 1;
    l.stride[0] = (int64_t)bytes;
    l.stride[1] = (int64_t)bytes;
    return l;
}

/* true when the layout is one run (a level of count 1 is unused) */
static inline bool layout_is_contiguous(const MPIX_Layout &l)
{
    return l.count[0] == 1 && l.count[1] == 1;
}

static inline uint64_t layout_bytes(const MPIX_Layout &l)
{
    return l.run_bytes * l.count[0] * l.count[1];
}

/* a * b + c in int64 without overflow; false if it does not fit */
static inline bool layout_muladd(int64_t a, uint64_t b, uint64_t c,
                                 int64_t *out)
{
    if (b > (uint64_t)INT64_MAX || c > (uint64_t)INT64_MAX) return false;
    int64_t t;
    if (__builtin_mul_overflow(a, (int64_t)b, &t)) return false;
    return !__builtin_add_overflow(t, (int64_t)c, out);
}

/* 0 when `l` is a legal layout, -1 otherwise: strides of used levels are
 * positive, no byte is addressed twice (stride[0] >= run_bytes, stride[1] >=
 * extent of one plane), and neither the message length nor the extent
 * overflows.  A zero-length layout is legal.  *extent_out (optional) gets
 * the distance from the first to one past the last byte addressed. */
static inline int layout_validate(const MPIX_Layout &l,
                                  uint64_t *extent_out = nullptr)
{
    uint64_t total;
    if (__builtin_mul_overflow(l.run_bytes, l.count[0], &total)) return -1;
    if (__builtin_mul_overflow(total, l.count[1], &total)) return -1;
    if (total > (uint64_t)INT64_MAX) return -1;
    if (total == 0) {
        if (extent_out) *extent_out = 0;
        return 0;
    }
    int64_t ext = (int64_t)l.run_bytes;
    if (l.count[0] > 1) {
        if (l.stride[0] <= 0 || (uint64_t)l.stride[0] < l.run_bytes) return -1;
        if (!layout_muladd(l.stride[0], l.count[0] - 1, l.run_bytes, &ext))
            return -1;
    }
    if (l.count[1] > 1) {
        if (l.stride[1] <= 0 || l.stride[1] < ext) return -1;
        if (!layout_muladd(l.stride[1], l.count[1] - 1, (uint64_t)ext, &ext))
            return -1;
    }
    if (extent_out) *extent_out = (uint64_t)ext;
    return 0;
}

/* Canonical form of a VALID layout: levels of count 1 are dropped, a level
 * whose stride equals the extent below it is merged (into the run, or the
 * plane level into the run level), and unused levels get the strides a
 * contiguous continuation would have.  A layout that is really contiguous
 * becomes layout_contiguous(bytes); a zero-length one layout_contiguous(0).
 * Idempotent, and layout_offset() is the same function before and after. */
static inline MPIX_Layout layout_normalize(const MPIX_Layout &l)
{
    if (layout_bytes(l) == 0) return layout_contiguous(0);
    uint64_t run = l.run_bytes;
    uint64_t cnt[2] = {1, 1};
    int64_t str[2] = {0, 0};
    int n = 0;
    for (int i = 0; i < 2; i++) {
        if (l.count[i] > 1) {
            cnt[n] = l.count[i];
            str[n] = l.stride[i];
            n++;
        }
    }
    /* plane level continues the run level at the same pitch */
    if (n == 2 && (uint64_t)str[1] == (uint64_t)str[0] * cnt[0]) {
        cnt[0] *= cnt[1];
        n = 1;
    }
    while (n > 0 && (uint64_t)str[0] == run) {
        run *= cnt[0];
        cnt[0] = cnt[1];
        str[0] = str[1];
        n--;
    }
    MPIX_Layout o;
    o.run_bytes = run;
    o.count[0] = n > 0 ? cnt[0] : 1;
    o.stride[0] = n > 0 ? str[0] : (int64_t)run;
    o.count[1] = n > 1 ? cnt[1] : 1;
    o.stride[1] = n > 1 ? str[1] : o.stride[0] * (int64_t)o.count[0];
    return o;
}

/* Byte offset in the buffer of message position `pos` (< layout_bytes). */
static inline int64_t layout_offset(const MPIX_Layout &l, uint64_t pos)
{
    uint64_t r = pos / l.run_bytes;
    uint64_t o = pos % l.run_bytes;
    uint64_t plane = r / l.count[0];
    uint64_t rr = r % l.count[0];
    int64_t off = (int64_t)o;
    if (l.count[0] > 1) off += (int64_t)rr * l.stride[0];
    if (l.count[1] > 1) off += (int64_t)plane * l.stride[1];
    return off;
}

/* The same for a run of partitions: partition q is laid out as `l` at
 * q * part_stride, and the run's message is the partitions' messages one
 * after the other.  Byte offset from the first partition's buffer of message
 * position `pos` (< k * layout_bytes(l), layout_bytes(l) > 0).  THE
 * definition for everything that treats several partitions as one transfer:
 * part_layout_fold, the partition level of k_pull_strided, the expansion of
 * a run descriptor. */
static inline int64_t part_layout_offset(const MPIX_Layout &l,
                                         int64_t part_stride, uint64_t pos)
{
    const uint64_t pb = layout_bytes(l);
    const uint64_t q = pos / pb;
    return (int64_t)q * part_stride + layout_offset(l, pos - q * pb);
}

/* k partitions laid out as the NORMALISED layout `l`, part_stride apart, as
 * ONE layout: (k, part_stride) is a third, outermost level.  It folds when it
 * adds no level of its own to a strided partition: the partitions continue
 * the outermost level of `l` at its pitch (a y-face split along z:
 * part_stride == count[0] * stride[0]; with planes, count[1] * stride[1]), or
 * `l` is contiguous and the partitions become its only level (rows with a
 * gap; no gap: one run).  Anything else is refused, also a one-level layout
 * with an unrelated part stride, which MPIX_Layout could hold as planes: the
 * run then goes to the kernel variant with a partition level, and what folds
 * costs exactly what the same bytes cost as one plain strided message.
 * true: *out is normalised and layout_offset(*out, pos) ==
 * part_layout_offset(l, part_stride, pos) for every pos.  k == 1 folds to
 * `l`.  Needs layout_bytes(l) > 0 and part_stride >= the extent of `l`. */
static inline bool part_layout_fold(const MPIX_Layout &l, uint64_t k,
                                    int64_t part_stride, MPIX_Layout *out)
{
    if (k == 0 || layout_bytes(l) == 0) return false;
    if (k == 1) {
        *out = l;
        return true;
    }
    if (part_stride <= 0) return false;
    MPIX_Layout o = l;
    if (l.count[1] > 1) {
        if ((uint64_t)part_stride != l.count[1] * (uint64_t)l.stride[1])
            return false;
        o.count[1] = l.count[1] * k;
    } else if (l.count[0] > 1) {
        if ((uint64_t)part_stride != l.count[0] * (uint64_t)l.stride[0])
            return false;
        o.count[0] = l.count[0] * k;
    } else {
        if ((uint64_t)part_stride < l.run_bytes) return false;
        o.count[0] = k;
        o.stride[0] = part_stride;
    }
    *out = layout_normalize(o);
    return true;
}

/* Shared walk of message bytes [pos, pos + n): calls f(buffer_offset,
 * message_offset_from_pos, len) once per (piece of a) run. */
template <typename F>
static inline void layout_for_runs(const MPIX_Layout &l, uint64_t pos,
                                   uint64_t n, F f)
{
    uint64_t done = 0;
    while (done < n) {
        uint64_t p = pos + done;
        uint64_t in_run = p % l.run_bytes;
        uint64_t len = l.run_bytes - in_run;
        if (len > n - done) len = n - done;
        f(layout_offset(l, p), done, len);
        done += len;
    }
}

/* message bytes [pos, pos + n) of laid-out host buffer `buf` -> dst */
static inline void layout_copy_out(void *dst, const void *buf,
                                   const MPIX_Layout &l, uint64_t pos,
                                   uint64_t n)
{
    layout_for_runs(l, pos, n, [&](int64_t off, uint64_t m, uint64_t len) {
        memcpy((char *)dst + m, (const char *)buf + off, len);
    });
}

/* src -> message bytes [pos, pos + n) of laid-out host buffer `buf` */
static inline void layout_copy_in(void *buf, const MPIX_Layout &l,
                                  uint64_t pos, const void *src, uint64_t n)
{
    layout_for_runs(l, pos, n, [&](int64_t off, uint64_t m, uint64_t len) {
        memcpy((char *)buf + off, (const char *)src + m, len);
    });
}

/* src COMBINED into message bytes [pos, pos + n) of laid-out host buffer
 * `buf` (a reducing strided receive: reduce.h).  pos, n and the layout's run
 * are multiples of the element size, so no element straddles a piece. */
static inline void layout_reduce_in(void *buf, const MPIX_Layout &l,
                                    uint64_t pos, const void *src, uint64_t n,
                                    int type, int op)
{
    const uint32_t es = reduce_elem_size(type);
    layout_for_runs(l, pos, n, [&](int64_t off, uint64_t m, uint64_t len) {
        reduce_host((char *)buf + off, (const char *)src + m, len / es, type,
                    op);
    });
}

/* OR of everything a transfer unit must divide on one side */
static inline uint64_t layout_align_bits(const MPIX_Layout &l, uint64_t base)
{
    uint64_t bits = l.run_bytes | base;
    if (l.count[0] > 1) bits |= (uint64_t)l.stride[0];
    if (l.count[1] > 1) bits |= (uint64_t)l.stride[1];
    return bits;
}

/* Largest power of two <= 16 that divides both runs, all strides in use,
 * both base addresses and, for a run of partitions, both part strides (0
 * when there is no partition level): every unit of that size at a message position that
 * is a multiple of it lies inside one run on both sides, aligned.  16 selects
 * the vector path of k_pull_strided, 8/4/2/1 its element path. */
static inline uint32_t layout_granule(const MPIX_Layout &a, uint64_t base_a,
                                      const MPIX_Layout &b, uint64_t base_b,
                                      int64_t part_stride_a = 0,
                                      int64_t part_stride_b = 0)
{
    uint64_t bits = layout_align_bits(a, base_a) | layout_align_bits(b, base_b);
    /* a run of partitions: every partition has to start aligned too */
    bits |= (uint64_t)part_stride_a | (uint64_t)part_stride_b;
    uint32_t g = 16;
    while (g > 1 && (bits & (g - 1)) != 0) g >>= 1;
    return g;
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_LAYOUT_H */
