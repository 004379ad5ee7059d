/* mpix — completion words of the batched pull: host-side bookkeeping (no HIP
 * dependency, checked on its own by tests/native/done_ring_check.cpp).
 *
 * With MPIX_PULL_DONE=word a pull kernel tells the proxy that it
 * has finished by storing a sequence number into a 64-bit word in pinned host
 * memory (the kernel side is pull_signal_done in pull_kernels.h) instead of
 * through an event recorded behind the launch; with MPIX_PULL_DONE=tail a
 * one-thread kernel behind the copy stores it (k_pull_tail).  The words form
 * a small ring of MPIX_DONE_SLOTS; each slot also owns a 32-bit arrival
 * counter in device memory, which the arrival of the kernel's last block
 * leaves at 0 again (tail does not use it).
 *
 * A batch ACQUIRES a slot and with it a fresh sequence number, hands both to
 * the kernel, tests the word with done_seen(), and RELEASES the slot once
 * the word was seen (or the batch was failed).  Rules:
 *
 *  - sequence numbers are 64-bit, start at 1 and only grow, so no two uses
 *    of a slot ever share one, whatever the count of batches (2^32 is not a
 *    boundary), and 0 — what a fresh word holds — is never one;
 *  - "seen" is equality with the batch's own number: the word of the slot's
 *    previous use holds an older number and is never taken for the new one,
 *    and the ring does not need to clear words between uses;
 *  - slots are released in any order (batches on different streams finish
 *    in any order);
 *  - a full ring does not block: acquire() returns -1 and the caller sends
 *    that batch down the event path.
 */
#ifndef MPIX_TRANSPORT_DONE_RING_H
#define MPIX_TRANSPORT_DONE_RING_H

#include <stdint.h>

namespace mpix {

#define MPIX_DONE_SLOTS 16

struct DoneRing {
    uint64_t next_seq = 1;
    /* the number the slot's current user waits for; 0 = free */
    uint64_t waiting[MPIX_DONE_SLOTS] = {};
    uint32_t cursor = 0; /* where the search for a free slot starts */
    uint32_t in_use = 0;
};

/* A free slot and a fresh sequence number for it, or -1 (ring full: nothing
 * changed, not even the sequence counter). */
static inline int done_acquire(DoneRing *r, uint64_t *seq)
{
    if (r->in_use == MPIX_DONE_SLOTS) return -1;
    for (uint32_t i = 0; i < MPIX_DONE_SLOTS; i++) {
        const uint32_t s = (r->cursor + i) % MPIX_DONE_SLOTS;
        if (r->waiting[s] != 0) continue;
        if (r->next_seq == 0) r->next_seq = 1; /* 2^64 uses later */
        *seq = r->waiting[s] = r->next_seq++;
        r->cursor = (s + 1) % MPIX_DONE_SLOTS;
        r->in_use++;
        return (int)s;
    }
    return -1;
}

/* Has the kernel that was given (slot, seq) stored its word?  `word` is the
 * value just loaded (acquire) from the slot's host word. */
static inline bool done_seen(const DoneRing *r, int slot, uint64_t word)
{
    return r->waiting[slot] != 0 && word == r->waiting[slot];
}

/* false: the slot was not in use (nothing changed). */
static inline bool done_release(DoneRing *r, int slot)
{
    if (slot < 0 || slot >= MPIX_DONE_SLOTS || r->waiting[slot] == 0)
        return false;
    r->waiting[slot] = 0;
    r->in_use--;
    return true;
}

} /* namespace mpix */

#endif /* MPIX_TRANSPORT_DONE_RING_H */
