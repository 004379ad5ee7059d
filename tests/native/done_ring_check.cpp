/* Stand-alone check of src/transport/done_ring.h (host only, no HIP).
 * Built with -fsanitize=address,undefined and run as a program by
 * tests/test_done_ring.py.  Exit status 0 = every case passed.
 *
 * The "kernel" here is a plain store of the sequence number into an array of
 * host words; what is checked is the bookkeeping around it: filling up and
 * falling back, fresh numbers past 2^32, release in any order, and a "seen"
 * test that never takes the word of a slot's previous use for the new one. */
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "../../src/transport/done_ring.h"

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

struct Batch {
    int slot;
    uint64_t seq;
};

static void fill_and_fall_back()
{
    g_case = "fill up, fall back";
    DoneRing r;
    uint64_t words[MPIX_DONE_SLOTS] = {};
    std::vector<Batch> live;
    std::set<int> slots;
    std::set<uint64_t> seqs;
    for (int i = 0; i < MPIX_DONE_SLOTS; i++) {
        Batch b{-1, 0};
        b.slot = done_acquire(&r, &b.seq);
        CHECK(b.slot >= 0 && b.slot < MPIX_DONE_SLOTS);
        CHECK(b.seq != 0);
        CHECK(slots.insert(b.slot).second); /* no slot handed out twice */
        CHECK(seqs.insert(b.seq).second);
        CHECK(!done_seen(&r, b.slot, words[b.slot]));
        live.push_back(b);
    }
    CHECK(r.in_use == MPIX_DONE_SLOTS);
    /* full: -1, as often as asked, and nothing moves */
    for (int i = 0; i < 3; i++) {
        uint64_t seq = 77;
        const uint64_t next = r.next_seq;
        CHECK(done_acquire(&r, &seq) == -1);
        CHECK(seq == 77 && r.next_seq == next);
        CHECK(r.in_use == MPIX_DONE_SLOTS);
    }
    /* one finishes: exactly its slot comes back */
    words[live[5].slot] = live[5].seq;
    CHECK(done_seen(&r, live[5].slot, words[live[5].slot]));
    CHECK(done_release(&r, live[5].slot));
    Batch again{-1, 0};
    again.slot = done_acquire(&r, &again.seq);
    CHECK(again.slot == live[5].slot);
    CHECK(seqs.insert(again.seq).second);
    uint64_t seq = 0;
    CHECK(done_acquire(&r, &seq) == -1);
}

static void wrap_past_2_32()
{
    g_case = "sequence numbers past 2^32";
    DoneRing r;
    uint64_t words[MPIX_DONE_SLOTS] = {};
    r.next_seq = (1ull << 32) - 40; /* as after that many batches */
    uint64_t prev = 0;
    uint64_t last_of_slot[MPIX_DONE_SLOTS] = {};
    for (int i = 0; i < 100; i++) { /* one batch at a time, crossing 2^32 */
        uint64_t seq = 0;
        const int s = done_acquire(&r, &seq);
        CHECK(s >= 0);
        CHECK(seq > prev); /* strictly growing through the boundary */
        CHECK(seq != 0);
        /* a number that only differs above bit 31 from the slot's previous
         * one must not read as seen: the comparison is on 64 bits */
        CHECK(!done_seen(&r, s, words[s]));
        if (seq >> 32) CHECK(!done_seen(&r, s, (uint32_t)seq));
        CHECK(last_of_slot[s] == 0 || words[s] == last_of_slot[s]);
        words[s] = seq;
        CHECK(done_seen(&r, s, words[s]));
        CHECK(done_release(&r, s));
        last_of_slot[s] = seq;
        prev = seq;
    }
    CHECK(prev > (1ull << 32));
    /* the far end: 0 is never handed out */
    r.next_seq = UINT64_MAX;
    uint64_t a = 0, b = 0;
    const int sa = done_acquire(&r, &a);
    const int sb = done_acquire(&r, &b);
    CHECK(sa >= 0 && sb >= 0 && sa != sb);
    CHECK(a == UINT64_MAX && b == 1);
}

static void out_of_order_release()
{
    g_case = "release in any order";
    DoneRing r;
    uint64_t words[MPIX_DONE_SLOTS] = {};
    std::vector<Batch> live;
    for (int i = 0; i < 8; i++) {
        Batch b{-1, 0};
        b.slot = done_acquire(&r, &b.seq);
        live.push_back(b);
    }
    /* batches 6, 1, 4 finish, in that order */
    const int order[] = {6, 1, 4};
    for (int i : order) {
        words[live[i].slot] = live[i].seq;
        for (int j = 0; j < 8; j++) { /* the others are not seen */
            const bool fin = words[live[j].slot] == live[j].seq;
            if (r.waiting[live[j].slot] != 0)
                CHECK(done_seen(&r, live[j].slot, words[live[j].slot]) == fin);
        }
        CHECK(done_release(&r, live[i].slot));
        CHECK(!done_release(&r, live[i].slot)); /* twice: refused */
    }
    CHECK(r.in_use == 5);
    /* the freed slots, and only they or never-used ones, are handed out */
    std::set<int> busy;
    for (int j = 0; j < 8; j++)
        if (j != 6 && j != 1 && j != 4) busy.insert(live[j].slot);
    for (int i = 0; i < MPIX_DONE_SLOTS - 5; i++) {
        uint64_t seq = 0;
        const int s = done_acquire(&r, &seq);
        CHECK(s >= 0 && busy.count(s) == 0);
        busy.insert(s);
    }
    uint64_t seq = 0;
    CHECK(done_acquire(&r, &seq) == -1);
    CHECK(!done_release(&r, -1));
    CHECK(!done_release(&r, MPIX_DONE_SLOTS));
}

static void never_a_stale_word()
{
    g_case = "stale word";
    DoneRing r;
    uint64_t words[MPIX_DONE_SLOTS] = {};
    /* 40 batches one after the other go round the 16 slots: at every
     * acquire the slot's word still holds what its previous user stored */
    for (int i = 0; i < 40; i++) {
        uint64_t seq = 0;
        const int s = done_acquire(&r, &seq);
        CHECK(s >= 0);
        if (i >= MPIX_DONE_SLOTS) CHECK(words[s] != 0); /* really reused */
        CHECK(!done_seen(&r, s, words[s]));
        words[s] = seq;
        CHECK(done_seen(&r, s, words[s]));
        CHECK(done_release(&r, s));
        /* a released slot has no user: nothing is "seen" on it */
        CHECK(!done_seen(&r, s, words[s]));
    }
    /* a fresh ring over fresh words: 0 is not a sequence number */
    DoneRing f;
    uint64_t seq = 0;
    const int s = done_acquire(&f, &seq);
    CHECK(s >= 0 && !done_seen(&f, s, 0));
}

int main()
{
    fill_and_fall_back();
    wrap_past_2_32();
    out_of_order_release();
    never_a_stale_word();
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
