/* Stand-alone check of src/transport/shm_ring.h (host only, no HIP).
 * Built twice by tests/test_shm_ring.py, with -fsanitize=address,undefined
 * and with -fsanitize=thread, and run as a program.  Exit status 0 = every
 * case passed.
 *
 * The "segment" is a 64-byte-aligned heap block, zeroed as the transport
 * zeroes its mapping, with ring_slots = 4 and stage_chunks = 2 for 2 ranks.
 * What is checked is the geometry, the space and credit arithmetic across
 * wrap-arounds, and, with a producer and a consumer thread, the memory
 * orders: the consumer must never read a descriptor before it is whole, and
 * the producer must never overwrite one that is still being read. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>

#include "../../src/transport/shm_ring.h"

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

static const int NRANKS = 2;
static const uint32_t SLOTS = 4, CHUNKS = 2;

struct Segment {
    ShmGeom g;
    void *base;
    Segment() : g(shm_geometry(NRANKS, SLOTS, CHUNKS)) {
        base = aligned_alloc(64, g.segment_bytes);
        if (base == nullptr) abort();
        memset(base, 0, g.segment_bytes);
    }
    ~Segment() { free(base); }
};

/* descriptor number `seq`: the number in token, a pattern derived from it in
 * every byte of ipc and every field of layout */
static Desc make_desc(uint64_t seq)
{
    Desc d;
    d.type = DESC_DEV_NOTIFY;
    d.token = seq;
    for (size_t i = 0; i < sizeof(d.ipc); i++)
        d.ipc[i] = (uint8_t)(seq * 31 + i * 7 + 1);
    d.layout.run_bytes = seq ^ 0x5a5a5a5a5a5a5a5aull;
    d.layout.count[0] = seq + 1;
    d.layout.count[1] = seq * 3 + 2;
    d.layout.stride[0] = (int64_t)(seq * 5 + 3);
    d.layout.stride[1] = -(int64_t)(seq + 4);
    return d;
}

static bool desc_intact(const Desc &d, uint64_t seq)
{
    const Desc w = make_desc(seq);
    return d.type == w.type && d.token == seq &&
           memcmp(d.ipc, w.ipc, sizeof(d.ipc)) == 0 &&
           d.layout.run_bytes == w.layout.run_bytes &&
           d.layout.count[0] == w.layout.count[0] &&
           d.layout.count[1] == w.layout.count[1] &&
           d.layout.stride[0] == w.layout.stride[0] &&
           d.layout.stride[1] == w.layout.stride[1];
}

static void geometry()
{
    g_case = "geometry";
    Segment s;
    CHECK(sizeof(Desc) == 192);
    CHECK(s.g.ring_slots == SLOTS && s.g.stage_chunks == CHUNKS);
    CHECK(s.g.inbox_bytes % 64 == 0);
    CHECK(s.g.segment_bytes == s.g.inbox_bytes * NRANKS);
    const InboxView a = inbox_view(s.base, s.g, 0);
    const InboxView b = inbox_view(s.base, s.g, 1);
    CHECK((char *)a.hdr == (char *)s.base);
    /* header, ring and stage of inbox 0 follow each other and end before
     * inbox 1 begins, which ends inside the segment */
    CHECK((char *)a.ring == (char *)a.hdr + sizeof(InboxHdr));
    CHECK(a.stage == (char *)(a.ring + SLOTS));
    CHECK(a.stage + (size_t)CHUNKS * CHUNK_BYTES <= (char *)b.hdr);
    CHECK(b.stage + (size_t)CHUNKS * CHUNK_BYTES <=
          (char *)s.base + s.g.segment_bytes);
    CHECK((uintptr_t)b.hdr % 64 == 0 && (uintptr_t)b.ring % 64 == 0);
}

static void space()
{
    g_case = "space";
    Segment s;
    const InboxView v = inbox_view(s.base, s.g, 1);
    uint64_t head = 0, tail = 0;
    CHECK(ring_has_space(v, s.g, head, 4));
    CHECK(!ring_has_space(v, s.g, head, 5));
    for (uint64_t i = 0; i < 4; i++) {
        CHECK(ring_has_space(v, s.g, head, 1));
        ring_emit(v, s.g, &head, make_desc(i));
    }
    CHECK(head == 4 && ring_head(v) == 4);
    CHECK(!ring_has_space(v, s.g, head, 1));
    CHECK(desc_intact(ring_front(v, s.g, tail), 0));
    ring_pop(v, &tail);
    CHECK(tail == 1);
    CHECK(ring_has_space(v, s.g, head, 1));
    CHECK(!ring_has_space(v, s.g, head, 2));
    /* the other inbox of the segment saw none of it */
    const InboxView o = inbox_view(s.base, s.g, 0);
    CHECK(ring_head(o) == 0 && ring_has_space(o, s.g, 0, 4));
}

static void wrap_around()
{
    g_case = "3 wrap-arounds";
    Segment s;
    const InboxView v = inbox_view(s.base, s.g, 0);
    uint64_t head = 0, tail = 0, sent = 0, got = 0;
    /* uneven bursts, so that the ring is full, empty and in between */
    const uint64_t burst[] = {4, 1, 3, 2, 4, 4, 1, 1};
    const uint64_t total = 3 * SLOTS + 3;
    for (size_t b = 0; sent < total; b++) {
        uint64_t n = burst[b % 8];
        for (uint64_t i = 0; i < n && sent < total; i++) {
            if (!ring_has_space(v, s.g, head, 1)) break;
            const uint64_t before = head;
            ring_emit(v, s.g, &head, make_desc(sent++));
            CHECK(head == before + 1 && ring_head(v) == head);
        }
        CHECK(head - tail <= SLOTS);
        /* drain all but one on even bursts, all on odd ones */
        const uint64_t upto = ring_head(v) - (b % 2 == 0 ? 1 : 0);
        while (tail < upto) {
            CHECK(desc_intact(ring_front(v, s.g, tail), got));
            got++;
            const uint64_t before = tail;
            ring_pop(v, &tail);
            CHECK(tail == before + 1);
            CHECK(v.hdr->tail.load(std::memory_order_relaxed) == tail);
        }
    }
    while (tail < ring_head(v)) {
        CHECK(desc_intact(ring_front(v, s.g, tail), got));
        got++;
        ring_pop(v, &tail);
    }
    CHECK(sent == total && got == total && head == total && tail == total);
    CHECK(head / SLOTS >= 3);
}

static void stage_credits()
{
    g_case = "stage credits";
    Segment s;
    const InboxView v = inbox_view(s.base, s.g, 1);
    uint64_t stage_head = 0;
    CHECK(stage_free_chunks(v, s.g, stage_head) == 2);
    stage_head += 2; /* 2 taken */
    CHECK(stage_free_chunks(v, s.g, stage_head) == 0);
    stage_release(v);
    CHECK(stage_free_chunks(v, s.g, stage_head) == 1);
    stage_release(v);
    /* across the wrap: chunk index is cursor % stage_chunks, the payload
     * written there is what the consumer finds at the descriptor's index */
    uint64_t head = 0, tail = 0;
    for (uint64_t i = 0; i < 7; i++) {
        CHECK(stage_free_chunks(v, s.g, stage_head) == 2 - i % 2);
        const uint64_t idx = stage_head % s.g.stage_chunks;
        CHECK(idx == (2 + i) % 2);
        memset(v.stage + idx * CHUNK_BYTES, (int)(0x40 + i), CHUNK_BYTES);
        Desc d = make_desc(i);
        d.type = DESC_HOST_CHUNK;
        d.stage_chunk = idx;
        stage_head++;
        ring_emit(v, s.g, &head, d);
        if (i % 2 == 1) { /* the consumer takes two at a time */
            for (uint64_t j = i - 1; j <= i; j++) {
                const Desc &r = ring_front(v, s.g, tail);
                CHECK(r.token == j && r.stage_chunk == (2 + j) % 2);
                const char *p = v.stage + r.stage_chunk * CHUNK_BYTES;
                CHECK(p[0] == (char)(0x40 + j) &&
                      p[CHUNK_BYTES - 1] == (char)(0x40 + j));
                stage_release(v);
                ring_pop(v, &tail);
            }
        }
    }
    CHECK(stage_free_chunks(v, s.g, stage_head) == 1);
}

static void two_threads()
{
    g_case = "producer and consumer threads";
    Segment s;
    const uint64_t N = 20000;
    uint64_t bad = 0, seen = 0;
    std::thread producer([&s] {
        const InboxView v = inbox_view(s.base, s.g, 1);
        uint64_t head = 0;
        while (head < N) {
            if (!ring_has_space(v, s.g, head, 1)) {
                std::this_thread::yield();
                continue;
            }
            ring_emit(v, s.g, &head, make_desc(head));
        }
    });
    std::thread consumer([&s, &bad, &seen] {
        const InboxView v = inbox_view(s.base, s.g, 1);
        uint64_t tail = 0;
        while (tail < N) {
            const uint64_t head = ring_head(v);
            if (tail == head) {
                std::this_thread::yield();
                continue;
            }
            if (head - tail > SLOTS) bad++;
            while (tail < head) {
                if (!desc_intact(ring_front(v, s.g, tail), tail)) bad++;
                ring_pop(v, &tail);
                seen++;
            }
        }
    });
    producer.join();
    consumer.join();
    CHECK(seen == N);
    CHECK(bad == 0);
}

int main()
{
    geometry();
    space();
    wrap_around();
    stage_credits();
    two_threads();
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
