"""Host hand-offs around the batched pull (src/proxy.cpp, src/partitioned.cpp,
src/transport/native.cpp): slots of a persistent request armed once, ops of a
pass completed under one acquisition of the completion mutex, the proxy
walking again while a request's Pready flags are still landing (settle,
MPIX_SETTLE=0 turns it off), and a pull kernel's completion reaching the
proxy through a word in pinned host memory (MPIX_PULL_DONE=word) or through
an event (MPIX_PULL_DONE=event).

Loopback.  Payloads are position-dependent (byte i of a source is
((start + i) * 7 + 3) % 251, with a start of its own for every message and
iteration) and every destination sits between sentinel bytes that must
survive.  The partitioned cases run 5 iterations on the same requests.

The MPIX_* switches are read once per process, so the cases run in fresh
child processes (this file, started with --child NAME) under a time limit: a
lost wake-up or a lost completion word shows as a wait that never returns.
The file is chained: after a child that failed or timed out no further
process is started and the remaining tests fail at once.  The children run
with MPIX_STATS=1 and a fresh init/finalize per case; the counters printed
at finalize are what the tests read.
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5
PAD = 64
PARTS = 8
PER = 4112
ITERS = 5
FILLERS = 24  # loopback messages between the two pairs of the arm-once case
CHILD_TIMEOUT = 180  # s; a child takes a few seconds

TILE = 16384  # bytes one block of k_pull_multi moves per turn

PART_CASES = ["kernel", "host_descending", "host_descending_paced",
              "device_parrived"]
DONE_CASES = PART_CASES + ["msg_16", "msg_tile", "msg_tile_16", "slot_reuse",
                           "strided"]
# child name -> (environment on top of MPIX_STATS=1, cases it runs)
CHILDREN = {
    "event": ({"MPIX_PULL_DONE": "event"}, DONE_CASES),
    "word": ({"MPIX_PULL_DONE": "word"}, DONE_CASES),
    "nosettle": ({"MPIX_SETTLE": "0", "MPIX_PULL_DONE": "event"}, PART_CASES),
    # two blocks grid-stride over the 65 tiles of 1 MiB + 21 B; the block
    # that takes the last tile runs its tail branch last
    "event_blocks2": ({"MPIX_PULL_DONE": "event", "MPIX_PULL_BLOCKS": "2"},
                      ["msg_1m21"]),
    "word_blocks2": ({"MPIX_PULL_DONE": "word", "MPIX_PULL_BLOCKS": "2"},
                     ["msg_1m21"]),
    # a pool of 64 slots (the smallest): the second pair of requests gets the
    # slots of the first back; the trace says which slots each pair used
    "armonce": ({"MPIX_NFLAGS": "64", "MPIX_TRACE": "1"}, ["arm_once"]),
}
ENV_KEYS = ("MPIX_SETTLE", "MPIX_TRACE", "MPIX_NFLAGS", "MPIX_PULL_DONE",
            "MPIX_PULL_BLOCKS")


# ------------------------------------------------------------------ child

def pattern(torch, n, start, device="cuda"):
    i = torch.arange(start, start + n, dtype=torch.int64, device=device)
    return ((i * 7 + 3) % 251).to(torch.uint8)


class Pair:
    """A send and a receive request over PARTS partitions of PER bytes."""

    def __init__(self, mpix, torch, tag, kernel, side=False):
        self.mpix, self.torch = mpix, torch
        self.n = PARTS * PER
        self.src = torch.zeros(self.n, dtype=torch.uint8, device="cuda")
        self.dst = torch.full((self.n + 2 * PAD,), SENT, dtype=torch.uint8,
                              device="cuda")
        self.ps = mpix.psend_init((self.src.data_ptr(), self.n), PARTS,
                                  dest=0, tag=tag)
        self.pr = mpix.precv_init((self.dst.data_ptr() + PAD, self.n), PARTS,
                                  source=0, tag=tag)
        self.dps = mpix.prequest_create(self.ps) if kernel else None
        self.side = torch.cuda.Stream() if side else None

    def iteration(self, start, order, digest, paced=False):
        mpix, torch = self.mpix, self.torch
        stream = torch.cuda.current_stream()
        self.src.copy_(pattern(torch, self.n, start))
        self.dst.fill_(SENT)
        want = pattern(torch, self.n, start)
        torch.cuda.synchronize()
        mpix.start(self.pr)
        mpix.start(self.ps)
        if order is None:
            mpix.launch_pready_all(self.dps, PARTS, stream.cuda_stream)
        else:
            for p in order:
                mpix.pready(p, self.ps)
                # paced: the next partition is made ready only after this
                # one has arrived, so no walk ever sees two of them
                while paced and not mpix.parrived(self.pr, p):
                    pass
        st_r = mpix.wait(self.pr)
        # a consumer on ANOTHER stream, no device-wide synchronize before it:
        # what the wait returned for must be visible to it
        seen = True
        if self.side is not None:
            with torch.cuda.stream(self.side):
                seen = bool(torch.equal(self.dst[PAD:PAD + self.n], want))
        st_s = mpix.wait(self.ps)
        assert seen, f"payload seen from a second stream, start {start}"
        torch.cuda.synchronize()
        got = self.dst.cpu()
        assert torch.equal(got[PAD:PAD + self.n], want.cpu()), \
            f"payload, start {start}"
        assert bool((got[:PAD] == SENT).all()), f"bytes before, start {start}"
        assert bool((got[PAD + self.n:] == SENT).all()), \
            f"bytes after, start {start}"
        digest.update(got.numpy().tobytes())
        return [st_r, st_s]

    def free(self):
        if self.dps is not None:
            self.mpix.prequest_free(self.dps)
        self.mpix.request_free(self.ps)
        self.mpix.request_free(self.pr)


def case_transfer(mpix, torch, order, paced=False):
    digest, statuses = hashlib.sha256(), []
    pair = Pair(mpix, torch, tag=41, kernel=order is None, side=True)
    try:
        for it in range(ITERS):
            statuses.append(pair.iteration(1000 * it, order, digest, paced))
    finally:
        pair.free()
    return {"digest": digest.hexdigest(), "status": statuses}


def case_messages(mpix, torch, sizes, together=False):
    """One enqueued send/receive pair per entry of `sizes`, tags 0, 1, ...:
    each posted and waited for alone, or all posted before one waitall."""
    stream = torch.cuda.current_stream()
    srcs = [pattern(torch, n, 17 * i + n) for i, n in enumerate(sizes)]
    dsts = [torch.full((n + 2 * PAD,), SENT, dtype=torch.uint8, device="cuda")
            for n in sizes]
    torch.cuda.synchronize()
    pending = []
    for i, n in enumerate(sizes):
        pending.append(mpix.irecv_enqueue((dsts[i].data_ptr() + PAD, n),
                                          source=0, tag=i, stream=stream))
        pending.append(mpix.isend_enqueue((srcs[i].data_ptr(), n), dest=0,
                                          tag=i, stream=stream))
        if not together:
            mpix.waitall_enqueue(pending, stream=stream)
            torch.cuda.synchronize()
            pending = []
    if pending:
        mpix.waitall_enqueue(pending, stream=stream)
        torch.cuda.synchronize()
    digest = hashlib.sha256()
    for i, n in enumerate(sizes):
        got = dsts[i].cpu()
        assert torch.equal(got[PAD:PAD + n], srcs[i].cpu()), f"payload {i}"
        assert bool((got[:PAD] == SENT).all()), f"bytes before {i}"
        assert bool((got[PAD + n:] == SENT).all()), f"bytes after {i}"
        digest.update(got.numpy().tobytes())
    return digest


def case_slot_reuse(mpix, torch):
    """More batches than the ring has completion slots, one after the
    other, then 40 messages in flight at once."""
    one = case_messages(mpix, torch, [32768] * 40)
    many = case_messages(mpix, torch, [32768] * 40, together=True)
    return {"digest": one.hexdigest() + many.hexdigest(), "status": []}


def case_strided(mpix, torch):
    """A y-face-like view on both sides: 32 rows of 64 B, 128 B apart."""
    stream = torch.cuda.current_stream()
    src = pattern(torch, 32 * 128, 5).view(32, 128)
    dst = torch.full((32, 128), SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rr = mpix.irecv_enqueue(dst[:, 32:96], source=0, tag=7, stream=stream)
    rs = mpix.isend_enqueue(src[:, :64], dest=0, tag=7, stream=stream)
    mpix.waitall_enqueue([rs, rr], stream=stream)
    torch.cuda.synchronize()
    got = dst.cpu()
    assert torch.equal(got[:, 32:96], src[:, :64].cpu()), "payload"
    assert bool((got[:, :32] == SENT).all()), "bytes left of the rows"
    assert bool((got[:, 96:] == SENT).all()), "bytes right of the rows"
    return {"digest": hashlib.sha256(got.numpy().tobytes()).hexdigest(),
            "status": []}


def case_device_parrived(mpix, torch):
    """Producer and consumer both on the device: fill + Pready in one
    kernel, the consumer kernel waits with Parrived and checks the words."""
    per = PER // 4  # int32 words per partition
    send = torch.zeros(PARTS * per, dtype=torch.int32, device="cuda")
    recv = torch.zeros_like(send)
    errs = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    ps = mpix.psend_init(send, PARTS, dest=0, tag=43)
    pr = mpix.precv_init(recv, PARTS, source=0, tag=43)
    dps, dpr = mpix.prequest_create(ps), mpix.prequest_create(pr)
    digest = hashlib.sha256()
    try:
        for it in range(ITERS):
            base = 777 + 100000 * it
            recv.zero_()
            torch.cuda.synchronize()
            mpix.start(pr)
            mpix.start(ps)
            mpix.launch_fill_and_pready(send.data_ptr(), per, base, dps,
                                        PARTS, stream.cuda_stream)
            mpix.launch_wait_and_check(recv.data_ptr(), per, base, dpr,
                                       PARTS, errs.data_ptr(),
                                       stream.cuda_stream)
            torch.cuda.synchronize()
            mpix.wait(pr)
            mpix.wait(ps)
            assert errs.item() == 0, f"device-side check, iteration {it}"
            assert torch.equal(send, recv), f"payload, iteration {it}"
            digest.update(recv.cpu().numpy().tobytes())
    finally:
        mpix.prequest_free(dps)
        mpix.prequest_free(dpr)
        mpix.request_free(ps)
        mpix.request_free(pr)
    return {"digest": digest.hexdigest(), "status": []}


def case_arm_once(mpix, torch):
    """Five iterations on one pair, free it, then a new pair on the same
    slots: its first Start has to arm again, or its flags are never seen."""
    digest, statuses = hashlib.sha256(), []
    stream = torch.cuda.current_stream()
    first = Pair(mpix, torch, tag=41, kernel=True)
    try:
        for it in range(ITERS):
            statuses.append(first.iteration(1000 * it, None, digest))
    finally:
        first.free()
    # 2 slots per message, taken at the allocation cursor: after the 16 of
    # the first pair and these 48 the cursor is back at slot 0 of the 64.
    # Each one is waited for, and a message takes several proxy passes, so
    # the slots the first pair gave back are free long before the last.
    word = torch.zeros(4, dtype=torch.int32, device="cuda")
    for i in range(FILLERS):
        rs = mpix.isend_enqueue(word, dest=0, tag=100 + i, stream=stream)
        rr = mpix.irecv_enqueue(word, source=0, tag=100 + i, stream=stream)
        mpix.waitall_enqueue([rs, rr], stream=stream)
        torch.cuda.synchronize()
    second = Pair(mpix, torch, tag=42, kernel=True)
    try:
        for it in range(2):
            statuses.append(second.iteration(500 + 1000 * it, None, digest))
    finally:
        second.free()
    return {"digest": digest.hexdigest(), "status": statuses}


def child_main(name):
    sys.path.insert(0, REPO)
    import torch
    import mpix

    run = {
        "kernel": lambda: case_transfer(mpix, torch, None),
        "host_descending": lambda: case_transfer(
            mpix, torch, list(range(PARTS - 1, -1, -1))),
        "host_descending_paced": lambda: case_transfer(
            mpix, torch, list(range(PARTS - 1, -1, -1)), paced=True),
        "device_parrived": lambda: case_device_parrived(mpix, torch),
        "arm_once": lambda: case_arm_once(mpix, torch),
        "slot_reuse": lambda: case_slot_reuse(mpix, torch),
        "strided": lambda: case_strided(mpix, torch),
    }
    for case, n in (("msg_16", 16), ("msg_tile", TILE),
                    ("msg_tile_16", TILE + 16), ("msg_1m21", (1 << 20) + 21)):
        run[case] = lambda n=n: {
            "digest": case_messages(mpix, torch, [n]).hexdigest(),
            "status": []}
    for case in CHILDREN[name][1]:
        # the library's counters go to stderr at finalize: mark whose they are
        sys.stderr.write(f"CASE-BEGIN {case}\n")
        sys.stderr.flush()
        mpix.init()
        try:
            res = run[case]()
        finally:
            mpix.finalize()
        print("CASE " + json.dumps({"name": case, **res}, default=str),
              flush=True)
    print("CHILD-DONE", flush=True)


# ----------------------------------------------------------------- parent

_results = {}  # child -> {case: {"digest", "status", "stderr"}}
_dead = []     # why no further process may be started

_NOTIFY = re.compile(r"device notifies: (\d+) descriptors for (\d+) "
                     r"messages sent")
_ARMS = re.compile(r"arm pushes (\d+);")
_GROUPS = re.compile(r"completion groups: (\d+) for (\d+) ops")
_ISSUED = re.compile(r"ops issued=(\d+) completed=(\d+)")
_TRACE_PART = re.compile(r"slot (\d+) part peer=\d+ tag=(\d+) ")


def _child(name):
    if name in _results:
        return _results[name]
    if _dead:
        pytest.fail("not started: " + _dead[0])
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", MPIX_STATS="1")
    for k in ENV_KEYS:
        env.pop(k, None)
    env.update(CHILDREN[name][0])
    try:
        run = subprocess.run([sys.executable, os.path.abspath(__file__),
                              "--child", name], env=env, capture_output=True,
                             text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout
        done = re.findall(r'^CASE {"name": "(\w+)"', out or "", re.M)
        _dead.append(f"child {name} timed out after {CHILD_TIMEOUT} s (a "
                     f"lost wake-up?); finished cases: {done}")
        pytest.fail(_dead[0])
    if run.returncode != 0 or "CHILD-DONE" not in run.stdout:
        _dead.append(f"child {name} failed (exit {run.returncode}):\n"
                     f"{run.stdout[-2000:]}\n{run.stderr[-4000:]}")
        pytest.fail(_dead[0])
    res = {}
    for line in run.stdout.splitlines():
        if line.startswith("CASE "):
            r = json.loads(line[5:])
            res[r["name"]] = r
    for block in run.stderr.split("CASE-BEGIN ")[1:]:
        res[block.split("\n", 1)[0].strip()]["stderr"] = block
    _results[name] = res
    return res


def _counter(regex, block, what):
    m = regex.search(block)
    assert m is not None, f"no {what} in the counters:\n{block[-3000:]}"
    return [int(g) for g in m.groups()]


_WORD = re.compile(r"MPIX_PULL_DONE=word: completion word seen -> event "
                   r"seen, mean us over (\d+) batches")


@pytest.mark.parametrize("case", DONE_CASES)
def test_same_bytes_by_word_and_by_event(case):
    word, event = _child("word")[case], _child("event")[case]
    # payload and sentinels were checked in the children
    assert word["digest"] == event["digest"]
    assert word["status"] == event["status"]
    # the word path really ran (and only where it was asked for): the
    # batches whose word was seen are counted at finalize
    assert _WORD.search(event["stderr"]) is None
    (batches,) = _counter(_WORD, word["stderr"], "completion word line")
    print(f"{case}: {batches} batches completed by word")
    assert batches >= 1
    if case == "slot_reuse":
        assert batches > 40  # 40 alone + at least one for the 40 together


def test_two_blocks_tail_last():
    word = _child("word_blocks2")["msg_1m21"]
    event = _child("event_blocks2")["msg_1m21"]
    assert word["digest"] == event["digest"]
    (batches,) = _counter(_WORD, word["stderr"], "completion word line")
    assert batches == 1


@pytest.mark.parametrize("case", PART_CASES)
def test_same_bytes_with_and_without_settle(case):
    on, off = _child("event")[case], _child("nosettle")[case]
    assert on["digest"] == off["digest"]
    assert on["status"] == off["status"]


def test_kernel_trigger_is_one_run_per_iteration():
    """One wave stores the 8 flags; with settle the request goes out as ONE
    descriptor in at least 4 of the 5 iterations.  Every iteration needs at
    least one descriptor, so a total of at most 6 means that at most one
    iteration was split, and that one in two (a little stricter than "4 of
    5", which would also allow one iteration in three or more)."""
    for child in ("event", "word"):
        block = _child(child)["kernel"]["stderr"]
        descs, msgs = _counter(_NOTIFY, block, "notify line")
        print(f"settle on, {child}: {descs} descriptors for {msgs} "
              f"partitions")
        assert msgs == PARTS * ITERS
        assert ITERS <= descs <= ITERS + 1
    off = _child("nosettle")["kernel"]["stderr"]
    d_off, m_off = _counter(_NOTIFY, off, "notify line")
    print(f"settle off: {d_off} descriptors for {m_off} partitions")
    assert m_off == PARTS * ITERS and ITERS <= d_off <= PARTS * ITERS


@pytest.mark.parametrize("child", ["event", "word", "nosettle"])
def test_host_descending_stays_runs_of_one(child):
    """Partitions made ready 7, 6, ... 0 by the host, each only after the
    one before has arrived: 8 runs of one per iteration, with and without
    settle — a partition published on its own is announced at once, never
    held back for a later one.

    Without the pacing the count is a matter of timing, before this change
    as after it: the walk visits the slots in partition order whatever the
    order of the Pready calls, so flags that are all up when a walk comes by
    leave as ONE ascending run (measured: 5 descriptors for the 40
    partitions of 5 iterations, the same with MPIX_SETTLE=0).  For that case
    only the bounds hold, as in tests/test_part_runs_gpu.py."""
    res = _child(child)
    descs, msgs = _counter(_NOTIFY, res["host_descending_paced"]["stderr"],
                           "notify line")
    assert (descs, msgs) == (PARTS * ITERS, PARTS * ITERS)
    descs, msgs = _counter(_NOTIFY, res["host_descending"]["stderr"],
                           "notify line")
    print(f"{child}, not paced: {descs} descriptors for {msgs} partitions")
    assert msgs == PARTS * ITERS and ITERS <= descs <= PARTS * ITERS


def test_completions_are_grouped():
    """Every op is completed exactly once, and under fewer acquisitions of
    the completion mutex than there are ops: the 16 ops of an iteration
    become done in one progress() call."""
    block = _child("event")["kernel"]["stderr"]
    issued, completed = _counter(_ISSUED, block, "ops line")
    groups, ops = _counter(_GROUPS, block, "completion groups line")
    print(f"{groups} groups for {ops} ops")
    assert issued == completed == ops == 2 * PARTS * ITERS
    assert groups < ops


def test_arm_once_and_again_after_free():
    res = _child("armonce")["arm_once"]
    block = res["stderr"]
    slots = {41: set(), 42: set()}
    for slot, tag in _TRACE_PART.findall(block):
        if int(tag) in slots:
            slots[int(tag)].add(int(slot))
    print(f"slots of the first pair {sorted(slots[41])}, of the second "
          f"{sorted(slots[42])}")
    assert len(slots[41]) == 2 * PARTS
    # the scenario is the one meant: the new requests sit on the old slots
    assert slots[42] == slots[41]
    (arms,) = _counter(_ARMS, block, "arm pushes")
    # 16 per pair of requests, whatever the number of iterations (5 and 2),
    # and 2 per loopback message in between
    assert arms == 2 * (2 * PARTS) + 2 * FILLERS


if __name__ == "__main__":
    if "--child" in sys.argv:
        child_main(sys.argv[sys.argv.index("--child") + 1])
