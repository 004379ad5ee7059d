"""How a pull batch's completion reaches the proxy (src/transport/native.cpp,
pull_kernels.h): MPIX_PULL_DONE=event (an event behind the launch), word (the
copy kernel stores its payload write-through and its last block stores a
sequence number to pinned host memory) and tail (a one-thread kernel behind
the copy stores the number).  Every case must deliver the same bytes under
every mode, and with MPIX_PULL_DONE unset, which is word.

Loopback, in the shape of tests/test_batch_handoffs_gpu.py, whose helpers
this file uses: position-dependent payloads between sentinel bytes that must
survive, cases in fresh child processes per mode (the MPIX_* switches are read
once per process) under a time limit, chained so that nothing is started after
a child that failed or timed out.  The children run with MPIX_STATS=1; the
counters printed at finalize say which path completed the batches.

The single messages are requests of one partition, so that the receive is
waited for on the host and the destination is then read by a consumer on a
second stream with no device-wide synchronise in front: what the wait
returned for must be visible to it.

Cases (the smallest shapes at which each branch of the kernels can go wrong):
  msg_16         one block, one vector: the slow branch alone
  msg_tile       exactly one tile of 16384 B: the fast branch alone
  msg_tile_16    one tile + 16 B: two blocks, one on each branch
  msg_1m21       1 MiB + 21 B, 65 tiles.  Default block cap: 65 blocks, the
                 last arriver is usually not block 0.  MPIX_PULL_BLOCKS=2
                 (the *_blocks2 children): two blocks take tickets, and the
                 one with the last tile runs the partial tile and the 5-byte
                 tail through the write-through slow branch
  kernel         8 kernel-triggered partitions of 4112 B, 5 iterations on
                 the same requests
  ring_wrap      40 messages one after another on one pair of requests: the
                 ring of 16 slots wraps, and the number a slot's earlier use
                 left in its word is never taken for the new one
  misaligned     a destination misaligned by 4 B: the hipMemcpyAsync pull,
                 completed by the tail kernel in tail and by event in word
  strided        one strided message: write-through stores and the word in
                 word, the tail kernel in tail
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_batch_handoffs_gpu as hb  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = hb.REPO
SENT, PAD, PARTS, ITERS, TILE = hb.SENT, hb.PAD, hb.PARTS, hb.ITERS, hb.TILE
CHILD_TIMEOUT = 180  # s; a child takes a few seconds
RING_MSGS = 40       # > 2 * MPIX_DONE_SLOTS

MODES = ["event", "word", "tail", "default"]
WORD_MODES = ["word", "tail", "default"]
CASES = ["msg_16", "msg_tile", "msg_tile_16", "msg_1m21", "kernel",
         "ring_wrap", "misaligned", "strided"]
CHILDREN = {}
for _m in MODES:
    _env = {} if _m == "default" else {"MPIX_PULL_DONE": _m}
    CHILDREN[_m] = (_env, CASES)
    if _m != "default":
        CHILDREN[_m + "_blocks2"] = (dict(_env, MPIX_PULL_BLOCKS="2"),
                                     ["msg_1m21"])
ENV_KEYS = hb.ENV_KEYS + ("MPIX_PULL_NT", "MPIX_PULL_UNROLL")


# ------------------------------------------------------------------ child

def case_single(mpix, torch, sizes, misalign=0, repeat=1):
    """Each entry of `sizes` as a request of one partition, `repeat`
    iterations on the same requests with a payload of their own each."""
    digest, statuses = hashlib.sha256(), []
    side = torch.cuda.Stream()
    for i, n in enumerate(sizes):
        src = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dst = torch.full((n + 2 * PAD + misalign,), SENT, dtype=torch.uint8,
                         device="cuda")
        at = PAD + misalign
        ps = mpix.psend_init((src.data_ptr(), n), 1, dest=0, tag=60 + i)
        pr = mpix.precv_init((dst.data_ptr() + at, n), 1, source=0,
                             tag=60 + i)
        try:
            for it in range(repeat):
                start = 17 * i + n + 1000 * it
                want = hb.pattern(torch, n, start)
                src.copy_(want)
                dst.fill_(SENT)
                torch.cuda.synchronize()
                mpix.start(pr)
                mpix.start(ps)
                mpix.pready(0, ps)
                st_r = mpix.wait(pr)
                with torch.cuda.stream(side):
                    seen = bool(torch.equal(dst[at:at + n], want))
                st_s = mpix.wait(ps)
                assert seen, f"payload seen from a second stream, {n} B #{it}"
                torch.cuda.synchronize()
                got = dst.cpu()
                assert torch.equal(got[at:at + n], want.cpu()), \
                    f"payload, {n} B #{it}"
                assert bool((got[:at] == SENT).all()), f"bytes before, {n} B"
                assert bool((got[at + n:] == SENT).all()), \
                    f"bytes after, {n} B"
                digest.update(got.numpy().tobytes())
                statuses.append([st_r, st_s])
        finally:
            mpix.request_free(ps)
            mpix.request_free(pr)
    return {"digest": digest.hexdigest(), "status": statuses}


def child_main(name):
    sys.path.insert(0, REPO)
    import torch
    import mpix

    run = {
        "msg_16": lambda: case_single(mpix, torch, [16]),
        "msg_tile": lambda: case_single(mpix, torch, [TILE]),
        "msg_tile_16": lambda: case_single(mpix, torch, [TILE + 16]),
        "msg_1m21": lambda: case_single(mpix, torch, [(1 << 20) + 21]),
        "kernel": lambda: hb.case_transfer(mpix, torch, None),
        "ring_wrap": lambda: case_single(mpix, torch, [4096],
                                         repeat=RING_MSGS),
        "misaligned": lambda: case_single(mpix, torch, [4096 + 20],
                                          misalign=4),
        "strided": lambda: hb.case_strided(mpix, torch),
    }
    for case in CHILDREN[name][1]:
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

_results = {}
_dead = []

_WORD = re.compile(r"MPIX_PULL_DONE=([\w-]+): completion word seen -> event "
                   r"seen, mean us over (\d+) batches")


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
                     f"lost completion word?); finished cases: {done}")
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


def _by_word(block):
    """(mode named in the counters, batches completed by their word)"""
    m = _WORD.search(block)
    return (m.group(1), int(m.group(2))) if m else (None, 0)


@pytest.mark.parametrize("case", CASES)
def test_same_bytes_under_every_mode(case):
    event = _child("event")[case]
    # payload, sentinels and the second-stream read were checked in the child
    assert _by_word(event["stderr"]) == (None, 0)
    for mode in WORD_MODES:
        res = _child(mode)[case]
        assert res["digest"] == event["digest"], mode
        assert res["status"] == event["status"], mode
        named, batches = _by_word(res["stderr"])
        print(f"{case}, {mode}: {batches} batches completed by word")
        if case == "misaligned" and mode != "tail":
            # a runtime copy stores no word: by event
            assert batches == 0, mode
            continue
        assert named == ("word" if mode == "default" else mode)
        if case == "ring_wrap":
            assert batches == RING_MSGS, mode
        elif case == "kernel":
            assert ITERS <= batches <= PARTS * ITERS, mode
        else:
            assert batches == 1, mode


@pytest.mark.parametrize("mode", ["word", "tail"])
def test_two_blocks_slow_branch_last(mode):
    res = _child(mode + "_blocks2")["msg_1m21"]
    event = _child("event_blocks2")["msg_1m21"]
    assert res["digest"] == event["digest"]
    assert res["digest"] == _child("event")["msg_1m21"]["digest"]
    assert _by_word(res["stderr"]) == (mode, 1)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child_main(sys.argv[sys.argv.index("--child") + 1])
