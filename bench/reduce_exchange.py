"""Time an exchange that ends with the sum in place, two ranks on one GPU:

  reduce   irecv_reduce_enqueue: the pull kernel combines into the buffer
  staged   irecv_enqueue into a staging buffer, then an add kernel
           (buf += staging) on the user's stream behind the wait

Both ranks send to and receive from the other in every step, all ordered by
one stream; the host synchronises once after `--steps` steps.  Each
(variant, dtype, size) runs in a fresh pair of processes, `--reps` times;
the line printed per configuration has the median step time and the range.

    python bench/reduce_exchange.py [--reps 5] [--json out.json]
"""
import argparse
import json
import multiprocessing as mp
import os
import socket
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"64KiB": 64 << 10, "64MiB": 64 << 20}
STEPS = {"64KiB": (200, 20), "64MiB": (20, 3)}  # (timed, warm-up)


def _rank(rank, port, variant, dtype_name, nbytes, steps, warmup, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, REPO)
    import torch
    import mpix
    dtype = getattr(torch, dtype_name)
    mpix.init()
    try:
        n = nbytes // torch.empty(0, dtype=dtype).element_size()
        other = 1 - rank
        buf = torch.zeros(n, dtype=dtype, device="cuda")
        msg = torch.ones(n, dtype=dtype, device="cuda")
        stage = torch.empty_like(buf)
        stream = torch.cuda.current_stream()

        def step(tag):
            if variant == "reduce":
                rr = mpix.irecv_reduce_enqueue(buf, source=other, tag=tag,
                                               stream=stream)
            else:
                rr = mpix.irecv_enqueue(stage, source=other, tag=tag,
                                        stream=stream)
            rs = mpix.isend_enqueue(msg, dest=other, tag=tag, stream=stream)
            mpix.waitall_enqueue([rs, rr], stream=stream)
            if variant != "reduce":
                buf.add_(stage)

        for i in range(warmup):
            step(i)
        torch.cuda.synchronize()
        buf.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(warmup + i)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        # ones summed `steps` <= 256 times: exact in f32 and in bf16
        ok = bool((buf.float() == float(steps)).all())
        q.put((rank, dt, ok))
    finally:
        mpix.finalize()


def run_pair(variant, dtype_name, size, rep):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    steps, warmup = STEPS[size]
    procs = [ctx.Process(target=_rank, args=(r, port, variant, dtype_name,
                                             SIZES[size], steps, warmup, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=30)
    assert all(ok for _, _, ok in out), (variant, dtype_name, size, out)
    return max(dt for _, dt, _ in out)  # the slower rank ends the step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for size in SIZES:
        for dtype_name in ("float32", "bfloat16"):
            for variant in ("reduce", "staged"):
                ts = [run_pair(variant, dtype_name, size, r) * 1e6
                      for r in range(args.reps)]
                row = {"size": size, "dtype": dtype_name, "variant": variant,
                       "median_us": round(statistics.median(ts), 1),
                       "min_us": round(min(ts), 1),
                       "max_us": round(max(ts), 1), "reps": args.reps}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
