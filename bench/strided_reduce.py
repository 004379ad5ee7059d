"""Time an exchange that ends with the sum in a strided view, two ranks on
one GPU:

  reduce   irecv_reduce_strided_enqueue: the pull kernel walks both layouts
           and combines into the view
  staged   irecv_enqueue of the same (strided) message into a contiguous
           staging buffer, then view.add_(staging) on the user's stream
           behind the wait

Both ranks send the same view of their own buffer to the other and receive
from it in every step, all ordered by one stream; the host synchronises once
after the timed steps.  Shapes:

  yface    grid(nx, 4, nz)[:, 1, :]: nx runs of 1 KiB, 4 KiB apart
  block    m(rows, 4 * cols)[:, :cols]: rows runs of 512 B, 2 KiB apart
  zface    grid(n, 4)[:, 1]: runs of ONE element, 4 elements apart (only
           with --shapes zface: the shape a strided pull serves correctly,
           not fast)

in float32 and bfloat16, with a 64 KiB message (latency-bound) and a 32 MiB
one (bandwidth-bound).  Each (shape, dtype, size, variant) runs in a fresh
pair of processes, `--reps` times, the two variants alternating; the line
printed per configuration has the median step time and the range.

    python bench/strided_reduce.py [--reps 5] [--shapes yface,block]
                                   [--json out.json]
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
SIZES = {"64KiB": 64 << 10, "32MiB": 32 << 20}
STEPS = {"64KiB": (200, 20), "32MiB": (20, 3)}  # (timed, warm-up)
RUN_BYTES = {"yface": 1024, "block": 512}


def make_view(torch, shape, dtype, nbytes):
    """(whole buffer, the view of it that holds `nbytes`)"""
    es = torch.empty(0, dtype=dtype).element_size()
    if shape == "zface":
        whole = torch.zeros(nbytes // es, 4, dtype=dtype, device="cuda")
        return whole, whole[:, 1]
    run = RUN_BYTES[shape] // es
    runs = nbytes // RUN_BYTES[shape]
    if shape == "yface":
        whole = torch.zeros(runs, 4, run, dtype=dtype, device="cuda")
        return whole, whole[:, 1, :]
    whole = torch.zeros(runs, 4 * run, dtype=dtype, device="cuda")
    return whole, whole[:, :run]


def _rank(rank, port, variant, shape, dtype_name, nbytes, steps, warmup, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, REPO)
    import torch
    import mpix
    dtype = getattr(torch, dtype_name)
    mpix.init()
    try:
        other = 1 - rank
        whole, view = make_view(torch, shape, dtype, nbytes)
        src_whole, src = make_view(torch, shape, dtype, nbytes)
        src.fill_(1)
        stage = torch.empty(view.shape, dtype=dtype, device="cuda")
        stream = torch.cuda.current_stream()

        def step(tag):
            if variant == "reduce":
                rr = mpix.irecv_reduce_strided_enqueue(view, source=other,
                                                       tag=tag, stream=stream)
            else:
                rr = mpix.irecv_enqueue(stage, source=other, tag=tag,
                                        stream=stream)
            rs = mpix.isend_enqueue(src, dest=other, tag=tag, stream=stream)
            mpix.waitall_enqueue([rs, rr], stream=stream)
            if variant != "reduce":
                view.add_(stage)

        for i in range(warmup):
            step(i)
        torch.cuda.synchronize()
        whole.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(warmup + i)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        # ones summed `steps` <= 256 times: exact in f32 and in bf16; what
        # lies between the runs stayed zero
        total = float(whole.sum(dtype=torch.float64))
        ok = bool((view.float() == float(steps)).all()) and \
            total == float(steps) * view.numel()
        q.put((rank, dt, ok))
    finally:
        mpix.finalize()


def run_pair(variant, shape, dtype_name, size):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    steps, warmup = STEPS[size]
    procs = [ctx.Process(target=_rank,
                         args=(r, port, variant, shape, dtype_name,
                               SIZES[size], steps, warmup, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=30)
    assert all(ok for _, _, ok in out), (variant, shape, dtype_name, size, out)
    return max(dt for _, dt, _ in out)  # the slower rank ends the step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="yface,block")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for size in SIZES:
        for shape in args.shapes.split(","):
            for dtype_name in ("float32", "bfloat16"):
                ts = {"reduce": [], "staged": []}
                for _ in range(args.reps):
                    for variant in ts:
                        ts[variant].append(
                            run_pair(variant, shape, dtype_name, size) * 1e6)
                for variant, t in ts.items():
                    row = {"size": size, "shape": shape, "dtype": dtype_name,
                           "variant": variant,
                           "median_us": round(statistics.median(t), 1),
                           "min_us": round(min(t), 1),
                           "max_us": round(max(t), 1), "reps": args.reps}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
