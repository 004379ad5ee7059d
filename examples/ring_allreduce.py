"""Ring allreduce built from the stream-triggered calls, self-checking.

Reduce-scatter with irecv_reduce_enqueue: what arrives from the left
neighbour is summed straight into the local chunk by the receiver's pull
kernel (no staging buffer, no add kernel behind the wait).  Allgather with the
plain calls.  Every step is ordered by the stream alone; the host never
waits between steps.  Works GPU-less too (numpy arrays, host waits).

    RANK=0 WORLD_SIZE=1 python ring_allreduce.py          # 1 process
    torchrun --nproc-per-node 2 ring_allreduce.py         # 2 ranks
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import mpix  # noqa: E402


def ring_allreduce(x, rank, size, stream=None, op="sum"):
    """x (1-d, contiguous, its length a multiple of `size`) becomes the
    elementwise `op` of every rank's x.  `stream`: the torch stream that
    orders the steps, or None for host buffers (host waits)."""
    if size == 1:
        return
    n = len(x) // size
    assert n * size == len(x), "the length must divide by the number of ranks"
    left, right = (rank - 1) % size, (rank + 1) % size

    def chunk(i):
        i %= size
        return x[i * n:(i + 1) * n]

    def step(recv, send, tag):
        reqs = [recv, mpix.isend_enqueue(send, dest=right, tag=tag,
                                         stream=stream)]
        if stream is None:
            mpix.waitall(reqs)
        else:
            mpix.waitall_enqueue(reqs, stream=stream)

    # reduce-scatter: after it, chunk rank + 1 holds the full result
    for s in range(size - 1):
        step(mpix.irecv_reduce_enqueue(chunk(rank - s - 1), source=left,
                                       op=op, tag=s, stream=stream),
             chunk(rank - s), s)
    # allgather: pass the finished chunks round
    for s in range(size - 1):
        step(mpix.irecv_enqueue(chunk(rank - s), source=left,
                                tag=size + s, stream=stream),
             chunk(rank + 1 - s), size + s)


def main():
    mpix.init()
    rank, size = mpix.world()
    n = (1 << 16) // size * size
    gpu = mpix.config()["have_gpu"]
    if gpu:
        import torch
        torch.cuda.set_device(rank % torch.cuda.device_count())
        # bf16 holds the integers up to 256: exact sums for up to 4 ranks
        dtype = torch.bfloat16 if size <= 4 else torch.float32
        x = (torch.arange(n, device="cuda") % 61 + rank).to(dtype)
        stream = torch.cuda.current_stream()
    else:
        import numpy as np
        x = (np.arange(n) % 61 + rank).astype(np.float32)
        stream = None

    ring_allreduce(x, rank, size, stream)
    if gpu:
        torch.cuda.synchronize()
        base = (torch.arange(n, device="cuda") % 61).float()
    else:
        base = (np.arange(n) % 61).astype(np.float32)
    want = base * size + sum(range(size))
    ok = bool((x == want).all()) if not gpu else bool((x.float() == want).all())
    print(f"rank {rank}: ring allreduce over {size} ranks "
          f"{'OK' if ok else 'WRONG'}")
    mpix.finalize()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
