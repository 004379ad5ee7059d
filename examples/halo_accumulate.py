"""Reverse halo exchange: ghost-layer contributions ADDED into the owner's
boundary faces, with no staging buffer and no unpack-add kernel.

Every rank holds a small 3-d grid whose layer 0 of each dimension is a ghost
layer that collected contributions for its neighbour (forces, deposited
charge, an adjoint stencil).  The x-, y- and z-ghost faces go out as the
views they are, and irecv_reduce_strided_enqueue adds what arrives into the
boundary faces (layer n-2 of each dimension): on the GPU one kernel on the
receiver walks both layouts and combines in registers.  The three boundary
faces share edges; the library runs their launches one after the other, and
the values are whole numbers, so the sum is exact in any order.  Works
GPU-less too (numpy arrays, host waits).  Exits non-zero when the result
differs from the same sums done on the CPU.

    RANK=0 WORLD_SIZE=1 python halo_accumulate.py        # 1 process (self)
    torchrun --nproc-per-node 2 halo_accumulate.py       # 2 ranks
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import mpix  # noqa: E402

SHAPE = (10, 12, 16)


def initial(rank):
    """The grid of `rank`: whole numbers that differ by rank and position."""
    n = int(np.prod(SHAPE))
    return ((np.arange(n) * (rank + 3)) % 97).astype(np.float32).reshape(SHAPE)


def face(grid, dim, index):
    """Layer `index` of dimension `dim`, without the ghost layers of the
    other two dimensions: a ghost face (index 0) and a boundary face then
    never share an element, so no send reads what a receive adds to."""
    cut = [slice(1, n - 1) for n in SHAPE]
    cut[dim] = index
    return grid[tuple(cut)]


def main():
    mpix.init()
    rank, size = mpix.world()
    peer = rank ^ 1 if size >= 2 else rank
    gpu = mpix.config()["have_gpu"]
    if gpu:
        import torch
        torch.cuda.set_device(rank % torch.cuda.device_count())
        grid = torch.from_numpy(initial(rank)).cuda()
        stream = torch.cuda.current_stream()
        torch.cuda.synchronize()
    else:
        grid = initial(rank)
        stream = None

    reqs = []
    for dim, n in enumerate(SHAPE):
        reqs.append(mpix.irecv_reduce_strided_enqueue(
            face(grid, dim, n - 2), source=peer, op="sum", tag=dim,
            stream=stream))
    for dim in range(3):
        reqs.append(mpix.isend_enqueue(face(grid, dim, 0), dest=peer, tag=dim,
                                       stream=stream))
    if gpu:
        mpix.waitall_enqueue(reqs, stream=stream)
        torch.cuda.synchronize()
        got = grid.cpu().numpy()
    else:
        mpix.waitall(reqs)
        got = grid

    want = initial(rank)
    theirs = initial(peer)
    for dim, n in enumerate(SHAPE):
        face(want, dim, n - 2)[...] += face(theirs, dim, 0)
    ok = got.tobytes() == want.tobytes()
    print(f"rank {rank}: ghost faces accumulated {'OK' if ok else 'WRONG'}")
    mpix.finalize()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
