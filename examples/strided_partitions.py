"""A y-face of a 3-d grid sent as partitions, straight from the view.

grid[:, 1, :] is nx runs of nz floats, ny * nz floats apart.  psend_init /
precv_init split dimension 0 of the view: partition p is the slab
grid[p * rows:(p + 1) * rows, 1, :], rows = nx / partitions, and nothing is
packed.  On the GPU a kernel publishes the partitions with __device__
MPIX_Pready (here the helper that flags them all; a stencil kernel would
flag each slab as it finishes it), partitions made ready together travel as
one run, and one kernel entry on the receiver moves the run from the
sender's grid into the receiver's halo.  Works GPU-less too (numpy arrays,
host pready).

    RANK=0 WORLD_SIZE=1 python strided_partitions.py       # 1 process (self)
    torchrun --nproc-per-node 2 strided_partitions.py      # 2 ranks
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import mpix  # noqa: E402


def main():
    mpix.init()
    rank, size = mpix.world()
    peer = rank ^ 1 if size >= 2 else rank
    nx, ny, nz, parts = 64, 48, 32, 8
    gpu = mpix.config()["have_gpu"]
    if gpu:
        import torch
        torch.cuda.set_device(rank % torch.cuda.device_count())
        grid = torch.zeros((nx, ny, nz), device="cuda")
        stream = torch.cuda.current_stream()
    else:
        import numpy as np
        grid = np.zeros((nx, ny, nz), dtype=np.float32)

    # interior face 1 -> the peer's halo face ny - 1, as 8 slabs of 8 rows
    pr = mpix.precv_init(grid[:, ny - 1, :], parts, source=peer, tag=0)
    ps = mpix.psend_init(grid[:, 1, :], parts, dest=peer, tag=0)
    dps = mpix.prequest_create(ps) if gpu else None

    ok = True
    for it in range(3):  # the requests are persistent: reuse them
        grid[:, 1:ny - 1, :] = float(100 * it + rank)
        grid[:, ny - 1, :] = -1.0
        if gpu:
            torch.cuda.synchronize()
        mpix.start(pr)
        mpix.start(ps)
        if gpu:
            mpix.launch_pready_all(dps, parts, stream.cuda_stream)
        else:
            for p in range(parts):
                mpix.pready(p, ps)
        mpix.wait(pr)
        mpix.wait(ps)
        ok = ok and bool((grid[:, ny - 1, :] == 100 * it + peer).all()
                         and (grid[:, 1:ny - 1, :] == 100 * it + rank).all()
                         and (grid[:, 0, :] == 0).all())

    if dps is not None:
        mpix.prequest_free(dps)
    mpix.request_free(ps)
    mpix.request_free(pr)
    print(f"rank {rank}: y-face partitions {'OK' if ok else 'WRONG'}")
    mpix.finalize()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
