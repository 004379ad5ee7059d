"""y-face halo exchange of a 3-d grid with no pack or unpack.

grid[:, 1, :] is nx runs of nz floats, ny * nz floats apart: a strided view.
isend_enqueue / irecv_enqueue take the views as they are; on the GPU one
kernel on the receiver walks both layouts and moves the face straight from
the sender's grid into the receiver's halo.  Works GPU-less too (numpy
arrays, host waits).

    RANK=0 WORLD_SIZE=1 python strided_yface.py          # 1 process (self)
    torchrun --nproc-per-node 2 strided_yface.py         # 2 ranks
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import mpix  # noqa: E402


def main():
    mpix.init()
    rank, size = mpix.world()
    peer = rank ^ 1 if size >= 2 else rank
    nx, ny, nz = 64, 48, 32
    gpu = mpix.config()["have_gpu"]
    if gpu:
        import torch
        torch.cuda.set_device(rank % torch.cuda.device_count())
        grid = torch.full((nx, ny, nz), float(rank), device="cuda")
        stream = torch.cuda.current_stream()
    else:
        import numpy as np
        grid = np.full((nx, ny, nz), float(rank), dtype=np.float32)
        stream = None

    # low interior face -> peer's high halo, high interior -> peer's low halo
    reqs = [mpix.irecv_enqueue(grid[:, ny - 1, :], source=peer, tag=0, stream=stream),
            mpix.irecv_enqueue(grid[:, 0, :], source=peer, tag=1, stream=stream),
            mpix.isend_enqueue(grid[:, 1, :], dest=peer, tag=0, stream=stream),
            mpix.isend_enqueue(grid[:, ny - 2, :], dest=peer, tag=1, stream=stream)]
    if gpu:
        mpix.waitall_enqueue(reqs, stream=stream)
        torch.cuda.synchronize()
    else:
        mpix.waitall(reqs)

    ok = bool((grid[:, 0, :] == peer).all() and (grid[:, ny - 1, :] == peer).all()
              and (grid[:, 1:ny - 1, :] == rank).all())
    print(f"rank {rank}: y-face halos {'OK' if ok else 'WRONG'}")
    mpix.finalize()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
