#!/usr/bin/env python3
"""mpix flagship benchmark — BASELINE.json metrics on MI355X.

Measures, on N ranks (one per GPU, torchrun layout):
  1. (only with --full) stream-enqueued ping-pong half-RTT (us) —
     MPIX_Isend/Irecv_enqueue + MPIX_Wait_enqueue on hipStream memOps,
     device buffers, rank pairs (0<->1, 2<->3, ...); loopback-self at N=1.
     A plain run reports `pingpong_half_rtt_us: null`.
  2. Psend bandwidth (GB/s) — HEADLINE `value`: partitioned ring exchange,
     device buffers, __device__ MPIX_Pready trigger kernel, 64 partitions.
     `value` is the whole-job aggregate over all N ranks (weak scaling:
     per-rank message size is fixed as N grows).

A plain run does only what the headline needs: set up, warm up, time the K
steps, print the result line.  --dump-outputs DIR additionally writes each
rank's receive buffer after the last timed step as DIR/recv.npy (rank 0) /
DIR/recv_rank<r>.npy, float64, a fixed sample when the buffer is large; the
payload is seeded per rank, so two builds can be compared output for output.

Before mpix starts its proxy thread each rank confines its host threads to
the CPUs of one last-level cache on its GPU's NUMA node (pin_to_one_cache;
--no-pin turns it off).  Left to the scheduler the two threads often sit on
different sockets and ms_per_step differs from one process to the next
(46 % spread against 4 % pinned: profiles/bench_thread_placement.md), which
makes runs impossible to compare.

Run:  python bench.py [--gpus N] [--steps K] [--warmup W] [--full]
                      [--dump-outputs DIR] [--no-pin]
The driver launches N>1 via `python -m torch.distributed.run --nnodes=1
--nproc-per-node N ... bench.py --gpus N`; we read RANK/LOCAL_RANK/
WORLD_SIZE/MASTER_* from the environment (mpix's TCP bootstrap uses
MASTER_PORT+31, next to torchrun's c10d store).

Timing discipline (driver contract): W untimed warmup steps, then EXACTLY K
timed steps bracketed by barrier + torch.cuda.synchronize() on both sides;
elapsed is max-reduced over ranks; rank 0 prints ONE JSON line.

Reference (NVIDIA/mpi-acx) publishes no numbers — vs_baseline
is null; these are the self-measured targets BASELINE.json defines.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--msg-mib", type=int, default=256,
                   help="per-rank Psend message size (MiB)")
    p.add_argument("--partitions", type=int, default=64)
    p.add_argument("--pp-iters", type=int, default=200,
                   help="ping-pong iterations per timed block")
    p.add_argument("--pp-bytes", type=int, default=8,
                   help="ping-pong message size (bytes)")
    p.add_argument("--full", action="store_true",
                   help="also run the side measurements (stream-enqueued "
                        "ping-pong half-RTT) before the headline")
    p.add_argument("--no-pin", action="store_true",
                   help="leave thread placement to the scheduler (default: "
                        "keep the host threads on one last-level cache "
                        "next to the GPU, see pin_to_one_cache)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last step "
                        "delivered as DIR/<name>.npy (float64)")
    return p.parse_args()


def _cpulist(text):
    cpus = set()
    for part in text.strip().split(","):
        if part:
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def _read(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return None


def choose_cpus(pci_addr, local_rank, allowed, sysfs="/sys"):
    """The CPUs of ONE last-level cache for rank `local_rank`: among the
    allowed CPUs of the NUMA node of the GPU at `pci_addr` (all allowed CPUs
    if there is no GPU or the host does not say), list the distinct L3
    sharing groups in CPU order and take group local_rank mod count, so
    ranks never pile onto one cache.  None if the host describes no L3."""
    pool = allowed
    if pci_addr is not None:
        node = _read(f"{sysfs}/bus/pci/devices/{pci_addr}/numa_node")
        if node is not None and int(node) >= 0:
            text = _read(f"{sysfs}/devices/system/node/node{int(node)}"
                         "/cpulist")
            if text and _cpulist(text) & allowed:
                pool = _cpulist(text) & allowed
    groups = {}
    for c in sorted(pool):
        text = _read(f"{sysfs}/devices/system/cpu/cpu{c}/cache/index3/"
                     "shared_cpu_list")
        if text:
            groups.setdefault(text, _cpulist(text) & allowed)
    groups = [g for g in groups.values() if len(g) >= 2]
    return groups[local_rank % len(groups)] if groups else None


def pin_to_one_cache(pci_addr, local_rank):
    """Restrict the calling thread — and every thread it starts later, so
    the mpix proxy thread created by mpix.init() — to choose_cpus().  A Psend
    step is a chain of handoffs between the main thread, the proxy thread
    and the GPU; left to the scheduler on a two-socket host the two threads
    often sit on different sockets, and ms_per_step then takes a different
    value in each process, which no number of steps averages out
    (profiles/bench_thread_placement.md has the measurements).  Returns the
    CPU set, or None (mask untouched) if the host describes no L3."""
    cpus = choose_cpus(pci_addr, local_rank, os.sched_getaffinity(0))
    if cpus:
        os.sched_setaffinity(0, cpus)
    return cpus


PAYLOAD_SEED = 0  # rank r fills its send buffer from seed PAYLOAD_SEED + r
DUMP_BUDGET_BYTES = 48 << 20  # all ranks together stay well under 64 MB


def dump_outputs(dirpath, name, out, parts, world):
    """Write int32 tensor `out` to dirpath/name.npy as float64 (exact for
    int32).  A buffer over this rank's share of the budget is sampled at a
    fixed set of indices: the first and last word of every partition plus
    seeded uniform draws, sorted — a function of the shape alone, so two
    runs with the same arguments sample the same words."""
    import numpy as np
    import torch

    n = out.numel()
    limit = DUMP_BUDGET_BYTES // 8 // world
    if n > limit:
        per = n // parts
        edges = np.arange(parts, dtype=np.int64) * per
        draws = np.random.default_rng(0).integers(
            0, n, size=max(limit - 2 * parts, 0), dtype=np.int64)
        idx = np.unique(np.concatenate([edges, edges + per - 1, draws]))
        out = out[torch.from_numpy(idx).to(out.device)]
    os.makedirs(dirpath, exist_ok=True)
    np.save(os.path.join(dirpath, name + ".npy"),
            out.to(torch.float64).cpu().numpy())


def main():
    args = parse_args()
    import torch
    import mpix

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", str(args.gpus)))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    os.environ.setdefault("RANK", str(rank))
    os.environ.setdefault("WORLD_SIZE", str(world))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")

    use_gpu = torch.cuda.is_available()
    if mpix.have_gpu() and not use_gpu:
        # never run a silently degraded CPU bench on a GPU box
        raise RuntimeError("mpix sees a GPU but torch.cuda does not — "
                           "HIP runtime clash (import order?)")
    if use_gpu:
        torch.cuda.set_device(local_rank % torch.cuda.device_count())
        dev = "cuda"
    else:
        dev = "cpu"  # CPU sanity mode: host buffers through the same paths

    dist = None
    if world > 1:
        import torch.distributed as tdist
        tdist.init_process_group("gloo", rank=rank, world_size=world)
        dist = tdist

    def barrier_sync():
        if dist is not None:
            dist.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    def max_over_ranks(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def trace(msg):
        print(f"[bench r{rank}] {msg}", file=sys.stderr, flush=True)

    # before mpix.init(): the proxy thread inherits the mask
    pinned = None
    if not args.no_pin:
        pci_addr = None
        if use_gpu:
            gpu = torch.cuda.get_device_properties(
                torch.cuda.current_device())
            pci_addr = "%04x:%02x:%02x.0" % (
                gpu.pci_domain_id, gpu.pci_bus_id, gpu.pci_device_id)
        pinned = pin_to_one_cache(pci_addr, local_rank)
    trace(f"host threads pinned to CPUs {sorted(pinned)}" if pinned
          else "host threads not pinned")

    mpix.init()
    trace(f"init done: {mpix.config()}")
    stream = torch.cuda.current_stream() if use_gpu else None

    # ------------------------------------------------ 1. ping-pong half-RTT
    # side measurement, not part of the headline: only with --full
    half_rtt_us = None
    pingpong_role = "self"
    if args.full:
        n_pp = max(args.pp_bytes // 4, 1)
        buf = torch.zeros(n_pp, dtype=torch.int32, device=dev)
        if world == 1:
            peer, pingpong_role = 0, "self"
        else:
            pair = rank ^ 1
            # odd world: last rank loops back
            peer = pair if pair < world else rank
            pingpong_role = "ping" if rank % 2 == 0 else "pong"
            if peer == rank:
                pingpong_role = "self"

        def pp_iter():
            if pingpong_role == "self":
                rs = mpix.isend_enqueue(buf, dest=rank, tag=1, stream=stream)
                rr = mpix.irecv_enqueue(buf, source=rank, tag=1, stream=stream)
                mpix.waitall_enqueue([rs, rr], stream=stream)
            elif pingpong_role == "ping":
                rs = mpix.isend_enqueue(buf, dest=peer, tag=1, stream=stream)
                mpix.wait_enqueue(rs, stream=stream)
                rr = mpix.irecv_enqueue(buf, source=peer, tag=1, stream=stream)
                mpix.wait_enqueue(rr, stream=stream)
            else:
                rr = mpix.irecv_enqueue(buf, source=peer, tag=1, stream=stream)
                mpix.wait_enqueue(rr, stream=stream)
                rs = mpix.isend_enqueue(buf, dest=peer, tag=1, stream=stream)
                mpix.wait_enqueue(rs, stream=stream)

        trace("pingpong warmup")
        for _ in range(max(args.warmup * 4, 20)):
            pp_iter()
        barrier_sync()
        trace("pingpong timed")
        t0 = time.perf_counter()
        for _ in range(args.pp_iters):
            pp_iter()
        barrier_sync()
        pp_elapsed = max_over_ranks(time.perf_counter() - t0)
        # one pair iteration = 2 messages = 1 RTT; loopback iteration = 1
        legs = 2.0 if pingpong_role != "self" else 1.0
        half_rtt_us = pp_elapsed / args.pp_iters / legs * 1e6

    # --------------------------------------- 2. Psend ring bandwidth (value)
    parts = args.partitions
    msg_bytes = args.msg_mib * (1 << 20)
    n_words = msg_bytes // 4
    right = (rank + 1) % world
    left = (rank - 1 + world) % world
    # seeded payload (per rank), so the same arguments give the same inputs
    # and --dump-outputs of two builds can be compared word for word
    gen = torch.Generator().manual_seed(PAYLOAD_SEED + rank)
    send = torch.randint(-2**31, 2**31 - 1, (n_words,), dtype=torch.int32,
                         generator=gen).to(dev)
    recv = torch.zeros_like(send)
    ps = mpix.psend_init(send, parts, dest=right, tag=9)
    pr = mpix.precv_init(recv, parts, source=left, tag=9)
    dps = mpix.prequest_create(ps) if use_gpu else None

    def psend_step():
        mpix.start(pr)
        mpix.start(ps)
        if use_gpu:
            # kernel-triggered: one __device__ MPIX_Pready per partition
            mpix.launch_pready_all(dps, parts, stream.cuda_stream)
        else:
            for p in range(parts):
                mpix.pready(p, ps)
        mpix.wait(pr)
        mpix.wait(ps)

    if half_rtt_us is not None:
        trace(f"pingpong done: half_rtt={half_rtt_us:.2f}us")
    trace("psend warmup")
    for _ in range(args.warmup):
        psend_step()
    barrier_sync()
    trace("psend timed")
    t0 = time.perf_counter()
    for _ in range(args.steps):
        psend_step()
    barrier_sync()
    elapsed = max_over_ranks(time.perf_counter() - t0)
    ms_per_step = elapsed / args.steps * 1e3
    # aggregate: every rank moves msg_bytes per step
    agg_gbps = world * msg_bytes * args.steps / elapsed / 1e9

    if args.dump_outputs:
        # what the last timed step delivered: this rank's receive buffer
        dump_outputs(args.dump_outputs, "recv" if rank == 0
                     else f"recv_rank{rank}", recv, parts, world)

    if dps is not None:
        mpix.prequest_free(dps)
    mpix.request_free(ps)
    mpix.request_free(pr)
    mpix.finalize()
    if dist is not None:
        dist.destroy_process_group()

    if rank == 0:
        print(json.dumps({
            "metric": "Psend GB/s over xGMI (+ stream-enqueued ping-pong half-RTT us)",
            "value": round(agg_gbps, 3),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int32",
            "data": "synthetic",
            "full": args.full,
            "config": {
                "model": "partitioned-ring",
                "pattern": f"ring x{world} ranks, device buffers" if use_gpu
                           else f"ring x{world} ranks, host buffers (no GPU)",
                "msg_bytes_per_rank": msg_bytes,
                "partitions": parts,
                "trigger": "__device__ MPIX_Pready kernel" if use_gpu
                           else "host MPIX_Pready",
                "pingpong_half_rtt_us": (round(half_rtt_us, 3)
                                         if half_rtt_us is not None else None),
                "pingpong_bytes": args.pp_bytes,
                "pingpong_iters": args.pp_iters,
                "pingpong_mode": pingpong_role if world == 1 else "pairs",
                "parallelism": f"spmd{world}",
                "host_cpus": len(pinned) if pinned else None,
            },
        }))


if __name__ == "__main__":
    main()
