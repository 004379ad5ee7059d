/* A y-face of an nx x ny x nz float grid sent as PARTITIONS, packed vs
 * strided, published from a kernel with __device__ MPIX_Pready.
 *
 * The y-face (index 1) of a row-major grid is nx runs of nz floats, ny * nz
 * floats apart.  It is split along x into P slabs of R = nx / P rows; slab p
 * is partition p.  Each exchange sends the face to the peer (rank ^ 1, or
 * ourselves at np = 1), which receives it into its halo face (index ny - 1).
 *
 *   pack     one producer block per partition packs its slab into a staging
 *            buffer and calls MPIX_Pready; plain MPIX_Psend_init /
 *            MPIX_Precv_init on the staging buffers; an unpack kernel after
 *            the wait                              (the plain calls only)
 *   strided  MPIX_Psend_init_strided / MPIX_Precv_init_strided on the grid
 *            itself; the producer block only calls MPIX_Pready
 *
 * Whether the strided partitions go out one descriptor each or as runs is
 * the library's switch, MPIX_PART_RUNS=0 / unset, read once per process: run
 * the program once per variant.  MPIX_STATS=1 then prints the descriptors of
 * exactly that variant at finalize.
 *
 *   fold     a partition is all R rows of its slab: partitions continue the
 *            face at its pitch, a run of them folds into one layout
 *   nofold   a partition is the first R - 1 rows of its slab: the partition
 *            stride is not count * stride, the run takes the kernel variant
 *            with a partition level
 *
 * The program first runs one exchange on a freshly initialised grid and
 * verifies the halo (rows that belong to no partition must be untouched),
 * then times `iters` exchanges, each from MPIX_Start to the end of the
 * waits (and of the unpack kernel).  One JSON line.
 *
 * Run: mpiexec -np 2 bench/bin/strided_parts <pack|strided> <P> <fold|nofold>
 *                                            [nx ny nz iters]
 */
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <mpi.h>

#include "mpix/mpix.h"
#include "mpix/mpix_device.h"

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "[r%d] %s:%d FAILED: %s\n", rank, __FILE__,   \
                    __LINE__, #cond);                                     \
            MPI_Abort(MPI_COMM_WORLD, 1);                                 \
        }                                                                 \
    } while (0)

#define HIP(call) CHECK((call) == hipSuccess)

static int rank = 0;

/* the face at y = j, split into slabs of R rows of which `rows` are sent */
struct Slabs {
    long base;  /* float index of (0, j, 0) */
    long pitch; /* floats between rows: ny * nz */
    long nz;
    long R, rows;
    int P;
    /* floats per partition */
    __device__ __host__ long per() const { return rows * nz; }
};

__device__ __host__ static inline float cell_value(int r, long idx)
{
    return (float)(r * 1000003 + idx % 999983);
}

__global__ void k_init(float *g, long n, int r)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = cell_value(r, i);
}

/* producer, pack variant: block p packs slab p, then publishes it */
__global__ void k_pack_pready(float *buf, const float *g, Slabs s,
                              mpix_prequest_dev_t *preq)
{
    const long p = blockIdx.x, per = s.per();
    for (long i = threadIdx.x; i < per; i += blockDim.x)
        buf[p * per + i] =
            g[s.base + (p * s.R + i / s.nz) * s.pitch + i % s.nz];
    __syncthreads();
    if (threadIdx.x == 0) (void)MPIX_Pready((int)p, preq);
}

/* producer, strided variant: the slab is sent from where it is */
__global__ void k_pready(mpix_prequest_dev_t *preq)
{
    if (threadIdx.x == 0) (void)MPIX_Pready((int)blockIdx.x, preq);
}

__global__ void k_unpack(float *g, const float *buf, Slabs s)
{
    const long p = blockIdx.x, per = s.per();
    for (long i = threadIdx.x; i < per; i += blockDim.x)
        g[s.base + (p * s.R + i / s.nz) * s.pitch + i % s.nz] =
            buf[p * per + i];
}

/* halo face `h` must hold the peer's face `f` in the rows that were sent
 * and its own initial values in the others */
__global__ void k_verify(const float *g, Slabs h, Slabs f, long nx, int me,
                         int peer, int *errs)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nx * h.nz) return;
    long a = i / h.nz, b = i % h.nz;
    long at = h.base + a * h.pitch + b;
    float want = (a % h.R < h.rows)
        ? cell_value(peer, f.base + a * f.pitch + b)
        : cell_value(me, at);
    if (g[at] != want) atomicAdd(errs, 1);
}

int main(int argc, char **argv)
{
    int provided, size;
    MPI_Init_thread(&argc, &argv, MPI_THREAD_MULTIPLE, &provided);
    MPI_Comm_rank(MPI_COMM_WORLD, &rank);
    MPI_Comm_size(MPI_COMM_WORLD, &size);

    CHECK(argc >= 4);
    const bool pack = strcmp(argv[1], "pack") == 0;
    CHECK(pack || strcmp(argv[1], "strided") == 0);
    const int P = atoi(argv[2]);
    const bool fold = strcmp(argv[3], "fold") == 0;
    CHECK(fold || strcmp(argv[3], "nofold") == 0);
    long nx = argc > 4 ? atol(argv[4]) : 256;
    long ny = argc > 5 ? atol(argv[5]) : 256;
    long nz = argc > 6 ? atol(argv[6]) : 256;
    int iters = argc > 7 ? atoi(argv[7]) : 50;
    int warmup = iters / 5 + 3;
    CHECK(P > 0 && nx % P == 0 && nx / P >= 2 && ny >= 4 && nz >= 4 &&
          iters > 0);

    int ndev = 0;
    HIP(hipGetDeviceCount(&ndev));
    CHECK(ndev > 0);
    HIP(hipSetDevice(rank % ndev));
    CHECK(MPIX_Init() == 0);

    int peer = (size >= 2) ? (rank ^ 1) : rank;
    CHECK(peer < size);
    hipStream_t st;
    HIP(hipStreamCreate(&st));

    const long n = nx * ny * nz;
    const long R = nx / P, rows = fold ? R : R - 1;
    const Slabs snd{1 * nz, ny * nz, nz, R, rows, P};
    const Slabs rcv{(ny - 1) * nz, ny * nz, nz, R, rows, P};
    const long per = snd.per();
    const long part_bytes = per * (long)sizeof(float);

    float *grid, *sbuf, *rbuf;
    int *errs;
    HIP(hipMalloc(&grid, n * sizeof(float)));
    HIP(hipMalloc(&sbuf, P * part_bytes));
    HIP(hipMalloc(&rbuf, P * part_bytes));
    HIP(hipMalloc(&errs, sizeof(int)));

    MPIX_Request sreq, rreq;
    if (pack) {
        CHECK(MPIX_Precv_init(rbuf, P, part_bytes, MPI_BYTE, peer, 0,
                              MPI_COMM_WORLD, MPI_INFO_NULL, &rreq) == 0);
        CHECK(MPIX_Psend_init(sbuf, P, part_bytes, MPI_BYTE, peer, 0,
                              MPI_COMM_WORLD, MPI_INFO_NULL, &sreq) == 0);
    } else {
        MPIX_Layout l;
        l.run_bytes = (uint64_t)nz * sizeof(float);
        l.count[0] = (uint64_t)rows;
        l.count[1] = 1;
        l.stride[0] = snd.pitch * (int64_t)sizeof(float);
        l.stride[1] = l.stride[0] * (int64_t)rows;
        const int64_t part_stride = R * snd.pitch * (int64_t)sizeof(float);
        CHECK(MPIX_Precv_init_strided(grid + rcv.base, P, &l, part_stride,
                                      peer, 0, MPI_COMM_WORLD, MPI_INFO_NULL,
                                      &rreq) == 0);
        CHECK(MPIX_Psend_init_strided(grid + snd.base, P, &l, part_stride,
                                      peer, 0, MPI_COMM_WORLD, MPI_INFO_NULL,
                                      &sreq) == 0);
    }
    MPIX_Prequest preq;
    CHECK(MPIX_Prequest_create(sreq, &preq) == 0);

    auto exchange = [&]() {
        CHECK(MPIX_Start(&rreq) == 0);
        CHECK(MPIX_Start(&sreq) == 0);
        if (pack)
            hipLaunchKernelGGL(k_pack_pready, dim3(P), dim3(1024), 0, st,
                               sbuf, grid, snd, (mpix_prequest_dev_t *)preq);
        else
            hipLaunchKernelGGL(k_pready, dim3(P), dim3(64), 0, st,
                               (mpix_prequest_dev_t *)preq);
        CHECK(MPIX_Wait(&rreq, MPI_STATUS_IGNORE) == 0);
        CHECK(MPIX_Wait(&sreq, MPI_STATUS_IGNORE) == 0);
        if (pack)
            hipLaunchKernelGGL(k_unpack, dim3(P), dim3(1024), 0, st, grid,
                               rbuf, rcv);
        HIP(hipStreamSynchronize(st));
    };

    /* one verified exchange on a fresh grid */
    hipLaunchKernelGGL(k_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       st, grid, n, rank);
    HIP(hipMemsetAsync(errs, 0, sizeof(int), st));
    HIP(hipStreamSynchronize(st));
    MPI_Barrier(MPI_COMM_WORLD);
    exchange();
    hipLaunchKernelGGL(k_verify, dim3((unsigned)((nx * nz + 255) / 256)),
                       dim3(256), 0, st, grid, rcv, snd, nx, rank, peer, errs);
    int bad = -1;
    HIP(hipMemcpyAsync(&bad, errs, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP(hipStreamSynchronize(st));
    if (bad != 0)
        fprintf(stderr, "[r%d] %s %s: %d halo cells wrong\n", rank, argv[1],
                argv[3], bad);
    CHECK(bad == 0);

    std::vector<double> us;
    for (int it = 0; it < warmup + iters; it++) {
        MPI_Barrier(MPI_COMM_WORLD);
        auto t0 = std::chrono::steady_clock::now();
        exchange();
        auto t1 = std::chrono::steady_clock::now();
        if (it >= warmup)
            us.push_back(
                std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    std::sort(us.begin(), us.end());
    double sum = 0;
    for (double v : us) sum += v;
    const char *runs = getenv("MPIX_PART_RUNS");
    if (rank == 0)
        printf("{\"bench\": \"strided_parts\", \"ranks\": %d, "
               "\"grid\": [%ld, %ld, %ld], \"mode\": \"%s\", "
               "\"runs\": \"%s\", \"shape\": \"%s\", \"partitions\": %d, "
               "\"run_bytes\": %ld, \"part_bytes\": %ld, \"iters\": %d, "
               "\"us_min\": %.1f, \"us_median\": %.1f, \"us_mean\": %.1f, "
               "\"us_max\": %.1f}\n",
               size, nx, ny, nz, argv[1],
               pack ? "n/a" : (runs && atoi(runs) == 0 ? "off" : "on"),
               argv[3], P, nz * (long)sizeof(float), part_bytes, iters,
               us.front(), us[us.size() / 2], sum / us.size(), us.back());
    fflush(stdout);

    CHECK(MPIX_Prequest_free(&preq) == 0);
    CHECK(MPIX_Request_free(&sreq) == 0);
    CHECK(MPIX_Request_free(&rreq) == 0);
    HIP(hipFree(grid));
    HIP(hipFree(sbuf));
    HIP(hipFree(rbuf));
    HIP(hipFree(errs));
    HIP(hipStreamDestroy(st));
    CHECK(MPIX_Finalize() == 0);
    MPI_Finalize();
    return 0;
}
