/* Face exchange of an nx x ny x nz float grid, packed vs strided.
 *
 * The three face orientations of a row-major grid are the three shapes a
 * strided transfer meets:
 *   x-face  one contiguous plane of ny*nz floats,
 *   y-face  nx runs of nz floats (run = nz * 4 bytes),
 *   z-face  nx*ny single floats (4-byte runs, the worst case).
 * Per exchange a rank sends its two interior faces (index 1 and n-2) of one
 * orientation and receives into its two halo faces (index n-1 and 0), from
 * its peer (rank ^ 1) or, at np = 1, from itself.
 *
 *   pack     pack kernel -> contiguous MPIX_Isend/Irecv_enqueue ->
 *            MPIX_Waitall_enqueue -> unpack kernel   (the existing API only)
 *   strided  MPIX_Isend/Irecv_strided_enqueue -> MPIX_Waitall_enqueue
 *
 * Every (mode, orientation) first runs one exchange on a freshly initialised
 * grid and verifies the halos, then times `iters` exchanges, each retired by
 * hipStreamSynchronize.  One JSON line per (mode, orientation).
 *
 * Built twice: bin/strided_faces (both modes) and bin/strided_faces_pack
 * (-DSTRIDED_FACES_PACK_ONLY: no reference to the strided entry points, so
 * it also runs against a libmpix.so that predates them — the baseline).
 *
 * Run: mpiexec -np 2 bench/bin/strided_faces [nx ny nz iters]
 */
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>
#include <mpi.h>

#include "mpix/mpix.h"

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

/* face element (a, b), a < A, b < B, sits at base + a * sa + b * sb */
struct Face {
    long base, A, B, sa, sb;
    long count() const { return A * B; }
};

static Face face_of(int dim, long p, long nx, long ny, long nz)
{
    switch (dim) {
    case 0: return Face{p * ny * nz, ny, nz, nz, 1};
    case 1: return Face{p * nz, nx, nz, ny * nz, 1};
    default: return Face{p, nx, ny, ny * nz, nz};
    }
}

__device__ __host__ static inline float cell_value(int r, long idx)
{
    return (float)(r * 1000003 + idx % 999983);
}

__global__ void k_init(float *g, long n, int r)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = cell_value(r, i);
}

__global__ void k_pack(float *buf, const float *g, Face f)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < f.A * f.B) buf[i] = g[f.base + (i / f.B) * f.sa + (i % f.B) * f.sb];
}

__global__ void k_unpack(float *g, const float *buf, Face f)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < f.A * f.B) g[f.base + (i / f.B) * f.sa + (i % f.B) * f.sb] = buf[i];
}

/* halo face `h` must hold the peer's interior face `s` */
__global__ void k_verify(const float *g, Face h, Face s, int peer, int *errs)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h.A * h.B) return;
    long a = i / h.B, b = i % h.B;
    float want = cell_value(peer, s.base + a * s.sa + b * s.sb);
    if (g[h.base + a * h.sa + b * h.sb] != want) atomicAdd(errs, 1);
}

static dim3 grid_for(long n) { return dim3((unsigned)((n + 255) / 256)); }

int main(int argc, char **argv)
{
    int provided, size;
    MPI_Init_thread(&argc, &argv, MPI_THREAD_MULTIPLE, &provided);
    MPI_Comm_rank(MPI_COMM_WORLD, &rank);
    MPI_Comm_size(MPI_COMM_WORLD, &size);

    long nx = argc > 1 ? atol(argv[1]) : 256;
    long ny = argc > 2 ? atol(argv[2]) : 256;
    long nz = argc > 3 ? atol(argv[3]) : 256;
    int iters = argc > 4 ? atoi(argv[4]) : 50;
    int warmup = iters / 5 + 3;
    CHECK(nx >= 4 && ny >= 4 && nz >= 4 && iters > 0);

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
    const long dims[3] = {nx, ny, nz};
    long max_face = std::max(ny * nz, std::max(nx * nz, nx * ny));
    float *grid, *sbuf[2], *rbuf[2];
    int *errs;
    HIP(hipMalloc(&grid, n * sizeof(float)));
    for (int i = 0; i < 2; i++) {
        HIP(hipMalloc(&sbuf[i], max_face * sizeof(float)));
        HIP(hipMalloc(&rbuf[i], max_face * sizeof(float)));
    }
    HIP(hipMalloc(&errs, sizeof(int)));

#ifdef STRIDED_FACES_PACK_ONLY
    const int n_modes = 1;
#else
    const int n_modes = 2;
#endif
    const char *mode_name[2] = {"pack", "strided"};
    const char *face_name[3] = {"x", "y", "z"};

    for (int mode = 0; mode < n_modes; mode++) {
        for (int dim = 0; dim < 3; dim++) {
            /* send interior 1 -> peer's halo n-1 (tag 0), interior n-2 ->
             * peer's halo 0 (tag 1) */
            Face snd[2] = {face_of(dim, 1, nx, ny, nz),
                           face_of(dim, dims[dim] - 2, nx, ny, nz)};
            Face rcv[2] = {face_of(dim, dims[dim] - 1, nx, ny, nz),
                           face_of(dim, 0, nx, ny, nz)};
            const long cnt = snd[0].count();
            const int bytes = (int)(cnt * sizeof(float));

            auto exchange = [&]() {
                MPIX_Request req[4];
                if (mode == 0) {
                    for (int i = 0; i < 2; i++)
                        hipLaunchKernelGGL(k_pack, grid_for(cnt), dim3(256), 0,
                                           st, sbuf[i], grid, snd[i]);
                    for (int i = 0; i < 2; i++) {
                        CHECK(MPIX_Irecv_enqueue(rbuf[i], bytes, MPI_BYTE,
                                                 peer, i, MPI_COMM_WORLD,
                                                 &req[i],
                                                 MPIX_QUEUE_HIP_STREAM,
                                                 &st) == 0);
                        CHECK(MPIX_Isend_enqueue(sbuf[i], bytes, MPI_BYTE,
                                                 peer, i, MPI_COMM_WORLD,
                                                 &req[2 + i],
                                                 MPIX_QUEUE_HIP_STREAM,
                                                 &st) == 0);
                    }
                    CHECK(MPIX_Waitall_enqueue(4, req, MPI_STATUSES_IGNORE,
                                               MPIX_QUEUE_HIP_STREAM,
                                               &st) == 0);
                    for (int i = 0; i < 2; i++)
                        hipLaunchKernelGGL(k_unpack, grid_for(cnt), dim3(256),
                                           0, st, grid, rbuf[i], rcv[i]);
                }
#ifndef STRIDED_FACES_PACK_ONLY
                else {
                    for (int i = 0; i < 2; i++) {
                        MPIX_Layout ls, lr;
                        ls.run_bytes = lr.run_bytes = sizeof(float);
                        ls.count[0] = lr.count[0] = (uint64_t)snd[i].B;
                        ls.count[1] = lr.count[1] = (uint64_t)snd[i].A;
                        ls.stride[0] = lr.stride[0] =
                            snd[i].sb * (long)sizeof(float);
                        ls.stride[1] = lr.stride[1] =
                            snd[i].sa * (long)sizeof(float);
                        CHECK(MPIX_Irecv_strided_enqueue(
                                  grid + rcv[i].base, &lr, peer, i,
                                  MPI_COMM_WORLD, &req[i],
                                  MPIX_QUEUE_HIP_STREAM, &st) == 0);
                        CHECK(MPIX_Isend_strided_enqueue(
                                  grid + snd[i].base, &ls, peer, i,
                                  MPI_COMM_WORLD, &req[2 + i],
                                  MPIX_QUEUE_HIP_STREAM, &st) == 0);
                    }
                    CHECK(MPIX_Waitall_enqueue(4, req, MPI_STATUSES_IGNORE,
                                               MPIX_QUEUE_HIP_STREAM,
                                               &st) == 0);
                }
#endif
            };

            /* one verified exchange on a fresh grid */
            hipLaunchKernelGGL(k_init, grid_for(n), dim3(256), 0, st, grid, n,
                               rank);
            HIP(hipMemsetAsync(errs, 0, sizeof(int), st));
            HIP(hipStreamSynchronize(st));
            MPI_Barrier(MPI_COMM_WORLD);
            exchange();
            for (int i = 0; i < 2; i++)
                hipLaunchKernelGGL(k_verify, grid_for(cnt), dim3(256), 0, st,
                                   grid, rcv[i], snd[i], peer, errs);
            int bad = -1;
            HIP(hipMemcpyAsync(&bad, errs, sizeof(int), hipMemcpyDeviceToHost,
                               st));
            HIP(hipStreamSynchronize(st));
            if (bad != 0)
                fprintf(stderr, "[r%d] %s %s-face: %d halo cells wrong\n",
                        rank, mode_name[mode], face_name[dim], bad);
            CHECK(bad == 0);

            std::vector<double> us;
            for (int it = 0; it < warmup + iters; it++) {
                MPI_Barrier(MPI_COMM_WORLD);
                auto t0 = std::chrono::steady_clock::now();
                exchange();
                HIP(hipStreamSynchronize(st));
                auto t1 = std::chrono::steady_clock::now();
                if (it >= warmup)
                    us.push_back(std::chrono::duration<double, std::micro>(
                                     t1 - t0).count());
            }
            std::sort(us.begin(), us.end());
            double sum = 0;
            for (double v : us) sum += v;
            if (rank == 0)
                printf("{\"bench\": \"strided_faces\", \"ranks\": %d, "
                       "\"grid\": [%ld, %ld, %ld], \"mode\": \"%s\", "
                       "\"face\": \"%s\", \"run_bytes\": %ld, "
                       "\"face_bytes\": %d, \"iters\": %d, "
                       "\"us_min\": %.1f, \"us_median\": %.1f, "
                       "\"us_mean\": %.1f, \"us_max\": %.1f}\n",
                       size, nx, ny, nz, mode_name[mode], face_name[dim],
                       dim == 0 ? (long)bytes
                                : dim == 1 ? nz * (long)sizeof(float)
                                           : (long)sizeof(float),
                       bytes, iters, us.front(), us[us.size() / 2],
                       sum / us.size(), us.back());
            fflush(stdout);
        }
    }

    HIP(hipFree(grid));
    for (int i = 0; i < 2; i++) {
        HIP(hipFree(sbuf[i]));
        HIP(hipFree(rbuf[i]));
    }
    HIP(hipFree(errs));
    HIP(hipStreamDestroy(st));
    CHECK(MPIX_Finalize() == 0);
    MPI_Finalize();
    return 0;
}
