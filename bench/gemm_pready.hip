/* Compute/comm overlap: per-band __device__ MPIX_Pready inside a
 * hand-written CDNA4 MFMA bf16 GEMM (BASELINE.json config 5).
 *
 * Each rank computes C = A x B (bf16 in, fp32 accumulate, bf16 out) with a
 * gfx950 MFMA kernel (v_mfma_f32_16x16x32_bf16; the default variant 4 has
 * 256x256 tiles with BK=64 staged into two LDS buffers by global_load_lds,
 * an XCD-aware workgroup remap and a grouped block order; variants 2 and 3
 * have 128x128 tiles, 5 and 6 other pipelines on the 256x256 tile) and
 * partition-sends C to its right neighbor: C's row bands are the NPARTS
 * partitions of a persistent MPIX_Psend.  When the LAST workgroup of a band
 * finishes its C tile it publishes the band from inside the kernel
 * (system-release ticket counter + MPIX_Pready), so the proxy streams
 * finished bands over xGMI while the rest of the GEMM is still running.
 * The receiver MPIX_Waits; every VERIFY_EVERY iterations an xor checksum of
 * what it received is compared with the sender's C.
 *
 * Reports overlapped time vs GEMM-then-send, GEMM TFLOP/s, and effective
 * bandwidth.  Run: mpiexec -np N bench/bin/gemm_pready [M N K iters]
 *
 * --check [M N K [nparts]] (default 256 256 512, one band per tile row)
 * verifies the kernel instead of timing it: ALL of C against a float64
 * host reference (bench/gemm_check.h) with publish off, then again with the
 * bands published and sent, Crecv byte-identical to the sender's C and every
 * band counter complete.  See run_check below.
 *
 * Publish protocol per §6 Guideline 16 of the CDNA4 guide: plain C stores
 * -> s_waitcnt vmcnt(0) -> __syncthreads -> lane0 system release fence +
 * restated vmcnt wait -> relaxed system fetch_add ticket; the last arriver
 * (acquire fence) calls MPIX_Pready, itself a system-scope release store.
 */
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <mpi.h>

#include "mpix/mpix.h"
#include "mpix/mpix_device.h"

#include "gemm_check.h"

#define NPARTS 64

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "[r%d] %s:%d FAILED: %s\n", rank, __FILE__,   \
                    __LINE__, #cond);                                     \
            MPI_Abort(MPI_COMM_WORLD, 1);                                 \
        }                                                                 \
    } while (0)

#define HIP(call) CHECK((call) == hipSuccess)

using bf16 = __bf16;
typedef __attribute__((ext_vector_type(8))) short frag8;   /* A/B: 8 bf16 */
typedef __attribute__((ext_vector_type(4))) float frag4f;  /* C/D: 4 fp32 */
typedef __attribute__((ext_vector_type(4))) float float4v;

/* ------------------------------------------------------------- the kernel
 * BM=BN=128, BK=32, 256 threads = 4 waves in a 2x2 wave grid; each wave
 * owns a 64x64 quadrant = 4x4 mfma_f32_16x16x32_bf16 accumulators.
 * A is [M][K] row-major, B is [K][N] row-major, C is [M][N] row-major.
 * LDS images: As[128][32] linear; Bs stored transposed as Bt[128][32]
 * (n-major) so both A and B fragments are contiguous ds_read_b128 loads
 * (lane l of a 16x16x32 fragment reads 8 bf16 at k = (l>>4)*8).
 */
#define BM 128
#define BN 128
#define BK 32
#ifndef MPIX_GEMM_VARIANT
/* default = variant 4 (256^2 tile, BK=64, 8-wave glds double-buffer,
 * source-side bank swizzle): 909.8 TF @8192^3 — ladder: v1 236, v2 476,
 * v3 511, v5 (BK=32 4-buf raw-barrier pipeline) 722 — see
 * profiles/r02_gemm_ladder.md */
#define MPIX_GEMM_VARIANT 4
#endif

#if MPIX_GEMM_VARIANT == 6
/* Variant 6 — 8-phase C-quadrant interleave on v4's 256x256 / BK=64 / 2
 * LDS buffer geometry (the guide's T3+T4 structure: counted vmcnt keeps
 * the LDS-DMA pipeline alive ACROSS raw barriers; never vmcnt(0) in the
 * main loop).  One iteration computes K-tiles (2i, 2i+1) in 8 phases;
 * each phase = one C-quadrant (16 MFMAs) + ONE 16-KiB piece prefetch.
 *
 * Piece-death schedule (every wave reads quadrant (qm,qn) at the same
 * phase, so a region is globally dead one barrier after its last use):
 *   buf0 (tile 2i):   A-qm0 dies p1, B-qn0 p2, A-qm1 p3, B-qn1 p3
 *   buf1 (tile 2i+1): A-qm0 dies p5, B-qn0 p6, A-qm1 p7, B-qn1 p7
 * Prefetch rotation (issue exactly after death of the region it fills):
 *   p0:A1(2i+1)  p1:B1(2i+1)  p2:A0(2i+2)  p3:B0(2i+2)
 *   p4:A1(2i+2)  p5:B1(2i+2)  p6:A0(2i+3)  p7:B0(2i+3)
 * The tightest consumer (p1/p5: B-qn1 issued 4 phases earlier) sets the
 * uniform wait: s_waitcnt vmcnt(6) (newest 3 pieces = 6 glds stay in
 * flight) before each barrier; the tail (no more issues) degrades to
 * vmcnt(0).  Prologue preloads tile0 (4 pieces) + tile1
 * A0,B0 — exactly what a previous iteration would have issued. */
#undef BM
#undef BN
#undef BK
#define BM 256
#define BN 256
#define BK 64
#define V4_THREADS 512

__global__ __launch_bounds__(V4_THREADS)
void gemm_bf16_pready(const bf16 *__restrict__ A, const bf16 *__restrict__ Bt,
                      bf16 *__restrict__ C, int M, int N, int K,
                      uint32_t *band_cnt, int nparts, int blocks_per_band,
                      void *dpreq, int publish)
{
    __shared__ bf16 lds[2 * 2 * BM * BK];
    auto As = [&](int b) -> bf16 * { return lds + b * 2 * BM * BK; };
    auto Bs = [&](int b) -> bf16 * { return As(b) + BM * BK; };

    int nwg = gridDim.x;
    int wg = blockIdx.x;
    {
        int q = nwg / 8, r = nwg % 8, xcd = wg % 8;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + wg / 8;
    }
    int tiles_n = N / BN;
    int tm = wg / tiles_n, tn = wg % tiles_n;

    int tid = threadIdx.x;
    int wave = tid >> 6, lane = tid & 63;
    int wm = wave >> 2, wn = wave & 3;
    int lrow = lane & 15, lk8 = (lane >> 4) * 8;

    frag4f acc[8][4] = {};
    const bf16 *Ab = A + (size_t)tm * BM * K;
    const bf16 *Bb = Bt + (size_t)tn * BN * K;

    /* 16-KiB piece = 16 x 1-KiB LDS chunks (quarters of the operand's
     * 32-KiB tile image), 2 glds passes x (8 waves x 1 chunk) */
    static const __device__ uint8_t CH_A0[16] = {0, 1, 2,  3,  4,  5,  6,  7,
                                                 16, 17, 18, 19, 20, 21, 22, 23};
    static const __device__ uint8_t CH_A1[16] = {8,  9,  10, 11, 12, 13, 14, 15,
                                                 24, 25, 26, 27, 28, 29, 30, 31};
    static const __device__ uint8_t CH_B0[16] = {0, 1, 2,  3,  8,  9,  10, 11,
                                                 16, 17, 18, 19, 24, 25, 26, 27};
    static const __device__ uint8_t CH_B1[16] = {4, 5, 6,  7,  12, 13, 14, 15,
                                                 20, 21, 22, 23, 28, 29, 30, 31};

    auto glds_piece = [&](const bf16 *gbase, bf16 *lbase, int t,
                          const uint8_t *chunks) {
        const char *g0 = (const char *)gbase + (size_t)t * BK * sizeof(bf16);
        #pragma unroll
        for (int p = 0; p < 2; p++) {
            unsigned o = ((unsigned)chunks[p * 8 + wave] * 64 +
                          (unsigned)lane) * 16;
            unsigned row = o >> 7;
            unsigned cb = (o & 127u) ^ ((row & 7u) << 4);
            const void *src = g0 + (size_t)row * K * sizeof(bf16) + cb;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) uint32_t *)src,
                (__attribute__((address_space(3))) uint32_t *)
                    ((char *)lbase + o),
                16, 0, 0);
        }
    };
    auto frag_at = [&](const bf16 *base, int row, int kb) -> frag8 {
        int col = kb ^ ((row & 7) << 3);
        return *(const frag8 *)&base[row * BK + col];
    };
    /* one C-quadrant (4x2 fragments) over the tile's full K=64 */
    auto compute_quad = [&](int buf, int qm, int qn) {
        #pragma unroll
        for (int kh = 0; kh < 2; kh++) {
            int kb = kh * 32 + lk8;
            frag8 af[4], bf[2];
            #pragma unroll
            for (int i = 0; i < 4; i++)
                af[i] = frag_at(As(buf),
                                wm * 128 + qm * 64 + i * 16 + lrow, kb);
            #pragma unroll
            for (int j = 0; j < 2; j++)
                bf[j] = frag_at(Bs(buf),
                                wn * 64 + qn * 32 + j * 16 + lrow, kb);
            #pragma unroll
            for (int i = 0; i < 4; i++)
                #pragma unroll
                for (int j = 0; j < 2; j++)
                    acc[qm * 4 + i][qn * 2 + j] =
                        __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            af[i], bf[j], acc[qm * 4 + i][qn * 2 + j], 0, 0,
                            0);
        }
    };

    int tiles = K / BK; /* host asserts tiles even and >= 4 for this variant */
    /* prologue = what a previous iteration would have left in flight */
    glds_piece(Ab, As(0), 0, CH_A0);
    glds_piece(Bb, Bs(0), 0, CH_B0);
    glds_piece(Ab, As(0), 0, CH_A1);
    glds_piece(Bb, Bs(0), 0, CH_B1);
    glds_piece(Ab, As(1), 1, CH_A0);
    glds_piece(Bb, Bs(1), 1, CH_B0);

    for (int t2 = 0; t2 < tiles; t2 += 2) {
        bool tail = (t2 + 3 >= tiles);
        #pragma unroll
        for (int p = 0; p < 8; p++) {
            /* leave newest 3 pieces (6 glds) in flight: the tightest
             * consumer (p1/p5: B-qn1 issued 4 phases earlier) still
             * retires under vmcnt(6); everything else is >=5 deep */
            if (!tail)
                asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            /* prefetch rotation (see header comment) */
            switch (p) {
            case 0:
                glds_piece(Ab, As(1), t2 + 1, CH_A1);
                break;
            case 1:
                glds_piece(Bb, Bs(1), t2 + 1, CH_B1);
                break;
            case 2:
                if (t2 + 2 < tiles) glds_piece(Ab, As(0), t2 + 2, CH_A0);
                break;
            case 3:
                if (t2 + 2 < tiles) glds_piece(Bb, Bs(0), t2 + 2, CH_B0);
                break;
            case 4:
                if (t2 + 2 < tiles) glds_piece(Ab, As(0), t2 + 2, CH_A1);
                break;
            case 5:
                if (t2 + 2 < tiles) glds_piece(Bb, Bs(0), t2 + 2, CH_B1);
                break;
            case 6:
                if (t2 + 3 < tiles) glds_piece(Ab, As(1), t2 + 3, CH_A0);
                break;
            case 7:
                if (t2 + 3 < tiles) glds_piece(Bb, Bs(1), t2 + 3, CH_B0);
                break;
            }
            compute_quad(p >> 2, (p >> 1) & 1, p & 1);
        }
    }

    size_t crow0 = (size_t)tm * BM + wm * 128;
    size_t ccol0 = (size_t)tn * BN + wn * 64;
    #pragma unroll
    for (int i = 0; i < 8; i++)
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            size_t col = ccol0 + j * 16 + (lane & 15);
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                size_t row = crow0 + i * 16 + (lane >> 4) * 4 + r;
                C[row * N + col] = (bf16)acc[i][j][r];
            }
        }

    if (!publish) return;
    int band = (int)((size_t)tm * BM * (size_t)nparts / M);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t prev = __hip_atomic_fetch_add(&band_cnt[band], 1,
                                               __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_SYSTEM);
        if (prev == (uint32_t)blocks_per_band - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            MPIX_Pready(band, dpreq);
        }
    }
}

#elif MPIX_GEMM_VARIANT == 5
/* Variant 5 — v4's 256x256 glds structure pushed to the guide's pipelined
 * tier: BK=32 tiles in FOUR LDS buffers (4 x 32 KiB), two tiles in flight
 * across RAW barriers with counted vmcnt (never vmcnt(0) in the loop —
 * __syncthreads would drain the LDS-DMA), one barrier per K-tile:
 *
 *   iter t: s_waitcnt vmcnt(4)      // everything but the newest tile landed
 *           s_barrier + lgkmcnt(0)  // raw barrier: glds stays in flight
 *           glds tile t+3 -> buf[(t+3)&3]   // overwrite of buf[(t-1)&3]
 *                                           // is ordered by the barrier
 *           compute tile t from buf[t&3]
 *
 * 64-B LDS rows (BK=32): rows r, r+4, r+8, r+12 share a 256-B bank row,
 * so the source-side swizzle XORs the 16-B slot with (row>>2)&3 —
 * fragment groups hit 16 distinct (quarter, slot) pairs, conflict-free.
 */
#undef BM
#undef BN
#undef BK
#define BM 256
#define BN 256
#define BK 32
#define V4_THREADS 512

__global__ __launch_bounds__(V4_THREADS)
void gemm_bf16_pready(const bf16 *__restrict__ A, const bf16 *__restrict__ Bt,
                      bf16 *__restrict__ C, int M, int N, int K,
                      uint32_t *band_cnt, int nparts, int blocks_per_band,
                      void *dpreq, int publish)
{
    __shared__ bf16 lds[4 * 2 * BM * BK]; /* 4 bufs x (A+B) x 16 KiB */
    auto As = [&](int b) -> bf16 * { return lds + b * 2 * BM * BK; };
    auto Bs = [&](int b) -> bf16 * { return As(b) + BM * BK; };

    int nwg = gridDim.x;
    int wg = blockIdx.x;
    {
        int q = nwg / 8, r = nwg % 8, xcd = wg % 8;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + wg / 8;
    }
    int tiles_n = N / BN;
    int tm = wg / tiles_n, tn = wg % tiles_n;

    int tid = threadIdx.x;
    int wave = tid >> 6, lane = tid & 63;
    int wm = wave >> 2, wn = wave & 3;
    int lrow = lane & 15, lk8 = (lane >> 4) * 8;

    frag4f acc[8][4] = {};
    const bf16 *Ab = A + (size_t)tm * BM * K;
    const bf16 *Bb = Bt + (size_t)tn * BN * K;

    /* 16-KiB tile = 2 glds passes x 8 KiB; swizzle on the global source */
    auto glds_tile = [&](const bf16 *gbase, bf16 *lbase, int t) {
        const char *g0 = (const char *)(gbase) + (size_t)t * BK * sizeof(bf16);
        #pragma unroll
        for (int p = 0; p < 2; p++) {
            unsigned o = ((unsigned)(p * 8 + wave) * 64 + (unsigned)lane) * 16;
            unsigned row = o >> 6;
            unsigned cb = (o & 63u) ^ (((row >> 2) & 3u) << 4);
            const void *src = g0 + (size_t)row * K * sizeof(bf16) + cb;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) uint32_t *)src,
                (__attribute__((address_space(3))) uint32_t *)
                    ((char *)lbase + o),
                16, 0, 0);
        }
    };
    auto frag_at = [&](const bf16 *base, int row, int kb) -> frag8 {
        int col = kb ^ (((row >> 2) & 3) << 3);
        return *(const frag8 *)&base[row * BK + col];
    };

    auto compute = [&](int buf) {
        frag8 af[8], bf[4];
        #pragma unroll
        for (int i = 0; i < 8; i++)
            af[i] = frag_at(As(buf), wm * 128 + i * 16 + lrow, lk8);
        #pragma unroll
        for (int j = 0; j < 4; j++)
            bf[j] = frag_at(Bs(buf), wn * 64 + j * 16 + lrow, lk8);
        #pragma unroll
        for (int i = 0; i < 8; i++)
            #pragma unroll
            for (int j = 0; j < 4; j++)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    af[i], bf[j], acc[i][j], 0, 0, 0);
    };

    int tiles = K / BK;
    glds_tile(Ab, As(0), 0);
    glds_tile(Bb, Bs(0), 0);
    if (tiles > 1) { glds_tile(Ab, As(1), 1); glds_tile(Bb, Bs(1), 1); }
    if (tiles > 2) { glds_tile(Ab, As(2), 2); glds_tile(Bb, Bs(2), 2); }
    for (int t = 0; t < tiles; t++) {
        if (t + 2 < tiles)
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (t + 3 < tiles) {
            glds_tile(Ab, As((t + 3) & 3), t + 3);
            glds_tile(Bb, Bs((t + 3) & 3), t + 3);
        }
        compute(t & 3);
    }

    size_t crow0 = (size_t)tm * BM + wm * 128;
    size_t ccol0 = (size_t)tn * BN + wn * 64;
    #pragma unroll
    for (int i = 0; i < 8; i++)
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            size_t col = ccol0 + j * 16 + (lane & 15);
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                size_t row = crow0 + i * 16 + (lane >> 4) * 4 + r;
                C[row * N + col] = (bf16)acc[i][j][r];
            }
        }

    if (!publish) return;
    int band = (int)((size_t)tm * BM * (size_t)nparts / M);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t prev = __hip_atomic_fetch_add(&band_cnt[band], 1,
                                               __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_SYSTEM);
        if (prev == (uint32_t)blocks_per_band - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            MPIX_Pready(band, dpreq);
        }
    }
}

#elif MPIX_GEMM_VARIANT == 4
/* Grouped block order (default G=4, measured +9.7%: 900->987 TF @8192^3):
 * consecutive workgroups cover a tiles_m x G super-column so the A rows
 * of a block-row re-hit L2 (PMC showed 2.25x HBM re-read in plain order).
 * -DMPIX_GEMM_GROUP=0 restores the plain row-major order. */
#ifndef MPIX_GEMM_GROUP
#define MPIX_GEMM_GROUP 4
#endif
/* Variant 4 — guide §5 "glds + 2 LDS buffers + BK=64" structure on a
 * 256x256 tile (the measured ~1.1-1.2 PF tier for this shape):
 *  - 512 threads = 8 waves in a 2(M)x4(N) grid, each owning a 128x64
 *    C sub-tile = 8x4 mfma_f32_16x16x32_bf16 accumulators;
 *  - both operands staged HBM->LDS with __builtin_amdgcn_global_load_lds
 *    (dwordx4), double-buffered (2 x 64 KiB of the 160 KiB LDS);
 *  - B is taken PRE-TRANSPOSED [N][K] so A and B tiles are both [256][64]
 *    row-major and every fragment is one 16-B ds_read_b128;
 *  - glds writes are lane-linear, so the T2 bank-conflict swizzle is
 *    applied on the per-lane GLOBAL source address (and undone on the
 *    ds_read): rows alternate 256-B bank-row halves (128-B rows), the
 *    XOR spreads a 16-lane fragment group over 16 distinct 16-B slots —
 *    conflict-free.
 */
#undef BM
#undef BN
#undef BK
#define BM 256
#define BN 256
#define BK 64
#define V4_THREADS 512

__global__ __launch_bounds__(V4_THREADS)
void gemm_bf16_pready(const bf16 *__restrict__ A, const bf16 *__restrict__ Bt,
                      bf16 *__restrict__ C, int M, int N, int K,
                      uint32_t *band_cnt, int nparts, int blocks_per_band,
                      void *dpreq, int publish)
{
    /* one buffer = A[256][64] + B[256][64] bf16 = 64 KiB; two buffers */
    __shared__ bf16 lds[2 * 2 * BM * BK];
    auto As = [&](int b) -> bf16 * { return lds + b * 2 * BM * BK; };
    auto Bs = [&](int b) -> bf16 * { return As(b) + BM * BK; };

    int nwg = gridDim.x;
    int wg = blockIdx.x;
    {
        int q = nwg / 8, r = nwg % 8, xcd = wg % 8;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + wg / 8;
    }
    int tiles_n = N / BN;
    int tm, tn;
#if MPIX_GEMM_GROUP > 0
    {
        /* bijective grouped order: full G-wide column groups first, then a
         * (tiles_n % G)-wide tail group — a naive modulo fallback silently
         * COLLIDED for tiles_n % G != 0 (two wgs computing one C tile,
         * another tile never written; mirrored in the host bijectivity
         * test tests/test_units.py::test_gemm_group_mapping_bijective) */
        int tiles_m = M / BM;
        int gcols = (tiles_n / MPIX_GEMM_GROUP) * MPIX_GEMM_GROUP;
        int ngrouped = tiles_m * gcols;
        if (wg < ngrouped) {
            int per_group = tiles_m * MPIX_GEMM_GROUP;
            int group = wg / per_group, rem = wg % per_group;
            tn = group * MPIX_GEMM_GROUP + rem % MPIX_GEMM_GROUP;
            tm = rem / MPIX_GEMM_GROUP;
        } else {
            int tail = tiles_n - gcols; /* >= 1 when any wg lands here */
            int r = wg - ngrouped;
            tn = gcols + r % tail;
            tm = r / tail;
        }
    }
#else
    tm = wg / tiles_n;
    tn = wg % tiles_n;
#endif

    int tid = threadIdx.x;
    int wave = tid >> 6, lane = tid & 63;
    int wm = wave >> 2, wn = wave & 3; /* 2x4 wave grid */
    int lrow = lane & 15, lk8 = (lane >> 4) * 8;

    frag4f acc[8][4] = {};
    const bf16 *Ab = A + (size_t)tm * BM * K;
    const bf16 *Bb = Bt + (size_t)tn * BN * K;

    /* glds: each wave stages 4 contiguous 1-KiB LDS chunks per operand
     * tile (8 waves x 4 passes x 1 KiB = 32 KiB).  LDS dest is
     * wave-uniform base + lane*16; the per-lane GLOBAL source carries the
     * swizzle: LDS linear byte o <- global (row = o/128,
     * col_byte = (o%128) ^ ((row&7)<<4)). */
    auto glds_tile = [&](const bf16 *gbase, bf16 *lbase, int t) {
        const char *g0 = (const char *)(gbase) + (size_t)t * BK * sizeof(bf16);
        #pragma unroll
        for (int p = 0; p < 4; p++) {
            unsigned o = ((unsigned)(p * 8 + wave) * 64 + (unsigned)lane) * 16;
            unsigned row = o >> 7;
            unsigned cb = (o & 127u) ^ ((row & 7u) << 4);
            const void *src = g0 + (size_t)row * K * sizeof(bf16) + cb;
            /* dest uses the lane-linear address; hardware applies
             * base+lane*16 itself, per-lane addr must match that shape */
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) uint32_t *)src,
                (__attribute__((address_space(3))) uint32_t *)
                    ((char *)lbase + o),
                16, 0, 0);
        }
    };
    /* fragment read: element (row, k..k+7) lives at row*64 + (k ^ swz) */
    auto frag_at = [&](const bf16 *base, int row, int kb) -> frag8 {
        int col = kb ^ ((row & 7) << 3);
        return *(const frag8 *)&base[row * BK + col];
    };

    auto compute = [&](int buf) {
        #pragma unroll
        for (int kh = 0; kh < 2; kh++) {
            int kb = kh * 32 + lk8;
            frag8 af[8], bf[4];
            #pragma unroll
            for (int i = 0; i < 8; i++)
                af[i] = frag_at(As(buf), wm * 128 + i * 16 + lrow, kb);
            #pragma unroll
            for (int j = 0; j < 4; j++)
                bf[j] = frag_at(Bs(buf), wn * 64 + j * 16 + lrow, kb);
            #pragma unroll
            for (int i = 0; i < 8; i++)
                #pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    };

    int tiles = K / BK;
    glds_tile(Ab, As(0), 0);
    glds_tile(Bb, Bs(0), 0);
    __syncthreads(); /* hipcc inserts the vmcnt(0) drain for the glds */
    for (int t = 0; t < tiles; t++) {
        int cur = t & 1;
        if (t + 1 < tiles) {
            glds_tile(Ab, As(1 - cur), t + 1);
            glds_tile(Bb, Bs(1 - cur), t + 1);
        }
        compute(cur);
        __syncthreads();
    }

    size_t crow0 = (size_t)tm * BM + wm * 128;
    size_t ccol0 = (size_t)tn * BN + wn * 64;
    #pragma unroll
    for (int i = 0; i < 8; i++)
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            size_t col = ccol0 + j * 16 + (lane & 15);
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                size_t row = crow0 + i * 16 + (lane >> 4) * 4 + r;
                C[row * N + col] = (bf16)acc[i][j][r];
            }
        }

    if (!publish) return;
    int band = (int)((size_t)tm * BM * (size_t)nparts / M);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t prev = __hip_atomic_fetch_add(&band_cnt[band], 1,
                                               __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_SYSTEM);
        if (prev == (uint32_t)blocks_per_band - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            MPIX_Pready(band, dpreq);
        }
    }
}

#elif MPIX_GEMM_VARIANT == 3
/* Variant 3 (round-2 candidate, compile-validated; measure with --check
 * first): BK=64 (half the barriers of v1/v2), double-buffered LDS, and a
 * T14-style register prefetch — tile t+1 streams HBM->VGPRs while tile t
 * computes, then drains into the other LDS buffer; ONE barrier per K-tile.
 * Images stay the conflict-free padded row-major layout measured in v2. */
#undef BK
#define BK 64
#define LPA (BK + 8)   /* A row pitch, 144 B (16-B aligned frag reads) */
#define LPB (BN + 8)   /* B row pitch, 272 B */

__global__ __launch_bounds__(256)
void gemm_bf16_pready(const bf16 *__restrict__ A, const bf16 *__restrict__ B,
                      bf16 *__restrict__ C, int M, int N, int K,
                      uint32_t *band_cnt, int nparts, int blocks_per_band,
                      void *dpreq, int publish)
{
    __shared__ bf16 lds[2 * (BM * LPA + BK * LPB)];
    /* buffer b: A at b*(BM*LPA+BK*LPB), B right after its A */
    auto As = [&](int b) -> bf16 * { return lds + b * (BM * LPA + BK * LPB); };
    auto Bs = [&](int b) -> bf16 * { return As(b) + BM * LPA; };

    int nwg = gridDim.x;
    int wg = blockIdx.x;
    {
        int q = nwg / 8, r = nwg % 8, xcd = wg % 8;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + wg / 8;
    }
    int tiles_n = N / BN;
    int tm = wg / tiles_n, tn = wg % tiles_n;

    int tid = threadIdx.x;
    int wave = tid >> 6, lane = tid & 63;
    int wm = wave >> 1, wn = wave & 1;
    int lrow = lane & 15, lk8 = (lane >> 4) * 8;

    frag4f acc[4][4] = {};
    const bf16 *Ab = A + (size_t)tm * BM * K;
    const bf16 *Bb = B + tn * BN;

    /* per-thread slices: 4 x 16 B of A and of B per K-tile */
    int a_row[4], a_col[4], b_k[4], b_n[4];
    #pragma unroll
    for (int p = 0; p < 4; p++) {
        int ia = (p * 256 + tid) * 8;
        a_row[p] = ia / BK; a_col[p] = ia % BK;
        b_k[p] = ia / BN;  b_n[p] = ia % BN;
    }
    frag8 pa[4], pb[4];

    auto load_tile = [&](int t) {
        const bf16 *sa = Ab + (size_t)t * BK;
        const bf16 *sb = Bb + (size_t)t * BK * N;
        #pragma unroll
        for (int p = 0; p < 4; p++) {
            pa[p] = *(const frag8 *)&sa[(size_t)a_row[p] * K + a_col[p]];
            pb[p] = *(const frag8 *)&sb[(size_t)b_k[p] * N + b_n[p]];
        }
    };
    auto store_tile = [&](int buf) {
        #pragma unroll
        for (int p = 0; p < 4; p++) {
            *(frag8 *)&As(buf)[a_row[p] * LPA + a_col[p]] = pa[p];
            *(frag8 *)&Bs(buf)[b_k[p] * LPB + b_n[p]] = pb[p];
        }
    };
    auto compute = [&](int buf) {
        #pragma unroll
        for (int kh = 0; kh < 2; kh++) {
            frag8 af[4], bf[4];
            int kb = kh * 32 + lk8;
            #pragma unroll
            for (int i = 0; i < 4; i++) {
                int row = wm * 64 + i * 16 + lrow;
                af[i] = *(const frag8 *)&As(buf)[row * LPA + kb];
            }
            #pragma unroll
            for (int j = 0; j < 4; j++) {
                int col = wn * 64 + j * 16 + lrow;
                #pragma unroll
                for (int e = 0; e < 8; e++)
                    ((bf16 *)&bf[j])[e] = Bs(buf)[(kb + e) * LPB + col];
            }
            #pragma unroll
            for (int i = 0; i < 4; i++)
                #pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    };

    int tiles = K / BK;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < tiles; t++) {
        int cur = t & 1;
        bool more = (t + 1 < tiles);
        if (more) load_tile(t + 1);   /* HBM -> regs, overlaps the MFMAs */
        compute(cur);
        if (more) store_tile(1 - cur);
        __syncthreads();
    }

    size_t crow0 = (size_t)tm * BM + wm * 64;
    size_t ccol0 = (size_t)tn * BN + wn * 64;
    #pragma unroll
    for (int i = 0; i < 4; i++)
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            size_t col = ccol0 + j * 16 + (lane & 15);
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                size_t row = crow0 + i * 16 + (lane >> 4) * 4 + r;
                C[row * N + col] = (bf16)acc[i][j][r];
            }
        }

    if (!publish) return;
    int band = (int)(crow0 * (size_t)nparts / M);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t prev = __hip_atomic_fetch_add(&band_cnt[band], 1,
                                               __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_SYSTEM);
        if (prev == (uint32_t)blocks_per_band - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            MPIX_Pready(band, dpreq);
        }
    }
}

#else /* variants 1 and 2 */
__global__ __launch_bounds__(256)
void gemm_bf16_pready(const bf16 *__restrict__ A, const bf16 *__restrict__ B,
                      bf16 *__restrict__ C, int M, int N, int K,
                      uint32_t *band_cnt, int nparts, int blocks_per_band,
                      void *dpreq, int publish)
{
/* LDS row pitch: BK+8 makes every frag ds_read_b128 bank-conflict-free
 * (rows in a 16-lane service group land on 4 distinct 64-B bank rows
 * instead of 1; measured 4.0e9 SQ_LDS_BANK_CONFLICT cycles at pitch BK). */
#define LP (BK + 8)
    __shared__ bf16 lds[BM * LP + BN * LP];
    bf16 *As = lds;            /* [BM][LP] */
#if MPIX_GEMM_VARIANT == 2
    bf16 *Bs = lds + BM * LP;  /* [BK][BN+8] row-major (no transpose pass) */
#else
    bf16 *Bt = lds + BM * LP;  /* [BN][LP] (transposed B tile) */
#endif

    /* XCD-aware swizzle: consecutive XCDs get consecutive tile columns so
     * each XCD's L2 sees a contiguous band of B (guide T1, bijective). */
    int nwg = gridDim.x;
    int wg = blockIdx.x;
    {
        int q = nwg / 8, r = nwg % 8, xcd = wg % 8;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + wg / 8;
    }
    int tiles_n = N / BN;
    int tm = wg / tiles_n, tn = wg % tiles_n;

    int tid = threadIdx.x;
    int wave = tid >> 6, lane = tid & 63;
    int wm = wave >> 1, wn = wave & 1;          /* 2x2 wave grid */
    int lrow = lane & 15, lk8 = (lane >> 4) * 8;

    frag4f acc[4][4] = {};

    const bf16 *Ab = A + (size_t)tm * BM * K;
    const bf16 *Bb = B + tn * BN;

    for (int k0 = 0; k0 < K; k0 += BK) {
        /* stage A tile: 256 threads x 8 bf16 = 4096 per pass, 2 passes */
        {
            const bf16 *src = Ab + k0;
            for (int p = 0; p < 2; p++) {
                int idx = (p * 256 + tid) * 8;       /* element offset */
                int row = idx / BK, col = idx % BK;
                *(frag8 *)&As[row * LP + col] =
                    *(const frag8 *)&src[(size_t)row * K + col];
            }
        }
        /* stage B tile */
        {
            const bf16 *src = Bb + (size_t)k0 * N;
            for (int p = 0; p < 2; p++) {
                int idx = (p * 256 + tid) * 8;
                int k = idx / BN, n = idx % BN;
#if MPIX_GEMM_VARIANT == 2
                /* row-major image, coalesced contiguous 16-B writes */
                *(frag8 *)&Bs[k * (BN + 8) + n] =
                    *(const frag8 *)&src[(size_t)k * N + n];
#else
                /* transpose scatter (2-byte writes) */
                frag8 v = *(const frag8 *)&src[(size_t)k * N + n];
                #pragma unroll
                for (int j = 0; j < 8; j++)
                    Bt[(n + j) * LP + k] = ((const bf16 *)&v)[j];
#endif
            }
        }
        __syncthreads();
        /* 4x4 quadrant of 16x16 tiles, two K=32 halves... BK=32 = one K */
        frag8 af[4], bf[4];
        #pragma unroll
        for (int i = 0; i < 4; i++) {
            int row = wm * 64 + i * 16 + lrow;
            af[i] = *(const frag8 *)&As[row * LP + lk8];
        }
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            int col = wn * 64 + j * 16 + lrow;
#if MPIX_GEMM_VARIANT == 2
            /* gather 8 ks of one column from the row-major image */
            #pragma unroll
            for (int e = 0; e < 8; e++)
                ((bf16 *)&bf[j])[e] = Bs[(lk8 + e) * (BN + 8) + col];
#else
            bf[j] = *(const frag8 *)&Bt[col * LP + lk8];
#endif
        }
        #pragma unroll
        for (int i = 0; i < 4; i++)
            #pragma unroll
            for (int j = 0; j < 4; j++)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    af[i], bf[j], acc[i][j], 0, 0, 0);
        __syncthreads();
    }

    /* epilogue: fp32 acc -> bf16 C.  Lane l of tile (i,j) holds C rows
     * (l>>4)*4 + r, col l&15 (C/D map col=lane&15, row=(lane>>4)*4+reg). */
    size_t crow0 = (size_t)tm * BM + wm * 64;
    size_t ccol0 = (size_t)tn * BN + wn * 64;
    #pragma unroll
    for (int i = 0; i < 4; i++)
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            size_t col = ccol0 + j * 16 + (lane & 15);
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                size_t row = crow0 + i * 16 + (lane >> 4) * 4 + r;
                C[row * N + col] = (bf16)acc[i][j][r];
            }
        }

    if (!publish) return;

    /* ---- publish the band when this is its last finishing workgroup ---- */
    int band = (int)(crow0 * (size_t)nparts / M); /* band of this tile's rows */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_last;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t prev = __hip_atomic_fetch_add(&band_cnt[band], 1,
                                               __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_SYSTEM);
        s_last = (prev == (uint32_t)blocks_per_band - 1);
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            MPIX_Pready(band, dpreq);
        }
    }
}

#endif /* MPIX_GEMM_VARIANT */

#if MPIX_GEMM_VARIANT >= 4
#define GEMM_THREADS V4_THREADS
#else
#define GEMM_THREADS 256
#endif

/* ---------------------------------------------------- payload verification
 * Sampled end-to-end check of the RECEIVED buffer in timed mode (not just
 * --check of the GEMM): every VERIFY_EVERY iterations the receiver's Crecv
 * partitions are poisoned before Start, then after the waits an xor
 * checksum of Crecv is compared against the checksum of the left rank's C
 * (exchanged over MPI).  A stale/skipped transfer leaves the poison words
 * in place and fails the compare; corrupt data fails it outright. */
#define VERIFY_EVERY 4

__global__ void k_xorsum(const uint32_t *p, size_t n_words,
                         unsigned long long *out)
{
    __shared__ unsigned long long blk;
    if (threadIdx.x == 0) blk = 0;
    __syncthreads();
    unsigned long long acc = 0;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n_words; i += stride)
        /* fold the word index in so permuted data doesn't cancel out */
        acc ^= (unsigned long long)p[i] * 2654435761ull + i;
    atomicXor(&blk, acc);
    __syncthreads();
    if (threadIdx.x == 0) atomicXor(out, blk);
}

__global__ void k_poison(uint32_t *buf, int nparts, size_t part_words)
{
    int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p < nparts) buf[(size_t)p * part_words] = 0xDEADBEEFu;
}

/* -------------------------------------------------------------- --check
 * The kernel against the float64 reference of gemm_check.h, in both data
 * modes (unit only while K <= 256, where it is bit-exact).
 *
 * A and B sit inside larger allocations whose guard regions (one tile row
 * before and after) hold bf16 NaN: a K-tile or a tile row read past the end
 * poisons the result.  C and Crecv sit between sentinel guards that must
 * survive, and both are filled with NaN before every launch.
 *
 * Pass A launches with publish = 0 and checks all of C.  Pass B launches
 * with publish = 1 and sends C as nparts bands to the right neighbour (the
 * process itself when alone) through the same requests as the timed mode:
 * C is checked again, Crecv must be byte-identical to the sender's C (a band
 * published before its last tile was stored arrives with NaN in it), and
 * every band counter must stand at blocks_per_band.  With several ranks the
 * receiver also regenerates the left rank's inputs from its seed and checks
 * Crecv against that reference.
 *
 * One JSON line per pass and mode; returns the number of failed passes. */
static bool all_equal(const uint16_t *p, size_t n, uint16_t v)
{
    for (size_t i = 0; i < n; i++)
        if (p[i] != v) return false;
    return true;
}

static int run_check(int rank, int size, int M, int N, int K, int nparts)
{
    namespace gc = gemm_check;
    const uint16_t SENTINEL = 0xA5A5u;
    int right = (rank + 1) % size, left = (rank - 1 + size) % size;
    int blocks_per_band = (M / nparts / BM) * (N / BN);
    int grid = (M / BM) * (N / BN);

    size_t an = (size_t)M * K, bn = (size_t)K * N, cn = (size_t)M * N;
    size_t ga = (size_t)BM * K; /* guards: one tile row of each operand */
#if MPIX_GEMM_VARIANT >= 4
    size_t gb = (size_t)BN * K;
#else
    size_t gb = (size_t)BK * N;
#endif
    size_t gcn = (size_t)BM * N;
    uint16_t *Aall, *Ball, *Call, *Rall;
    HIP(hipMalloc(&Aall, (an + 2 * ga) * sizeof(uint16_t)));
    HIP(hipMalloc(&Ball, (bn + 2 * gb) * sizeof(uint16_t)));
    HIP(hipMalloc(&Call, (cn + 2 * gcn) * sizeof(uint16_t)));
    HIP(hipMalloc(&Rall, (cn + 2 * gcn) * sizeof(uint16_t)));
    HIP(hipMemset(Aall, 0xFF, (an + 2 * ga) * sizeof(uint16_t)));
    HIP(hipMemset(Ball, 0xFF, (bn + 2 * gb) * sizeof(uint16_t)));
    HIP(hipMemset(Call, 0xA5, (cn + 2 * gcn) * sizeof(uint16_t)));
    HIP(hipMemset(Rall, 0xA5, (cn + 2 * gcn) * sizeof(uint16_t)));
    bf16 *A = (bf16 *)(Aall + ga), *B = (bf16 *)(Ball + gb);
    bf16 *C = (bf16 *)(Call + gcn), *Crecv = (bf16 *)(Rall + gcn);
    uint32_t *band_cnt;
    HIP(hipMalloc(&band_cnt, nparts * sizeof(uint32_t)));
    hipStream_t st;
    HIP(hipStreamCreate(&st));

    MPIX_Request ps, pr;
    int count = (int)(cn / nparts);
    CHECK(MPIX_Psend_init(C, nparts, count, MPI_SHORT, right, 21,
                          MPI_COMM_WORLD, MPI_INFO_NULL, &ps) == 0);
    CHECK(MPIX_Precv_init(Crecv, nparts, count, MPI_SHORT, left, 21,
                          MPI_COMM_WORLD, MPI_INFO_NULL, &pr) == 0);
    MPIX_Prequest dps;
    CHECK(MPIX_Prequest_create(ps, &dps) == 0);

    std::vector<uint16_t> hA(an), hBt(bn), hB, hC(cn + 2 * gcn),
        hR(cn + 2 * gcn), leftC(cn);
    std::vector<uint32_t> hcnt(nparts);
    gc::Reference ref, ref_left;
    int failed = 0;

    for (gc::Mode mode : {gc::UNIT, gc::UNIFORM}) {
        if (mode == gc::UNIT && K > 256) continue;
        if (size > 1) {
            gc::fill(mode, 12345 + left, gc::OP_A, M, K, hA.data());
            gc::fill(mode, 12345 + left, gc::OP_B, N, K, hBt.data());
            gc::reference(hA.data(), hBt.data(), M, N, K, ref_left);
        }
        gc::fill(mode, 12345 + rank, gc::OP_A, M, K, hA.data());
        gc::fill(mode, 12345 + rank, gc::OP_B, N, K, hBt.data());
        gc::reference(hA.data(), hBt.data(), M, N, K, ref);
        HIP(hipMemcpy(A, hA.data(), an * sizeof(uint16_t),
                      hipMemcpyHostToDevice));
#if MPIX_GEMM_VARIANT >= 4
        /* the kernel takes B pre-transposed [N][K], as generated */
        HIP(hipMemcpy(B, hBt.data(), bn * sizeof(uint16_t),
                      hipMemcpyHostToDevice));
#else
        hB.resize(bn);
        for (int n = 0; n < N; n++)
            for (int k = 0; k < K; k++)
                hB[(size_t)k * N + n] = hBt[(size_t)n * K + k];
        HIP(hipMemcpy(B, hB.data(), bn * sizeof(uint16_t),
                      hipMemcpyHostToDevice));
#endif

        for (int publish = 0; publish <= 1; publish++) {
            HIP(hipMemset(C, 0xFF, cn * sizeof(uint16_t)));
            HIP(hipMemset(Crecv, 0xFF, cn * sizeof(uint16_t)));
            HIP(hipMemset(band_cnt, 0, nparts * sizeof(uint32_t)));
            HIP(hipDeviceSynchronize());
            MPI_Barrier(MPI_COMM_WORLD);
            if (publish) {
                MPIX_Request act[2] = {pr, ps};
                CHECK(MPIX_Startall(2, act) == 0);
            }
            hipLaunchKernelGGL(gemm_bf16_pready, dim3(grid),
                               dim3(GEMM_THREADS), 0, st, A, B, C, M, N, K,
                               band_cnt, nparts, blocks_per_band,
                               publish ? dps : nullptr, publish);
            HIP(hipGetLastError());
            HIP(hipStreamSynchronize(st));
            if (publish) {
                /* the kernel is over: a band whose counter is short now was
                 * never published, and a wait for it would never return */
                HIP(hipMemcpy(hcnt.data(), band_cnt,
                              nparts * sizeof(uint32_t),
                              hipMemcpyDeviceToHost));
                for (int b = 0; b < nparts; b++)
                    if (hcnt[b] != (uint32_t)blocks_per_band) {
                        printf("{\"check\": \"gemm_pready\", \"variant\": "
                               "%d, \"rank\": %d, \"pass\": \"B\", \"mode\": "
                               "\"%s\", \"mnk\": [%d, %d, %d], \"nparts\": "
                               "%d, \"bands_ok\": false, \"ok\": false}\n",
                               MPIX_GEMM_VARIANT, rank, gc::mode_name(mode),
                               M, N, K, nparts);
                        fflush(stdout);
                        fprintf(stderr, "[r%d] band_cnt[%d] = %u after the "
                                "kernel, want %d: band not published, not "
                                "waiting for it\n", rank, b, hcnt[b],
                                blocks_per_band);
                        MPI_Abort(MPI_COMM_WORLD, 1);
                    }
                CHECK(MPIX_Wait(&pr, MPI_STATUS_IGNORE) == 0);
                CHECK(MPIX_Wait(&ps, MPI_STATUS_IGNORE) == 0);
            }
            HIP(hipMemcpy(hC.data(), Call, hC.size() * sizeof(uint16_t),
                          hipMemcpyDeviceToHost));
            HIP(hipMemcpy(hR.data(), Rall, hR.size() * sizeof(uint16_t),
                          hipMemcpyDeviceToHost));
            HIP(hipMemcpy(hcnt.data(), band_cnt, nparts * sizeof(uint32_t),
                          hipMemcpyDeviceToHost));
            const uint16_t *c = hC.data() + gcn, *r = hR.data() + gcn;

            gc::Result res = gc::compare(mode, c, ref), res_recv;
            bool guards = all_equal(hC.data(), gcn, SENTINEL) &&
                          all_equal(c + cn, gcn, SENTINEL) &&
                          all_equal(hR.data(), gcn, SENTINEL) &&
                          all_equal(r + cn, gcn, SENTINEL);
            bool bands = true, identical = true;
            for (int b = 0; b < nparts; b++)
                bands = bands &&
                        hcnt[b] == (publish ? (uint32_t)blocks_per_band : 0u);
            if (publish) {
                /* the sender's C, byte for byte */
                const uint16_t *sent = c;
                if (size > 1) {
                    MPI_Sendrecv(c, (int)cn, MPI_UINT16_T, right, 78,
                                 leftC.data(), (int)cn, MPI_UINT16_T, left,
                                 78, MPI_COMM_WORLD, MPI_STATUS_IGNORE);
                    sent = leftC.data();
                }
                identical = memcmp(r, sent, cn * sizeof(uint16_t)) == 0;
                res_recv = gc::compare(mode, r, size > 1 ? ref_left : ref);
            } else {
                /* nothing was sent: Crecv is still all poison */
                identical = all_equal(r, cn, gc::BF16_POISON);
            }
            bool ok = res.ok() && res_recv.ok() && guards && bands &&
                      identical;
            if (!ok) failed++;
            char first[64] = "null", first_recv[64] = "null";
            if (res.bad)
                snprintf(first, sizeof first, "[%ld, %ld]", res.first_row,
                         res.first_col);
            if (res_recv.bad)
                snprintf(first_recv, sizeof first_recv, "[%ld, %ld]",
                         res_recv.first_row, res_recv.first_col);
            printf("{\"check\": \"gemm_pready\", \"variant\": %d, "
                   "\"rank\": %d, \"ranks\": %d, \"pass\": \"%s\", "
                   "\"mode\": \"%s\", \"mnk\": [%d, %d, %d], \"nparts\": %d, "
                   "\"grid\": %d, \"refused\": %s, \"bad\": %zu, "
                   "\"worst\": %.6g, \"first_bad\": %s, \"recv_bad\": %zu, "
                   "\"recv_worst\": %.6g, \"recv_first_bad\": %s, "
                   "\"recv_identical\": %s, \"bands_ok\": %s, "
                   "\"guards_ok\": %s, \"ok\": %s}\n",
                   MPIX_GEMM_VARIANT, rank, size, publish ? "B" : "A",
                   gc::mode_name(mode), M, N, K, nparts, grid,
                   res.refused || res_recv.refused ? "true" : "false",
                   res.bad, gc::json_num(res.worst), first, res_recv.bad,
                   gc::json_num(res_recv.worst), first_recv,
                   identical ? "true" : "false", bands ? "true" : "false",
                   guards ? "true" : "false", ok ? "true" : "false");
            fflush(stdout);
            if (res.bad)
                fprintf(stderr, "[r%d] pass %s %s: first bad of C: %s\n",
                        rank, publish ? "B" : "A", gc::mode_name(mode),
                        gc::address(res).c_str());
            if (res_recv.bad)
                fprintf(stderr, "[r%d] pass %s %s: first bad of Crecv: %s\n",
                        rank, publish ? "B" : "A", gc::mode_name(mode),
                        gc::address(res_recv).c_str());
            if (!bands)
                for (int b = 0; b < nparts; b++)
                    fprintf(stderr, "[r%d] band_cnt[%d] = %u, want %d\n",
                            rank, b, hcnt[b],
                            publish ? blocks_per_band : 0);
        }
    }

    CHECK(MPIX_Prequest_free(&dps) == 0);
    CHECK(MPIX_Request_free(&ps) == 0);
    CHECK(MPIX_Request_free(&pr) == 0);
    (void)hipFree(Aall); (void)hipFree(Ball); (void)hipFree(Call);
    (void)hipFree(Rall); (void)hipFree(band_cnt);
    (void)hipStreamDestroy(st);
    printf("[r%d] gemm --check M=%d N=%d K=%d nparts=%d -> %s\n", rank, M, N,
           K, nparts, failed ? "FAIL" : "PASS");
    return failed;
}

int main(int argc, char **argv)
{
    int provided, rank, size;
    MPI_Init_thread(&argc, &argv, MPI_THREAD_MULTIPLE, &provided);
    MPI_Comm_rank(MPI_COMM_WORLD, &rank);
    MPI_Comm_size(MPI_COMM_WORLD, &size);

    /* --check [M N K [nparts]]; bare --check is 256 256 512, one band per
     * tile row */
    bool check = argc > 1 && strcmp(argv[1], "--check") == 0;
    bool shaped = check && argc > 4;
    int M = check ? 256 : (argc > 1 ? atoi(argv[1]) : 8192);
    int N = check ? 256 : (argc > 2 ? atoi(argv[2]) : 8192);
    int K = check ? 512 : (argc > 3 ? atoi(argv[3]) : 8192);
    if (shaped) {
        M = atoi(argv[2]);
        N = atoi(argv[3]);
        K = atoi(argv[4]);
    }
    int iters = check ? 1 : (argc > 4 ? atoi(argv[4]) : 10);
    int warmup = check ? 0 : 3;

    /* the shape is judged before anything touches the device */
    CHECK(M > 0 && N > 0 && K > 0);
    CHECK(M % BM == 0 && N % BN == 0 && K % BK == 0);
    /* one band >= one tile row; clamp so small M still works */
    int nparts = check ? (argc > 5 ? atoi(argv[5]) : M / BM)
                       : (M / BM < NPARTS ? M / BM : NPARTS);
#if MPIX_GEMM_VARIANT == 6
    /* 8-phase pair schedule: K-tiles are computed in pairs, and the
     * prologue has six pieces of tiles 0 and 1 in flight for a first
     * iteration that is followed by another */
    CHECK(K % (2 * BK) == 0 && K >= 4 * BK);
#endif
    CHECK(nparts >= 1 && M % nparts == 0 && (M / nparts) % BM == 0);
    int blocks_per_band = (M / nparts / BM) * (N / BN);

    int ndev = 0;
    HIP(hipGetDeviceCount(&ndev));
    CHECK(ndev > 0);
    HIP(hipSetDevice(rank % ndev));
    CHECK(MPIX_Init() == 0);
    int right = (rank + 1) % size, left = (rank - 1 + size) % size;

    if (check) {
        int failed = run_check(rank, size, M, N, K, nparts);
        MPIX_Finalize();
        MPI_Finalize();
        return failed ? 1 : 0;
    }

    size_t an = (size_t)M * K, bn = (size_t)K * N, cn = (size_t)M * N;
    bf16 *A, *B, *C, *Crecv;
    HIP(hipMalloc(&A, an * sizeof(bf16)));
    HIP(hipMalloc(&B, bn * sizeof(bf16)));
    HIP(hipMalloc(&C, cn * sizeof(bf16)));
    HIP(hipMalloc(&Crecv, cn * sizeof(bf16)));
    uint32_t *band_cnt;
    HIP(hipMalloc(&band_cnt, nparts * sizeof(uint32_t)));

    /* fill A/B host-side: bounded pseudo-random bf16 in [-1, 1) */
    {
        std::vector<bf16> h(an);
        unsigned s = 12345 + rank;
        for (size_t i = 0; i < an; i++) {
            s = s * 1664525u + 1013904223u;
            h[i] = (bf16)(((float)(s >> 8) / (float)(1 << 24)) * 2.f - 1.f);
        }
        HIP(hipMemcpy(A, h.data(), an * sizeof(bf16), hipMemcpyHostToDevice));
        h.resize(bn);
        for (size_t i = 0; i < bn; i++) {
            s = s * 1664525u + 1013904223u;
            /* asymmetric B (guide: catches row/col-swapped C writes) */
            h[i] = (bf16)(((float)(s >> 8) / (float)(1 << 24)) * 2.f - 1.f);
        }
        HIP(hipMemcpy(B, h.data(), bn * sizeof(bf16), hipMemcpyHostToDevice));
    }

    hipStream_t st;
    HIP(hipStreamCreate(&st));
    int grid = (M / BM) * (N / BN);

    MPIX_Request ps, pr;
    int count = (int)(cn / nparts);
    CHECK(MPIX_Psend_init(C, nparts, count, MPI_SHORT, right, 21,
                          MPI_COMM_WORLD, MPI_INFO_NULL, &ps) == 0);
    CHECK(MPIX_Precv_init(Crecv, nparts, count, MPI_SHORT, left, 21,
                          MPI_COMM_WORLD, MPI_INFO_NULL, &pr) == 0);
    MPIX_Prequest dps;
    CHECK(MPIX_Prequest_create(ps, &dps) == 0);

    unsigned long long *d_sum; /* [0]=xorsum(C), [1]=xorsum(Crecv) */
    HIP(hipMalloc(&d_sum, 2 * sizeof(unsigned long long)));
    size_t sum_words = cn * sizeof(bf16) / 4;
    size_t part_words = sum_words / nparts;

    auto run = [&](bool overlap) {
        auto one = [&](int it) {
            bool verify = (it % VERIFY_EVERY) == 0;
            if (verify) {
                hipLaunchKernelGGL(k_poison, dim3(1), dim3(64), 0, st,
                                   (uint32_t *)Crecv, nparts, part_words);
                HIP(hipStreamSynchronize(st)); /* land before the pull */
            }
            MPIX_Request act[2] = {pr, ps};
            CHECK(MPIX_Startall(2, act) == 0);
            HIP(hipMemsetAsync(band_cnt, 0, nparts * sizeof(uint32_t), st));
            if (overlap) {
                hipLaunchKernelGGL(gemm_bf16_pready, dim3(grid), dim3(GEMM_THREADS),
                                   0, st, A, B, C, M, N, K, band_cnt, nparts,
                                   blocks_per_band, dps, 1);
                HIP(hipStreamSynchronize(st));
            } else {
                hipLaunchKernelGGL(gemm_bf16_pready, dim3(grid), dim3(GEMM_THREADS),
                                   0, st, A, B, C, M, N, K, band_cnt, nparts,
                                   blocks_per_band, nullptr, 0);
                HIP(hipStreamSynchronize(st));
                for (int p = 0; p < nparts; p++)
                    CHECK(MPIX_Pready(p, ps) == 0);
            }
            CHECK(MPIX_Wait(&pr, MPI_STATUS_IGNORE) == 0);
            CHECK(MPIX_Wait(&ps, MPI_STATUS_IGNORE) == 0);
            if (verify) {
                HIP(hipMemsetAsync(d_sum, 0, 2 * sizeof(unsigned long long),
                                   st));
                hipLaunchKernelGGL(k_xorsum, dim3(256), dim3(256), 0, st,
                                   (const uint32_t *)C, sum_words, d_sum);
                hipLaunchKernelGGL(k_xorsum, dim3(256), dim3(256), 0, st,
                                   (const uint32_t *)Crecv, sum_words,
                                   d_sum + 1);
                unsigned long long h[2], left_sum = 0;
                HIP(hipMemcpy(h, d_sum, sizeof(h), hipMemcpyDeviceToHost));
                MPI_Sendrecv(&h[0], 1, MPI_UNSIGNED_LONG_LONG, right, 77,
                             &left_sum, 1, MPI_UNSIGNED_LONG_LONG, left, 77,
                             MPI_COMM_WORLD, MPI_STATUS_IGNORE);
                if (left_sum != h[1]) {
                    fprintf(stderr, "[r%d] VERIFY FAIL iter %d: Crecv xorsum "
                            "%016llx != sender C %016llx (overlap=%d)\n",
                            rank, it, h[1], left_sum, (int)overlap);
                    MPI_Abort(MPI_COMM_WORLD, 2);
                }
            }
        };
        for (int i = 0; i < warmup; i++) one(i);
        HIP(hipDeviceSynchronize());
        MPI_Barrier(MPI_COMM_WORLD);
        auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < iters; i++) one(i);
        MPI_Barrier(MPI_COMM_WORLD);
        double dt = std::chrono::duration<double>(
                        std::chrono::steady_clock::now() - t0).count();
        double mx;
        MPI_Allreduce(&dt, &mx, 1, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
        return mx / iters;
    };

    /* GEMM-only reference time (no send) for TFLOP/s */
    auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < iters; i++) {
        hipLaunchKernelGGL(gemm_bf16_pready, dim3(grid), dim3(GEMM_THREADS), 0, st,
                           A, B, C, M, N, K, band_cnt, nparts, blocks_per_band,
                           nullptr, 0);
    }
    HIP(hipStreamSynchronize(st));
    double t_gemm = std::chrono::duration<double>(
                        std::chrono::steady_clock::now() - t0).count() / iters;

    double t_overlap = run(true);
    double t_serial = run(false);

    if (rank == 0) {
        double tf = 2.0 * M * N * K / t_gemm / 1e12;
        printf("{\"bench\": \"gemm_pready\", \"ranks\": %d, "
               "\"mnk\": [%d,%d,%d], \"nparts\": %d, "
               "\"gemm_tflops\": %.1f, \"ms_gemm\": %.3f, "
               "\"ms_overlap\": %.3f, \"ms_serial\": %.3f, "
               "\"overlap_speedup\": %.4f, \"c_bytes\": %zu}\n",
               size, M, N, K, nparts, tf, t_gemm * 1e3, t_overlap * 1e3,
               t_serial * 1e3, t_serial / t_overlap, cn * sizeof(bf16));
    }

    CHECK(MPIX_Prequest_free(&dps) == 0);
    CHECK(MPIX_Request_free(&ps) == 0);
    CHECK(MPIX_Request_free(&pr) == 0);
    (void)hipFree(A); (void)hipFree(B); (void)hipFree(C);
    (void)hipFree(Crecv); (void)hipFree(band_cnt); (void)hipFree(d_sum);
    (void)hipStreamDestroy(st);
    MPIX_Finalize();
    MPI_Finalize();
    return 0;
}
