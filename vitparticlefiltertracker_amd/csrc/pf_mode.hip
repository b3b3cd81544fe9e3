// Mode estimate (SPEC S17): the local weighted mean of the posterior's densest cluster, beside SPEC S6's mean.
//
// k_mode_density is the all-pairs pass, D_i = sum_j Q_j in(i, j) with in(i, j) = |x_i - x_j| <= hx and |y_i - y_j| <= hy
// (one rounded fp32 subtraction per axis; false for anything NaN). The grid is seed blocks x j-chunks: a workgroup of
// 256 lanes keeps MODE_SEEDS seeds' (x, y) per lane in registers and walks its chunk in LDS tiles of MODE_TILE
// (x_j, y_j, Q_j) entries, every lane reading the same entry (an LDS broadcast), summing int64 partials in registers;
// one 64-bit integer atomic per seed and chunk adds them to dens (zeroed by a memset node ahead of the launch), and a
// zero partial (a chunk with nothing in the seed's window: most of them) adds nothing. The sum is an integer, so the
// grid, the tiling and the atomics' arrival order change no bit. A seed or an entry past P is (NaN, NaN): in no window.
// k_mode_pick_sum is one workgroup: the arg-max (largest D, smallest index), then pf_tree.h's stats_tree with the
// weight Q_j in(i*, j), once over x | y | s and once over the extra rows. A particle outside the window contributes
// +0 to every row, whatever its state holds, so a non-finite x or y never reaches a sum.
// Both kernels take the frame's decision from the statistics block the estimate + resample call has written on the
// same stream (T at [0]; with `gate`, held at [7]): every weight counts as 1 when T == 0 or the frame is held.
#pragma clang fp contract(off)
#include <cmath>
#include "vpf_common.h"
#include "../../include/vpf.h"
#include "pf_tree.h"

using namespace vpf;

constexpr int MODE_BLOCK = 256;                        // lanes of a density workgroup
constexpr int MODE_SEEDS = 2;                          // seeds per lane
constexpr int MODE_SEED_BLOCK = MODE_BLOCK * MODE_SEEDS;
constexpr int MODE_TILE = 128;                         // (x_j, y_j, Q_j) entries of one LDS tile
constexpr int MODE_GRID = 512;                         // workgroups the j-chunking aims for (two per CU)

struct alignas(16) Jxyq { float x, y; int64_t q; };

__device__ __forceinline__ bool mode_uniform(const int64_t* __restrict__ stats, int gate) {
    return stats[0] == 0 || (gate != 0 && stats[7] != 0);
}

__device__ __forceinline__ bool in_window(float xa, float ya, float xb, float yb, float hx, float hy) {
    return fabsf(xa - xb) <= hx && fabsf(ya - yb) <= hy;
}

__global__ __launch_bounds__(MODE_BLOCK) void k_mode_density(GlobalView g, int64_t P, int tiles_per_chunk, float hx,
                                                             float hy, const int64_t* __restrict__ stats, int gate,
                                                             int64_t* __restrict__ dens) {
    __shared__ Jxyq tile[MODE_TILE];
    const int t = threadIdx.x;
    const bool uni = mode_uniform(stats, gate);
    int64_t seed[MODE_SEEDS], d[MODE_SEEDS];
    float xi[MODE_SEEDS], yi[MODE_SEEDS];
#pragma unroll
    for (int e = 0; e < MODE_SEEDS; ++e) {
        seed[e] = (int64_t)blockIdx.x * MODE_SEED_BLOCK + e * MODE_BLOCK + t;
        d[e] = 0;
        xi[e] = yi[e] = __builtin_nanf("");
        if (seed[e] < P) {
            const float* st = g.state((uint32_t)seed[e]);
            xi[e] = st[0]; yi[e] = st[g.ld];
        }
    }
    const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_chunk;
    for (int k = 0; k < tiles_per_chunk; ++k) {
        const int64_t j0 = (tile0 + k) * MODE_TILE;
        if (j0 >= P) break;                 // the same for every lane of the workgroup
        __syncthreads();                    // the previous tile has been read
        if (t < MODE_TILE) {
            const int64_t j = j0 + t;
            Jxyq v{__builtin_nanf(""), __builtin_nanf(""), 0};
            if (j < P) {
                const float* st = g.state((uint32_t)j);
                v.x = st[0]; v.y = st[g.ld];
                v.q = uni ? (int64_t)1 : g.q((uint32_t)j);
            }
            tile[t] = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int jj = 0; jj < MODE_TILE; ++jj) {
            const Jxyq v = tile[jj];
#pragma unroll
            for (int e = 0; e < MODE_SEEDS; ++e)
                d[e] += in_window(xi[e], yi[e], v.x, v.y, hx, hy) ? v.q : (int64_t)0;
        }
    }
#pragma unroll
    for (int e = 0; e < MODE_SEEDS; ++e)
        if (seed[e] < P && d[e] != 0)
            atomicAdd((unsigned long long*)(dens + seed[e]), (unsigned long long)d[e]);
}

__global__ __launch_bounds__(1024) void k_mode_pick_sum(GlobalView g, int64_t P, int n_extra, float hx, float hy,
                                                        const int64_t* __restrict__ stats, int gate,
                                                        const int64_t* __restrict__ dens, int64_t* __restrict__ out) {
    const int t = threadIdx.x;
    const bool uni = mode_uniform(stats, gate);
    // i* = min{i : D_i = max D}: a lane's own indices ascend, so `>` keeps its smallest; lanes then halve pairwise
    int64_t bd = -1, bi = 0;                // D_i >= 0: a lane without an index never wins
    for (int64_t i = t; i < P; i += 1024) {
        const int64_t di = dens[i];
        if (di > bd) { bd = di; bi = i; }
    }
    smx[t] = bd; sT[t] = bi;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) {
            const int64_t d2 = smx[t + o], i2 = sT[t + o];
            if (d2 > smx[t] || (d2 == smx[t] && i2 < sT[t])) { smx[t] = d2; sT[t] = i2; }
        }
        __syncthreads();
    }
    const int64_t istar = sT[0];
    __syncthreads();                        // every lane has read sT[0] before the tree rewrites it
    const float* ss = g.state((uint32_t)istar);
    const float xs = ss[0], ys = ss[g.ld];
    for (int pass = 0; pass < 2; ++pass) {
        const int n_rows = pass == 0 ? 3 : n_extra;
        if (n_rows > 0) {
            stats_tree<false>(P, false, [=](int64_t i) {
                const float* r = g.state((uint32_t)i);
                if (!in_window(xs, ys, r[0], r[g.ld], hx, hy)) return Wxys{0, 0.0f, 0.0f, 0.0f};
                r += (int64_t)(3 * pass) * g.ld;
                return Wxys{uni ? (int64_t)1 : g.q((uint32_t)i), r[0], n_rows > 1 ? r[g.ld] : 0.0f,
                            n_rows > 2 ? r[2 * g.ld] : 0.0f};
            });
        }
        if (t == 0) {
            int64_t* o = out + 2 + 3 * pass;
            if (pass == 0) { out[0] = istar; out[1] = sT[0]; }
            o[0] = n_rows > 0 ? __double_as_longlong(sx[0]) : 0;
            o[1] = n_rows > 1 ? __double_as_longlong(sy[0]) : 0;
            o[2] = n_rows > 2 ? __double_as_longlong(sz[0]) : 0;
        }
        __syncthreads();                    // lane 0 has read the tree before the second pass rewrites it
    }
}

VPF_API int vpf_mode_estimate(const int64_t* Q, int64_t q_stride, const float* particles, int64_t ld,
                              int64_t p_stride, int64_t n_shard, int64_t P, int n_extra, float hx, float hy,
                              const int64_t* stats, int gate, int64_t* dens_ws, int64_t* out, void* stream) {
    if (n_extra < 0 || n_extra > 3 || !rows_args_ok(ld, p_stride, n_shard, P, 3 + n_extra, 6) ||
        (P > n_shard && q_stride < n_shard) || !std::isfinite(hx) || !std::isfinite(hy) || hx < 0.0f || hy < 0.0f ||
        !Q || !particles || !stats || !dens_ws || !out)
        return VPF_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const GlobalView g{Q, q_stride, particles, ld, p_stride, (uint32_t)n_shard};
    // seed blocks x j-chunks: chunks of whole tiles, as many as bring the grid to MODE_GRID workgroups
    const int64_t seed_blocks = (P + MODE_SEED_BLOCK - 1) / MODE_SEED_BLOCK;
    const int64_t tiles = (P + MODE_TILE - 1) / MODE_TILE;
    const int64_t want = (MODE_GRID + seed_blocks - 1) / seed_blocks;
    const int64_t tiles_per_chunk = (tiles + (want < tiles ? want : tiles) - 1) / (want < tiles ? want : tiles);
    const int64_t chunks = (tiles + tiles_per_chunk - 1) / tiles_per_chunk;
    const hipError_t e = hipMemsetAsync(dens_ws, 0, (size_t)P * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_mode_density, dim3((unsigned)seed_blocks, (unsigned)chunks), dim3(MODE_BLOCK), 0, s, g, P,
                       (int)tiles_per_chunk, hx, hy, stats, gate, dens_ws);
    hipLaunchKernelGGL(k_mode_pick_sum, dim3(1), dim3(1024), 0, s, g, P, n_extra, hx, hy, stats, gate, dens_ws, out);
    VPF_RETURN_LAUNCH();
}
