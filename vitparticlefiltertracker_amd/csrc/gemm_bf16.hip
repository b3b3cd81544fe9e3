// bf16 GEMM with fused epilogues for the ViT encoder.
//
//   C[M][N] = epi( A[M][K] . W[N][K]^T ),  bf16 operands, fp32 accumulation on MFMA.
//
// Design (gfx950; MI355X_MICROARCH.md / cdna_hip_programming.md §5):
//  * 256x256 output tile, BK = 64, 512 threads = 8 waves laid out 2 (M) x 4 (N); each wave owns a
//    128 (M) x 64 (N) sub-tile = 8 x 4 fragments of v_mfma_f32_16x16x32_bf16 (128 accumulator VGPRs).
//  * Operands are staged HBM/L2 -> LDS by global_load_lds_dwordx4 (LDS-DMA, 1 KiB per wave-instruction,
//    no VGPR round trip). Ring: 3 A K-tiles + 2 B K-tiles (5 x 32 KiB = the whole 160 KiB of LDS): the
//    activation panel (the operand that misses L2) is prefetched 2 K-tiles ahead, the L2-hot weights 1.
//    The LDS image is lane-linear; bank conflicts of the fragment reads (ds_read_b128) are removed by
//    XOR-swizzling the per-lane SOURCE address: 16-B chunk c of row r lives at physical chunk
//    c ^ ((r >> 1) & 7) (tools/lds_banks.py: conflict-free for every 16-lane group).
//  * One raw s_barrier per K-step behind a counted vmcnt (the next A K-tile stays in flight across it);
//    the refills are issued from the MFMA block: B(t+1)'s DMA right behind the fragment reads, A(t+2)'s four
//    issues interleaved into the 64 MFMAs per wave (one per 16), instead of 8 back-to-back issues after the
//    barrier while the MFMA pipes idle (QKV / proj / FC1 / FC2 -1.8..-4.5 %, profiles/r1_gemm_lab/ilv_ab.txt).
//  * MFMA operands are "swapped" (W fragment as A, activation fragment as B) so the accumulator holds
//    D[n][m]: each lane owns 4 consecutive output columns of one row. Epilogue (gemm_common.h): bias
//    (+ GELU, gelu_sig2) in fp32 on the accumulators, bf16 pack, 8-B writes into a per-wave XOR-swizzled
//    LDS image, then fully coalesced 16-B row stores (+ 16-B residual reads / position-embedding adds), and
//    optionally an MX-fp8 copy of the output (the A operand of the MX8 GEMMs, gemm_mx8.hip).
//  * Workgroup -> tile mapping is XCD-aware (bijective remap, cdna_hip_programming.md §5 T1): the blocks
//    that share an XCD walk consecutive tiles of one 256-row A panel, so the panel is an L2 hit.
#include <algorithm>
#include <atomic>
#include "gemm_common.h"

using namespace vpf;
using namespace vpf::gemm;

namespace {

constexpr int BK = 64;
constexpr int OPERAND_BYTES = BM * BK * 2;      // 32 KiB per operand tile
static_assert(OPERAND_BYTES == TILE_BYTES, "bf16 K-tile geometry");
// epilogue operands: bias (1 KiB) | colsum (1 KiB) | row statistics (up to AUX_PARTS planes of 2 KiB).
// 16 planes (D = 1024) do not fit next to bias / colsum: the deep ring then lands them in a second free A
// slot at the last K-step (wide path).
constexpr int AUX_PARTS = 15;
constexpr int MAX_PARTS = 16;
constexpr int AUX_BYTES = 2048 + AUX_PARTS * 2048;

// WIDE: LN-folded consumers of more than AUX_PARTS statistics planes (ViT-L: 16); the planes land in the second free
// A slot at the last K-step. OUT8: residual-stream producers that also write an MX-fp8 copy of their output.
// PART (vpf_gemm_bf16_splitk): blockIdx.y = split s of gridDim.y; the block runs K-tiles [s K/S, (s+1) K/S) and stores
// its raw fp32 accumulators to the partial plane s ((float*)C + s M N, row-major [M][N]) with no epilogue.
template <int EPI, bool WIDE = false, bool OUT8 = false, bool PART = false>
__global__ __launch_bounds__(NTHREADS) void k_gemm_bf16(const bf16_t* __restrict__ A, int lda,
                                                        const bf16_t* __restrict__ W,
                                                        const float* __restrict__ bias,
                                                        const bf16_t* residual,
                                                        const float* __restrict__ pos, int g2,
                                                        const float2* __restrict__ stats,
                                                        const float* __restrict__ colsum,
                                                        bf16_t* C, int ldc, int M, int N, int K, int group,
                                                        int stats_parts, float ln_eps, float* stats_out,
                                                        int stats_rows, Out8 o8) {
    // Deep ring: A ring of 3 K-tiles (A prefetched 2 K-tiles ahead: the activation panel is the operand that misses
    // L2), B ring of 2 (weights stay L2-hot); 5 x 32 KiB = all 160 KiB of LDS, and the epilogue operands go into the
    // A slot no K-tile uses any more (slot nk % 3, DMA'd at K-tile max(nk-2, 0)).
    constexpr int SMEM = 5 * OPERAND_BYTES;
    static_assert(AUX_BYTES <= OPERAND_BYTES, "aux region must fit the free A slot of the deep ring");
    __shared__ __attribute__((aligned(16))) char smem[SMEM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);

    int m0, n0;
    tile_of(M, N, group, m0, n0);   // XCD-aware grouped tile order (gemm_common.h)
    // the GELU epilogues store straight from the accumulators (store_wave_tile_direct: W rows permuted in the DMA)
    constexpr bool DIRECT = (EPI == VPF_EPI_LN_GELU || EPI == VPF_EPI_BIAS_GELU) && !OUT8 && !PART;

    // ---- per-lane DMA source offsets (bytes, relative to the block's panel base) ----
    const int kbase = PART ? (int)blockIdx.y * (K / (int)gridDim.y) : 0;   // PART: this split's first K column
    const char* Ablk = reinterpret_cast<const char*>(A) + (size_t)m0 * lda * 2 + (size_t)kbase * 2;
    const char* Bblk = reinterpret_cast<const char*>(W) + (size_t)n0 * K * 2 + (size_t)kbase * 2;
    uint32_t offA[4], offB[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int g = i * 8 + wid;                 // wave-instruction index: rows [8g, 8g+8)
        const int row = 8 * g + (lane >> 3);
        const int pch = lane & 7;
        const int lch = pch ^ ((row >> 1) & 7);    // logical chunk stored at this physical slot
        const int ra = min(row, M - 1 - m0);
        const int rb = min(DIRECT ? wperm(row) : row, N - 1 - n0);
        offA[i] = (uint32_t)ra * (uint32_t)(lda * 2) + (uint32_t)(lch * 16);
        offB[i] = (uint32_t)rb * (uint32_t)(K * 2) + (uint32_t)(lch * 16);
    }
    auto stage_a = [&](int kt) {   // A K-tile kt -> A slot kt % 3
        char* la = smem + (kt % 3) * OPERAND_BYTES;
        const uint32_t koff = (uint32_t)kt * (BK * 2);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((gptr_t)(Ablk + offA[i] + koff), (lptr_t)(la + (i * 8 + wid) * 1024), 16, 0, 0);
    };
    auto stage_b = [&](int kt) {   // B K-tile kt -> B slot kt & 1
        char* lb = smem + (3 + (kt & 1)) * OPERAND_BYTES;
        const uint32_t koff = (uint32_t)kt * (BK * 2);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((gptr_t)(Bblk + offB[i] + koff), (lptr_t)(lb + (i * 8 + wid) * 1024), 16, 0, 0);
    };

    const int wm = wid >> 2, wn = wid & 3;
    f32x4 acc[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment read addresses (byte offsets inside an operand tile), excluding the ks chunk term
    const int fr = lane & 15, fq = lane >> 4;

    // Epilogue operands ride the DMA stream into the aux region of LDS (gemm_common.h: bias | colsum | per-row
    // (mean, rstd) or statistics planes).
    constexpr bool LN = (EPI == VPF_EPI_LN || EPI == VPF_EPI_LN_GELU) && !PART;
    const int nk = (PART ? K / (int)gridDim.y : K) / BK;
    char* aux = smem + (nk % 3) * OPERAND_BYTES;
    constexpr bool wide = LN && WIDE;   // host: only for stats_parts > AUX_PARTS
    char* planes_lds = wide ? smem + ((nk + 1) % 3) * OPERAND_BYTES : aux + 2048;
    // The epilogue-operand DMAs re-read the lane id (opaque_lane): their per-lane addresses are then computed where they
    // are issued (once per tile) instead of being hoisted above the K loop, where they would stay live across it.
    auto load_planes = [&](char* dst) { dma_planes(dst, stats, stats_parts, m0, M, wid, opaque_lane()); };
    auto load_aux = [&]() {
        if constexpr (PART) return;   // no epilogue operands
        dma_bias_colsum<LN>(aux, bias, colsum, n0, N, wid, opaque_lane());
        if constexpr (LN && !wide) load_planes(aux + 2048);
    };
    stage_a(0);
    stage_b(0);
    if (nk > 1) stage_a(1);
    // At nk >= 2 the epilogue operands are issued at K-tile nk - 2 and the last K-step's vmcnt(0) + barrier retires
    // them; at nk == 1 (K = 64) that barrier is the loop's only one, so they go out with the prologue (issued
    // after it, the direct-store GELU epilogue read bias that waves 0 / 1 had not yet landed).
    if (nk == 1) load_aux();
    for (int kt = 0; kt < nk; ++kt) {
        // issue order: A0 B0 A1 | per K-tile t: B(t+1) A(t+2). A(kt), B(kt) are older than everything but A(kt+1)
        // (4 pieces per wave) until the last two K-tiles, where the tail is B / aux only.
        if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (nk >= 2 && kt == nk - 2) load_aux();
        if (wide && kt == nk - 1) load_planes(planes_lds);   // slot of A(nk-2): free after this barrier
        const char* la = smem + (kt % 3) * OPERAND_BYTES;
        const char* lb = smem + (3 + (kt & 1)) * OPERAND_BYTES;
        // both 32-deep halves' fragments are read up front (24 ds_read_b128): the second half's reads complete under
        // the first half's 32 MFMAs instead of stalling between them
        bf16x8 a[2][8], b[2][4];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wn * 64 + j * 16 + fr;
                const int ch = (ks * 4 + fq) ^ ((row >> 1) & 7);
                b[ks][j] = *reinterpret_cast<const bf16x8*>(lb + row * 128 + ch * 16);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = wm * 128 + i * 16 + fr;
                const int ch = (ks * 4 + fq) ^ ((row >> 1) & 7);
                a[ks][i] = *reinterpret_cast<const bf16x8*>(la + row * 128 + ch * 16);
            }
        }
        // The refills are issued from the MFMA block, after the fragment reads in program order (a DMA into LDS is never
        // hoisted over an LDS read; MFMAs may pass it): B(t+1)'s 4 issues right behind the reads, whose latency they
        // overlap, then A(t+2)'s 4 interleaved one per 16 MFMAs, instead of 8 back-to-back issues after the barrier
        // while the MFMA pipes idle (QKV / proj / FC1 / FC2 -1.8..-4.5 %, profiles/r1_gemm_lab/ilv_ab.txt).
        // Unconditional, so they stay in this block: past the end they re-read K-tile nk-1 into that K-tile's own slot
        // (identical bytes). Program order B, A keeps the counted vmcnt(4) at the next barrier meaning "B(t+1) has
        // landed".
        stage_b(min(kt + 1, nk - 1));
        stage_a(min(kt + 2, nk - 1));
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[ks][j], a[ks][i], acc[j][i], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 24, 0);   // the 24 fragment reads
        __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);    // B(t+1)'s DMA
#pragma unroll
        for (int q = 0; q < 4; ++q) {                          // 16 MFMAs per A(t+2) DMA issue
            __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
    }

    if constexpr (PART) {
        __builtin_amdgcn_s_waitcnt(0x0F70);   // the past-the-end refills land before the wave exits
        // lane: output row m0 + wm*128 + i*16 + (lane & 15), columns n0 + wn*64 + j*16 + 4*(lane >> 4) .. +3
        float* P = reinterpret_cast<float*>(C) + (size_t)blockIdx.y * M * N;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = m0 + wm * 128 + i * 16 + fr;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + wn * 64 + j * 16 + fq * 4;
                if (m < M && n < N) *reinterpret_cast<f32x4*>(P + (size_t)m * N + n) = acc[j][i];
            }
        }
        return;
    }
    // ---------------- epilogue (gemm_common.h) ----------------
    if constexpr (LN) {
        if constexpr (wide) {   // the planes DMA'd at the last K-step must land for every wave
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        combine_planes(planes_lds, aux, stats_parts, K, ln_eps, tid);   // the aux DMA landed before the last barrier
    }
    // this wave's image: the four 32 KiB slots other than the aux slot
    const int region = (wid >> 1) + ((wid >> 1) >= (nk % 3) ? 1 : 0);
    finish_tile<EPI, OUT8, DIRECT>(smem + region * OPERAND_BYTES + (wid & 1) * 16384, aux, acc, wm, wn, m0, n0, lane,
                                   residual, pos, g2, C, ldc, M, N, stats_out, stats_rows, o8);
}

// ---------------------------------------------------------------------------------------------------------------
// Ping-pong main loop (cdna_hip_programming.md §5 "The 256² 8-phase template", T3+T4): same tile, waves and
// epilogues as k_gemm_bf16, different sync structure.
//  * A K-tile is cut into four 16 KiB half-tiles, one per quadrant operand of a wave's 128x64 sub-tile:
//    A0 / A1 = the A rows of quadrant-row mh = 0 / 1 of BOTH wave rows (rows g*128 + mh*64 + r), B0 / B1 = the
//    W rows of quadrant-column nh = 0 / 1 of all four wave columns (rows wn*64 + nh*32 + r). Slot (buffer, type)
//    = 16 KiB at ((kt & 1) * 4 + type) * 16 KiB; 128 KiB ring + 32 KiB epilogue operands.
//  * Four phases per K-tile, one output quadrant (16 MFMAs) each: q0 (mh0,nh0) reads A0 + B0, q1 (mh0,nh1)
//    reads B1, q2 (mh1,nh1) reads A1, q3 (mh1,nh0) reads nothing (A1, B0 still in registers). Phase body:
//    [fragment reads | one half-tile DMA (2 pieces per wave) | counted vmcnt] barrier [lgkmcnt(0), 16 MFMAs]
//    barrier.
//  * The wave row wm = 1 runs one barrier behind wm = 0 (one extra barrier before the loop, matched by wm = 0
//    after it): the two waves that share a SIMD alternate, one issuing MFMAs while the other issues its LDS
//    reads and DMA (ping-pong).
//  * Half-tiles are consumed in the order n = 4k + {A0, B0, B1, A1} and half-tile n is DMA'd in phase n - 6:
//    q0 of K-tile t stages B1(t+1), q1 A1(t+1), q2 A0(t+2), q3 B0(t+2). WAR: a slot is re-staged >= 2 phases
//    after the phase that last read it (the reads of both wave rows are retired by then). RAW: the vmcnt(8) at
//    the end of the memory part of phase p leaves the 4 youngest half-tiles (n = p+3 .. p+6) in flight and
//    retires n <= p+2, which phase p+1 reads after one more barrier. q2 needs no wait (q3 reads nothing).
//  * Past the last K-tile the DMAs re-stage K-tile nk-1 (identical bytes), so every phase is branch-free.
template <int EPI, bool OUT8 = false>
__global__ __launch_bounds__(NTHREADS) void k_gemm_pp(const bf16_t* __restrict__ A, int lda,
                                                      const bf16_t* __restrict__ W,
                                                      const float* __restrict__ bias,
                                                      const bf16_t* residual,
                                                      const float* __restrict__ pos, int g2,
                                                      const float2* __restrict__ stats,
                                                      const float* __restrict__ colsum,
                                                      bf16_t* C, int ldc, int M, int N, int K, int group,
                                                      int stats_parts, float ln_eps, float* stats_out,
                                                      int stats_rows, Out8 o8) {
    constexpr int HALF = 16384;
    constexpr int RING = 8 * HALF;   // 2 buffers x {A0, B0, B1, A1}
    static_assert(RING + AUX_BYTES <= 160 * 1024, "LDS budget");
    __shared__ __attribute__((aligned(16))) char smem[RING + AUX_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid >> 2, wn = wid & 3;

    int m0, n0;
    tile_of(M, N, group, m0, n0);
    constexpr bool DIRECT = (EPI == VPF_EPI_LN_GELU || EPI == VPF_EPI_BIAS_GELU) && !OUT8;

    const char* Ablk = reinterpret_cast<const char*>(A) + (size_t)m0 * lda * 2;
    const char* Bblk = reinterpret_cast<const char*>(W) + (size_t)n0 * K * 2;
    // per-lane DMA source offsets: [type][piece]; piece p of a half-tile = local rows (wid + 8p) * 8 + lane / 8
    uint32_t off[4][2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int rho = (wid + 8 * p) * 8 + (lane >> 3);             // local row 0..127
        const int lch = (lane & 7) ^ ((rho >> 1) & 7);               // logical chunk at this physical slot
        const int ra0 = (rho >> 6) * 128 + (rho & 63);               // A0: g*128 + r
        const int rb0 = (rho >> 5) * 64 + (DIRECT ? wperm(rho & 31) : (rho & 31));   // B0: wn*64 + r
        const int ra[2] = {ra0, ra0 + 64}, rb[2] = {rb0, rb0 + 32};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            off[h == 0 ? 0 : 3][p] = (uint32_t)min(ra[h], M - 1 - m0) * (uint32_t)(lda * 2) + (uint32_t)(lch * 16);
            off[h == 0 ? 1 : 2][p] = (uint32_t)min(rb[h], N - 1 - n0) * (uint32_t)(K * 2) + (uint32_t)(lch * 16);
        }
    }
    const int nk = K / BK;
    // type: 0 = A0, 1 = B0, 2 = B1, 3 = A1
    auto stage = [&](int type, int kt) {
        kt = min(kt, nk - 1);
        char* slot = smem + ((kt & 1) * 4 + type) * HALF;
        const char* src = (type == 0 || type == 3) ? Ablk : Bblk;
        const uint32_t koff = (uint32_t)kt * (BK * 2);
#pragma unroll
        for (int p = 0; p < 2; ++p)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + off[type][p] + koff), (lptr_t)(slot + (wid + 8 * p) * 1024),
                                             16, 0, 0);
    };

    // epilogue operands (same layout as k_gemm_bf16's aux region), issued first: retired by the prologue wait
    constexpr bool LN = (EPI == VPF_EPI_LN || EPI == VPF_EPI_LN_GELU);
    char* aux = smem + RING;
    dma_bias_colsum<LN>(aux, bias, colsum, n0, N, wid, lane);
    if constexpr (LN) dma_planes(aux + 2048, stats, stats_parts, m0, M, wid, lane);
    // prologue: half-tiles n = 0..5 (K-tile 0 whole, A0 / B0 of K-tile 1); retire n <= 1 (+ the aux pieces)
    stage(0, 0); stage(1, 0); stage(2, 0); stage(3, 0); stage(0, 1); stage(1, 1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wm == 1) __builtin_amdgcn_s_barrier();   // the ping-pong offset
    asm volatile("" ::: "memory");

    f32x4 acc[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    // fragment read byte offsets inside a half-tile slot (without the k-chunk term): A rows wm*64 + i*16 + fr,
    // B rows wn*32 + j*16 + fr; (row >> 1) & 7 = (fr >> 1) & 7 for every fragment (row bases are multiples of 16)
    const int sw = (fr >> 1) & 7;
    const int abase = (wm * 64 + fr) * 128, bbase = (wn * 32 + fr) * 128;
    auto mfma_quadrant = [&](const i32x4 (&fa)[2][4], const i32x4 (&fb)[2][2], int mh, int nh) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[nh * 2 + j][mh * 4 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        __builtin_bit_cast(bf16x8, fb[ks][j]), __builtin_bit_cast(bf16x8, fa[ks][i]),
                        acc[nh * 2 + j][mh * 4 + i], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto read_a = [&](i32x4 (&fa)[2][4], const char* slot) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[ks][i] = lds16(slot + abase + i * 2048 + (((ks * 4 + fq) ^ sw) << 4));
    };
    auto read_b = [&](i32x4 (&fb)[2][2], const char* slot) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[ks][j] = lds16(slot + bbase + j * 2048 + (((ks * 4 + fq) ^ sw) << 4));
    };
    auto bar = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };

    for (int kt = 0; kt < nk; ++kt) {
        const char* buf = smem + (kt & 1) * 4 * HALF;
        i32x4 fa0[2][4], fa1[2][4], fb0[2][2], fb1[2][2];
        // q0: (mh0, nh0)
        read_a(fa0, buf);
        read_b(fb0, buf + HALF);
        stage(2, kt + 1);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        bar();
        mfma_quadrant(fa0, fb0, 0, 0);
        bar();
        // q1: (mh0, nh1)
        read_b(fb1, buf + 2 * HALF);
        stage(3, kt + 1);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        bar();
        mfma_quadrant(fa0, fb1, 0, 1);
        bar();
        // q2: (mh1, nh1)
        read_a(fa1, buf + 3 * HALF);
        stage(0, kt + 2);
        bar();
        mfma_quadrant(fa1, fb1, 1, 1);
        bar();
        // q3: (mh1, nh0)
        stage(1, kt + 2);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        bar();
        mfma_quadrant(fa1, fb0, 1, 0);
        bar();
    }
    if (wm == 0) __builtin_amdgcn_s_barrier();   // matches wm = 1's offset barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped re-stages past the end

    // ---------------- epilogue (k_gemm_bf16's, on the ring's 8 x 16 KiB) ----------------
    if constexpr (LN) combine_planes(aux + 2048, aux, stats_parts, K, ln_eps, tid);
    finish_tile<EPI, OUT8, DIRECT>(smem + wid * 16384, aux, acc, wm, wn, m0, n0, lane, residual, pos, g2, C, ldc, M, N,
                                   stats_out, stats_rows, o8);
}

// ---------------------------------------------------------------------------------------------------------------
// Tile-walking form of k_gemm_pp for FC1 (the direct-store GELU epilogues) and QKV (EPI_LN): one resident workgroup
// per CU walks several output tiles, and the six half-tile stages that fall past the end of a tile (A0 / B0 of "K-tile nk" at K-tile
// nk - 2; B1 / A1 of it and A0 / B0 of "nk + 1" at K-tile nk - 1), which k_gemm_pp spends on re-staging K-tile nk - 1,
// stage K-tiles 0 and 1 of the workgroup's NEXT tile instead. They are that tile's prologue set, in the prologue's
// order, and for even nk they land in the prologue's ring slots, so the ring runs on across the seam as if the walk
// were one long K loop: no redundant operand bytes (12.5 % of a K = 768 tile's), and no ring fill or workgroup launch
// with the MFMA pipe idle. The direct-store epilogue uses no LDS image, and EPI_LN's pipelined image epilogue runs
// on one 16-row group image per wave behind the aux sets (store_wave_tile_group), so the ring is free to fill under
// either. Measurements: DESIGN.md section 3.3 (round 10).
//  * Walk: workgroup b of a grid of G (a multiple of 8; at most the CU count) takes the logical ids
//    xcd_first(tiles, b & 7) + (b >> 3) + j G / 8, j = 0, 1, ... inside its XCD's range: at every step the workgroups
//    of an XCD cover consecutive ids, as the dispatcher's order does for k_gemm_pp (same tile_of_lid, same group). No
//    workgroup waits on another. The walk state is wave-uniform.
//  * Seam: before q2 of K-tile nk - 2 (the last stages of the current tile are issued by then) the panel bases and the
//    per-lane offsets are recomputed for the next tile and its epilogue operands are DMA'd into the other 4 KiB aux
//    set (stats_parts == 0: bias | colsum | one {mean, rstd} plane). The set was last read by the epilogue two tiles
//    back, which every wave has left by then (nk >= 2: at least the offset barrier and q0's lie between).
//  * Waits: the counted waits stay vmcnt(8). Across a seam the epilogue's global stores are younger than the prefetched
//    half-tiles and vmcnt retires in issue order, so in the first K-tile of a tile the 8 youngest operations hold
//    stores as well as half-tiles: the wait is then stricter than needed (it also retires the earlier stores, which
//    were issued a GELU row group or more before), never laxer, whatever number of stores a wave issued. The RAW rule
//    is k_gemm_pp's (a staged half-tile is read one phase after the wait that retires it), the WAR rule too.
//  * Read order (walk_reads_early instances: EARLY). k_gemm_pp's phases issue a wave's 24 ds_read_b128 of a K-tile as
//    12 / 4 / 8 / 0 (q0: A0 + B0, q1: B1, q2: A1, q3: none), and q0's 12 do not fit under the other wave row's 16
//    MFMAs. EARLY reads A0 of K-tile kt + 1 in q3 of K-tile kt, from the other buffer, into fa0's registers (dead since
//    q1's MFMAs): 4 / 4 / 8 / 8, the same MFMAs on the same bits. Per wave the half-tiles are issued in the order
//    ... A0(kt+1) [q2 of kt-1], B0(kt+1) [q3 of kt-1], B1(kt+1) [q0], A1(kt+1) [q1], A0(kt+2) [q2], B0(kt+2) [q3],
//    two operations each, and vmcnt retires in that order. In k_gemm_pp's scheme A0(kt+1) is retired only by q3's wait
//    (which leaves {B0(kt+2), A0(kt+2), A1(kt+1), B1(kt+1)} in flight) and read in q0 of kt + 1. EARLY adds one wait,
//    vmcnt(8) behind q2's stage: the 8 youngest operations are then {A0(kt+2), A1(kt+1), B1(kt+1), B0(kt+1)}, so
//    A0(kt+1), issued a whole K-tile earlier, has landed for this wave; q3 reads it one phase later, behind q2's two
//    barriers. With the one-barrier offset between the wave rows, wm = 0 leaves q2's second barrier only when wm = 1 has
//    reached q2's first one, i.e. has passed its own q2 wait, and wm = 1 leaves it only when wm = 0 has passed its q3
//    wait: every wave's pieces of A0(kt+1) are retired before any wave reads them (the RAW rule, unchanged: read one
//    phase after the wait that retires it, never in the same phase). No other count changes and no wait gets laxer.
//    WAR: the A0 slot read in q3 of kt is re-staged by stage(A0, kt+3) in q2 of kt + 1, three phases later; it was
//    staged in q2 of kt - 1, behind its previous readers (q3 of kt - 2).
//    Tile edges: a tile's first A0 fragments (K-tile 0, buffer 0) are read at the tile's top, in front of the offset
//    barrier: for the first tile behind the prologue's wait and barrier, for a later tile behind q3's wait of the
//    previous tile's last K-tile (it retires everything up to B0 of "K-tile nk") and the barriers that close the
//    offset. q3 of a tile's last K-tile still issues its eight reads (the next tile's K-tile 0, or on the last tile a
//    clamped re-stage, possibly still in flight) so that the loop stays branch-free, but nothing uses them: the
//    tile-top reads overwrite the registers, so no fragment is live across the epilogue. nk = 2: q3 of K-tile 0 reads
//    for K-tile 1, the tile's last. The reads carry slot and row as instruction offsets (frag_read): four address
//    registers per K-tile instead of one per read, which is what lets the 32 extra live registers of q3 fit without
//    scratch. The instances that are not EARLY compile to k_gemm_pp's order, instruction for instruction as before.
//  * The ping-pong offset is closed before the epilogue and reopened after it, as in k_gemm_pp, so both wave rows run
//    their epilogues side by side; no barrier inside the epilogue (nothing is combined in LDS at stats_parts == 0).
//  * On the workgroup's last tile the past-the-end stages stay clamped (k_gemm_pp's), retired before the wave exits.
// Same K order, MFMAs and epilogue math as k_gemm_pp / k_gemm_bf16: bit-identical outputs.
//
// The residual GEMMs (proj, FC2: EPI_BIAS_RESIDUAL with the statistics planes) walk with the same body under their own
// kernel name, k_gemm_walk_res: the aux set of a tile is the bias alone (1 KiB), the lane's 16 residual pieces are
// loaded by plain loads right behind the last MFMA quadrant of the tile (the fragment registers are dead from there
// on; at the loop's peak there is no room for 64 more VGPRs), and the epilogue is store_wave_tile_group_res
// (gemm_common.h) on the per-wave group image. The residual may be C itself: a lane reads exactly the pieces it later
// stores and no other workgroup touches the tile, so neither pointer is __restrict__. A call that also wants the fp8
// copy keeps the deep ring.
constexpr int WALK_HALF = 16384;
constexpr int WALK_RING = 8 * WALK_HALF;   // 2 buffers x {A0, B0, B1, A1}
constexpr int WALK_GROUP_IMG = 2048;       // 16 rows x 128 B
// aux set: bias | colsum | {mean, rstd} of 256 rows; the residual epilogue reads the bias only
constexpr int walk_aux_set(int epi) { return epi == VPF_EPI_BIAS_RESIDUAL ? 1024 : 4096; }
constexpr int walk_smem(int epi) {
    return WALK_RING + 2 * walk_aux_set(epi) + (epi_is_gelu(epi) ? 0 : 8 * WALK_GROUP_IMG);
}
// which instances read K-tile kt + 1's A0 fragments in q3 of K-tile kt (the 4 / 4 / 8 / 8 order; the others keep
// 12 / 4 / 8 / 0): decided per instance by its own A/B against the parent's order
constexpr bool walk_reads_early(int epi) {
    return epi == VPF_EPI_LN || epi == VPF_EPI_LN_GELU || epi == VPF_EPI_BIAS_RESIDUAL;
}

// ds_read_b128 of the 16 B at LDS address `addr + OFF`, OFF in the instruction (16 bits)
template <int OFF>
__device__ __forceinline__ i32x4 lds16_at(uint32_t addr) {
    static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field");
    i32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
// the NF row fragments (16 rows = 2 KiB apart) of both k-steps of the half-tile slot at byte SLOT of a buffer;
// ad[ks] = the buffer's address + the lane's row and k-chunk term
template <int SLOT, int NF>
__device__ __forceinline__ void frag_read(i32x4 (&f)[2][NF], const uint32_t (&ad)[2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        f[ks][0] = lds16_at<SLOT>(ad[ks]);
        f[ks][1] = lds16_at<SLOT + 2048>(ad[ks]);
        if constexpr (NF == 4) {
            f[ks][2] = lds16_at<SLOT + 4096>(ad[ks]);
            f[ks][3] = lds16_at<SLOT + 6144>(ad[ks]);
        }
    }
}

template <int EPI, bool EARLY = walk_reads_early(EPI)>
__device__ __forceinline__ void gemm_walk_body(char* smem, const bf16_t* __restrict__ A, int lda,
                                               const bf16_t* __restrict__ W, const float* __restrict__ bias,
                                               const float2* __restrict__ stats, const float* __restrict__ colsum,
                                               const bf16_t* residual, bf16_t* C, int ldc, int M, int N, int K,
                                               int group, int tiles, float* stats_out) {
    constexpr bool RES = EPI == VPF_EPI_BIAS_RESIDUAL;
    constexpr bool DIRECT = epi_is_gelu(EPI);   // else one 16-row group image per wave, outside the ring
    constexpr int HALF = WALK_HALF;
    constexpr int RING = WALK_RING;
    constexpr int AUX_SET = walk_aux_set(EPI);
    constexpr int GROUP_IMG = WALK_GROUP_IMG;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid >> 2, wn = wid & 3;
    constexpr bool LN = epi_is_ln(EPI);
    const int nk = K / BK;   // even, >= 2 (host)

    // ---- the walk (wave-uniform) ----
    const int stride = (int)gridDim.x >> 3;
    int lid = xcd_first(tiles, (int)blockIdx.x & 7) + ((int)blockIdx.x >> 3);
    const int lid_end = xcd_first(tiles, ((int)blockIdx.x & 7) + 1);
    if (lid >= lid_end) return;
    int m0, n0;
    tile_of_lid(M, N, group, lid, m0, n0);

    // staging state: panel bases and per-lane DMA source offsets [type][piece] of the tile being staged (k_gemm_pp's)
    const char* Ablk;
    const char* Bblk;
    uint32_t off[4][2];
    auto set_panels = [&](int tm0, int tn0, int ln) {
        Ablk = reinterpret_cast<const char*>(A) + (size_t)tm0 * lda * 2;
        Bblk = reinterpret_cast<const char*>(W) + (size_t)tn0 * K * 2;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int rho = (wid + 8 * p) * 8 + (ln >> 3);              // local row 0..127
            const int lch = (ln & 7) ^ ((rho >> 1) & 7);                // logical chunk at this physical slot
            const int ra0 = (rho >> 6) * 128 + (rho & 63);              // A0: g*128 + r
            const int rb0 = (rho >> 5) * 64 + (DIRECT ? wperm(rho & 31) : (rho & 31));   // B0: wn*64 + r
            const int ra[2] = {ra0, ra0 + 64}, rb[2] = {rb0, rb0 + 32};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                off[h == 0 ? 0 : 3][p] = (uint32_t)min(ra[h], M - 1 - tm0) * (uint32_t)(lda * 2) + (uint32_t)(lch * 16);
                off[h == 0 ? 1 : 2][p] = (uint32_t)min(rb[h], N - 1 - tn0) * (uint32_t)(K * 2) + (uint32_t)(lch * 16);
            }
        }
    };
    // type: 0 = A0, 1 = B0, 2 = B1, 3 = A1; kt counts from the first K-tile of the tile being staged
    auto stage = [&](int type, int kt) {
        kt = min(kt, nk - 1);
        char* slot = smem + ((kt & 1) * 4 + type) * HALF;
        const char* src = (type == 0 || type == 3) ? Ablk : Bblk;
        const uint32_t koff = (uint32_t)kt * (BK * 2);
#pragma unroll
        for (int p = 0; p < 2; ++p)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + off[type][p] + koff), (lptr_t)(slot + (wid + 8 * p) * 1024),
                                             16, 0, 0);
    };
    auto load_aux = [&](char* dst, int tm0, int tn0, int ln) {
        dma_bias_colsum<LN>(dst, bias, colsum, tn0, N, wid, ln);
        if constexpr (LN) dma_planes(dst + 2048, stats, 0, tm0, M, wid, ln);
    };

    // prologue of the first tile (k_gemm_pp's): epilogue operands, half-tiles n = 0..5; retire n <= 1 and the aux pieces
    set_panels(m0, n0, lane);
    load_aux(smem + RING, m0, n0, lane);
    stage(0, 0); stage(1, 0); stage(2, 0); stage(3, 0); stage(0, 1); stage(1, 1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    f32x4 acc[4][8];
    const int fr = lane & 15, fq = lane >> 4;
    const int sw = (fr >> 1) & 7;
    const int abase = (wm * 64 + fr) * 128, bbase = (wn * 32 + fr) * 128;
    auto mfma_quadrant = [&](const i32x4 (&fa)[2][4], const i32x4 (&fb)[2][2], int mh, int nh) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[nh * 2 + j][mh * 4 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        __builtin_bit_cast(bf16x8, fb[ks][j]), __builtin_bit_cast(bf16x8, fa[ks][i]),
                        acc[nh * 2 + j][mh * 4 + i], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto read_a = [&](i32x4 (&fa)[2][4], const char* slot) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[ks][i] = lds16(slot + abase + i * 2048 + (((ks * 4 + fq) ^ sw) << 4));
    };
    auto read_b = [&](i32x4 (&fb)[2][2], const char* slot) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[ks][j] = lds16(slot + bbase + j * 2048 + (((ks * 4 + fq) ^ sw) << 4));
    };
    auto bar = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    i32x4 fa0[2][4];   // EARLY: K-tile kt + 1's are read in q3 of K-tile kt and carried into the next iteration
    // EARLY: the fragment reads carry the slot and the row term as the instruction's offset (frag_read), so a K-tile
    // needs four address registers (A and B, ks = 0 / 1), not one per read: 32 more fragment registers are live in q3
    const uint32_t ring32 = (uint32_t)(uintptr_t)(lptr_t)smem;
    const uint32_t arel[2] = {(uint32_t)(abase + ((fq ^ sw) << 4)), (uint32_t)(abase + (((4 + fq) ^ sw) << 4))};
    const uint32_t brel[2] = {(uint32_t)(bbase + ((fq ^ sw) << 4)), (uint32_t)(bbase + (((4 + fq) ^ sw) << 4))};

    int skt = 0;   // the stages of a K-step are K-tiles skt + 1, skt + 2 of the tile being staged
    int par = 0;   // aux set of the current tile
    for (;;) {
        const int lid_next = lid + stride;
        const bool more = lid_next < lid_end;
        int m0n = m0, n0n = n0;
        if constexpr (EARLY) {   // A0 of the tile's K-tile 0 (buffer 0: nk is even), retired before the barrier behind us
            const uint32_t a0[2] = {ring32 + arel[0], ring32 + arel[1]};
            frag_read<0>(fa0, a0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (wm == 1) __builtin_amdgcn_s_barrier();   // the ping-pong offset
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int kt = 0; kt < nk; ++kt, ++skt) {
            const char* buf = smem + (kt & 1) * 4 * HALF;
            i32x4 fa1[2][4], fb0[2][2], fb1[2][2];
            const uint32_t buf32 = ring32 + (kt & 1) * 4 * HALF, nbuf32 = ring32 + ((kt + 1) & 1) * 4 * HALF;
            [[maybe_unused]] const uint32_t ad[2] = {buf32 + arel[0], buf32 + arel[1]};
            [[maybe_unused]] const uint32_t bd[2] = {buf32 + brel[0], buf32 + brel[1]};
            [[maybe_unused]] const uint32_t nad[2] = {nbuf32 + arel[0], nbuf32 + arel[1]};
            // q0: (mh0, nh0)
            if constexpr (EARLY) {
                frag_read<HALF>(fb0, bd);
            } else {
                read_a(fa0, buf);
                read_b(fb0, buf + HALF);
            }
            stage(2, skt + 1);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            bar();
            mfma_quadrant(fa0, fb0, 0, 0);
            bar();
            // q1: (mh0, nh1)
            if constexpr (EARLY) frag_read<2 * HALF>(fb1, bd);
            else read_b(fb1, buf + 2 * HALF);
            stage(3, skt + 1);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            bar();
            mfma_quadrant(fa0, fb1, 0, 1);
            bar();
            // the seam: everything staged from here on belongs to the next tile
            if (more && kt == nk - 2) {
                const int ln = opaque_lane();   // keeps the per-lane terms out of the registers live across the loop
                tile_of_lid(M, N, group, lid_next, m0n, n0n);
                set_panels(m0n, n0n, ln);
                load_aux(smem + RING + (par ^ 1) * AUX_SET, m0n, n0n, ln);
                skt -= nk;
            }
            // q2: (mh1, nh1)
            if constexpr (EARLY) frag_read<3 * HALF>(fa1, ad);
            else read_a(fa1, buf + 3 * HALF);
            stage(0, skt + 2);
            if constexpr (EARLY) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // retires A0(kt + 1) for q3
            bar();
            mfma_quadrant(fa1, fb1, 1, 1);
            bar();
            // q3: (mh1, nh0)
            if constexpr (EARLY) frag_read<0>(fa0, nad);   // A0(kt + 1); fa0's registers died in q1
            stage(1, skt + 2);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            bar();
            mfma_quadrant(fa1, fb0, 1, 0);
            bar();
        }
        // the residual pieces go out here, where the fragment registers have just died; the lane id is re-read so
        // that no per-lane epilogue address is computed above the K loop and kept live across it
        [[maybe_unused]] uint4 res[16];
        [[maybe_unused]] int eln = lane;
        if constexpr (RES) {
            eln = opaque_lane();
            load_residual<true>(res, residual, wm, wn, m0, n0, eln, ldc, M, N);
        } else if constexpr (EARLY && !DIRECT) {
            eln = opaque_lane();   // as above: with fa0 carried through q3 the loop has no register to spare
        }
        if (wm == 0) __builtin_amdgcn_s_barrier();   // matches wm = 1's offset barrier
        asm volatile("" ::: "memory");
        // the aux set landed with (first tile) the prologue wait or (later) long before the half-tiles staged after it
        if constexpr (DIRECT)
            store_wave_tile_direct<EPI, true>(smem + RING + par * AUX_SET, acc, wm, wn, m0, n0, lane, C, ldc, M, N);
        else if constexpr (RES)
            store_wave_tile_group_res(smem + RING + 2 * AUX_SET + wid * GROUP_IMG, smem + RING + par * AUX_SET, acc, wm,
                                      wn, m0, n0, eln, res, C, ldc, M, N, stats_out, M);
        else
            store_wave_tile_group<EPI>(smem + RING + 2 * AUX_SET + wid * GROUP_IMG, smem + RING + par * AUX_SET, acc, wm,
                                       wn, m0, n0, eln, C, ldc, M, N);
        if (!more) break;
        lid = lid_next;
        m0 = m0n;
        n0 = n0n;
        par ^= 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped re-stages past the end of the last tile
}

template <int EPI>
__global__ __launch_bounds__(NTHREADS) void k_gemm_walk(const bf16_t* __restrict__ A, int lda,
                                                        const bf16_t* __restrict__ W,
                                                        const float* __restrict__ bias,
                                                        const float2* __restrict__ stats,
                                                        const float* __restrict__ colsum, bf16_t* C, int ldc, int M,
                                                        int N, int K, int group, int tiles) {
    static_assert(EPI == VPF_EPI_LN_GELU || EPI == VPF_EPI_BIAS_GELU || EPI == VPF_EPI_LN, "FC1's and QKV's epilogues");
    __shared__ __attribute__((aligned(16))) char smem[walk_smem(EPI)];
    gemm_walk_body<EPI>(smem, A, lda, W, bias, stats, colsum, nullptr, C, ldc, M, N, K, group, tiles, nullptr);
}

// proj / FC2: stats_out (null: no planes) holds ceil(N / 64) planes of M rows x {sum, sumsq}
__global__ __launch_bounds__(NTHREADS) void k_gemm_walk_res(const bf16_t* __restrict__ A, int lda,
                                                            const bf16_t* __restrict__ W,
                                                            const float* __restrict__ bias, const bf16_t* residual,
                                                            bf16_t* C, int ldc, int M, int N, int K, int group,
                                                            int tiles, float* stats_out) {
    __shared__ __attribute__((aligned(16))) char smem[walk_smem(VPF_EPI_BIAS_RESIDUAL)];
    gemm_walk_body<VPF_EPI_BIAS_RESIDUAL>(smem, A, lda, W, bias, nullptr, nullptr, residual, C, ldc, M, N, K, group,
                                          tiles, stats_out);
}

}  // namespace

#define VPF_IS_LN(E) ((E) == VPF_EPI_LN || (E) == VPF_EPI_LN_GELU)
#define VPF_IS_PROD(E) ((E) == VPF_EPI_BIAS_RESIDUAL || (E) == VPF_EPI_PATCH)
#define VPF_GEMM_ARGS                                                                                        \
    A, (int)lda, W, bias, residual, pos, patch_rows, reinterpret_cast<const float2*>(row_stats), colsum, C,     \
        (int)ldc, m, n, k, group, stats_parts, ln_eps, stats_out, stats_rows, o8
// fp8 copies are produced by the residual-stream producers only (proj, patch embed): the only bf16 GEMMs whose output
// an MX8 GEMM reads. Kernel 5 (the ping-pong loop) holds at most AUX_PARTS planes next to its ring.
#define VPF_GEMM_LAUNCH(E)                                                                                   \
    do {                                                                                                     \
        if (kern == 5 && !(VPF_IS_LN(E) && stats_parts > AUX_PARTS) && o8.q == nullptr)                      \
            hipLaunchKernelGGL((k_gemm_pp<E, false>), grid, block, 0, s, VPF_GEMM_ARGS);                     \
        else if (kern == 5 && VPF_IS_PROD(E) && o8.q != nullptr)                                             \
            hipLaunchKernelGGL((k_gemm_pp<E, VPF_IS_PROD(E)>), grid, block, 0, s, VPF_GEMM_ARGS);            \
        else if (VPF_IS_LN(E) && stats_parts > AUX_PARTS)                                                    \
            hipLaunchKernelGGL((k_gemm_bf16<E, VPF_IS_LN(E)>), grid, block, 0, s, VPF_GEMM_ARGS);             \
        else if (VPF_IS_PROD(E) && o8.q != nullptr)                                                          \
            hipLaunchKernelGGL((k_gemm_bf16<E, false, VPF_IS_PROD(E)>), grid, block, 0, s, VPF_GEMM_ARGS);    \
        else                                                                                                 \
            hipLaunchKernelGGL((k_gemm_bf16<E>), grid, block, 0, s, VPF_GEMM_ARGS);                           \
    } while (0)

// Kernel and tile order per shape. The product library has two bf16 kernels, bit-identical on every output
// (test_gemm_kernel_variants_bit_identical): 1 = k_gemm_bf16 (deep ring, refills from the MFMA block), 5 = the ping-pong
// loop k_gemm_pp. The A/B variants of earlier rounds (2-stage ring, refills after the barrier, two-pass epilogue, the
// four-wave AGPR loop, staggered starts, the persistent kernel, the mid-K barrier loop, timing probes) live in the lab
// build (tools/gemm_lab, libvpf_lab.so); no environment variable selects a kernel here.
//  * QKV (the LN-folded bias-only epilogue) runs kernel 5: 2.5 % faster there in one process (2.603 vs 2.670 ms,
//    profiles/r2_gemm_lab/kernel_ab_r2s5.txt). FC1 (LN + GELU) runs kernel 5 since its epilogue stores straight from
//    the accumulators (store_wave_tile_direct): 3.751 vs 3.817 ms (profiles/r4_lab/fc1_direct_kernel_group_ab.txt);
//    with the LDS-image epilogue the two kernels were level on FC1. Every other epilogue is fastest on kernel 1.
//    (This is the choice among the one-tile-per-workgroup kernels; at two or more tiles per CU FC1, QKV, proj and FC2
//    take the tile-walking kernels instead: walk_grid_for below.)
//  * Tile order (A panels per group; the order never changes a bit), profiles/r2_gemm_lab/group_sweep_r2.txt: the
//    N <= 1024 GEMMs (proj / FC2: 3 column tiles) are 1-1.5 % faster with 2 panels per group (FC2 3.196 vs 3.226 ms,
//    proj 1.070 vs 1.082), QKV with 4; FC1 (LN + GELU, 12 column tiles at ViT-B) takes 8: 16 was -0.9 % on FC1 and
//    -0.7 % on the frame against 4 (fc1_group16_pmc.txt), and 8 another 0.3-0.5 % ahead of 16 (group_sweep_r2s5.txt,
//    fc1_pp_group_ab.txt).
// vpf_gemm_tune(kernel, group) is an explicit test / A/B hook: kernel 1 or 5 for every shape (and a fixed group when
// group >= 0), 0 = back to the per-shape defaults. It is process state set by a call, never read from the environment.
constexpr int kDefaultGroup = 4;
static int g_kernel = 0;   // 0: per-shape default; 1 / 5: forced by vpf_gemm_tune
static int g_group = -1;   // -1: per-shape default
static int gemm_kernel_for(int epilogue) {
    if (g_kernel) return g_kernel;
    return (epilogue == VPF_EPI_LN || epilogue == VPF_EPI_LN_GELU) ? 5 : 1;
}
static int tile_group_for(int64_t N, int epilogue) {
    if (g_group >= 0) return g_group;
    if (N <= 1024) return 2;
    return epilogue == VPF_EPI_LN_GELU ? 8 : kDefaultGroup;
}
int vpf_gemm_tile_group() { return g_group >= 0 ? g_group : kDefaultGroup; }   // shared with gemm_mx8.hip
// MX8 GEMMs' default group (profiles/r2_gemm_lab/mx8_group_sweep.txt, fp8 frames): the LN-folded bias-only QKV is ~5 %
// faster with 8 A panels per group (1.93-1.95 vs 2.05 ms); proj / FC1 / FC2 keep 4.
int vpf_gemm_tile_group_mx8(int epilogue) {
    if (g_group >= 0) return g_group;
    return epilogue == VPF_EPI_LN ? 8 : kDefaultGroup;
}
VPF_API int vpf_gemm_tune(int kernel, int group) {
    if (kernel != 0 && kernel != 1 && kernel != 5) return VPF_ERR_ARG;
    if (group < -1 || group > 64) return VPF_ERR_ARG;
    g_kernel = kernel;
    g_group = kernel == 0 ? -1 : group;
    return 0;
}

// The tile-walking kernels (k_gemm_walk, k_gemm_walk_res) are routed per call on the host. They can run the direct-store
// epilogues (EPI_LN_GELU, EPI_BIAS_GELU), EPI_LN and EPI_BIAS_RESIDUAL (without the fp8 copy) with an even number of
// K-tiles, {mean, rstd} row statistics (stats_parts == 0) and no kernel forced by vpf_gemm_tune. The per-shape rule
// routes EPI_LN_GELU (FC1), EPI_LN (QKV) and the K-tile counts of EPI_BIAS_RESIDUAL named below at two or more tiles
// per workgroup of a grid of one workgroup per CU (rounded down to a multiple of 8: the
// XCD count); everything else keeps k_gemm_bf16 / k_gemm_pp. vpf_gemm_persistent is its test / A/B hook, process
// state set by a call like vpf_gemm_tune: mode -1 = never, 0 = the per-shape rule above, 1 = whenever the kernel can
// run (at least 8 tiles; the grid shrinks to the tile count's multiple of 8), and an optional grid cap so that a small
// problem is walked by few workgroups. The CU count is read once per device and cached: by vpf_gemm_persistent and
// vpf_gemm_persistent_grid, which the engine calls when it is constructed (outside any stream capture); a caller that
// never does leaves the read to its first eligible launch (two host queries, no stream operation).
// Per-shape default: only what passed its own A/B against the parent build (gain > twice the session's A/A spread),
// EPI_LN_GELU (FC1) and EPI_LN (QKV). EPI_BIAS_GELU can run the kernel (forced mode, tested for bits) but nobody has
// timed it against kernel 1, its default, so it is not routed by default. EPI_BIAS_RESIDUAL is decided per K-tile
// count, because its default (kernel 1, the deep ring) and the walk differ in the K loop as well as in the seam: the
// two counts that were measured and passed are routed, proj's nk = 12 (-7.9 / -8.5 %) and FC2's nk = 48 (-5.7 /
// -5.2 %, A/A spread 0.4 - 0.5 %). Every other count keeps the deep ring.
static bool walk_by_default(int epilogue, int64_t nk) {
    if (epilogue == VPF_EPI_BIAS_RESIDUAL) return nk == 12 || nk == 48;
    return epilogue == VPF_EPI_LN_GELU || epilogue == VPF_EPI_LN;
}
static int g_walk_mode = 0;
static int g_walk_cap = 0;                 // 0: no cap
static std::atomic<int> g_walk_cus[64];    // per device: CU count rounded down to a multiple of 8 (0: not read yet)
static int walk_device_grid() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int cus = g_walk_cus[dev].load(std::memory_order_relaxed);
    if (cus == 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        cus &= ~7;
        g_walk_cus[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}
// grid of the walking kernel for this call, 0 = keep the one-tile-per-workgroup kernels
static int walk_grid_for(int epilogue, int64_t tiles, int64_t K, int stats_parts) {
    if (epilogue != VPF_EPI_LN_GELU && epilogue != VPF_EPI_BIAS_GELU && epilogue != VPF_EPI_LN &&
        epilogue != VPF_EPI_BIAS_RESIDUAL)
        return 0;
    if (g_kernel != 0 || g_walk_mode < 0 || (g_walk_mode == 0 && !walk_by_default(epilogue, K / BK))) return 0;
    if ((K / BK) % 2 != 0 || stats_parts != 0 || tiles < 8) return 0;
    int grid = walk_device_grid();
    if (g_walk_cap > 0) grid = std::min(grid, g_walk_cap);
    if (grid < 8) return 0;
    if (g_walk_mode == 0) return tiles >= 2 * (int64_t)grid ? grid : 0;
    return (int)std::min<int64_t>(grid, tiles & ~(int64_t)7);
}
VPF_API int vpf_gemm_persistent(int mode, int grid_cap) {
    if (mode < -1 || mode > 1 || grid_cap < 0 || grid_cap % 8 != 0 || grid_cap > 4096) return VPF_ERR_ARG;
    g_walk_mode = mode;
    g_walk_cap = grid_cap;
    (void)walk_device_grid();   // without a device the first launch reads it
    return 0;
}
VPF_API int vpf_gemm_persistent_grid(int64_t M, int64_t N, int64_t K, int epilogue, int stats_parts) {
    (void)walk_device_grid();   // caches the current device's CU count whatever the shape
    if (M <= 0 || N <= 0 || K <= 0 || K % BK != 0) return 0;
    const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    return tiles > INT32_MAX ? 0 : walk_grid_for(epilogue, tiles, K, stats_parts);
}

// fp8 output operand check shared with gemm_mx8.hip: element rows ld8 >= N bytes (8-B aligned pieces), scale
// planes of lds_c >= output rows words (lds_c % 64 == 0, mx8_scale_byte), N % 128 == 0.
int vpf_check_out8(const uint8_t* C8, int64_t ld8, const uint32_t* Cs, int64_t lds_c, int64_t rows, int64_t N) {
    if (!C8) return Cs ? VPF_ERR_ARG : 0;
    if (!Cs || N % 128 != 0 || ld8 < N || ld8 % 8 != 0 || ((uintptr_t)C8 & 7) || lds_c < rows || lds_c % 64 != 0 ||
        ((uintptr_t)Cs & 3) || ld8 > INT32_MAX || lds_c > INT32_MAX / 4)
        return VPF_ERR_ARG;
    return 0;
}

// Argument checks common to vpf_gemm_bf16, vpf_gemm_bf16_splitk and vpf_gemm_mx8 (each adds its own): dimensions
// (K a multiple of k_unit), leading dimensions (lda a multiple of a_align elements of a_bytes bytes; ldc only when
// there is a bf16 output), what the kernels hold in 32 bits (int rows / columns, uint32 DMA offsets inside a 256-row A
// panel), the alignment of the DMA'd epilogue operands (bias / colsum in 16-B pieces, row statistics in 4-B pieces;
// null: not DMA'd), the tile count. Returns the number of 256 x 256 output tiles, 0 for a bad argument.
int64_t vpf_gemm_check(int64_t M, int64_t N, int64_t K, int64_t k_unit, int64_t lda, int a_align, int a_bytes,
                       bool has_c, int64_t ldc, const float* bias, const float* colsum, const float* row_stats) {
    if (M <= 0 || N <= 0 || K <= 0 || K % k_unit != 0 || N % 8 != 0 || lda < K || lda % a_align != 0) return 0;
    if (has_c && (ldc < N || ldc % 8 != 0 || ldc > INT32_MAX / 2)) return 0;
    if (M > INT32_MAX / 2 || N > 65536 || K > 65536 || lda > INT32_MAX / 2) return 0;
    if ((uint64_t)BM * (uint64_t)lda * (uint64_t)a_bytes > UINT32_MAX) return 0;
    if (((uintptr_t)bias & 15) || ((uintptr_t)colsum & 15) || ((uintptr_t)row_stats & 7)) return 0;
    const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    return tiles > INT32_MAX ? 0 : tiles;
}

VPF_API int vpf_gemm_bf16(const uint16_t* A, int64_t lda, const uint16_t* W, const float* bias,
                          const uint16_t* residual, const float* pos, int patch_rows, const float* row_stats,
                          const float* colsum, uint16_t* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                          int epilogue, int stats_parts, float ln_eps, float* stats_out, uint8_t* C8, int64_t ld8,
                          uint32_t* Cs, int64_t lds_c, void* stream) {
    const int64_t tiles = vpf_gemm_check(M, N, K, BK, lda, 8, 2, true, ldc, bias, colsum, row_stats);
    if (!tiles) return VPF_ERR_ARG;
    if (!A || !W || !bias || !C) return VPF_ERR_ARG;
    if (epilogue == VPF_EPI_BIAS_RESIDUAL && !residual) return VPF_ERR_ARG;
    if (epilogue == VPF_EPI_PATCH && (!pos || patch_rows <= 0 || M % patch_rows != 0)) return VPF_ERR_ARG;
    if ((epilogue == VPF_EPI_LN || epilogue == VPF_EPI_LN_GELU) && (!row_stats || !colsum)) return VPF_ERR_ARG;
    if (stats_parts < 0 || stats_parts > MAX_PARTS || !(ln_eps >= 0.f)) return VPF_ERR_ARG;
    if (stats_out && (((uintptr_t)stats_out & 7) || (epilogue != VPF_EPI_BIAS_RESIDUAL && epilogue != VPF_EPI_PATCH)))
        return VPF_ERR_ARG;
    // producer plane stride: rows of C (EPI_PATCH interleaves one CLS row per patch_rows rows)
    const int64_t srows = epilogue == VPF_EPI_PATCH ? (M / patch_rows) * (patch_rows + 1) : M;
    if (srows > INT32_MAX) return VPF_ERR_ARG;
    const int stats_rows = (int)srows;
    // fp8 copy of C: residual-stream producers only, deep-ring kernel
    if (C8 && epilogue != VPF_EPI_BIAS_RESIDUAL && epilogue != VPF_EPI_PATCH) return VPF_ERR_ARG;
    if (vpf_check_out8(C8, ld8, Cs, lds_c, srows, N)) return VPF_ERR_ARG;
    const Out8 o8{C8, reinterpret_cast<uint8_t*>(Cs), (int)ld8, (int)lds_c};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles), block(NTHREADS);
    const int kern = gemm_kernel_for(epilogue);
    const int group = tile_group_for(N, epilogue);
    const int m = (int)M, n = (int)N, k = (int)K;
    if (const int wgrid = C8 ? 0 : walk_grid_for(epilogue, tiles, K, stats_parts)) {
        const float2* st = reinterpret_cast<const float2*>(row_stats);
        if (epilogue == VPF_EPI_BIAS_RESIDUAL)
            hipLaunchKernelGGL(k_gemm_walk_res, dim3((unsigned)wgrid), block, 0, s, A, (int)lda, W, bias, residual, C,
                               (int)ldc, m, n, k, group, (int)tiles, stats_out);
        else if (epilogue == VPF_EPI_LN_GELU)
            hipLaunchKernelGGL((k_gemm_walk<VPF_EPI_LN_GELU>), dim3((unsigned)wgrid), block, 0, s, A, (int)lda, W, bias,
                               st, colsum, C, (int)ldc, m, n, k, group, (int)tiles);
        else if (epilogue == VPF_EPI_LN)
            hipLaunchKernelGGL((k_gemm_walk<VPF_EPI_LN>), dim3((unsigned)wgrid), block, 0, s, A, (int)lda, W, bias, st,
                               colsum, C, (int)ldc, m, n, k, group, (int)tiles);
        else
            hipLaunchKernelGGL((k_gemm_walk<VPF_EPI_BIAS_GELU>), dim3((unsigned)wgrid), block, 0, s, A, (int)lda, W, bias,
                               st, colsum, C, (int)ldc, m, n, k, group, (int)tiles);
        VPF_RETURN_LAUNCH();
    }
    switch (epilogue) {
        case VPF_EPI_BIAS: VPF_GEMM_LAUNCH(VPF_EPI_BIAS); break;
        case VPF_EPI_BIAS_GELU: VPF_GEMM_LAUNCH(VPF_EPI_BIAS_GELU); break;
        case VPF_EPI_BIAS_RESIDUAL: VPF_GEMM_LAUNCH(VPF_EPI_BIAS_RESIDUAL); break;
        case VPF_EPI_PATCH: VPF_GEMM_LAUNCH(VPF_EPI_PATCH); break;
        case VPF_EPI_LN: VPF_GEMM_LAUNCH(VPF_EPI_LN); break;
        case VPF_EPI_LN_GELU: VPF_GEMM_LAUNCH(VPF_EPI_LN_GELU); break;
        default: return VPF_ERR_ARG;
    }
    VPF_RETURN_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------
// Split-K form for GEMMs with few rows (the last block's CLS-row GEMMs: M = particles per GPU, so 6 - 48 output
// tiles each running the whole K loop on one CU). S blocks per tile each run K/S (k_gemm_bf16<PART>) into fp32
// partial planes; k_splitk_reduce sums the S planes in split order (fixed: the result does not depend on M) and
// applies the epilogue with the semantics of vpf_gemm_bf16's: LN / LN_GELU from {mean, rstd} row statistics,
// BIAS / BIAS_GELU, BIAS_RESIDUAL (bf16(acc + b) + residual, rounded again) with optional statistics planes of the
// stored values. One thread per 8 consecutive columns of a row; a 64-column plane block is 8 lanes (xor shuffles).
template <int EPI>
__global__ __launch_bounds__(256) void k_splitk_reduce(const float* __restrict__ P, int S, int M, int N,
                                                       const float* __restrict__ bias,
                                                       const float2* __restrict__ stats,
                                                       const float* __restrict__ colsum, const bf16_t* residual,
                                                       bf16_t* C, int64_t ldc, float* stats_out) {
    constexpr bool LN = (EPI == VPF_EPI_LN || EPI == VPF_EPI_LN_GELU);
    constexpr bool GELU = (EPI == VPF_EPI_BIAS_GELU || EPI == VPF_EPI_LN_GELU);
    const int per_row = N >> 3;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < (int64_t)M * per_row;
    const int m = live ? (int)(t / per_row) : 0;
    const int n = live ? (int)(t - (int64_t)m * per_row) * 8 : 0;
    float v[8];
    if (live) {
        const float* p = P + (size_t)m * N + n;
        const float4 a0 = *reinterpret_cast<const float4*>(p), a1 = *reinterpret_cast<const float4*>(p + 4);
        v[0] = a0.x; v[1] = a0.y; v[2] = a0.z; v[3] = a0.w; v[4] = a1.x; v[5] = a1.y; v[6] = a1.z; v[7] = a1.w;
        for (int s = 1; s < S; ++s) {
            const float* q = p + (size_t)s * M * N;
            const float4 b0 = *reinterpret_cast<const float4*>(q), b1 = *reinterpret_cast<const float4*>(q + 4);
            v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
        }
        float rstd = 1.f, nrm = 0.f;
        if constexpr (LN) {
            const float2 st = stats[m];
            rstd = st.y;
            nrm = -st.y * st.x;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float y = LN ? fmaf(rstd, v[e], fmaf(nrm, colsum[n + e], bias[n + e])) : v[e] + bias[n + e];
            if constexpr (GELU) {
                const f32x2 g = gelu_sig2(f32x2{y, y});
                y = g.x;
            }
            v[e] = y;
        }
    }
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf2(v[2 * e], v[2 * e + 1]);
    if constexpr (EPI == VPF_EPI_BIAS_RESIDUAL) {
        if (live) {
            const uint4 v = add_bf16x8(make_uint4(o[0], o[1], o[2], o[3]),
                                       *reinterpret_cast<const uint4*>(residual + (size_t)m * ldc + n));
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        }
        if (stats_out != nullptr) {   // {sum, sumsq} of the stored values over this lane's 64-column block
            float s1 = 0.f, s2 = 0.f;
            if (live) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float lo = bf2f((bf16_t)(o[e] & 0xffff)), hi = bf2f((bf16_t)(o[e] >> 16));
                    s1 += lo + hi;
                    s2 = fmaf(lo, lo, s2);
                    s2 = fmaf(hi, hi, s2);
                }
            }
#pragma unroll
            for (int x = 1; x < 8; x <<= 1) {
                s1 += __shfl_xor(s1, x, 64);
                s2 += __shfl_xor(s2, x, 64);
            }
            if (live && (n & 63) == 0)
                *reinterpret_cast<float2*>(stats_out + ((int64_t)(n >> 6) * M + m) * 2) = make_float2(s1, s2);
        }
    }
    if (live) *reinterpret_cast<uint4*>(C + (size_t)m * ldc + n) = make_uint4(o[0], o[1], o[2], o[3]);
}

#define VPF_REDUCE_LAUNCH(E)                                                                                 \
    hipLaunchKernelGGL(k_splitk_reduce<E>, rg, dim3(256), 0, s, partial_ws, splits, m, n, bias, st, colsum, R, Cb, ldc, \
                       stats_out)

VPF_API int vpf_gemm_bf16_splitk(const uint16_t* A, int64_t lda, const uint16_t* W, const float* bias,
                                 const uint16_t* residual, const float* row_stats, const float* colsum, uint16_t* C,
                                 int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue, int splits,
                                 float* stats_out, float* partial_ws, int64_t ws_elems, void* stream) {
    const bool ln = epilogue == VPF_EPI_LN || epilogue == VPF_EPI_LN_GELU;
    if (splits < 1 || splits > 64) return VPF_ERR_ARG;
    // the reduce kernel reads bias / colsum (and, LN, the {mean, rstd} pairs) with plain loads: nothing is DMA'd
    const int64_t tiles = vpf_gemm_check(M, N, K, (int64_t)splits * BK, lda, 8, 2, true, ldc, nullptr, nullptr,
                                         ln ? row_stats : nullptr);
    if (!tiles || tiles > 65535 * 256) return VPF_ERR_ARG;
    if (!A || !W || !bias || !C || !partial_ws || ws_elems < (int64_t)splits * M * N) return VPF_ERR_ARG;
    if (((uintptr_t)partial_ws & 15) || ((uintptr_t)C & 15) || ((uintptr_t)A & 15) || ((uintptr_t)W & 15))
        return VPF_ERR_ARG;
    if (ln && (!row_stats || !colsum)) return VPF_ERR_ARG;
    if (epilogue == VPF_EPI_BIAS_RESIDUAL && (!residual || ((uintptr_t)residual & 15))) return VPF_ERR_ARG;
    if (stats_out && (epilogue != VPF_EPI_BIAS_RESIDUAL || N % 64 != 0 || ((uintptr_t)stats_out & 7)))
        return VPF_ERR_ARG;
    if (epilogue != VPF_EPI_BIAS && epilogue != VPF_EPI_BIAS_GELU && epilogue != VPF_EPI_BIAS_RESIDUAL && !ln)
        return VPF_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int m = (int)M, n = (int)N, k = (int)K;
    const Out8 o8{nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL((k_gemm_bf16<VPF_EPI_BIAS, false, false, true>),
                       dim3((unsigned)tiles, (unsigned)splits), dim3(NTHREADS), 0, s, reinterpret_cast<const bf16_t*>(A),
                       (int)lda, reinterpret_cast<const bf16_t*>(W), nullptr, nullptr, nullptr, 1, nullptr, nullptr,
                       reinterpret_cast<bf16_t*>(partial_ws), n, m, n, k, vpf_gemm_tile_group(), 0, 0.f, nullptr, m, o8);
    const int e = (int)hipGetLastError();
    if (e) return e;
    const int64_t threads = M * (N / 8);
    const dim3 rg((unsigned)((threads + 255) / 256));
    const float2* st = reinterpret_cast<const float2*>(row_stats);
    const bf16_t* R = reinterpret_cast<const bf16_t*>(residual);
    bf16_t* Cb = reinterpret_cast<bf16_t*>(C);
    switch (epilogue) {   // stats_out is null unless EPI_BIAS_RESIDUAL (checked above)
        case VPF_EPI_BIAS: VPF_REDUCE_LAUNCH(VPF_EPI_BIAS); break;
        case VPF_EPI_BIAS_GELU: VPF_REDUCE_LAUNCH(VPF_EPI_BIAS_GELU); break;
        case VPF_EPI_BIAS_RESIDUAL: VPF_REDUCE_LAUNCH(VPF_EPI_BIAS_RESIDUAL); break;
        case VPF_EPI_LN: VPF_REDUCE_LAUNCH(VPF_EPI_LN); break;
        default: VPF_REDUCE_LAUNCH(VPF_EPI_LN_GELU); break;
    }
    VPF_RETURN_LAUNCH();
}
