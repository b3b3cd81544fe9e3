// Pieces shared by the bf16 GEMM (gemm_bf16.hip) and the MX-fp8 GEMM (gemm_mx8.hip): tile geometry, the
// XCD-aware tile order, the GELU, the MX (OCP e4m3 + e8m0 block scale) quantiser, the epilogue-operand DMA and
// {mean, rstd} combine, the per-wave epilogues and the kernel tail that dispatches to them, and the host argument checks.
#pragma once
#include "vpf_common.h"
#include "mx8.h"
#include "../../include/vpf.h"

// host helpers defined in gemm_bf16.hip, shared with gemm_mx8.hip
int vpf_gemm_tile_group();
int vpf_gemm_tile_group_mx8(int epilogue);
int vpf_check_out8(const uint8_t* C8, int64_t ld8, const uint32_t* Cs, int64_t lds_c, int64_t rows, int64_t N);
int64_t vpf_gemm_check(int64_t M, int64_t N, int64_t K, int64_t k_unit, int64_t lda, int a_align, int a_bytes,
                       bool has_c, int64_t ldc, const float* bias, const float* colsum, const float* row_stats);

namespace vpf {
namespace gemm {

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// LDS fragment reads as inline asm: with LDS-DMA writes of other ring slots in flight, hipcc's waitcnt pass
// cannot prove the reads independent and drains vmcnt(0) before them (losing the lookahead); kernels that use
// these wait for them themselves (s_waitcnt lgkmcnt(0) tied to the fragment registers).
__device__ __forceinline__ i32x4 lds16(const char* p) {
    i32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"((uint32_t)(uintptr_t)(lptr_t)p));
    return v;
}
typedef int i32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ i32x2 lds8(const void* p) {
    i32x2 v;
    asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"((uint32_t)(uintptr_t)(lptr_t)p));
    return v;
}
__device__ __forceinline__ int lds4(const void* p) {
    int v;
    asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"((uint32_t)(uintptr_t)(lptr_t)p));
    return v;
}
// the lane id through an opaque asm: values derived from it cannot be hoisted above the statement
__device__ __forceinline__ int opaque_lane() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int BM = 256, BN = 256;
constexpr int NTHREADS = 512;
constexpr int TILE_BYTES = BM * 128;       // one operand K-tile: 256 rows x 128 B (bf16 BK = 64 / fp8 BK = 128)

// 16-B global store with the non-temporal hint (global_store_dwordx4 ... nt): for an output tile that no later tile of
// this launch reads (the next kernel reads it from HBM anyway), so its lines need not displace the A / W panels the
// XCD's other tiles re-read from L2. Used by store_wave_tile_pipe's non-residual epilogues (whole 128-B rows per
// instruction): QKV -2.0 / -1.1 % in two same-process A/Bs; on the residual epilogues (proj, FC2) level, and on FC1's
// direct stores (16 half rows per instruction) +4.3 %, so those keep the default policy
// (profiles/r6_lab/gemm_ntstore_ab.txt, gemm_ntpipe_ab.txt).
typedef unsigned u32x4_nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st16_nt(void* p, uint4 v) {
    __builtin_nontemporal_store(u32x4_nt{v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4_nt*>(p));
}

// Workgroup -> output tile: XCD-aware bijective remap (cdna_hip_programming.md §5 T1) — consecutive blocks
// of one XCD get consecutive logical ids — then a grouped order inside each XCD's range: groups of `group`
// A row-panels with the A panel index running fastest, so the ~32 tiles an XCD has in flight cover ~group A
// panels x 32/group W panels and both stay in that XCD's L2 (profiles/r1_gemm_lab/group_sweep.txt).
// group = 0: plain tm-major.
// logical tile id -> output tile origin (the grouped order described above)
__device__ __forceinline__ void tile_of_lid(int M, int N, int group, int lid, int& m0, int& n0) {
    const int tiles_n = (N + BN - 1) / BN;
    int tm, tn;
    if (group > 0) {
        const int tiles_m = (M + BM - 1) / BM;
        const int per_group = group * tiles_n;
        const int g = lid / per_group, idx = lid - g * per_group;
        const int gm0 = g * group;
        const int gsz = min(group, tiles_m - gm0);
        tn = idx / gsz;
        tm = gm0 + (idx - tn * gsz);
    } else {
        tm = lid / tiles_n;
        tn = lid - tm * tiles_n;
    }
    m0 = tm * BM;
    n0 = tn * BN;
}
// block bid of nwg -> logical tile id: XCD xcd = bid & 7 owns the contiguous range of ids that starts at xcd_first
__device__ __forceinline__ int xcd_first(int nwg, int xcd) {
    const int q = nwg >> 3, r = nwg & 7;
    return xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
}
__device__ __forceinline__ void tile_of(int M, int N, int group, int& m0, int& n0) {
    const int nwg = gridDim.x, bid = blockIdx.x;
    tile_of_lid(M, N, group, xcd_first(nwg, bid & 7) + (bid >> 3), m0, n0);
}

// bf16-path GELU, two values at a time: x * sigmoid(x (a + b x^2)) = x / (1 + 2^(x (c1 + c2 x^2))), with (a, b)
// the minimax fit to the exact-erf GELU over [-10, 10] (a = 1.6003142, b = 0.0694018; the tanh form's
// a = 2 sqrt(2/pi), b = 0.044715 a has 4.7e-4): max |error| 2.7e-4, an eighth of the bf16 half-ulp at |y| = 1.
// 9 instructions per pair (3 packed mul/fma, 2 v_exp_f32, 1 packed add, 2 v_rcp_f32, 1 packed mul) against
// ~21 + hazard nops for an erf polynomial. x -> -inf: 2^(+inf) = inf, rcp = 0, y = -0; x -> +inf: y = x.
__device__ __forceinline__ f32x2 gelu_sig2(f32x2 x) {
    constexpr float L2E = 1.4426950408889634f;
    constexpr float c1 = -1.6003141571059616f * L2E, c2 = -0.06940178687219423f * L2E;
    const f32x2 q = (x * x) * c2 + c1;
    const f32x2 t = x * q;
    const f32x2 d = f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)} + 1.0f;
    return x * f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
}

// Optional MX-fp8 copy of a GEMM's bf16 output (the A operand of a following MX8 GEMM).
struct Out8 {
    uint8_t* q;      // elements, row stride ldq bytes (null: no fp8 output)
    uint8_t* s;      // scale planes as bytes (mx8_scale_byte)
    int ldq, lds;
};

constexpr bool epi_is_ln(int epi) { return epi == VPF_EPI_LN || epi == VPF_EPI_LN_GELU; }
constexpr bool epi_is_gelu(int epi) { return epi == VPF_EPI_BIAS_GELU || epi == VPF_EPI_LN_GELU; }

// ---- epilogue operands: LDS region `aux` = bias (1 KiB) | colsum (1 KiB) | row statistics planes (2 KiB each) ----
// They ride the DMA stream into LDS, so their latency hides under the K loop and nothing epilogue-related stays live in
// VGPRs across it (holding them in registers cost ~10 % on the LayerNorm-folded GEMMs: 250 VGPRs). Out-of-range columns
// / rows read clamped (valid) addresses; their values are never stored. They must land before a barrier that every wave
// passes ahead of the epilogue: one wave DMAs the bias, the next the colsum, all of them the planes, and every wave
// reads all of them. Each kernel issues them where its counted vmcnt waits expect them. Used by the two bf16 kernels
// (bias from wave 0, colsum from wave 1); k_gemm_mx8 carries its own copy with waves 2 / 3 (see there).
template <bool LN>
__device__ __forceinline__ void dma_bias_colsum(char* aux, const float* __restrict__ bias,
                                                const float* __restrict__ colsum, int n0, int N, int wid, int lane) {
    if (wid == 0)
        __builtin_amdgcn_global_load_lds((gptr_t)(bias + min(n0 + lane * 4, N - 4)), (lptr_t)aux, 16, 0, 0);
    if constexpr (LN) {
        if (wid == 1)
            __builtin_amdgcn_global_load_lds((gptr_t)(colsum + min(n0 + lane * 4, N - 4)), (lptr_t)(aux + 1024), 16, 0, 0);
    }
}
// stats_parts == 0: one {mean, rstd} plane; else stats_parts {sum, sumsq} planes of M rows each. A plane's 256-row
// slice is 2 KiB = two 16-B-per-lane pieces (M even, 16-B aligned base), dealt round-robin over the 8 waves (12
// planes: 3 pieces per wave instead of 12 4-B pieces); otherwise one 4-B-per-lane piece per plane and wave.
__device__ __forceinline__ void dma_planes(char* dst, const float2* __restrict__ stats, int stats_parts, int m0, int M,
                                           int wid, int lane) {
    const float* sd = reinterpret_cast<const float*>(stats);
    const int planes = stats_parts > 0 ? stats_parts : 1;
    if ((M & 1) == 0 && ((uintptr_t)sd & 15) == 0) {
        for (int pc = wid; pc < 2 * planes; pc += 8) {
            const int p = pc >> 1, hf = pc & 1;
            __builtin_amdgcn_global_load_lds(
                (gptr_t)(sd + (int64_t)p * 2 * M + min(2 * m0 + hf * 256 + lane * 4, 2 * M - 4)),
                (lptr_t)(dst + p * 2048 + hf * 1024), 16, 0, 0);
        }
    } else {
        for (int p = 0; p < planes; ++p)
            __builtin_amdgcn_global_load_lds(
                (gptr_t)(sd + (int64_t)p * 2 * M + min(2 * m0 + wid * 64 + lane, 2 * M - 1)),
                (lptr_t)(dst + p * 2048 + wid * 256), 4, 0, 0);
    }
}
// statistics planes -> {mean, rstd} once per row (into aux + 2048: in place over plane 0, which only this thread
// reads, unless the planes sit elsewhere), instead of in each of the 4 waves that share the row. The planes have landed
// for every wave (the kernel's last K-step barrier, or its own barrier); the barrier of the kernel tail publishes the result.
__device__ __forceinline__ void combine_planes(const char* planes_lds, char* aux, int stats_parts, int K, float ln_eps,
                                               int tid) {
    if (stats_parts > 0 && tid < BM) {
        float sm = 0.f, sq = 0.f;
        for (int p = 0; p < stats_parts; ++p) {
            const float2 st = *reinterpret_cast<const float2*>(planes_lds + p * 2048 + tid * 8);
            sm += st.x;
            sq += st.y;
        }
        const float inv_k = 1.0f / (float)K;
        const float mean = sm * inv_k;
        const float var = fmaxf(fmaf(sq, inv_k, -mean * mean), 0.f);
        *reinterpret_cast<float2*>(aux + 2048 + tid * 8) = make_float2(mean, __builtin_amdgcn_rsqf(var + ln_eps));
    }
}

// ---- fragment math: one accumulator fragment (4 consecutive columns of one row) -> 4 bf16 ----
struct EpiCols { float4 b, c; };        // bias and (LN) colsum of the fragment's 4 columns
struct EpiRow { f32x2 rstd, nrm; };     // LN: {rstd, rstd}, {-rstd mean, -rstd mean} of the fragment's row
struct Frag4 { f32x2 lo, hi; };         // the fragment's 4 epilogue values in fp32
// `col`: first column within the tile; `row`: row within the tile
template <bool LN>
__device__ __forceinline__ EpiCols epi_cols(const char* aux, int col) {
    EpiCols v;
    v.b = *reinterpret_cast<const float4*>(aux + col * 4);
    v.c = LN ? *reinterpret_cast<const float4*>(aux + 1024 + col * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    return v;
}
template <bool LN>
__device__ __forceinline__ EpiRow epi_row(const char* aux, int row) {
    if constexpr (LN) {
        const float2 st = *reinterpret_cast<const float2*>(aux + 2048 + row * 8);
        return EpiRow{f32x2{st.y, st.y}, f32x2{-st.y * st.x, -st.y * st.x}};
    } else {
        return EpiRow{f32x2{1.f, 1.f}, f32x2{0.f, 0.f}};
    }
}
// bias, or the LN fold LN(x) W^T + b = rstd (x W'^T) - rstd mean colsum(W') + b' (gamma folded into W', beta into b'),
// then the GELU epilogues' gelu_sig2, in fp32
template <int EPI>
__device__ __forceinline__ Frag4 epi_math4(const f32x4& a, const EpiCols& cl, const EpiRow& rw) {
    f32x2 v01, v23;
    const f32x2 a01 = {a[0], a[1]}, a23 = {a[2], a[3]};
    const f32x2 b01 = {cl.b.x, cl.b.y}, b23 = {cl.b.z, cl.b.w};
    if constexpr (epi_is_ln(EPI)) {
        const f32x2 c01 = {cl.c.x, cl.c.y}, c23 = {cl.c.z, cl.c.w};
        v01 = __builtin_elementwise_fma(rw.rstd, a01, __builtin_elementwise_fma(rw.nrm, c01, b01));
        v23 = __builtin_elementwise_fma(rw.rstd, a23, __builtin_elementwise_fma(rw.nrm, c23, b23));
    } else {
        v01 = a01 + b01;
        v23 = a23 + b23;
    }
    if constexpr (epi_is_gelu(EPI)) {
        v01 = gelu_sig2(v01);
        v23 = gelu_sig2(v23);
    }
    return Frag4{v01, v23};
}
__device__ __forceinline__ uint2 pack_bf4(const Frag4& v) {   // round-to-nearest-even
    return make_uint2(pack_bf2(v.lo.x, v.lo.y), pack_bf2(v.hi.x, v.hi.y));
}
template <int EPI>
__device__ __forceinline__ uint2 epi_pack4(const f32x4& a, const EpiCols& cl, const EpiRow& rw) {
    return pack_bf4(epi_math4<EPI>(a, cl, rw));
}

// ---- the wave's LDS image: 128 rows x 128 B, the 8-B chunk c8 of row r at chunk c8 ^ (r & 15) ----
template <int EPI>
__device__ __forceinline__ void epi_to_image4(char* img, int row, int c8, const f32x4& a, const EpiCols& cl,
                                              const EpiRow& rw) {
    const Frag4 v = epi_math4<EPI>(a, cl, rw);
    const int c = c8 ^ (row & 15);
    *reinterpret_cast<uint2*>(img + row * 128 + c * 8) = pack_bf4(v);
}
// 8 consecutive columns (16-B chunk c16) of a row; `odd` = row & 1 (the swizzle swaps the 8-B halves of odd rows)
__device__ __forceinline__ uint4 image_get16(const char* img, int row, int c16, bool odd) {
    uint4 v = *reinterpret_cast<const uint4*>(img + row * 128 + ((c16 ^ ((row & 15) >> 1)) * 16));
    if (odd) { const uint32_t t0 = v.x, t1 = v.y; v.x = v.z; v.y = v.w; v.z = t0; v.w = t1; }
    return v;
}

// ---- helpers on 8 packed bf16 values (a lane's 16 B of an output row) ----
// v + r per value in fp32, rounded to bf16 again: the residual add on the stored (already rounded) values
__device__ __forceinline__ uint4 add_bf16x8(uint4 v, uint4 r) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        o[e] = pack_bf2(bf2f((bf16_t)(w[e] & 0xffff)) + bf2f((bf16_t)(rr[e] & 0xffff)),
                        bf2f((bf16_t)(w[e] >> 16)) + bf2f((bf16_t)(rr[e] >> 16)));
    return make_uint4(o[0], o[1], o[2], o[3]);
}
// Row statistics of the stored values, step 1: {sum, sumsq} of the lane's 8 values by v_dot2_f32_bf16 on the packed
// pairs (sum = dot(w, (1, 1)), sumsq = dot(w, w); bf16 products are exact in fp32), parked in the image row the values
// were just read from (8 B at c16 * 8; the whole row was read by this same instruction and LDS ops of one wave stay in
// order). Lanes out of range park zeros.
__device__ __forceinline__ void park_row_partial(char* img, int row, int c16, uint4 v, bool ok) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const bf16x2_t one2 = __builtin_bit_cast(bf16x2_t, 0x3F803F80u);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bf16x2_t pr = __builtin_bit_cast(bf16x2_t, w[e]);
        s1 = __builtin_amdgcn_fdot2_f32_bf16(pr, one2, s1, false);
        s2 = __builtin_amdgcn_fdot2_f32_bf16(pr, pr, s2, false);
    }
    if (!ok) { s1 = 0.f; s2 = 0.f; }
    *reinterpret_cast<float2*>(img + row * 128 + c16 * 8) = make_float2(s1, s2);
}
// Step 2: each lane sums the 8 parked partials (64 B at the row start) of rows 2 lane, 2 lane + 1 and stores them to
// plane nb / 64 (plane stride stats_rows rows) with one 16-B store; no cross-wave step. mw / nb: the wave tile's first
// row / column. PATCH: output row = token row (one CLS row per g2 patch rows), so the two rows are stored apart.
template <bool PATCH>
__device__ __forceinline__ void store_row_stats(const char* img, float* stats_out, int stats_rows, int mw, int nb,
                                                int lane, int M, int N, int g2) {
    if (stats_out != nullptr && nb < N) {   // wave-uniform
        __builtin_amdgcn_wave_barrier();
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 u0 = *reinterpret_cast<const float4*>(img + (2 * lane) * 128 + q * 16);
            const float4 u1 = *reinterpret_cast<const float4*>(img + (2 * lane + 1) * 128 + q * 16);
            t.x += u0.x + u0.z; t.y += u0.y + u0.w;
            t.z += u1.x + u1.z; t.w += u1.y + u1.w;
        }
        float* plane = stats_out + (int64_t)(nb >> 6) * stats_rows * 2;
        const int m = mw + 2 * lane;
        if constexpr (PATCH) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int me = m + e;
                if (me < M) {
                    const int64_t orow = (int64_t)(me / g2) * (g2 + 1) + 1 + me % g2;
                    *reinterpret_cast<float2*>(plane + orow * 2) = e ? make_float2(t.z, t.w) : make_float2(t.x, t.y);
                }
            }
        } else {
            if (m + 1 < M) *reinterpret_cast<float4*>(plane + (int64_t)m * 2) = t;
            else if (m < M) *reinterpret_cast<float2*>(plane + (int64_t)m * 2) = make_float2(t.x, t.y);
        }
    }
}
// One MX scale word of the wave tile (mx8_scale_byte's layout: plane nb / 128, 64-row bricks, per brick 4 K-blocks x 16
// words, byte f of word r16 = row 16 f + r16 of the brick): the word of brick `brick` (0 / 1 of the wave's 128 rows),
// 32-column block `blk` (0 / 1 of its 64 columns), row r16. Only bricks that hold an output row (R < M <= lds) are
// stored: the words of later bricks of a longer plane belong to whoever owns those rows.
__device__ __forceinline__ void store_scale_word(Out8 o8, uint32_t word, int mw, int nb, int M, int N, int brick,
                                                 int blk, int r16) {
    const int R = mw + brick * 64;   // brick row base
    if (nb < N && R < M)
        reinterpret_cast<uint32_t*>(o8.s)[(int64_t)(nb >> 7) * o8.lds + R + (((nb >> 5) & 3) + blk) * 16 + r16] = word;
}

// ---- per-wave epilogues of one wave's 128 (M) x 64 (N) sub-tile ----
// `img` is this wave's private 16 KiB of LDS (free of any operand the other waves still read), `aux` the
// epilogue-operand region (bias | colsum at column offset wn*64 of the tile, row statistics at row offset wm*128).
// Bias / LN-fold / GELU in fp32 on the accumulators, bf16 pack (epi_pack4), 8-B writes into the XOR-swizzled image,
// then 16-B coalesced row stores (+ residual / position-embedding adds on the packed values). C may be null when only
// the fp8 copy is wanted.
// `stats_out` (may be null): for the producers of the residual stream (EPI_BIAS_RESIDUAL, EPI_PATCH) the per-row
// {sum, sumsq} of the stored bf16 values over the wave's 64 columns go to plane n0/64 + wn (park_row_partial,
// store_row_stats).
// OUT8: the same bf16 values are also MX-quantised (mx8_quant8: a 32-column block is one DPP quad of lanes)
// and stored as 8-B element pieces plus one scale byte per row and block.
template <int EPI>
__device__ __forceinline__ void epi_to_image(char* img, const char* aux, const f32x4 (&acc)[4][8], int wm, int wn,
                                             int lane) {
    constexpr bool LN = epi_is_ln(EPI);
    const int fr = lane & 15, fq = lane >> 4;
    EpiCols cl[4];
    EpiRow rw[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) cl[j] = epi_cols<LN>(aux, wn * 64 + j * 16 + fq * 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) rw[i] = epi_row<LN>(aux, wm * 128 + i * 16 + fr);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 8; ++i) epi_to_image4<EPI>(img, i * 16 + fr, j * 4 + fq, acc[j][i], cl[j], rw[i]);
    }
}

// Pipelined form of epi_to_image + store_wave_tile for the epilogues with a bf16 output only (EPI_BIAS / BIAS_GELU /
// LN / LN_GELU / BIAS_RESIDUAL with its statistics planes): fragment row-group i's math and image rows, then that
// group's two 16-B store iterations, so the stores start after the first 16 rows instead of after all 128 and drain
// under the remaining math. Same image layout as the two-pass form (bit-identical output).
// Store iteration h of group i covers the group's rows of parity h (rows i*16 + 2*(lane/8) + h; still 8 rows x 128 B
// per instruction), so the 8-B half swap that the image swizzle applies to odd rows is resolved at compile time instead
// of by 4 v_cndmask per chunk, and stores / residual loads address from one per-lane base pointer plus a wave-uniform
// row offset instead of a 64-bit multiply-add each (profiles/r2_gemm_lab/epilogue_parity_rows_ab.txt).
template <int EPI>
__device__ __forceinline__ void store_wave_tile_pipe(char* img, const char* aux, const f32x4 (&acc)[4][8], int wm,
                                                     int wn, int m0, int n0, int lane, const uint4 (&res)[16],
                                                     bf16_t* C, int ldc, int M, int N, float* stats_out,
                                                     int stats_rows) {
    constexpr bool LN = epi_is_ln(EPI);
    constexpr bool RES = EPI == VPF_EPI_BIAS_RESIDUAL;
    const int fr = lane & 15, fq = lane >> 4, c16 = lane & 7;
    // the lane's store pointer at row offset 0 of the wave tile (only dereferenced where ok)
    bf16_t* Cl = C + (int64_t)(m0 + wm * 128 + 2 * (lane >> 3)) * ldc + (n0 + wn * 64 + c16 * 8);
    EpiCols cl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cl[j] = epi_cols<LN>(aux, wn * 64 + j * 16 + fq * 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const EpiRow rw = epi_row<LN>(aux, wm * 128 + i * 16 + fr);
#pragma unroll
        for (int j = 0; j < 4; ++j) epi_to_image4<EPI>(img, i * 16 + fr, j * 4 + fq, acc[j][i], cl[j], rw);
        __builtin_amdgcn_wave_barrier();   // the image is private to this wave: LDS ops of one wave stay in order
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = i * 16 + 2 * (lane >> 3) + h;   // rows of group i only
            uint4 v = image_get16(img, row, c16, h == 1);
            const int m = m0 + wm * 128 + row;
            const int n = n0 + wn * 64 + c16 * 8;
            const bool ok = m < M && n < N;
            if constexpr (RES) {
                // add_bf16x8 and, below, store_row_stats<false>, written out: as calls they move two MFMAs of
                // k_gemm_bf16<EPI_BIAS_RESIDUAL>'s K loop (proj / FC2) past a DMA address add (hipcc's register
                // assignment of the accumulators follows the epilogue's block order; tools/kdiff.py)
                const uint4 rv = res[2 * i + h];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                const uint32_t rr[4] = {rv.x, rv.y, rv.z, rv.w};
                uint32_t o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    o[e] = pack_bf2(bf2f((bf16_t)(w[e] & 0xffff)) + bf2f((bf16_t)(rr[e] & 0xffff)),
                                    bf2f((bf16_t)(w[e] >> 16)) + bf2f((bf16_t)(rr[e] >> 16)));
                v = make_uint4(o[0], o[1], o[2], o[3]);
                if (stats_out != nullptr) park_row_partial(img, row, c16, v, ok);   // wave-uniform
            }
            if (ok) {
                if constexpr (RES) *reinterpret_cast<uint4*>(Cl + (int64_t)(i * 16 + h) * ldc) = v;
                else st16_nt(Cl + (int64_t)(i * 16 + h) * ldc, v);
            }
        }
    }
    if constexpr (RES) {
        const int nb = n0 + wn * 64;
        if (stats_out != nullptr && nb < N) {   // wave-uniform: rows 2 lane, 2 lane + 1, 8 partials each
            __builtin_amdgcn_wave_barrier();
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 u0 = *reinterpret_cast<const float4*>(img + (2 * lane) * 128 + q * 16);
                const float4 u1 = *reinterpret_cast<const float4*>(img + (2 * lane + 1) * 128 + q * 16);
                t.x += u0.x + u0.z; t.y += u0.y + u0.w;
                t.z += u1.x + u1.z; t.w += u1.y + u1.w;
            }
            float* plane = stats_out + (int64_t)(nb >> 6) * stats_rows * 2;
            const int m = m0 + wm * 128 + 2 * lane;
            if (m + 1 < M) *reinterpret_cast<float4*>(plane + (int64_t)m * 2) = t;
            else if (m < M) *reinterpret_cast<float2*>(plane + (int64_t)m * 2) = make_float2(t.x, t.y);
        }
    }
}

// store_wave_tile_pipe for k_gemm_walk's EPI_LN (QKV): the operand ring is being refilled for the next tile while the
// epilogue runs, so the wave's image is one 16-row group (2 KiB at `img`, outside the ring) reused by the 8 row groups:
// group i's rows sit at image rows (row & 15), where the swizzle (a function of row & 15 only) puts the same chunks
// as in the 16 KiB image. LDS operations of one wave stay in order, so group i + 1's writes cannot pass group i's
// reads. Every LDS access is asm (DMA_LIVE, see store_wave_tile_direct): the epilogue operands up front, then per
// group [math, 4 image writes, lgkmcnt(0), the previous group's two 16-B stores, this group's two image reads], so a
// group's reads land under the next group's math. Same values and stores as store_wave_tile_pipe: bit-identical.
__device__ __forceinline__ void lds_write8(const void* p, uint2 v) {
    const i32x2 w = {(int)v.x, (int)v.y};
    asm volatile("ds_write_b64 %0, %1" ::"v"((uint32_t)(uintptr_t)(lptr_t)p), "v"(w) : "memory");
}
template <int EPI>
__device__ __forceinline__ void store_wave_tile_group(char* img, const char* aux, const f32x4 (&acc)[4][8], int wm,
                                                      int wn, int m0, int n0, int lane, bf16_t* C, int ldc, int M,
                                                      int N) {
    static_assert(EPI == VPF_EPI_LN, "group image: the LN fold without GELU (QKV)");
    const int fr = lane & 15, fq = lane >> 4, c16 = lane & 7, r8 = lane >> 3;
    bf16_t* Cl = C + (int64_t)(m0 + wm * 128 + 2 * r8) * ldc + (n0 + wn * 64 + c16 * 8);
    i32x4 cb[4], cc[4];
    i32x2 st[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = wn * 64 + j * 16 + fq * 4;
        cb[j] = lds16(aux + col * 4);
        cc[j] = lds16(aux + 1024 + col * 4);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = lds8(aux + 2048 + (wm * 128 + i * 16 + fr) * 8);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cb[0]), "+v"(cb[1]), "+v"(cb[2]), "+v"(cb[3])::"memory");
    asm volatile("" : "+v"(cc[0]), "+v"(cc[1]), "+v"(cc[2]), "+v"(cc[3])::"memory");
    asm volatile("" : "+v"(st[0]), "+v"(st[1]), "+v"(st[2]), "+v"(st[3]), "+v"(st[4]), "+v"(st[5]), "+v"(st[6]),
                   "+v"(st[7])::"memory");
    EpiCols cl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cl[j] = EpiCols{__builtin_bit_cast(float4, cb[j]), __builtin_bit_cast(float4, cc[j])};
    // image addresses: writes row fr, 8-B chunk (j*4 + fq) ^ fr; reads row 2 r8 + h, 16-B chunk c16 ^ r8
    const char* wr = img + fr * 128;
    const char* rd = img + (2 * r8) * 128 + ((c16 ^ r8) << 4);
    const int n = n0 + wn * 64 + c16 * 8;
    i32x4 pend[2];
    auto store_group = [&](int i) {   // group i's rows of parity h: the 8-B halves of odd rows are swapped back
        asm volatile("" : "+v"(pend[0]), "+v"(pend[1])::"memory");
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint4 v = __builtin_bit_cast(uint4, pend[h]);
            if (h == 1) { const uint32_t t0 = v.x, t1 = v.y; v.x = v.z; v.y = v.w; v.z = t0; v.w = t1; }
            const int m = m0 + wm * 128 + i * 16 + 2 * r8 + h;
            if (m < M && n < N) st16_nt(Cl + (int64_t)(i * 16 + h) * ldc, v);
        }
    };
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float2 s2 = __builtin_bit_cast(float2, st[i]);   // epi_row's expressions
        const EpiRow rw = EpiRow{f32x2{s2.y, s2.y}, f32x2{-s2.y * s2.x, -s2.y * s2.x}};
        uint2 pk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pk[j] = epi_pack4<EPI>(acc[j][i], cl[j], rw);
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_write8(wr + (((j * 4 + fq) ^ fr) << 3), pk[j]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (i > 0) store_group(i - 1);
        pend[0] = lds16(rd);
        pend[1] = lds16(rd + 128);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    store_group(7);
}

// store_wave_tile_group for k_gemm_walk_res (EPI_BIAS_RESIDUAL: proj, FC2): the same reused 16-row group image and the
// same asm LDS accesses, then per 16-B piece store_wave_tile_pipe's residual add on the rounded values (add_bf16x8
// with res[2 i + h], load_residual<true>'s order), a plain 16-B store (no nt hint: level or worse on these epilogues,
// profiles/r6_lab), and the statistics planes of the stored values.
// Planes: the 2 KiB image is rewritten by the next group before this group's values exist, so the 8 partials of a row
// cannot be parked in it as park_row_partial does in the 16 KiB image. They are summed per group in registers instead:
// the lanes 8 r8 .. 8 r8 + 7 hold p0 .. p7 of row 2 r8 + h, and lane 8 r8 forms store_row_stats's sum,
// t = 0; t += p0 + p1; t += p2 + p3; t += p4 + p5; t += p6 + p7, with DPP row shifts inside its 16-lane row (p + p
// of the next lane, then that pair sum of lanes +2, +4, +6), so the bits are store_row_stats's. It stores rows
// 2 r8, 2 r8 + 1 as one 16-B piece: a group's 16 rows are 128 contiguous bytes of the plane.
// `res` was loaded before the epilogue (the kernel issues load_residual right behind its last MFMA quadrant): with the
// next tile's LDS-DMA in flight hipcc drains vmcnt(0) at the first use of a plain load's result, here in group 0's
// stores, which retires the prefetched half-tiles (older, and needed right after the epilogue) and all 16 pieces at
// once; nothing later in the epilogue waits on vmcnt.
__device__ __forceinline__ float2 row_partial8(uint4 v, bool ok) {   // park_row_partial's {sum, sumsq} of 8 values
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const bf16x2_t one2 = __builtin_bit_cast(bf16x2_t, 0x3F803F80u);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bf16x2_t pr = __builtin_bit_cast(bf16x2_t, w[e]);
        s1 = __builtin_amdgcn_fdot2_f32_bf16(pr, one2, s1, false);
        s2 = __builtin_amdgcn_fdot2_f32_bf16(pr, pr, s2, false);
    }
    if (!ok) { s1 = 0.f; s2 = 0.f; }
    return make_float2(s1, s2);
}
// the value of lane + N inside the 16-lane DPP row (row_shl:N; 0 past the row's end, which no result lane reads)
template <int SHL>
__device__ __forceinline__ float dpp_row_shl(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x100 + SHL, 0xF, 0xF, true));
}
// lanes 8 k .. 8 k + 7 hold p0 .. p7: at lane 8 k, store_row_stats's sum of the eight (other lanes: not a row sum)
__device__ __forceinline__ float row8_sum(float p) {
    const float q = p + dpp_row_shl<1>(p);   // even lanes: p0 + p1, p2 + p3, ...
    float t = 0.f;
    t += q;
    t += dpp_row_shl<2>(q);
    t += dpp_row_shl<4>(q);
    t += dpp_row_shl<6>(q);
    return t;
}
__device__ __forceinline__ void store_wave_tile_group_res(char* img, const char* aux, const f32x4 (&acc)[4][8], int wm,
                                                          int wn, int m0, int n0, int lane, const uint4 (&res)[16],
                                                          bf16_t* C, int ldc, int M, int N, float* stats_out,
                                                          int stats_rows) {
    constexpr int EPI = VPF_EPI_BIAS_RESIDUAL;
    const int fr = lane & 15, fq = lane >> 4, c16 = lane & 7, r8 = lane >> 3;
    bf16_t* Cl = C + (int64_t)(m0 + wm * 128 + 2 * r8) * ldc + (n0 + wn * 64 + c16 * 8);
    i32x4 cb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cb[j] = lds16(aux + (wn * 64 + j * 16 + fq * 4) * 4);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cb[0]), "+v"(cb[1]), "+v"(cb[2]), "+v"(cb[3])::"memory");
    EpiCols cl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cl[j] = EpiCols{__builtin_bit_cast(float4, cb[j]), make_float4(0.f, 0.f, 0.f, 0.f)};
    const EpiRow rw = EpiRow{f32x2{1.f, 1.f}, f32x2{0.f, 0.f}};
    // image addresses: writes row fr, 8-B chunk (j*4 + fq) ^ fr; reads row 2 r8 + h, 16-B chunk c16 ^ r8
    const char* wr = img + fr * 128;
    const char* rd = img + (2 * r8) * 128 + ((c16 ^ r8) << 4);
    const int n = n0 + wn * 64 + c16 * 8;
    const int nb = n0 + wn * 64;
    const bool planes = stats_out != nullptr && nb < N;   // wave-uniform
    // the lane's rows 2 r8, 2 r8 + 1 of group 0 in plane nb / 64 (only dereferenced by lanes c16 == 0, rows < M)
    float* pl = stats_out + ((int64_t)(nb >> 6) * stats_rows + (m0 + wm * 128 + 2 * r8)) * 2;
    i32x4 pend[2];
    auto store_group = [&](int i) {   // group i's rows of parity h: the 8-B halves of odd rows are swapped back
        asm volatile("" : "+v"(pend[0]), "+v"(pend[1])::"memory");
        const int m = m0 + wm * 128 + i * 16 + 2 * r8;   // parity 0's row
        uint4 v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            v[h] = __builtin_bit_cast(uint4, pend[h]);
            if (h == 1) { const uint32_t t0 = v[h].x, t1 = v[h].y; v[h].x = v[h].z; v[h].y = v[h].w; v[h].z = t0; v[h].w = t1; }
            v[h] = add_bf16x8(v[h], res[2 * i + h]);
            if (m + h < M && n < N) *reinterpret_cast<uint4*>(Cl + (int64_t)(i * 16 + h) * ldc) = v[h];
        }
        if (planes) {
            const float2 p0 = row_partial8(v[0], m < M && n < N), p1 = row_partial8(v[1], m + 1 < M && n < N);
            const float4 t = make_float4(row8_sum(p0.x), row8_sum(p0.y), row8_sum(p1.x), row8_sum(p1.y));
            if (c16 == 0) {
                if (m + 1 < M) *reinterpret_cast<float4*>(pl + i * 32) = t;
                else if (m < M) *reinterpret_cast<float2*>(pl + i * 32) = make_float2(t.x, t.y);
            }
        }
    };
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint2 pk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pk[j] = epi_pack4<EPI>(acc[j][i], cl[j], rw);
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_write8(wr + (((j * 4 + fq) ^ fr) << 3), pk[j]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (i > 0) store_group(i - 1);
        pend[0] = lds16(rd);
        pend[1] = lds16(rd + 128);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    store_group(7);
}

// Direct-store epilogue (no LDS image) for the GELU epilogues (FC1: EPI_LN_GELU; EPI_BIAS_GELU), bit-identical to
// store_wave_tile_pipe. The W K-tile is staged with its rows permuted inside each 32-row group: LDS row r of the B tile
// holds W row wperm(r) of the tile. Fragment j's MFMA row p then is output column (j >> 1)*32 + (p >> 2)*8 + (j & 1)*4 +
// (p & 3) of the wave's 64, so a lane's acc[2h][i] and acc[2h+1][i] are the 8 consecutive columns h*32 + fq*8 .. +7 of
// row i*16 + fr: one 16-B store straight from the accumulators (4 lanes = 64 contiguous bytes of a row, 16 rows per
// store instruction). The LDS layout and the fragment reads are unchanged (only the DMA source rows move).
// Measured in one process against the image path (profiles/r4_lab/gemm_direct_store_ab.txt, M = 806,912, outputs
// bit-identical): FC1 -1.3 %, but QKV +6.9 %, proj +3.3 %, FC2 +0.6 %. A store instruction that covers 16 half rows
// costs more than one that covers 8 whole rows, which only the VALU-bound GELU epilogue (no LDS image round trip to
// wait on) more than pays back; a DPP pair exchange that restores 8 whole rows per store costs 16 VALU per row group
// (QKV +1.2 %, FC1 -0.4 %). So only the GELU epilogues store directly.
__device__ __forceinline__ int wperm(int r) {
    return (r & ~31) | (((r >> 2) & 3) << 3) | (((r >> 4) & 1) << 2) | (r & 3);
}

// DMA_LIVE (k_gemm_walk): LDS-DMA of the next tile's operands is in flight while the epilogue runs. The epilogue
// operands are then read by asm (lds16 / lds8) behind one lgkmcnt(0) tied to their registers: at a plain LDS read
// hipcc's waitcnt pass would drain vmcnt(0) first (see lds16), and the epilogue would start by waiting for the prefetch.
template <int EPI, bool DMA_LIVE = false>
__device__ __forceinline__ void store_wave_tile_direct(const char* aux, const f32x4 (&acc)[4][8], int wm, int wn, int m0,
                                                       int n0, int lane, bf16_t* C, int ldc, int M, int N) {
    static_assert(epi_is_gelu(EPI), "direct stores: the GELU epilogues");
    constexpr bool LN = epi_is_ln(EPI);
    const int fr = lane & 15, fq = lane >> 4;
    bf16_t* Cl = C + (int64_t)(m0 + wm * 128 + fr) * ldc + (n0 + wn * 64 + fq * 8);
    EpiCols cl[4];
    EpiRow rws[8];
    if constexpr (DMA_LIVE) {
        i32x4 cb[4], cc[4];
        i32x2 st[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = wn * 64 + (j >> 1) * 32 + fq * 8 + (j & 1) * 4;
            cb[j] = lds16(aux + col * 4);
            if constexpr (LN) cc[j] = lds16(aux + 1024 + col * 4);
        }
        if constexpr (LN) {
#pragma unroll
            for (int i = 0; i < 8; ++i) st[i] = lds8(aux + 2048 + (wm * 128 + i * 16 + fr) * 8);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cb[0]), "+v"(cb[1]), "+v"(cb[2]), "+v"(cb[3])::"memory");
        if constexpr (LN) {
            asm volatile("" : "+v"(cc[0]), "+v"(cc[1]), "+v"(cc[2]), "+v"(cc[3])::"memory");
            asm volatile("" : "+v"(st[0]), "+v"(st[1]), "+v"(st[2]), "+v"(st[3]), "+v"(st[4]), "+v"(st[5]), "+v"(st[6]),
                           "+v"(st[7])::"memory");
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cl[j].b = __builtin_bit_cast(float4, cb[j]);
            cl[j].c = LN ? __builtin_bit_cast(float4, cc[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if constexpr (LN) {   // epi_row's expressions
                const float2 s2 = __builtin_bit_cast(float2, st[i]);
                rws[i] = EpiRow{f32x2{s2.y, s2.y}, f32x2{-s2.y * s2.x, -s2.y * s2.x}};
            } else {
                rws[i] = EpiRow{f32x2{1.f, 1.f}, f32x2{0.f, 0.f}};
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) cl[j] = epi_cols<LN>(aux, wn * 64 + (j >> 1) * 32 + fq * 8 + (j & 1) * 4);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        EpiRow rw;
        if constexpr (DMA_LIVE) rw = rws[i];
        else rw = epi_row<LN>(aux, wm * 128 + i * 16 + fr);
        const int m = m0 + wm * 128 + i * 16 + fr;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint2 lo = epi_pack4<EPI>(acc[2 * h][i], cl[2 * h], rw);
            const uint2 hi = epi_pack4<EPI>(acc[2 * h + 1][i], cl[2 * h + 1], rw);
            const int n = n0 + wn * 64 + h * 32 + fq * 8;
            if (m < M && n < N)
                *reinterpret_cast<uint4*>(Cl + (int64_t)(i * 16) * ldc + h * 32) = make_uint4(lo.x, lo.y, hi.x, hi.y);
        }
    }
}

// The residual rows a lane adds in store_wave_tile / store_wave_tile_pipe (EPI_BIAS_RESIDUAL): 16 x 16 B, all in flight
// at once. The kernels issue this right after their K loop, before the epilogue barrier (a raw s_barrier, so the loads
// stay in flight across it), which gives them the LN combine, the barrier and the image writes to land under.
// PAR: the row order of store_wave_tile_pipe (res[2i + h] = row i*16 + 2*(lane/8) + h), from one per-lane base
// pointer; !PAR: row it*8 + lane/8 (store_wave_tile).
template <bool PAR = true>
__device__ __forceinline__ void load_residual(uint4 (&res)[16], const bf16_t* residual, int wm, int wn, int m0,
                                              int n0, int lane, int ldc, int M, int N) {
    const int c16 = lane & 7;
    const int n = n0 + wn * 64 + c16 * 8;
    const bf16_t* rl = residual + (int64_t)(m0 + wm * 128 + (PAR ? 2 : 1) * (lane >> 3)) * ldc + n;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int roff = PAR ? (it >> 1) * 16 + (it & 1) : it * 8;
        const int m = m0 + wm * 128 + roff + (PAR ? 2 : 1) * (lane >> 3);
        res[it] = (m < M && n < N) ? *reinterpret_cast<const uint4*>(rl + (int64_t)roff * ldc) : make_uint4(0, 0, 0, 0);
    }
}

template <int EPI, bool OUT8>
__device__ __forceinline__ void store_wave_tile(char* img, const char* aux, const f32x4 (&acc)[4][8], int wm, int wn,
                                                int m0, int n0, int lane, const uint4 (&res)[16],
                                                const float* __restrict__ pos, int g2, bf16_t* C, int ldc, int M,
                                                int N, float* stats_out, int stats_rows, Out8 o8) {
    epi_to_image<EPI>(img, aux, acc, wm, wn, lane);
    const int c16 = lane & 7;
    constexpr bool PROD = (EPI == VPF_EPI_BIAS_RESIDUAL || EPI == VPF_EPI_PATCH);
    // OUT8 with output row = m (every epilogue but PATCH): the wave owns whole scale words (two 64-row bricks x
    // two K-blocks), gathered after the loop instead of one byte store per row and block
    constexpr bool GATHER8 = OUT8 && EPI != VPF_EPI_PATCH;
    uint32_t e8s[16];
    __builtin_amdgcn_wave_barrier();   // the image is private to this wave: LDS ops of one wave stay in order
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int row = it * 8 + (lane >> 3);
        uint4 v = image_get16(img, row, c16, row & 1);
        const int m = m0 + wm * 128 + row;
        const int n = n0 + wn * 64 + c16 * 8;
        const bool ok = m < M && n < N;
        int64_t orow = m;
        if constexpr (EPI == VPF_EPI_PATCH) {
            const int pi = m % g2;
            orow = (int64_t)(m / g2) * (g2 + 1) + 1 + pi;
            const float* pr = pos + (int64_t)(1 + pi) * N + min(n, N - 8);
            const float4 p0 = *reinterpret_cast<const float4*>(pr);
            const float4 p1 = *reinterpret_cast<const float4*>(pr + 4);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const float pv[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
            uint32_t o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                o[e] = pack_bf2(bf2f((bf16_t)(w[e] & 0xffff)) + pv[2 * e], bf2f((bf16_t)(w[e] >> 16)) + pv[2 * e + 1]);
            v = make_uint4(o[0], o[1], o[2], o[3]);
        }
        if constexpr (EPI == VPF_EPI_BIAS_RESIDUAL) v = add_bf16x8(v, res[it]);
        if constexpr (PROD) {
            if (stats_out != nullptr) park_row_partial(img, row, c16, v, ok);   // wave-uniform
        }
        if constexpr (OUT8) {
            // whole quads are in or out of range together (rows: a quad is one row; columns: N % 128 == 0)
            uint32_t e8;
            const uint2 q = mx8_quant8(v, e8);
            e8s[it] = e8;
            if (ok) {
                *reinterpret_cast<uint2*>(o8.q + orow * o8.ldq + n) = q;
                if (!GATHER8 && (c16 & 3) == 0) o8.s[mx8_scale_byte(orow, n, o8.lds)] = (uint8_t)e8;
            }
        }
        if (ok && C != nullptr) *reinterpret_cast<uint4*>(C + orow * ldc + n) = v;
    }
    if constexpr (GATHER8) {
        // word w = brick (w >> 5), block (w >> 4) & 1, row r16 = w & 15; byte f = rows 16f + r16 of the brick;
        // staged in bytes 64..127 of image rows 0..3 (the statistics partials use bytes 0..63)
        __builtin_amdgcn_wave_barrier();
        if ((c16 & 3) == 0) {
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int row = it * 8 + (lane >> 3);
                const int w = (row >> 6) * 32 + (c16 >> 2) * 16 + (row & 15);
                img[(w >> 4) * 128 + 64 + (w & 15) * 4 + ((row >> 4) & 3)] = (char)e8s[it];
            }
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t word = *reinterpret_cast<const uint32_t*>(img + (lane >> 4) * 128 + 64 + (lane & 15) * 4);
        store_scale_word(o8, word, m0 + wm * 128, n0 + wn * 64, M, N, lane >> 5, (lane >> 4) & 1, lane & 15);
    }
    if constexpr (PROD)
        store_row_stats<EPI == VPF_EPI_PATCH>(img, stats_out, stats_rows, m0 + wm * 128, n0 + wn * 64, lane, M, N, g2);
}

// fp8-only output straight from the accumulators (gemm_mx8.hip, FC1's LN + GELU epilogue): the MX8 kernel stages the W
// K-tile with its rows in the order wperm16 (inside each 64-row brick), so fragment j's MFMA row p is output column
// (p >> 2)*16 + j*4 + (p & 3) of the wave's 64 and a lane's acc[0..3][i] are the 16 consecutive columns fq*16 .. +15 of
// row i*16 + fr: the 32-column MX block is the lane pair fq, fq ^ 1 (one permlane16_swap), the 16 fp8 elements are one
// 16-B store (16 rows x 64 B per store instruction, as store_wave_tile_q8), and each lane assembles the scale bytes of
// its rows in registers (no LDS image). Bit-identical to store_wave_tile_q8.
__device__ __forceinline__ int wperm16(int r) {
    return (r & ~63) | (((r >> 2) & 3) << 4) | (((r >> 4) & 3) << 2) | (r & 3);
}

template <int EPI>
__device__ __forceinline__ void store_wave_tile_q8_direct(const char* aux, const f32x4 (&acc)[4][8], int wm, int wn,
                                                          int m0, int n0, int lane, int M, int N, Out8 o8) {
    static_assert(EPI == VPF_EPI_LN_GELU, "direct fp8 stores: FC1's epilogue");
    const int fr = lane & 15, fq = lane >> 4;
    EpiCols cl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cl[j] = epi_cols<true>(aux, wn * 64 + fq * 16 + j * 4);
    uint32_t word[2] = {0u, 0u};   // scale bytes of bricks 0 / 1 (byte i & 3 = rows (i & 3)*16 + fr of the brick)
    const int n = n0 + wn * 64 + fq * 16;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const EpiRow rw = epi_row<true>(aux, wm * 128 + i * 16 + fr);
        uint2 o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = epi_pack4<EPI>(acc[j][i], cl[j], rw);
        const uint4 h0 = make_uint4(o[0].x, o[0].y, o[1].x, o[1].y), h1 = make_uint4(o[2].x, o[2].y, o[3].x, o[3].y);
        uint32_t am = max(mx8_amax8(h0), mx8_amax8(h1));
        const auto u = __builtin_amdgcn_permlane16_swap(am, am, false, false);   // partner fq ^ 1: the block's 32 columns
        am = max((uint32_t)u[0], (uint32_t)u[1]);
        const int E = mx8_block_exp(am);
        word[i >> 2] |= (uint32_t)(E + 127) << (8 * (i & 3));
        const uint2 q0 = mx8_pack8(h0, E), q1 = mx8_pack8(h1, E);
        const int m = m0 + wm * 128 + i * 16 + fr;
        if (m < M && n < N) *reinterpret_cast<uint4*>(o8.q + (int64_t)m * o8.ldq + n) = make_uint4(q0.x, q0.y, q1.x, q1.y);
    }
    // lanes fq and fq ^ 1 hold the same words (block fq >> 1): lane (fr, fq) stores brick fq & 1's. store_scale_word
    // written out: as a call it reorders 140 instructions of the fp8 FC1 kernel's epilogue (tools/kdiff.py)
    const int nb = n0 + wn * 64;
    const int R = m0 + wm * 128 + (fq & 1) * 64;   // brick row base
    if (nb < N && R < M)   // bricks that hold an output row, as store_scale_word
        reinterpret_cast<uint32_t*>(o8.s)[(int64_t)(nb >> 7) * o8.lds + R + (((nb >> 5) & 3) + (fq >> 1)) * 16 + fr] =
            (fq & 1) ? word[1] : word[0];
}

// fp8-only output (no bf16 copy: FC1 -> FC2's A operand). Same image as store_wave_tile, read back 32 B per
// lane (16 consecutive columns: 4 lanes per 64-column row, 8 iterations) so every element store is 16 B, and a
// 32-column block is a lane pair (one DPP step). The wave owns whole scale words (its 128 rows are two 64-row
// bricks, its 64 columns two K-blocks of one plane): the bytes are gathered in the image, then one dword store
// per lane writes all 64 words.
template <int EPI>
__device__ __forceinline__ void store_wave_tile_q8(char* img, const char* aux, const f32x4 (&acc)[4][8], int wm, int wn,
                                                   int m0, int n0, int lane, int M, int N, Out8 o8) {
    epi_to_image<EPI>(img, aux, acc, wm, wn, lane);
    __builtin_amdgcn_wave_barrier();
    const int cc = lane & 3;   // 16-column group of the wave's 64 columns
    uint32_t e8[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int row = it * 16 + (lane >> 2);
        const uint4 h[2] = {image_get16(img, row, 2 * cc, row & 1), image_get16(img, row, 2 * cc + 1, row & 1)};
        uint32_t am = max(mx8_amax8(h[0]), mx8_amax8(h[1]));
        am = max(am, (uint32_t)__builtin_amdgcn_mov_dpp((int)am, 0xB1, 0xF, 0xF, false));   // lane pair = block
        const int E = mx8_block_exp(am);
        e8[it] = (uint32_t)(E + 127);
        const uint2 q0 = mx8_pack8(h[0], E), q1 = mx8_pack8(h[1], E);
        const int m = m0 + wm * 128 + row;
        const int n = n0 + wn * 64 + cc * 16;
        if (m < M && n < N) *reinterpret_cast<uint4*>(o8.q + (int64_t)m * o8.ldq + n) = make_uint4(q0.x, q0.y, q1.x, q1.y);
    }
    // scale bytes -> the wave's 64 words (word w = brick (w >> 5), block (w >> 4) & 1, row r16 = w & 15; byte f =
    // rows 16f + r16 of the brick), staged in image bytes no lane reads any more
    __builtin_amdgcn_wave_barrier();
    if ((lane & 1) == 0) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int row = it * 16 + (lane >> 2);
            const int w = (row >> 6) * 32 + (cc >> 1) * 16 + (row & 15);
            img[w * 4 + ((row >> 4) & 3)] = (char)e8[it];
        }
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t word = *reinterpret_cast<const uint32_t*>(img + lane * 4);
    store_scale_word(o8, word, m0 + wm * 128, n0 + wn * 64, M, N, lane >> 5, (lane >> 4) & 1, lane & 15);
}

// ---- kernel tail ----
// Every wave is done with the operand ring (reused as the 8 x 16 KiB images) and the LN combine is visible. A raw
// s_barrier behind lgkmcnt(0) only, so global loads (the residual rows) stay in flight across it; no LDS-DMA is
// outstanding after a K loop.
__device__ __forceinline__ void epilogue_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// The bf16 kernels' tail, after the K loop and the LN combine: the residual loads, the barrier, and this wave's
// epilogue - direct stores (DIRECT: the W rows were staged in wperm order), else the pipelined image epilogue, else
// (EPI_PATCH, OUT8) the two-pass one. `img`: this wave's 16 KiB of the ring.
template <int EPI, bool OUT8, bool DIRECT>
__device__ __forceinline__ void finish_tile(char* img, const char* aux, const f32x4 (&acc)[4][8], int wm, int wn, int m0,
                                            int n0, int lane, const bf16_t* residual, const float* __restrict__ pos,
                                            int g2, bf16_t* C, int ldc, int M, int N, float* stats_out, int stats_rows,
                                            Out8 o8) {
    // no LDS-DMA is outstanding after the K loop; saying so with the builtin (which hipcc's waitcnt pass reads, unlike
    // asm) keeps it from draining vmcnt(0) - and with it the residual loads - at the first LDS access below
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    uint4 res[16];
    constexpr bool PIPE = EPI != VPF_EPI_PATCH && !OUT8;
    if constexpr (DIRECT) {
        if constexpr (epi_is_ln(EPI)) epilogue_barrier();   // only the LN combine is read by the other waves
        store_wave_tile_direct<EPI>(aux, acc, wm, wn, m0, n0, lane, C, ldc, M, N);
        return;
    }
    if constexpr (EPI == VPF_EPI_BIAS_RESIDUAL) load_residual<PIPE>(res, residual, wm, wn, m0, n0, lane, ldc, M, N);
    epilogue_barrier();
    float* prod_stats = (EPI == VPF_EPI_BIAS_RESIDUAL || EPI == VPF_EPI_PATCH) ? stats_out : nullptr;
    if constexpr (PIPE)
        store_wave_tile_pipe<EPI>(img, aux, acc, wm, wn, m0, n0, lane, res, C, ldc, M, N, prod_stats, stats_rows);
    else
        store_wave_tile<EPI, OUT8>(img, aux, acc, wm, wn, m0, n0, lane, res, pos, g2, C, ldc, M, N, prod_stats,
                                   stats_rows, o8);
}

}  // namespace gemm
}  // namespace vpf
