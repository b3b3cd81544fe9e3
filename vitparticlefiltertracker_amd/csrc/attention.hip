// Multi-head self-attention per (particle, head): out = softmax(q k^T * scale) v,
// non-causal, N tokens (197 for /16@224, 577 for /14@336), head_dim 64.
//
// bf16 path (vpf_attention_bf16), N <= 256: one 512-thread workgroup (8 waves) per (particle, head). K and V of
// the head are staged once into LDS by LDS-DMA, in 32-key chunks that compute follows (k_attn_bf16_pipe). N is
// rounded up to 32 keys; the padding rows are copies of row N - 1 (finite, masked in the last key step: a pad row
// let through the mask counts key N - 1 again, it does not score 0):
//   K image: 128-B rows, 16-B chunk c of row r at K_SWZ(r, c) -> ds_read_b128 conflict-free
//   V image: 128-B rows, 16-B chunk c of row r at V_SWZ(r, c) -> ds_read_b64_tr_b16
//            conflict-free (T10 hardware-transposed read feeds V^T as the MFMA A operand).
// Each wave takes one 32-query strip. "Swapped" QK^T (K as A, Q as B) on v_mfma_f32_32x32x16_bf16 puts one
// query per lane column and its keys in the lane's 16 accumulator registers, so the online-softmax row
// max / sum is register-local plus one cross-half shuffle, and the bf16-packed probabilities are
// directly the B operand of O^T = V^T P^T (cdna_hip_programming.md §3, accumulator as next operand).
// Keys are processed in 32-key chunks with online softmax (exp2 with scale*log2e folded in), so the
// register footprint does not grow with N. N > 256 streams the same chunks through a ring (k_attn_stream);
// q_rows = 1 runs k_attn_cls_bf16.
//
// fp32 parity path (vpf_attention_f32): one thread per query, K/V of the head streamed through LDS as fp32 in
// chunks of 128 keys, exact two-pass expf softmax (any N <= 4096).
//
// Layout of this file: every piece the two MFMA kernels share is defined once, in this order:
//   LDS swizzles (K_SWZ / V_SWZ) and lane shuffles;
//   step pieces: lazy_rescale / raise_max, pack_bf8, acc_key / mask_keys, lsum4, qk32, pv32;
//   the steps: attn_step16 (16-query strip), attn_step_pl<MASK, NR> (k_attn_bf16_pipe), attn_step_lf<MASK, NR>
//     (k_attn_stream); NR = 16 is a whole 32-key tile, NR = 4 the last tile when at most 8 of its keys are real;
//   kernel plumbing: wait_vmcnt, load_q / pin_q, strip32_out / store_strip32 / store_strip16;
//   the kernels, each a DMA schedule around one run_strip (chunk loop + epilogue, instantiated per strip kind);
//   the host entry points (launch_pipe<OUT8> serves both k_attn_bf16_pipe instances).
#include <type_traits>

#include "vpf_common.h"
#include "mx8.h"
#include "../../include/vpf.h"

using namespace vpf;

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int HD = 64;
constexpr int ROWB = HD * 2;  // 128 B per K/V row

// where 16-B chunk c of row r sits inside the row's 128 B in the K / V image. The kernels' LDS-DMA pieces (one
// wave-instruction of 1 KiB = 8 rows, 16 B per lane, lane (sub, slot) = (lane / 8, lane % 8) on row sub) have a lane-linear
// LDS destination, so they apply the same map to the source address: the lane fetches the chunk that belongs in its slot.
// Macros over plain identifiers, not functions: as __forceinline__ functions (in every form tried: a ternary of two
// calls, both calls and a select, one helper holding the ternary) the DMA issue loops compiled to three more VALU each
// (the ternary of calls to a branch) and N = 197 measured 0.5 - 1 % slower; the macro text compiles like the written-out
// expressions (profiles/r9_lab/attn_refactor_ab.txt).
#define K_SWZ(r, c) (c ^ ((r >> 1) & 7))
#define V_SWZ(r, c) (c ^ (((r >> 1) & 1) << 2))
__device__ __forceinline__ int k_off(int r, int c) { return r * ROWB + (K_SWZ(r, c) << 4); }
__device__ __forceinline__ int v_off(int r, int c) { return r * ROWB + (V_SWZ(r, c) << 4); }

// the lane id re-read through asm: address math derived from it stays where it is used instead of being hoisted above
// the enclosing loop as an invariant
__device__ __forceinline__ int lane_id_asm() {
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    return lane;
}

// max / sum of a value with its partner lane l ^ 32 by one v_permlane32_swap (VALU, no LDS round trip; the
// __shfl_xor form costs a ds_bpermute, its address VALU and an lgkmcnt wait on the step's critical path).
// Every lane of the wave must be active.
__device__ __forceinline__ float xor32_max(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    float y;   // one v_max_f32: fmaxf on bit-cast values adds two NaN-canonicalising v_max (scores are never NaN)
    asm("v_max_f32 %0, %1, %2" : "=v"(y) : "v"(__uint_as_float(r[0])), "v"(__uint_as_float(r[1])));
    return y;
}
__device__ __forceinline__ float xor32_sum(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xor16_max(float x) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    float y;   // scores are never NaN: one v_max_f32 (as xor32_max)
    asm("v_max_f32 %0, %1, %2" : "=v"(y) : "v"(__uint_as_float(r[0])), "v"(__uint_as_float(r[1])));
    return y;
}
__device__ __forceinline__ float xor16_sum(float x) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ds_read_b64_tr_b16 as inline asm: hipcc treats the builtin as a possible reader of in-flight LDS-DMA
// bytes and drains vmcnt(0) before it, which would serialise the key-pipelined kernel on its last chunk.
// The caller waits lgkmcnt itself (tr_wait) before the MFMA that consumes the result.
// A constant byte offset goes in the instruction's offset field. V rows r + 8 and r + 16 keep bit 1
// of r, so v_off(r + 8j, c) = v_off(r, c) + 1024 j: the four row blocks of a key step share one address VGPR
// per 32-dim column tile instead of one v_add each.
template <int OFF>
__device__ __forceinline__ bf16x4 ds_read_tr_asm_o(uint32_t addr) {
    bf16x4 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
    return r;
}

// ---------------- pieces of the online-softmax steps ----------------
// The running max moves to max(m, bm): alpha = 2^((m - new m) scale) goes to `scale_acc`, which applies it to the
// step's l and O accumulators.
template <class F>
__device__ __forceinline__ void raise_max(float bm, float scale_log2, float& m, F&& scale_acc) {
    const float mn = fmaxf(m, bm);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale_log2);
    m = mn;
    scale_acc(alpha);
}
// T13 lazy rescale: the max moves only when some lane's tile max bm exceeds it by more than 2^8 after scaling.
template <class F>
__device__ __forceinline__ void lazy_rescale(float bm, float scale_log2, float& m, F&& scale_acc) {
    if (__builtin_expect(__any(bm > m + 8.0f / scale_log2), 0))   // loop-invariant threshold: 2 VALU, not 3
        raise_max(bm, scale_log2, m, scale_acc);
}

// 8 probabilities -> the bf16x8 B operand of a PV MFMA
__device__ __forceinline__ bf16x8 pack_bf8(float p0, float p1, float p2, float p3, float p4, float p5, float p6,
                                           float p7) {
    return __builtin_bit_cast(bf16x8, make_uint4(pack_bf2(p0, p1), pack_bf2(p2, p3), pack_bf2(p4, p5), pack_bf2(p6, p7)));
}

// 32x32 score tile (qk32): accumulator register r of half-wave hh holds key acc_key(r, hh) of the tile. Registers
// 0..3 are keys 0..7, so a tile with at most 8 real keys needs only those (the steps' NR = 4 form).
__device__ __forceinline__ int acc_key(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// MASK: keys >= N get score -inf, i.e. probability 0 (the padded K / V rows are finite copies of row N - 1). kb: the
// tile's first key index. Only registers 0 .. NR-1 are looked at.
template <bool MASK, int NR>
__device__ __forceinline__ void mask_keys(f32x16& s, int kb, int hh, int N) {
    if constexpr (MASK) {
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (kb + acc_key(r, hh) >= N) s[r] = -INFINITY;
    }
}

template <int NR>
__device__ __forceinline__ float max_acc(const f32x16& s) {
    float bm = -INFINITY;
#pragma unroll
    for (int r = 0; r < NR; ++r) bm = fmaxf(bm, s[r]);
    return bm;
}

// The row sum on the matrix cores: 4 bf16 probabilities per lane against a ones A operand on
// v_mfma_f32_4x4x4_16b_bf16; every accumulator register gets acc + the lane's own sum.
__device__ __forceinline__ f32x4 lsum4(const bf16x4 p, f32x4 acc) {
    const bf16x4 ones = {(short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80};
    return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(ones, p, acc, 0, 0, 0);
}

// S^T = K Q^T for one 32-key tile: the four K fragment reads together, then the four MFMAs (attn_step's PRE form)
// Kt: the tile's first K row in LDS (the swizzles depend on the row's low bits only, so a 32-row tile is addressed by
// its local rows)
__device__ __forceinline__ f32x16 qk32(const char* Kt, int lane, const bf16x8 qf[4]) {
    const int l32 = lane & 31, hh = lane >> 5;
    f32x16 s = f32x16{};
    bf16x8 kf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) kf[ks] = *reinterpret_cast<const bf16x8*>(Kt + k_off(l32, ks * 2 + hh));
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    __builtin_amdgcn_sched_barrier(0);
    return s;
}

// O^T += V^T P^T over one 32-key tile (both 16-key halves when HALVES == 2; the tail step's first half only when 1)
template <int HALVES>
__device__ __forceinline__ void pv32(const char* Vt, int lane, const bf16x8 pf[2], f32x16& o0, f32x16& o1) {
    const int grp = lane >> 4, gi = lane & 15;
    const int rq = gi >> 2, cp = gi & 3;
    const int rbase = 4 * (grp >> 1) + rq;
    bf16x4 vr[2][2][2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        const int col = dt * 32 + 16 * (grp & 1) + 4 * cp;
        const int c16 = col >> 3, inner = (col & 7) * 2;
        const uint32_t a = (uint32_t)(size_t)Vt + (uint32_t)(v_off(rbase, c16) + inner);
        vr[0][dt][0] = ds_read_tr_asm_o<0>(a);
        vr[0][dt][1] = ds_read_tr_asm_o<1024>(a);
        if constexpr (HALVES == 2) {
            vr[1][dt][0] = ds_read_tr_asm_o<2048>(a);
            vr[1][dt][1] = ds_read_tr_asm_o<3072>(a);
        }
    }
    if constexpr (HALVES == 2)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vr[0][0][0]), "+v"(vr[0][0][1]), "+v"(vr[0][1][0]), "+v"(vr[0][1][1]),
                     "+v"(vr[1][0][0]), "+v"(vr[1][0][1]), "+v"(vr[1][1][0]), "+v"(vr[1][1][1])::"memory");
    else
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vr[0][0][0]), "+v"(vr[0][0][1]), "+v"(vr[0][1][0]), "+v"(vr[0][1][1])
                     ::"memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int st = 0; st < HALVES; ++st)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            const bf16x4 lo = vr[st][dt][0], hi = vr[st][dt][1];
            const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            if (dt == 0) o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[st], o0, 0, 0, 0);
            else o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[st], o1, 0, 0, 0);
        }
}

// ---------------- the steps: one 32-key tile of one strip ----------------
// 16-query strip on v_mfma_f32_16x16x32_bf16: the last strip when it holds at most 16 real queries (N = 197 ->
// queries 192..207, 5 real), at half the MFMA and softmax work of a 32-query strip (which spent 27 of its 32 rows
// on padding). Operand maps of 16x16x32 (g = lane / 16): A lane = row lane % 16, K slots 8g .. 8g+7; B lane = column
// lane % 16, the same K slots; D lane = rows 4g .. 4g+3 of column lane % 16.
//   S^T = K Q^T per 16-key tile kt: A = K rows kb + 16 kt + lane % 16 (dims 32 kk + 8g ..), B = Q^T (query
//   q0 + lane % 16, dims 32 kk + 8g ..), so lane (query lane % 16, g) holds the scores of keys kb + 16 kt + 4g + r.
//   A query's row max / sum combine the 4 lanes lane % 16 + 16g (permlane16 + permlane32 swaps).
//   O^T += V^T P^T with the PV K slots permuted: slot 8g + 4 kt + r <-> key kb + 16 kt + 4g + r. The lane's own
//   8 probabilities are then its B fragment as they stand, and its V^T A fragment is two transposed reads: lane
//   16g + 4q + p supplies row kb + 4g + q (then + 16 rows = + 2048 B: the V swizzle keeps bit 1 of the row), dims
//   16 dt + 4p .. +3, and receives dim 16 dt + lane % 16 of those 4 keys (cdna_hip_programming.md T10).
//   O^T lane = dims 16 dt + 4g .. +3 of query lane % 16.
// MASK: keys >= N get probability 0 (the padded K / V rows are finite copies of row N - 1).
// Kt / Vt: the tile's first K / V row in LDS; kb: its first key index (masking only).
template <bool MASK>
__device__ __forceinline__ void attn_step16(const char* Kt, const char* Vt, int kb, int N, int lane, const bf16x8 qf[2],
                                            float scale_log2, float& m, float& l, f32x4 (&o)[4]) {
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kr = 16 * kt + r16;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Kt + k_off(kr, 4 * kk + g));
            s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], s[kt], 0, 0, 0);
        }
    }
    float bm = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if constexpr (MASK) {
                if (kb + 16 * kt + 4 * g + r >= N) s[kt][r] = -INFINITY;
            }
            bm = fmaxf(bm, s[kt][r]);
        }
    lazy_rescale(xor32_max(xor16_max(bm)), scale_log2, m, [&](float alpha) {
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
    });
    const float msc = m * scale_log2;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(fmaf(s[kt][r], scale_log2, -msc));
            s[kt][r] = p;
            l += p;
        }
    const bf16x8 pf = pack_bf8(s[0][0], s[0][1], s[0][2], s[0][3], s[1][0], s[1][1], s[1][2], s[1][3]);
    const int q = r16 >> 2, p4 = r16 & 3;
    bf16x4 vr[4][2];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const int c16 = 2 * dt + (p4 >> 1), inner = 8 * (p4 & 1);
        const uint32_t a = (uint32_t)(size_t)Vt + (uint32_t)(v_off(4 * g + q, c16) + inner);
        vr[dt][0] = ds_read_tr_asm_o<0>(a);
        vr[dt][1] = ds_read_tr_asm_o<2048>(a);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vr[0][0]), "+v"(vr[0][1]), "+v"(vr[1][0]), "+v"(vr[1][1]),
                 "+v"(vr[2][0]), "+v"(vr[2][1]), "+v"(vr[3][0]), "+v"(vr[3][1])::"memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const bf16x4 lo = vr[dt][0], hi = vr[dt][1];
        const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
    }
}

// One 32-key step of a 32-query strip in the rounds 1-4 form (the N <= 256 kernel's): the row max of every tile (T13
// lazy rescale when it moved by more than 2^8), l summed from the fp32 probabilities. Bit-identical to the rounds 1-4
// attn_step.
// NR = 16: the whole tile. NR = 4 (the tail step of rounds 1-4): the last tile when at most 8 of its 32 keys are real:
// score registers 0..3 only (acc_key), the first 16-key PV half, pf[1] zero. That form starts with the lane id re-read
// through asm: its address math then stays inside this (last) step instead of being hoisted above the key loop, where
// it held ~40 extra VGPRs and spilled.
template <bool MASK, int NR>
__device__ __forceinline__ void attn_step_pl(const char* Kt, const char* Vt, int kb, int N, int lane, const bf16x8 qf[4],
                                             float scale_log2, float& m, float& l, f32x16& o0, f32x16& o1) {
    static_assert(NR == 16 || (NR == 4 && MASK), "a whole tile, or the masked tail of at most 8 keys");
    if constexpr (NR == 4) lane = lane_id_asm();
    f32x16 s = qk32(Kt, lane, qf);
    mask_keys<MASK, NR>(s, kb, lane >> 5, N);
    lazy_rescale(xor32_max(max_acc<NR>(s)), scale_log2, m, [&](float alpha) {
        l *= alpha;
        o0 *= alpha;
        o1 *= alpha;
    });
    const float msc = m * scale_log2;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(s[r], scale_log2, -msc));
        s[r] = p;
        l += p;
    }
    bf16x8 pf[2] = {};
    if constexpr (NR == 16) {
        pf[0] = pack_bf8(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
        pf[1] = pack_bf8(s[8], s[9], s[10], s[11], s[12], s[13], s[14], s[15]);
    } else {
        pf[0] = pack_bf8(s[0], s[1], s[2], s[3], 0.f, 0.f, 0.f, 0.f);
    }
    pv32<NR == 16 ? 2 : 1>(Vt, lane, pf, o0, o1);
}

// ---------------- round 5: the row sum on the matrix cores, and a speculative running max ----------------
// Per 32-key step a 32-query strip spent ~490 issue cycles per wave against 256 cycles of MFMA work (8 x 32x32x16):
// 16 v_exp_f32 (8 cyc each), 16 v_fma_f32 (the exp2 argument), 16 v_add_f32 (the row sum l), 8 v_max3_f32 + a permlane
// swap + compare (the running max), 8 v_cvt_pk_bf16_f32, address adds (MI355X_MICROARCH.md 'vector-instruction ISSUE
// cost'). Two of those groups move off the vector issue port here:
//  * l: each lane's bf16-packed probabilities (the PV MFMA's B operand) are summed by v_mfma_f32_4x4x4_16b_bf16 against
//    a ones A operand (lsum4, four per step: 4 values per lane each, every accumulator register gets the lane's own
//    sum), so the 16 v_add_f32 become 4 MFMA issues. l is then the sum of the very bf16 weights the PV MFMA multiplies.
//  * the running max: the step exponentiates against the current m without looking for a new maximum, and the
//    accumulated l tells whether that was safe: a lane whose 16 probabilities sum to at most 2^8 has none above 2^8,
//    the bound the lazy rescale (T13) already allowed. Only when some lane's step sum exceeds it (or is not finite) does
//    the step recompute its scores, take the max, rescale O and l and exponentiate again (rare after the first keys).
//    The first key step of a strip takes the max as before (m = -inf).
// One 32-key step of a 32-query strip in that form (the N > 256 kernel's). Kt / Vt: the tile's first K / V row in LDS;
// kb: its first key index (masking only). `first`: the strip's first key step (m = -inf: take the tile max). MASK: keys
// >= N in this tile get probability 0. lacc: the 4x4x4 MFMA accumulator (every register = the lane's running l).
// NR = 16 / NR = 4 as attn_step_pl (NR = 4: one 4x4x4 MFMA for l, the first 16-key PV half, the lane id re-read).
template <bool MASK, int NR>
__device__ __forceinline__ void attn_step_lf(const char* Kt, const char* Vt, int kb, int N, int lane, const bf16x8 qf[4],
                                             float scale_log2, bool first, float& m, f32x4& lacc, f32x16& o0,
                                             f32x16& o1) {
    static_assert(NR == 16 || (NR == 4 && MASK), "a whole tile, or the masked tail of at most 8 keys");
    if constexpr (NR == 4) lane = lane_id_asm();
    auto scores = [&]() {
        f32x16 t = qk32(Kt, lane, qf);
        mask_keys<MASK, NR>(t, kb, lane >> 5, N);
        return t;
    };
    bf16x8 pf[2] = {};
    f32x4 ln;
    auto expo = [&](f32x16& t) {   // t: scores in, probabilities out
        const float msc = m * scale_log2;
#pragma unroll
        for (int r = 0; r < NR; ++r) t[r] = __builtin_amdgcn_exp2f(fmaf(t[r], scale_log2, -msc));
        if constexpr (NR == 16) {
            pf[0] = pack_bf8(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
            pf[1] = pack_bf8(t[8], t[9], t[10], t[11], t[12], t[13], t[14], t[15]);
        } else {
            pf[0] = pack_bf8(t[0], t[1], t[2], t[3], 0.f, 0.f, 0.f, 0.f);
        }
        ln = lsum4(__builtin_shufflevector(pf[0], pf[0], 0, 1, 2, 3), lacc);
        if constexpr (NR == 16) {
            ln = lsum4(__builtin_shufflevector(pf[0], pf[0], 4, 5, 6, 7), ln);
            ln = lsum4(__builtin_shufflevector(pf[1], pf[1], 0, 1, 2, 3), ln);
            ln = lsum4(__builtin_shufflevector(pf[1], pf[1], 4, 5, 6, 7), ln);
        }
    };
    f32x16 s = scores();
    if (first) m = xor32_max(max_acc<NR>(s));
    expo(s);
    if (!first && __builtin_expect(__any(!(ln[0] - lacc[0] <= 256.0f)), 0)) {
        f32x16 t = scores();   // the scores again (s holds probabilities now)
        raise_max(xor32_max(max_acc<NR>(t)), scale_log2, m, [&](float alpha) {
            lacc *= alpha;
            o0 *= alpha;
            o1 *= alpha;
        });
        expo(t);
    }
    lacc = ln;
    pv32<NR == 16 ? 2 : 1>(Vt, lane, pf, o0, o1);
}

// ---------------- kernel plumbing shared by k_attn_bf16_pipe and k_attn_stream ----------------
// s_waitcnt vmcnt(n) for a runtime n (the immediate must be a constant): n >= the outstanding count is a no-op
__device__ __forceinline__ void wait_vmcnt(int n) {
    switch (n) {
#define VPF_VMW(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
        VPF_VMW(1) VPF_VMW(2) VPF_VMW(3) VPF_VMW(4) VPF_VMW(5) VPF_VMW(6) VPF_VMW(7) VPF_VMW(8) VPF_VMW(9)
        VPF_VMW(10) VPF_VMW(11) VPF_VMW(12) VPF_VMW(13) VPF_VMW(14) VPF_VMW(15) VPF_VMW(16) VPF_VMW(17)
        VPF_VMW(18) VPF_VMW(19) VPF_VMW(20) VPF_VMW(21) VPF_VMW(22) VPF_VMW(23)
#undef VPF_VMW
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

// Q fragments of the wave's strip (first query q0) by inline-asm loads: hipcc does not count them, so it cannot merge
// them into a vmcnt(0) at the first MFMA (which would also drain every K/V chunk). They are the wave's oldest
// vector-memory operations, older than all its DMA pieces, so the kernel's first counted wait retires them, and the
// pin_q<4> after that wait pins every use below it.
// 32-query strip: qf[ks] = Q[q0 + lane % 32][16 ks + 8 (lane / 32) ..] (qk32's B operand).
// 16-query strip (k16): qf[kk] (kk < 2) = Q[q0 + lane % 16][32 kk + 8 (lane / 16) ..] (attn_step16's B operand;
// qf[2], qf[3] re-read the same bytes and are unused).
// The shape every caller must keep (tests/test_host.py checks it on the compiled code):
//  * One asm load statement per register for both strip kinds, with the strip kind in the address only: loads issued
//    in two branches would leave each qf a phi of two asm outputs, and the copies that resolve it run at the branch
//    merge, before the loads land, so the registers the MFMAs read were stale (the NaNs of round 2's 16-query tail,
//    on the 32-query strips too).
//  * The counted wait and pin_q<4> come before the strip-kind branch: the compiler copies asm-load destinations
//    wherever register allocation wants (the phi / live-range copies of the strip-kind branch moved qf before any
//    wait, reading stale registers: the round-2 NaN).
//  * Round 4: folding the wait and the pin into one asm statement per wait-count case, as ADVICE r3 suggested, made
//    each qf a phi of several asm outputs again and brought the NaNs back: profiles/r4_pytest_gpu_a.log. The rule
//    kept: no branch or merge between an asm load and the wait that retires it; the wait carries no register operands.
__device__ __forceinline__ void load_q(bf16x8 (&qf)[4], const bf16_t* qbase, int D, int N, bool k16, int q0, int lane) {
    const bf16_t* qp = k16 ? qbase + (int64_t)min(q0 + (lane & 15), N - 1) * 3 * D + 8 * (lane >> 4)
                           : qbase + (int64_t)min(q0 + (lane & 31), N - 1) * 3 * D + (lane >> 5) * 8;
    const int step = k16 ? 32 : 16;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(qf[ks]) : "v"(qp + (k16 ? (ks & 1) : ks) * step));
}
// the empty asm that pins the first NQ Q registers: after the wait that retires load_q (NQ = 4), and after every
// barrier of a strip's chunk loop (the registers that strip kind reads)
template <int NQ>
__device__ __forceinline__ void pin_q(bf16x8 (&qf)[4]) {
    if constexpr (NQ == 2) asm volatile("" : "+v"(qf[0]), "+v"(qf[1]) :: "memory");
    else asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]) :: "memory");
}

// 32-query strip epilogue: O * inv as packed bf16, four 16-B pieces per lane.
// Lane (l32, hh) holds dims 8k + 4hh .. +3 of query l32 for the eight 8-dim groups k (o0: k < 4, o1: k >= 4).
// v_permlane32_swap per pair (k, k+1) gives the lower half-wave dims 8k..8k+7 and the upper half-wave
// 8k+8..8k+15: one 16-B store per pair (cdna_hip_programming.md T21) instead of two 8-B stores. Afterwards lane
// (l32, hh) holds dims 16k + 8hh .. +7 in ov[k]. All lanes active: the swaps read the partner half-wave.
__device__ __forceinline__ void strip32_out(const f32x16& o0, const f32x16& o1, float inv, uint4 (&ov)[4]) {
    uint32_t gx[8], gy[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const f32x16& o = k < 4 ? o0 : o1;
        const int b4 = 4 * (k & 3);
        gx[k] = pack_bf2(o[b4] * inv, o[b4 + 1] * inv);
        gy[k] = pack_bf2(o[b4 + 2] * inv, o[b4 + 3] * inv);
    }
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const auto rx = __builtin_amdgcn_permlane32_swap(gx[k], gx[k + 1], false, false);
        const auto ry = __builtin_amdgcn_permlane32_swap(gy[k], gy[k + 1], false, false);
        ov[k >> 1] = make_uint4(rx[0], ry[0], rx[1], ry[1]);
    }
}
// ... and its bf16 store; orow: the query's 64 output dims of this head
__device__ __forceinline__ void store_strip32(bf16_t* orow, int hh, const uint4 (&ov)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<uint4*>(orow + 8 * hh + 16 * k) = ov[k];
}

// 16-query strip epilogue and store: the 4 lanes lane % 16 + 16 g share query q0 + lane % 16 (l is summed over them);
// lane holds dims 16 dt + 4g .. +3. ohead: row 0 of this (particle, head) in the output.
__device__ __forceinline__ void store_strip16(const f32x4 (&o16)[4], float l, bf16_t* ohead, int D, int q0, int q_rows,
                                              int lane) {
    const float inv = 1.0f / xor32_sum(xor16_sum(l));
    const int qq = q0 + (lane & 15);
    if (qq < q_rows) {
        bf16_t* orow = ohead + (int64_t)qq * D + 4 * (lane >> 4);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<uint2*>(orow + 16 * dt) = make_uint2(pack_bf2(o16[dt][0] * inv, o16[dt][1] * inv),
                                                                  pack_bf2(o16[dt][2] * inv, o16[dt][3] * inv));
    }
}

// ---------------- N <= 256: the head's whole K / V image in LDS, compute follows the chunks as they land ----------------
// Key-pipelined: one 512-thread workgroup per (particle, head) as above, but the K/V images land in
// 32-key chunks and compute follows them: every wave issues its Q loads, then exactly one DMA piece per
// chunk (waves 0-3: the chunk's four 8-row K pieces, waves 4-7: its four V pieces), in chunk order. Before
// key tiles c .. c+PIPE_CPB-1: a counted vmcnt (this wave's pieces of those chunks landed; later chunks stay in
// flight) and one s_barrier (everyone's did), so the QK^T / softmax / PV of the first tiles overlap the
// HBM fetch of the later ones instead of waiting for the whole 57 KiB image. Waves without a query strip
// (8 waves, 7 strips at N = 197) only move data and keep the barrier count. N <= 256 (one strip per wave).
// PIPE_CPB: 32-key chunks per counted wait + barrier. Waiting for 4 chunks at a time (2 barriers at N = 197)
// measured 3-4 % faster than per-chunk barriers (1, 2, 3, 4: 1.223 / 1.210 / 1.196 / 1.178 ms at 4096 x 12
// heads, profiles/r1_gemm_lab/attn_cpb.txt): each barrier puts all 8 waves back in lockstep. Round 2 on the current
// kernel (profiles/r2_gemm_lab/attn_cpb_r2s5.txt, per-launch averages from bench.py): CPB 3 / 4 / 5 / 6 / 7 =
// 1.084 / 1.075 / 1.069 / 1.064 / 1.156 ms at N = 197; 6 and 4 are level on ViT-L (N = 577) and on the MX8 output.
constexpr int PIPE_CPB = 6;
// OUT8: the output is written as MX8 (the fp8 path's proj A operand) instead of bf16: the same packed bf16
// values, quantised per 32-dim block (a block = 16 dims of a lane + 16 of its partner half-wave lane).
// 16-query tail: when the last strip holds at most 16 real queries (N % 32 in 1..16: N = 197), its wave runs the
// 16-query step (attn_step16) instead of a 32-query strip. That wave runs the same chunk loop (run_strip below, one
// template for both strip kinds), so every wave of the workgroup passes the same barriers at the same chunks: a wave
// whose loop took another barrier schedule would release its partners' reads of K / V chunks that have not landed
// (the round-2 attempt at this tail, which gave its 16-query wave a chunk loop of its own, read such chunks: NaNs
// on the 32-query strips).
// The last key step runs the steps' NR = 4 form when at most 8 of its keys are real.
// The round-3 lab variants of this kernel (compute-only / load-only probes, staggered start, software-pipelined strip,
// the round-2 step order) are in the lab build (tools/gemm_lab/attention_lab.hip). Round 4's persistent chunk-ring form
// of this kernel is bit-identical but 1.5x slower: tools/gemm_lab/attention_lab.hip, profiles/r4_lab/attn_ring_ab_v*.txt.
template <bool OUT8>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void k_attn_bf16_pipe(
    const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int N, int H, float scale_log2, int q_rows,
    uint8_t* __restrict__ out8, int ld8, uint8_t* __restrict__ s8, int lds8) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int CPB = PIPE_CPB;
    const int NP = (N + 31) & ~31;
    const int NT = NP >> 5;              // 32-key chunks
    char* Ks = smem;
    char* Vs = smem + NP * ROWB;
    const int bh = blockIdx.x;
    const int b = bh / H, h = bh - (bh / H) * H;
    const int D = H * HD;
    const int64_t row0 = (int64_t)b * N;
    const bf16_t* qbase = qkv + row0 * 3 * D + h * HD;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, hh = lane >> 5;
    const int nstrips = (q_rows + 31) >> 5;
    // sid: this wave's query strip (the identity; round 5 tried swapping waves 4, 5 with 6, 7 in every other workgroup so
    // that the half-work and idle strips of two co-resident workgroups land on different SIMDs: 1.4 % slower,
    // profiles/r5_lab/attn_simd_balance_ab.txt)
    const int sid = wid;
    // wave-uniform: this wave's strip holds query N - 1 and at most 16 real queries. Decided by N, not q_rows, so a
    // row's result does not depend on how many rows the call computes.
    const int nlast = (N - 1) >> 5;
    const bool w16 = !OUT8 && sid == nlast && sid < nstrips && N - 32 * nlast <= 16;
    bf16x8 qf[4];
    load_q(qf, qbase, D, N, w16, sid * 32, lane);
    {
        const bool isv = wid >= 4;
        const int sub = lane >> 3, slot = lane & 7;
        const bf16_t* src0 = qbase + (isv ? 2 * D : D);
        char* img = isv ? Vs : Ks;
        for (int c = 0; c < NT; ++c) {
            const int g = c * 4 + (wid & 3);                 // 8-row piece index inside the image
            const int r = 8 * g + sub;
            const int ch = isv ? V_SWZ(r, slot) : K_SWZ(r, slot);
            __builtin_amdgcn_global_load_lds((gptr_t)(src0 + (int64_t)min(r, N - 1) * 3 * D + ch * 8),
                                             (lptr_t)(img + g * 1024), 16, 0, 0);
        }
    }
    // The Q loads are older than this wave's NT DMA pieces: landed once at most NT are outstanding (load_q's rules).
    // The first chunk barrier waits for CPB chunks, so this costs nothing.
    wait_vmcnt(NT);
    pin_q<4>(qf);
    const bool active = sid < nstrips;
    const int nfull = N >> 5;             // chunks without padded keys
    // The chunk loop and the stores of one strip kind: the barrier schedule (a counted wait + s_barrier before chunks
    // 0, CPB, 2 CPB, ..., and before the padded tail chunk) depends on N and CPB only, so every wave of the workgroup
    // passes the same barriers whatever its kind (or none: active = false keeps the barriers, computes nothing).
    auto run_strip = [&](auto k16) {
        constexpr bool W16 = decltype(k16)::value;
        f32x16 o0 = {}, o1 = {};
        f32x4 o16[4] = {};
        float m = -INFINITY, l = 0.f;
        int c = 0;
        for (; c < nfull; ++c) {
            if (c % CPB == 0) {   // chunks c .. c+CPB-1 landed for every wave
                wait_vmcnt(max(NT - c - CPB, 0));
                __builtin_amdgcn_s_barrier();
                pin_q<W16 ? 2 : 4>(qf);
            }
            if (active) {
                if constexpr (W16) attn_step16<false>(Ks + c * 4096, Vs + c * 4096, c * 32, N, lane, qf, scale_log2, m, l, o16);
                else attn_step_pl<false, 16>(Ks + c * 4096, Vs + c * 4096, c * 32, N, lane, qf, scale_log2, m, l, o0, o1);
            }
        }
        if (c < NT) {
            if (c % CPB == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                pin_q<W16 ? 2 : 4>(qf);
            }
            if (active) {
                if constexpr (W16) attn_step16<true>(Ks + c * 4096, Vs + c * 4096, c * 32, N, lane, qf, scale_log2, m, l, o16);
                else if (N - c * 32 <= 8)
                    attn_step_pl<true, 4>(Ks + c * 4096, Vs + c * 4096, c * 32, N, lane, qf, scale_log2, m, l, o0, o1);
                else attn_step_pl<true, 16>(Ks + c * 4096, Vs + c * 4096, c * 32, N, lane, qf, scale_log2, m, l, o0, o1);
            }
        }
        if (!active) return;
        if constexpr (W16) {
            store_strip16(o16, l, out + row0 * D + h * HD, D, sid * 32, q_rows, lane);
        } else {
            uint4 ov[4];
            strip32_out(o0, o1, 1.0f / xor32_sum(l), ov);
            const int q = sid * 32 + l32;
            if constexpr (OUT8) {
                // lane (l32, hh) holds dims 16k + 8hh .. +7 (k = 0..3): block b = dims 32b .. 32b+31 is ov[2b], ov[2b+1]
                // of this lane and of its partner lane l32 + 32 (1 - hh)
                int E[2];
#pragma unroll
                for (int b2 = 0; b2 < 2; ++b2) {
                    uint32_t am = max(mx8_amax8(ov[2 * b2]), mx8_amax8(ov[2 * b2 + 1]));
                    {
                        const auto r = __builtin_amdgcn_permlane32_swap(am, am, false, false);
                        am = max(r[0], r[1]);
                    }
                    E[b2] = mx8_block_exp(am);
                }
                if (q < q_rows) {
                    const int64_t r = row0 + q;
                    uint8_t* orow = out8 + r * ld8 + h * HD + 8 * hh;
#pragma unroll
                    for (int k = 0; k < 4; ++k) *reinterpret_cast<uint2*>(orow + 16 * k) = mx8_pack8(ov[k], E[k >> 1]);
                    s8[mx8_scale_byte(r, h * HD + 32 * hh, lds8)] = (uint8_t)(E[hh] + 127);
                }
            } else {
                if (q < q_rows) store_strip32(out + (row0 + q) * D + h * HD, hh, ov);
            }
        }
    };
    if (w16) run_strip(std::true_type{});   // never with OUT8
    else run_strip(std::false_type{});
}


// ---------------- N > 256 (ViT-L/14 @ 336: N = 577): K / V streamed through a ring, queries in blocks ----------------
// The N <= 256 kernel keeps a head's whole K / V image in LDS (57 KiB at N = 197); at N = 577 that image is 152 KiB, so
// one workgroup fits a CU, its load phase is not overlapped, and 19 strips over 8 waves leave the SIMDs unbalanced
// (rounds 1-4: 9.93 ms per launch at 4096 x 16 heads = 0.225 of the bf16 peak). Here (rounds 5-6):
//  * one workgroup = 4 waves = one 128-query block of one (particle, head): QB = 5 blocks cover N = 577 (four blocks of
//    4 x 32-query strips, then 2 strips, and the 16-query strip of query 576 on a wave of its own, attn_step16). A
//    4-wave workgroup has one wave on each SIMD whatever the dispatcher does (6-wave workgroups land 2/4/3/3 per SIMD,
//    tools/micro/simd_probe.hip). The 16-query strip always has a wave of its own: the host adds a block when every
//    wave of the last one holds a 32-query strip (N % 32 in 1..16 with a multiple of 4 full strips, e.g. N = 400).
//  * four workgroups per CU (round 6; round 5 ran three): one wave of each on every SIMD, so <= 128 VGPRs. A wave runs
//    one strip kind (run_strip, instantiated per kind), so the 32-query strip's registers (o0 / o1 / lacc) and the
//    16-query strip's (o16) are never live together, and one Q load set serves both kinds; the steps are attn_step_lf
//    with the V^T reads after the softmax (126 VGPRs).
//  * K / V arrive in 32-key chunks (4 KiB of K + 4 KiB of V) through a ring of 4 chunk slots (32 KiB per workgroup). A
//    group of 2 chunks = 16 LDS-DMA pieces of 1 KiB, 4 per wave; two groups are resident: while one is computed, the
//    next is in flight. One counted vmcnt + s_barrier per group; after the barrier of group g every wave has finished
//    group g - 1, whose slots take group g + 1.
//  * the blocks of a unit run on one XCD (blockIdx b -> XCD b % 8; consecutive blocks of that XCD are one unit's blocks),
//    so four of the five K / V reads of a unit are L2 hits.
// A row's bits depend on N only, not on q_rows or on the block it falls in. The variants measured against this form
// (round 5: 6-wave / 3-chunk workgroups, the attn_step_pl steps, software pipelining, two strips per wave,
// profiles/r5_lab/attn_stream_*_ab.txt; round 6: ring depths, the step forms and the wave counts,
// profiles/r6_lab/attn_stream_occupancy_ab.txt, tools/variants/_attn_split.py) are not compiled here.
constexpr int STREAM_WAVES = 4;
constexpr int STREAM_CPB = 2;                      // 32-key chunks per group (8 pieces each: 4 per wave per group)
constexpr int STREAM_RING = 2;                     // groups resident in the ring
constexpr int STREAM_SLOTS = STREAM_CPB * STREAM_RING;

__global__ __launch_bounds__(STREAM_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void k_attn_stream(
    const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int N, int H, float scale_log2, int q_rows, int QB,
    int BH) {
    constexpr int WAVES = STREAM_WAVES;
    constexpr int STREAM_LDS = STREAM_SLOTS * 2 * 4096;
    static_assert((STREAM_CPB * 8) % WAVES == 0, "a group's DMA pieces split evenly over the waves");
    constexpr int PPW = STREAM_CPB * 8 / WAVES;    // DMA pieces per wave per group
    __shared__ __attribute__((aligned(16))) char smem[STREAM_LDS];
    char* Ks = smem;
    char* Vs = smem + STREAM_SLOTS * 4096;
    const int xcd = blockIdx.x & 7, w8 = blockIdx.x >> 3;
    const int u = (w8 / QB) * 8 + xcd, qb = w8 - (w8 / QB) * QB;
    if (u >= BH) return;                           // padding of the XCD-grouped grid: the whole workgroup leaves
    const int b = u / H, h = u - (u / H) * H;
    const int D = H * HD;
    const int64_t row0 = (int64_t)b * N;
    const bf16_t* qbase = qkv + row0 * 3 * D + h * HD;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, hh = lane >> 5;
    const int NT = (N + 31) >> 5;                  // 32-key chunks
    const int NG = (NT + STREAM_CPB - 1) / STREAM_CPB;
    const int SF = N >> 5, tail = N & 31;
    const int SF32 = SF + (tail > 16 ? 1 : 0);     // 32-query strips (the last one partial when tail > 16)
    const int st = qb * WAVES + wid;
    const bool act32 = st < SF32 && st * 32 < q_rows;
    const int idle0 = SF32 - (QB - 1) * WAVES;     // first wave of the last block without a 32-query strip
    const bool act16 = tail >= 1 && tail <= 16 && 32 * SF < q_rows && qb == QB - 1 && wid == idle0;   // host: idle0 < WAVES

    // one Q load set for both strip kinds (load_q's rules); the 16-query strip is queries 32 SF ..
    bf16x8 qf[4];
    load_q(qf, qbase, D, N, act16, act16 ? SF * 32 : st * 32, lane);
    // group g = chunks [2g, 2g + 2): piece pi = 0..15 of a group is chunk pi / 8, K (pi & 4 == 0) or V, rows 8 (pi & 3) ..
    // + 7 of that chunk (one 1 KiB wave-instruction, lane-linear destination, swizzle on the source address as in
    // k_attn_bf16_pipe); wave w issues pieces w, w + WAVES, ... Rows >= N read row N - 1 (finite; masked keys).
    auto issue_group = [&](int g) {
        // the lane id re-read through asm: the pieces' addresses are then computed where they are issued instead of
        // being hoisted above the group loop as invariants (which spilled, and a scratch reload's vmcnt wait would
        // drain the DMA stream)
        const int ln = lane_id_asm();
        const int sub = ln >> 3, slot = ln & 7;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int pi = wid + WAVES * i;
            const int cc = pi >> 3, isv = (pi >> 2) & 1, j = pi & 3;
            const int c = g * STREAM_CPB + cc;
            const int r = c * 32 + 8 * j + sub;
            const int ch = isv ? V_SWZ(r, slot) : K_SWZ(r, slot);
            const int sl = c % STREAM_SLOTS;
            __builtin_amdgcn_global_load_lds(
                (gptr_t)(qbase + (isv ? 2 * D : D) + (int64_t)min(r, N - 1) * 3 * D + ch * 8),
                (lptr_t)((isv ? Vs : Ks) + sl * 4096 + j * 1024), 16, 0, 0);
        }
    };
    const int g0 = min(NG, STREAM_RING);
    for (int g = 0; g < g0; ++g) issue_group(g);
    // the Q loads are older than every DMA piece: landed once at most PPW * g0 pieces are outstanding; wait and pin here
    wait_vmcnt(PPW * g0);
    pin_q<4>(qf);
    const int nfull = N >> 5;                      // chunks without padded keys
    // the group loop and the stores of one strip kind; the barrier schedule depends on N only, so every wave of the
    // workgroup passes the same barriers whatever its kind (or none: act = false keeps the barriers, computes nothing)
    auto run_strip = [&](auto k16, bool act) {
        constexpr bool W16 = decltype(k16)::value;
        f32x16 o0 = {}, o1 = {};
        f32x4 lacc = {};
        f32x4 o16[4] = {};
        float m = -INFINITY, l = 0.f;
        for (int g = 0; g < NG; ++g) {
            // this wave's pieces of group g have landed (the groups issued after it stay in flight), then every wave's
            const int issued = min(NG, max(STREAM_RING, g + STREAM_RING - 1));
            wait_vmcnt(PPW * (issued - g - 1));
            __builtin_amdgcn_s_barrier();
            pin_q<W16 ? 2 : 4>(qf);
            // into group g - 1's slots, which every wave has finished
            if (g >= 1 && g + STREAM_RING - 1 < NG) issue_group(g + STREAM_RING - 1);
            const int c_end = min((g + 1) * STREAM_CPB, nfull);
#pragma unroll 1
            for (int c = g * STREAM_CPB; c < c_end; ++c) {   // the group's chunks without padded keys
                const int sl = c % STREAM_SLOTS;
                const char* Kt = Ks + sl * 4096;
                const char* Vt = Vs + sl * 4096;
                if (act) {
                    if constexpr (W16) attn_step16<false>(Kt, Vt, c * 32, N, lane, qf, scale_log2, m, l, o16);
                    else attn_step_lf<false, 16>(Kt, Vt, c * 32, N, lane, qf, scale_log2, c == 0, m, lacc, o0, o1);
                }
            }
        }
        if (nfull < NT && act) {   // the chunk with padded keys: the last one, in the last group (its barrier has passed)
            const int c = nfull, sl = c % STREAM_SLOTS;
            const char* Kt = Ks + sl * 4096;
            const char* Vt = Vs + sl * 4096;
            if constexpr (W16) attn_step16<true>(Kt, Vt, c * 32, N, lane, qf, scale_log2, m, l, o16);
            else if (N - c * 32 <= 8) attn_step_lf<true, 4>(Kt, Vt, c * 32, N, lane, qf, scale_log2, c == 0, m, lacc, o0, o1);
            else attn_step_lf<true, 16>(Kt, Vt, c * 32, N, lane, qf, scale_log2, c == 0, m, lacc, o0, o1);
        }
        if (!act) return;
        if constexpr (W16) {
            store_strip16(o16, l, out + row0 * D + h * HD, D, SF * 32, q_rows, lane);
        } else {
            uint4 ov[4];
            strip32_out(o0, o1, 1.0f / xor32_sum(lacc[0]), ov);
            const int q = st * 32 + l32;
            if (q < q_rows) store_strip32(out + (row0 + q) * D + h * HD, hh, ov);
        }
    };
    if (act16) run_strip(std::true_type{}, true);
    else run_strip(std::false_type{}, act32);
}

// CLS-only attention (q_rows == 1: the last encoder block, whose other query rows feed nothing): one wave
// per (particle, head), 4 per workgroup, no LDS, so occupancy is set by VGPRs and many heads stream K / V
// at once (the path is pure HBM streaming: 2 x N x 128 B per head for one query).
//   scores: lane j owns keys j, j+64, ...; K rows read whole (128 B) from global; fp32 dot with the CLS
//           query (broadcast loads), wave max / sum -> fp32 softmax in the exp2 domain;
//   PV:     lane (g, d8) = (lane >> 3, lane & 7) accumulates dims 8*d8..8*d8+7 over keys j = g (mod 8),
//           probabilities fetched with ds_bpermute, then a 3-step shuffle reduction over g.
constexpr int CLS_MAXT = 10;   // keys per lane in the score phase: N <= 640
__global__ __launch_bounds__(256) void k_attn_cls_bf16(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                       int N, int H, int BH, float scale_log2) {
    const int lane = threadIdx.x & 63;
    const int bh = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bh >= BH) return;
    const int b = bh / H, h = bh - (bh / H) * H;
    const int D = H * HD;
    const bf16_t* base = qkv + (int64_t)b * N * 3 * D + h * HD;
    float q[HD];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint4 u = *reinterpret_cast<const uint4*>(base + c * 8);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            q[c * 8 + 2 * e] = bf2f((bf16_t)(w[e] & 0xffff));
            q[c * 8 + 2 * e + 1] = bf2f((bf16_t)(w[e] >> 16));
        }
    }
    float sc[CLS_MAXT];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < CLS_MAXT; ++t) {
        const int j = lane + 64 * t;
        float sv = -INFINITY;
        if (j < N) {
            const bf16_t* kr = base + (int64_t)j * 3 * D + D;
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint4 u = *reinterpret_cast<const uint4*>(kr + c * 8);
                const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc = fmaf(q[c * 8 + 2 * e], bf2f((bf16_t)(w[e] & 0xffff)), acc);
                    acc = fmaf(q[c * 8 + 2 * e + 1], bf2f((bf16_t)(w[e] >> 16)), acc);
                }
            }
            sv = acc * scale_log2;
        }
        sc[t] = sv;
        mx = fmaxf(mx, sv);
    }
    mx = wave_max(mx);
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < CLS_MAXT; ++t) {
        sc[t] = (lane + 64 * t < N) ? __builtin_amdgcn_exp2f(sc[t] - mx) : 0.f;
        l += sc[t];
    }
    l = wave_sum(l);
    const int g = lane >> 3, d8 = lane & 7;
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < CLS_MAXT; ++t) {
        if (64 * t >= N) break;
#pragma unroll
        for (int ii = 0; ii < 8; ++ii) {
            const int j = 64 * t + 8 * ii + g;            // keys of this (t, ii) block: 8 consecutive
            const float pj = __shfl(sc[t], 8 * ii + g, 64);
            if (j < N) {
                const uint4 u = *reinterpret_cast<const uint4*>(base + (int64_t)j * 3 * D + 2 * D + d8 * 8);
                const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[2 * e] = fmaf(pj, bf2f((bf16_t)(w[e] & 0xffff)), o[2 * e]);
                    o[2 * e + 1] = fmaf(pj, bf2f((bf16_t)(w[e] >> 16)), o[2 * e + 1]);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o[e] += __shfl_xor(o[e], 8, 64);
        o[e] += __shfl_xor(o[e], 16, 64);
        o[e] += __shfl_xor(o[e], 32, 64);
    }
    if (g == 0) {
        const float inv = 1.0f / l;
        bf16_t* orow = out + (int64_t)b * N * D + h * HD + d8 * 8;
        *reinterpret_cast<uint4*>(orow) = make_uint4(pack_bf2(o[0] * inv, o[1] * inv), pack_bf2(o[2] * inv, o[3] * inv),
                                                     pack_bf2(o[4] * inv, o[5] * inv), pack_bf2(o[6] * inv, o[7] * inv));
    }
}

// ---------------- fp32 parity path ----------------
// One thread per query; K / V of the (particle, head) stream through LDS in chunks of KC keys, so any N
// works (ViT-L/14 @ 336: N = 577). Exact two-pass softmax in key order: pass 1 the row max over all keys,
// pass 2 p = expf(s*scale - max), l += p, acc += p v.
constexpr int KC = 128;
__global__ __launch_bounds__(256) void k_attn_f32(const float* __restrict__ qkv, float* __restrict__ out, int N,
                                                  int H, float scale, int q_rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Ks = reinterpret_cast<float*>(smem);
    float* Vs = Ks + KC * HD;
    const int bh = blockIdx.x;
    const int b = bh / H, h = bh - (bh / H) * H;
    const int D = H * HD;
    const int64_t row0 = (int64_t)b * N;
    const float* qbase = qkv + row0 * 3 * D + h * HD;
    auto stage = [&](int c0, bool with_v) {
        const int rows = min(KC, N - c0);
        __syncthreads();
        for (int idx = threadIdx.x; idx < rows * HD; idx += blockDim.x) {
            const int r = idx / HD, c = idx - (idx / HD) * HD;
            Ks[idx] = qbase[(int64_t)(c0 + r) * 3 * D + D + c];
            if (with_v) Vs[idx] = qbase[(int64_t)(c0 + r) * 3 * D + 2 * D + c];
        }
        __syncthreads();
        return rows;
    };
    for (int q0 = 0; q0 < q_rows; q0 += blockDim.x) {
        const int q = q0 + threadIdx.x;
        const bool active = q < q_rows;
        float qv[HD];
        for (int c = 0; c < HD; ++c) qv[c] = active ? qbase[(int64_t)q * 3 * D + c] : 0.f;
        float mx = -INFINITY;
        for (int c0 = 0; c0 < N; c0 += KC) {
            const int rows = stage(c0, false);
            if (active)
                for (int k = 0; k < rows; ++k) {
                    float s = 0.f;
                    for (int c = 0; c < HD; ++c) s = fmaf(qv[c], Ks[k * HD + c], s);
                    mx = fmaxf(mx, s * scale);
                }
        }
        float acc[HD];
        for (int c = 0; c < HD; ++c) acc[c] = 0.f;
        float l = 0.f;
        for (int c0 = 0; c0 < N; c0 += KC) {
            const int rows = stage(c0, true);
            if (active)
                for (int k = 0; k < rows; ++k) {
                    float s = 0.f;
                    for (int c = 0; c < HD; ++c) s = fmaf(qv[c], Ks[k * HD + c], s);
                    const float p = expf(s * scale - mx);
                    l += p;
                    for (int c = 0; c < HD; ++c) acc[c] = fmaf(p, Vs[k * HD + c], acc[c]);
                }
        }
        if (active) {
            float* orow = out + (row0 + q) * D + h * HD;
            for (int c = 0; c < HD; ++c) orow[c] = acc[c] / l;
        }
    }
}

// ---------------- host side ----------------
constexpr float LOG2E = 1.44269504088896341f;   // the kernels exponentiate with exp2: scale_log2 = scale * log2(e)

// N <= 256: the key-pipelined kernel (8 waves, one strip each, the head's whole K / V image in LDS), bf16 or MX8 output
template <bool OUT8>
int launch_pipe(const uint16_t* qkv, uint16_t* out, int64_t B, int N, int H, float scale, int q_rows, uint8_t* out8,
                int ld8, uint8_t* s8, int lds8, void* stream) {
    const int NP = (N + 31) & ~31;
    const size_t lds = (size_t)NP * ROWB * 2;   // the K image + the V image
    static bool attr = false;   // benign race: idempotent attribute set
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)k_attn_bf16_pipe<OUT8>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024);
        attr = true;
    }
    hipLaunchKernelGGL((k_attn_bf16_pipe<OUT8>), dim3((unsigned)(B * H)), dim3(512), lds, (hipStream_t)stream, qkv, out,
                       N, H, scale * LOG2E, q_rows, out8, ld8, s8, lds8);
    VPF_RETURN_LAUNCH();
}

}  // namespace

VPF_API int vpf_attention_bf16(const uint16_t* qkv, uint16_t* out, int64_t B, int N, int H, int hd, float scale,
                               int q_rows, void* stream) {
    if (B < 0 || N <= 0 || N > 640 || H <= 0 || hd != HD || B * H > INT32_MAX || q_rows < 1 || q_rows > N)
        return VPF_ERR_ARG;
    if (B == 0) return 0;
    const float scale_log2 = scale * LOG2E;
    const int64_t BH = B * H;
    if (q_rows == 1) {
        hipLaunchKernelGGL(k_attn_cls_bf16, dim3((unsigned)((BH + 3) / 4)), dim3(256), 0, (hipStream_t)stream, qkv, out,
                           N, H, (int)BH, scale_log2);
        VPF_RETURN_LAUNCH();
    }
    // N <= 256: the key-pipelined kernel; N > 256: the key-streamed, query-blocked kernel
    if (N <= 256) return launch_pipe<false>(qkv, out, B, N, H, scale, q_rows, nullptr, 0, nullptr, 0, stream);
    constexpr int W = STREAM_WAVES;
    const int sf32 = (N >> 5) + ((N & 31) > 16 ? 1 : 0);
    const int need = sf32 < (q_rows + 31) / 32 ? sf32 : (q_rows + 31) / 32;   // 32-query strips holding rows < q_rows
    const int t32 = N & 31;   // + the 16-query strip, which runs on a wave of its own (k_attn_stream's idle0 < WAVES)
    const int need16 = need + (t32 >= 1 && t32 <= 16 && 32 * (N >> 5) < q_rows ? 1 : 0);
    const int QB = need16 > W ? (need16 + W - 1) / W : 1;
    const int64_t blocks = (BH + 7) / 8 * 8 * QB;
    if (blocks > INT32_MAX) return VPF_ERR_ARG;
    hipLaunchKernelGGL(k_attn_stream, dim3((unsigned)blocks), dim3(64 * W), 0,
                       (hipStream_t)stream,
                       reinterpret_cast<const bf16_t*>(qkv), reinterpret_cast<bf16_t*>(out), N, H, scale_log2, q_rows,
                       QB, (int)BH);
    VPF_RETURN_LAUNCH();
}

VPF_API int vpf_attention_bf16_mx8(const uint16_t* qkv, int64_t B, int N, int H, int hd, float scale, uint8_t* out8,
                                   int64_t ld8, uint32_t* s8, int64_t lds, void* stream) {
    const int64_t D = (int64_t)H * HD;
    if (B < 0 || N <= 0 || N > 256 || H <= 0 || hd != HD || B * H > INT32_MAX || D % 128 != 0) return VPF_ERR_ARG;
    if (!qkv || !out8 || !s8 || ld8 < D || ld8 % 8 != 0 || ((uintptr_t)out8 & 7) || lds % 64 != 0 ||
        lds < B * N || ld8 > INT32_MAX || lds > INT32_MAX / 4)
        return VPF_ERR_ARG;
    if (B == 0) return 0;
    return launch_pipe<true>(qkv, nullptr, B, N, H, scale, N, out8, (int)ld8, reinterpret_cast<uint8_t*>(s8), (int)lds,
                             stream);
}

VPF_API int vpf_attention_f32(const float* qkv, float* out, int64_t B, int N, int H, int hd, float scale,
                              int q_rows, void* stream) {
    if (B < 0 || N <= 0 || N > 4096 || H <= 0 || hd != HD || B * H > INT32_MAX || q_rows < 1 || q_rows > N)
        return VPF_ERR_ARG;
    if (B == 0) return 0;
    const size_t lds = (size_t)KC * HD * 4 * 2;   // one K chunk + one V chunk
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)k_attn_f32, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    hipLaunchKernelGGL(k_attn_f32, dim3((unsigned)(B * H)), dim3(256), lds, (hipStream_t)stream, qkv, out, N, H,
                       scale, q_rows);
    VPF_RETURN_LAUNCH();
}
