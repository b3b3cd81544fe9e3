// Patch-token likelihood (SPEC S18): final LN of every patch-token row -> cosine with that row's own template -> mean
// over the rows -> fixed-point weight, multiplied into Q.
//
// k_token_weight. Memory-bound: one pass over the n (N - 1) token rows. One wave per particle, TW_WAVES particles per
// workgroup, all of them walking j = 1 .. N - 1 together: template row j is staged in LDS once per workgroup (two
// buffers, one barrier per j) instead of once per particle. A wave keeps its row in registers as ln_row.h holds it and
// applies the LayerNorm with gamma / beta held in registers (read once per wave, not once per row).
// Every global load of the loop is issued at one place, right after the previous row's registers have been unpacked:
// the template chunk and the token row of step j + 1, unconditionally (indices clamped, never branched on), and the one
// full wait of a step sits at its top, where exactly those loads are needed. Between the two lie the barrier and the
// whole arithmetic of row j, which touch no pending register, so the compiler places no other vector-memory wait in
// the loop and a wave has a row in flight all the time.
//
// The sum over j is one fp32 chain per particle in increasing j, from +0: fixed, independent of n and of the grid, no
// atomics; wave_sum leaves the same value in every lane, so every lane carries the same chain.
//
// k_token_rows (tmpl == NULL): the LN'd rows only. No template row is shared, so it takes one wave per row, as
// k_layernorm does: a template update of one or two crops is then N - 1 independent waves per crop, not one wave
// walking N - 1 rows.
#include "vpf_common.h"
#include "ln_row.h"
#include "../../include/vpf.h"

using namespace vpf;

namespace {

constexpr int TW_WAVES = 8;     // particles per workgroup (one wave each)

// crop.hip's mul_shift: (a b) >> sh with the 128-bit product.
__device__ __forceinline__ uint64_t mul_shift(uint64_t a, uint64_t b, int sh) {
    const uint64_t hi = __umul64hi(a, b), lo = a * b;
    return sh ? (hi << (64 - sh)) | (lo >> sh) : lo;
}

template <typename T, bool DO_LN>
__global__ __launch_bounds__(64 * TW_WAVES) void k_token_weight(
    const T* __restrict__ tok, int64_t n, int N, int D, const float* __restrict__ g, const float* __restrict__ b,
    float eps, const float* __restrict__ tmpl, float lam, double scale, int sh, int combine, float* __restrict__ feat,
    float* __restrict__ tok_sim, float* __restrict__ sim_out, int64_t* __restrict__ Q) {
    typedef typename Vec4<T>::Raw Raw;
    __shared__ float4 st[2][256];                       // template row j, D <= 1024
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t p = (int64_t)blockIdx.x * TW_WAVES + (tid >> 6);
    const bool valid = p < n;                           // wave-uniform; every wave keeps the barriers and the loads
    const int nch = D >> 2, np = N - 1;
    const int nit = (nch + 63) >> 6;                    // chunks per lane: wave-uniform
    // a wave past n reads the last particle's rows (in bounds, cached) and computes nothing
    const T* rows = tok + ((valid ? p : n - 1) * N + 1) * (int64_t)D;
    const float4* t4 = reinterpret_cast<const float4*>(tmpl);
    // a lane's chunk i, clamped into the row: a lane past the row's end re-reads the last chunk and ignores it
    int cc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cc[i] = min(lane + 64 * i, nch - 1);
    const int tc = min(tid, nch - 1);                   // the template chunk this thread stages

    float4 gg[4], bb[4];
    if constexpr (DO_LN) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < nit) {
                gg[i] = *reinterpret_cast<const float4*>(g + 4 * cc[i]);
                bb[i] = *reinterpret_cast<const float4*>(b + 4 * cc[i]);
            }
        }
    }
    float4 tn = t4[tc];
    Raw nxt[4] = {};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < nit) nxt[i] = Vec4<T>::load_raw(rows + 4 * cc[i]);
    float S = 0.f;
    for (int j = 0; j < np; ++j) {
        // the step's one wait: row j and template chunk j, issued a whole step ago
        float v[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (lane + 64 * i < nch) Vec4<T>::unpack(nxt[i], v + 4 * i);
            else v[4 * i] = v[4 * i + 1] = v[4 * i + 2] = v[4 * i + 3] = 0.f;
        }
        // buffer j & 1 was last read at j - 2; a wave writing it here has passed barrier j - 1, which every wave
        // reaches only after those reads
        if (tid < nch) st[j & 1][tid] = tn;
        // step j + 1's loads (the last step re-reads its own row: one row in N - 1, and no branch)
        const int jn = min(j + 1, np - 1);
        tn = t4[(int64_t)jn * nch + tc];
        const T* row = rows + (int64_t)jn * D;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nit) nxt[i] = Vec4<T>::load_raw(row + 4 * cc[i]);
        __syncthreads();
        if (!valid) continue;
        if constexpr (DO_LN) {
            float mean, rstd;
            ln_stats(D, eps, lane, v, mean, rstd);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (lane + 64 * i < nch) ln_affine4(v + 4 * i, mean, rstd, gg[i], bb[i]);
        }
        if (feat) {
            float* f = feat + (p * np + j) * (int64_t)D;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = lane + 64 * i;
                if (c < nch) Vec4<float>::store(f + 4 * c, v + 4 * i);
            }
        }
        // k_cls_weight's row arithmetic against template row j
        float dot = 0.f, nn = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) {
                const float4 t = st[j & 1][c];
                dot = fmaf(v[4 * i], t.x, dot); dot = fmaf(v[4 * i + 1], t.y, dot);
                dot = fmaf(v[4 * i + 2], t.z, dot); dot = fmaf(v[4 * i + 3], t.w, dot);
                nn = fmaf(v[4 * i], v[4 * i], nn); nn = fmaf(v[4 * i + 1], v[4 * i + 1], nn);
                nn = fmaf(v[4 * i + 2], v[4 * i + 2], nn); nn = fmaf(v[4 * i + 3], v[4 * i + 3], nn);
            }
        }
        dot = wave_sum(dot);
        nn = wave_sum(nn);
        // SPEC S5 per row: a zero row has sim 0; a row with a NaN / inf (or whose squared norm overflows fp32) NaN
        const bool finite = isfinite(dot) && isfinite(nn);
        const float sim = !finite ? __builtin_nanf("") : (nn > 0.f ? dot / sqrtf(nn) : 0.f);
        S += sim;
        if (tok_sim && lane == 0) tok_sim[p * np + j] = sim;
    }
    if (valid && lane == 0) {
        // SPEC S18: the mean, then S5's weight form; a non-finite mean (a NaN row) has zero weight
        const float sim = S / (float)np;
        const float w = isfinite(sim) ? fixed_expf(lam * (fminf(sim, 1.0f) - 1.0f)) : 0.0f;
        const uint64_t lt = (uint64_t)(int64_t)floor((double)w * scale);
        Q[p] = (int64_t)(combine ? mul_shift((uint64_t)Q[p], lt, sh) : lt);
        if (sim_out) sim_out[p] = sim;
    }
}

// feat[p][j - 1] = LN(tok[p][j]) (DO_LN) or the row itself, j = 1 .. N - 1: one wave per row.
template <typename T, bool DO_LN>
__global__ __launch_bounds__(256) void k_token_rows(const T* __restrict__ tok, int64_t rows, int N, int D,
                                                    const float* __restrict__ g, const float* __restrict__ b,
                                                    float eps, float* __restrict__ feat) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int np = N - 1, nch = D >> 2;
    const int64_t p = r / np;
    const T* x = tok + (p * N + 1 + (r - p * np)) * (int64_t)D;
    float v[16];
    if constexpr (DO_LN) {
        ln_row<T>(x, D, g, b, eps, lane, v);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i;
            if (c < nch) Vec4<T>::load(x + 4 * c, v + 4 * i);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) Vec4<float>::store(feat + r * D + 4 * c, v + 4 * i);
    }
}

template <typename T>
int tokw_launch(const T* tokens, int64_t n, int N, int D, const float* gamma, const float* beta, float eps,
                const float* tmpl, float lam, int bits, int combine, float* feat_out, float* tok_sim_out,
                float* sim_out, int64_t* Q, void* stream) {
    if (n < 0 || N < 2 || D < 4 || D % 4 != 0 || D > 1024 || bits < 0 || bits > 61 || !(lam >= 0.f) ||
        !(lam <= 3.4028234663852886e38f))
        return VPF_ERR_ARG;
    if (n == 0) return 0;       // no rows: nothing to read or write (an empty buffer's pointer may be NULL)
    if (!tokens || (gamma && !beta) || (tmpl ? !Q : !feat_out)) return VPF_ERR_ARG;
    if (((uintptr_t)tokens & (4 * sizeof(T) - 1)) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15) ||
        ((uintptr_t)tmpl & 15) || ((uintptr_t)feat_out & 15) || ((uintptr_t)tok_sim_out & 3) ||
        ((uintptr_t)sim_out & 3) || ((uintptr_t)Q & 7))
        return VPF_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (!tmpl) {
        const int64_t rows = n * (N - 1), blocks = (rows + 3) / 4;
        if (blocks > INT32_MAX) return VPF_ERR_ARG;
        if (gamma)
            hipLaunchKernelGGL((k_token_rows<T, true>), dim3((unsigned)blocks), dim3(256), 0, s, tokens, rows, N, D,
                               gamma, beta, eps, feat_out);
        else
            hipLaunchKernelGGL((k_token_rows<T, false>), dim3((unsigned)blocks), dim3(256), 0, s, tokens, rows, N, D,
                               gamma, beta, eps, feat_out);
        VPF_RETURN_LAUNCH();
    }
    const int64_t blocks = (n + TW_WAVES - 1) / TW_WAVES;
    if (blocks > INT32_MAX) return VPF_ERR_ARG;
    const dim3 grid((unsigned)blocks), block(64 * TW_WAVES);
    const double scale = ldexp(1.0, bits);
    if (gamma)
        hipLaunchKernelGGL((k_token_weight<T, true>), grid, block, 0, s, tokens, n, N, D, gamma, beta, eps, tmpl, lam,
                           scale, bits, combine, feat_out, tok_sim_out, sim_out, Q);
    else
        hipLaunchKernelGGL((k_token_weight<T, false>), grid, block, 0, s, tokens, n, N, D, gamma, beta, eps, tmpl, lam,
                           scale, bits, combine, feat_out, tok_sim_out, sim_out, Q);
    VPF_RETURN_LAUNCH();
}

}  // namespace

VPF_API int vpf_token_weight_bf16(const uint16_t* tokens, int64_t n, int N, int D, const float* gamma,
                                  const float* beta, float eps, const float* tmpl, float lam, int bits, int combine,
                                  float* feat_out, float* tok_sim_out, float* sim_out, int64_t* Q, void* stream) {
    return tokw_launch<bf16_t>(tokens, n, N, D, gamma, beta, eps, tmpl, lam, bits, combine, feat_out, tok_sim_out,
                               sim_out, Q, stream);
}
VPF_API int vpf_token_weight_f32(const float* tokens, int64_t n, int N, int D, const float* gamma, const float* beta,
                                 float eps, const float* tmpl, float lam, int bits, int combine, float* feat_out,
                                 float* tok_sim_out, float* sim_out, int64_t* Q, void* stream) {
    return tokw_launch<float>(tokens, n, N, D, gamma, beta, eps, tmpl, lam, bits, combine, feat_out, tok_sim_out,
                              sim_out, Q, stream);
}
