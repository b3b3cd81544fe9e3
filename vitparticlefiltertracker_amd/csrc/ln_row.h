// One LayerNorm row per wave, held in registers: what layernorm.hip's kernels (LayerNorm, the CLS weight) and
// token_weight.hip's (the patch-token weight, SPEC S18) share, so that both apply the same operations in the same order.
//
// Lane i holds the 4-element chunks i, i+64, i+128, i+192 (D <= 1024, D % 4 == 0), so the row is read once; mean and
// variance are two wave reductions over the register copy (two-pass, fp32).
#pragma once
#include "vpf_common.h"

namespace vpf {

// Four consecutive elements: `Raw` is what one load returns, `unpack` converts it to fp32 (a kernel that prefetches the
// next row keeps the Raw registers and unpacks when it needs the values).
template <typename T> struct Vec4;
template <> struct Vec4<float> {
    typedef float4 Raw;
    static __device__ __forceinline__ Raw load_raw(const float* p) { return *reinterpret_cast<const float4*>(p); }
    static __device__ __forceinline__ void unpack(const Raw& x, float v[4]) {
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    }
    static __device__ __forceinline__ void load(const float* p, float v[4]) { unpack(load_raw(p), v); }
    static __device__ __forceinline__ void store(float* p, const float v[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <> struct Vec4<bf16_t> {
    typedef uint2 Raw;
    static __device__ __forceinline__ Raw load_raw(const bf16_t* p) { return *reinterpret_cast<const uint2*>(p); }
    static __device__ __forceinline__ void unpack(const Raw& x, float v[4]) {
        v[0] = bf2f((bf16_t)(x.x & 0xffff)); v[1] = bf2f((bf16_t)(x.x >> 16));
        v[2] = bf2f((bf16_t)(x.y & 0xffff)); v[3] = bf2f((bf16_t)(x.y >> 16));
    }
    static __device__ __forceinline__ void load(const bf16_t* p, float v[4]) { unpack(load_raw(p), v); }
    static __device__ __forceinline__ void store(bf16_t* p, const float v[4]) {
        *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
    }
};

// {mean, rstd} of a row in registers (up to 4 chunks of 4 per lane; the chunks past D hold zeros).
__device__ __forceinline__ void ln_stats(int D, float eps, int lane, const float v[16], float& mean, float& rstd) {
    const int nch = D >> 2;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) s += (v[4 * i] + v[4 * i + 1]) + (v[4 * i + 2] + v[4 * i + 3]);
    }
    mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[4 * i + e] - mean; q = fmaf(d, d, q); }
        }
    }
    const float var = wave_sum(q) / (float)D;
    rstd = 1.0f / sqrtf(var + eps);
}

// The affine step of one chunk: v <- (v - mean) rstd gamma + beta.
__device__ __forceinline__ void ln_affine4(float v[4], float mean, float rstd, const float4& gg, const float4& bb) {
    v[0] = (v[0] - mean) * rstd * gg.x + bb.x;
    v[1] = (v[1] - mean) * rstd * gg.y + bb.y;
    v[2] = (v[2] - mean) * rstd * gg.z + bb.z;
    v[3] = (v[3] - mean) * rstd * gg.w + bb.w;
}

// Normalise a row already in registers, in place.
__device__ __forceinline__ void ln_regs(int D, const float* __restrict__ g, const float* __restrict__ b, float eps,
                                        int lane, float v[16]) {
    const int nch = D >> 2;
    float mean, rstd;
    ln_stats(D, eps, lane, v, mean, rstd);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < nch)
            ln_affine4(v + 4 * i, mean, rstd, *reinterpret_cast<const float4*>(g + 4 * c),
                       *reinterpret_cast<const float4*>(b + 4 * c));
    }
}

// Load one row and normalise it. Returns values in v.
template <typename T>
__device__ __forceinline__ void ln_row(const T* __restrict__ x, int D, const float* __restrict__ g,
                                       const float* __restrict__ b, float eps, int lane, float v[16]) {
    const int nch = D >> 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            Vec4<T>::load(x + 4 * c, v + 4 * i);
        } else {
            v[4 * i] = v[4 * i + 1] = v[4 * i + 2] = v[4 * i + 3] = 0.f;
        }
    }
    ln_regs(D, g, b, eps, lane, v);
}

}  // namespace vpf
