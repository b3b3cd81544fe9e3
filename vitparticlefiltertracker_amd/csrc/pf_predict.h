// The predict kernels' shared pieces (SPEC S2, S11, S12, S16), each defined once: Box-Muller on two Philox words, the
// clamp, S2's noise triple and log-normal scale step, and the entry points' common shape check. pf_kernels.hip builds
// the random walk, the constant-velocity model and the angle row's predict from them, pf_search.hip SPEC S16's search
// predict. Everything here is compiled with fp contraction off, as the files that include it are.
#pragma once
#pragma clang fp contract(off)
#include "vpf_common.h"

using namespace vpf;

// The pieces predict's two motion models share (SPEC S2, S11), each defined once.
// Two standard normals from two Philox words (Box-Muller): rad = sqrt(-2 ln u(w0)), (rad cos, rad sin)(2 pi u(w1)).
__device__ __forceinline__ void gauss_pair(uint32_t w0, uint32_t w1, float& a, float& b) {
    const float rad = __builtin_sqrtf(-2.0f * fixed_logf(uniform01(w0)));
    float c, s;
    fixed_sincos2pi(uniform01(w1), c, s);
    a = rad * c; b = rad * s;
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// Particle gi's S2 noise n0, n1, n2 from Philox counter (gi, frame, 0, 0).
struct Noise3 { float n0, n1, n2; };
__device__ __forceinline__ Noise3 predict_noise(uint32_t gi, uint32_t frame, uint32_t k0, uint32_t k1) {
    const u32x4 r = philox4x32_10(gi, frame, 0u, 0u, k0, k1);
    Noise3 z;
    float unused;
    gauss_pair(r.v[0], r.v[1], z.n0, z.n1);
    gauss_pair(r.v[2], r.v[3], z.n2, unused);
    return z;
}

// S2's log-normal scale step.
__device__ __forceinline__ float predict_scale(float s, float sig_s, float n2, float smin, float smax) {
    return clampf(s * fixed_expf(sig_s * n2), smin, smax);
}

static bool predict_args_ok(int64_t n, int64_t ld, int64_t global_begin) {
    return !(n < 0 || ld < n || global_begin < 0 || (global_begin + n) > (int64_t)0xffffffffLL);
}
