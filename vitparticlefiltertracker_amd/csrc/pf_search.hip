// Search predict (SPEC S16): once the occlusion gate has held for `after` frames the target may be anywhere, so this
// frame's predict scatters the particles over the whole frame instead of diffusing them (S2 / S11).
//
// k_predict_search: one thread per particle, launched as k_predict is. The position is a jittered, hole-free lattice
// in the GLOBAL index gi alone, so the bits do not depend on the sharding: particle gi owns the y-stratum
// [gi / P, (gi + 1) / P) of the frame and the x-stratum c = gi mod gx of its band, and the words r0, r1 of Philox counter
// (gi, frame, 0, 3) place it inside the cell. Each run of gx consecutive particles covers one band with one particle
// per x-stratum; no cell is empty for any P. The scale row takes exactly S2's step (n2 of counter (gi, frame, 0, 0)),
// so it has the bits an ordinary predict gives it. The CV instance also stores +0.0f to both velocity rows: a stale
// velocity would throw the re-acquired cloud off. The old x, y (and vx, vy) are not read. The angle row's predict
// (k_predict_angle) follows unchanged. Every operation is one rounded fp32 operation; gx, 1 / gx and 1 / P come from the
// host (config.redetect_lattice).
#pragma clang fp contract(off)
#include "vpf_common.h"
#include "../../include/vpf.h"
#include "pf_predict.h"

using namespace vpf;

struct SearchParams { float sig_s, width, height, smin, smax, inv_gx, inv_P; uint32_t gx; };

template <bool CV>
__device__ __forceinline__ void predict_search(float* __restrict__ p, int64_t ld, int64_t n, int64_t gbegin,
                                               uint32_t k0, uint32_t k1, uint32_t frame, const SearchParams& c) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t gi = (uint32_t)(gbegin + i);        // < P <= 2^24: exact as fp32
    const Noise3 z = predict_noise(gi, frame, k0, k1);
    const u32x4 q = philox4x32_10(gi, frame, 0u, 3u, k0, k1);
    const float u0 = uniform01(q.v[0]), u1 = uniform01(q.v[1]);
    const float wm1 = c.width - 1.0f, hm1 = c.height - 1.0f;
    const float col = (float)(gi % c.gx);
    p[i] = clampf(((col + u0) * c.inv_gx) * wm1, 0.0f, wm1);
    p[ld + i] = clampf((((float)gi + u1) * c.inv_P) * hm1, 0.0f, hm1);
    p[2 * ld + i] = predict_scale(p[2 * ld + i], c.sig_s, z.n2, c.smin, c.smax);
    if constexpr (CV) {
        p[3 * ld + i] = 0.0f;
        p[4 * ld + i] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_predict_search(float* __restrict__ p, int64_t ld, int64_t n, int64_t gbegin,
                                                        uint32_t k0, uint32_t k1, uint32_t frame, SearchParams c) {
    predict_search<false>(p, ld, n, gbegin, k0, k1, frame, c);
}

__global__ __launch_bounds__(256) void k_predict_search_cv(float* __restrict__ p, int64_t ld, int64_t n,
                                                           int64_t gbegin, uint32_t k0, uint32_t k1, uint32_t frame,
                                                           SearchParams c) {
    predict_search<true>(p, ld, n, gbegin, k0, k1, frame, c);
}

VPF_API int vpf_predict_search(float* particles, int64_t n, int64_t ld, int64_t global_begin, int64_t P, int rows,
                               uint64_t seed, uint32_t frame, float sig_s, float width, float height, float smin,
                               float smax, int64_t gx, float inv_gx, float inv_P, void* stream) {
    if (!predict_args_ok(n, ld, global_begin)) return VPF_ERR_ARG;
    if ((rows != 3 && rows != 5) || P < 1 || P > ((int64_t)1 << 24) || global_begin + n > P || gx < 1 ||
        gx > (int64_t)0xffffffffLL)
        return VPF_ERR_ARG;
    if (n == 0) return 0;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const SearchParams c{sig_s, width, height, smin, smax, inv_gx, inv_P, (uint32_t)gx};
    if (rows == 5)
        hipLaunchKernelGGL(k_predict_search_cv, dim3(blocks), dim3(256), 0, (hipStream_t)stream, particles, ld, n,
                           global_begin, (uint32_t)seed, (uint32_t)(seed >> 32), frame, c);
    else
        hipLaunchKernelGGL(k_predict_search, dim3(blocks), dim3(256), 0, (hipStream_t)stream, particles, ld, n,
                           global_begin, (uint32_t)seed, (uint32_t)(seed >> 32), frame, c);
    VPF_RETURN_LAUNCH();
}
