// Particle-filter kernels (SPEC S2, S6, S7, S10, S11).
//
// predict: one thread per particle, counter-based Philox so the noise depends only on (seed, frame,
//   global index) and never on the sharding. The random walk (k_predict) and the constant-velocity model
//   (k_predict_cv, SPEC S11) share the noise, clamp and scale pieces (pf_predict.h; pf_search.hip builds SPEC S16's
//   search predict from the same); the velocity rows are resampled and summed by k_gather_rows / vpf_weighted_sums over the same global view and the same tree as the states. The angle row
//   (SPEC S12) has a kernel of its own, k_predict_angle, launched after either model's, and the same gather and sums.
// Three shared pieces, each defined once in pf_tree.h (pf_gate.hip builds SPEC S15's occlusion-gated instances from
// the same), carry SPEC S6 / S7 / S10's "same arithmetic in the same order":
//   stats_tree: one 1024-thread workgroup's fixed-order sums (int64 T exact, three fp64 sums; the adaptive
//     instance adds an exact 128-bit sum of squares and the maximum). Thread t takes i = t, t + 1024, ... in
//     order, then a 512 -> 1 pairwise halving.
//   block_scan_cdf: the workgroup's inclusive int64 scan into a CDF, 4 elements per thread, a wave scan by
//     DPP-free shuffles, one LDS carry per 4096-element chunk.
//   cdf_upper_bound + gather_store: a slot's ancestor a = min{i : C_i > pos} and the copy of its state.
// Their users: k_shard_stats (vpf_shard_stats over one shard's flat arrays, vpf_weighted_sums over further rows of
// the global view), k_scan + k_resample_search over one shard's flat arrays (vpf_resample), and over the global set
// (the product path) k_stats_scan_global + k_resample_global and their
// adaptive _ex instances (SPEC S10: the ESS gate decided once on the device, then per slot either the systematic /
// stratified search or the identity copy with the weight carry), each pair two instances of one body. All integer
// where it matters: ancestors are bit-identical to oracle/pf_oracle.c for any shard count.
#pragma clang fp contract(off)
#include "vpf_common.h"
#include "../../include/vpf.h"
#include "pf_tree.h"
#include "pf_predict.h"

using namespace vpf;

__global__ __launch_bounds__(256) void k_predict(float* __restrict__ xs, float* __restrict__ ys,
                                                 float* __restrict__ ss, int64_t n, int64_t gbegin,
                                                 uint32_t k0, uint32_t k1, uint32_t frame, float sig_x,
                                                 float sig_y, float sig_s, float width, float height,
                                                 float smin, float smax) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Noise3 z = predict_noise((uint32_t)(gbegin + i), frame, k0, k1);
    xs[i] = clampf(fmaf(sig_x, z.n0, xs[i]), 0.0f, width - 1.0f);
    ys[i] = clampf(fmaf(sig_y, z.n1, ys[i]), 0.0f, height - 1.0f);
    ss[i] = predict_scale(ss[i], sig_s, z.n2, smin, smax);
}

VPF_API int vpf_predict(float* particles, int64_t n, int64_t ld, int64_t global_begin, uint64_t seed,
                        uint32_t frame, float sig_x, float sig_y, float sig_s, float width, float height,
                        float smin, float smax, void* stream) {
    if (!predict_args_ok(n, ld, global_begin)) return VPF_ERR_ARG;
    if (n == 0) return 0;
    const int threads = 256;
    const unsigned blocks = (unsigned)((n + threads - 1) / threads);
    hipLaunchKernelGGL(k_predict, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, particles,
                       particles + ld, particles + 2 * ld, n, global_begin, (uint32_t)seed,
                       (uint32_t)(seed >> 32), frame, sig_x, sig_y, sig_s, width, height, smin, smax);
    VPF_RETURN_LAUNCH();
}

// Constant-velocity predict (SPEC S11) on particles[5][ld] = x | y | s | vx | vy: the velocity takes its own noise
// n3, n4 from Philox counter (gi, frame, 0, 1), decays by d and is clamped to +-vmax; the position then moves by the
// new velocity plus S2's noise. A particle clamped at the frame border keeps its velocity.
struct CvParams { float sig_x, sig_y, sig_s, sig_vx, sig_vy, decay, vmax, width, height, smin, smax; };

__global__ __launch_bounds__(256) void k_predict_cv(float* __restrict__ p, int64_t ld, int64_t n, int64_t gbegin,
                                                    uint32_t k0, uint32_t k1, uint32_t frame, CvParams c) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t gi = (uint32_t)(gbegin + i);
    const Noise3 z = predict_noise(gi, frame, k0, k1);
    const u32x4 q = philox4x32_10(gi, frame, 0u, 1u, k0, k1);
    float n3, n4;
    gauss_pair(q.v[0], q.v[1], n3, n4);
    const float vx = clampf(fmaf(c.sig_vx, n3, c.decay * p[3 * ld + i]), -c.vmax, c.vmax);
    const float vy = clampf(fmaf(c.sig_vy, n4, c.decay * p[4 * ld + i]), -c.vmax, c.vmax);
    p[i] = clampf(fmaf(c.sig_x, z.n0, p[i] + vx), 0.0f, c.width - 1.0f);
    p[ld + i] = clampf(fmaf(c.sig_y, z.n1, p[ld + i] + vy), 0.0f, c.height - 1.0f);
    p[2 * ld + i] = predict_scale(p[2 * ld + i], c.sig_s, z.n2, c.smin, c.smax);
    p[3 * ld + i] = vx;
    p[4 * ld + i] = vy;
}

VPF_API int vpf_predict_cv(float* particles, int64_t n, int64_t ld, int64_t global_begin, uint64_t seed,
                           uint32_t frame, float sig_x, float sig_y, float sig_s, float sig_vx, float sig_vy,
                           float decay, float vmax, float width, float height, float smin, float smax,
                           void* stream) {
    if (!predict_args_ok(n, ld, global_begin)) return VPF_ERR_ARG;
    if (!(decay >= 0.0f && decay <= 1.0f) || !(sig_vx >= 0.0f && sig_vx < INFINITY) ||
        !(sig_vy >= 0.0f && sig_vy < INFINITY) || !(vmax > 0.0f && vmax < INFINITY))
        return VPF_ERR_ARG;
    if (n == 0) return 0;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const CvParams c{sig_x, sig_y, sig_s, sig_vx, sig_vy, decay, vmax, width, height, smin, smax};
    hipLaunchKernelGGL(k_predict_cv, dim3(blocks), dim3(256), 0, (hipStream_t)stream, particles, ld, n, global_begin,
                       (uint32_t)seed, (uint32_t)(seed >> 32), frame, c);
    VPF_RETURN_LAUNCH();
}

// Angle predict (SPEC S12) over the angle row alone, after k_predict or k_predict_cv: the noise n5 is the cosine
// branch of Box-Muller on words 0, 1 of Philox counter (gi, frame, 0, 2); a' = clamp(fmaf(sig_a, n5, a), amin, amax).
// Angles are clamped, not wrapped.
__global__ __launch_bounds__(256) void k_predict_angle(float* __restrict__ as, int64_t n, int64_t gbegin, uint32_t k0,
                                                       uint32_t k1, uint32_t frame, float sig_a, float amin,
                                                       float amax) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32x4 q = philox4x32_10((uint32_t)(gbegin + i), frame, 0u, 2u, k0, k1);
    float n5, unused;
    gauss_pair(q.v[0], q.v[1], n5, unused);
    as[i] = clampf(fmaf(sig_a, n5, as[i]), amin, amax);
}

VPF_API int vpf_predict_angle(float* angles, int64_t n, int64_t global_begin, uint64_t seed, uint32_t frame,
                              float sig_a, float amin, float amax, void* stream) {
    const float pi = 3.14159274101257324f;   // fp32(pi)
    if (!predict_args_ok(n, n, global_begin)) return VPF_ERR_ARG;
    if (!(sig_a >= 0.0f && sig_a < INFINITY) || !(amin >= -pi && amin < amax && amax <= pi)) return VPF_ERR_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_predict_angle, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, angles, n,
                       global_begin, (uint32_t)seed, (uint32_t)(seed >> 32), frame, sig_a, amin, amax);
    VPF_RETURN_LAUNCH();
}

// Inclusive scan of a shard's Q (or of 1s when uniform) into cdf.
__global__ __launch_bounds__(1024) void k_scan(const int64_t* __restrict__ Q, int64_t n, int uniform,
                                               int64_t* __restrict__ cdf) {
    block_scan_cdf(n, cdf, [=](int64_t i) { return uniform ? (int64_t)1 : Q[i]; });
}

__global__ __launch_bounds__(256) void k_resample_search(
    const int64_t* __restrict__ cdf, int64_t n_local, int64_t global_begin, int64_t offset, int64_t total,
    int64_t P, uint32_t U, int64_t slot_begin, int64_t slot_end, const float* __restrict__ xs,
    const float* __restrict__ ys, const float* __restrict__ ss, int32_t* __restrict__ anc,
    float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ os) {
    const int64_t jj = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t j = slot_begin + jj;
    if (j >= slot_end) return;
    const uint64_t pos = sys_position((uint64_t)j, (uint64_t)total, (uint64_t)P, U);
    // local position; the caller guarantees pos in [offset, offset + shard total)
    const int64_t lo = cdf_upper_bound(cdf, n_local, pos - (uint64_t)offset);
    gather_store(jj, global_begin + lo, xs + lo, ys + lo, ss + lo, anc, ox, oy, os);
}

VPF_API int vpf_resample(const int64_t* Q, int64_t n_local, int64_t global_begin, int64_t offset,
                         int64_t total, int64_t P, uint32_t U, int uniform, int64_t slot_begin,
                         int64_t slot_end, const float* particles, int64_t ld, int32_t* anc_out,
                         float* states_out, int64_t out_ld, int64_t* cdf_ws, void* stream) {
    if (n_local < 0 || ld < n_local || P <= 0 || total <= 0 || slot_begin < 0 || slot_end < slot_begin ||
        slot_end > P || out_ld < slot_end - slot_begin || offset < 0)
        return VPF_ERR_ARG;
    const int64_t cnt = slot_end - slot_begin;
    if (cnt == 0) return 0;
    if (n_local == 0) return VPF_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, Q, n_local, uniform, cdf_ws);
    const unsigned blocks = (unsigned)((cnt + 255) / 256);
    hipLaunchKernelGGL(k_resample_search, dim3(blocks), dim3(256), 0, s, cdf_ws, n_local, global_begin,
                       offset, total, P, U, slot_begin, slot_end, particles, particles + ld,
                       particles + 2 * ld, anc_out, states_out, states_out + out_ld,
                       states_out + 2 * out_ld);
    VPF_RETURN_LAUNCH();
}

__global__ __launch_bounds__(1024) void k_stats_scan_global(GlobalView g, int64_t P, int64_t* __restrict__ cdf,
                                                            int64_t* __restrict__ stats_out) {
    stats_scan_global<false>(g, P, 0.0, 0, cdf, stats_out);
}

__global__ __launch_bounds__(1024) void k_stats_scan_global_ex(GlobalView g, int64_t P, double ess_tau,
                                                               int64_t* __restrict__ cdf,
                                                               int64_t* __restrict__ stats_out) {
    stats_scan_global<true>(g, P, ess_tau, 0, cdf, stats_out);
}

__global__ __launch_bounds__(256) void k_resample_global(const int64_t* __restrict__ cdf, int64_t P, uint32_t k0,
                                                         uint32_t k1, uint32_t frame, int64_t slot_begin,
                                                         int64_t slot_end, GlobalView g, int32_t* __restrict__ anc,
                                                         float* __restrict__ ox, float* __restrict__ oy,
                                                         float* __restrict__ os) {
    resample_global<false>(cdf, nullptr, P, k0, k1, frame, slot_begin, slot_end, g, 0, 0, anc, ox, oy, os, nullptr);
}

__global__ __launch_bounds__(256) void k_resample_global_ex(const int64_t* __restrict__ cdf,
                                                            const int64_t* __restrict__ stats, int64_t P,
                                                            uint32_t k0, uint32_t k1, uint32_t frame,
                                                            int64_t slot_begin, int64_t slot_end, GlobalView g,
                                                            int method, int bits, int32_t* __restrict__ anc,
                                                            float* __restrict__ ox, float* __restrict__ oy,
                                                            float* __restrict__ os, int64_t* __restrict__ carry_out) {
    resample_global<true>(cdf, stats, P, k0, k1, frame, slot_begin, slot_end, g, method, bits, anc, ox, oy, os,
                          carry_out);
}

// The statistics + CDF workgroup, then one thread per slot; ex selects the adaptive instances (and only then are
// method, ess_tau, bits and carry_out read).
static int estimate_resample(bool ex, const int64_t* Q, int64_t q_stride, const float* particles, int64_t ld,
                             int64_t p_stride, int64_t n_shard, int64_t P, uint64_t seed, uint32_t frame,
                             int64_t slot_begin, int64_t slot_end, int32_t* anc_out, float* states_out,
                             int64_t out_ld, int64_t* cdf_ws, int64_t* stats_out, int method, double ess_tau,
                             int bits, int64_t* carry_out, void* stream) {
    if (!global_args_ok(q_stride, ld, p_stride, n_shard, P, slot_begin, slot_end, out_ld)) return VPF_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const GlobalView g{Q, q_stride, particles, ld, p_stride, (uint32_t)n_shard};
    if (ex)
        hipLaunchKernelGGL(k_stats_scan_global_ex, dim3(1), dim3(1024), 0, s, g, P, ess_tau, cdf_ws, stats_out);
    else
        hipLaunchKernelGGL(k_stats_scan_global, dim3(1), dim3(1024), 0, s, g, P, cdf_ws, stats_out);
    const int64_t cnt = slot_end - slot_begin;
    const dim3 blocks((unsigned)((cnt + 255) / 256));
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    float *ox = states_out, *oy = states_out + out_ld, *os = states_out + 2 * out_ld;
    if (cnt > 0 && ex)
        hipLaunchKernelGGL(k_resample_global_ex, blocks, dim3(256), 0, s, cdf_ws, stats_out, P, k0, k1, frame,
                           slot_begin, slot_end, g, method, bits, anc_out, ox, oy, os, carry_out);
    else if (cnt > 0)
        hipLaunchKernelGGL(k_resample_global, blocks, dim3(256), 0, s, cdf_ws, P, k0, k1, frame, slot_begin,
                           slot_end, g, anc_out, ox, oy, os);
    VPF_RETURN_LAUNCH();
}

VPF_API int vpf_estimate_resample(const int64_t* Q, int64_t q_stride, const float* particles, int64_t ld,
                                  int64_t p_stride, int64_t n_shard, int64_t P, uint64_t seed, uint32_t frame,
                                  int64_t slot_begin, int64_t slot_end, int32_t* anc_out, float* states_out,
                                  int64_t out_ld, int64_t* cdf_ws, int64_t* stats_out, void* stream) {
    return estimate_resample(false, Q, q_stride, particles, ld, p_stride, n_shard, P, seed, frame, slot_begin,
                             slot_end, anc_out, states_out, out_ld, cdf_ws, stats_out, 0, 0.0, 0, nullptr, stream);
}

VPF_API int vpf_estimate_resample_ex(const int64_t* Q, int64_t q_stride, const float* particles, int64_t ld,
                                     int64_t p_stride, int64_t n_shard, int64_t P, uint64_t seed, uint32_t frame,
                                     int64_t slot_begin, int64_t slot_end, int32_t* anc_out, float* states_out,
                                     int64_t out_ld, int64_t* cdf_ws, int64_t* stats_out, int method, double ess_tau,
                                     int bits, int64_t* carry_out, void* stream) {
    if ((method != VPF_RESAMPLE_SYSTEMATIC && method != VPF_RESAMPLE_STRATIFIED) || bits < 0 || bits > 61 ||
        !(ess_tau < 0.0 || (ess_tau > 0.0 && ess_tau <= 1.0)))
        return VPF_ERR_ARG;
    return estimate_resample(true, Q, q_stride, particles, ld, p_stride, n_shard, P, seed, frame, slot_begin,
                             slot_end, anc_out, states_out, out_ld, cdf_ws, stats_out, method, ess_tau, bits,
                             carry_out, stream);
}

// ---------------- weighted sums of rows over a view (SPEC S6; S11's velocity rows) ----------------
// One workgroup, one kernel for both entry points: weighted_sums over n_rows <= 3 rows starting at g.p (0 for the rows
// not given). vpf_shard_stats: one shard's flat arrays, no uniform pass (the caller combines the shards' sums).
// vpf_weighted_sums: further rows of the global view with the uniform pass, so over x | y | s it writes
// k_stats_scan_global's stats_out[0..3].
__global__ __launch_bounds__(1024) void k_shard_stats(GlobalView g, int64_t n, int n_rows, bool uniform,
                                                      int64_t* __restrict__ out_T, int64_t* __restrict__ out_sums) {
    weighted_sums<false, false>(g, n, [=](uint32_t i) {
        const float* r = g.state(i);
        return Wxys{0, r[0], n_rows > 1 ? r[g.ld] : 0.0f, n_rows > 2 ? r[2 * g.ld] : 0.0f};
    }, uniform, 0, out_T, out_sums);
}

VPF_API int vpf_shard_stats(const int64_t* Q, const float* particles, int64_t ld, int64_t n,
                            int64_t* out_T, double* out_sums, void* stream) {
    if (n < 0 || n > 0x7fffffffLL || ld < n) return VPF_ERR_ARG;
    const GlobalView g{Q, n, particles, ld, 3 * ld, (uint32_t)(n > 0 ? n : 1)};
    hipLaunchKernelGGL(k_shard_stats, dim3(1), dim3(1024), 0, (hipStream_t)stream, g, n, 3, false, out_T,
                       (int64_t*)out_sums);
    VPF_RETURN_LAUNCH();
}

VPF_API int vpf_weighted_sums(const int64_t* Q, int64_t q_stride, const float* rows, int64_t ld, int64_t p_stride,
                              int64_t n_shard, int64_t P, int n_rows, int64_t* out, void* stream) {
    if (!rows_args_ok(ld, p_stride, n_shard, P, n_rows, 3) || (P > n_shard && q_stride < n_shard))
        return VPF_ERR_ARG;
    const GlobalView g{Q, q_stride, rows, ld, p_stride, (uint32_t)n_shard};
    hipLaunchKernelGGL(k_shard_stats, dim3(1), dim3(1024), 0, (hipStream_t)stream, g, P, n_rows, true, out, out + 1);
    VPF_RETURN_LAUNCH();
}

// One thread per slot j < n_slots: the n_rows values of its ancestor a = anc[j] (a global index). An ancestor outside
// [0, P) writes nothing.
__global__ __launch_bounds__(256) void k_gather_rows(const int32_t* __restrict__ anc, int64_t n_slots, GlobalView g,
                                                     int64_t P, int n_rows, float* __restrict__ out,
                                                     int64_t out_ld) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_slots) return;
    const int64_t a = anc[j];
    if (a < 0 || a >= P) return;
    const float* r = g.state((uint32_t)a);
    for (int c = 0; c < n_rows; ++c) out[c * out_ld + j] = r[c * g.ld];
}

VPF_API int vpf_gather_rows(const int32_t* anc, int64_t n_slots, const float* rows, int64_t ld, int64_t p_stride,
                            int64_t n_shard, int64_t P, int n_rows, float* out, int64_t out_ld, void* stream) {
    if (!rows_args_ok(ld, p_stride, n_shard, P, n_rows, 8) || n_slots < 0 || out_ld < n_slots) return VPF_ERR_ARG;
    if (n_slots == 0) return 0;
    const GlobalView g{nullptr, 0, rows, ld, p_stride, (uint32_t)n_shard};
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       anc, n_slots, g, P, n_rows, out, out_ld);
    VPF_RETURN_LAUNCH();
}

// ---------------- the weight carry of adaptive resampling (SPEC S10 rule 1) ----------------
// Q_i <- (Q_i * C_i) >> sh, sh = K + 1 in [1, 62], from the exact 128-bit product (hi, lo).
__global__ __launch_bounds__(256) void k_weight_prior(int64_t* __restrict__ Q, const int64_t* __restrict__ carry,
                                                      int64_t n, int sh) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t l = (uint64_t)Q[i], c = (uint64_t)carry[i];
    const uint64_t hi = __umul64hi(l, c), lo = l * c;
    Q[i] = (int64_t)((hi << (64 - sh)) | (lo >> sh));
}

VPF_API int vpf_weight_prior(int64_t* Q, const int64_t* carry, int64_t n, int bits, void* stream) {
    if (n < 0 || bits < 0 || bits > 61) return VPF_ERR_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_weight_prior, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Q,
                       carry, n, bits + 1);
    VPF_RETURN_LAUNCH();
}

VPF_API const char* vpf_version(void) { return "libvpf 0.1.0 gfx950"; }
