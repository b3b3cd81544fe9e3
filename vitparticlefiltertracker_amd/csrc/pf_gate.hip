// Occlusion gate (SPEC S15): the third instance of the estimate + resample pair, beside pf_kernels.hip's default and
// adaptive (_ex) ones, built from the same bodies in pf_tree.h, and vpf_weighted_sums' gated twin.
//
// k_stats_scan_global_gate is stats_scan_global<EX, GATE>: the one workgroup reduces T, the three sums, S2 and
// m = max Q_i as the adaptive instance does, then decides once, in integers, held iff m < gate_q. Every thread reads m
// from LDS after the tree's last barrier, so all 1024 take the same branch around the barriers that follow: a held
// frame takes weighted_sums' second pass (every weight 1: the uniform sums) and skips the CDF scan; nothing reads it.
// k_resample_global_gate is resample_global<EX, GATE>: a held frame (stats[7]) is the skip branch with the identity
// carry, a_j = j, no Philox draw; any other frame is the adaptive instance with the ESS gate off, bit for bit.
// k_shard_stats_gate recomputes the same decision from the same tree over the same weights for the extra state rows.
#pragma clang fp contract(off)
#include "vpf_common.h"
#include "../../include/vpf.h"
#include "pf_tree.h"

using namespace vpf;

__global__ __launch_bounds__(1024) void k_stats_scan_global_gate(GlobalView g, int64_t P, int64_t gate_q,
                                                                 int64_t* __restrict__ cdf,
                                                                 int64_t* __restrict__ stats_out) {
    stats_scan_global<true, true>(g, P, -1.0, gate_q, cdf, stats_out);
}

__global__ __launch_bounds__(256) void k_resample_global_gate(const int64_t* __restrict__ cdf,
                                                              const int64_t* __restrict__ stats, int64_t P,
                                                              uint32_t k0, uint32_t k1, uint32_t frame,
                                                              int64_t slot_begin, int64_t slot_end, GlobalView g,
                                                              int method, int bits, int32_t* __restrict__ anc,
                                                              float* __restrict__ ox, float* __restrict__ oy,
                                                              float* __restrict__ os, int64_t* __restrict__ carry_out) {
    resample_global<true, true>(cdf, stats, P, k0, k1, frame, slot_begin, slot_end, g, method, bits, anc, ox, oy, os,
                                carry_out);
}

VPF_API int vpf_estimate_resample_gate(const int64_t* Q, int64_t q_stride, const float* particles, int64_t ld,
                                       int64_t p_stride, int64_t n_shard, int64_t P, uint64_t seed, uint32_t frame,
                                       int64_t slot_begin, int64_t slot_end, int32_t* anc_out, float* states_out,
                                       int64_t out_ld, int64_t* cdf_ws, int64_t* stats_out, int method, int bits,
                                       int64_t gate_q, int64_t* carry_out, void* stream) {
    if ((method != VPF_RESAMPLE_SYSTEMATIC && method != VPF_RESAMPLE_STRATIFIED) || bits < 0 || bits > 61 ||
        gate_q < 0 || gate_q > ((int64_t)1 << bits))
        return VPF_ERR_ARG;
    if (!global_args_ok(q_stride, ld, p_stride, n_shard, P, slot_begin, slot_end, out_ld)) return VPF_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const GlobalView g{Q, q_stride, particles, ld, p_stride, (uint32_t)n_shard};
    hipLaunchKernelGGL(k_stats_scan_global_gate, dim3(1), dim3(1024), 0, s, g, P, gate_q, cdf_ws, stats_out);
    const int64_t cnt = slot_end - slot_begin;
    if (cnt > 0)
        hipLaunchKernelGGL(k_resample_global_gate, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, cdf_ws,
                           stats_out, P, (uint32_t)seed, (uint32_t)(seed >> 32), frame, slot_begin, slot_end, g, method,
                           bits, anc_out, states_out, states_out + out_ld, states_out + 2 * out_ld, carry_out);
    VPF_RETURN_LAUNCH();
}

__global__ __launch_bounds__(1024) void k_shard_stats_gate(GlobalView g, int64_t n, int n_rows, int64_t gate_q,
                                                           int64_t* __restrict__ out_T,
                                                           int64_t* __restrict__ out_sums) {
    weighted_sums<true, true>(g, n, [=](uint32_t i) {
        const float* r = g.state(i);
        return Wxys{0, r[0], n_rows > 1 ? r[g.ld] : 0.0f, n_rows > 2 ? r[2 * g.ld] : 0.0f};
    }, true, gate_q, out_T, out_sums);
}

VPF_API int vpf_weighted_sums_gate(const int64_t* Q, int64_t q_stride, const float* rows, int64_t ld,
                                   int64_t p_stride, int64_t n_shard, int64_t P, int n_rows, int64_t gate_q,
                                   int64_t* out, void* stream) {
    if (!rows_args_ok(ld, p_stride, n_shard, P, n_rows, 3) || (P > n_shard && q_stride < n_shard) || gate_q < 0 ||
        gate_q > ((int64_t)1 << 61))
        return VPF_ERR_ARG;
    const GlobalView g{Q, q_stride, rows, ld, p_stride, (uint32_t)n_shard};
    hipLaunchKernelGGL(k_shard_stats_gate, dim3(1), dim3(1024), 0, (hipStream_t)stream, g, P, n_rows, gate_q, out,
                       out + 1);
    VPF_RETURN_LAUNCH();
}
