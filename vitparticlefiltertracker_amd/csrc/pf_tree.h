// The particle-filter kernels' shared device pieces (SPEC S6, S7, S10, S15), each defined once: the stats tree, the CDF
// scan, the slot search and gather, the global view, and the two bodies of the estimate + resample pair
// (stats_scan_global, resample_global) with their instances' switches. pf_kernels.hip instantiates the default and the
// adaptive (_ex) kernels, pf_gate.hip the occlusion-gated ones; a kernel is charged only for the LDS its instance
// touches. Everything here is compiled with fp contraction off, as the files that include it are.
#pragma once
#pragma clang fp contract(off)
#include "vpf_common.h"
#include "../../include/vpf.h"

using namespace vpf;

// ---------------- the stats tree (SPEC S6; S10's sum of squares and maximum) ----------------
// The tree's LDS, one slot per thread. A kernel is charged only for the arrays its instance touches: s2h, s2l and smx
// belong to the SQ instance alone.
__shared__ int64_t sT[1024];
__shared__ double sx[1024], sy[1024], sz[1024];
__shared__ uint64_t s2h[1024], s2l[1024];
__shared__ int64_t smx[1024];

struct Wxys { int64_t q; float x, y, s; };   // particle i's weight and state, as stats_tree's callable returns it

// One 1024-thread workgroup: sT[0] = sum q_i (exact), sx/sy/sz[0] = sum q_i * (x_i, y_i, s_i) in fp64 over at(i),
// i < n: thread t takes i = t, t + 1024, ... in order, then a 512 -> 1 pairwise halving. An SQ instance reduces, when
// sq, also S2 = sum q_i^2 as an exact unsigned 128-bit integer (an LDS (hi, lo) pair per thread; a lo overflow carries
// into hi) and smx[0] = max q_i; without sq it leaves them as they are.
template <bool SQ, class At>
__device__ __forceinline__ void stats_tree(int64_t n, bool sq, At at) {
    const int t = threadIdx.x;
    int64_t T = 0, m = 0;
    uint64_t h2 = 0, l2 = 0;
    double ax = 0, ay = 0, az = 0;
    for (int64_t i = t; i < n; i += 1024) {
        const Wxys w = at(i);
        const double qd = (double)w.q;
        T += w.q;
        ax += qd * (double)w.x; ay += qd * (double)w.y; az += qd * (double)w.s;
        if constexpr (SQ) if (sq) {
            const uint64_t uq = (uint64_t)w.q, lo = uq * uq;
            l2 += lo;
            h2 += __umul64hi(uq, uq) + (uint64_t)(l2 < lo);
            m = w.q > m ? w.q : m;
        }
    }
    sT[t] = T; sx[t] = ax; sy[t] = ay; sz[t] = az;
    if constexpr (SQ) if (sq) { s2h[t] = h2; s2l[t] = l2; smx[t] = m; }
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) {
            sT[t] += sT[t + o]; sx[t] += sx[t + o]; sy[t] += sy[t + o]; sz[t] += sz[t + o];
            if constexpr (SQ) if (sq) {
                const uint64_t a = s2l[t], s = a + s2l[t + o];
                s2l[t] = s;
                s2h[t] += s2h[t + o] + (uint64_t)(s < a);
                const int64_t mo = smx[t + o];
                if (mo > smx[t]) smx[t] = mo;
            }
        }
        __syncthreads();
    }
}

// ---------------- the CDF scan and the slot search (SPEC S7) ----------------
__device__ __forceinline__ int64_t wave_incl_scan(int64_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// cdf[i] = weight(0) + ... + weight(i), i < n. One workgroup, 1024 threads, 4 per thread.
template <class W>
__device__ __forceinline__ void block_scan_cdf(int64_t n, int64_t* __restrict__ cdf, W weight) {
    __shared__ int64_t wsum[16];
    __shared__ int64_t carry_s;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 4096) {
        int64_t v[4];
        int64_t loc = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = base + (int64_t)t * 4 + e;
            loc += (i < n) ? weight(i) : (int64_t)0;
            v[e] = loc;
        }
        const int64_t incl = wave_incl_scan(loc, lane);
        if (lane == 63) wsum[wid] = incl;
        __syncthreads();
        int64_t wprefix = 0;
        for (int w = 0; w < wid; ++w) wprefix += wsum[w];
        const int64_t excl = carry_s + wprefix + (incl - loc);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = base + (int64_t)t * 4 + e;
            if (i < n) cdf[i] = excl + v[e];
        }
        __syncthreads();
        if (t == 1023) {
            int64_t tot = 0;
            for (int w = 0; w < 16; ++w) tot += wsum[w];
            carry_s += tot;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ uint64_t sys_position(uint64_t j, uint64_t T, uint64_t P, uint32_t U) {
    const uint64_t u = (uint64_t)U * (T >> 32) + (((uint64_t)U * (T & 0xffffffffull)) >> 32);
    const uint64_t qT = T / P, rT = T % P, qu = u / P, ru = u % P;
    return j * qT + qu + (j * rT + ru) / P;
}

// min{i : cdf[i] > pos}; the caller guarantees pos < cdf[n - 1].
__device__ __forceinline__ int64_t cdf_upper_bound(const int64_t* __restrict__ cdf, int64_t n, uint64_t pos) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((uint64_t)cdf[mid] > pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Output slot jj takes ancestor a (a global index) and the state at (x, y, s).
__device__ __forceinline__ void gather_store(int64_t jj, int64_t a, const float* x, const float* y, const float* s,
                                             int32_t* __restrict__ anc, float* __restrict__ ox,
                                             float* __restrict__ oy, float* __restrict__ os) {
    anc[jj] = (int32_t)a;
    ox[jj] = *x; oy[jj] = *y; os[jj] = *s;
}

// ---------------- estimate + resample over the global particle set (SPEC S6 + S7 + S10, device-resident) --------
// The product path (ParticleFilter): every rank holds the GLOBAL weights and states — its own arrays (world 1) or
// the all-gathered shard chunks (world > 1, one fixed-size all-gather of 20 B per particle) — so the totals, the
// CDF, the resample word and the ancestors of its own output slots are computed on the device with no host
// round trip in between, and every rank (and every world size) sums in the same fixed order over the global
// index: the estimate is bit-identical for any G. Global index i lives in shard r = i / n_shard at k = i % n_shard.
struct GlobalView {
    const int64_t* Q;
    int64_t q_stride;      // int64 elements from shard r's Q to shard r + 1's
    const float* p;        // shard 0's x row; y at + ld, s at + 2 ld
    int64_t ld;
    int64_t p_stride;      // floats from shard r's x row to shard r + 1's
    uint32_t n_shard;
    __device__ __forceinline__ int64_t off(uint32_t i, int64_t stride) const {
        const uint32_t r = i / n_shard;
        return (int64_t)r * stride + (int64_t)(i - r * n_shard);
    }
    __device__ __forceinline__ int64_t q(uint32_t i) const { return Q[off(i, q_stride)]; }
    __device__ __forceinline__ const float* state(uint32_t i) const { return p + off(i, p_stride); }
};

// One workgroup: SPEC S6's sums by stats_tree over the weights g.q(i) and the values xyz(i) (a Wxys whose q is
// ignored), i < P; with `uniform`, repeated with every Q_i = 1 when T == 0 (the uniform fallback's plain sums). Writes
// out_T[0] = T and out_sums[0..2] = the bits of the three fp64 sums, and returns T. An EX instance's first pass also
// leaves S2 and max Q_i in the tree. A GATE instance (SPEC S15, an EX one) takes the occlusion decision from that
// maximum, held iff max Q_i < gate_q: every thread reads smx[0] from LDS after the tree's last barrier, so the whole
// workgroup takes the same branch, and a held frame takes the second pass whatever T is (its sums are the uniform
// ones while out_T[0] keeps the true T; the second pass leaves S2 and the maximum as they are).
struct SumsT { int64_t T; bool held; };

template <bool EX, bool GATE, class V>
__device__ __forceinline__ SumsT weighted_sums(const GlobalView& g, int64_t P, V xyz, bool uniform, int64_t gate_q,
                                               int64_t* __restrict__ out_T, int64_t* __restrict__ out_sums) {
    static_assert(EX || !GATE, "the gate reads the SQ instance's maximum");
    const int t = threadIdx.x;
    int64_t T0 = 0;
    bool held = false;
    for (int pass = 0; pass < 2; ++pass) {
        stats_tree<EX>(P, pass == 0, [=](int64_t i) {
            Wxys w = xyz((uint32_t)i);
            w.q = pass == 0 ? g.q((uint32_t)i) : (int64_t)1;
            return w;
        });
        const int64_t Tall = sT[0];
        if (pass == 0) {
            T0 = Tall;
            if (t == 0) out_T[0] = Tall;
            if constexpr (GATE) held = smx[0] < gate_q;
        }
        bool done = pass == 1 || Tall != 0 || !uniform;
        if constexpr (GATE) done = pass == 1 || (done && !held);
        if (done) {
            if (t == 0) {
                out_sums[0] = __double_as_longlong(sx[0]);
                out_sums[1] = __double_as_longlong(sy[0]);
                out_sums[2] = __double_as_longlong(sz[0]);
            }
            break;
        }
        __syncthreads();   // every thread has read sT[0] before pass 1 rewrites the tree
    }
    return SumsT{T0, held};
}

// One workgroup: weighted_sums over the states x | y | s; then the inclusive int64 CDF. The EX instance (SPEC S10)
// also takes S2 and m = max Q_i from the first pass and the decision, once: ess = T^2 / S2 in fp64, resample iff
// T == 0, the gate is disabled (ess_tau < 0) or ess < ess_tau * P; its stats_out continues
// {..., bits of ess, resampled, m, 0}. The GATE instance (SPEC S15) ends it with held instead of 0; a held frame is
// not resampled (0) and skips the scan, which nothing reads: the whole workgroup returns together.
template <bool EX, bool GATE = false>
__device__ __forceinline__ void stats_scan_global(const GlobalView& g, int64_t P, double ess_tau, int64_t gate_q,
                                                  int64_t* __restrict__ cdf, int64_t* __restrict__ stats_out) {
    const int t = threadIdx.x;
    const SumsT r = weighted_sums<EX, GATE>(g, P, [=](uint32_t i) {
        const float* st = g.state(i);
        return Wxys{0, st[0], st[g.ld], st[2 * g.ld]};
    }, true, gate_q, stats_out, stats_out + 1);
    const int64_t T0 = r.T;
    if constexpr (EX) if (t == 0) {
        double ess = 0.0;
        if (T0 != 0) {
            const double Td = (double)T0;
            const double S2d = (double)s2h[0] * 18446744073709551616.0 + (double)s2l[0];
            ess = (Td * Td) / S2d;
        }
        const bool resampled = T0 == 0 || ess_tau < 0.0 || ess < ess_tau * (double)P;
        stats_out[4] = __double_as_longlong(ess);
        stats_out[5] = resampled && !r.held ? 1 : 0;
        stats_out[6] = smx[0];
        stats_out[7] = r.held ? 1 : 0;
    }
    if (r.held) return;
    block_scan_cdf(P, cdf, [=](int64_t i) { return g.q((uint32_t)i); });
}

// One thread per output slot j in [slot_begin, slot_end): T = cdf[P-1] (0 -> uniform: C_i = i + 1, so a_j =
// pos_j), U = Philox(ctr = (0, frame, 1, 0), key = seed) word 0 (SPEC S1), pos_j exact (SPEC S7), a_j =
// min{i : C_i > pos_j} by binary search over the global CDF, and the ancestor's state. The EX instance reads the
// decision stats_scan_global<true> left in stats. Resample: the same with the method's position (stratified: the
// slot's own word, Philox ctr = (j, frame, 1, 1)) and the identity carry 2^(K+1). Skip: a_j = j, the state
// unchanged, C_j = Q_j << (K + 1 - bitlen(m)). The default instance reads no stats and writes no carry. The GATE
// instance's held frame (SPEC S15, stats[7]) is the skip with the identity carry; it reads neither Q nor the CDF.
template <bool EX, bool GATE = false>
__device__ __forceinline__ void resample_global(const int64_t* __restrict__ cdf, const int64_t* __restrict__ stats,
                                                int64_t P, uint32_t k0, uint32_t k1, uint32_t frame,
                                                int64_t slot_begin, int64_t slot_end, const GlobalView& g, int method,
                                                int bits, int32_t* __restrict__ anc, float* __restrict__ ox,
                                                float* __restrict__ oy, float* __restrict__ os,
                                                int64_t* __restrict__ carry_out) {
    const int64_t jj = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t j = slot_begin + jj;
    if (j >= slot_end) return;
    int64_t lo, carry;
    if (GATE && stats[7] != 0) {
        lo = j;
        carry = (int64_t)1 << (bits + 1);
    } else if (EX && stats[5] == 0) {
        const int sh = bits + 1 - (64 - __clzll((long long)stats[6]));   // m > 0: T != 0 on this branch
        const int64_t q = g.q((uint32_t)j);
        lo = j;
        carry = sh >= 0 ? q << sh : q >> -sh;
    } else {
        const int64_t T = cdf[P - 1];
        const uint32_t U = EX && method == VPF_RESAMPLE_STRATIFIED
                               ? philox4x32_10((uint32_t)j, frame, 1u, 1u, k0, k1).v[0]
                               : philox4x32_10(0u, frame, 1u, 0u, k0, k1).v[0];
        const uint64_t pos = sys_position((uint64_t)j, (uint64_t)(T == 0 ? P : T), (uint64_t)P, U);
        lo = T == 0 ? (int64_t)pos : cdf_upper_bound(cdf, P, pos);
        carry = (int64_t)1 << (bits + 1);
    }
    const float* st = g.state((uint32_t)lo);
    gather_store(jj, lo, st, st + g.ld, st + 2 * g.ld, anc, ox, oy, os);
    if constexpr (EX) carry_out[jj] = carry;
}

// The shape contract of the global layout (include/vpf.h), shared by both entry points.
static bool global_args_ok(int64_t q_stride, int64_t ld, int64_t p_stride, int64_t n_shard, int64_t P,
                           int64_t slot_begin, int64_t slot_end, int64_t out_ld) {
    if (P <= 0 || P > 0x7fffffffLL || n_shard <= 0 || P % n_shard != 0 || ld < n_shard || slot_begin < 0 ||
        slot_end < slot_begin || slot_end > P || out_ld < slot_end - slot_begin)
        return false;
    return !(P > n_shard && (q_stride < n_shard || p_stride < 2 * ld + n_shard));
}

// The global layout's shape contract for n_rows rows of ld floats per shard.
static bool rows_args_ok(int64_t ld, int64_t p_stride, int64_t n_shard, int64_t P, int n_rows, int max_rows) {
    if (P <= 0 || P > 0x7fffffffLL || n_shard <= 0 || P % n_shard != 0 || ld < n_shard || n_rows < 1 ||
        n_rows > max_rows)
        return false;
    return !(P > n_shard && p_stride < (int64_t)(n_rows - 1) * ld + n_shard);
}
