"""N <= 256 bf16 attention with three units in flight per CU (k_attn_pipe4, round 6): one 4-wave workgroup per
(particle, head), each wave two query strips in turn (strips w and w + 4), the head's K / V image in LDS cut at the
16-row tail tile when N % 32 is 1..16 (N = 197: 208 rows, 52 KiB: three workgroups per CU, three waves per SIMD).
The first strip runs the product's chunk loop (counted waits + barriers as the chunks land), the second one over the
landed image without barriers. Layout [V image][K image]: the steps' reads past the tail tile (V rows 16..31 of the
last chunk land in the K image: finite, times probability 0; K rows past the image: out of the workgroup's LDS range,
scores masked to -inf) need no padding. The MX8-output path keeps k_attn_bf16_pipe. The N sweep
(r6_lab/attn_nsweep.txt) says a unit's fixed cost dominates at two resident units per CU; this puts three in flight
with the 32-query steps (round 6's 16-query-strip form of three units, attn_q16, lost on the 16x16x32 steps)."""
_K = r'''
// ---- lab: k_attn_pipe4 (tools/variants/attn_p4.py) ----
template <int CPB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_attn_pipe4(
    const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int N, int H, float scale_log2, int q_rows, int NR) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int NP = (N + 31) & ~31;
    const int NT = NP >> 5;
    char* Vs = smem;
    char* Ks = smem + NR * ROWB;
    const int bh = blockIdx.x;
    const int b = bh / H, h = bh - (bh / H) * H;
    const int D = H * HD;
    const int64_t row0 = (int64_t)b * N;
    const bf16_t* qbase = qkv + row0 * 3 * D + h * HD;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, hh = lane >> 5;
    const int nstrips = (q_rows + 31) >> 5;
    const int nlast = (N - 1) >> 5;
    const int sA = wid, sB = wid + 4;
    const bool w16A = sA == nlast && sA < nstrips && N - 32 * nlast <= 16;
    const bool w16B = sB == nlast && sB < nstrips && N - 32 * nlast <= 16;
    bf16x8 qa[4], qb[4];
    load_q(qa, qbase, D, N, w16A, sA * 32, lane);
    load_q(qb, qbase, D, N, w16B, sB * 32, lane);
    {
        const int sub = lane >> 3, slot = lane & 7;
        for (int c = 0; c < NT; ++c) {
            int g = c * 4 + wid;                       // 8-row piece index inside the image
            if (8 * g >= NR) g -= 2;                   // past the tail tile: re-stage the tile's own rows (same bytes)
            const int r = 8 * g + sub;
            const bf16_t* src = qbase + (int64_t)min(r, N - 1) * 3 * D;
            __builtin_amdgcn_global_load_lds((gptr_t)(src + D + K_SWZ(r, slot) * 8), (lptr_t)(Ks + g * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(src + 2 * D + V_SWZ(r, slot) * 8), (lptr_t)(Vs + g * 1024), 16, 0, 0);
        }
    }
    wait_vmcnt(2 * NT);
    asm volatile("" : "+v"(qa[0]), "+v"(qa[1]), "+v"(qa[2]), "+v"(qa[3]), "+v"(qb[0]), "+v"(qb[1]), "+v"(qb[2]),
                 "+v"(qb[3]) :: "memory");
    const int nfull = N >> 5;
    auto run_strip = [&](auto k16, auto bar_c, bf16x8 (&qf)[4], int sid, bool active) {
        constexpr bool W16 = decltype(k16)::value;
        constexpr bool BAR = decltype(bar_c)::value;
        f32x16 o0 = {}, o1 = {};
        f32x4 o16[4] = {};
        float m = -INFINITY, l = 0.f;
        int c = 0;
        for (; c < nfull; ++c) {
            if constexpr (BAR) {
                if (c % CPB == 0) {
                    wait_vmcnt(2 * max(NT - c - CPB, 0));
                    __builtin_amdgcn_s_barrier();
                    pin_q<W16 ? 2 : 4>(qf);
                }
            }
            if (active) {
                if constexpr (W16) attn_step16<false>(Ks + c * 4096, Vs + c * 4096, c * 32, N, lane, qf, scale_log2, m, l, o16);
                else attn_step_pl<false, 16>(Ks + c * 4096, Vs + c * 4096, c * 32, N, lane, qf, scale_log2, m, l, o0, o1);
            }
        }
        if (c < NT) {
            if constexpr (BAR) {
                if (c % CPB == 0) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    pin_q<W16 ? 2 : 4>(qf);
                }
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
            if (q < q_rows) store_strip32(out + (row0 + q) * D + h * HD, hh, ov);
        }
    };
    if (w16A) run_strip(std::true_type{}, std::true_type{}, qa, sA, true);
    else run_strip(std::false_type{}, std::true_type{}, qa, sA, sA < nstrips);
    if (sB < nstrips) {
        asm volatile("" : "+v"(qb[0]), "+v"(qb[1]), "+v"(qb[2]), "+v"(qb[3]) :: "memory");
        if (w16B) run_strip(std::true_type{}, std::false_type{}, qb, sB, true);
        else run_strip(std::false_type{}, std::false_type{}, qb, sB, true);
    }
}

'''
_f = "attention.hip"
EDITS = [
    (_f, "// ---------------- N > 256 (ViT-L/14 @ 336: N = 577): K / V streamed through a ring, queries in blocks",
     _K + "// ---------------- N > 256 (ViT-L/14 @ 336: N = 577): K / V streamed through a ring, queries in blocks"),
    (_f, """    if (N <= 256) return launch_pipe<false>(""",
     """    if (N <= 256) {
        const int NP = (N + 31) & ~31;
        const int t32 = N & 31;
        const int NR = (t32 >= 1 && t32 <= 16) ? NP - 16 : NP;
        static bool p4_attr = false;
        if (!p4_attr) {
            (void)hipFuncSetAttribute((const void*)k_attn_pipe4<PIPE_CPB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      160 * 1024);
            p4_attr = true;
        }
        hipLaunchKernelGGL((k_attn_pipe4<PIPE_CPB>), dim3((unsigned)(B * H)), dim3(256), (size_t)NR * ROWB * 2,
                           (hipStream_t)stream, qkv, reinterpret_cast<bf16_t*>(out), N, H, scale_log2, q_rows, NR);
        VPF_RETURN_LAUNCH();
    }
    if (N <= 256) return launch_pipe<false>("""),
]
