"""N <= 256 attention with 16-query strips at three workgroups per CU (k_attn_q16, bf16 output; the MX8-output path keeps
k_attn_bf16_pipe): one 512-thread workgroup per (particle, head) as the product, but every strip is a 16-query strip
on v_mfma_f32_16x16x32_bf16 (attn_step16, the product's tail-strip step), each wave takes strips ls and ls + 8 (ls its
wave slot, rotated by (blockIdx >> 3) & 3 so co-resident workgroups put their two-strip waves on different SIMDs),
and the head's K / V image ends at the 16-row tail tile (N = 197: 208 rows, 52 KiB, three per CU) with a tail step that
reads only those 16 rows. The VGPR budget is set for six waves per SIMD (three workgroups). Round 6: the N sweep says
a unit's fixed cost dominates at two resident units per CU (r6_lab/attn_nsweep.txt); this puts three in flight."""
_STEP16_END = '''// ---------------- round 5: the row sum on the matrix cores, and a speculative running max ----------------'''
_TAIL = r'''// attn_step16 on the last key tile when it holds at most 16 real keys: only the tile's first 16 rows are read (the K / V
// image of k_attn_q16 ends there); the second 16-key half's probabilities are 0 and its V^T rows are taken as 0.
__device__ __forceinline__ void attn_step16_t(const char* Kt, const char* Vt, int kb, int N, int lane, const bf16x8 qf[2],
                                              float scale_log2, float& m, float& l, f32x4 (&o)[4]) {
    lane = lane_id_asm();
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Kt + k_off(r16, 4 * kk + g));
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], s, 0, 0, 0);
    }
    float bm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (kb + 4 * g + r >= N) s[r] = -INFINITY;
        bm = fmaxf(bm, s[r]);
    }
    lazy_rescale(xor32_max(xor16_max(bm)), scale_log2, m, [&](float alpha) {
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
    });
    const float msc = m * scale_log2;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(s[r], scale_log2, -msc));
        s[r] = p;
        l += p;
    }
    const bf16x8 pf = pack_bf8(s[0], s[1], s[2], s[3], 0.f, 0.f, 0.f, 0.f);
    const int q = r16 >> 2, p4 = r16 & 3;
    bf16x4 vr[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const int c16 = 2 * dt + (p4 >> 1), inner = 8 * (p4 & 1);
        vr[dt] = ds_read_tr_asm_o<0>((uint32_t)(size_t)Vt + (uint32_t)(v_off(4 * g + q, c16) + inner));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vr[0]), "+v"(vr[1]), "+v"(vr[2]), "+v"(vr[3])::"memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const bf16x4 lo = vr[dt];
        const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
    }
}

'''
_KERNEL_ANCHOR = '''// ---------------- N > 256 (ViT-L/14 @ 336: N = 577): K / V streamed through a ring, queries in blocks ----------------'''
_KERNEL = r'''// ---------------- N <= 256 with a <= 16-key tail tile: 16-query strips, three workgroups per CU (round 6 lab) ----------------
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(6))) void k_attn_q16(
    const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int N, int H, float scale_log2, int q_rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int CPB = PIPE_CPB;
    const int nfull = N >> 5;
    const int NT = nfull + 1;                      // the last chunk holds 1..16 keys (host-checked)
    const int NP = nfull * 32 + 16;
    char* Ks = smem;
    char* Vs = smem + NP * ROWB;
    const int bh = blockIdx.x;
    const int b = bh / H, h = bh - (bh / H) * H;
    const int D = H * HD;
    const int64_t row0 = (int64_t)b * N;
    const bf16_t* qbase = qkv + row0 * 3 * D + h * HD;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S16 = (q_rows + 15) >> 4;
    const int ls = (wid - ((bh >> 3) & 3)) & 7;
    const int sA = ls, sB = ls + 8;
    const bool hasA = sA < S16, hasB = sB < S16;
    bf16x8 qa[2], qb[2];
    {
        const bf16_t* pa = qbase + (int64_t)min(sA * 16 + (lane & 15), N - 1) * 3 * D + 8 * (lane >> 4);
        const bf16_t* pb = qbase + (int64_t)min(sB * 16 + (lane & 15), N - 1) * 3 * D + 8 * (lane >> 4);
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(qa[0]) : "v"(pa));
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(qa[1]) : "v"(pa + 32));
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(qb[0]) : "v"(pb));
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(qb[1]) : "v"(pb + 32));
    }
    {
        const bool isv = wid >= 4;
        const int sub = lane >> 3, slot = lane & 7;
        const bf16_t* src0 = qbase + (isv ? 2 * D : D);
        char* img = isv ? Vs : Ks;
        for (int c = 0; c < NT; ++c) {
            const int j = c == nfull ? (wid & 1) : (wid & 3);   // the tail chunk has 2 pieces: waves 2, 3 repeat 0, 1
            const int g = c * 4 + j;
            const int r = 8 * g + sub;
            const int ch = isv ? V_SWZ(r, slot) : K_SWZ(r, slot);
            __builtin_amdgcn_global_load_lds((gptr_t)(src0 + (int64_t)min(r, N - 1) * 3 * D + ch * 8),
                                             (lptr_t)(img + g * 1024), 16, 0, 0);
        }
    }
    wait_vmcnt(NT);
    asm volatile("" : "+v"(qa[0]), "+v"(qa[1]), "+v"(qb[0]), "+v"(qb[1]) :: "memory");
    auto store16 = [&](int s, float m, float l, const f32x4 (&o)[4]) {
        (void)m;
        store_strip16(o, l, out + row0 * D + h * HD, D, s * 16, q_rows, lane);
    };
    {
        float m = -INFINITY, l = 0.f;
        f32x4 o[4] = {};
        for (int c = 0; c < nfull; ++c) {
            if (c % CPB == 0) {
                wait_vmcnt(max(NT - c - CPB, 0));
                __builtin_amdgcn_s_barrier();
                asm volatile("" : "+v"(qa[0]), "+v"(qa[1]), "+v"(qb[0]), "+v"(qb[1]) :: "memory");
            }
            if (hasA) attn_step16<false>(Ks + c * 4096, Vs + c * 4096, c * 32, N, lane, qa, scale_log2, m, l, o);
        }
        if (nfull % CPB == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" : "+v"(qa[0]), "+v"(qa[1]), "+v"(qb[0]), "+v"(qb[1]) :: "memory");
        }
        if (!hasA) return;
        attn_step16_t(Ks + nfull * 4096, Vs + nfull * 4096, nfull * 32, N, lane, qa, scale_log2, m, l, o);
        store16(sA, m, l, o);
    }
    if (!hasB) return;
    {
        float m = -INFINITY, l = 0.f;
        f32x4 o[4] = {};
#pragma unroll 1
        for (int c = 0; c < nfull; ++c)
            attn_step16<false>(Ks + c * 4096, Vs + c * 4096, c * 32, N, lane, qb, scale_log2, m, l, o);
        attn_step16_t(Ks + nfull * 4096, Vs + nfull * 4096, nfull * 32, N, lane, qb, scale_log2, m, l, o);
        store16(sB, m, l, o);
    }
}

'''
_DISPATCH = '''    if (N <= 256) return launch_pipe<false>('''
EDITS = [
    ("attention.hip", _STEP16_END, _TAIL + _STEP16_END),
    ("attention.hip", _KERNEL_ANCHOR, _KERNEL + _KERNEL_ANCHOR),
    ("attention.hip", _DISPATCH, '''    if (N <= 256 && (N & 31) >= 1 && (N & 31) <= 16 && q_rows > 16) {
        const size_t lds16 = (size_t)((N >> 5) * 32 + 16) * ROWB * 2;
        hipLaunchKernelGGL(k_attn_q16, dim3((unsigned)(B * H)), dim3(512), lds16, (hipStream_t)stream, qkv,
                           reinterpret_cast<bf16_t*>(out), N, H, scale_log2, q_rows);
        VPF_RETURN_LAUNCH();
    }
''' + _DISPATCH),
]
