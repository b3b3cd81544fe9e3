"""The 4 / 4 / 8 / 8 order of the walk GEMMs with q3's eight early reads (A0 of K-tile kt + 1) issued behind the phase's
first barrier, at the head of the wave row's own 16 MFMAs, instead of in front of the phase's stage (the product's
placement). Same bits. q3 has no other LDS read, so its MFMAs need no lgkmcnt wait of their own; the reads are awaited
by q0's. A/B: profiles/gemm_read_balance_ab.txt."""
EDITS = [
    ("gemm_bf16.hip",
     '''            if constexpr (EARLY) frag_read<0>(fa0, nad);   // A0(kt + 1); fa0's registers died in q1
            stage(1, skt + 2);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            bar();
            mfma_quadrant(fa1, fb0, 1, 0);''',
     '''            stage(1, skt + 2);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            bar();
            if constexpr (EARLY) {
                frag_read<0>(fa0, nad);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            acc[j][4 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                __builtin_bit_cast(bf16x8, fb0[ks][j]), __builtin_bit_cast(bf16x8, fa1[ks][i]),
                                acc[j][4 + i], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            } else {
                mfma_quadrant(fa1, fb0, 1, 0);
            }'''),
]
