"""PROBE (wrong outputs by design; timing only, never compared for bits): the walk GEMMs in the 12 / 4 / 8 / 0 order
with q0's read_a(fa0) left out, i.e. 4 / 4 / 8 / 0 reads per K-tile. The MFMAs of q0 and q1 run on whatever the
registers hold (an empty asm in the reads' place defines them, so their live range is the parent's). The ceiling of any re-placement of those 8
ds_read_b128 per wave and K-tile: profiles/gemm_read_balance_bound.txt."""
EARLY_RULE = '''constexpr bool walk_reads_early(int epi) {
    return epi == VPF_EPI_LN || epi == VPF_EPI_LN_GELU || epi == VPF_EPI_BIAS_RESIDUAL;
}'''
EDITS = [
    ("gemm_bf16.hip",
     EARLY_RULE,
     "constexpr bool walk_reads_early(int epi) { return false; }"),
    ("gemm_bf16.hip",
     '''                read_a(fa0, buf);
                read_b(fb0, buf + HALF);''',
     '''#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int i = 0; i < 4; ++i) asm volatile("" : "=v"(fa0[ks][i]));
                read_b(fb0, buf + HALF);'''),
]
