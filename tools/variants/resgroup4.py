"""Round 11: tile group 4 instead of 2 for the N <= 1024 GEMMs (proj / FC2, on the walking kernel since round 11):
the group sweep of profiles/r11_lab/gemm_walk_res_ab.txt. The order never changes a bit."""
EDITS = [("gemm_bf16.hip", "    if (N <= 1024) return 2;\n", "    if (N <= 1024) return 4;\n")]
