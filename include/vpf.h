/*
 * libvpf — C-ABI of the MI355X (gfx950) tracking hot path.
 *
 * The reference (tugitbartlomiej/ViTParticleFilterTracker) is a README with no code: its ViT feature
 * extractor and particle filter are named at /root/reference/README.md:7-8 and driven per frame by
 * main.py (README.md:37, 42). It has no FFI; the interface each entry point replaces is therefore the
 * SPEC.md / SURVEY.md §8a row it implements (H1..H14), and the Python binding that a maintainer of the
 * reference would add is `vitparticlefiltertracker_amd/_lib.py` (INTEGRATION.md shows it).
 *
 * Conventions:
 *   - Every pointer is DEVICE memory unless the parameter name ends in `_host`.
 *   - The caller allocates every buffer, including workspaces; the library never allocates or frees.
 *   - Every call only enqueues work on `stream` (a hipStream_t) and never synchronises: re-entrant,
 *     stream-ordered, asynchronous, graph-capturable.
 *   - Return value: 0 on success, otherwise a hipError_t code, or VPF_ERR_ARG (-1) for an argument that
 *     violates the documented shape contract (checked on the host before any launch).
 *   - bf16 tensors are passed as uint16_t (bit pattern of bfloat16).
 *   - Particles are structure-of-arrays float[3][ld] (rows x, y, scale), `ld` >= n; float[5][ld] with the rows
 *     vx, vy after them under the constant-velocity motion model (SPEC S11).
 */
#ifndef VPF_H
#define VPF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPF_ERR_ARG (-1)

/* GEMM epilogues (vpf_gemm_bf16 / vpf_gemm_f32) */
#define VPF_EPI_BIAS 0          /* C = A W^T + bias                                              */
#define VPF_EPI_BIAS_GELU 1     /* C = gelu_erf(A W^T + bias)                                      */
#define VPF_EPI_BIAS_RESIDUAL 2 /* C = R + (A W^T + bias); R may alias C                          */
#define VPF_EPI_PATCH 3         /* row m -> token (m/g2)*(g2+1)+1+m%g2; C = A W^T + bias + pos[1+m%g2] */
#define VPF_EPI_LN 4            /* LayerNorm folded: C = rstd_m (A W'^T) - rstd_m mean_m colsum + bias'     */
#define VPF_EPI_LN_GELU 5       /* gelu_erf of the above                                                  */

/* library identity: returns a static string "libvpf <version> gfx950" */
const char* vpf_version(void);

/* H1 ParticleFilter.predict: SPEC S2, in place on particles[3][ld] (n local particles whose global
 * indices start at global_begin). */
int vpf_predict(float* particles, int64_t n, int64_t ld, int64_t global_begin, uint64_t seed,
                uint32_t frame, float sig_x, float sig_y, float sig_s, float width, float height,
                float smin, float smax, void* stream);

/* H2+H3 (A operand of the patch embed): bilinear crop + normalise + im2col, SPEC S3.
 * frame: uint8[H][W][3]; rgba_ws: caller-owned workspace of (H+2)*(W+2) uint32 (the zero-bordered RGBA
 * frame the taps read; rewritten by every call); out: [n * (S/patch)^2][Kp] bf16 (vpf_crop_patches_bf16) or
 * fp32 (_f32). norm_ab_host: 6 floats {a0,a1,a2,b0,b1,b2} (SPEC S3). Requires S > 0, S % patch == 0, Kp % 8 == 0,
 * Kp >= 3*patch^2, and non-null particles and out when n > 0. Any state is safe to pass: SPEC S3's last paragraph
 * says what a non-finite or far-away one gives. */
int vpf_crop_patches_bf16(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                          int64_t ld, int64_t n, float w0, float h0, int S, int patch, int Kp,
                          const float* norm_ab_host, uint16_t* out, void* stream);
int vpf_crop_patches_f32(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                         int64_t ld, int64_t n, float w0, float h0, int S, int patch, int Kp,
                         const float* norm_ab_host, float* out, void* stream);

/* H3 (CLS row): tokens[p][0][:] = cls + pos[0] for p < n_part; tokens: [n_part][N][D].
 * stats_out (bf16 only, may be NULL): the CLS rows' entries of the GEMM stats planes (see vpf_gemm_bf16):
 * fp32[parts][n_part*N][2], plane 0 row p*N = {sum, sumsq} of the stored bf16 row, planes 1.. = 0. */
int vpf_cls_rows_bf16(uint16_t* tokens, int64_t n_part, int N, int D, const float* cls,
                      const float* pos, float* stats_out, int parts, void* stream);
int vpf_cls_rows_f32(float* tokens, int64_t n_part, int N, int D, const float* cls, const float* pos,
                     void* stream);

/* H3/H5/H7/H8: C[M][N] = epilogue(A[M][K] * W[N][K]^T). bf16 in/out, fp32 accumulate (MFMA).
 * Row m of A at A + m*lda; row m of C (and of the residual, which has C's layout) at C + m*ldc.
 * bias: fp32[N]; residual: bf16 (EPI_BIAS_RESIDUAL, may alias C); pos: fp32[g2+1][N] (EPI_PATCH, with
 * g2 = patch_rows, M % g2 == 0); EPI_LN / EPI_LN_GELU (LayerNorm folded into the GEMM, A = the raw
 * residual stream): W = W * diag(gamma), colsum fp32[N] = sum_k W[n][k] (of the bf16 W), bias = b + W_orig beta,
 * and row_stats either (stats_parts == 0) fp32[M][2] = {mean, rstd} of A's rows (vpf_row_stats_*), or
 * (stats_parts = P in 1..16) fp32[P][M][2] planes of {sum, sumsq} over
 * disjoint column blocks of A's rows (the stats_out of the GEMM that produced A), combined with eps = ln_eps:
 * rstd = 1/sqrt(sumsq/K - mean^2 + eps).
 * stats_out (EPI_BIAS_RESIDUAL / EPI_PATCH only, may be NULL): fp32[ceil(N/64)][R][2] planes, plane t =
 * {sum, sumsq} of the stored bf16 values of each output row over columns [64t, 64t+64); R = M, or
 * (M/g2)*(g2+1) token rows for EPI_PATCH (plane rows of the CLS tokens are left to vpf_cls_rows_bf16).
 * C8 / Cs (EPI_BIAS_RESIDUAL / EPI_PATCH only, may be NULL): an MX8 copy of the stored bf16 output (rows as in
 * C: token rows for EPI_PATCH) — the A operand of a following vpf_gemm_mx8; ld8 bytes per element row,
 * lds_c >= output rows; requires N % 128 == 0 (see "MX8 operands" below).
 * Unused pointers may be NULL. Requires K % 64 == 0, N % 8 == 0, lda % 8 == 0, ldc % 8 == 0. */
int vpf_gemm_bf16(const uint16_t* A, int64_t lda, const uint16_t* W, const float* bias,
                  const uint16_t* residual, const float* pos, int patch_rows, const float* row_stats,
                  const float* colsum, uint16_t* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                  int epilogue, int stats_parts, float ln_eps, float* stats_out, uint8_t* C8, int64_t ld8,
                  uint32_t* Cs, int64_t lds_c, void* stream);
/* Split-K form of vpf_gemm_bf16 for GEMMs with few rows (the last block's CLS-row GEMMs): `splits` blocks per
 * 256 x 256 output tile each run K/splits of the K loop into fp32 partial planes (partial_ws: fp32[splits][M][N],
 * ws_elems >= splits*M*N, 16-B aligned), then one pass sums the planes in split order and applies the epilogue.
 * The summation order is fixed by (K, splits), never by M, so a row's result does not depend on how many rows the
 * call has. Epilogues: VPF_EPI_BIAS, _BIAS_GELU, _BIAS_RESIDUAL (residual: C's layout, may alias C; stats_out
 * optional, as vpf_gemm_bf16's with R = M, N % 64 == 0), _LN, _LN_GELU (row_stats = {mean, rstd} per row, colsum).
 * Requires K % (64*splits) == 0, 1 <= splits <= 64, N % 8 == 0, lda % 8 == 0, ldc % 8 == 0, 16-B aligned A, W, C. */
int vpf_gemm_bf16_splitk(const uint16_t* A, int64_t lda, const uint16_t* W, const float* bias,
                         const uint16_t* residual, const float* row_stats, const float* colsum, uint16_t* C,
                         int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue, int splits, float* stats_out,
                         float* partial_ws, int64_t ws_elems, void* stream);
/* Kernel choice for vpf_gemm_bf16 (process-wide; call it only between launches; tests and A/B timing). The product
 * library has two bf16 kernels and both give the same bits for every epilogue: kernel 1 = the deep-ring k_gemm_bf16
 * (3 A + 2 B K-tiles in LDS), 5 = the ping-pong k_gemm_pp (<= 15 statistics planes; otherwise kernel 1's form).
 * kernel 0 = the per-shape defaults (5 for VPF_EPI_LN, 1 otherwise; A-panel group 2 for N <= 1024, 8 for
 * VPF_EPI_LN_GELU, 4 otherwise). kernel 1 / 5 apply to every shape, with group >= 0 as the A-panel group size of the
 * tile order for every shape (also used by vpf_gemm_mx8; 0 = row-major) or -1 for the per-shape groups. Returns
 * VPF_ERR_ARG for any other kernel (the A/B variants of earlier rounds are in the lab build, tools/gemm_lab) or a
 * group outside [-1, 64]. Nothing in the library reads the environment. */
int vpf_gemm_tune(int kernel, int group);
/* Routing of vpf_gemm_bf16 to the tile-walking kernel k_gemm_walk (process-wide; call it only between launches; tests
 * and A/B timing). That kernel runs one workgroup per CU, each walking several 256 x 256 output tiles with the next
 * tile's first K-tiles staged under the current tile's last K-steps and epilogue; its outputs are bit-identical to
 * kernels 1 and 5. It can run VPF_EPI_LN_GELU / VPF_EPI_BIAS_GELU (FC1), VPF_EPI_LN (QKV) and, as k_gemm_walk_res,
 * VPF_EPI_BIAS_RESIDUAL without the MX8 copy (proj, FC2; stats_out or not) with K % 128 == 0,
 * stats_parts == 0, at least 8 output tiles and no kernel forced by vpf_gemm_tune; every other call keeps kernels
 * 1 / 5 whatever the mode.
 * mode 0 = the per-shape default (VPF_EPI_LN_GELU / VPF_EPI_LN calls, and VPF_EPI_BIAS_RESIDUAL calls with K = 768 or
 * K = 3072, the two K-tile counts measured against kernel 1, that can run it and have at least two tiles per
 * workgroup; VPF_EPI_BIAS_GELU keeps kernel 1, against which the walking kernel has not been timed), 1 = every call
 * that can run it (the grid shrinks to the tile count's multiple of 8), -1 = never. grid_cap: 0, or a multiple of 8 that
 * bounds the number of workgroups (so that a small problem is walked by few of them). Returns VPF_ERR_ARG otherwise. */
int vpf_gemm_persistent(int mode, int grid_cap);
/* The number of workgroups a vpf_gemm_bf16 call of this shape (no MX8 copy) would run k_gemm_walk with under the
 * current vpf_gemm_tune / vpf_gemm_persistent state on the current device; 0 = the call keeps kernels 1 / 5. Any call
 * also reads and caches the current device's CU count if that has not happened yet: call it once per device outside
 * stream capture (the engine does at construction), so that no launch inside a capture has to. */
int vpf_gemm_persistent_grid(int64_t M, int64_t N, int64_t K, int epilogue, int stats_parts);

/* MX8 operands (OCP MX-FP8: e4m3fn elements, one e8m0 scale per 32 consecutive K values):
 *   elements X8[r][k] (uint8, row stride ld8 bytes); scales (e8m0 bytes) in one plane of lds uint32 words per
 *   128-deep K-tile (lds % 64 == 0, lds >= rows), rows in bricks of 64: the scale of row r for K values
 *   [32*(k/32), +32) is byte (r/16)%4 of word (k/128)*lds + (r/64)*64 + ((k/32)%4)*16 + r%16.
 *   value(r, k) = e4m3(X8[r][k]) * 2^(scale - 127).
 * Quantisation (vpf_quantize_mx8 and every fp8-producing epilogue): per block, E = the smallest exponent with
 * amax * 2^-E <= 448 (no element saturates), clamped to [-127, 125]; byte = E + 127; elements = RNE(x * 2^-E).
 *
 * fp8 weight path (configs[4]): C[M][N] = epilogue(value(A8)[M][K] . value(W8)[N][K]^T), fp32 accumulation on
 * v_mfma_scale_f32_16x16x128_f8f6f4. A8 / As: lda bytes per row (lda % 16 == 0), scale planes of lds_a
 * words; W8 [N][K] bytes, Ws scale planes of N words (N % 64 == 0). Epilogues as vpf_gemm_bf16 except EPI_PATCH; LN
 * epilogues take colsum = the row sums of value(W8) and stats_parts <= 13 (planes over any disjoint column blocks
 * of A's rows; combined exactly as vpf_stats_combine does, so {mean, rstd} from vpf_stats_combine with
 * stats_parts = 0 gives the same bits as the planes themselves, as for vpf_gemm_bf16). C (bf16, may be NULL when C8
 * is given) and/or C8 / Cs (MX8 copy of the output, N % 128 == 0). 16-B aligned A8, W8, As, Ws; K % 128 == 0,
 * N % 8 == 0.
 * An MX8 output (here and vpf_gemm_bf16's C8 / Cs) writes element rows < M, columns < N only, and the scale words of
 * the 64-row bricks that hold a row < M; within the last such brick the bytes of rows >= M are unspecified. */
int vpf_gemm_mx8(const uint8_t* A8, int64_t lda, const uint32_t* As, int64_t lds_a, const uint8_t* W8,
                 const uint32_t* Ws, const float* bias, const uint16_t* residual, const float* row_stats,
                 const float* colsum, uint16_t* C, int64_t ldc, uint8_t* C8, int64_t ld8, uint32_t* Cs,
                 int64_t lds_c, int64_t M, int64_t N, int64_t K, int epilogue, int stats_parts, float ln_eps,
                 float* stats_out, void* stream);
/* bf16 rows -> MX8: row r of X (at X + r*ldx) -> element row r*out_stride of X8 and its scale words.
 * K % 128 == 0, X 16-B aligned, ld8 % 8 == 0, lds >= (rows-1)*out_stride + 1. */
int vpf_quantize_mx8(const uint16_t* X, int64_t ldx, int64_t rows, int64_t K, int64_t out_stride, uint8_t* X8,
                     int64_t ld8, uint32_t* S, int64_t lds, void* stream);
/* fp32 parity mode: same contract with fp32 tensors (exact-f32 MFMA, v_mfma_f32_32x32x2_f32).
 * Requires K % 32 == 0, lda % 4 == 0, ldc % 4 == 0. */
int vpf_gemm_f32(const float* A, int64_t lda, const float* W, const float* bias, const float* residual,
                 const float* pos, int patch_rows, const float* row_stats, const float* colsum, float* C,
                 int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue, void* stream);

/* H4 (folded form): out[r] = {mean, rstd = 1/sqrt(var + eps)} of row r (at x + r*x_stride), fp32.
 * bf16: D % 8 == 0; fp32: D % 4 == 0; D <= 1024. */
int vpf_row_stats_bf16(const uint16_t* x, int64_t rows, int D, int64_t x_stride, float eps, float* out,
                       void* stream);
int vpf_row_stats_f32(const float* x, int64_t rows, int D, int64_t x_stride, float eps, float* out,
                      void* stream);

/* H4 (folded form, from the producers' statistics planes): out[r] = {mean, rstd} of row r from parts planes
 * fp32[parts][plane_stride][2] of {sum, sumsq} over disjoint column blocks (a vpf_gemm_bf16 stats_out), D the row
 * length: mean = sum/D, rstd = 1/sqrt(max(sumsq/D - mean^2, 0) + eps), computed exactly as vpf_gemm_bf16's in-kernel
 * combine (so an EPI_LN* GEMM given these {mean, rstd} with stats_parts = 0 writes the same bits as one given the
 * planes). For consumers whose plane count exceeds what the ping-pong GEMM keeps in LDS (ViT-L: 16). */
int vpf_stats_combine(const float* planes, int parts, int64_t plane_stride, int64_t rows, int D, float eps, float* out,
                      void* stream);

/* H4: y = LayerNorm(x) per row (fp32 statistics). Row r of x at x + r*x_stride, of y at y + r*y_stride;
 * D % 4 == 0, D <= 1024. The kernels move 4 elements per access: x_stride and y_stride must be multiples of 4
 * elements and x and y aligned to 4 elements (8 bytes for bf16, 16 for fp32); gamma and beta 16-byte aligned.
 * Only stride >= D is checked on the host. */
int vpf_layernorm_bf16(const uint16_t* x, int64_t rows, int D, int64_t x_stride, const float* gamma,
                       const float* beta, float eps, uint16_t* y, int64_t y_stride, void* stream);
int vpf_layernorm_f32(const float* x, int64_t rows, int D, int64_t x_stride, const float* gamma,
                      const float* beta, float eps, float* y, int64_t y_stride, void* stream);

/* H6: per (particle, head) softmax(q k^T * scale) v. qkv: [B][N][3][H][hd], out: [B][N][H][hd].
 * Only the first q_rows queries of every particle are computed (q_rows = N: all; 1: the CLS row, used by
 * the last encoder layer whose other rows feed nothing). hd == 64, N <= 640 (f32: N <= 4096, keys streamed through LDS in 128-key chunks). */
int vpf_attention_bf16(const uint16_t* qkv, uint16_t* out, int64_t B, int N, int H, int hd,
                       float scale, int q_rows, void* stream);
/* fp8 path: vpf_attention_bf16 (all N <= 256 query rows) writing its output as MX8 (out8 / s8: the A operand of
 * the MX8 proj GEMM, "MX8 operands" at vpf_gemm_mx8; D = H*hd, D % 128 == 0, lds >= B*N) instead of bf16. */
int vpf_attention_bf16_mx8(const uint16_t* qkv, int64_t B, int N, int H, int hd, float scale, uint8_t* out8,
                           int64_t ld8, uint32_t* s8, int64_t lds, void* stream);
int vpf_attention_f32(const float* qkv, float* out, int64_t B, int N, int H, int hd, float scale,
                      int q_rows, void* stream);
/* H6 for the last block's CLS query with K and V never materialised (LN-folded bf16 mode). With
 * LNraw_j = (h_j - mean_j) rstd_j (statistics from the planes, as vpf_gemm_bf16's stats_parts), G_h the D-vector
 * W'_k,h^T q_h and c0_h = q_h . bk_h:  p_h = softmax_j((LNraw_j . G_h + c0_h) scale),  out_h = sum_j p_hj LNraw_j.
 * The caller finishes o_h = W'_v,h out_h + b'_v,h with one GEMM over the [n*H][D] rows of out and
 * vpf_head_gather_bf16 (vit.py).
 * tokens: bf16 [n_part][N][D] contiguous (D = 64 H, H in {6, 12, 16}, N <= 640); planes: fp32 [H][plane_rows][2]
 * {sum, sumsq} per 64-column block, row p*N + j; G: bf16 rows of ldg >= H*D ([h][D] per particle);
 * q: bf16 CLS queries (row stride ldq); bk: fp32[D]; out: bf16 rows of ldo >= H*D ([h][D]). */
/* out[p][h*hd + d] = Y[p*H + h][h*hd + d] for p < n (the diagonal blocks of a per-(particle, head) projection
 * Y: bf16 [n*H][H*hd] contiguous); out rows of ldo >= H*hd elements. hd % 8 == 0, 16-B aligned pointers. */
int vpf_head_gather_bf16(const uint16_t* Y, int64_t n, int H, int hd, uint16_t* out, int64_t ldo, void* stream);
int vpf_cls_attn_fold_bf16(const uint16_t* tokens, int64_t n_part, int N, int H, const float* planes,
                           int64_t plane_rows, float eps, const uint16_t* G, int64_t ldg, const uint16_t* q,
                           int64_t ldq, const float* bk, float scale, uint16_t* out, int64_t ldo, void* stream);

/* H9+H10: final LayerNorm of each particle's CLS row (tokens + p*N*D), cosine similarity with the
 * unit template `tmpl`, w = exp(lam (sim - 1)), Q = floor(w 2^bits) (SPEC S5).
 * feat_out (optional, may be NULL): fp32[n][D] LN'd CLS features. sim_out (optional): fp32[n].
 * tokens: [n][N][D] contiguous, D % 4 == 0, D <= 1024, so every row starts on a multiple of 4 elements; tokens aligned
 * to 4 elements (8 bytes for bf16, 16 for fp32), gamma, beta, tmpl and feat_out 16-byte aligned (4-element accesses).
 * gamma == NULL skips the LayerNorm (the CLS row itself is the feature). */
int vpf_cls_weight_bf16(const uint16_t* tokens, int64_t n, int N, int D, const float* gamma,
                        const float* beta, float eps, const float* tmpl, float lam, int bits,
                        float* feat_out, float* sim_out, int64_t* Q, void* stream);
int vpf_cls_weight_f32(const float* tokens, int64_t n, int N, int D, const float* gamma,
                       const float* beta, float eps, const float* tmpl, float lam, int bits,
                       float* feat_out, float* sim_out, int64_t* Q, void* stream);

/* Patch-token likelihood (SPEC S18): a spatial ViT cue per particle, multiplied into the CLS weight.
 *
 * tokens: [n][N][D] contiguous; row 0 of each particle (the CLS row) is skipped. For particle p and j in [1, N):
 * g_pj = LayerNorm(tokens[p][j]) with gamma, beta, eps and fp32 statistics, exactly vpf_cls_weight_*'s row arithmetic
 * (gamma == NULL skips the LayerNorm), sim_pj = <g_pj, tmpl[j-1]> / sqrtf(<g_pj, g_pj>) by SPEC S5's rule (a zero row
 * gives 0; a row with a NaN / inf, or whose squared norm overflows fp32, gives NaN), sim_p = (sum_j sim_pj) / fp32(N-1):
 * one fp32 chain from +0 in increasing j, then one IEEE division (a NaN sim_pj makes sim_p NaN), and
 * Lt_p = floor(fixed_expf(lam (fminf(sim_p, 1) - 1)) 2^bits), 0 for a non-finite sim_p.
 *   combine == 0: Q[p] = Lt_p.      combine != 0: Q[p] = (Q[p] Lt_p) >> bits in place, the product exact (128 bits).
 * tmpl: fp32[N-1][D], row j-1 the unit template of token row j. tok_sim_out (fp32[n][N-1], the sim_pj), sim_out
 * (fp32[n]) and feat_out (fp32[n][N-1][D], the g_pj) are written when not NULL. tmpl == NULL writes feat_out only
 * (feat_out is then required, Q is not read): the template of a crop is its feat_out rows, each divided by its norm.
 * The result of a particle depends on nothing but its own rows (not on n, the grid or the run). The call only
 * enqueues (no allocation, graph-capturable); n == 0 returns 0 and launches nothing (no pointer is looked at).
 * Requires N >= 2, 4 <= D <= 1024, D % 4 == 0, lam finite and >= 0, 0 <= bits <= 61, and when n > 0: tokens, beta with
 * gamma, Q with tmpl; tokens aligned to 4 elements, gamma, beta, tmpl and feat_out to 16 bytes. */
int vpf_token_weight_bf16(const uint16_t* tokens, int64_t n, int N, int D, const float* gamma, const float* beta,
                          float eps, const float* tmpl, float lam, int bits, int combine, float* feat_out,
                          float* tok_sim_out, float* sim_out, int64_t* Q, void* stream);
int vpf_token_weight_f32(const float* tokens, int64_t n, int N, int D, const float* gamma, const float* beta,
                         float eps, const float* tmpl, float lam, int bits, int combine, float* feat_out,
                         float* tok_sim_out, float* sim_out, int64_t* Q, void* stream);

/* H10 alone (ParticleFilter.update with explicit features): feat fp32[n][D] (already LN'd CLS features),
 * same weight rule as vpf_cls_weight_*. */
int vpf_cosine_weight_f32(const float* feat, int64_t n, int D, const float* tmpl, float lam, int bits,
                          float* sim_out, int64_t* Q, void* stream);

/* H11: shard partial sums, SPEC S6. out_T: int64[1] = sum Q; out_sums: fp64[3] = sum Q*{x,y,s}.
 * Fixed-order tree reduction (deterministic run to run). 0 <= n < 2^31, ld >= n. */
int vpf_shard_stats(const int64_t* Q, const float* particles, int64_t ld, int64_t n, int64_t* out_T,
                    double* out_sums, void* stream);

/* H12: systematic resample of the slots [slot_begin, slot_end) whose positions fall in this shard
 * (SPEC S7). Q: local weights (n_local); offset: sum of the weights of the shards before this one;
 * total: global sum T; P: global particle count; U: Philox offset word; uniform != 0 treats every
 * Q_i as 1 (T == 0 fallback; the caller passes offset/total in those units).
 * Writes anc_out[j - slot_begin] = global ancestor index (local + global_begin) and
 * states_out[3][out_ld] (x, y, s of the ancestor). cdf_ws: int64[n_local] workspace. */
int vpf_resample(const int64_t* Q, int64_t n_local, int64_t global_begin, int64_t offset,
                 int64_t total, int64_t P, uint32_t U, int uniform, int64_t slot_begin,
                 int64_t slot_end, const float* particles, int64_t ld, int32_t* anc_out,
                 float* states_out, int64_t out_ld, int64_t* cdf_ws, void* stream);

/* H11 + H12 over the GLOBAL particle set, device-resident (the product path of ParticleFilter): every rank
 * holds all P weights and states — its own arrays (world 1: one shard, n_shard = P) or the all-gathered shard
 * chunks (world > 1) — so nothing goes back to the host between the weights and the resample.
 * Global index i is shard r = i / n_shard, k = i % n_shard: Q_i = Q[r*q_stride + k] (int64),
 * (x, y, s)_i = particles[r*p_stride + k + {0, ld, 2*ld}] (fp32).
 * stats_out: int64[4] = {T = sum Q, then the bits of the fp64 sums sum Q*x, Q*y, Q*s} (SPEC S6, fixed-order tree
 * over the global index, so every rank and every world size gets the same bits; when T == 0 the sums are taken
 * with every Q_i = 1 and the estimate is sum / P). cdf_ws: int64[P] workspace (the inclusive CDF).
 * Resample (SPEC S7, uniform when T == 0) of the output slots [slot_begin, slot_end): anc_out = global ancestor
 * index, states_out[3][out_ld] its state. The resample word U = Philox(ctr = (0, frame, 1, 0), key = seed) word 0
 * is drawn on the device (SPEC S1). Requires 0 < P < 2^31, P % n_shard == 0, ld >= n_shard, and for several
 * shards q_stride >= n_shard, p_stride >= 2*ld + n_shard. Two launches (one workgroup, then one thread per slot). */
int vpf_estimate_resample(const int64_t* Q, int64_t q_stride, const float* particles, int64_t ld,
                          int64_t p_stride, int64_t n_shard, int64_t P, uint64_t seed, uint32_t frame,
                          int64_t slot_begin, int64_t slot_end, int32_t* anc_out, float* states_out,
                          int64_t out_ld, int64_t* cdf_ws, int64_t* stats_out, void* stream);

/* Adaptive resampling (SPEC S10). Resample schemes of vpf_estimate_resample_ex: */
#define VPF_RESAMPLE_SYSTEMATIC 0 /* SPEC S7: one word per frame, Philox ctr (0, frame, 1, 0)          */
#define VPF_RESAMPLE_STRATIFIED 1 /* SPEC S10: one word per slot j, Philox ctr (j, frame, 1, 1)         */

/* SPEC S10 rule 1, in place on a shard's n weights: Q_i = (Q_i * carry_i) >> (bits + 1), from the exact 128-bit
 * product (Q_i, carry_i >= 0; the identity carry 2^(bits+1) leaves Q_i unchanged). 0 <= bits <= 61. */
int vpf_weight_prior(int64_t* Q, const int64_t* carry, int64_t n, int bits, void* stream);

/* vpf_estimate_resample with SPEC S10's ESS gate and choice of scheme, decided on the device. Arguments, layout and
 * checks as vpf_estimate_resample, plus: method (VPF_RESAMPLE_*); ess_tau, the threshold in (0, 1], or any value < 0
 * to disable the gate (resample every frame); bits = K, 0 <= bits <= 61, with every Q_i <= 2^K; carry_out:
 * int64[>= slots], the next frame's carry of the output slots.
 * stats_out: int64[8] = {T, bits of the fp64 sums Q*x, Q*y, Q*s (as vpf_estimate_resample), bits of the fp64
 * ess = T^2 / sum Q_i^2 (sum Q_i^2 an exact 128-bit integer; 0.0 when T == 0), resampled (1 / 0), m = max Q_i, 0}.
 * resampled = T == 0, or ess_tau < 0, or ess < ess_tau * P. Resampled: anc_out / states_out as
 * vpf_estimate_resample with the scheme's positions, carry_out = 2^(K+1). Skipped: anc_out[j] = j, states_out the
 * slot's own state, carry_out[j] = Q_j << (K + 1 - bitlen(m)). With VPF_RESAMPLE_SYSTEMATIC and ess_tau < 0 it writes
 * vpf_estimate_resample's anc_out, states_out, cdf_ws and stats_out[0..3] bits. Two launches, as
 * vpf_estimate_resample. */
int vpf_estimate_resample_ex(const int64_t* Q, int64_t q_stride, const float* particles, int64_t ld,
                             int64_t p_stride, int64_t n_shard, int64_t P, uint64_t seed, uint32_t frame,
                             int64_t slot_begin, int64_t slot_end, int32_t* anc_out, float* states_out,
                             int64_t out_ld, int64_t* cdf_ws, int64_t* stats_out, int method, double ess_tau,
                             int bits, int64_t* carry_out, void* stream);

/* Occlusion gate (SPEC S15): vpf_estimate_resample_ex without the ESS gate (as ess_tau < 0), which first decides, on
 * the device and in integers, whether the frame's weights say anything at all: with m = max Q_i over the global set
 * the frame is HELD iff m < gate_q (gate_q = floor(theta 2^K) from the caller; 0 never holds; T == 0 with gate_q > 0
 * holds). Arguments, layout and checks as vpf_estimate_resample_ex, plus 0 <= gate_q <= 2^bits.
 * stats_out: int64[8] = {T (the true sum, also when held), bits of the three fp64 sums (held: the sums with every
 * weight 1, as vpf_estimate_resample's T == 0 pass), ess bits as _ex, resampled (0 when held), m, held (1 / 0)}.
 * Held: anc_out[j] = j, states_out the slot's own state, carry_out = 2^(K+1), no Philox draw; cdf_ws is unspecified.
 * Not held: every output but stats_out[7] is vpf_estimate_resample_ex's with ess_tau < 0, bit for bit (gate_q = 0:
 * always). Two launches. */
int vpf_estimate_resample_gate(const int64_t* Q, int64_t q_stride, const float* particles, int64_t ld,
                               int64_t p_stride, int64_t n_shard, int64_t P, uint64_t seed, uint32_t frame,
                               int64_t slot_begin, int64_t slot_end, int32_t* anc_out, float* states_out,
                               int64_t out_ld, int64_t* cdf_ws, int64_t* stats_out, int method, int bits,
                               int64_t gate_q, int64_t* carry_out, void* stream);

/* Constant-velocity motion model (SPEC S11): the state is (x, y, s, vx, vy), particles[5][ld]. */

/* vpf_predict for the five-row state, in place. The velocity takes the noise n3, n4 of Philox counter
 * (i, frame, 0, 1): v' = clamp(fmaf(sig_v, n, decay * v), -vmax, vmax); the position then moves by it,
 * x' = clamp(fmaf(sig_x, n0, x + vx'), 0, width - 1) (y alike), with vpf_predict's n0, n1, n2; s' is vpf_predict's.
 * With sig_v = 0, decay = 1 and zero velocities rows 0-2 are vpf_predict's bits. Requires vpf_predict's shapes,
 * 0 <= decay <= 1, sig_vx and sig_vy finite and >= 0, vmax finite and > 0. */
int vpf_predict_cv(float* particles, int64_t n, int64_t ld, int64_t global_begin, uint64_t seed, uint32_t frame,
                   float sig_x, float sig_y, float sig_s, float sig_vx, float sig_vy, float decay, float vmax,
                   float width, float height, float smin, float smax, void* stream);

/* Rotated particle boxes (SPEC S12): one more state row, the angle a in radians, appended last
 * (x | y | s | [vx | vy] | a). Angles are clamped to [amin, amax], not wrapped. */

/* Predict of the angle row alone, in place on angles[n] (global indices from global_begin), launched after
 * vpf_predict or vpf_predict_cv: a' = clamp(fmaf(sig_a, n5, a), amin, amax), n5 = sqrt(-2 ln u(g0)) cos(2 pi u(g1))
 * from words g0, g1 of Philox counter (i, frame, 0, 2). With sig_a = 0 an angle inside the range keeps its bits.
 * Requires n >= 0, global_begin >= 0, global_begin + n < 2^32, sig_a finite and >= 0, and
 * -fp32(pi) <= amin < amax <= fp32(pi). */
int vpf_predict_angle(float* angles, int64_t n, int64_t global_begin, uint64_t seed, uint32_t frame, float sig_a,
                      float amin, float amax, void* stream);

/* vpf_crop_patches_* for particles that carry an angle: angles[n] in radians, particle p's sample grid turned by
 * angles[p] about its centre (y points down the frame: a positive angle turns the box from +x towards +y). With
 * (c, s) = fixed_sincos2pi(frac(a * fp32(1 / 2 pi))), sample (ox, oy) is taken at
 *   sx = (xc + (c ex - s ey)) - 0.5, sy = (yc + (s ex + c ey)) - 0.5,
 *   ex = (ox + 0.5) dx - 0.5 bw, ey = (oy + 0.5) dy - 0.5 bh   (bw, bh, dx, dy as SPEC S3),
 * one rounded fp32 operation each; the taps, the bilinear weights, the normalisation and the im2col layout are
 * vpf_crop_patches_*'s. At a = 0 the coordinates are within 1e-5 px of SPEC S3's but not their bits. Same arguments and
 * requirements as vpf_crop_patches_*, plus angles != NULL when n > 0; only the first n columns of particles are read. */
int vpf_crop_patches_rot_bf16(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                              int64_t ld, const float* angles, int64_t n, float w0, float h0, int S, int patch, int Kp,
                              const float* norm_ab_host, uint16_t* out, void* stream);
int vpf_crop_patches_rot_f32(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                             int64_t ld, const float* angles, int64_t n, float w0, float h0, int S, int patch, int Kp,
                             const float* norm_ab_host, float* out, void* stream);

/* Resample of further state rows by ancestors already computed (vpf_estimate_resample's anc_out): for slot
 * j < n_slots and a = anc[j], out[c*out_ld + j] = rows[(a / n_shard)*p_stride + c*ld + a % n_shard], c < n_rows.
 * `rows` is the first extra row in vpf_estimate_resample's global layout (same ld, p_stride, n_shard, P): for the
 * velocity, particles + 3*ld. A slot whose anc[j] is outside [0, P) is left unwritten. Requires 1 <= n_rows <= 8,
 * out_ld >= n_slots >= 0, 0 < P < 2^31, P % n_shard == 0, ld >= n_shard, and for several shards
 * p_stride >= (n_rows - 1)*ld + n_shard. */
int vpf_gather_rows(const int32_t* anc, int64_t n_slots, const float* rows, int64_t ld, int64_t p_stride,
                    int64_t n_shard, int64_t P, int n_rows, float* out, int64_t out_ld, void* stream);

/* SPEC S6's sums over 1 <= n_rows <= 3 rows of the global layout (as vpf_gather_rows' `rows`; Q as
 * vpf_estimate_resample's): out int64[4] = {T = sum Q, bits of the fp64 sums Q_i * row_c(i); 0 for c >= n_rows},
 * with every weight 1 when T == 0. The same one-workgroup fixed-order tree as vpf_estimate_resample: over the rows
 * x | y | s it writes that call's stats_out[0..3] bit for bit, and the bits do not depend on the shard count. */
int vpf_weighted_sums(const int64_t* Q, int64_t q_stride, const float* rows, int64_t ld, int64_t p_stride,
                      int64_t n_shard, int64_t P, int n_rows, int64_t* out, void* stream);

/* vpf_weighted_sums under SPEC S15's gate: the same decision as vpf_estimate_resample_gate's, recomputed from the
 * same tree over the same weights (held iff max Q_i < gate_q), so the sums are the every-weight-1 ones exactly when
 * that call holds the frame; out[0] is the true T either way. Requires vpf_weighted_sums' shapes and
 * 0 <= gate_q <= 2^61. */
int vpf_weighted_sums_gate(const int64_t* Q, int64_t q_stride, const float* rows, int64_t ld, int64_t p_stride,
                           int64_t n_shard, int64_t P, int n_rows, int64_t gate_q, int64_t* out, void* stream);

/* Colour-histogram likelihood (SPEC S13): a second cue per particle, multiplied into the ViT weight.
 *
 * Particle i takes grid x grid bilinear samples of its box: vpf_crop_patches_*'s sample coordinates with S replaced by
 * `grid` (angles == NULL), or vpf_crop_patches_rot_*'s (angles[n] given), in raw 0..255 units with zero padding and no
 * normalisation. A sample's channel values v_c fall into bin b = (q_R bins + q_G) bins + q_B,
 * q_c = min((int)v_c, 255) >> (8 - log2 bins); h_i[b] counts the samples (sum_b h_i[b] = grid^2, nb = bins^3 bins).
 * With a template tmpl (fp32[nb], device): rho_i = sum_b sqrtf((h_i[b] / grid^2) tmpl[b]) in the pinned order (lane
 * l of 64 adds its terms b = l, l + 64, ... in increasing order from +0, then v_l += v_{l xor o} for o = 32 .. 1) and
 * Lc_i = floor(fixed_expf(lam_c (fminf(rho_i, 1) - 1)) 2^bits) (vpf_cls_weight_*'s form; a non-finite rho gives 0).
 *   combine == 0: Q[i] = Lc_i.      combine != 0: Q[i] = (Q[i] Lc_i) >> bits in place, the product exact (128 bits).
 * hist_out (uint32[n][nb]) and rho_out (fp32[n]) receive the counts and the scores when not NULL. tmpl == NULL computes
 * the histograms only (hist_out is then required, Q is not read): the template of a box is its hist_out / grid^2.
 * fill_ws != 0 first rebuilds the zero-bordered RGBA workspace rgba_ws (uint32[(H+2)(W+2)]) from `frame`; fill_ws == 0
 * reads the workspace an earlier vpf_crop_patches* / vpf_color_weight call on the same stream filled for this frame
 * (`frame` may then be NULL). The call only enqueues (no allocation, graph-capturable).
 * Requires bins in {4, 8, 16}, grid in {8, 16, 32, 64}, lam_c finite and >= 0, 0 <= bits <= 61, ld >= n >= 0,
 * (H+2)(W+2) < 2^31, rgba_ws, particles when n > 0, Q when tmpl is given; only the first n columns of particles[3][ld]
 * are read. n == 0 returns 0 and launches nothing. */
int vpf_color_weight(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, int fill_ws, const float* particles,
                     int64_t ld, const float* angles, int64_t n, float w0, float h0, int grid, int bins,
                     const float* tmpl, float lam_c, int bits, int combine, uint32_t* hist_out, float* rho_out,
                     int64_t* Q, void* stream);

/* Colour cue with a surround ring (SPEC S14): vpf_color_weight's cue and a second one over the ring around the box, in
 * one launch.
 *
 * The ring of particle i: of the grid x grid samples of its box doubled about its centre (the sample coordinates above
 * with (w0, h0) replaced by (2 w0, 2 h0); same centre, scale and angle) those with ox or oy outside
 * [grid/4, 3 grid/4), nr = 3 grid^2 / 4 samples. hs_i[b] counts them as h_i[b] counts the box's (same taps, zero
 * padding, bins). rho_i and Lc_i are vpf_color_weight's. rho_s_i = sum_b sqrtf((fp32(hs_i[b]) / fp32(nr)) tmpl[b]):
 * one IEEE division per bin, then the same pinned order, against the SAME template; a particle with a non-finite state
 * (x, y, scale or angle) has rho_s_i = NaN. sim_s = 1.0f - fminf(rho_s, 1.0f) and
 * Ls_i = floor(fixed_expf(lam_s (fminf(sim_s, 1) - 1)) 2^bits), 0 for a non-finite rho_s.
 *   combine == 0: Q[i] = (Lc_i Ls_i) >> bits.    combine != 0: Q[i] = (((Q[i] Lc_i) >> bits) Ls_i) >> bits in place.
 * Both products are exact (128 bits). hist_out / hist_s_out (uint32[n][nb]) and rho_out / rho_s_out (fp32[n]) receive
 * the box's and the ring's counts and scores when not NULL. tmpl == NULL computes the histograms only (at least one of
 * hist_out, hist_s_out is then required, Q is not read). fill_ws as for vpf_color_weight; the call only enqueues.
 * Requires vpf_color_weight's ranges and lam_s finite and >= 0. n == 0 returns 0 and launches nothing. */
int vpf_color_weight_surround(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, int fill_ws,
                              const float* particles, int64_t ld, const float* angles, int64_t n, float w0, float h0,
                              int grid, int bins, const float* tmpl, float lam_c, float lam_s, int bits, int combine,
                              uint32_t* hist_out, uint32_t* hist_s_out, float* rho_out, float* rho_s_out, int64_t* Q,
                              void* stream);

/* Search predict (SPEC S16), in place of vpf_predict (rows == 3: particles[3][ld]) or vpf_predict_cv (rows == 5:
 * particles[5][ld]) for a frame whose target is lost: particle i (global index, of P) is scattered over the frame on a
 * jittered, hole-free lattice,
 *   x = clamp(((fp32(i mod gx) + u0) inv_gx) (width - 1), 0, width - 1),
 *   y = clamp(((fp32(i) + u1) inv_P) (height - 1), 0, height - 1),
 * u0, u1 = uniform(r0), uniform(r1) of Philox counter (i, frame, 0, 3), one rounded fp32 operation each; the old x, y
 * are not read. s' is vpf_predict's for the same seed and frame, bit for bit. rows == 5 also writes +0.0f to vx and vy.
 * gx, inv_gx = fp32(1) / fp32(gx) and inv_P = fp32(1) / fp32(P) come from the caller (gx: the smallest integer >= 1
 * with gx^2 height >= P width). Only the global index enters: shard calls over [0, P) equal one whole call. Requires
 * vpf_predict's shapes, rows in {3, 5}, 1 <= P <= 2^24 (fp32(i) exact), global_begin + n <= P and 1 <= gx < 2^32.
 * n == 0 returns 0 and launches nothing. */
int vpf_predict_search(float* particles, int64_t n, int64_t ld, int64_t global_begin, int64_t P, int rows,
                       uint64_t seed, uint32_t frame, float sig_s, float width, float height, float smin, float smax,
                       int64_t gx, float inv_gx, float inv_P, void* stream);

/* Mode estimate (SPEC S17): the local weighted mean of the posterior's densest cluster, over the global particle set.
 * Q and particles in vpf_estimate_resample's global layout, with n_extra in 0..3 further state rows after x | y | s
 * (particles + 3*ld on, as vpf_weighted_sums' `rows`). With in(i, j) = fabsf(x_i - x_j) <= hx && fabsf(y_i - y_j) <= hy
 * (one rounded fp32 subtraction per axis, inclusive, false for anything NaN: a particle with a non-finite x or y is in
 * no window, not even its own):
 *   D_i = sum_j Q_j in(i, j), an exact int64, left in dens_ws (int64[P], caller-owned; zeroed inside the call);
 *   i* = min{i : D_i = max D};
 *   the sums of vpf_estimate_resample's fixed-order tree with Q_j replaced by Q_j in(i*, j), over x | y | s and the
 *   extra rows; a particle outside the window contributes +0 to every row whatever its state holds.
 * stats: the device int64 statistics block that the frame's vpf_estimate_resample / _ex / _gate call has already written
 * on the same stream: T is read at [0] and, when gate != 0, the held flag at [7]; every weight counts as 1 when T == 0
 * or the frame is held. Nothing is decided again here.
 * out: int64[8] = {i*, Tm = D_{i*}, bits of the fp64 sums of x, y, s, then of the extra rows; 0 where unused}. The mode
 * estimate is sum / Tm; Tm == 0 (no particle with a finite position carries weight) leaves the caller with SPEC S6's mean.
 * No bit depends on the grid, the tiling, the order the atomics arrive in or the shard count.
 * Requires vpf_weighted_sums' shapes for 3 + n_extra rows, hx and hy finite and >= 0, non-null pointers. One memset node
 * and two launches; the call only enqueues, allocates nothing and is graph-capturable. Every rank of a multi-rank run
 * computes the whole P^2 on its gathered view. */
int vpf_mode_estimate(const int64_t* Q, int64_t q_stride, const float* particles, int64_t ld, int64_t p_stride,
                      int64_t n_shard, int64_t P, int n_extra, float hx, float hy, const int64_t* stats, int gate,
                      int64_t* dens_ws, int64_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPF_H */
