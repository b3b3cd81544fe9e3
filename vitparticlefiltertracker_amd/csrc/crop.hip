// Particle crop gather (SPEC S3) and CLS rows (H3).
//
// vpf_crop_patches_*: the frame is first expanded into a zero-bordered RGBA workspace (one dword per pixel:
// every bilinear tap is one aligned load, no bounds branch), then each thread writes 8 consecutive im2col
// columns (16-B bf16 stores, coalesced across the wave): all three channels of 8 pixels on the fast path
// (patch % 8 == 0), 8 columns of one channel otherwise. The frame (150 KB at 224x224) stays L2-resident.
// Arithmetic order is SPEC S3's, contraction off, so the fp32 values are bit-identical to
// oracle/pf_oracle.c and the bf16 values are their RNE rounding.
// Degenerate states (SPEC S3, last paragraph): the tap window is the min and max over the first and the last sample,
// so a mirrored grid (non-positive scale or box side) has a correct one, and it is staged into LDS only for a finite
// state of bounded magnitude whose window is at least 1 x 1 and within the budget (the guard in stage_window). Every
// other state takes rgba_tap, which clamps any int into the zero border, and the second tap's index is next_px(i), a
// wrapping add: no LDS or workspace read lands outside its buffer whatever the state holds.
// vpf_crop_patches_rot_* (SPEC S12) is the same gather for particles that carry an angle: its own kernels further down,
// the unrotated entry points and kernels untouched.
// vpf_color_weight (SPEC S13) is the colour-histogram cue over the same RGBA workspace and sample coordinates: its own
// kernel at the end of the file.
#pragma clang fp contract(off)
#include <cstdlib>

#include "vpf_common.h"
#include "../../include/vpf.h"

using namespace vpf;

struct NormAB { float a[3]; float b[3]; };

// The frame as a zero-bordered RGBA image: rgba[(y+1)*(W+2) + (x+1)] = r | g << 8 | b << 16 for the pixel
// (y, x), 0 on the one-pixel border. A bilinear tap is then ONE aligned dword load with no bounds branch
// (coordinates clamp into the border, whose zeros are SPEC S3's zero padding).
__global__ __launch_bounds__(256) void k_frame_rgba(const uint8_t* __restrict__ frame, int H, int W,
                                                    uint32_t* __restrict__ rgba) {
    const int Wp = W + 2;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)(H + 2) * Wp) return;
    const int py = (int)(idx / Wp), px = (int)(idx - (int64_t)py * Wp);
    const int y = py - 1, x = px - 1;
    uint32_t v = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {
        const uint8_t* q = frame + ((int64_t)y * W + x) * 3;
        v = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
    rgba[idx] = v;
}

__device__ __forceinline__ uint32_t rgba_tap(const uint32_t* __restrict__ rgba, int H, int W, int yy, int xx) {
    yy = min(max(yy, -1), H);
    xx = min(max(xx, -1), W);
    return rgba[(int64_t)(yy + 1) * (W + 2) + (xx + 1)];
}
__device__ __forceinline__ float chan(uint32_t px, int c) { return (float)((px >> (8 * c)) & 255u); }
// i + 1 for a tap index that may be INT_MAX (the float -> int conversion saturates for a coordinate of 2^31 or more,
// +inf included): the sum wraps to INT_MIN, which rgba_tap clamps into the border like any other int. Written as a
// plain `i + 1` the overflow is undefined, and the compiler used that: it turned clamp(iy + 1) into
// min(max(iy, -2) + 1, H), which wraps AFTER the max and indexed the workspace 2^31 rows before its start.
__device__ __forceinline__ int next_px(int i) { return (int)((uint32_t)i + 1u); }
// fminf(fmaxf(v, lo), hi): a NaN comes out as lo.
__device__ __forceinline__ float clamp_f(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// Fast path (patch % 8 == 0, Kp == 3 patch^2), LDS-staged: one 512-thread workgroup per particle; a thread writes 8
// consecutive output pixels of one patch row (ky, kx0..kx0+7) in all three channels, the source row (sy, fy, iy)
// computed once, each sample's column once, and one dword tap serving all three channels. The particle's source window (every
// bilinear tap of its S x S samples, clamped into the zero border as rgba_tap does) is copied from the RGBA workspace
// into LDS once, and the taps read LDS instead of issuing 32 gathered dword loads per thread through the vector
// memory path, which bound the global form (the im2col stores are the same). A window larger than CROP_LDS_DW dwords
// (a large template at a large scale) takes the global taps. Same per-value arithmetic (and order) as the generic
// kernel and the oracle.
constexpr int CROP_LDS_DW = 10240;   // 40 KiB: four workgroups per CU (0.45-0.49 vs 0.53 ms at 80 KiB and two per CU,
// profiles/r2_gemm_lab/crop_lds_window_ab.txt); windows up to ~101 x 101 (a 64 x 64 template to scale ~1.55)
// The particle's crop geometry and its source window (every bilinear tap of its S x S samples, clamped into the zero
// border as rgba_tap does), staged into LDS when it fits; shared by both LDS kernels.
struct CropWin {
    float x0, y0, dx, dy;
    int cx0, cy0, wx;
    bool staged;
};
template <int NT>
__device__ __forceinline__ CropWin stage_window(uint32_t* win, const uint32_t* __restrict__ rgba, int H, int W, float xc,
                                                float yc, float sc, float w0, float h0, int S) {
    CropWin cw;
    const float bw = sc * w0, bh = sc * h0;
    cw.x0 = xc - 0.5f * bw;
    cw.y0 = yc - 0.5f * bh;
    cw.dx = bw / (float)S;
    cw.dy = bh / (float)S;
    // tap range: the computed sample coordinate is monotone in the output index (every step is a rounded monotone
    // operation), rising for a positive step and falling for a negative one (a mirrored grid), so the min and max
    // over the first and the last sample bound every sample's floor, and floor + 1 its second tap
    const float sxa = (cw.x0 + (0.0f + 0.5f) * cw.dx) - 0.5f, sxb = (cw.x0 + ((float)(S - 1) + 0.5f) * cw.dx) - 0.5f;
    const float sya = (cw.y0 + (0.0f + 0.5f) * cw.dy) - 0.5f, syb = (cw.y0 + ((float)(S - 1) + 0.5f) * cw.dy) - 0.5f;
    // the float -> int conversions are taken after the clamp into [-2, W + 1]: no out-of-range conversion
    const float fw = (float)W + 1.0f, fh = (float)H + 1.0f;
    cw.cx0 = min(max((int)clamp_f(floorf(fminf(sxa, sxb)), -2.0f, fw), -1), W);
    const int cx1 = min(max((int)clamp_f(floorf(fmaxf(sxa, sxb)) + 1.0f, -2.0f, fw), -1), W);
    cw.cy0 = min(max((int)clamp_f(floorf(fminf(sya, syb)), -2.0f, fh), -1), H);
    const int cy1 = min(max((int)clamp_f(floorf(fmaxf(sya, syb)) + 1.0f, -2.0f, fh), -1), H);
    cw.wx = cx1 - cw.cx0 + 1;
    const int wy = cy1 - cw.cy0 + 1;
    // Staged only for a finite state of bounded magnitude (stage_window_rot's bound: every sample coordinate then
    // converts to int in range, and win_tap's clamped index lies inside the window); anything else takes rgba_tap.
    const bool bounded = fabsf(xc) + fabsf(yc) + fabsf(bw) + fabsf(bh) < 262144.0f;   // false for NaN
    cw.staged = bounded && cw.wx >= 1 && wy >= 1 && (int64_t)cw.wx * wy <= CROP_LDS_DW;   // workgroup-uniform
    if (cw.staged) {
        for (int i = threadIdx.x; i < cw.wx * wy; i += NT) {
            const int r = i / cw.wx, c = i - r * cw.wx;
            win[i] = rgba[(int64_t)(cw.cy0 + r + 1) * (W + 2) + (cw.cx0 + c + 1)];
        }
    }
    __syncthreads();
    return cw;
}
__device__ __forceinline__ uint32_t win_tap(const CropWin& cw, const uint32_t* win, const uint32_t* __restrict__ rgba,
                                            int H, int W, int yy, int xx) {
    if (cw.staged) return win[(min(max(yy, -1), H) - cw.cy0) * cw.wx + (min(max(xx, -1), W) - cw.cx0)];
    return rgba_tap(rgba, H, W, yy, xx);
}

template <typename OutT>
__global__ __launch_bounds__(512) void k_crop_patches_lds(const uint32_t* __restrict__ rgba, int H, int W,
                                                          const float* __restrict__ xs, const float* __restrict__ ys,
                                                          const float* __restrict__ ss, int n_patches, int g, float w0,
                                                          float h0, int S, int patch, NormAB nab,
                                                          OutT* __restrict__ out, int split) {
    __shared__ uint32_t win[CROP_LDS_DW];
    // `split` workgroups per particle (small batches: the 8-GPU share's 512 particles would fill 2 workgroups per CU),
    // each staging the window and writing a contiguous share of the particle's rows
    const int64_t p = blockIdx.x / split;
    const int part = blockIdx.x - (int)(p * split);
    const CropWin cw = stage_window<512>(win, rgba, H, W, xs[p], ys[p], ss[p], w0, h0, S);
    const float x0 = cw.x0, y0 = cw.y0, dx = cw.dx, dy = cw.dy;
    auto tap = [&](int yy, int xx) -> uint32_t { return win_tap(cw, win, rgba, H, W, yy, xx); };
    const int per_row = patch * (patch >> 3);             // threads per im2col row
    const int pp = patch * patch;
    const int total = n_patches * per_row;
    const int t_end = (int)((int64_t)total * (part + 1) / split);
    for (int t = (int)((int64_t)total * part / split) + threadIdx.x; t < t_end; t += 512) {
        const int pi = t / per_row;
        const int tt = t - pi * per_row;
        const int ky = tt / (patch >> 3), kx0 = (tt - ky * (patch >> 3)) * 8;
        const int py = pi / g, px = pi - (pi / g) * g;
        const int oy = py * patch + ky;
        const float sy = (y0 + ((float)oy + 0.5f) * dy) - 0.5f;
        const float fy0 = floorf(sy);
        const float fy = sy - fy0;
        const int iy = (int)fy0;
        float vals[3][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ox = px * patch + kx0 + e;
            const float sx = (x0 + ((float)ox + 0.5f) * dx) - 0.5f;
            const float fx0 = floorf(sx);
            const float fx = sx - fx0;
            const int ix = (int)fx0;
            const uint32_t t00 = tap(iy, ix), t01 = tap(iy, next_px(ix));
            const uint32_t t10 = tap(next_px(iy), ix), t11 = tap(next_px(iy), next_px(ix));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float top = (1.0f - fx) * chan(t00, c) + fx * chan(t01, c);
                const float bot = (1.0f - fx) * chan(t10, c) + fx * chan(t11, c);
                const float v = (1.0f - fy) * top + fy * bot;
                vals[c][e] = fmaf(v, nab.a[c], nab.b[c]);
            }
        }
        const int64_t row = p * n_patches + pi;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            OutT* dst = out + row * (int64_t)(3 * pp) + c * pp + ky * patch + kx0;
            if constexpr (sizeof(OutT) == 2) {
                uint4 pk;
                pk.x = pack_bf2(vals[c][0], vals[c][1]); pk.y = pack_bf2(vals[c][2], vals[c][3]);
                pk.z = pack_bf2(vals[c][4], vals[c][5]); pk.w = pack_bf2(vals[c][6], vals[c][7]);
                *reinterpret_cast<uint4*>(dst) = pk;
            } else {
                *reinterpret_cast<float4*>(dst) = make_float4(vals[c][0], vals[c][1], vals[c][2], vals[c][3]);
                *reinterpret_cast<float4*>(dst + 4) = make_float4(vals[c][4], vals[c][5], vals[c][6], vals[c][7]);
            }
        }
    }
}

// Any patch / Kp (ViT-L/14: patch 14, Kp = 640 > 3 x 196), LDS-staged like the fast path: one 512-thread workgroup
// per particle stages its source window, then a thread walks one patch row (ky) of one patch: each sample's source row
// and column are computed once and one dword tap serves all three channels; bf16 pairs go out as dword stores (even
// patch). The columns past 3 patch^2 are the zero padding. Same per-value arithmetic (and order) as the oracle.
// Round 5: replaces a global-tap form (4.8 ms per ViT-L frame) and a per-element form (4.35 ms) whose index and tap
// work was repeated for every channel.
template <typename OutT>
__global__ __launch_bounds__(512) void k_crop_patches_gen(const uint32_t* __restrict__ rgba, int H, int W,
                                                          const float* __restrict__ xs, const float* __restrict__ ys,
                                                          const float* __restrict__ ss, int n_patches, int g, float w0,
                                                          float h0, int S, int patch, int Kp, NormAB nab,
                                                          OutT* __restrict__ out) {
    __shared__ uint32_t win[CROP_LDS_DW];
    const int64_t p = blockIdx.x;
    const CropWin cw = stage_window<512>(win, rgba, H, W, xs[p], ys[p], ss[p], w0, h0, S);
    auto tap = [&](int yy, int xx) -> uint32_t { return win_tap(cw, win, rgba, H, W, yy, xx); };
    const int pp = patch * patch, K = 3 * pp;
    OutT* const base = out + p * n_patches * (int64_t)Kp;
    const bool pairs = sizeof(OutT) == 2 && (patch & 1) == 0;   // 4-B aligned bf16 pairs
    for (int t = threadIdx.x; t < n_patches * patch; t += 512) {
        const int pi = t / patch, ky = t - pi * patch;
        const int py = pi / g, px = pi - py * g;
        const float sy = (cw.y0 + ((float)(py * patch + ky) + 0.5f) * cw.dy) - 0.5f;
        const float fy0 = floorf(sy);
        const float fy = sy - fy0;
        const int iy = (int)fy0;
        OutT* const row = base + (int64_t)pi * Kp + ky * patch;
        for (int kx = 0; kx < patch; kx += 2) {
            float v[3][2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int ox = px * patch + min(kx + e, patch - 1);   // odd patch: the last pair repeats a column
                const float sx = (cw.x0 + ((float)ox + 0.5f) * cw.dx) - 0.5f;
                const float fx0 = floorf(sx);
                const float fx = sx - fx0;
                const int ix = (int)fx0;
                const uint32_t t00 = tap(iy, ix), t01 = tap(iy, next_px(ix));
                const uint32_t t10 = tap(next_px(iy), ix), t11 = tap(next_px(iy), next_px(ix));
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float top = (1.0f - fx) * chan(t00, c) + fx * chan(t01, c);
                    const float bot = (1.0f - fx) * chan(t10, c) + fx * chan(t11, c);
                    const float vv = (1.0f - fy) * top + fy * bot;
                    v[c][e] = fmaf(vv, nab.a[c], nab.b[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                OutT* dst = row + c * pp + kx;
                if constexpr (sizeof(OutT) == 2) {
                    const uint32_t pk = pack_bf2(v[c][0], v[c][1]);
                    if (pairs) {
                        *reinterpret_cast<uint32_t*>(dst) = pk;
                    } else {
                        dst[0] = (OutT)(pk & 0xffffu);
                        if (kx + 1 < patch) dst[1] = (OutT)(pk >> 16);
                    }
                } else {
                    dst[0] = v[c][0];
                    if (kx + 1 < patch) dst[1] = v[c][1];
                }
            }
        }
    }
    const int pad = Kp - K;
    for (int t = threadIdx.x; t < n_patches * pad; t += 512) {
        const int pi = t / pad;
        base[(int64_t)pi * Kp + K + (t - pi * pad)] = (OutT)0;
    }
}

template <typename OutT>
static int crop_launch(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles, int64_t ld,
                       int64_t n, float w0, float h0, int S, int patch, int Kp, const float* norm_ab_host, OutT* out,
                       void* stream) {
    if (H <= 0 || W <= 0 || n < 0 || ld < n || patch <= 0 || S <= 0 || S % patch != 0 || Kp % 8 != 0 ||
        Kp < 3 * patch * patch || !norm_ab_host || !frame || !rgba_ws || (n > 0 && (!particles || !out)))
        return VPF_ERR_ARG;
    if ((int64_t)(H + 2) * (W + 2) > INT32_MAX) return VPF_ERR_ARG;
    if (n == 0) return 0;
    NormAB nab;
    for (int c = 0; c < 3; ++c) { nab.a[c] = norm_ab_host[c]; nab.b[c] = norm_ab_host[3 + c]; }
    hipStream_t st = (hipStream_t)stream;
    const int64_t npix = (int64_t)(H + 2) * (W + 2);
    hipLaunchKernelGGL(k_frame_rgba, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, frame, H, W, rgba_ws);
    const int g = S / patch;
    if (patch % 8 == 0 && Kp == 3 * patch * patch && n <= INT32_MAX / 4) {
        const int split = n >= 2048 ? 1 : n >= 1024 ? 2 : 4;   // at least ~4096 workgroups when the batch is small
        hipLaunchKernelGGL(k_crop_patches_lds<OutT>, dim3((unsigned)(n * split)), dim3(512), 0, st, rgba_ws, H, W,
                           particles, particles + ld, particles + 2 * ld, g * g, g, w0, h0, S, patch, nab, out, split);
    } else if (n <= INT32_MAX) {
        hipLaunchKernelGGL(k_crop_patches_gen<OutT>, dim3((unsigned)n), dim3(512), 0, st, rgba_ws, H, W, particles,
                           particles + ld, particles + 2 * ld, g * g, g, w0, h0, S, patch, Kp, nab, out);
    } else {
        return VPF_ERR_ARG;
    }
    VPF_RETURN_LAUNCH();
}

VPF_API int vpf_crop_patches_bf16(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                                  int64_t ld, int64_t n, float w0, float h0, int S, int patch, int Kp,
                                  const float* norm_ab_host, uint16_t* out, void* stream) {
    return crop_launch<uint16_t>(frame, H, W, rgba_ws, particles, ld, n, w0, h0, S, patch, Kp, norm_ab_host, out,
                                 stream);
}

VPF_API int vpf_crop_patches_f32(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                                 int64_t ld, int64_t n, float w0, float h0, int S, int patch, int Kp,
                                 const float* norm_ab_host, float* out, void* stream) {
    return crop_launch<float>(frame, H, W, rgba_ws, particles, ld, n, w0, h0, S, patch, Kp, norm_ab_host, out,
                              stream);
}

// ---------------- rotated crop gather (SPEC S12) ----------------
// vpf_crop_patches_rot_*: the crop of a particle that also carries an angle a. The S x S sample grid is the unrotated
// one turned by a about the box centre: sample (ox, oy) sits at (xc, yc) + R(a) (ex, ey), with (ex, ey) its offset from
// the centre in the box's own axes and (c, s) = fixed_sincos2pi(frac(a / 2 pi)) workgroup-uniform. Everything from
// ix = floor(sx) on is S3's, and both forms the unrotated gather has are kept: 8 pixels per thread with 16-B stores,
// and the per-row form for any patch / Kp. A source row is no longer shared by an output row, so every sample computes
// both coordinates; s * ey and c * ey are computed once per output row (the same single fp32 operations).
struct RotWin {
    float xc, yc, c, s, dx, dy, hbw, hbh;
    int cx0, cy0, cx1, cy1, wx;
    bool staged;
};

// SPEC S12's sample coordinates, one rounded fp32 operation each (contraction is off in this file).
__device__ __forceinline__ float rot_offset(int o, float d, float half) { return ((float)o + 0.5f) * d - half; }
__device__ __forceinline__ void rot_coord(const RotWin& w, float ex, float sey, float cey, float& sx, float& sy) {
    const float rx = w.c * ex - sey;
    const float ry = w.s * ex + cey;
    sx = (w.xc + rx) - 0.5f;
    sy = (w.yc + ry) - 0.5f;
}

// The particle's geometry and its source window, staged into LDS when it fits. The window is the bounding box of the
// four corner samples' taps, widened by one pixel on every side and clamped into the zero border.
// Why one pixel is enough: with the particle's fp32 constants (c, s, dx, dy, hbw, hbh) fixed, the exact map
// (ox, oy) -> (sx, sy) is affine, so over the grid its extremes are at the four corners. A computed coordinate differs
// from the exact one by at most E <= 8 M 2^-24 (ex or ey: two roundings; the products, their sum, + xc and - 0.5 one
// each, every intermediate bounded by M = |xc| + |yc| + bw + bh). The corners are samples too, computed by the same
// operations, so a computed interior coordinate exceeds the computed corner extremes by less than 2 E, and its floor
// by at most one pixel when 2 E < 1. Staging requires M < 2^18, where 2 E < 2^-2; a particle past that bound (or with
// a non-finite state) takes the global taps. win_tap_rot clamps every index into the window besides, so no LDS read
// lands outside it whatever the state holds.
template <int NT>
__device__ __forceinline__ RotWin stage_window_rot(uint32_t* win, const uint32_t* __restrict__ rgba, int H, int W,
                                                   float xc, float yc, float sc, float a, float w0, float h0, int S) {
    RotWin rw;
    float u = a * 0.15915494309189535f;
    u = u - floorf(u);
    fixed_sincos2pi(u, rw.c, rw.s);
    const float bw = sc * w0, bh = sc * h0;
    rw.xc = xc; rw.yc = yc;
    rw.dx = bw / (float)S;
    rw.dy = bh / (float)S;
    rw.hbw = 0.5f * bw;
    rw.hbh = 0.5f * bh;
    float xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float ex = rot_offset((k & 1) ? S - 1 : 0, rw.dx, rw.hbw);
        const float ey = rot_offset((k & 2) ? S - 1 : 0, rw.dy, rw.hbh);
        float sx, sy;
        rot_coord(rw, ex, rw.s * ey, rw.c * ey, sx, sy);
        xlo = fminf(xlo, sx); xhi = fmaxf(xhi, sx);
        ylo = fminf(ylo, sy); yhi = fmaxf(yhi, sy);
    }
    const bool bounded = fabsf(xc) + fabsf(yc) + fabsf(bw) + fabsf(bh) < 262144.0f;   // false for NaN
    // the float -> int conversions are taken after the clamp into [-2, W + 1]: no out-of-range conversion
    const float fw = (float)W + 1.0f, fh = (float)H + 1.0f;
    rw.cx0 = min(max((int)clamp_f(floorf(xlo) - 1.0f, -2.0f, fw), -1), W);
    rw.cx1 = min(max((int)clamp_f(floorf(xhi) + 2.0f, -2.0f, fw), -1), W);
    rw.cy0 = min(max((int)clamp_f(floorf(ylo) - 1.0f, -2.0f, fh), -1), H);
    rw.cy1 = min(max((int)clamp_f(floorf(yhi) + 2.0f, -2.0f, fh), -1), H);
    rw.wx = rw.cx1 - rw.cx0 + 1;
    const int wy = rw.cy1 - rw.cy0 + 1;
    rw.staged = bounded && rw.wx >= 1 && wy >= 1 && (int64_t)rw.wx * wy <= CROP_LDS_DW;   // workgroup-uniform
    if (rw.staged) {
        for (int i = threadIdx.x; i < rw.wx * wy; i += NT) {
            const int r = i / rw.wx, c = i - r * rw.wx;
            win[i] = rgba[(int64_t)(rw.cy0 + r + 1) * (W + 2) + (rw.cx0 + c + 1)];
        }
    }
    __syncthreads();
    return rw;
}
__device__ __forceinline__ uint32_t win_tap_rot(const RotWin& rw, const uint32_t* win,
                                                const uint32_t* __restrict__ rgba, int H, int W, int yy, int xx) {
    if (rw.staged) return win[(min(max(yy, rw.cy0), rw.cy1) - rw.cy0) * rw.wx + (min(max(xx, rw.cx0), rw.cx1) - rw.cx0)];
    return rgba_tap(rgba, H, W, yy, xx);
}

// One sample's three normalised channels: S3's bilinear taps and arithmetic at (sx, sy).
template <class Tap>
__device__ __forceinline__ void rot_pixel(Tap tap, float sx, float sy, const NormAB& nab, float& v0, float& v1,
                                          float& v2) {
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    const float fx = sx - fx0, fy = sy - fy0;
    const int ix = (int)fx0, iy = (int)fy0;
    const uint32_t t00 = tap(iy, ix), t01 = tap(iy, ix + 1);
    const uint32_t t10 = tap(iy + 1, ix), t11 = tap(iy + 1, ix + 1);
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = (1.0f - fx) * chan(t00, c) + fx * chan(t01, c);
        const float bot = (1.0f - fx) * chan(t10, c) + fx * chan(t11, c);
        const float vv = (1.0f - fy) * top + fy * bot;
        v[c] = fmaf(vv, nab.a[c], nab.b[c]);
    }
    v0 = v[0]; v1 = v[1]; v2 = v[2];
}

// The 8-pixel form (patch % 8 == 0, Kp == 3 patch^2): k_crop_patches_lds's work split and stores.
template <typename OutT>
__global__ __launch_bounds__(512) void k_crop_patches_rot_lds(const uint32_t* __restrict__ rgba, int H, int W,
                                                              const float* __restrict__ xs,
                                                              const float* __restrict__ ys,
                                                              const float* __restrict__ ss,
                                                              const float* __restrict__ as, int n_patches, int g,
                                                              float w0, float h0, int S, int patch, NormAB nab,
                                                              OutT* __restrict__ out, int split) {
    __shared__ uint32_t win[CROP_LDS_DW];
    const int64_t p = blockIdx.x / split;
    const int part = blockIdx.x - (int)(p * split);
    const RotWin rw = stage_window_rot<512>(win, rgba, H, W, xs[p], ys[p], ss[p], as[p], w0, h0, S);
    auto tap = [&](int yy, int xx) -> uint32_t { return win_tap_rot(rw, win, rgba, H, W, yy, xx); };
    const int per_row = patch * (patch >> 3);             // threads per im2col row
    const int pp = patch * patch;
    const int total = n_patches * per_row;
    const int t_end = (int)((int64_t)total * (part + 1) / split);
    for (int t = (int)((int64_t)total * part / split) + threadIdx.x; t < t_end; t += 512) {
        const int pi = t / per_row;
        const int tt = t - pi * per_row;
        const int ky = tt / (patch >> 3), kx0 = (tt - ky * (patch >> 3)) * 8;
        const int py = pi / g, px = pi - (pi / g) * g;
        const float ey = rot_offset(py * patch + ky, rw.dy, rw.hbh);
        const float sey = rw.s * ey, cey = rw.c * ey;
        float vals[3][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float sx, sy;
            rot_coord(rw, rot_offset(px * patch + kx0 + e, rw.dx, rw.hbw), sey, cey, sx, sy);
            rot_pixel(tap, sx, sy, nab, vals[0][e], vals[1][e], vals[2][e]);
        }
        const int64_t row = p * n_patches + pi;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            OutT* dst = out + row * (int64_t)(3 * pp) + c * pp + ky * patch + kx0;
            if constexpr (sizeof(OutT) == 2) {
                uint4 pk;
                pk.x = pack_bf2(vals[c][0], vals[c][1]); pk.y = pack_bf2(vals[c][2], vals[c][3]);
                pk.z = pack_bf2(vals[c][4], vals[c][5]); pk.w = pack_bf2(vals[c][6], vals[c][7]);
                *reinterpret_cast<uint4*>(dst) = pk;
            } else {
                *reinterpret_cast<float4*>(dst) = make_float4(vals[c][0], vals[c][1], vals[c][2], vals[c][3]);
                *reinterpret_cast<float4*>(dst + 4) = make_float4(vals[c][4], vals[c][5], vals[c][6], vals[c][7]);
            }
        }
    }
}

// The per-row form (any patch / Kp; ViT-L/14's patch 14 and Kp = 640): k_crop_patches_gen's work split, stores and
// zero padding columns.
template <typename OutT>
__global__ __launch_bounds__(512) void k_crop_patches_rot_gen(const uint32_t* __restrict__ rgba, int H, int W,
                                                              const float* __restrict__ xs,
                                                              const float* __restrict__ ys,
                                                              const float* __restrict__ ss,
                                                              const float* __restrict__ as, int n_patches, int g,
                                                              float w0, float h0, int S, int patch, int Kp, NormAB nab,
                                                              OutT* __restrict__ out) {
    __shared__ uint32_t win[CROP_LDS_DW];
    const int64_t p = blockIdx.x;
    const RotWin rw = stage_window_rot<512>(win, rgba, H, W, xs[p], ys[p], ss[p], as[p], w0, h0, S);
    auto tap = [&](int yy, int xx) -> uint32_t { return win_tap_rot(rw, win, rgba, H, W, yy, xx); };
    const int pp = patch * patch, K = 3 * pp;
    OutT* const base = out + p * n_patches * (int64_t)Kp;
    const bool pairs = sizeof(OutT) == 2 && (patch & 1) == 0;   // 4-B aligned bf16 pairs
    for (int t = threadIdx.x; t < n_patches * patch; t += 512) {
        const int pi = t / patch, ky = t - pi * patch;
        const int py = pi / g, px = pi - py * g;
        const float ey = rot_offset(py * patch + ky, rw.dy, rw.hbh);
        const float sey = rw.s * ey, cey = rw.c * ey;
        OutT* const row = base + (int64_t)pi * Kp + ky * patch;
        for (int kx = 0; kx < patch; kx += 2) {
            float v[3][2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int ox = px * patch + min(kx + e, patch - 1);   // odd patch: the last pair repeats a column
                float sx, sy;
                rot_coord(rw, rot_offset(ox, rw.dx, rw.hbw), sey, cey, sx, sy);
                rot_pixel(tap, sx, sy, nab, v[0][e], v[1][e], v[2][e]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                OutT* dst = row + c * pp + kx;
                if constexpr (sizeof(OutT) == 2) {
                    const uint32_t pk = pack_bf2(v[c][0], v[c][1]);
                    if (pairs) {
                        *reinterpret_cast<uint32_t*>(dst) = pk;
                    } else {
                        dst[0] = (OutT)(pk & 0xffffu);
                        if (kx + 1 < patch) dst[1] = (OutT)(pk >> 16);
                    }
                } else {
                    dst[0] = v[c][0];
                    if (kx + 1 < patch) dst[1] = v[c][1];
                }
            }
        }
    }
    const int pad = Kp - K;
    for (int t = threadIdx.x; t < n_patches * pad; t += 512) {
        const int pi = t / pad;
        base[(int64_t)pi * Kp + K + (t - pi * pad)] = (OutT)0;
    }
}

template <typename OutT>
static int crop_launch_rot(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles, int64_t ld,
                           const float* angles, int64_t n, float w0, float h0, int S, int patch, int Kp,
                           const float* norm_ab_host, OutT* out, void* stream) {
    if (H <= 0 || W <= 0 || n < 0 || ld < n || patch <= 0 || S <= 0 || S % patch != 0 || Kp % 8 != 0 ||
        Kp < 3 * patch * patch || !norm_ab_host || !frame || !rgba_ws || (n > 0 && (!angles || !particles || !out)))
        return VPF_ERR_ARG;
    if ((int64_t)(H + 2) * (W + 2) > INT32_MAX) return VPF_ERR_ARG;
    if (n == 0) return 0;
    NormAB nab;
    for (int c = 0; c < 3; ++c) { nab.a[c] = norm_ab_host[c]; nab.b[c] = norm_ab_host[3 + c]; }
    hipStream_t st = (hipStream_t)stream;
    const int64_t npix = (int64_t)(H + 2) * (W + 2);
    hipLaunchKernelGGL(k_frame_rgba, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, frame, H, W, rgba_ws);
    const int g = S / patch;
    if (patch % 8 == 0 && Kp == 3 * patch * patch && n <= INT32_MAX / 4) {
        const int split = n >= 2048 ? 1 : n >= 1024 ? 2 : 4;   // as the unrotated form
        hipLaunchKernelGGL(k_crop_patches_rot_lds<OutT>, dim3((unsigned)(n * split)), dim3(512), 0, st, rgba_ws, H, W,
                           particles, particles + ld, particles + 2 * ld, angles, g * g, g, w0, h0, S, patch, nab, out,
                           split);
    } else if (n <= INT32_MAX) {
        hipLaunchKernelGGL(k_crop_patches_rot_gen<OutT>, dim3((unsigned)n), dim3(512), 0, st, rgba_ws, H, W, particles,
                           particles + ld, particles + 2 * ld, angles, g * g, g, w0, h0, S, patch, Kp, nab, out);
    } else {
        return VPF_ERR_ARG;
    }
    VPF_RETURN_LAUNCH();
}

VPF_API int vpf_crop_patches_rot_bf16(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                                      int64_t ld, const float* angles, int64_t n, float w0, float h0, int S, int patch,
                                      int Kp, const float* norm_ab_host, uint16_t* out, void* stream) {
    return crop_launch_rot<uint16_t>(frame, H, W, rgba_ws, particles, ld, angles, n, w0, h0, S, patch, Kp, norm_ab_host,
                                     out, stream);
}

VPF_API int vpf_crop_patches_rot_f32(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                                     int64_t ld, const float* angles, int64_t n, float w0, float h0, int S, int patch,
                                     int Kp, const float* norm_ab_host, float* out, void* stream) {
    return crop_launch_rot<float>(frame, H, W, rgba_ws, particles, ld, angles, n, w0, h0, S, patch, Kp, norm_ab_host,
                                  out, stream);
}

// ---------------- CLS rows: tokens[p][0][:] = cls + pos[0] ----------------
template <typename T>
__global__ __launch_bounds__(256) void k_cls_rows(T* __restrict__ tok, int64_t n_part, int N, int D,
                                                  const float* __restrict__ cls, const float* __restrict__ pos) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n_part * D) return;
    const int64_t p = tid / D;
    const int d = (int)(tid - p * D);
    const float v = cls[d] + pos[d];
    if constexpr (sizeof(T) == 2) tok[p * (int64_t)N * D + d] = f2bf(v);
    else tok[p * (int64_t)N * D + d] = v;
}

// Stats-plane entries of the CLS rows (vpf_gemm_bf16 stats_out layout): every CLS row holds the same bf16
// values bf16(cls + pos[0]), so one workgroup reduces {sum, sumsq} once and writes it to plane 0 of each
// particle's CLS row (planes 1.. get 0: the consumer sums the planes).
__global__ __launch_bounds__(256) void k_cls_stats(int64_t n_part, int N, int D, const float* __restrict__ cls,
                                                   const float* __restrict__ pos, float2* __restrict__ st,
                                                   int parts) {
    __shared__ float red[2][4];
    float s = 0.f, q = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        const float v = bf2f(f2bf(cls[d] + pos[d]));
        s += v;
        q = fmaf(v, v, q);
    }
    s = wave_sum(s);
    q = wave_sum(q);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = s; red[1][w] = q; }
    __syncthreads();
    const float2 t = make_float2(red[0][0] + red[0][1] + red[0][2] + red[0][3],
                                 red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    const int64_t rows = n_part * N;
    for (int64_t p = threadIdx.x; p < n_part; p += 256)
        for (int k = 0; k < parts; ++k) st[k * rows + p * N] = k == 0 ? t : make_float2(0.f, 0.f);
}

VPF_API int vpf_cls_rows_bf16(uint16_t* tokens, int64_t n_part, int N, int D, const float* cls,
                              const float* pos, float* stats_out, int parts, void* stream) {
    if (n_part < 0 || N <= 0 || D <= 0) return VPF_ERR_ARG;
    if (stats_out && (parts < 1 || parts > 64 || ((uintptr_t)stats_out & 7))) return VPF_ERR_ARG;
    if (n_part == 0) return 0;
    const unsigned blocks = (unsigned)((n_part * D + 255) / 256);
    hipLaunchKernelGGL(k_cls_rows<uint16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, tokens, n_part, N,
                       D, cls, pos);
    if (stats_out) {
        const int e = (int)hipGetLastError();
        if (e) return e;
        hipLaunchKernelGGL(k_cls_stats, dim3(1), dim3(256), 0, (hipStream_t)stream, n_part, N, D, cls, pos,
                           reinterpret_cast<float2*>(stats_out), parts);
    }
    VPF_RETURN_LAUNCH();
}

VPF_API int vpf_cls_rows_f32(float* tokens, int64_t n_part, int N, int D, const float* cls, const float* pos,
                             void* stream) {
    if (n_part < 0 || N <= 0 || D <= 0) return VPF_ERR_ARG;
    if (n_part == 0) return 0;
    const unsigned blocks = (unsigned)((n_part * D + 255) / 256);
    hipLaunchKernelGGL(k_cls_rows<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, tokens, n_part, N, D,
                       cls, pos);
    VPF_RETURN_LAUNCH();
}

// ---------------- colour-histogram likelihood (SPEC S13) ----------------
// vpf_color_weight: a second cue per particle. One 256-thread workgroup per particle takes C x C bilinear samples of
// its box (S3's coordinates, or S12's with an angle row; raw 0..255 values, no normalisation), bins each sample's
// (R, G, B) into B^3 bins with LDS atomics, and wave 0 scores the histogram against the template by the Bhattacharyya
// coefficient in SPEC S13's pinned order: lane l sums its terms b = l, l + 64, ... in increasing order, then wave_sum's
// butterfly. The counts are integers, so their order of arrival does not matter; for B <= 8 every wave counts into a
// histogram of its own (4 x 512 bins), summed after the barrier, which spreads same-address atomics over four
// addresses. Taps are global loads through rgba_tap: the frame is L2-resident and 4 C^2 taps per particle do not repay
// staging a window. The existing kernels and entry points above are untouched.
constexpr int COLOR_NT = 256;
constexpr int COLOR_MAX_BINS = 4096;   // B = 16: 16 KiB of LDS

template <bool ROT>
__global__ __launch_bounds__(COLOR_NT) void k_color_weight(const uint32_t* __restrict__ rgba, int H, int W,
                                                            const float* __restrict__ xs, const float* __restrict__ ys,
                                                            const float* __restrict__ ss, const float* __restrict__ as,
                                                            float w0, float h0, int C, int lb,
                                                            const float* __restrict__ tmpl, float lam_c, double scale,
                                                            int sh, int combine, uint32_t* __restrict__ hist_out,
                                                            float* __restrict__ rho_out, int64_t* __restrict__ Q) {
    __shared__ uint32_t hist[COLOR_MAX_BINS];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const int nb = 1 << (3 * lb);
    const int nsub = 4 * nb <= COLOR_MAX_BINS ? 4 : 1;     // a histogram per wave when four fit
    for (int i = tid; i < nsub * nb; i += COLOR_NT) hist[i] = 0u;
    __syncthreads();
    uint32_t* const mine = hist + (nsub == 4 ? (tid >> 6) * nb : 0);
    const float xc = xs[p], yc = ys[p], sc = ss[p];
    const float bw = sc * w0, bh = sc * h0;
    const float dx = bw / (float)C, dy = bh / (float)C;
    const float x0 = xc - 0.5f * bw, y0 = yc - 0.5f * bh;  // S3's origin (unrotated form)
    RotWin rw;                                             // S12's constants (rotated form); the window is not used
    rw.xc = xc; rw.yc = yc; rw.dx = dx; rw.dy = dy; rw.hbw = 0.5f * bw; rw.hbh = 0.5f * bh;
    rw.c = 1.0f; rw.s = 0.0f;
    if constexpr (ROT) {
        float u = as[p] * 0.15915494309189535f;
        u = u - floorf(u);
        fixed_sincos2pi(u, rw.c, rw.s);
    }
    const int shift = 8 - lb;
    for (int t = tid; t < C * C; t += COLOR_NT) {
        const int oy = t / C, ox = t - oy * C;
        float sx, sy;
        if constexpr (ROT) {
            const float ey = rot_offset(oy, rw.dy, rw.hbh);
            rot_coord(rw, rot_offset(ox, rw.dx, rw.hbw), rw.s * ey, rw.c * ey, sx, sy);
        } else {
            sx = (x0 + ((float)ox + 0.5f) * dx) - 0.5f;
            sy = (y0 + ((float)oy + 0.5f) * dy) - 0.5f;
        }
        const float fx0 = floorf(sx), fy0 = floorf(sy);
        const float fx = sx - fx0, fy = sy - fy0;
        const int ix = (int)fx0, iy = (int)fy0;
        const uint32_t t00 = rgba_tap(rgba, H, W, iy, ix), t01 = rgba_tap(rgba, H, W, iy, ix + 1);
        const uint32_t t10 = rgba_tap(rgba, H, W, iy + 1, ix), t11 = rgba_tap(rgba, H, W, iy + 1, ix + 1);
        int b = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = (1.0f - fx) * chan(t00, c) + fx * chan(t01, c);
            const float bot = (1.0f - fx) * chan(t10, c) + fx * chan(t11, c);
            const float v = (1.0f - fy) * top + fy * bot;
            const int q = min(max((int)v, 0), 255) >> shift;   // v >= 0 for every finite state; the max keeps b in range
            b = (b << lb) | q;
        }
        atomicAdd(&mine[b], 1u);
    }
    __syncthreads();
    for (int b = tid; b < nb; b += COLOR_NT) {
        uint32_t h = hist[b];
        if (nsub == 4) {
            h += hist[nb + b] + hist[2 * nb + b] + hist[3 * nb + b];
            hist[b] = h;
        }
        if (hist_out) hist_out[p * nb + b] = h;
    }
    if (!tmpl) return;                                     // workgroup-uniform
    __syncthreads();
    if (tid >= 64) return;
    const float cc = (float)(C * C);
    float acc = 0.0f;
    for (int b = tid; b < nb; b += 64) {
        const float pb = (float)hist[b] / cc;              // exact: C^2 is a power of two
        acc = acc + sqrtf(pb * tmpl[b]);
    }
    const float rho = wave_sum(acc);
    if (tid == 0) {
        const float w = isfinite(rho) ? fixed_expf(lam_c * (fminf(rho, 1.0f) - 1.0f)) : 0.0f;
        const uint64_t lc = (uint64_t)(int64_t)floor((double)w * scale);
        if (rho_out) rho_out[p] = rho;
        if (combine) {
            const uint64_t l = (uint64_t)Q[p];
            const uint64_t hi = __umul64hi(l, lc), lo = l * lc;
            Q[p] = (int64_t)(sh ? (hi << (64 - sh)) | (lo >> sh) : lo);
        } else {
            Q[p] = (int64_t)lc;
        }
    }
}

VPF_API int vpf_color_weight(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, int fill_ws,
                             const float* particles, int64_t ld, const float* angles, int64_t n, float w0, float h0,
                             int grid, int bins, const float* tmpl, float lam_c, int bits, int combine,
                             uint32_t* hist_out, float* rho_out, int64_t* Q, void* stream) {
    if (H <= 0 || W <= 0 || n < 0 || ld < n || !rgba_ws || (fill_ws && !frame)) return VPF_ERR_ARG;
    if ((int64_t)(H + 2) * (W + 2) > INT32_MAX || n > INT32_MAX) return VPF_ERR_ARG;
    if (bins != 4 && bins != 8 && bins != 16) return VPF_ERR_ARG;
    if (grid != 8 && grid != 16 && grid != 32 && grid != 64) return VPF_ERR_ARG;
    if (!(lam_c >= 0.0f) || !(lam_c <= 3.4028234663852886e38f) || bits < 0 || bits > 61) return VPF_ERR_ARG;
    if (tmpl ? !Q : !hist_out) return VPF_ERR_ARG;         // a template needs Q; without one the histograms are the output
    if (n > 0 && !particles) return VPF_ERR_ARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (fill_ws) {
        const int64_t npix = (int64_t)(H + 2) * (W + 2);
        hipLaunchKernelGGL(k_frame_rgba, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, frame, H, W, rgba_ws);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    const int lb = bins == 4 ? 2 : bins == 8 ? 3 : 4;
    const double scale = (double)((uint64_t)1 << bits);
    if (angles)
        hipLaunchKernelGGL(k_color_weight<true>, dim3((unsigned)n), dim3(COLOR_NT), 0, st, rgba_ws, H, W, particles,
                           particles + ld, particles + 2 * ld, angles, w0, h0, grid, lb, tmpl, lam_c, scale, bits,
                           combine, hist_out, rho_out, Q);
    else
        hipLaunchKernelGGL(k_color_weight<false>, dim3((unsigned)n), dim3(COLOR_NT), 0, st, rgba_ws, H, W, particles,
                           particles + ld, particles + 2 * ld, angles, w0, h0, grid, lb, tmpl, lam_c, scale, bits,
                           combine, hist_out, rho_out, Q);
    VPF_RETURN_LAUNCH();
}

// ---------------- colour cue with a surround ring (SPEC S14) ----------------
// vpf_color_weight_surround: S13's cue and a second one over the ring around the box, fused in one launch. The ring is
// the box doubled about its centre minus the box: of the C x C samples of the doubled box (S3's / S12's coordinates
// with (w0, h0) -> (2 w0, 2 h0); same centre, scale and angle) those with ox or oy outside [C/4, 3C/4), 3 C^2 / 4 of
// them. One 256-thread workgroup per particle walks the C^2 inner and 3 C^2 / 4 ring samples as ONE list (7 C^2 / 4
// items, strided over the threads; C^2 is a multiple of 64, so a wave's items of one pass are all inner or all ring),
// ring samples enumerated directly: two full-width bands of C/4 rows, then the C/2 middle rows' two side pieces.
// Two LDS histograms (inner at 0, ring at COLOR_MAX_BINS; 2 x 16 KiB at B = 16), one pair per wave for B <= 8 as in
// k_color_weight. After the barrier wave 0 scores rho (counts / C^2) and wave 1 rho_s (counts / (3 C^2 / 4), one IEEE
// division) at the same time, both in S13's pinned order; lane 0 then forms Lc and Ls = weight(1 - min(rho_s, 1)) and
// does both exact products on Q. A particle with a non-finite state has rho_s = NaN and so Ls = 0.
// k_color_weight, its entry point and the helpers it uses are untouched; the sample's value and bin are restated here.
__device__ __forceinline__ int color_sample_bin(const uint32_t* __restrict__ rgba, int H, int W, float sx, float sy,
                                                int lb) {
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    const float fx = sx - fx0, fy = sy - fy0;
    const int ix = (int)fx0, iy = (int)fy0;
    const uint32_t t00 = rgba_tap(rgba, H, W, iy, ix), t01 = rgba_tap(rgba, H, W, iy, ix + 1);
    const uint32_t t10 = rgba_tap(rgba, H, W, iy + 1, ix), t11 = rgba_tap(rgba, H, W, iy + 1, ix + 1);
    const int shift = 8 - lb;
    int b = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = (1.0f - fx) * chan(t00, c) + fx * chan(t01, c);
        const float bot = (1.0f - fx) * chan(t10, c) + fx * chan(t11, c);
        const float v = (1.0f - fy) * top + fy * bot;
        const int q = min(max((int)v, 0), 255) >> shift;       // as k_color_weight: the max keeps b in range
        b = (b << lb) | q;
    }
    return b;
}

// (a b) >> sh with the product exact (128 bits), 0 <= sh <= 61.
__device__ __forceinline__ uint64_t mul_shift(uint64_t a, uint64_t b, int sh) {
    const uint64_t hi = __umul64hi(a, b), lo = a * b;
    return sh ? (hi << (64 - sh)) | (lo >> sh) : lo;
}

// A grid's constants for a box of bw x bh: the sample steps and the half sides (S3's x0 is xc - hbw).
__device__ __forceinline__ void surround_grid(RotWin& g, float xc, float yc, float c, float s, float bw, float bh,
                                              int C) {
    g.xc = xc; g.yc = yc; g.c = c; g.s = s;
    g.dx = bw / (float)C; g.dy = bh / (float)C;
    g.hbw = 0.5f * bw; g.hbh = 0.5f * bh;
}

template <bool ROT>
__global__ __launch_bounds__(COLOR_NT) void k_color_weight_surround(
    const uint32_t* __restrict__ rgba, int H, int W, const float* __restrict__ xs, const float* __restrict__ ys,
    const float* __restrict__ ss, const float* __restrict__ as, float w0, float h0, int C, int lc2, int lb,
    const float* __restrict__ tmpl, float lam_c, float lam_s, double scale, int sh, int combine,
    uint32_t* __restrict__ hist_out, uint32_t* __restrict__ hist_s_out, float* __restrict__ rho_out,
    float* __restrict__ rho_s_out, int64_t* __restrict__ Q) {
    __shared__ uint32_t hist[2 * COLOR_MAX_BINS];          // inner histogram(s) at 0, ring histogram(s) at COLOR_MAX_BINS
    __shared__ float rho_sh[2];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nb = 1 << (3 * lb);
    const int nsub = 4 * nb <= COLOR_MAX_BINS ? 4 : 1;     // a pair of histograms per wave when four fit
    for (int i = tid; i < nsub * nb; i += COLOR_NT) {
        hist[i] = 0u;
        hist[COLOR_MAX_BINS + i] = 0u;
    }
    __syncthreads();
    uint32_t* const mine = hist + (nsub == 4 ? wave * nb : 0);
    const float xc = xs[p], yc = ys[p], sc = ss[p];
    bool fin = isfinite(xc) && isfinite(yc) && isfinite(sc);
    // both grids' constants, once: g0 the box (S13's), g1 the doubled box (2 w0 and 2 h0 are exact)
    float c = 1.0f, s = 0.0f;
    if constexpr (ROT) {
        const float a = as[p];
        fin = fin && isfinite(a);
        float u = a * 0.15915494309189535f;
        u = u - floorf(u);
        fixed_sincos2pi(u, c, s);
    }
    RotWin g0, g1;
    surround_grid(g0, xc, yc, c, s, sc * w0, sc * h0, C);
    surround_grid(g1, xc, yc, c, s, sc * (2.0f * w0), sc * (2.0f * h0), C);
    const int CC = C * C, Q4 = CC >> 2, C4 = C >> 2;
    for (int t = tid; t < CC + 3 * Q4; t += COLOR_NT) {
        const int ring = t >= CC;                          // wave-uniform: CC is a multiple of 64
        int ox, oy;
        if (!ring) {
            oy = t >> lc2;
            ox = t & (C - 1);
        } else {
            const int r = t - CC, band = r >> (2 * lc2 - 2), j = r & (Q4 - 1);
            if (band < 2) {                                // rows [0, C/4) and [3C/4, C), full width
                oy = (j >> lc2) + (band ? 3 * C4 : 0);
                ox = j & (C - 1);
            } else {                                       // rows [C/4, 3C/4): columns [0, C/4) and [3C/4, C)
                const int k = j & (2 * C4 - 1);
                oy = C4 + (j >> (lc2 - 1));
                ox = k < C4 ? k : k + 2 * C4;
            }
        }
        RotWin w;                                          // a select per constant, no indexed array
        w.xc = xc; w.yc = yc; w.c = c; w.s = s;
        w.dx = ring ? g1.dx : g0.dx; w.dy = ring ? g1.dy : g0.dy;
        w.hbw = ring ? g1.hbw : g0.hbw; w.hbh = ring ? g1.hbh : g0.hbh;
        float sx, sy;
        if constexpr (ROT) {
            const float ey = rot_offset(oy, w.dy, w.hbh);
            rot_coord(w, rot_offset(ox, w.dx, w.hbw), w.s * ey, w.c * ey, sx, sy);
        } else {
            sx = ((xc - w.hbw) + ((float)ox + 0.5f) * w.dx) - 0.5f;     // S3: x0 = xc - 0.5 bw
            sy = ((yc - w.hbh) + ((float)oy + 0.5f) * w.dy) - 0.5f;
        }
        atomicAdd(&mine[ring * COLOR_MAX_BINS + color_sample_bin(rgba, H, W, sx, sy, lb)], 1u);
    }
    __syncthreads();
    for (int b = tid; b < nb; b += COLOR_NT) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            uint32_t* const hk = hist + k * COLOR_MAX_BINS;
            uint32_t h = hk[b];
            if (nsub == 4) {
                h += hk[nb + b] + hk[2 * nb + b] + hk[3 * nb + b];
                hk[b] = h;
            }
            uint32_t* const out = k ? hist_s_out : hist_out;
            if (out) out[p * nb + b] = h;
        }
    }
    if (!tmpl) return;                                     // workgroup-uniform
    __syncthreads();
    if (wave < 2) {                                        // wave 0: rho over the box, wave 1: rho_s over the ring
        const uint32_t* const hk = hist + wave * COLOR_MAX_BINS;
        const float den = wave ? (float)(3 * Q4) : (float)CC;
        float acc = 0.0f;
        for (int b = lane; b < nb; b += 64) {
            const float pb = (float)hk[b] / den;           // the box: exact; the ring: one rounded division
            acc = acc + sqrtf(pb * tmpl[b]);
        }
        const float r = wave_sum(acc);
        if (lane == 0) rho_sh[wave] = r;
    }
    __syncthreads();
    if (tid == 0) {
        const float rho = rho_sh[0];
        const float rho_s = fin ? rho_sh[1] : __builtin_nanf("");
        const float wc = isfinite(rho) ? fixed_expf(lam_c * (fminf(rho, 1.0f) - 1.0f)) : 0.0f;
        const float sim_s = 1.0f - fminf(rho_s, 1.0f);
        const float ws = isfinite(rho_s) ? fixed_expf(lam_s * (fminf(sim_s, 1.0f) - 1.0f)) : 0.0f;
        const uint64_t lc = (uint64_t)(int64_t)floor((double)wc * scale);
        const uint64_t ls = (uint64_t)(int64_t)floor((double)ws * scale);
        if (rho_out) rho_out[p] = rho;
        if (rho_s_out) rho_s_out[p] = rho_s;
        const uint64_t l = combine ? mul_shift((uint64_t)Q[p], lc, sh) : lc;
        Q[p] = (int64_t)mul_shift(l, ls, sh);
    }
}

VPF_API int vpf_color_weight_surround(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, int fill_ws,
                                      const float* particles, int64_t ld, const float* angles, int64_t n, float w0,
                                      float h0, int grid, int bins, const float* tmpl, float lam_c, float lam_s,
                                      int bits, int combine, uint32_t* hist_out, uint32_t* hist_s_out, float* rho_out,
                                      float* rho_s_out, int64_t* Q, void* stream) {
    if (H <= 0 || W <= 0 || n < 0 || ld < n || !rgba_ws || (fill_ws && !frame)) return VPF_ERR_ARG;
    if ((int64_t)(H + 2) * (W + 2) > INT32_MAX || n > INT32_MAX) return VPF_ERR_ARG;
    if (bins != 4 && bins != 8 && bins != 16) return VPF_ERR_ARG;
    if (grid != 8 && grid != 16 && grid != 32 && grid != 64) return VPF_ERR_ARG;
    if (!(lam_c >= 0.0f) || !(lam_c <= 3.4028234663852886e38f) || bits < 0 || bits > 61) return VPF_ERR_ARG;
    if (!(lam_s >= 0.0f) || !(lam_s <= 3.4028234663852886e38f)) return VPF_ERR_ARG;
    if (tmpl ? !Q : !(hist_out || hist_s_out)) return VPF_ERR_ARG;   // without a template the histograms are the output
    if (n > 0 && !particles) return VPF_ERR_ARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (fill_ws) {
        const int64_t npix = (int64_t)(H + 2) * (W + 2);
        hipLaunchKernelGGL(k_frame_rgba, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, frame, H, W, rgba_ws);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    const int lb = bins == 4 ? 2 : bins == 8 ? 3 : 4;
    const int lc2 = grid == 8 ? 3 : grid == 16 ? 4 : grid == 32 ? 5 : 6;
    const double scale = (double)((uint64_t)1 << bits);
    if (angles)
        hipLaunchKernelGGL(k_color_weight_surround<true>, dim3((unsigned)n), dim3(COLOR_NT), 0, st, rgba_ws, H, W,
                           particles, particles + ld, particles + 2 * ld, angles, w0, h0, grid, lc2, lb, tmpl, lam_c,
                           lam_s, scale, bits, combine, hist_out, hist_s_out, rho_out, rho_s_out, Q);
    else
        hipLaunchKernelGGL(k_color_weight_surround<false>, dim3((unsigned)n), dim3(COLOR_NT), 0, st, rgba_ws, H, W,
                           particles, particles + ld, particles + 2 * ld, angles, w0, h0, grid, lc2, lb, tmpl, lam_c,
                           lam_s, scale, bits, combine, hist_out, hist_s_out, rho_out, rho_s_out, Q);
    VPF_RETURN_LAUNCH();
}
