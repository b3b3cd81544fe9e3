// Particle crop gather (SPEC S3, rotated S12), CLS rows (H3) and the colour cues (SPEC S13, S14).
//
// Everything that samples the frame here is built from one set of pieces, each defined once:
//   the sample   bilinear_at / bilinear: S3's four taps and arithmetic, the second tap's index always next_px(i);
//   the grid     UprightGrid (S3's coordinates) and RotGrid (S12's), the same interface, different formulas;
//   the window   Window / make_window / stage_particle / win_tap: the particle's tap window, staged into LDS when it fits;
//   the stores   store8 (16 B) and store2 (a pair, or elements for an odd patch).
// vpf_crop_patches_* and vpf_crop_patches_rot_*: the frame is first expanded into a zero-bordered RGBA workspace (one
// dword per pixel: every bilinear tap is one aligned load, no bounds branch), then each thread writes 8 consecutive
// im2col columns (16-B bf16 stores, coalesced across the wave): all three channels of 8 pixels on the fast path
// (patch % 8 == 0), one patch row of one patch otherwise. The frame (150 KB at 224x224) stays L2-resident. The two
// kernel bodies are templates over the grid; with an angle row the launcher picks the RotGrid instantiation.
// Arithmetic order is SPEC S3's / S12's, contraction off, so the fp32 values are bit-identical to oracle/pf_oracle.c
// and the bf16 values are their RNE rounding.
// Degenerate states (SPEC S3, last paragraph): the window is staged only for a finite state of bounded magnitude whose
// window is at least 1 x 1 and within the budget (the guard in make_window), and a staged tap's index is clamped into
// the window. Every other state takes rgba_tap, which clamps any int into the zero border, and the second tap's index
// is next_px(i), a wrapping add: no LDS or workspace read lands outside its buffer whatever the state holds.
// vpf_color_weight (SPEC S13) and vpf_color_weight_surround (S14) are the colour-histogram cues over the same RGBA
// workspace, grids and sample: two kernels at the end of the file, built from shared helpers.
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

// Fills the workspace on the stream; returns the launch's status.
static int fill_rgba_ws(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, hipStream_t st) {
    const int64_t npix = (int64_t)(H + 2) * (W + 2);
    hipLaunchKernelGGL(k_frame_rgba, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, frame, H, W, rgba_ws);
    return (int)hipGetLastError();
}

__device__ __forceinline__ uint32_t rgba_tap(const uint32_t* __restrict__ rgba, int H, int W, int yy, int xx) {
    yy = min(max(yy, -1), H);
    xx = min(max(xx, -1), W);
    return rgba[(int64_t)(yy + 1) * (W + 2) + (xx + 1)];
}
__device__ __forceinline__ float chan(uint32_t px, int c) { return (float)((px >> (8 * c)) & 255u); }
// i + 1 for a tap index that may be INT_MAX (the float -> int conversion saturates for a coordinate of 2^31 or more,
// +inf included): the sum wraps to INT_MIN, which every tap function clamps like any other int. Written as a plain
// `i + 1` the overflow is undefined, and the compiler used that: it turned clamp(i + 1) into min(max(i, -2) + 1, H),
// which wraps AFTER the max and indexed the workspace 2^31 rows before its start.
__device__ __forceinline__ int next_px(int i) { return (int)((uint32_t)i + 1u); }
// fminf(fmaxf(v, lo), hi): a NaN comes out as lo.
__device__ __forceinline__ float clamp_f(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---------------- the sample (SPEC S3) ----------------
// A coordinate's pixel index and fraction: s = i + f.
__device__ __forceinline__ void split_px(float s, int& i, float& f) {
    const float s0 = floorf(s);
    f = s - s0;
    i = (int)s0;
}
// S3's value at the pre-floored (ix, iy, fx, fy): the three raw channel values (0..255) of the bilinear sample, one
// dword tap serving all three. tap(yy, xx) takes any int. This is the only place that forms a second tap's index.
template <class Tap>
__device__ __forceinline__ void bilinear_at(Tap tap, int ix, int iy, float fx, float fy, float (&v)[3]) {
    const int ix1 = next_px(ix), iy1 = next_px(iy);
    const uint32_t t00 = tap(iy, ix), t01 = tap(iy, ix1);
    const uint32_t t10 = tap(iy1, ix), t11 = tap(iy1, ix1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const auto across = [&](uint32_t l, uint32_t r) { return (1.0f - fx) * chan(l, c) + fx * chan(r, c); };
        const float top = across(t00, t01);
        const float bot = across(t10, t11);
        v[c] = (1.0f - fy) * top + fy * bot;
    }
}
template <class Tap>
__device__ __forceinline__ void bilinear(Tap tap, float sx, float sy, float (&v)[3]) {
    int ix, iy;
    float fx, fy;
    split_px(sx, ix, fx);
    split_px(sy, iy, fy);
    bilinear_at(tap, ix, iy, fx, fy, v);
}

// ---------------- the two sample grids ----------------
// An n x n grid over a bw x bh box centred on (xc, yc). Both kinds offer: row(oy), the part of a sample that its whole
// output row shares (hoisted by the callers); sample(tap, row, ox, v), the sample (ox, oy); taps(n), the first and last
// tap index of each axis over the whole grid, as floats of any value (NaN included), for make_window. Each line is
// SPEC's single rounded fp32 operation, in SPEC's order. The formulas differ (S3 subtracts half the box from the
// centre, S12 from the sample's offset), so a RotGrid at angle 0 is not an UprightGrid bit for bit.
struct TapRange { float x0, x1, y0, y1; };

struct UprightGrid {   // SPEC S3
    static constexpr bool rotated = false;
    float x0, y0, dx, dy;
    struct Row { int iy; float fy; };
    __device__ __forceinline__ UprightGrid(float xc, float yc, float bw, float bh, int n)
        : x0(xc - 0.5f * bw), y0(yc - 0.5f * bh), dx(bw / (float)n), dy(bh / (float)n) {}
    __device__ __forceinline__ float x(int ox) const { return (x0 + ((float)ox + 0.5f) * dx) - 0.5f; }
    __device__ __forceinline__ float y(int oy) const { return (y0 + ((float)oy + 0.5f) * dy) - 0.5f; }
    __device__ __forceinline__ Row row(int oy) const {
        Row r;
        split_px(y(oy), r.iy, r.fy);
        return r;
    }
    template <class Tap>
    __device__ __forceinline__ void sample(Tap tap, const Row& r, int ox, float (&v)[3]) const {
        int ix;
        float fx;
        split_px(x(ox), ix, fx);
        bilinear_at(tap, ix, r.iy, fx, r.fy, v);
    }
    // The computed coordinate is monotone in the output index (every step is a rounded monotone operation), rising
    // for a positive step and falling for a negative one (a mirrored grid), so the min and max over the first and the
    // last sample bound every sample's floor, and floor + 1 its second tap.
    __device__ __forceinline__ TapRange taps(int n) const {
        const float xa = x(0), xb = x(n - 1), ya = y(0), yb = y(n - 1);
        return {floorf(fminf(xa, xb)), floorf(fmaxf(xa, xb)) + 1.0f, floorf(fminf(ya, yb)), floorf(fmaxf(ya, yb)) + 1.0f};
    }
};

// SPEC S12's angle reduction: (c, s) = fixed_sincos2pi(frac(a / 2 pi)).
__device__ __forceinline__ void angle_cs(float a, float& c, float& s) {
    float u = a * 0.15915494309189535f;
    u = u - floorf(u);
    fixed_sincos2pi(u, c, s);
}

struct RotGrid {   // SPEC S12: the upright grid turned by the angle about the box centre
    static constexpr bool rotated = true;
    float xc, yc, c, s, dx, dy, hbw, hbh;
    struct Row { float sey, cey; };   // s ey and c ey: a source row is not shared by an output row, these two are
    __device__ __forceinline__ RotGrid(float xc_, float yc_, float bw, float bh, int n, float angle)
        : xc(xc_), yc(yc_), dx(bw / (float)n), dy(bh / (float)n), hbw(0.5f * bw), hbh(0.5f * bh) {
        angle_cs(angle, c, s);
    }
    // a sample's offset from the centre in the box's own axes
    static __device__ __forceinline__ float offset(int o, float d, float half) { return ((float)o + 0.5f) * d - half; }
    __device__ __forceinline__ Row row(int oy) const {
        const float ey = offset(oy, dy, hbh);
        return {s * ey, c * ey};
    }
    __device__ __forceinline__ void at(const Row& r, int ox, float& sx, float& sy) const {
        const float ex = offset(ox, dx, hbw);
        const float rx = c * ex - r.sey;
        const float ry = s * ex + r.cey;
        sx = (xc + rx) - 0.5f;
        sy = (yc + ry) - 0.5f;
    }
    template <class Tap>
    __device__ __forceinline__ void sample(Tap tap, const Row& r, int ox, float (&v)[3]) const {
        float sx, sy;
        at(r, ox, sx, sy);
        bilinear(tap, sx, sy, v);
    }
    // The bounding box of the four corner samples' taps, widened by one pixel on every side.
    // Why one pixel is enough: with the particle's fp32 constants (c, s, dx, dy, hbw, hbh) fixed, the exact map
    // (ox, oy) -> (sx, sy) is affine, so over the grid its extremes are at the four corners. A computed coordinate
    // differs from the exact one by at most E <= 8 M 2^-24 (ex or ey: two roundings; the products, their sum, + xc and
    // - 0.5 one each, every intermediate bounded by M = |xc| + |yc| + bw + bh). The corners are samples too, computed
    // by the same operations, so a computed interior coordinate exceeds the computed corner extremes by less than 2 E,
    // and its floor by at most one pixel when 2 E < 1. Staging requires M < 2^18 (make_window), where 2 E < 2^-2; a
    // particle past that bound (or with a non-finite state) takes the global taps. win_tap clamps every index into the
    // window besides, so no LDS read lands outside it whatever the state holds.
    __device__ __forceinline__ TapRange taps(int n) const {
        float xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float sx, sy;
            at(row((k & 2) ? n - 1 : 0), (k & 1) ? n - 1 : 0, sx, sy);
            xlo = fminf(xlo, sx); xhi = fmaxf(xhi, sx);
            ylo = fminf(ylo, sy); yhi = fmaxf(yhi, sy);
        }
        return {floorf(xlo) - 1.0f, floorf(xhi) + 2.0f, floorf(ylo) - 1.0f, floorf(yhi) + 2.0f};
    }
};

// Particle p's grid of n x n samples over its bw x bh box; `as` is read only by the rotated kind.
template <class Grid>
__device__ __forceinline__ Grid make_grid(float xc, float yc, float bw, float bh, int n, const float* __restrict__ as,
                                          int64_t p) {
    if constexpr (Grid::rotated) return Grid(xc, yc, bw, bh, n, as[p]);
    else return Grid(xc, yc, bw, bh, n);
}

// ---------------- the LDS window ----------------
// The particle's source window (every bilinear tap of its S x S samples, clamped into the zero border as rgba_tap
// does) is copied from the RGBA workspace into LDS once, and the taps read LDS instead of issuing 32 gathered dword
// loads per thread through the vector memory path, which bound the global form. A window larger than CROP_LDS_DW dwords
// (a large template at a large scale, or turned) takes the global taps.
constexpr int CROP_LDS_DW = 10240;   // 40 KiB: four workgroups per CU (0.45-0.49 vs 0.53 ms at 80 KiB and two per CU,
// profiles/r2_gemm_lab/crop_lds_window_ab.txt); windows up to ~101 x 101 (a 64 x 64 template to scale ~1.55 upright)
struct Window {   // taps are clamped into [cx0, cx1] x [cy0, cy1]; staged: that window is in LDS, wx dwords per row
    int cx0, cy0, cx1, cy1, wx;
    bool staged;
};
// The window of a grid's tap range. M = |xc| + |yc| + |bw| + |bh|. Staged only for a finite state of bounded magnitude
// (M < 2^18, false for NaN: every sample coordinate then converts to int in range, and RotGrid::taps' margin holds)
// whose window is at least 1 x 1 and within the budget; workgroup-uniform.
__device__ __forceinline__ Window make_window(const TapRange& t, float M, int H, int W) {
    Window w;
    // the float -> int conversions are taken after the clamp into [-2, W + 1]: no out-of-range conversion
    const float fw = (float)W + 1.0f, fh = (float)H + 1.0f;
    w.cx0 = min(max((int)clamp_f(t.x0, -2.0f, fw), -1), W);
    w.cx1 = min(max((int)clamp_f(t.x1, -2.0f, fw), -1), W);
    w.cy0 = min(max((int)clamp_f(t.y0, -2.0f, fh), -1), H);
    w.cy1 = min(max((int)clamp_f(t.y1, -2.0f, fh), -1), H);
    w.wx = w.cx1 - w.cx0 + 1;
    const int wy = w.cy1 - w.cy0 + 1;
    w.staged = M < 262144.0f && w.wx >= 1 && wy >= 1 && (int64_t)w.wx * wy <= CROP_LDS_DW;
    if (!w.staged) { w.cx0 = w.cy0 = -1; w.cx1 = W; w.cy1 = H; }   // unstaged: the whole bordered frame, rgba_tap's clamp
    return w;
}
// Particle p's grid and window, the window copied into `win` when it is staged; ends with the workgroup's barrier.
template <int NT, class Grid>
__device__ __forceinline__ Grid stage_particle(uint32_t* win, Window& wd, const uint32_t* __restrict__ rgba, int H, int W,
                                               const float* __restrict__ xs, const float* __restrict__ ys,
                                               const float* __restrict__ ss, const float* __restrict__ as, int64_t p,
                                               float w0, float h0, int S) {
    const float xc = xs[p], yc = ys[p], sc = ss[p];
    const float bw = sc * w0, bh = sc * h0;
    const Grid grid = make_grid<Grid>(xc, yc, bw, bh, S, as, p);
    wd = make_window(grid.taps(S), fabsf(xc) + fabsf(yc) + fabsf(bw) + fabsf(bh), H, W);
    if (wd.staged) {
        const int wy = wd.cy1 - wd.cy0 + 1;
        for (int i = threadIdx.x; i < wd.wx * wy; i += NT) {
            const int r = i / wd.wx, c = i - r * wd.wx;
            win[i] = rgba[(int64_t)(wd.cy0 + r + 1) * (W + 2) + (wd.cx0 + c + 1)];
        }
    }
    __syncthreads();
    return grid;
}
// A tap clamps its index into the window: one clamp for both sources. Staged, it reads LDS (for an upright grid every
// tap already lies inside the window; for a rotated one the clamp is the net under the one-pixel margin); unstaged, the
// window is the bordered frame and the read is rgba_tap's.
__device__ __forceinline__ uint32_t win_tap(const Window& wd, const uint32_t* win, const uint32_t* __restrict__ rgba,
                                            int W, int yy, int xx) {
    yy = min(max(yy, wd.cy0), wd.cy1);
    xx = min(max(xx, wd.cx0), wd.cx1);
    if (wd.staged) return win[(yy - wd.cy0) * wd.wx + (xx - wd.cx0)];
    return rgba[(int64_t)(yy + 1) * (W + 2) + (xx + 1)];
}

// ---------------- the im2col stores ----------------
// 8 consecutive columns at a 16-B aligned dst (32-B for fp32).
template <typename OutT>
__device__ __forceinline__ void store8(OutT* dst, const float (&v)[8]) {
    if constexpr (sizeof(OutT) == 2) {
        uint4 pk;
        pk.x = pack_bf2(v[0], v[1]); pk.y = pack_bf2(v[2], v[3]);
        pk.z = pack_bf2(v[4], v[5]); pk.w = pack_bf2(v[6], v[7]);
        *reinterpret_cast<uint4*>(dst) = pk;
    } else {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
}
// Two consecutive columns, the second only if `both` (the last pair of an odd patch repeats a column); bf16 as one
// dword when `pairs` (even patch: 4-B aligned).
template <typename OutT>
__device__ __forceinline__ void store2(OutT* dst, float v0, float v1, bool pairs, bool both) {
    if constexpr (sizeof(OutT) == 2) {
        const uint32_t pk = pack_bf2(v0, v1);
        if (pairs) {
            *reinterpret_cast<uint32_t*>(dst) = pk;
        } else {
            dst[0] = (OutT)(pk & 0xffffu);
            if (both) dst[1] = (OutT)(pk >> 16);
        }
    } else {
        dst[0] = v0;
        if (both) dst[1] = v1;
    }
}

// ---------------- the gather kernels ----------------
// Fast path (patch % 8 == 0, Kp == 3 patch^2), LDS-staged: one 512-thread workgroup per particle; a thread writes 8
// consecutive output pixels of one patch row (ky, kx0..kx0+7) in all three channels, the row's shared part computed
// once, each sample's column once, and one dword tap serving all three channels. Same per-value arithmetic (and order)
// as the generic kernel and the oracle.
template <typename OutT, class Grid>
__global__ __launch_bounds__(512) void k_crop_patches_lds(const uint32_t* __restrict__ rgba, int H, int W,
                                                          const float* __restrict__ xs, const float* __restrict__ ys,
                                                          const float* __restrict__ ss, const float* __restrict__ as,
                                                          int n_patches, int g, float w0, float h0, int S, int patch,
                                                          NormAB nab, OutT* __restrict__ out, int split) {
    __shared__ uint32_t win[CROP_LDS_DW];
    // `split` workgroups per particle (small batches: the 8-GPU share's 512 particles would fill 2 workgroups per CU),
    // each staging the window and writing a contiguous share of the particle's rows
    const int64_t p = blockIdx.x / split;
    const int part = blockIdx.x - (int)(p * split);
    Window wd;
    const Grid grid = stage_particle<512, Grid>(win, wd, rgba, H, W, xs, ys, ss, as, p, w0, h0, S);
    auto tap = [&](int yy, int xx) -> uint32_t { return win_tap(wd, win, rgba, W, yy, xx); };
    const int per_row = patch * (patch >> 3);             // threads per im2col row
    const int pp = patch * patch;
    const int total = n_patches * per_row;
    const int t_end = (int)((int64_t)total * (part + 1) / split);
    for (int t = (int)((int64_t)total * part / split) + threadIdx.x; t < t_end; t += 512) {
        const int pi = t / per_row;
        const int tt = t - pi * per_row;
        const int ky = tt / (patch >> 3), kx0 = (tt - ky * (patch >> 3)) * 8;
        const int py = pi / g, px = pi - (pi / g) * g;
        const typename Grid::Row gr = grid.row(py * patch + ky);
        float vals[3][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v[3];
            grid.sample(tap, gr, px * patch + kx0 + e, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) vals[c][e] = fmaf(v[c], nab.a[c], nab.b[c]);
        }
        const int64_t row = p * n_patches + pi;
#pragma unroll
        for (int c = 0; c < 3; ++c) store8(out + row * (int64_t)(3 * pp) + c * pp + ky * patch + kx0, vals[c]);
    }
}

// Any patch / Kp (ViT-L/14: patch 14, Kp = 640 > 3 x 196), LDS-staged like the fast path: one 512-thread workgroup
// per particle stages its source window, then a thread walks one patch row (ky) of one patch: the row's shared part
// and each sample's column are computed once and one dword tap serves all three channels; bf16 pairs go out as dword
// stores (even patch). The columns past 3 patch^2 are the zero padding. Same per-value arithmetic (and order) as the
// oracle. Round 5: replaces a global-tap form (4.8 ms per ViT-L frame) and a per-element form (4.35 ms) whose index
// and tap work was repeated for every channel.
template <typename OutT, class Grid>
__global__ __launch_bounds__(512) void k_crop_patches_gen(const uint32_t* __restrict__ rgba, int H, int W,
                                                          const float* __restrict__ xs, const float* __restrict__ ys,
                                                          const float* __restrict__ ss, const float* __restrict__ as,
                                                          int n_patches, int g, float w0, float h0, int S, int patch,
                                                          int Kp, NormAB nab, OutT* __restrict__ out) {
    __shared__ uint32_t win[CROP_LDS_DW];
    const int64_t p = blockIdx.x;
    Window wd;
    const Grid grid = stage_particle<512, Grid>(win, wd, rgba, H, W, xs, ys, ss, as, p, w0, h0, S);
    auto tap = [&](int yy, int xx) -> uint32_t { return win_tap(wd, win, rgba, W, yy, xx); };
    const int pp = patch * patch, K = 3 * pp;
    OutT* const base = out + p * n_patches * (int64_t)Kp;
    const bool pairs = sizeof(OutT) == 2 && (patch & 1) == 0;   // 4-B aligned bf16 pairs
    for (int t = threadIdx.x; t < n_patches * patch; t += 512) {
        const int pi = t / patch, ky = t - pi * patch;
        const int py = pi / g, px = pi - py * g;
        const typename Grid::Row gr = grid.row(py * patch + ky);
        OutT* const row = base + (int64_t)pi * Kp + ky * patch;
        for (int kx = 0; kx < patch; kx += 2) {
            float v[2][3];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                grid.sample(tap, gr, px * patch + min(kx + e, patch - 1), v[e]);   // odd patch: the last pair repeats a column
#pragma unroll
                for (int c = 0; c < 3; ++c) v[e][c] = fmaf(v[e][c], nab.a[c], nab.b[c]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) store2(row + c * pp + kx, v[0][c], v[1][c], pairs, kx + 1 < patch);
        }
    }
    const int pad = Kp - K;
    for (int t = threadIdx.x; t < n_patches * pad; t += 512) {
        const int pi = t / pad;
        base[(int64_t)pi * Kp + K + (t - pi * pad)] = (OutT)0;
    }
}

// `angles` null: the upright grid (SPEC S3); otherwise one angle per particle (S12).
template <typename OutT>
static int crop_launch(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles, int64_t ld,
                       const float* angles, int64_t n, float w0, float h0, int S, int patch, int Kp,
                       const float* norm_ab_host, OutT* out, void* stream) {
    if (H <= 0 || W <= 0 || n < 0 || ld < n || patch <= 0 || S <= 0 || S % patch != 0 || Kp % 8 != 0 ||
        Kp < 3 * patch * patch || !norm_ab_host || !frame || !rgba_ws || (n > 0 && (!particles || !out)))
        return VPF_ERR_ARG;
    if ((int64_t)(H + 2) * (W + 2) > INT32_MAX) return VPF_ERR_ARG;
    if (n == 0) return 0;
    NormAB nab;
    for (int c = 0; c < 3; ++c) { nab.a[c] = norm_ab_host[c]; nab.b[c] = norm_ab_host[3 + c]; }
    hipStream_t st = (hipStream_t)stream;
    const bool fast = patch % 8 == 0 && Kp == 3 * patch * patch && n <= INT32_MAX / 4;
    if (!fast && n > INT32_MAX) return VPF_ERR_ARG;
    const int e = fill_rgba_ws(frame, H, W, rgba_ws, st);
    if (e) return e;
    const int g = S / patch;
    if (fast) {
        const int split = n >= 2048 ? 1 : n >= 1024 ? 2 : 4;   // at least ~4096 workgroups when the batch is small
        const auto k = angles ? k_crop_patches_lds<OutT, RotGrid> : k_crop_patches_lds<OutT, UprightGrid>;
        hipLaunchKernelGGL(k, dim3((unsigned)(n * split)), dim3(512), 0, st, rgba_ws, H, W, particles, particles + ld,
                           particles + 2 * ld, angles, g * g, g, w0, h0, S, patch, nab, out, split);
    } else {
        const auto k = angles ? k_crop_patches_gen<OutT, RotGrid> : k_crop_patches_gen<OutT, UprightGrid>;
        hipLaunchKernelGGL(k, dim3((unsigned)n), dim3(512), 0, st, rgba_ws, H, W, particles, particles + ld,
                           particles + 2 * ld, angles, g * g, g, w0, h0, S, patch, Kp, nab, out);
    }
    VPF_RETURN_LAUNCH();
}

VPF_API int vpf_crop_patches_bf16(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                                  int64_t ld, int64_t n, float w0, float h0, int S, int patch, int Kp,
                                  const float* norm_ab_host, uint16_t* out, void* stream) {
    return crop_launch<uint16_t>(frame, H, W, rgba_ws, particles, ld, nullptr, n, w0, h0, S, patch, Kp, norm_ab_host,
                                 out, stream);
}

VPF_API int vpf_crop_patches_f32(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                                 int64_t ld, int64_t n, float w0, float h0, int S, int patch, int Kp,
                                 const float* norm_ab_host, float* out, void* stream) {
    return crop_launch<float>(frame, H, W, rgba_ws, particles, ld, nullptr, n, w0, h0, S, patch, Kp, norm_ab_host, out,
                              stream);
}

// The rotated entry points (SPEC S12) need their angle row.
VPF_API int vpf_crop_patches_rot_bf16(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                                      int64_t ld, const float* angles, int64_t n, float w0, float h0, int S, int patch,
                                      int Kp, const float* norm_ab_host, uint16_t* out, void* stream) {
    return n > 0 && !angles ? VPF_ERR_ARG : crop_launch<uint16_t>(frame, H, W, rgba_ws, particles, ld, angles, n, w0,
                                                                  h0, S, patch, Kp, norm_ab_host, out, stream);
}

VPF_API int vpf_crop_patches_rot_f32(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, const float* particles,
                                     int64_t ld, const float* angles, int64_t n, float w0, float h0, int S, int patch,
                                     int Kp, const float* norm_ab_host, float* out, void* stream) {
    return n > 0 && !angles ? VPF_ERR_ARG : crop_launch<float>(frame, H, W, rgba_ws, particles, ld, angles, n, w0, h0,
                                                               S, patch, Kp, norm_ab_host, out, stream);
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

// ---------------- colour-histogram likelihood (SPEC S13, S14) ----------------
// vpf_color_weight (S13): a second cue per particle. One 256-thread workgroup per particle takes C x C bilinear samples
// of its box (an UprightGrid, or a RotGrid with an angle row; raw 0..255 values, no normalisation), bins each sample's
// (R, G, B) into B^3 bins with LDS atomics, and wave 0 scores the histogram against the template by the Bhattacharyya
// coefficient in S13's pinned order. The counts are integers, so their order of arrival does not matter; for B <= 8
// every wave counts into a histogram of its own (4 x 512 bins), summed after the barrier, which spreads same-address
// atomics over four addresses. Taps are global loads through rgba_tap: the frame is L2-resident and 4 C^2 taps per
// particle do not repay staging a window. A degenerate state follows S3's last paragraph: beyond the int range every
// tap is padding and every sample falls in bin 0.
// vpf_color_weight_surround (S14) adds a cue over the ring around the box; it is a kernel of its own because it needs
// twice the LDS. Both kernels are the helpers below put together.
constexpr int COLOR_NT = 256;
constexpr int COLOR_MAX_BINS = 4096;   // B = 16: 16 KiB of LDS

// The bin of the grid's sample (ox, oy): each channel's value truncated to its top lb bits.
template <class Grid>
__device__ __forceinline__ int sample_bin(const Grid& grid, const uint32_t* __restrict__ rgba, int H, int W, int ox,
                                          int oy, int lb) {
    float v[3];
    grid.sample([&](int yy, int xx) -> uint32_t { return rgba_tap(rgba, H, W, yy, xx); }, grid.row(oy), ox, v);
    int b = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int q = min(max((int)v[c], 0), 255) >> (8 - lb);   // v >= 0 for every finite state; the max keeps b in range
        b = (b << lb) | q;
    }
    return b;
}

// After the counting barrier: the per-wave histograms summed into the first, and the counts stored to out_row if given.
__device__ __forceinline__ void fold_hist(uint32_t* hist, int nb, int nsub, uint32_t* __restrict__ out_row) {
    for (int b = threadIdx.x; b < nb; b += COLOR_NT) {
        uint32_t h = hist[b];
        if (nsub == 4) {
            h += hist[nb + b] + hist[2 * nb + b] + hist[3 * nb + b];
            hist[b] = h;
        }
        if (out_row) out_row[b] = h;
    }
}

// The Bhattacharyya coefficient of hist / den against tmpl, by one whole wave, in SPEC S13's pinned order: lane l sums
// its terms b = l, l + 64, ... in increasing order, then wave_sum's butterfly. The division is one IEEE operation
// (exact when den is a power of two).
__device__ __forceinline__ float bhattacharyya(const uint32_t* hist, float den, const float* __restrict__ tmpl, int nb,
                                               int lane) {
    float acc = 0.0f;
    for (int b = lane; b < nb; b += 64) {
        const float pb = (float)hist[b] / den;
        acc = acc + sqrtf(pb * tmpl[b]);
    }
    return wave_sum(acc);
}

// floor(w 2^K) for the weight w = fixed_expf(lam (min(sim, 1) - 1)) of a similarity derived from the score rho; 0 when
// rho is not finite.
__device__ __forceinline__ uint64_t fixed_weight(float rho, float sim, float lam, double scale) {
    const float w = isfinite(rho) ? fixed_expf(lam * (fminf(sim, 1.0f) - 1.0f)) : 0.0f;
    return (uint64_t)(int64_t)floor((double)w * scale);
}

// (a b) >> sh with the product exact (128 bits), 0 <= sh <= 61.
__device__ __forceinline__ uint64_t mul_shift(uint64_t a, uint64_t b, int sh) {
    const uint64_t hi = __umul64hi(a, b), lo = a * b;
    return sh ? (hi << (64 - sh)) | (lo >> sh) : lo;
}

template <class Grid>
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
    const float sc = ss[p];
    const Grid grid = make_grid<Grid>(xs[p], ys[p], sc * w0, sc * h0, C, as, p);
    for (int t = tid; t < C * C; t += COLOR_NT) {
        const int oy = t / C, ox = t - oy * C;
        atomicAdd(&mine[sample_bin(grid, rgba, H, W, ox, oy, lb)], 1u);
    }
    __syncthreads();
    fold_hist(hist, nb, nsub, hist_out ? hist_out + p * nb : nullptr);
    if (!tmpl) return;                                     // workgroup-uniform
    __syncthreads();
    if (tid >= 64) return;
    const float rho = bhattacharyya(hist, (float)(C * C), tmpl, nb, tid);   // exact: C^2 is a power of two
    if (tid == 0) {
        const uint64_t lc = fixed_weight(rho, rho, lam_c, scale);
        if (rho_out) rho_out[p] = rho;
        Q[p] = (int64_t)(combine ? mul_shift((uint64_t)Q[p], lc, sh) : lc);
    }
}

// What the two colour entry points check alike.
static bool color_args_ok(const uint8_t* frame, int H, int W, const uint32_t* rgba_ws, int fill_ws,
                          const float* particles, int64_t ld, int64_t n, int grid, int bins, float lam_c, int bits) {
    if (H <= 0 || W <= 0 || n < 0 || ld < n || !rgba_ws || (fill_ws && !frame)) return false;
    if ((int64_t)(H + 2) * (W + 2) > INT32_MAX || n > INT32_MAX) return false;
    if (bins != 4 && bins != 8 && bins != 16) return false;
    if (grid != 8 && grid != 16 && grid != 32 && grid != 64) return false;
    if (!(lam_c >= 0.0f) || !(lam_c <= 3.4028234663852886e38f) || bits < 0 || bits > 61) return false;
    return n == 0 || particles;
}

VPF_API int vpf_color_weight(const uint8_t* frame, int H, int W, uint32_t* rgba_ws, int fill_ws,
                             const float* particles, int64_t ld, const float* angles, int64_t n, float w0, float h0,
                             int grid, int bins, const float* tmpl, float lam_c, int bits, int combine,
                             uint32_t* hist_out, float* rho_out, int64_t* Q, void* stream) {
    if (!color_args_ok(frame, H, W, rgba_ws, fill_ws, particles, ld, n, grid, bins, lam_c, bits)) return VPF_ERR_ARG;
    if (tmpl ? !Q : !hist_out) return VPF_ERR_ARG;         // a template needs Q; without one the histograms are the output
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (fill_ws) {
        const int e = fill_rgba_ws(frame, H, W, rgba_ws, st);
        if (e) return e;
    }
    const int lb = bins == 4 ? 2 : bins == 8 ? 3 : 4;
    const double scale = (double)((uint64_t)1 << bits);
    const auto k = angles ? k_color_weight<RotGrid> : k_color_weight<UprightGrid>;
    hipLaunchKernelGGL(k, dim3((unsigned)n), dim3(COLOR_NT), 0, st, rgba_ws, H, W, particles, particles + ld,
                       particles + 2 * ld, angles, w0, h0, grid, lb, tmpl, lam_c, scale, bits, combine, hist_out,
                       rho_out, Q);
    VPF_RETURN_LAUNCH();
}

// ---------------- colour cue with a surround ring (SPEC S14) ----------------
// vpf_color_weight_surround: S13's cue and a second one over the ring around the box, fused in one launch. The ring is
// the box doubled about its centre minus the box: of the C x C samples of the doubled box (the same kind of grid with
// (w0, h0) -> (2 w0, 2 h0); same centre, scale and angle) those with ox or oy outside [C/4, 3C/4), 3 C^2 / 4 of
// them. One 256-thread workgroup per particle walks the C^2 inner and 3 C^2 / 4 ring samples as ONE list (7 C^2 / 4
// items, strided over the threads; C^2 is a multiple of 64, so a wave's items of one pass are all inner or all ring),
// ring samples enumerated directly: two full-width bands of C/4 rows, then the C/2 middle rows' two side pieces.
// Two LDS histograms (inner at 0, ring at COLOR_MAX_BINS; 2 x 16 KiB at B = 16), one pair per wave for B <= 8 as in
// k_color_weight. After the barrier wave 0 scores rho (counts / C^2) and wave 1 rho_s (counts / (3 C^2 / 4), one IEEE
// division) at the same time; lane 0 then forms Lc and Ls = weight(1 - min(rho_s, 1)) and does both exact products on
// Q. A particle with a non-finite state has rho_s = NaN and so Ls = 0.
template <class Grid>
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
    if constexpr (Grid::rotated) fin = fin && isfinite(as[p]);
    // both grids, once: the box (S13's) and the doubled box (2 w0 and 2 h0 are exact)
    const Grid box = make_grid<Grid>(xc, yc, sc * w0, sc * h0, C, as, p);
    const Grid dbl = make_grid<Grid>(xc, yc, sc * (2.0f * w0), sc * (2.0f * h0), C, as, p);
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
        const Grid grid = ring ? dbl : box;                // a select per constant, no indexed array
        atomicAdd(&mine[ring * COLOR_MAX_BINS + sample_bin(grid, rgba, H, W, ox, oy, lb)], 1u);
    }
    __syncthreads();
    fold_hist(hist, nb, nsub, hist_out ? hist_out + p * nb : nullptr);
    fold_hist(hist + COLOR_MAX_BINS, nb, nsub, hist_s_out ? hist_s_out + p * nb : nullptr);
    if (!tmpl) return;                                     // workgroup-uniform
    __syncthreads();
    if (wave < 2) {                                        // wave 0: rho over the box (exact division), wave 1: rho_s over the ring
        const float r = bhattacharyya(hist + wave * COLOR_MAX_BINS, wave ? (float)(3 * Q4) : (float)CC, tmpl, nb, lane);
        if (lane == 0) rho_sh[wave] = r;
    }
    __syncthreads();
    if (tid == 0) {
        const float rho = rho_sh[0];
        const float rho_s = fin ? rho_sh[1] : __builtin_nanf("");
        const uint64_t lc = fixed_weight(rho, rho, lam_c, scale);
        const uint64_t ls = fixed_weight(rho_s, 1.0f - fminf(rho_s, 1.0f), lam_s, scale);
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
    if (!color_args_ok(frame, H, W, rgba_ws, fill_ws, particles, ld, n, grid, bins, lam_c, bits)) return VPF_ERR_ARG;
    if (!(lam_s >= 0.0f) || !(lam_s <= 3.4028234663852886e38f)) return VPF_ERR_ARG;
    if (tmpl ? !Q : !(hist_out || hist_s_out)) return VPF_ERR_ARG;   // without a template the histograms are the output
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (fill_ws) {
        const int e = fill_rgba_ws(frame, H, W, rgba_ws, st);
        if (e) return e;
    }
    const int lb = bins == 4 ? 2 : bins == 8 ? 3 : 4;
    const int lc2 = grid == 8 ? 3 : grid == 16 ? 4 : grid == 32 ? 5 : 6;
    const double scale = (double)((uint64_t)1 << bits);
    const auto k = angles ? k_color_weight_surround<RotGrid> : k_color_weight_surround<UprightGrid>;
    hipLaunchKernelGGL(k, dim3((unsigned)n), dim3(COLOR_NT), 0, st, rgba_ws, H, W, particles, particles + ld,
                       particles + 2 * ld, angles, w0, h0, grid, lc2, lb, tmpl, lam_c, lam_s, scale, bits, combine,
                       hist_out, hist_s_out, rho_out, rho_s_out, Q);
    VPF_RETURN_LAUNCH();
}
