"""The crop (SPEC S3 and its rotated form S12, csrc/crop.hip) restated for tests/test_gpu_crop_exact.py,
tests/test_gpu_crop_rot_exact.py and tests/test_crop_host.py: the LDS window's geometry and staging guard in numpy fp32
(one numpy float32 operation per fp32 operation of the grids' taps() and make_window) for both grids, which kernel form a
shape takes, closed forms of the crop that do not go through the oracle, and a model of the rotated crop's memory reads
(the window as a flat array, win_tap's clamp) with the one-line mutants that the rotated cases must tell apart."""
import numpy as np

import s11_reference as R11
import s12_reference as R12

f32 = np.float32
CROP_LDS_DW = 10240          # csrc/crop.hip's LDS window budget, in dwords (one per pixel)
M_BOUND = f32(262144.0)      # 2^18: the staging guard's bound on |xc| + |yc| + |bw| + |bh|


def kernel_form(patch: int, kp: int) -> str:
    """crop_launch's choice: the 8-pixel form with 16-B stores, or the per-row form."""
    return "lds8" if patch % 8 == 0 and kp == 3 * patch * patch else "row"


def split_of(n: int) -> int:
    """Workgroups per particle of the 8-pixel form."""
    return 1 if n >= 2048 else 2 if n >= 1024 else 4


def window(particles, box_wh, S: int, H: int, W: int) -> dict:
    """stage_window's geometry per particle of float32[3][n]: the unclamped tap range (ix_lo, ix_hi, iy_lo, iy_hi, as
    floats: they may be far out of the int range, or NaN), the window clamped into the zero border (cx0, cx1, cy0,
    cy1), its sides wx, wy, its area px (int64) and `staged`, the branch the workgroup takes."""
    p = np.asarray(particles, np.float32)
    xc, yc, sc = p[0], p[1], p[2]
    half, one = f32(0.5), f32(1.0)
    last = f32(S - 1) + half
    with np.errstate(all="ignore"):
        bw, bh = sc * f32(box_wh[0]), sc * f32(box_wh[1])
        x0, y0 = xc - half * bw, yc - half * bh
        dx, dy = bw / f32(S), bh / f32(S)
        sxa, sxb = (x0 + half * dx) - half, (x0 + last * dx) - half
        sya, syb = (y0 + half * dy) - half, (y0 + last * dy) - half
        ix_lo, ix_hi = np.floor(np.fmin(sxa, sxb)), np.floor(np.fmax(sxa, sxb)) + one
        iy_lo, iy_hi = np.floor(np.fmin(sya, syb)), np.floor(np.fmax(sya, syb)) + one
        m = np.abs(xc) + np.abs(yc) + np.abs(bw) + np.abs(bh)
        bounded = m < M_BOUND                                       # False for NaN
    assert all(v.dtype == np.float32 for v in (ix_lo, ix_hi, iy_lo, iy_hi, m))

    def clamp(v, hi):
        """(int)clamp_f(v, -2, hi + 1), then into [-1, hi]: fminf(fmaxf(v, lo), hi) sends a NaN to lo."""
        c = np.fmin(np.fmax(v, f32(-2.0)), f32(hi) + one)
        return np.clip(c.astype(np.int64), -1, hi)

    cx0, cx1, cy0, cy1 = clamp(ix_lo, W), clamp(ix_hi, W), clamp(iy_lo, H), clamp(iy_hi, H)
    wx, wy = cx1 - cx0 + 1, cy1 - cy0 + 1
    px = wx * wy
    staged = bounded & (wx >= 1) & (wy >= 1) & (px <= CROP_LDS_DW)
    return dict(ix_lo=ix_lo, ix_hi=ix_hi, iy_lo=iy_lo, iy_hi=iy_hi, cx0=cx0, cx1=cx1, cy0=cy0, cy1=cy1, wx=wx, wy=wy,
                px=px, staged=staged)


def sample_floors(particles, box_wh, S: int):
    """floor(sx) int64[n][S] and floor(sy) int64[n][S] of every sample of finite in-range states, S3's operations."""
    p = np.asarray(particles, np.float32)
    xc, yc, sc = (p[k].reshape(-1, 1) for k in range(3))
    half = f32(0.5)
    bw, bh = sc * f32(box_wh[0]), sc * f32(box_wh[1])
    x0, y0 = xc - half * bw, yc - half * bh
    dx, dy = bw / f32(S), bh / f32(S)
    o = (np.arange(S, dtype=np.float32) + half).reshape(1, S)
    sx, sy = (x0 + o * dx) - half, (y0 + o * dy) - half
    assert sx.dtype == np.float32
    return np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)


# ---------------------------------------------------------------------------------------------- the rotated window
def _clamp_into_border(v, hi):
    """make_window's (int)clamp_f(v, -2, hi + 1), then into [-1, hi]: fminf(fmaxf(v, lo), hi) sends a NaN to lo."""
    c = np.fmin(np.fmax(v, f32(-2.0)), f32(hi) + f32(1.0))
    return np.clip(c.astype(np.int64), -1, hi)


def rot_corners(particles, angles, box_wh, S: int, coords=None):
    """RotGrid::taps' four corner samples, (sx, sy) float32[n][4] in the order (0, 0), (0, S-1), (S-1, 0), (S-1, S-1)
    of (oy, ox): s12_reference.sample_coords at the indices 0 and S - 1 (`coords`: that call's result, if the caller
    has it). A non-finite angle has c = s = NaN (u - floorf(u) is NaN for NaN and for +-inf), so every coordinate is
    NaN: the oracle's C routine is not called with it, its (int) conversion is not defined there."""
    a = np.asarray(angles, np.float32).reshape(-1)
    fin = np.isfinite(a)
    if coords is None:
        with np.errstate(all="ignore"):
            coords = R12.sample_coords(particles, np.where(fin, a, f32(0.0)).astype(np.float32), box_wh, S)
    oy, ox = [0, 0, -1, -1], [0, -1, 0, -1]
    cx, cy = coords[0][:, oy, ox].copy(), coords[1][:, oy, ox].copy()
    cx[~fin], cy[~fin] = np.nan, np.nan
    return cx, cy


def rot_window(particles, angles, box_wh, S: int, H: int, W: int, coords=None, corners=(0, 1, 2, 3)) -> dict:
    """RotGrid::taps + make_window per particle of float32[3][n] with angles float32[n]: window()'s dict. The tap range
    is the bounding box of the corner samples' floors widened by one pixel: (ix_lo, ix_hi) = (floor(min) - 1,
    floor(max) + 2), the min and max folded with fminf / fmaxf from +inf / -inf as the kernel does, so a particle
    whose corners are all NaN (a NaN state or a non-finite angle) keeps the seeds: ix_lo = +inf, ix_hi = -inf, which
    clamp to cx0 = W and cx1 = -1, a window of side -W that the guard's `wx >= 1` refuses. The geometry is the one
    before make_window resets an unstaged window to the whole bordered frame. `corners`: which of the four corners
    bound the box (all, in the kernel)."""
    p = np.asarray(particles, np.float32)
    xc, yc, sc = p[0], p[1], p[2]
    cx, cy = rot_corners(p, angles, box_wh, S, coords)
    n = p.shape[1]
    xlo, xhi = np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)
    ylo, yhi = xlo.copy(), xhi.copy()
    for k in corners:
        xlo, xhi = np.fmin(xlo, cx[:, k]), np.fmax(xhi, cx[:, k])
        ylo, yhi = np.fmin(ylo, cy[:, k]), np.fmax(yhi, cy[:, k])
    with np.errstate(all="ignore"):
        ix_lo, ix_hi = np.floor(xlo) - f32(1.0), np.floor(xhi) + f32(2.0)
        iy_lo, iy_hi = np.floor(ylo) - f32(1.0), np.floor(yhi) + f32(2.0)
        bw, bh = sc * f32(box_wh[0]), sc * f32(box_wh[1])
        m = np.abs(xc) + np.abs(yc) + np.abs(bw) + np.abs(bh)
        bounded = m < M_BOUND                                       # False for NaN
    assert all(v.dtype == np.float32 for v in (ix_lo, ix_hi, iy_lo, iy_hi, m))
    cx0, cx1 = _clamp_into_border(ix_lo, W), _clamp_into_border(ix_hi, W)
    cy0, cy1 = _clamp_into_border(iy_lo, H), _clamp_into_border(iy_hi, H)
    wx, wy = cx1 - cx0 + 1, cy1 - cy0 + 1
    px = wx * wy
    staged = bounded & (wx >= 1) & (wy >= 1) & (px <= CROP_LDS_DW)
    return dict(ix_lo=ix_lo, ix_hi=ix_hi, iy_lo=iy_lo, iy_hi=iy_hi, cx0=cx0, cx1=cx1, cy0=cy0, cy1=cy1, wx=wx, wy=wy,
                px=px, staged=staged, m=m)


def rot_sample_floors(particles, angles, box_wh, S: int, coords=None):
    """floor(sx) and floor(sy), int64[n][S * S] each, of every sample of finite in-range states (S12's operations)."""
    sx, sy = R12.sample_coords(particles, angles, box_wh, S) if coords is None else coords
    n = sx.shape[0]
    return np.floor(sx).reshape(n, -1).astype(np.int64), np.floor(sy).reshape(n, -1).astype(np.int64)


# ---------------------------------------------------------------------------------------------- the rotated crop, modelled
# What vpf_crop_patches_rot_* reads, for finite in-range states: S12's coordinates, the window of rot_window as a flat
# array (the LDS copy when staged, the bordered workspace otherwise), win_tap's clamp, S3's arithmetic. Without a
# mutant it must equal s12_reference.crop_raw bit for bit: the clamp into the window changes no tap (tests/
# test_crop_host.py). Each mutant is one line of it changed; a GPU case that claims to exercise a path is shown there to
# tell the mutants of that path from the real thing.
MUTANTS = {
    1: "s -> -s",
    2: "ex and ey swapped",
    3: "the half box subtracted from the centre (as S3 does), not from the offset",
    4: "floorf omitted from the angle reduction",
    5: "the window bounded by the corners (0, 0) and (S-1, S-1) only",
    6: "the second tap's index formed as clamp(i) + 1, not clamp(i + 1)",
}
GARBAGE = 255.0      # what the model reads past the end of the window's array


def sincos2pi_any(u):
    """fixed_sincos2pi (csrc/vpf_common.h, oracle/pf_oracle.c) restated for any finite u, each line one fp32 operation;
    the quadrant's (int) conversion saturates as the device's does. Equals the oracle's routine on [0, 1]."""
    u = f32(u)
    t = u * f32(4.0)
    q = np.floor(t)
    r = t - q
    a = (r - f32(0.5)) * f32(1.57079632679489662)
    z = a * a
    sp = R11.fmaf(R11.fmaf(f32(-1.9515295891e-4), z, f32(8.3321608736e-3)), z, f32(-1.6666654611e-1))
    sa = R11.fmaf(a * z, sp, a)
    cp = R11.fmaf(R11.fmaf(f32(2.443315711809948e-5), z, f32(-1.388731625493765e-3)), z, f32(4.166664568298827e-2))
    ca = R11.fmaf(z * z, cp, R11.fmaf(z, f32(-0.5), f32(1.0)))
    h = f32(0.70710678118654752)
    c0, s0 = (ca - sa) * h, (ca + sa) * h
    qi = int(min(max(float(q), -2.0 ** 31), 2.0 ** 31 - 1)) & 3
    return [(c0, s0), (-s0, c0), (-c0, -s0), (s0, -c0)][qi]


def _angle_cs(a, mutant):
    u = f32(a) * R12.INV_2PI
    if mutant == 4:
        return sincos2pi_any(u)
    return R12.sincos_angle(a)


def rot_coords_model(particles, angles, box_wh, S: int, mutant=None):
    """s12_reference.sample_coords restated with the coordinate mutants 1-4."""
    p = np.asarray(particles, np.float32)
    n = p.shape[1]
    cs = np.array([_angle_cs(a, mutant) for a in np.asarray(angles, np.float32).reshape(-1)], np.float32).reshape(n, 2)
    c, s = cs[:, 0].reshape(n, 1, 1), cs[:, 1].reshape(n, 1, 1)
    if mutant == 1:
        s = -s
    xc, yc, sc = (p[k].reshape(n, 1, 1) for k in range(3))
    half = f32(0.5)
    bw, bh = sc * f32(box_wh[0]), sc * f32(box_wh[1])
    dx, dy = bw / f32(S), bh / f32(S)
    o = np.arange(S, dtype=np.float32) + half
    if mutant == 3:
        ex, ey = o.reshape(1, 1, S) * dx, o.reshape(1, S, 1) * dy
        xc, yc = xc - half * bw, yc - half * bh
    else:
        ex, ey = o.reshape(1, 1, S) * dx - half * bw, o.reshape(1, S, 1) * dy - half * bh
    if mutant == 2:
        ex, ey = ey, ex
    rx = c * ex - s * ey
    ry = s * ex + c * ey
    sx, sy = (xc + rx) - half, (yc + ry) - half
    assert sx.dtype == np.float32 and sy.dtype == np.float32
    return np.broadcast_to(sx, (n, S, S)), np.broadcast_to(sy, (n, S, S))


def rot_crop_model(frame, particles, angles, box_wh, S: int, mutant=None) -> np.ndarray:
    """The rotated crops of finite in-range states before normalisation, float32[n][S][S][3], read as the kernel reads
    them (see above)."""
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    H, W, _ = frame.shape
    n = np.asarray(particles).shape[1]
    sx, sy = rot_coords_model(particles, angles, box_wh, S, mutant)
    # the kernel's window is its own grid's: a coordinate mutant moves its window along
    w = rot_window(particles, angles, box_wh, S, H, W, coords=(sx, sy), corners=(0, 3) if mutant == 5 else (0, 1, 2, 3))
    st = w["staged"].reshape(n, 1, 1)
    cx0, cx1 = np.where(st, w["cx0"].reshape(n, 1, 1), -1), np.where(st, w["cx1"].reshape(n, 1, 1), W)
    cy0, cy1 = np.where(st, w["cy0"].reshape(n, 1, 1), -1), np.where(st, w["cy1"].reshape(n, 1, 1), H)
    wx, wy = cx1 - cx0 + 1, cy1 - cy0 + 1
    pad = np.zeros((H + 2, W + 2, 3), np.float32)
    pad[1:-1, 1:-1] = frame
    fx0, fy0 = np.floor(sx), np.floor(sy)
    fx, fy = (sx - fx0)[..., None], (sy - fy0)[..., None]
    ix, iy = fx0.astype(np.int64), fy0.astype(np.int64)

    def second(i, lo, hi):
        return np.clip(i, lo, hi) + 1 if mutant == 6 else np.clip(i + 1, lo, hi)

    def tap(yy, xx):
        """The window as a flat array of wx * wy dwords: element (yy - cy0) * wx + (xx - cx0), GARBAGE past its end."""
        flat = (yy - cy0) * wx + (xx - cx0)
        inside = (flat >= 0) & (flat < wx * wy)
        flat = np.where(inside, flat, 0)
        v = pad[cy0 + flat // wx + 1, cx0 + flat % wx + 1]
        return np.where(inside[..., None], v, f32(GARBAGE))

    x_a, x_b = np.clip(ix, cx0, cx1), second(ix, cx0, cx1)
    y_a, y_b = np.clip(iy, cy0, cy1), second(iy, cy0, cy1)
    one = f32(1.0)
    top = (one - fx) * tap(y_a, x_a) + fx * tap(y_a, x_b)
    bot = (one - fx) * tap(y_b, x_a) + fx * tap(y_b, x_b)
    v = (one - fy) * top + fy * bot
    assert v.dtype == np.float32
    return v


def im2col(v: np.ndarray, patch: int, kp: int) -> np.ndarray:
    """Crops [n][S(oy)][S(ox)][3] -> S3's patch matrix [n * g*g][kp], the columns past 3 patch^2 zero."""
    n, S = v.shape[0], v.shape[1]
    g = S // patch
    m = v.reshape(n, g, patch, g, patch, 3).transpose(0, 1, 3, 5, 2, 4).reshape(n * g * g, 3 * patch * patch)
    out = np.zeros((n * g * g, kp), v.dtype)
    out[:, : 3 * patch * patch] = m
    return out


def where(row: int, col: int, S: int, patch: int) -> str:
    """Names the cell (row, col) of a patch matrix for a failure message."""
    g2, pp = (S // patch) ** 2, patch * patch
    if col >= 3 * pp:
        return f"particle {row // g2} patch {row % g2} padding column {col}"
    c, r = divmod(col, pp)
    return f"particle {row // g2} patch {row % g2} channel {c} ky {r // patch} kx {r % patch}"


# ---------------------------------------------------------------------------------------------- closed forms
def position_frame(H: int, W: int) -> np.ndarray:
    """A frame whose bytes encode the position: r = x mod 256, g = y mod 256, b = (x + 3 y) mod 256."""
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([x % 256, y % 256, (x + 3 * y) % 256], axis=-1).astype(np.uint8)


def norm_a(std) -> np.ndarray:
    """SPEC S3's a_c. With mean 0, b_c = -0 and out_c = fmaf(v, a_c, -0) = fp32(v a_c): ONE rounding."""
    inv255 = f32(1.0) / f32(255.0)
    return np.array([f32(inv255 * (f32(1.0) / f32(s))) for s in std], np.float32)


def _pixels(frame: np.ndarray, yy: np.ndarray, xx: np.ndarray) -> np.ndarray:
    """frame[yy][xx] as float64[len(yy)][len(xx)][3], zero outside the frame."""
    H, W, _ = frame.shape
    pad = np.zeros((H + 2, W + 2, 3), np.float64)
    pad[1:-1, 1:-1] = frame
    return pad[np.clip(yy, -1, H)[:, None] + 1, np.clip(xx, -1, W)[None, :] + 1]


CLOSED_CASES = ("identity", "half_x", "half_y", "mean4", "flip")


def closed_case(frame: np.ndarray, case: str, xo: int, yo: int, S: int):
    """One particle (x, y, s) for the box (S, S), and its crop in raw 0..255 units as float64[S][S][3], from integer
    arithmetic on the frame alone. (xo, yo) is the integer pixel of the crop's first sample; every coordinate, weight
    and product below is exact in fp32 (halves and quarters of integers below 2^10), so the kernel's v must equal it.
      identity  s = 1: dx = 1, the samples sit on the pixels            v = frame[yo + oy][xo + ox]
      half_x    the same, x + 0.5: fx = 0.5                             v = mean of the pixel and its right neighbour
      half_y    the same, y + 0.5: fy = 0.5                             v = mean of the pixel and the one below
      mean4     s = 2 (a 2S box): dx = 2, fx = fy = 0.5                 v = mean of the 2 x 2 block at (yo + 2 oy, xo + 2 ox)
      flip      s = -1: dx = -1, x0 = x + S/2                           v = the identity crop flipped in both axes"""
    o = np.arange(S)
    h = S / 2.0
    if case == "identity":
        return (xo + h, yo + h, 1.0), _pixels(frame, yo + o, xo + o)
    if case == "half_x":
        return (xo + h + 0.5, yo + h, 1.0), 0.5 * (_pixels(frame, yo + o, xo + o) + _pixels(frame, yo + o, xo + o + 1))
    if case == "half_y":
        return (xo + h, yo + h + 0.5, 1.0), 0.5 * (_pixels(frame, yo + o, xo + o) + _pixels(frame, yo + o + 1, xo + o))
    if case == "mean4":
        yy, xx = yo + 2 * o, xo + 2 * o
        v = 0.25 * (_pixels(frame, yy, xx) + _pixels(frame, yy, xx + 1) + _pixels(frame, yy + 1, xx)
                    + _pixels(frame, yy + 1, xx + 1))
        return (xo + float(S), yo + float(S), 2.0), v
    if case == "flip":
        return (xo + h, yo + h, -1.0), _pixels(frame, yo + o, xo + o)[::-1, ::-1]
    raise ValueError(case)


def closed_forms(frame: np.ndarray, S: int, patch: int, kp: int, std, origins):
    """Every case of CLOSED_CASES at every (xo, yo) of `origins`: particles float32[3][n] and the expected patch matrix
    float32[n * g*g][kp] for mean 0 and the box (S, S): fp32(v a_c), the single rounding of the exact fp64 product."""
    parts, crops = [], []
    for xo, yo in origins:
        for case in CLOSED_CASES:
            p, v = closed_case(frame, case, xo, yo, S)
            parts.append(p)
            crops.append(v)
    a = norm_a(std).astype(np.float64)
    v = np.stack(crops) * a.reshape(1, 1, 1, 3)          # exact in fp64: 12 bits x 24 bits
    return np.array(parts, np.float32).T.copy(), im2col(v.astype(np.float32), patch, kp)
