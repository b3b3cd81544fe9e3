"""The unrotated crop (SPEC S3, csrc/crop.hip) restated for tests/test_gpu_crop_exact.py and tests/test_crop_host.py:
the LDS window's geometry and staging guard in numpy fp32 (one numpy float32 operation per fp32 operation of
stage_window), which kernel form a shape takes, and closed forms of the crop that do not go through the oracle."""
import numpy as np

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
