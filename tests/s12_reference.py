"""SPEC S12 (rotated particle boxes) restated in numpy: the reference of tests/test_s12_*.py. Every fp32 operation is
one numpy float32 operation (one rounding each). The angle predict is scalar code over s11_reference's pieces (libm's
single-rounding fmaf, the oracle's fixed ln / sincos and Philox). The crop is vectorised over particles and samples; its
one fused operation, the normalisation fmaf(v, a_c, b_c), is `fmaf_vec`: the exact fp64 product, an error-free fp64 sum
and a round-to-odd fix-up before the single rounding to fp32 (tests/test_s12_host.py checks it against libm's fmaf).
sincos is the oracle's fixed routine. Everything S12 does not change is reused: s10_reference.step for the ancestors,
oracle.pf.predict (S2) and s11_reference.predict_cv (S11) for the other rows."""
import ctypes
import math

import numpy as np

import s10_reference as R10
import s11_reference as R11
from oracle import pf as opf

f32 = np.float32
INV_2PI = f32(0.15915494309189535)
CROP_LDS_DW = 10240     # csrc/crop.hip's LDS window budget, in pixels


# ---------------------------------------------------------------------------------------------- predict
def angle_noise(gi: int, frame: int, seed: int) -> np.float32:
    """n5 = sqrt(-2 ln u(g0)) cos(2 pi u(g1)) from words g0, g1 of Philox counter (gi, frame, 0, 2)."""
    seed &= (1 << 64) - 1
    g = opf.philox4x32_10((gi, frame, 0, 2), (seed & 0xFFFFFFFF, seed >> 32))
    return R11.gauss_pair(g[0], g[1])[0]


def predict_angle(a: np.ndarray, global_begin: int, seed: int, frame: int, sig_a, amin, amax) -> None:
    """SPEC S12 predict, in place on the angle row float32[n]: a' = clamp(fmaf(sig_a, n5, a), amin, amax)."""
    assert a.dtype == np.float32 and a.ndim == 1
    for i in range(a.shape[0]):
        a[i] = R11.clampf(R11.fmaf(f32(sig_a), angle_noise(global_begin + i, frame, seed), a[i]), amin, amax)


# ---------------------------------------------------------------------------------------------- crop
def fmaf_vec(a, b, c) -> np.ndarray:
    """fp32 a * b + c with ONE rounding, elementwise (finite fp32 inputs). p = a * b is exact in fp64 (48 bits);
    s = RN64(p + c) with its exact error e by two-sum; where e != 0 the fp64 sum is moved to the neighbouring odd
    significand (round to odd), after which the rounding to fp32 (29 bits fewer) is the rounding of the exact value."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (e != 0.0) & ((bits & 1) == 0)
    away = (e > 0.0) == (s > 0.0)               # the exact value lies farther from zero than s
    bits[fix & away] += 1
    bits[fix & ~away] -= 1
    return bits.view(np.float64).astype(np.float32)


def sincos_angle(a):
    """(c, s) = fixed_sincos2pi(u), u = a * fp32(1 / 2 pi), u <- u - floor(u)."""
    u = f32(f32(a) * INV_2PI)
    u = f32(u - np.floor(u))
    c, s = ctypes.c_float(), ctypes.c_float()
    opf.lib().orc_sincos2pi(float(u), ctypes.byref(c), ctypes.byref(s))
    return f32(c.value), f32(s.value)


def sample_coords(particles: np.ndarray, angles: np.ndarray, box_wh, S: int):
    """SPEC S12's sample coordinates (sx, sy), float32[n][S(oy)][S(ox)] each, of particles float32[3][n] with angles
    float32[n]."""
    particles = np.asarray(particles, np.float32)
    n = particles.shape[1]
    cs = np.array([sincos_angle(a) for a in np.asarray(angles, np.float32).reshape(-1)], np.float32).reshape(n, 2)
    c, s = cs[:, 0].reshape(n, 1, 1), cs[:, 1].reshape(n, 1, 1)
    xc, yc, sc = (particles[k].reshape(n, 1, 1) for k in range(3))
    bw, bh = sc * f32(box_wh[0]), sc * f32(box_wh[1])
    dx, dy = bw / f32(S), bh / f32(S)
    o = np.arange(S, dtype=np.float32) + f32(0.5)
    ex = o.reshape(1, 1, S) * dx - f32(0.5) * bw
    ey = o.reshape(1, S, 1) * dy - f32(0.5) * bh
    rx = c * ex - s * ey
    ry = s * ex + c * ey
    sx = (xc + rx) - f32(0.5)
    sy = (yc + ry) - f32(0.5)
    assert sx.dtype == np.float32 and sy.dtype == np.float32
    return sx, sy


def s3_coords(particles: np.ndarray, box_wh, S: int):
    """SPEC S3's (unrotated) sample coordinates, as oracle/pf_oracle.c computes them: sx float32[n][1][S],
    sy float32[n][S][1]."""
    particles = np.asarray(particles, np.float32)
    n = particles.shape[1]
    xc, yc, sc = (particles[k].reshape(n, 1, 1) for k in range(3))
    bw, bh = sc * f32(box_wh[0]), sc * f32(box_wh[1])
    x0, y0 = xc - f32(0.5) * bw, yc - f32(0.5) * bh
    dx, dy = bw / f32(S), bh / f32(S)
    o = np.arange(S, dtype=np.float32) + f32(0.5)
    return (x0 + o.reshape(1, 1, S) * dx) - f32(0.5), (y0 + o.reshape(1, S, 1) * dy) - f32(0.5)


def bilinear(frame: np.ndarray, sx: np.ndarray, sy: np.ndarray) -> np.ndarray:
    """SPEC S3 from ix = floor(sx) on: the bilinear value in raw 0-255 units, float32[..., 3], zero outside the frame."""
    H, W, _ = frame.shape
    pad = np.zeros((H + 2, W + 2, 3), np.float32)
    pad[1:-1, 1:-1] = frame
    fx0, fy0 = np.floor(sx), np.floor(sy)
    fx, fy = (sx - fx0)[..., None], (sy - fy0)[..., None]
    ix, iy = fx0.astype(np.int64), fy0.astype(np.int64)

    def tap(yy, xx):
        return pad[np.clip(yy, -1, H) + 1, np.clip(xx, -1, W) + 1]

    one = f32(1.0)
    top = (one - fx) * tap(iy, ix) + fx * tap(iy, ix + 1)
    bot = (one - fx) * tap(iy + 1, ix) + fx * tap(iy + 1, ix + 1)
    v = (one - fy) * top + fy * bot
    assert v.dtype == np.float32
    return v


def crop_raw(frame, particles, angles, box_wh, S: int) -> np.ndarray:
    """The rotated crops before normalisation: float32[n][S][S][3] in raw 0-255 units."""
    sx, sy = sample_coords(particles, angles, box_wh, S)
    return bilinear(np.ascontiguousarray(frame, dtype=np.uint8), sx, sy)


def crop_patches_rot(frame, particles, angles, box_wh, S: int, patch: int, kp: int, mean, std) -> np.ndarray:
    """SPEC S12 crop + S3 normalise + im2col: float32[n * g*g][kp], columns past 3 patch^2 zero."""
    v = crop_raw(frame, particles, angles, box_wh, S)
    a, b = opf.norm_affine(mean, std)
    v = fmaf_vec(v, a.reshape(1, 1, 1, 3), b.reshape(1, 1, 1, 3))
    n, g = v.shape[0], S // patch
    v = v.reshape(n, g, patch, g, patch, 3).transpose(0, 1, 3, 5, 2, 4).reshape(n * g * g, 3 * patch * patch)
    out = np.zeros((n * g * g, kp), np.float32)
    out[:, : 3 * patch * patch] = v
    return out


def tap_bbox_pixels(particles, angles, box_wh, S: int, H: int, W: int) -> np.ndarray:
    """Per particle: the pixel count of the bounding box of every bilinear tap of its samples, clipped into the frame's
    zero border ([-1, W] x [-1, H]). The kernel's staged window contains it, so a count above CROP_LDS_DW means the
    particle takes the global-tap branch."""
    sx, sy = sample_coords(particles, angles, box_wh, S)
    n = sx.shape[0]
    fx, fy = np.floor(sx).reshape(n, -1).astype(np.int64), np.floor(sy).reshape(n, -1).astype(np.int64)
    wx = np.clip(fx.max(1) + 1, -1, W) - np.clip(fx.min(1), -1, W) + 1
    wy = np.clip(fy.max(1) + 1, -1, H) - np.clip(fy.min(1), -1, H) + 1
    return wx * wy


def bf16_rne(x: np.ndarray) -> np.ndarray:
    """The bf16 bit patterns (uint16) of finite fp32 values, round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ---------------------------------------------------------------------------------------------- the recursion
def step(Q, state: np.ndarray, seed: int, frame: int, method: str, tau, K: int) -> dict:
    """One frame's estimate + (gated) resample of the posterior weights Q over float32[rows][P], rows = 4 or 6:
    s10_reference.step on rows 0-2, every row gathered by its ancestors, and the extra rows' sums over the same weights
    (every weight 1 when T == 0); the angle is the last row."""
    r = R10.step(Q, state[:3], seed, frame, method, tau, K)
    w = [int(q) for q in Q] if r["T"] else [1] * len(Q)
    r["xsums"] = [math.fsum(float(q) * float(v) for q, v in zip(w, state[c])) for c in range(3, state.shape[0])]
    r["state"] = np.ascontiguousarray(state[:, r["anc"]])
    return r


def extras(r: dict, P: int):
    """The extra rows' estimates (vx, vy under constant velocity, then the angle)."""
    d = float(r["T"]) if r["T"] else float(P)
    return tuple(s / d for s in r["xsums"])


def rotation(r: dict, P: int) -> float:
    return extras(r, P)[-1]


class Filter:
    """The S12 recursion of one target: predict (S2, or S11 with `cv` = (velocity_std, decay, vmax)), predict_angle,
    posterior = carry x likelihood (S10; the identity carry without a gate), step. `init_state`: every row, in order."""

    def __init__(self, P, init_state, motion_std, scale_range, seed, frame_size, K, rotation_std, rotation_range,
                 cv=None, method=R10.SYSTEMATIC, tau=None):
        self.P, self.K, self.method, self.tau, self.seed = P, K, method, tau, seed
        self.motion_std, self.scale_range, self.cv = motion_std, scale_range, cv
        self.rotation_std, self.rotation_range = rotation_std, rotation_range
        self.height, self.width = frame_size
        rows = 6 if cv else 4
        assert len(init_state) == rows
        self.state = np.zeros((rows, P), np.float32)
        for c, v in enumerate(init_state):
            self.state[c] = v
        self.carry = [R10.identity(K)] * P
        self.frame = 0

    def predict(self, frame=None):
        self.frame = self.frame + 1 if frame is None else frame
        if self.cv:
            head = np.ascontiguousarray(self.state[:5])
            R11.predict_cv(head, 0, self.seed, self.frame, self.motion_std, self.cv[0], self.cv[1], self.cv[2],
                           self.width, self.height, self.scale_range)
        else:
            head = np.ascontiguousarray(self.state[:3])
            opf.predict(head, 0, self.seed, self.frame, self.motion_std, self.width, self.height, self.scale_range)
        self.state[: head.shape[0]] = head
        predict_angle(self.state[-1], 0, self.seed, self.frame, self.rotation_std, *self.rotation_range)

    def update(self, L) -> dict:
        r = step(R10.weight_prior(L, self.carry, self.K), self.state, self.seed, self.frame, self.method, self.tau,
                 self.K)
        self.state = r["state"]
        self.carry = [int(c) for c in r["carry"]]
        return r


# ---------------------------------------------------------------------------------------------- the convergence check
# A deterministic recursion with no ViT, shared by the CPU and GPU tests: from a = 0 with sigma_a = 0.1, the likelihood
# L_i = floor(2^40 exp(-(a_i - 0.6)^2 / (2 0.05^2))) for 12 frames. The seed was chosen on the CPU: the angle estimate
# ends 0.003 rad from 0.6.
CONV_SEED, CONV_P = 321, 300
CONV = dict(init=(100.0, 90.0, 1.0, 0.0), motion_std=(3.0, 2.0, 0.03), scale_range=(0.6, 1.8), frame_size=(224, 224),
            K=40, rotation_std=0.1, rotation_range=(-math.pi / 2, math.pi / 2))


def conv_likelihood(a: np.ndarray) -> np.ndarray:
    d = a.astype(np.float64) - 0.6
    return np.floor(2.0 ** 40 * np.exp(-(d * d) / (2 * 0.05 ** 2))).astype(np.int64)


def run_convergence(seed, frames=12):
    """The angle estimates of the reference recursion, one per frame."""
    ref = Filter(CONV_P, CONV["init"], CONV["motion_std"], CONV["scale_range"], seed, CONV["frame_size"], CONV["K"],
                 CONV["rotation_std"], CONV["rotation_range"])
    est = []
    for _ in range(frames):
        ref.predict()
        r = ref.update(conv_likelihood(ref.state[-1]))
        est.append(rotation(r, CONV_P))
    return est
