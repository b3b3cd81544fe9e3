"""SPEC S11 (constant-velocity motion model) restated in Python: the reference of tests/test_s11_*.py. Every fp32
operation is one numpy float32 operation (one rounding each); the fmaf is a true single-rounding one (math.fma where
this Python has it, else libm's fmaf); ln, sincos and exp are the oracle's fixed fp32 routines and Philox the oracle's.
The position noise is computed here from the Philox words, not taken from oracle.pf.predict, so that the identity with
S2 (sigma_v = 0, d = 1, zero velocities) is a check of this file and not a tautology. The resample and the estimate
reuse s10_reference.step for the ancestors and gather five rows by them; the velocity sums are math.fsum."""
import ctypes
import ctypes.util
import math

import numpy as np

import s10_reference as R10
from oracle import pf as opf

f32 = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.argtypes = [ctypes.c_float] * 3
_libm.fmaf.restype = ctypes.c_float


def fmaf(a, b, c) -> np.float32:
    """fp32 a * b + c with ONE rounding: libm's fmaf on every Python. (math.fma, where it exists, is the fp64 fma: its
    result rounded to fp32 afterwards is rounded twice, which is what this reference must not do.)"""
    return f32(_libm.fmaf(float(a), float(b), float(c)))


def uniform01(r: int) -> np.float32:
    """SPEC S2: (2 (r >> 9) + 1) 2^-24, in (0, 1); both factors and the product are exact in fp32."""
    return f32(2 * (int(r) >> 9) + 1) * f32(2.0 ** -24)


def gauss_pair(w0: int, w1: int):
    """Box-Muller on two Philox words: rad = sqrt(-2 ln u(w0)) (IEEE sqrt), (rad cos, rad sin)(2 pi u(w1))."""
    L = opf.lib()
    rad = np.sqrt(f32(-2.0) * f32(L.orc_logf(float(uniform01(w0)))))
    c, s = ctypes.c_float(), ctypes.c_float()
    L.orc_sincos2pi(float(uniform01(w1)), ctypes.byref(c), ctypes.byref(s))
    return f32(rad * f32(c.value)), f32(rad * f32(s.value))


def clampf(v, lo, hi) -> np.float32:
    """fminf(fmaxf(v, lo), hi) for finite v."""
    v, lo, hi = f32(v), f32(lo), f32(hi)
    v = lo if v < lo else v
    return hi if v > hi else v


def noise(gi: int, frame: int, seed: int):
    """(n0, n1, n2) from counter (gi, frame, 0, 0) — S2's — and (n3, n4) from counter (gi, frame, 0, 1)."""
    seed &= (1 << 64) - 1
    key = (seed & 0xFFFFFFFF, seed >> 32)
    r = opf.philox4x32_10((gi, frame, 0, 0), key)
    q = opf.philox4x32_10((gi, frame, 0, 1), key)
    n0, n1 = gauss_pair(r[0], r[1])
    n2, _ = gauss_pair(r[2], r[3])
    n3, n4 = gauss_pair(q[0], q[1])
    return n0, n1, n2, n3, n4


def predict_cv(p: np.ndarray, global_begin: int, seed: int, frame: int, motion_std, velocity_std, decay, vmax,
               width, height, scale_range) -> None:
    """SPEC S11 predict, in place on float32[5][n] = x | y | s | vx | vy."""
    assert p.dtype == np.float32 and p.shape[0] == 5
    L = opf.lib()
    sx, sy, ss = (f32(v) for v in motion_std)
    svx, svy = (f32(v) for v in velocity_std)
    d, vmax = f32(decay), f32(vmax)
    wmax, hmax = f32(width) - f32(1.0), f32(height) - f32(1.0)
    smin, smax = (f32(v) for v in scale_range)
    for i in range(p.shape[1]):
        n0, n1, n2, n3, n4 = noise(global_begin + i, frame, seed)
        vx = clampf(fmaf(svx, n3, f32(d * p[3, i])), -vmax, vmax)
        vy = clampf(fmaf(svy, n4, f32(d * p[4, i])), -vmax, vmax)
        p[0, i] = clampf(fmaf(sx, n0, f32(p[0, i] + vx)), 0.0, wmax)
        p[1, i] = clampf(fmaf(sy, n1, f32(p[1, i] + vy)), 0.0, hmax)
        p[2, i] = clampf(f32(p[2, i] * f32(L.orc_expf(float(f32(ss * n2))))), smin, smax)
        p[3, i], p[4, i] = vx, vy


def step(Q, state: np.ndarray, seed: int, frame: int, method: str, tau, K: int) -> dict:
    """One frame's estimate + (gated) resample of the posterior weights Q over float32[5][P]: s10_reference.step on
    rows 0-2 (T, sums, ess, flag, ancestors, carry), five rows gathered by its ancestors, and the velocity sums over the
    same weights (every weight 1 when T == 0)."""
    r = R10.step(Q, state[:3], seed, frame, method, tau, K)
    w = [int(q) for q in Q] if r["T"] else [1] * len(Q)
    r["vsums"] = [math.fsum(float(q) * float(v) for q, v in zip(w, state[c])) for c in (3, 4)]
    r["state"] = np.ascontiguousarray(state[:, r["anc"]])
    return r


def velocity(r: dict, P: int):
    d = float(r["T"]) if r["T"] else float(P)
    return tuple(s / d for s in r["vsums"])


class Filter:
    """The S11 recursion of one target: predict_cv, posterior = carry x likelihood (S10; the identity carry without a
    gate), step."""

    def __init__(self, P, init_state, motion_std, scale_range, seed, frame_size, K, velocity_std, decay, vmax,
                 method=R10.SYSTEMATIC, tau=None):
        self.P, self.K, self.method, self.tau, self.seed = P, K, method, tau, seed
        self.motion_std, self.scale_range = motion_std, scale_range
        self.velocity_std, self.decay, self.vmax = velocity_std, decay, vmax
        self.height, self.width = frame_size
        self.state = np.zeros((5, P), np.float32)
        for c, v in enumerate(init_state):
            self.state[c] = v
        self.carry = [R10.identity(K)] * P
        self.frame = 0

    def predict(self, frame=None):
        self.frame = self.frame + 1 if frame is None else frame
        predict_cv(self.state, 0, self.seed, self.frame, self.motion_std, self.velocity_std, self.decay, self.vmax,
                   self.width, self.height, self.scale_range)

    def update(self, L) -> dict:
        r = step(R10.weight_prior(L, self.carry, self.K), self.state, self.seed, self.frame, self.method, self.tau,
                 self.K)
        self.state = r["state"]
        self.carry = [int(c) for c in r["carry"]]
        return r
