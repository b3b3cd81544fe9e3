"""SPEC S10 (adaptive resampling) restated in Python ints: the reference of tests/test_s10_*.py. Everything integer is
exact by construction (Python ints); the ESS is the three IEEE fp64 operations S10 names; the estimate sums are
math.fsum (the tests compare them at 1e-12 relative, as the S6 tests do). Philox and predict come from oracle.pf."""
import bisect
import itertools
import math
import struct

import numpy as np

from oracle import pf as opf

SYSTEMATIC, STRATIFIED = "systematic", "stratified"


def identity(K: int) -> int:
    return 1 << (K + 1)


def weight_prior(L, C, K: int):
    """Rule 1: Q_i = (L_i * C_i) >> (K + 1)."""
    return [(int(l) * int(c)) >> (K + 1) for l, c in zip(L, C)]


def ess(Q) -> float:
    """Rule 3: (Td * Td) / S2d with S2 = sum Q^2 split into 64-bit words; 0.0 when T == 0."""
    T = sum(int(q) for q in Q)
    if T == 0:
        return 0.0
    S2 = sum(int(q) * int(q) for q in Q)
    hi, lo = S2 >> 64, S2 & ((1 << 64) - 1)
    Td = float(T)
    S2d = float(hi) * 18446744073709551616.0 + float(lo)
    return (Td * Td) / S2d


def f64_bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def gate(Q, P: int, tau) -> bool:
    """Rule 4: resample iff T == 0, or the gate is disabled (tau None), or ess < tau * P."""
    return sum(int(q) for q in Q) == 0 or tau is None or ess(Q) < tau * float(P)


def word(seed: int, frame: int, j: int, method: str) -> int:
    seed &= (1 << 64) - 1
    key = (seed & 0xFFFFFFFF, seed >> 32)
    ctr = (j, frame, 1, 1) if method == STRATIFIED else (0, frame, 1, 0)
    return int(opf.philox4x32_10(ctr, key)[0])


def positions(T: int, P: int, seed: int, frame: int, method: str):
    """Rule 5: pos_j = floor((j T + floor(U_j T / 2^32)) / P); U_j the frame's word (systematic) or slot j's."""
    if method == SYSTEMATIC:
        U = word(seed, frame, 0, method)
        return [(j * T + ((U * T) >> 32)) // P for j in range(P)]
    return [(j * T + ((word(seed, frame, j, method) * T) >> 32)) // P for j in range(P)]


def step(Q, states: np.ndarray, seed: int, frame: int, method: str, tau, K: int) -> dict:
    """One frame's estimate + (gated) resample of the posterior weights Q (ints) and states float32[3][P]:
    T, the three sums, ess, the flag, m, ancestors, the new states and the new carry."""
    Q = [int(q) for q in Q]
    P = len(Q)
    T, m = sum(Q), max(Q)
    w = Q if T else [1] * P
    sums = [math.fsum(float(q) * float(v) for q, v in zip(w, states[c])) for c in range(3)]
    flag = gate(Q, P, tau)
    if flag:
        if T:
            cdf = list(itertools.accumulate(Q))
            anc = [bisect.bisect_right(cdf, p) for p in positions(T, P, seed, frame, method)]
        else:
            anc = positions(P, P, seed, frame, method)
        carry = [identity(K)] * P
    else:
        sh = K + 1 - m.bit_length()
        anc = list(range(P))
        carry = [q << sh if sh >= 0 else q >> -sh for q in Q]
    anc = np.array(anc, np.int32)
    return {"T": T, "sums": sums, "ess": ess(Q), "resampled": flag, "m": m, "anc": anc,
            "states": np.ascontiguousarray(states[:, anc]), "carry": np.array(carry, np.int64)}


def estimate(r: dict, P: int):
    d = float(r["T"]) if r["T"] else float(P)
    return tuple(s / d for s in r["sums"])


class Filter:
    """The S10 recursion of one target over frames: predict (oracle S2), posterior = prior x likelihood, step."""

    def __init__(self, P, init_state, motion_std, scale_range, seed, frame_size, K, method, tau):
        self.P, self.K, self.method, self.tau, self.seed = P, K, method, tau, seed
        self.motion_std, self.scale_range = motion_std, scale_range
        self.height, self.width = frame_size
        self.particles = np.empty((3, P), np.float32)
        for c in range(3):
            self.particles[c] = init_state[c]
        self.carry = [identity(K)] * P
        self.frame = 0

    def predict(self, frame=None):
        self.frame = self.frame + 1 if frame is None else frame
        opf.predict(self.particles, 0, self.seed, self.frame, self.motion_std, self.width, self.height,
                    self.scale_range)

    def update(self, L) -> dict:
        r = step(weight_prior(L, self.carry, self.K), self.particles, self.seed, self.frame, self.method, self.tau,
                 self.K)
        self.particles = r["states"]
        self.carry = [int(c) for c in r["carry"]]
        return r
