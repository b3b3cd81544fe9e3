"""The references of tests/test_gpu_pf_exact.py, in plain numpy and Python ints (no torch), on top of the oracle
(oracle/pf_oracle.c: Philox, the fixed fp32 ln / exp / sincos, S2's predict) and of s10 / s11 / s12 / s16_reference.

* the classes of a Philox word that tools/philox_hunt.py hunts, restated from the definitions (`word_classes`), so the
  pasted table is checked without trusting the tool;
* the predict kernels at "transparent" parameters, under which an output row is one fixed function's result:
  `walk`, `cv`, `angle`, `search`, and `exp_steps` (the n of fixed_expf's range reduction per particle);
* `tree_sums`: SPEC S6's sums in the stats tree's documented order, with T, S2 and m as Python ints and the uniform
  pass for T == 0; `index_order_sums`: the same sums in index order (the oracle's order);
* `tie_weights`, `resample`, `tie_slots`: a real CDF whose values the systematic positions land on constantly.
"""
import bisect
import itertools

import numpy as np

import s10_reference as R10
import s11_reference as R11
import s12_reference as R12
import s16_reference as R16
from oracle import pf as opf

f32 = np.float32
PI32 = float(f32(np.pi))
BIG = float(2 ** 30)                          # width = height: the position clamp's upper end, out of every noise's reach
# The scale clamp out of fixed_expf's reach on both sides, so that s' = exp(sig_s n2) exactly: its results span
# {0} and [e^-87, e^88] = [1.6e-38, 1.7e38], which (2^-100, 2^100) would cut at |x| > 69.3.
SCALE_RANGE = (0.0, float(np.finfo(np.float32).max))
K_MAX = (1 << 23) - 1


# ---------------------------------------------------------------------------------------------- hunted words
def key(seed: int):
    seed &= (1 << 64) - 1
    return seed & 0xFFFFFFFF, seed >> 32


def entry_word(entry) -> int:
    """The word a table row (seed, frame, c2, c3, gi, word, class) names, by the oracle's Philox."""
    seed, frame, c2, c3, gi, word, _ = entry
    return int(opf.philox4x32_10((gi, frame, c2, c3), key(seed))[word])


def word_classes(c3: int, word: int, w: int) -> set:
    """The classes of word `word` = w of a counter (gi, frame, 0, c3), from their definitions: k = w >> 9,
    u = (2k + 1) 2^-24. Words 0 and 2 of c3 = 0 and word 0 of c3 = 1, 2 feed fixed_logf; words 1 and 3 of c3 = 0 and
    word 1 of c3 = 1, 2 feed fixed_sincos2pi; words 0, 1 of c3 = 3 are the search lattice's jitter."""
    k = int(w) >> 9
    out = set()
    is_log = (c3 == 0 and word in (0, 2)) or (c3 in (1, 2) and word == 0)
    is_ang = (c3 == 0 and word in (1, 3)) or (c3 in (1, 2) and word == 1)
    if is_log:
        u = R11.uniform01(w)
        m = (np.array([u], np.float32).view(np.uint32)[0] & 0x007FFFFF) | 0x3F000000
        if k == 0:
            out.add("log_lo")
        if k == K_MAX:
            out.add("log_hi")
        if m == 0x3F3504F3:                    # fp32(0.70710678118654752): m < it is false
            out.add("split_hi")
        if m == 0x3F3504F2:                    # the fp32 number just below: the branch is taken
            out.add("split_lo")
    if is_ang:
        t = f32(R11.uniform01(w) * f32(4.0))
        q = int(np.floor(t))
        r = f32(t - f32(q))
        if r == f32(2.0 ** -22):
            out.add(f"ang_q{q}_lo")
        if r == f32(1.0 - 2.0 ** -22):
            out.add(f"ang_q{q}_hi")
    if c3 == 3 and word in (0, 1):
        if k == 0:
            out.add("u_lo")
        if k == K_MAX:
            out.add("u_hi")
    return out


def radius(w: int) -> np.float32:
    """Box-Muller's radius sqrt(-2 ln u(w)) by the oracle's ln."""
    return np.sqrt(f32(-2.0) * f32(opf.lib().orc_logf(float(R11.uniform01(w)))))


# ---------------------------------------------------------------------------------------------- transparent predicts
def walk(n: int, gb: int, seed: int, frame: int, sig: float, sig_s: float) -> np.ndarray:
    """vpf_predict on x = y = 0, s = 1, width = height = 2^30, SCALE_RANGE, by the C oracle:
    x' = max(sig n0, 0), y' = max(sig n1, 0) (sig = +1 shows the positive noises' bits, -1 the negative ones'),
    s' = fixed_expf(sig_s n2)."""
    p = np.zeros((3, n), np.float32)
    p[2] = 1.0
    opf.predict(p, gb, seed, frame, (sig, sig, sig_s), BIG, BIG, SCALE_RANGE)
    return p


def cv(n: int, gb: int, seed: int, frame: int, sig_s: float = 1.0) -> np.ndarray:
    """vpf_predict_cv on zero positions and velocities, s = 1, decay 1, sig_vx = sig_vy = 1, vmax = 64 (the symmetric
    clamp never binds: |n| < 5.78), sig_x = sig_y = 1: vx' = n3, vy' = n4 exactly, by s11_reference."""
    p = np.zeros((5, n), np.float32)
    p[2] = 1.0
    R11.predict_cv(p, gb, seed, frame, (1.0, 1.0, sig_s), (1.0, 1.0), 1.0, 64.0, BIG, BIG, SCALE_RANGE)
    return p


def angle(n: int, gb: int, seed: int, frame: int) -> np.ndarray:
    """vpf_predict_angle on angle 0 with sig_a = 0.5 over [-fp32(pi), fp32(pi)]: |n5| / 2 < 2.89, so a' = n5 / 2
    exactly, by s12_reference."""
    a = np.zeros(n, np.float32)
    R12.predict_angle(a, gb, seed, frame, 0.5, -PI32, PI32)
    return a


def search(n: int, gb: int, P: int, seed: int, frame: int, sig_s: float, W: int, H: int, rows: int) -> np.ndarray:
    """vpf_predict_search on s = 1 (x, y, and the velocity rows hold a value that must not survive), SCALE_RANGE, by
    s16_reference."""
    p = np.full((rows, n), 7.0, np.float32)
    p[2] = 1.0
    R16.predict_search(p, gb, P, seed, frame, sig_s, W, H, SCALE_RANGE)
    return p


def scale_noise(n: int, gb: int, seed: int, frame: int) -> np.ndarray:
    """n2 float32[n] of particles gb .. gb + n - 1: the cosine branch on words 2, 3 of counter (gi, frame, 0, 0)."""
    out = np.empty(n, np.float32)
    for i in range(n):
        r = opf.philox4x32_10((gb + i, frame, 0, 0), key(seed))
        out[i] = R11.gauss_pair(r[2], r[3])[0]
    return out


def exp_steps(n2: np.ndarray, sig_s: float):
    """Per particle what fixed_expf(x), x = fp32(sig_s n2), does: (None, False) for the exact zero (x < -87), else its
    n = floor(fmaf(x', log2 e, 0.5)) with x' = min(x, 88), and whether that clamp bound."""
    out = []
    for v in n2:
        x = f32(f32(sig_s) * f32(v))
        if x < f32(-87.0):
            out.append((None, False))
            continue
        clamped = bool(x > f32(88.0))
        x = f32(88.0) if clamped else x
        out.append((int(np.floor(R11.fmaf(x, f32(1.44269504088896341), f32(0.5)))), clamped))
    return out


def search_geometry(gi: int, word: int):
    """(P, W, H) for a hunted jitter word of particle gi: gi is the last particle (the last y-band). Word 0: W = 224 P,
    H = 224, so gx = P and gi also stands in the last column; word 1: the 320 x 224 frame."""
    P = gi + 1
    return (P, 224 * P, 224) if word == 0 else (P, 320, 224)


# ---------------------------------------------------------------------------------------------- the stats tree
def tree_sums(Q, rows: np.ndarray) -> dict:
    """SPEC S6 / S10's reductions in the stats tree's order (csrc/pf_tree.h), over rows float32[R][P]: partial t of
    1024 accumulates i = t, t + 1024, ... in order from +0, each term the single rounded product fp64(q_i) fp64(x_i);
    then the halving o = 512 .. 1 with s[t] += s[t + o]. T, S2 = sum q^2 and m = max q are exact Python ints. When
    T == 0 the sums are repeated with every weight 1 (`uniform`: the fallback's plain sums)."""
    Q = [int(q) for q in Q]
    P = len(Q)
    rows = np.asarray(rows, np.float32)
    assert rows.ndim == 2 and rows.shape[1] == P
    T = sum(Q)
    uniform = T == 0
    w = np.array([1.0] * P if uniform else [float(q) for q in Q], np.float64)     # q < 2^53: float(q) is exact
    assert uniform or max(Q) < 1 << 53
    sums = []
    for c in range(rows.shape[0]):
        x = rows[c].astype(np.float64)
        s = np.zeros(1024, np.float64)
        for b in range(0, P, 1024):
            e = min(P, b + 1024)
            s[:e - b] += w[b:e] * x[b:e]
        o = 512
        while o:
            s[:o] += s[o:2 * o]
            o >>= 1
        sums.append(float(s[0]))
    return {"T": T, "sums": sums, "S2": sum(q * q for q in Q), "m": max(Q), "uniform": uniform}


def index_order_sums(Q, rows: np.ndarray):
    """The same fp64 sums accumulated in index order (oracle/pf_oracle.c's orc_shard_stats)."""
    out = []
    for c in range(rows.shape[0]):
        s = 0.0
        for q, x in zip(Q, rows[c]):
            s += float(int(q)) * float(x)
        out.append(s)
    return out


def order_case(P: int, seed: int = 0):
    """40-bit weights and states spread over [1e-3, 1e4] (log-uniform, 24-bit mantissas): the products round and the
    partial sums span many binades, so the order of the additions shows in the last bits. For P > 1 the first draw is
    taken at which each of the three tree-order sums differs in bits from its index-order sum (decided by this file's
    two restatements alone), so that a pass cannot come from order-blind data."""
    while True:
        rng = np.random.default_rng(1000 * P + seed)
        Q = rng.integers(1 << 39, 1 << 40, P, dtype=np.int64)
        rows = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), (3, P))).astype(np.float32)
        if P == 1 or all(a != b for a, b in zip(tree_sums(Q, rows)["sums"], index_order_sums(Q, rows))):
            return Q, rows
        seed += 1


# ---------------------------------------------------------------------------------------------- ties on a real CDF
def tie_weights(P: int) -> np.ndarray:
    """Q_i in {0, 1, 2, 3}, deterministic, sum exactly 2 P: the period 0 0 3 3 2 3 3 2 (a run of two zeros per period),
    a 1 every 16, zeros forced at both ends, over a middle run, and (P > 4096) over the run 4090 .. 4096 that crosses
    the 4096-element scan chunk; then the twos (and ones) nearest the front are raised until the sum is 2 P."""
    assert P >= 33
    Q = np.array([(0, 0, 3, 3, 2, 3, 3, 2)[i % 8] for i in range(P)], np.int64)
    Q[5::16] = 1
    zero = {0, 1, P - 2, P - 1, P // 2, P // 2 + 1, P // 2 + 2}
    if P > 4096:
        zero |= set(range(4090, 4097))
    Q[sorted(zero)] = 0
    d = 2 * P - int(Q.sum())
    assert d >= 0
    for i in range(P):
        while d > 0 and 0 < Q[i] < 3:
            Q[i] += 1
            d -= 1
    assert d == 0 and int(Q.sum()) == 2 * P and Q.min() == 0 and Q.max() == 3
    return Q


def positions(T: int, P: int, U: int):
    """SPEC S7: pos_j = floor((j T + floor(U T / 2^32)) / P), in Python ints."""
    return [(j * T + ((U * T) >> 32)) // P for j in range(P)]


def resample(Q, U: int) -> np.ndarray:
    """SPEC S7's systematic ancestors a_j = min{i : C_i > pos_j} for a given word U (T > 0), in Python ints."""
    Q = [int(q) for q in Q]
    cdf = list(itertools.accumulate(Q))
    return np.array([bisect.bisect_right(cdf, p) for p in positions(cdf[-1], len(Q), U)], np.int32)


def tie_slots(Q, pos) -> int:
    """The number of slots whose position equals a CDF value: exactly the slots at which min{i : C_i > pos} and
    min{i : C_i >= pos} differ."""
    cdf = set(itertools.accumulate(int(q) for q in Q))
    return sum(1 for p in pos if p in cdf)


def step_positions(Q, seed: int, frame: int, method: str):
    Q = [int(q) for q in Q]
    return R10.positions(sum(Q), len(Q), seed, frame, method)
