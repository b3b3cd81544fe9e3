"""Exact tests of the particle-filter kernel family (csrc/pf_kernels.hip, pf_tree.h, pf_predict.h, pf_search.hip,
pf_gate.hip, pf_mode.hip) at the parameters and edges the other suites do not reach. Every GPU comparison is bit or
integer equality with tests/pf_exact_reference.py, oracle/pf_oracle.c or s10 / s11 / s12 / s15 / s16 / s17_reference.

1. transparent parameters: an output row IS a fixed fp32 function's result (Box-Muller's two branches, fixed_expf over
   its whole range with both cut-offs);
2. hunted counters (HUNTED, from tools/philox_hunt.py): the extremes of fixed_logf / fixed_sincos2pi / the lattice
   jitter on one-particle windows, and global indices up to 2^32 - 2;
3. the stats tree's order, bit for bit, through all five entry points;
4. the integer range at SPEC S5's bound K + ceil(log2 P) = 62;
5. ties between the systematic positions and a real CDF with runs of zero weights;
6. the skip carry's right shift and vpf_gather_rows' out-of-range ancestors.

The tests without the gpu mark check the table, the references and the cases' own conditions on the CPU.
Run: python -m pytest tests/test_gpu_pf_exact.py [-m gpu]."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import pf_exact_reference as X
import s10_reference as R10
import s11_reference as R11
import s15_reference as R15
import s17_reference as R17
from oracle import pf as opf

gpu = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
SENT = -12345.0
SEED = 1234
SIZES = [1, 257, 4099]
SIG_S = (1.0, -1.0, 4.0, 16.0, -16.0)
METHODS = {R10.SYSTEMATIC: 0, R10.STRATIFIED: 1}

# tools/philox_hunt.py --seed 1234: (seed, frame, c2, c3, gi, word, class), two hits per (c3, word, class).
HUNTED = [
    (1234, 1555, 0, 0, 1696, 0, "log_hi"), (1234, 5335, 0, 0, 1592, 0, "log_hi"),
    (1234, 1845, 0, 0, 427, 0, "log_lo"), (1234, 2783, 0, 0, 2877, 0, "log_lo"),
    (1234, 1012, 0, 0, 2348, 0, "split_hi"), (1234, 2616, 0, 0, 1449, 0, "split_hi"),
    (1234, 376, 0, 0, 1152, 0, "split_lo"), (1234, 2545, 0, 0, 2086, 0, "split_lo"),
    (1234, 202, 0, 0, 3825, 1, "ang_q0_hi"), (1234, 2802, 0, 0, 97, 1, "ang_q0_hi"),
    (1234, 947, 0, 0, 625, 1, "ang_q0_lo"), (1234, 2767, 0, 0, 63, 1, "ang_q0_lo"),
    (1234, 623, 0, 0, 1711, 1, "ang_q1_hi"), (1234, 4380, 0, 0, 34, 1, "ang_q1_hi"),
    (1234, 1274, 0, 0, 3851, 1, "ang_q1_lo"), (1234, 4970, 0, 0, 2238, 1, "ang_q1_lo"),
    (1234, 1197, 0, 0, 1251, 1, "ang_q2_hi"), (1234, 10505, 0, 0, 1419, 1, "ang_q2_hi"),
    (1234, 4120, 0, 0, 2563, 1, "ang_q2_lo"), (1234, 5321, 0, 0, 45, 1, "ang_q2_lo"),
    (1234, 4263, 0, 0, 354, 1, "ang_q3_hi"), (1234, 6827, 0, 0, 3917, 1, "ang_q3_hi"),
    (1234, 1968, 0, 0, 330, 1, "ang_q3_lo"), (1234, 3910, 0, 0, 268, 1, "ang_q3_lo"),
    (1234, 7132, 0, 0, 2578, 2, "exp_cut"), (1234, 11868, 0, 0, 1657, 2, "exp_cut"),
    (1234, 994, 0, 0, 1654, 2, "log_hi"), (1234, 2478, 0, 0, 2997, 2, "log_hi"),
    (1234, 2742, 0, 0, 367, 2, "log_lo"), (1234, 3536, 0, 0, 3664, 2, "log_lo"),
    (1234, 1448, 0, 0, 1293, 2, "split_hi"), (1234, 4790, 0, 0, 867, 2, "split_hi"),
    (1234, 378, 0, 0, 3731, 2, "split_lo"), (1234, 6167, 0, 0, 617, 2, "split_lo"),
    (1234, 788, 0, 0, 696, 3, "ang_q0_hi"), (1234, 6189, 0, 0, 1218, 3, "ang_q0_hi"),
    (1234, 928, 0, 0, 3452, 3, "ang_q0_lo"), (1234, 6025, 0, 0, 3094, 3, "ang_q0_lo"),
    (1234, 1475, 0, 0, 1123, 3, "ang_q1_hi"), (1234, 4822, 0, 0, 2746, 3, "ang_q1_hi"),
    (1234, 1175, 0, 0, 883, 3, "ang_q1_lo"), (1234, 13046, 0, 0, 4064, 3, "ang_q1_lo"),
    (1234, 1069, 0, 0, 1412, 3, "ang_q2_hi"), (1234, 1331, 0, 0, 2441, 3, "ang_q2_hi"),
    (1234, 2700, 0, 0, 3179, 3, "ang_q2_lo"), (1234, 7015, 0, 0, 1361, 3, "ang_q2_lo"),
    (1234, 3062, 0, 0, 2766, 3, "ang_q3_hi"), (1234, 5629, 0, 0, 626, 3, "ang_q3_hi"),
    (1234, 4049, 0, 0, 1692, 3, "ang_q3_lo"), (1234, 4792, 0, 0, 3022, 3, "ang_q3_lo"),
    (1234, 5400, 0, 1, 3809, 0, "log_hi"), (1234, 6746, 0, 1, 138, 0, "log_hi"),
    (1234, 4516, 0, 1, 1961, 0, "log_lo"), (1234, 4612, 0, 1, 3880, 0, "log_lo"),
    (1234, 2019, 0, 1, 3712, 0, "split_hi"), (1234, 3737, 0, 1, 3959, 0, "split_hi"),
    (1234, 3414, 0, 1, 4067, 0, "split_lo"), (1234, 3665, 0, 1, 1459, 0, "split_lo"),
    (1234, 5053, 0, 1, 2958, 1, "ang_q0_hi"), (1234, 13124, 0, 1, 1355, 1, "ang_q0_hi"),
    (1234, 1070, 0, 1, 701, 1, "ang_q0_lo"), (1234, 1203, 0, 1, 22, 1, "ang_q0_lo"),
    (1234, 1643, 0, 1, 718, 1, "ang_q1_hi"), (1234, 4820, 0, 1, 90, 1, "ang_q1_hi"),
    (1234, 830, 0, 1, 674, 1, "ang_q1_lo"), (1234, 1754, 0, 1, 2915, 1, "ang_q1_lo"),
    (1234, 382, 0, 1, 2125, 1, "ang_q2_hi"), (1234, 2023, 0, 1, 954, 1, "ang_q2_hi"),
    (1234, 190, 0, 1, 2790, 1, "ang_q2_lo"), (1234, 1045, 0, 1, 1555, 1, "ang_q2_lo"),
    (1234, 2709, 0, 1, 2936, 1, "ang_q3_hi"), (1234, 6034, 0, 1, 2925, 1, "ang_q3_hi"),
    (1234, 5024, 0, 1, 2431, 1, "ang_q3_lo"), (1234, 5489, 0, 1, 854, 1, "ang_q3_lo"),
    (1234, 1743, 0, 2, 1679, 0, "log_hi"), (1234, 5510, 0, 2, 2542, 0, "log_hi"),
    (1234, 1619, 0, 2, 1697, 0, "log_lo"), (1234, 1663, 0, 2, 1963, 0, "log_lo"),
    (1234, 918, 0, 2, 1176, 0, "split_hi"), (1234, 4400, 0, 2, 2539, 0, "split_hi"),
    (1234, 179, 0, 2, 3791, 0, "split_lo"), (1234, 2027, 0, 2, 1990, 0, "split_lo"),
    (1234, 429, 0, 2, 3727, 1, "ang_q0_hi"), (1234, 3213, 0, 2, 3419, 1, "ang_q0_hi"),
    (1234, 1481, 0, 2, 263, 1, "ang_q0_lo"), (1234, 3565, 0, 2, 3814, 1, "ang_q0_lo"),
    (1234, 2618, 0, 2, 3729, 1, "ang_q1_hi"), (1234, 3737, 0, 2, 1949, 1, "ang_q1_hi"),
    (1234, 4481, 0, 2, 2885, 1, "ang_q1_lo"), (1234, 8805, 0, 2, 1521, 1, "ang_q1_lo"),
    (1234, 8674, 0, 2, 4068, 1, "ang_q2_hi"), (1234, 9007, 0, 2, 1445, 1, "ang_q2_hi"),
    (1234, 336, 0, 2, 2168, 1, "ang_q2_lo"), (1234, 1084, 0, 2, 2422, 1, "ang_q2_lo"),
    (1234, 5586, 0, 2, 3322, 1, "ang_q3_hi"), (1234, 5879, 0, 2, 1497, 1, "ang_q3_hi"),
    (1234, 114, 0, 2, 107, 1, "ang_q3_lo"), (1234, 576, 0, 2, 1850, 1, "ang_q3_lo"),
    (1234, 1550, 0, 3, 2559, 0, "u_hi"), (1234, 2609, 0, 3, 858, 0, "u_hi"),
    (1234, 433, 0, 3, 3765, 0, "u_lo"), (1234, 695, 0, 3, 3605, 0, "u_lo"),
    (1234, 2658, 0, 3, 2547, 1, "u_hi"), (1234, 14872, 0, 3, 3, 1, "u_hi"),
    (1234, 2827, 0, 3, 3346, 1, "u_lo"), (1234, 4619, 0, 3, 3683, 1, "u_lo"),
]
LOG_CLASSES = ("log_lo", "log_hi", "split_lo", "split_hi")
ANG_CLASSES = tuple(f"ang_q{q}_{e}" for q in range(4) for e in ("lo", "hi"))
# (c3, word) -> the classes the table must hold, two entries each
REQUIRED = {(0, 0): LOG_CLASSES, (0, 2): LOG_CLASSES + ("exp_cut",), (0, 1): ANG_CLASSES, (0, 3): ANG_CLASSES,
            (1, 0): LOG_CLASSES, (1, 1): ANG_CLASSES, (2, 0): LOG_CLASSES, (2, 1): ANG_CLASSES,
            (3, 0): ("u_lo", "u_hi"), (3, 1): ("u_lo", "u_hi")}
EXP_FRAME = 7132           # HUNTED's first exp_cut entry: particle 2578 of the 4099-particle batch at global_begin 0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f64_bits(x) -> int:
    return R10.f64_bits(float(x))


# =========================================================================================== CPU: table and references
def test_hunted_table_holds_what_it_says():
    """Every entry's word, recomputed with the oracle's Philox, is of the class the row names; every (counter kind,
    word, class) has at least two entries; an exp_cut entry's n2 passes both of fixed_expf's cut-offs at |sig_s| = 16;
    and the hunted u = 2^-24 gives the largest radius any word can give."""
    count = {}
    for e in HUNTED:
        seed, frame, c2, c3, gi, word, cls = e
        assert seed == SEED and c2 == 0 and 0 <= gi < 4099
        if cls == "exp_cut":
            n2 = X.scale_noise(1, gi, seed, frame)[0]
            assert abs(n2) > 5.5 and f32(16.0) * abs(n2) > f32(88.0) and f32(-16.0) * abs(n2) < f32(-87.0), e
        else:
            assert cls in X.word_classes(c3, word, X.entry_word(e)), e
        count[(c3, word, cls)] = count.get((c3, word, cls), 0) + 1
    for (c3, word), classes in REQUIRED.items():
        for cls in classes:
            assert count.get((c3, word, cls), 0) >= 2, (c3, word, cls)
    assert sum(count.values()) == len(HUNTED) and len(set(HUNTED)) == len(HUNTED)
    top = X.radius(0)                                   # k = 0: u = 2^-24
    for e in HUNTED:
        if e[6] == "log_lo":
            assert X.entry_word(e) >> 9 == 0 and bits(X.radius(X.entry_word(e))) == bits(top)
    rng = np.random.default_rng(0)
    ks = set(range(1, 4097)) | {1 << j for j in range(23)} | {X.K_MAX} | set(rng.integers(1, 1 << 23, 4096).tolist())
    assert all(X.radius(k << 9) < top for k in ks) and 5.76 < float(top) < 5.77


@functools.lru_cache(maxsize=None)
def _exp_noise():
    return X.scale_noise(4099, 0, SEED, EXP_FRAME)


def test_scale_batch_reaches_every_path_of_fixed_expf():
    """The 4099-particle batch at EXP_FRAME under sig_s in SIG_S, from the reference alone: an exact 0, a value at the 88
    clamp (n = 127), odd and even n of both signs down to below -64, and n = 0."""
    steps = [s for sig in SIG_S for s in X.exp_steps(_exp_noise(), sig)]
    ns = {n for n, _ in steps if n is not None}
    assert (None, False) in steps and any(c for _, c in steps)
    assert any(n > 0 and n % 2 for n in ns) and any(n > 0 and n % 2 == 0 for n in ns)
    assert any(n < 0 and n % 2 for n in ns) and any(n < 0 and n % 2 == 0 for n in ns)
    assert 0 in ns and max(ns) == 127 and min(ns) < -64
    out = np.concatenate([X.walk(4099, 0, SEED, EXP_FRAME, 1.0, sig)[2] for sig in (16.0, -16.0)])
    assert (out == 0.0).any() and (bits(out) == bits([opf.lib().orc_expf(88.0)])[0]).any()
    one = [n for n, _ in X.exp_steps(_exp_noise(), 0.02)]          # the other suites' sigma: n is always 0
    assert set(one) == {0}


def test_transparent_rows_are_the_functions_own_results():
    """At the transparent parameters the reference's rows are the noises themselves: vx, vy = n3, n4; a = n5 / 2;
    max(x', 0) under sig = +-1 shows n0 with one of the two signs; s' = orc_expf(sig_s n2)."""
    n, frame = 257, 5
    p, c, a = X.walk(n, 0, SEED, frame, 1.0, 1.0), X.cv(n, 0, SEED, frame), X.angle(n, 0, SEED, frame)
    m = X.walk(n, 0, SEED, frame, -1.0, -1.0)
    for i in range(n):
        n0, n1, n2, n3, n4 = R11.noise(i, frame, SEED)
        assert bits(c[3, i]) == bits(n3) and bits(c[4, i]) == bits(n4)
        assert bits(p[0, i]) == bits(max(n0, f32(0))) and bits(m[0, i]) == bits(max(-n0, f32(0)))
        assert bits(p[1, i]) == bits(max(n1, f32(0))) and bits(m[1, i]) == bits(max(-n1, f32(0)))
        assert bits(p[2, i]) == bits(f32(opf.lib().orc_expf(float(n2))))
        n5 = R11.gauss_pair(*opf.philox4x32_10((i, frame, 0, 2), X.key(SEED))[:2])[0]
        assert bits(a[i]) == bits(f32(0.5) * n5)
    assert ((p[:2] != 0) ^ (m[:2] != 0)).all()


@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 2049, 5000])
def test_tree_reference_against_fsum_and_the_oracle(P):
    """tree_sums against math.fsum to 1e-12 and against the oracle's index-order sums at rtol 1e-13 (the only
    tolerances of this file: the reference's own self-check); its integers against plain Python; and, from P = 1023 on,
    every one of its sums differs in bits from the index-order sum, so the order is visible in this data."""
    Q, rows = X.order_case(P)
    r = X.tree_sums(Q, rows)
    T, osums = opf.shard_stats(Q, rows)
    assert r["T"] == T == int(Q.sum()) and r["m"] == int(Q.max()) and not r["uniform"]
    assert r["S2"] == sum(int(q) ** 2 for q in Q)
    for c in range(3):
        exact = math.fsum(float(q) * float(x) for q, x in zip(Q, rows[c]))
        assert abs(r["sums"][c] - exact) <= 1e-12 * abs(exact)
    np.testing.assert_allclose(r["sums"], osums, rtol=1e-13)
    assert [f64_bits(s) for s in X.index_order_sums(Q, rows)] == [f64_bits(s) for s in osums]
    assert r["sums"] == R15.tree_sums(Q, rows)
    if P >= 1023:
        assert all(f64_bits(a) != f64_bits(b) for a, b in zip(r["sums"], osums))
    z = X.tree_sums(np.zeros(P, np.int64), rows)
    assert z["uniform"] and z["T"] == 0 and z["sums"] == X.tree_sums([1] * P, rows)["sums"]


@pytest.mark.parametrize("P", [33, 4097])
def test_tie_weights_put_a_quarter_of_the_slots_on_a_cdf_value(P):
    """From the reference alone: T = 2 P, zeros at both ends and across the scan chunk, and for every U used at least
    a quarter of the slots have pos_j equal to a CDF value; the reference's ancestors equal the C oracle's."""
    Q = X.tie_weights(P)
    assert Q[0] == 0 and Q[-1] == 0 and (P < 4096 or not Q[4090:4097].any())
    for U in (0, 1 << 31, (1 << 32) - 1):
        assert X.tie_slots(Q, X.positions(2 * P, P, U)) * 4 >= P, U
        anc = X.resample(Q, U)
        assert np.array_equal(anc, opf.resample(Q, U)) and (Q[anc] > 0).all()
    for method in METHODS:
        assert X.tie_slots(Q, X.step_positions(Q, SEED, 9, method)) * 4 >= P, method


# =========================================================================================== GPU plumbing
@pytest.fixture(scope="module")
def L():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()
    assert torch.cuda.is_available()
    return _lib.lib()


def vpf():
    return torch.ops.vpf


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(host, n, call):
    """Runs call(device pointer) on a copy of host float32[R][ld]; returns (rc, the rows' first n columns), having
    checked that the padding columns keep their sentinel."""
    d = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
    rc = call(d.data_ptr())
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    assert np.array_equal(bits(out[:, n:]), bits(host[:, n:])), "a padding column was written"
    return rc, out[:, :n]


def _rows(R, n, ld, ones=(2,), fill=0.0):
    h = np.full((R, ld), SENT, np.float32)
    h[:, :n] = fill
    for c in ones:
        h[c, :n] = 1.0
    return h


def gpu_walk(L, n, gb, frame, sig, sig_s, ld=None, expect=0):
    ld = ld or n
    rc, out = _launch(_rows(3, n, ld), n, lambda p: L.vpf_predict(
        p, n, ld, gb, SEED, frame, sig, sig, sig_s, X.BIG, X.BIG, X.SCALE_RANGE[0], X.SCALE_RANGE[1], _stream()))
    assert rc == expect
    return out


def gpu_cv(L, n, gb, frame, sig_s=1.0, ld=None, expect=0):
    ld = ld or n
    rc, out = _launch(_rows(5, n, ld), n, lambda p: L.vpf_predict_cv(
        p, n, ld, gb, SEED, frame, 1.0, 1.0, sig_s, 1.0, 1.0, 1.0, 64.0, X.BIG, X.BIG, X.SCALE_RANGE[0],
        X.SCALE_RANGE[1], _stream()))
    assert rc == expect
    return out


def gpu_angle(L, n, gb, frame, expect=0):
    rc, out = _launch(_rows(1, n, n, ones=()), n, lambda p: L.vpf_predict_angle(
        p, n, gb, SEED, frame, 0.5, -X.PI32, X.PI32, _stream()))
    assert rc == expect
    return out[0]


def gpu_search(L, n, gb, P, frame, sig_s, W, H, rows, ld=None):
    from s16_reference import lattice
    ld = ld or n
    gx, inv_gx, inv_P = lattice(P, W, H)
    rc, out = _launch(_rows(rows, n, ld, fill=7.0), n, lambda p: L.vpf_predict_search(
        p, n, ld, gb, P, rows, SEED, frame, sig_s, float(W), float(H), X.SCALE_RANGE[0], X.SCALE_RANGE[1], gx,
        float(inv_gx), float(inv_P), _stream()))
    assert rc == 0
    return out


@functools.lru_cache(maxsize=None)
def ref_walk(n, gb, frame, sig, sig_s):
    return X.walk(n, gb, SEED, frame, sig, sig_s)


@functools.lru_cache(maxsize=None)
def ref_cv(n, gb, frame):
    return X.cv(n, gb, SEED, frame)


@functools.lru_cache(maxsize=None)
def ref_angle(n, gb, frame):
    return X.angle(n, gb, SEED, frame)


@functools.lru_cache(maxsize=None)
def ref_search(n, gb, P, frame, sig_s, W, H, rows):
    return X.search(n, gb, P, SEED, frame, sig_s, W, H, rows)


def same(got, ref, tag=""):
    assert got.shape == ref.shape and np.array_equal(bits(got), bits(ref)), tag


# =========================================================================================== 1. transparent parameters
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_walk_rows_are_the_noise_bits(L, n):
    """vpf_predict on x = y = 0 under sig = +1 and -1: each call shows the exact bits of the noises of one sign, and
    every particle's x (and y) is non-zero in exactly one of the two."""
    plus, minus = gpu_walk(L, n, 0, 5, 1.0, 1.0), gpu_walk(L, n, 0, 5, -1.0, -1.0)
    same(plus, ref_walk(n, 0, 5, 1.0, 1.0))
    same(minus, ref_walk(n, 0, 5, -1.0, -1.0))
    assert ((plus[:2] != 0) ^ (minus[:2] != 0)).all()


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_cv_velocity_rows_are_both_box_muller_branches(L, n):
    ref = ref_cv(n, 0, 5)
    assert np.abs(ref[3:]).max() < 64.0 and (ref[3:] != 0).all()          # the clamp never binds: vx = n3, vy = n4
    same(gpu_cv(L, n, 0, 5), ref)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_angle_row_is_half_the_cosine_branch(L, n):
    ref = ref_angle(n, 0, 5)
    assert np.abs(ref).max() < 2.89
    same(gpu_angle(L, n, 0, 5), ref)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_scale_row_is_fixed_expf_over_its_whole_range(L, n):
    """s = 1 and a scale range fixed_expf cannot reach: s' = exp(sig_s n2) exactly, for sig_s in {1, -1, 4, 16, -16}
    at the frame of a hunted exp_cut particle (test_scale_batch_reaches_every_path_of_fixed_expf lists what the
    4099-particle batch holds). vpf_predict_search's scale step (rows 3 and 5) gives the same bits."""
    for sig_s in SIG_S:
        ref = ref_walk(n, 0, EXP_FRAME, 1.0, sig_s)
        same(gpu_walk(L, n, 0, EXP_FRAME, 1.0, sig_s), ref, f"sig_s={sig_s}")
        for rows in (3, 5):
            got = gpu_search(L, n, 0, 4099, EXP_FRAME, sig_s, 320, 224, rows)
            same(got[2], ref[2], f"search rows={rows} sig_s={sig_s}")
            same(got, ref_search(n, 0, 4099, EXP_FRAME, sig_s, 320, 224, rows), f"search rows={rows} sig_s={sig_s}")


@gpu
def test_three_unequal_shards_equal_the_whole_call(L):
    """n = 4099 as shards of 1500, 2 and 2597 particles in buffers with ld > n: every kernel's rows equal the whole
    call's (and the reference's) bits."""
    n, frame = 4099, EXP_FRAME
    whole = {"walk": gpu_walk(L, n, 0, frame, 1.0, 16.0), "cv": gpu_cv(L, n, 0, frame, 16.0),
             "angle": gpu_angle(L, n, 0, frame)[None], "s3": gpu_search(L, n, 0, n, frame, 16.0, 320, 224, 3),
             "s5": gpu_search(L, n, 0, n, frame, -16.0, 320, 224, 5)}
    same(whole["walk"], ref_walk(n, 0, frame, 1.0, 16.0))
    same(whole["angle"][0], ref_angle(n, 0, frame))
    parts = {k: [] for k in whole}
    for b, m in ((0, 1500), (1500, 2), (1502, 2597)):
        parts["walk"].append(gpu_walk(L, m, b, frame, 1.0, 16.0, ld=m + 5))
        parts["cv"].append(gpu_cv(L, m, b, frame, 16.0, ld=m + 3))
        parts["angle"].append(gpu_angle(L, m, b, frame)[None])
        parts["s3"].append(gpu_search(L, m, b, n, frame, 16.0, 320, 224, 3, ld=m + 7))
        parts["s5"].append(gpu_search(L, m, b, n, frame, -16.0, 320, 224, 5, ld=m + 1))
    for k in whole:
        same(np.concatenate(parts[k], axis=1), whole[k], k)


# =========================================================================================== 2. hunted counters
def _windows(gi, last=False):
    """The n = 1 call at gi and the n = 3 window around it (ending at gi when gi must stay the last particle)."""
    w = [(gi, 1)]
    if last and gi >= 2:
        w.append((gi - 2, 3))
    elif not last and gi >= 1:
        w.append((gi - 1, 3))
    return w


@gpu
@pytest.mark.parametrize("c3", [0, 1, 2, 3])
def test_hunted_counters(L, c3):
    """Every HUNTED entry of counter kind c3 through the kernels that read that counter, at the transparent
    parameters, on the one-particle window and the three-particle window around it. Kind 0 (S2's noise): vpf_predict
    under both signs and |sig_s| in {1, 16}, vpf_predict_cv, vpf_predict_search; 1: vpf_predict_cv; 2:
    vpf_predict_angle; 3: vpf_predict_search with the particle in the last band (and, for word 0, the last column),
    where u -> 1 must clamp to W - 1 / H - 1 as s16_reference says."""
    entries = [e for e in HUNTED if e[3] == c3]
    assert len(entries) >= 8
    for seed, frame, _, _, gi, word, cls in entries:
        tag = f"{cls} word {word} frame {frame} gi {gi}"
        if c3 == 3:
            P, W, H = X.search_geometry(gi, word)
            for gb, n in _windows(gi, last=True):
                for rows in (3, 5):
                    ref = ref_search(n, gb, P, frame, 1.0, W, H, rows)
                    same(gpu_search(L, n, gb, P, frame, 1.0, W, H, rows), ref, tag)
                    if cls == "u_hi":
                        assert ref[word, -1] == f32((W, H)[word]) - f32(1.0), tag
            continue
        for gb, n in _windows(gi):
            if c3 == 0:
                for sig, sig_s in ((1.0, 1.0), (-1.0, -1.0), (1.0, 16.0), (-1.0, -16.0)):
                    same(gpu_walk(L, n, gb, frame, sig, sig_s), ref_walk(n, gb, frame, sig, sig_s), tag)
                same(gpu_search(L, n, gb, 4099, frame, 1.0, 320, 224, 3),
                     ref_search(n, gb, 4099, frame, 1.0, 320, 224, 3), tag)
            if c3 in (0, 1):
                same(gpu_cv(L, n, gb, frame), ref_cv(n, gb, frame), tag)
            if c3 == 2:
                same(gpu_angle(L, n, gb, frame), ref_angle(n, gb, frame), tag)


HIGH = [((1 << 32) - 1 - 300, 300), ((1 << 31) - 128, 257)]


@gpu
@pytest.mark.parametrize("gb,n", HIGH)
def test_high_global_indices(L, gb, n):
    """The predict kernels ending at global_begin + n = 2^32 - 1, the contract's last index, and straddling 2^31."""
    for sig in (1.0, -1.0):
        same(gpu_walk(L, n, gb, 5, sig, sig), ref_walk(n, gb, 5, sig, sig))
    same(gpu_cv(L, n, gb, 5), ref_cv(n, gb, 5))
    same(gpu_angle(L, n, gb, 5), ref_angle(n, gb, 5))


@gpu
def test_an_index_past_the_contract_is_refused_and_writes_nothing(L):
    n, gb = 300, (1 << 32) - 300
    assert gb + n == 1 << 32
    same(gpu_walk(L, n, gb, 5, 1.0, 1.0, expect=-1), _rows(3, n, n))
    same(gpu_cv(L, n, gb, 5, expect=-1), _rows(5, n, n))
    same(gpu_angle(L, n, gb, 5, expect=-1), _rows(1, n, n, ones=())[0])
    same(gpu_walk(L, n, gb - 1, 5, 1.0, 1.0)[:, -1:], ref_walk(1, (1 << 32) - 2, 5, 1.0, 1.0))


# =========================================================================================== 3. the stats tree's order
def _layout(Q, p, G, pad):
    """The global view of Q int64[P] and rows float32[R][P] as G shards; pad: q_stride, ld and p_stride larger than they
    need be, the gaps filled with values that would show if read (NaN, a huge weight)."""
    P, R_ = Q.shape[0], p.shape[0]
    n = P // G
    assert n * G == P
    ld = n + (3 if pad else 0)
    qs = n + (5 if pad else 0)
    ps = R_ * ld + (7 if pad else 0)
    Qb = np.full((G - 1) * qs + n + (2 if pad else 0), 1 << 60, np.int64)
    pb = np.full((G - 1) * ps + (R_ - 1) * ld + n + (2 if pad else 0), np.nan, np.float32)
    for r in range(G):
        Qb[r * qs: r * qs + n] = Q[r * n:(r + 1) * n]
        for c in range(R_):
            pb[r * ps + c * ld: r * ps + c * ld + n] = p[c, r * n:(r + 1) * n]
    return torch.from_numpy(Qb).to(DEV), qs, torch.from_numpy(pb).to(DEV), ld, ps, n


def _outs(P, n):
    return (torch.full((n,), -1, device=DEV, dtype=torch.int32), torch.full((3, n), SENT, device=DEV),
            torch.full((P,), -1, device=DEV, dtype=torch.int64), torch.full((8,), -1, device=DEV, dtype=torch.int64),
            torch.full((n,), -1, device=DEV, dtype=torch.int64))


def run_plain(view, P, seed, frame, b, e):
    anc, st, cdf, stats, _ = _outs(P, e - b)
    vpf().estimate_resample(*view, P, seed, frame, b, e, anc, st, cdf, stats)
    return anc.cpu().numpy(), st.cpu().numpy(), cdf.cpu().numpy(), stats.cpu().numpy(), None


def run_ex(view, P, seed, frame, b, e, method, tau, K):
    anc, st, cdf, stats, carry = _outs(P, e - b)
    vpf().estimate_resample_ex(*view, P, seed, frame, b, e, anc, st, cdf, stats, METHODS[method],
                               -1.0 if tau is None else tau, K, carry)
    return anc.cpu().numpy(), st.cpu().numpy(), cdf.cpu().numpy(), stats.cpu().numpy(), carry.cpu().numpy()


def run_gate(view, P, seed, frame, b, e, method, K, gq):
    anc, st, cdf, stats, carry = _outs(P, e - b)
    vpf().estimate_resample_gate(*view, P, seed, frame, b, e, anc, st, cdf, stats, METHODS[method], K, gq, carry)
    return anc.cpu().numpy(), st.cpu().numpy(), cdf.cpu().numpy(), stats.cpu().numpy(), carry.cpu().numpy()


def sum_bits(r, rows=3):
    return [f64_bits(s) for s in r["sums"][:rows]] + [0] * (3 - rows)


@gpu
@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 2049, 5000])
def test_tree_order_bit_for_bit_through_every_entry_point(L, P):
    """T and the bits of the three fp64 sums equal pf_exact_reference.tree_sums for vpf_shard_stats,
    vpf_estimate_resample, _ex, _gate (held: the every-weight-1 sums; not held) and vpf_weighted_sums with 1, 2 and 3
    rows, over one shard and (where 4 divides P) four padded shards. The data is order-sensitive: the reference's sums
    differ in bits from the index-order sums (asserted here from the reference and the oracle alone)."""
    Q, rows = X.order_case(P)
    ref, uni = X.tree_sums(Q, rows), X.tree_sums([1] * P, rows)
    if P > 1:
        assert all(f64_bits(a) != f64_bits(b) for a, b in zip(ref["sums"], opf.shard_stats(Q, rows)[1]))
    m, K = ref["m"], 40
    for G in (1, 4):
        if P % G:
            continue
        view = _layout(Q, rows, G, G > 1)
        Qd, qs, pd, ld, ps, n = view
        tag = f"P={P} G={G}"
        for r in range(G):                                    # vpf_shard_stats reduces one shard's flat arrays
            part = X.tree_sums(Q[r * n:(r + 1) * n], rows[:, r * n:(r + 1) * n])
            oT = torch.full((1,), -1, device=DEV, dtype=torch.int64)
            oS = torch.full((3,), -1.0, device=DEV, dtype=torch.float64)
            assert L.vpf_shard_stats(Qd[r * qs:].data_ptr(), pd[r * ps:].data_ptr(), ld, n, oT.data_ptr(),
                                     oS.data_ptr(), _stream()) == 0
            assert int(oT[0]) == part["T"] and oS.view(torch.int64).tolist() == sum_bits(part), (tag, r)
        got = run_plain(view, P, SEED, 9, 0, P)[3]
        assert got[:4].tolist() == [ref["T"]] + sum_bits(ref), tag
        got = run_ex(view, P, SEED, 9, 0, P, R10.STRATIFIED, None, K)[3]
        assert got[:4].tolist() == [ref["T"]] + sum_bits(ref) and got[6] == m, tag
        got = run_gate(view, P, SEED, 9, 0, P, R10.SYSTEMATIC, K, m)[3]
        assert got[:4].tolist() == [ref["T"]] + sum_bits(ref) and got[7] == 0, tag
        got = run_gate(view, P, SEED, 9, 0, P, R10.SYSTEMATIC, K, m + 1)[3]
        assert got[:4].tolist() == [ref["T"]] + sum_bits(uni) and got[7] == 1, tag
        for n_rows in (1, 2, 3):
            out = torch.full((4,), -1, device=DEV, dtype=torch.int64)
            vpf().weighted_sums(Qd, qs, pd, ld, ps, n, P, n_rows, out)
            assert out.tolist() == [ref["T"]] + sum_bits(ref, n_rows), (tag, n_rows)
    zero = np.zeros(P, np.int64)                              # T == 0: the uniform pass, in the same order
    view = _layout(zero, rows, 1, False)
    assert run_plain(view, P, SEED, 9, 0, P)[3][:4].tolist() == [0] + sum_bits(uni)
    out = torch.full((4,), -1, device=DEV, dtype=torch.int64)
    vpf().weighted_sums(view[0], view[1], view[2], view[3], view[4], view[5], P, 3, out)
    assert out.tolist() == [0] + sum_bits(uni)


# =========================================================================================== 4. the integer bound
def _bound_weights(kind, P, K, rng):
    Q = np.zeros(P, np.int64)
    if kind == "full":
        Q[:] = 1 << K
    elif kind == "random":
        Q = rng.integers(0, (1 << K) + 1, P, dtype=np.int64)
        Q[P // 2] = 1 << K
    else:
        Q[P // 3] = (1 << K) - 7
        Q[(2 * P) // 3] = 3 << (K - 20)
    return Q


@gpu
@pytest.mark.parametrize("kind", ["full", "random", "two"])
@pytest.mark.parametrize("P,K", [(4096, 50), (4097, 49), (1000, 52)])
def test_at_the_integer_bound(L, P, K, kind):
    """K + ceil(log2 P) = 62: T up to 2^62, S2 up to 2^112. T, the CDF, ancestors, states, carries, the ess bits, the
    flag and m equal s10_reference.step (Python ints), the sums' bits tree_sums; both schemes, the ESS gate off and
    0.5, one shard and two padded shards."""
    assert K + (P - 1).bit_length() == 62
    rng = np.random.default_rng(P + K)
    Q = _bound_weights(kind, P, K, rng)
    p = rng.uniform(0, 224, (3, P)).astype(np.float32)
    tree = X.tree_sums(Q, p)
    cdf_ref = list(itertools.accumulate(int(q) for q in Q))
    assert cdf_ref[-1] == tree["T"] <= 1 << 62 and (kind != "full" or tree["T"] == P << K)
    flags = set()
    views = {G: _layout(Q, p, G, G > 1) for G in (1, 2) if P % G == 0}
    for method in METHODS:
        for tau in (None, 0.5):
            ref = R10.step(Q, p, SEED, 9, method, tau, K)
            flags.add(ref["resampled"])
            assert ref["T"] == tree["T"] and ref["m"] == tree["m"]
            for G, view in views.items():
                n = P // G
                for r in range(G):
                    b = r * n
                    anc, st, cdf, stats, carry = run_ex(view, P, SEED, 9, b, b + n, method, tau, K)
                    tag = f"{method} tau={tau} G={G} shard {r}"
                    assert np.array_equal(anc, ref["anc"][b:b + n]), tag
                    assert np.array_equal(bits(st), bits(ref["states"][:, b:b + n])), tag
                    assert carry.tolist() == [int(c) for c in ref["carry"][b:b + n]], tag
                    assert stats.tolist() == [ref["T"]] + sum_bits(tree) + [
                        f64_bits(ref["ess"]), int(ref["resampled"]), ref["m"], 0], tag
                    assert cdf.tolist() == cdf_ref, tag
            if tau is None and method == R10.SYSTEMATIC:
                anc, st, cdf, stats, _ = run_plain(views[1], P, SEED, 9, 0, P)
                assert np.array_equal(anc, ref["anc"]) and np.array_equal(bits(st), bits(ref["states"]))
                assert stats[:4].tolist() == [ref["T"]] + sum_bits(tree) and cdf.tolist() == cdf_ref
    assert flags == ({True} if kind == "two" else {True, False})    # full: ess == P; random: ess about 0.75 P


@gpu
def test_mode_density_of_two_to_the_62(L):
    """P = 4096 weights of 2^50 in one window: every density is 2^62 exactly; vpf_mode_estimate equals s17_reference."""
    P, K = 4096, 50
    rng = np.random.default_rng(62)
    st = np.stack([100 + rng.integers(0, 17, P) / 4, 90 + rng.integers(0, 17, P) / 4,
                   rng.integers(8, 32, P) / 16]).astype(np.float32)
    Q = np.full(P, 1 << K, np.int64)
    ref = R17.mode(Q, st, f32(8.0), f32(8.0), False)
    assert ref["D"].tolist() == [1 << 62] * P and ref["i"] == 0 and ref["Tm"] == 1 << 62
    stats = torch.tensor([1 << 62] + [-1] * 7, device=DEV, dtype=torch.int64)
    dens = torch.full((P,), -1, device=DEV, dtype=torch.int64)
    out = torch.full((8,), -1, device=DEV, dtype=torch.int64)
    vpf().mode_estimate(*_layout(Q, st, 1, False), P, 0, 8.0, 8.0, stats, False, dens, out)
    assert dens.tolist() == ref["D"].tolist() and out.tolist() == R17.out_words(ref).tolist()


# =========================================================================================== 5. ties on a real CDF
@gpu
@pytest.mark.parametrize("P", [33, 4097])
def test_ties_between_positions_and_a_real_cdf(L, P):
    """Weights in {0, 1, 2, 3} with T = 2 P: pos_j lands on a CDF value in at least a quarter of the slots (asserted from
    the reference), where `>` and `>=` choose different ancestors and a run of zero weights sits right at the tie.
    vpf_resample with U given, vpf_estimate_resample and _ex under both schemes: ancestors and states equal the
    reference, and no zero-weight particle is ever an ancestor."""
    Q = X.tie_weights(P)
    rng = np.random.default_rng(P)
    p = rng.uniform(0, 224, (3, P)).astype(np.float32)
    Qd, pd = torch.from_numpy(Q).to(DEV), torch.from_numpy(p).to(DEV)
    for U in (0, 1 << 31, (1 << 32) - 1):
        assert X.tie_slots(Q, X.positions(2 * P, P, U)) * 4 >= P
        ref = X.resample(Q, U)
        anc, st, cdf, _, _ = _outs(P, P)
        vpf().resample(Qd, 0, 0, 2 * P, P, U, False, 0, P, pd, anc, st, cdf)
        anc = anc.cpu().numpy()
        assert np.array_equal(anc, ref) and (Q[anc] > 0).all(), U
        assert np.array_equal(bits(st.cpu().numpy()), bits(p[:, ref])), U
        assert cdf.cpu().tolist() == np.cumsum(Q).tolist()
    view = (Qd, P, pd.view(-1), P, 3 * P, P)
    for method in METHODS:
        assert X.tie_slots(Q, X.step_positions(Q, SEED, 9, method)) * 4 >= P
        ref = R10.step(Q, p, SEED, 9, method, None, 40)
        runs = [run_ex(view, P, SEED, 9, 0, P, method, None, 40)]
        if method == R10.SYSTEMATIC:
            runs.append(run_plain(view, P, SEED, 9, 0, P))
        for anc, st, cdf, stats, _ in runs:
            assert np.array_equal(anc, ref["anc"]) and (Q[anc] > 0).all(), method
            assert np.array_equal(bits(st), bits(ref["states"])), method
            assert stats[0] == 2 * P and cdf.tolist() == np.cumsum(Q).tolist()


# =========================================================================================== 6. small pieces
@gpu
@pytest.mark.parametrize("tau,equal", [(0.5, False), (1.0, True)])
def test_skip_carry_shifts_right_when_the_weights_outgrow_the_bits(L, tau, equal):
    """bits = 8 with weights near 2^20: bitlen(m) - 1 > bits, so the skipped frame's carry is Q >> (bitlen(m) - 9), the
    sh < 0 branch. Near-equal weights skip at tau = 0.5; exactly equal ones (ess == P) also at tau = 1."""
    P, K = 1000, 8
    rng = np.random.default_rng(8)
    Q = np.full(P, 1 << 20, np.int64) if equal else rng.integers((1 << 20) - 4096, (1 << 20) + 1, P, dtype=np.int64)
    p = rng.uniform(0, 224, (3, P)).astype(np.float32)
    for method in METHODS:
        ref = R10.step(Q, p, SEED, 9, method, tau, K)
        sh = K + 1 - ref["m"].bit_length()
        assert not ref["resampled"] and sh < 0 and ref["carry"].tolist() == [int(q) >> -sh for q in Q]
        anc, st, _, stats, carry = run_ex(_layout(Q, p, 1, False), P, SEED, 9, 0, P, method, tau, K)
        assert carry.tolist() == ref["carry"].tolist() and np.array_equal(anc, np.arange(P))
        assert np.array_equal(bits(st), bits(p)) and stats[5] == 0 and stats[6] == ref["m"]
        assert stats[4] == f64_bits(ref["ess"])


@gpu
@pytest.mark.parametrize("n_rows", [1, 8])
def test_gather_rows_leaves_the_slots_of_out_of_range_ancestors(L, n_rows):
    """Ancestors -1, P and 2^31 - 1 among valid ones: those slots keep the sentinel, every other slot is exact."""
    P, nsh, G = 12, 4, 3
    ld, ps = 5, n_rows * 5 + 3
    flat = np.arange(G * ps, dtype=np.float32) + 0.5
    anc = np.array([3, -1, 0, P, P - 1, (1 << 31) - 1, 7, -(1 << 31), P + 1, 11] + list(range(P)) * 25, np.int32)
    out = torch.full((n_rows + 1, anc.size + 2), SENT, device=DEV)
    vpf().gather_rows(torch.from_numpy(anc).to(DEV), torch.from_numpy(flat).to(DEV), ld, ps, nsh, P, n_rows, out)
    got = out.cpu().numpy()
    a = anc.astype(np.int64)
    ok = (a >= 0) & (a < P)
    assert (~ok).sum() == 5
    want = np.full_like(got, SENT)
    for c in range(n_rows):
        want[c, :anc.size][ok] = flat[(a[ok] // nsh) * ps + c * ld + a[ok] % nsh]
    assert np.array_equal(bits(got), bits(want))
