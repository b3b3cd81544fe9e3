"""CPU: exactly computable operands for the bf16 / fp32 GEMM family (shared with tests/test_gpu_gemm_exact.py, which
imports this module), their references, and the proofs that the bars set on them are fair.

The GEMMs are C = epi(A[M][K] W[N][K]^T) with fp32 accumulation and the epilogues of include/vpf.h. Gaussian data
against rtol 1.6e-2 cannot see one misrouted element of a long dot product, a bias taken from the neighbouring 4-column
fragment, a dropped statistics plane or a wrong rounding tie. Three operand families make every output exact instead.

Dense exact operands. A and W are integers in [-4, 4] (exact in bf16), bias integers in [-384, 384], colsum and pos
integers in [-8, 8], the residual integers in [-64, 64], {mean, rstd} per row {integer in [-3, 3], 2^-(m % 4)}. Every
partial sum of a dot product is an integer of magnitude <= 16 K < 2^24, so the fp32 accumulator is exact whatever the
order of accumulation (K order, MFMA internals, split-K); the epilogue's adds and fmas act on multiples of 1/8 below
2^21 and are exact too. The only rounding left is the bf16 round-to-nearest-even of an exact value (twice for the
residual and patch epilogues: bf16(bf16(acc + b) + r)), and the bias range puts a large share of the outputs above 256,
where integers need rounding and odd ones are exact ties. The statistics planes of a producer ({sum, sumsq} of the
stored integers per 64 columns) are integers below 2^24: exact in fp32 in any order.

Coded operands switch the product off (A = 0) and give every epilogue operand a value that names its index:
code(i) = +-(1 + (i & 127) / 128) 2^((i >> 7) & 3), an 8-bit significand (exact in bf16), distinct over 512
consecutive indices. bias, colsum and the pos rows are coded by column, mean and the residual by row. The references
below reproduce the kernels' fp32 operation order (fma(rstd, acc, fma(-rstd mean, colsum, bias)), one rounding per
fma), so a coded output is one exactly known bf16 value and an operand read from a neighbouring column, row, fragment
or tile changes bits.

Planes form. The LN epilogues may take their row statistics as P planes of {sum, sumsq}; the kernel combines them as
mean = sum / K, rstd = rsq(sumsq / K - mean^2 + eps). Row m's sum = K mean goes to plane m % P, its
sumsq = K (var + mean^2) to plane (m + 1) % P, every other plane is 0 and eps = 0: every plane and both of its
components decide some row (a dropped sum gives mean 0, a dropped sumsq gives var 0 and rstd = inf). The combine is
not exact (1 / K is rounded, var cancels, rsq is good to 1 ulp), so bit equality needs outputs that are bf16 values
with room around them: A = 0, bias = 0, mean coded, var = 1 and power-of-two colsums make the ideal output
-mean colsum, an 8-bit significand, which everything within 2^-9 relative rounds to.
test_planes_form_combine_is_fair emulates the combine in fp32 (with rsq off by -1, 0, +1 ulp) and asserts both that
rounding and a deviation below 2^-12. On the dense operands the planes form is held to the interval that deviation
allows (dense_planes_slack): the bf16 roundings of [y - slack, y + slack], which is bit equality except at ties.

GELU epilogues. gelu_sig2 is approximate by design; its bar is the project's own (test_gemm_bf16_gelu_accuracy):
|out - gelu(x)| <= 2.8e-4 + |gelu(x)| 2^-8 with x the exact pre-activation. The coded operands of a GELU epilogue are
positive codes gcode(i) in [0.5, 8) with 6-bit significands, one operand coded at a time with the others neutral, so
the pre-activation is the code itself; test_gelu_codes_are_separated asserts that the GELU images of any two such
codes are farther apart than the sum of their bars, so a misrouted column or row cannot pass."""
import numpy as np
import pytest
import torch

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, EPI_PATCH, EPI_LN, EPI_LN_GELU = range(6)

# (M, N, K): see tests/test_gpu_gemm_exact.py for what each one reaches in the kernels
SHAPES = [(600, 520, 256), (300, 328, 64), (257, 256, 128), (394, 64, 384), (5, 128, 320), (300, 384, 192)]
# patch rows per image (EPI_PATCH needs M % g2 == 0); 25 and 40 at M = 600 and 60 at M = 300 put images across the
# 128-row wave and 256-row tile boundaries
PATCH_G2 = {600: (25, 40), 300: (60,), 257: (257,), 394: (197,), 5: (1,)}
F32_SHAPES = [(300, 136, 32), (129, 264, 96), (5, 128, 64)]
GELU_ABS = 2.8e-4            # gelu_sig2's minimax bound (gemm_common.h)
PLANES_DEV = 2.0 ** -12      # bar on the relative deviation of the in-kernel {mean, rstd} combine


# ---- number formats --------------------------------------------------------------------------------------------------

def bf16_bits(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 round-to-nearest-even bit patterns (the project's rule, tests/test_gpu_kernels.py)."""
    u = np.asarray(x).astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(bits: np.ndarray) -> np.ndarray:
    """bf16 bit patterns -> float64 values."""
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def exact_bf16(x: np.ndarray) -> np.ndarray:
    """Bits of values that must already be bf16 values."""
    b = bf16_bits(x)
    assert np.array_equal(bf16_val(b), np.asarray(x, dtype=np.float64)), "operand is not exact in bf16"
    return b


def f32(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def gelu64(x: np.ndarray) -> np.ndarray:
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return (0.5 * t * (1.0 + torch.erf(t / 2.0 ** 0.5))).numpy()


def code(i) -> np.ndarray:
    i = np.asarray(i, dtype=np.int64)
    return np.where(i & 1, -1.0, 1.0) * (1.0 + (i & 127) / 128.0) * np.exp2((i >> 7) & 3)


def gcode(i) -> np.ndarray:
    """Positive codes in [0.5, 8) for the GELU epilogues: 6-bit significands (4 bf16 ulps apart, so that the GELU bars
    of neighbouring codes do not meet), distinct over 128 consecutive indices."""
    i = np.asarray(i, dtype=np.int64)
    return (1.0 + (i & 31) / 32.0) * np.exp2(((i >> 5) & 3) - 1.0)


# ---- operands --------------------------------------------------------------------------------------------------------

class Operands:
    """One GEMM's operands on the CPU: a / w / residual as bf16 bits, acc = A W^T in float64 (exact), the fp32
    epilogue operands, g2 (patch rows per image, or None)."""

    def __init__(self, a, w, bias, colsum, mean, rstd, residual, pos, g2):
        self.M, self.K = a.shape
        self.N = w.shape[0]
        self.a, self.w, self.residual = exact_bf16(a), exact_bf16(w), exact_bf16(residual)
        self.acc = np.asarray(a, dtype=np.float64) @ np.asarray(w, dtype=np.float64).T
        self.absacc = np.abs(np.asarray(a, dtype=np.float64)) @ np.abs(np.asarray(w, dtype=np.float64)).T
        self.bias, self.colsum, self.mean, self.rstd = f32(bias), f32(colsum), f32(mean), f32(rstd)
        for v, x in ((self.bias, bias), (self.colsum, colsum), (self.mean, mean), (self.rstd, rstd)):
            assert np.array_equal(v.astype(np.float64), np.asarray(x, dtype=np.float64))
        self.pos = None if pos is None else f32(pos)
        self.g2 = g2

    def row_stats(self) -> np.ndarray:
        return np.stack([self.mean, self.rstd], 1).astype(np.float32)


def default_g2(M):
    return PATCH_G2[M][0] if M in PATCH_G2 else None


def dense(M, N, K, g2="default") -> Operands:
    g2 = default_g2(M) if g2 == "default" else g2
    rng = np.random.default_rng(1000003 * M + 1009 * N + K)
    m = np.arange(M)
    return Operands(a=rng.integers(-4, 5, (M, K)), w=rng.integers(-4, 5, (N, K)),
                    bias=rng.integers(-384, 385, N), colsum=rng.integers(-8, 9, N),
                    mean=rng.integers(-3, 4, M), rstd=np.exp2(-(m % 4).astype(np.float64)),
                    residual=rng.integers(-64, 65, (M, N)),
                    pos=None if g2 is None else rng.integers(-8, 9, (g2 + 1, N)), g2=g2)


def coded(M, N, K, g2="default") -> Operands:
    """A = 0; bias, colsum, pos coded by column, mean and the residual by row; rstd = 2^-(m % 4)."""
    g2 = default_g2(M) if g2 == "default" else g2
    rng = np.random.default_rng(7 * M + N + K)
    m, n = np.arange(M), np.arange(N)
    pos = None if g2 is None else code(n[None, :] + 37 * np.arange(g2 + 1)[:, None] + 11)
    return Operands(a=np.zeros((M, K)), w=rng.integers(-4, 5, (N, K)), bias=code(n), colsum=code(n + 200),
                    mean=code(m + 100), rstd=np.exp2(-(m % 4).astype(np.float64)),
                    residual=code(7 * m[:, None] + n[None, :]), pos=pos, g2=g2)


GELU_CODED = ("bias", "colsum", "mean", "rstd")


def coded_gelu(M, N, K, which) -> Operands:
    """A = 0 and one epilogue operand = gcode of its index, the others neutral, so that the pre-activation of every
    output is that code: bias (also for BIAS_GELU), colsum (mean = -1), mean (colsum = -1), rstd (mean = -1,
    colsum = 1)."""
    rng = np.random.default_rng(M + 7 * N + K)
    m, n = np.arange(M), np.arange(N)
    one_m, one_n = np.ones(M), np.ones(N)
    bias, colsum, mean, rstd = 0 * one_n, 0 * one_n, 0 * one_m, one_m
    if which == "bias":
        bias, mean = gcode(n), 3 * one_m
    elif which == "colsum":
        colsum, mean = gcode(n + 200), -one_m
    elif which == "mean":
        colsum, mean = -one_n, gcode(m + 100)
    else:
        colsum, mean, rstd = one_n, -one_m, gcode(m + 300)
    return Operands(a=np.zeros((M, K)), w=rng.integers(-4, 5, (N, K)), bias=bias, colsum=colsum, mean=mean, rstd=rstd,
                    residual=np.zeros((M, N)), pos=None, g2=None)


def coded_planes(M, N, K) -> Operands:
    """The planes form's coded operands: A = 0, bias = 0, mean coded by row, var = 1 (rstd = 1), colsum a signed power
    of two by column: the ideal output -mean colsum is a bf16 value."""
    rng = np.random.default_rng(3 * M + N + 5 * K)
    m, n = np.arange(M), np.arange(N)
    colsum = np.where(n & 1, -1.0, 1.0) * np.exp2((n >> 1) % 4 - 1.0)
    return Operands(a=np.zeros((M, K)), w=rng.integers(-4, 5, (N, K)), bias=np.zeros(N), colsum=colsum,
                    mean=code(m + 100), rstd=np.ones(M), residual=np.zeros((M, N)), pos=None, g2=None)


def gcoded_planes(M, N, K) -> Operands:
    """coded_planes for LN_GELU: mean = -gcode(row), colsum = 2^(n % 3) > 0, so the pre-activation is
    gcode(row) 2^(n % 3) > 0."""
    o = coded_planes(M, N, K)
    n = np.arange(N)
    return Operands(a=np.zeros((M, K)), w=bf16_val(o.w), bias=np.zeros(N), colsum=np.exp2(n % 3),
                    mean=-gcode(np.arange(M) + 100), rstd=np.ones(M), residual=np.zeros((M, N)), pos=None, g2=None)


def planes_form(mean, rstd, K, P) -> np.ndarray:
    """fp32 [P][M][2]: row m's sum = K mean in plane m % P, its sumsq = K (1 / rstd^2 + mean^2) in plane
    (m + 1) % P, zeros elsewhere (ln_eps = 0). Both are exact in fp32 for the operands of this module."""
    mean, var = np.asarray(mean, dtype=np.float64), 1.0 / np.asarray(rstd, dtype=np.float64) ** 2
    M = mean.shape[0]
    m = np.arange(M)
    pl = np.zeros((P, M, 2))
    pl[m % P, m, 0] = K * mean
    pl[(m + 1) % P, m, 1] = K * (var + mean * mean)
    out = pl.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), pl), "plane entries must be exact in fp32"
    return out


# ---- references ------------------------------------------------------------------------------------------------------

def ln_pre(acc, mean, rstd, colsum, bias) -> np.ndarray:
    """The LN fold in the kernels' fp32 operation order: fma(rstd, acc, fma(-rstd mean, colsum, bias)), each fma one
    rounding (float64 holds the exact product-sum of these operands). fp32 [M][N]."""
    nrm = (-f32(rstd)) * f32(mean)
    inner = (nrm.astype(np.float64)[:, None] * colsum.astype(np.float64)[None, :]
             + bias.astype(np.float64)[None, :]).astype(np.float32)
    return (f32(rstd).astype(np.float64)[:, None] * acc + inner.astype(np.float64)).astype(np.float32)


def pre_activation(o: Operands, epi, mean=None, rstd=None) -> np.ndarray:
    """fp32 [M][N]: the value the epilogue rounds to bf16 (BIAS, LN), feeds to the GELU, or rounds and adds to."""
    if epi in (EPI_LN, EPI_LN_GELU):
        return ln_pre(o.acc, o.mean if mean is None else mean, o.rstd if rstd is None else rstd, o.colsum, o.bias)
    return (o.acc + o.bias.astype(np.float64)[None, :]).astype(np.float32)


def want_bits(o: Operands, epi) -> np.ndarray:
    """bf16 bits [M][N] of the non-GELU epilogues (EPI_PATCH: rows in A's order; patch_rows maps them)."""
    y = bf16_bits(pre_activation(o, epi))
    if epi == EPI_BIAS_RESIDUAL:
        y = bf16_bits((bf16_val(y) + bf16_val(o.residual)).astype(np.float32))
    elif epi == EPI_PATCH:
        p = o.pos[1 + np.arange(o.M) % o.g2].astype(np.float64)
        y = bf16_bits((bf16_val(y) + p).astype(np.float32))
    return y


def want_f32(o: Operands, epi) -> np.ndarray:
    """fp32 [M][N] of vpf_gemm_f32's non-GELU epilogues (no intermediate bf16 rounding)."""
    y = pre_activation(o, epi)
    if epi == EPI_BIAS_RESIDUAL:
        y = (y.astype(np.float64) + bf16_val(o.residual)).astype(np.float32)
    elif epi == EPI_PATCH:
        y = (y.astype(np.float64) + o.pos[1 + np.arange(o.M) % o.g2].astype(np.float64)).astype(np.float32)
    return y


def patch_rows(M, g2) -> np.ndarray:
    """Output (token) row of A row m under EPI_PATCH: one CLS row ahead of every g2 patch rows."""
    m = np.arange(M)
    return (m // g2) * (g2 + 1) + 1 + m % g2


def stats_planes(bits: np.ndarray) -> np.ndarray:
    """float64 [ceil(N / 64)][M][2]: {sum, sumsq} of the stored bf16 values per 64-column block."""
    v = bf16_val(bits)
    M, N = v.shape
    P = (N + 63) // 64
    pad = np.zeros((M, P * 64))
    pad[:, :N] = v
    blk = pad.reshape(M, P, 64)
    return np.stack([blk.sum(2).T, (blk * blk).sum(2).T], 2)


def gelu_bar(pre, slack=0.0):
    """(reference, bound) of a GELU epilogue on the exact pre-activation `pre`; `slack` = what the pre-activation itself
    may deviate by (planes form), times the GELU's largest slope 1.13."""
    ref = gelu64(np.asarray(pre, dtype=np.float64))
    return ref, GELU_ABS + np.maximum(np.abs(ref), 2.0 ** -126) * 2.0 ** -8 + 1.13 * slack


def dense_planes_slack(o: Operands, mean=None, rstd=None) -> np.ndarray:
    """float64 [M][N]: how far the pre-activation of an LN epilogue may move when {mean, rstd} each deviate by
    PLANES_DEV relative (rstd scales both terms, mean the second), plus the fp32 roundings of the two fmas."""
    mean = o.mean if mean is None else mean
    rstd = o.rstd if rstd is None else rstd
    t1 = np.abs(rstd.astype(np.float64)[:, None] * o.acc)
    t2 = np.abs((rstd * mean).astype(np.float64)[:, None] * o.colsum.astype(np.float64)[None, :])
    return PLANES_DEV * t1 + 2 * PLANES_DEV * t2 + 2.0 ** -22 * (t1 + t2 + np.abs(o.bias)[None, :])


def interval_bits(y, slack):
    """bf16 values (float64) of y - slack and y + slack: rounding is monotonic, so a value within slack of y rounds
    into [lo, hi]."""
    y = np.asarray(y, dtype=np.float64)
    return bf16_val(bf16_bits((y - slack).astype(np.float32))), bf16_val(bf16_bits((y + slack).astype(np.float32)))


def emulate_combine(planes: np.ndarray, K, eps=0.0, rsq_ulps=0):
    """combine_planes (gemm_common.h) in fp32: planes summed in order, mean = sum (1 / K), var =
    max(fma(sumsq, 1 / K, -mean mean), 0), rstd = rsq(var + eps) correctly rounded and then moved by rsq_ulps ulps."""
    sm = np.zeros(planes.shape[1], np.float32)
    sq = np.zeros(planes.shape[1], np.float32)
    for p in range(planes.shape[0]):
        sm = sm + planes[p, :, 0]
        sq = sq + planes[p, :, 1]
    inv_k = np.float32(1.0) / np.float32(K)
    mean = sm * inv_k
    mm = mean * mean
    var = np.maximum((sq.astype(np.float64) * np.float64(inv_k) - mm.astype(np.float64)).astype(np.float32),
                     np.float32(0))
    with np.errstate(divide="ignore"):
        rstd = (1.0 / np.sqrt((var + np.float32(eps)).astype(np.float64))).astype(np.float32)
    for _ in range(abs(rsq_ulps)):
        rstd = np.nextafter(rstd, np.float32(np.inf if rsq_ulps > 0 else 0))
    return mean.astype(np.float32), rstd


# ---- failure reports -------------------------------------------------------------------------------------------------

def _show(v) -> str:
    if isinstance(v, np.uint16):
        return f"0x{int(v):04x} ({float(bf16_val(np.array([v]))[0])!r})"
    if isinstance(v, np.uint32):
        return f"0x{int(v):08x} ({float(np.array([v]).view(np.float32)[0])!r})"
    return repr(float(v))


def diff_report(bad: np.ndarray, got, want, tile=(256, 256), sub=(128, 64)) -> str:
    """Where a comparison failed: count, first (row, col) with got / want, counts per output tile and per wave
    sub-tile (row, col indices of the tiles; the first 32 that hold a difference)."""
    idx = np.argwhere(bad)
    r, c = idx[0]
    lines = [f"{len(idx)} of {bad.size} outputs differ; first at (row {r}, col {c}): got {_show(got[r, c])}, "
             f"want {_show(want[r, c])}"]
    for name, (th, tw) in (("tile", tile), ("wave sub-tile", sub)):
        keys, cnt = np.unique(np.stack([idx[:, 0] // th, idx[:, 1] // tw], 1), axis=0, return_counts=True)
        shown = ", ".join(f"({a},{b}): {n}" for (a, b), n in list(zip(keys, cnt))[:32])
        more = f", ... ({len(keys) - 32} more)" if len(keys) > 32 else ""
        lines.append(f"per {th}x{tw} {name}: {shown}{more}")
    return "\n".join(lines)


def require(bad: np.ndarray, message) -> None:
    """Fail with message() when any element of `bad` is set."""
    if bad.any():
        raise AssertionError(message())


# ---- fairness proofs -------------------------------------------------------------------------------------------------

def _rounding_census(pre32):
    """(share of values that are not bf16 values, share that are exact ties) of fp32 values."""
    u = pre32.astype(np.float32).view(np.uint32)
    low = u & 0xFFFF
    return float((low != 0).mean()), float((low == 0x8000).mean())


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dense_operands_make_bit_equality_fair(M, N, K):
    """The dense operands: every partial sum is an integer below 2^24 whatever the order (the sum of the magnitudes
    is), every epilogue value is a multiple of 1/8 below 2^21 (exact through fp32 adds and fmas, so the fp32-ordered
    references equal plain float64), a useful share of the outputs needs rounding with exact ties among them, the
    outputs are not degenerate, and the producers' statistics are integers below 2^24."""
    o = dense(M, N, K)
    assert np.abs(bf16_val(o.a)).max() == 4 and np.abs(bf16_val(o.w)).max() == 4
    assert o.absacc.max() <= 16 * K < 2 ** 24 and 4 * 4 * 3072 < 2 ** 24
    assert np.array_equal(o.acc, np.round(o.acc))
    mean, rstd = o.mean[:, None].astype(np.float64), o.rstd[:, None].astype(np.float64)
    plain = {EPI_BIAS: o.acc + o.bias[None, :].astype(np.float64),
             EPI_LN: rstd * (o.acc - mean * o.colsum[None, :]) + o.bias[None, :]}
    for epi in (EPI_BIAS, EPI_LN):
        pre = pre_activation(o, epi)
        assert np.array_equal(pre.astype(np.float64), plain[epi])           # nothing was rounded on the way
        assert np.array_equal(pre * 8, np.round(pre * 8)) and np.abs(pre).max() < 2 ** 21
        inexact, ties = _rounding_census(pre)
        if M * N >= 4096:
            assert inexact >= 0.10 and ties >= 0.02, (epi, inexact, ties)
        assert len(np.unique(bf16_bits(pre))) >= min(M * N // 4, 200)
    # second rounding of the residual / patch epilogues: exact integer sums, again with ties
    for epi in (EPI_BIAS_RESIDUAL, EPI_PATCH):
        first = bf16_val(bf16_bits(pre_activation(o, epi)))
        add = bf16_val(o.residual) if epi == EPI_BIAS_RESIDUAL else o.pos[1 + np.arange(M) % o.g2].astype(np.float64)
        s = first + add
        assert np.array_equal(s, np.round(s)) and np.abs(s).max() < 2 ** 24
        inexact, ties = _rounding_census(s.astype(np.float32))
        if M * N >= 4096:
            assert inexact >= 0.05 and ties >= 0.01, (epi, inexact, ties)
        pl = stats_planes(want_bits(o, epi))
        assert np.array_equal(pl, np.round(pl)) and pl[..., 1].max() < 2 ** 24
        assert (pl[..., 1] > 0).all() and len(np.unique(pl[..., 0])) > min(M, 16)
    # the GELU epilogues see both branches and the curved part
    pre = pre_activation(o, EPI_LN_GELU)
    assert (pre > 10).mean() > 0.1 and (pre < -10).mean() > 0.1 and (np.abs(pre) < 3).sum() >= min(M * N // 200, 50)


def test_f32_dense_operands_are_exact():
    """vpf_gemm_f32 on the dense operands (held as fp32): same integers, so fp32 bit equality is exact arithmetic."""
    for M, N, K in F32_SHAPES:
        o = dense(M, N, K, g2=1)
        for epi in (EPI_BIAS, EPI_BIAS_RESIDUAL, EPI_PATCH, EPI_LN):
            y = want_f32(o, epi)
            assert np.array_equal(y * 8, np.round(y * 8)) and np.abs(y).max() < 2 ** 21
            assert len(np.unique(y)) >= min(M * N // 4, 200)


def test_codes_are_distinct_bf16_values():
    for f, span in ((code, 512), (gcode, 128)):
        c = f(np.arange(1024))
        exact_bf16(c)
        for start in (0, 100, 200, 300, 512):
            assert len(np.unique(c[start:start + span])) == span
    assert gcode(np.arange(512)).min() == 0.5 and gcode(np.arange(512)).max() < 8


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_coded_operands_name_their_index(M, N, K):
    """A = 0: every output is decided by the epilogue operands alone, and an operand taken from another column
    or row gives other bits. EPI_BIAS stores the bias codes themselves: all columns of a 256-column tile differ. The
    other epilogues round a sum of codes, which may collide here and there: an output differs from the one 1, 4, 8,
    16 or 64 columns away (piece, fragment, lane and wave distances) and 1, 2, 16 or 128 rows away in more than half
    of the places."""
    o = coded(M, N, K)
    assert not o.acc.any()
    for epi in (EPI_BIAS, EPI_BIAS_RESIDUAL, EPI_PATCH, EPI_LN):
        y = want_bits(o, epi).astype(np.int64)
        if epi == EPI_BIAS:
            for lo in range(0, N, 256):
                assert len(np.unique(y[0, lo:lo + 256])) == min(256, N - lo)
            continue
        for d in (1, 4, 8, 16, 64):
            if d < N:
                assert (y[:, d:] != y[:, :-d]).mean() > 0.5, (epi, d)
        for d in (1, 2, 16, 128):
            if d < M and not (epi == EPI_PATCH and o.g2 == 1):   # g2 = 1: every row adds pos row 1
                assert (y[d:] != y[:-d]).mean() > 0.5, (epi, d)


def test_gelu_codes_are_separated():
    """Any two distinct codes of gcode's 128 have GELU images farther apart than the sum of their bars, so a GELU
    output within its bar of one code's image is outside every other code's."""
    c = np.sort(gcode(np.arange(128)))
    ref, bar = gelu_bar(c)
    assert np.all(np.diff(ref) > 0)
    assert np.all(np.diff(ref) > bar[:-1] + bar[1:]), float((np.diff(ref) - bar[:-1] - bar[1:]).min())
    for M, N, K in SHAPES:
        for which in GELU_CODED:
            o = coded_gelu(M, N, K, which)
            pre = pre_activation(o, EPI_LN_GELU).astype(np.float64)
            want = gcode(np.arange(N) + (200 if which == "colsum" else 0))[None, :].repeat(M, 0) \
                if which in ("bias", "colsum") else \
                gcode(np.arange(M) + (100 if which == "mean" else 300))[:, None].repeat(N, 1)
            assert np.array_equal(pre, want), which
        o = coded_gelu(M, N, K, "bias")
        assert np.array_equal(pre_activation(o, EPI_BIAS_GELU).astype(np.float64),
                              gcode(np.arange(N))[None, :].repeat(M, 0))


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 384, 768, 1024])
@pytest.mark.parametrize("P", [1, 3, 12, 13, 15, 16])
def test_planes_form_combine_is_fair(K, P):
    """An fp32 emulation of combine_planes on the planes form, 600 rows: with the coded operands (power-of-two
    colsums) the output deviates from the ideal -mean colsum by less than 2^-12 relative and rounds to the ideal bf16
    value, with rsq correctly rounded or 1 ulp off either way; with the dense statistics (integer mean, rstd =
    2^-(m % 4)) the combined {mean, rstd} are within 2^-12 relative of the ideal, which is what dense_planes_slack
    grants the dense outputs. Every plane holds a sum and a sumsq that decide some row."""
    M, N = 600, 64
    for o in (coded_planes(M, N, K), gcoded_planes(M, N, K)):
        pl = planes_form(o.mean, o.rstd, K, P)
        assert all(pl[p, :, 0].any() and pl[p, :, 1].any() for p in range(P))
        ideal = -o.mean.astype(np.float64)[:, None] * o.colsum.astype(np.float64)[None, :]
        want = exact_bf16(ideal)
        worst = 0.0
        for ulps in (-1, 0, 1):
            mean, rstd = emulate_combine(pl, K, 0.0, ulps)
            y = ln_pre(o.acc, mean, rstd, o.colsum, o.bias).astype(np.float64)
            worst = max(worst, float(np.abs(y / ideal - 1).max()))
            assert np.array_equal(bf16_bits(y), want), (K, P, ulps)
        assert worst < PLANES_DEV, worst
    d = dense(M, N, K)
    pl = planes_form(d.mean, d.rstd, K, P)
    for ulps in (-1, 0, 1):
        mean, rstd = emulate_combine(pl, K, 0.0, ulps)
        assert np.abs(rstd / d.rstd.astype(np.float64) - 1).max() < PLANES_DEV
        assert np.abs(mean.astype(np.float64) - d.mean).max() <= PLANES_DEV * np.abs(d.mean).max()
        assert np.all(mean[d.mean == 0] == 0)
        y = ln_pre(d.acc, mean, rstd, d.colsum, d.bias).astype(np.float64)
        assert np.all(np.abs(y - pre_activation(d, EPI_LN)) <= dense_planes_slack(d))


def test_dropped_plane_or_component_changes_bits():
    """The planes form bites: dropping any one plane, or the sumsq of plane 0, changes the coded output bits of the
    rows that plane decides (emulated combine)."""
    M, N, K = 600, 64, 256
    o = coded_planes(M, N, K)
    want = exact_bf16(-o.mean.astype(np.float64)[:, None] * o.colsum.astype(np.float64)[None, :])
    for P in (1, 12, 15, 16):
        pl = planes_form(o.mean, o.rstd, K, P)
        for drop in range(P):
            cut = pl.copy()
            cut[drop] = 0
            mean, rstd = emulate_combine(cut, K)
            with np.errstate(invalid="ignore", over="ignore"):
                got = bf16_bits(ln_pre(o.acc, mean, rstd, o.colsum, o.bias))
            assert (got != want).any(axis=1).sum() >= M // P
        cut = pl.copy()
        cut[0, :, 1] = 0
        mean, rstd = emulate_combine(cut, K)
        with np.errstate(invalid="ignore", over="ignore"):
            got = bf16_bits(ln_pre(o.acc, mean, rstd, o.colsum, o.bias))
        assert (got != want).any()
