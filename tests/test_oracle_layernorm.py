"""CPU: exactly computable operands for the LayerNorm family (shared with tests/test_gpu_layernorm_exact.py, which
imports this module), their numpy-fp32 references, and the proofs that the bars set on them are fair.

The kernels are k_layernorm, k_row_stats, k_stats_combine and k_cls_weight (csrc/layernorm.hip) and k_cls_rows /
k_cls_stats (csrc/crop.hip). Gaussian rows against rtol 1e-2 cannot see an element lost from a row's sum (it moves the
mean by 3e-3 at D = 768), a mean taken from the neighbouring row or gamma read one chunk off. The operand families
below make every output one known bit pattern instead.

Dense rows. x[c] = m + d[c]: m a non-zero multiple of 1/4 with |m| <= 12 (neighbouring rows differ), d a shuffled
multiset of +-a pairs with a in {1/4 .. 4} in steps of 1/4 (one pair is +-1). Every x is a bf16 value. Every partial
sum of x is a multiple of 1/4 below 2^14, so the fp32 row sum is exactly D m in any order and the correctly rounded
s / D is m; every d = x - m and every partial sum of d^2 (multiples of 2^-4 below 2^14) is exact, so q is one value in
any order. var = q / D is one rounding, rstd = 1 / sqrt(var + eps) three more, each a correctly rounded fp32 operation
(the file compiles without fast-math: IEEE divide and sqrt). Any dropped, duplicated or foreign element moves q by at
least 2^-4. gamma is a signed power of two coded by column, so t gamma is exact and f32(t gamma + beta) is the same
with or without contraction; beta is a 24-bit fp32 code by column. y = f32(f32(d rstd) gamma + beta), bf16 by RNE.

Coded rows. d = +-2^j uniform per row and eps = 0: var = 4^j, rstd = 2^-j and the normalised values are +-1, all
exact, so y = +-gamma[c] + beta[c]. The LayerNorm cases use gamma = a 6-bit-significand code distinct over 1024
columns and beta = gamma {-2, 0, 2}: y = gamma {+-1, +-3} is a bf16 value, so the fp32 and bf16 outputs both pin the
column that gamma and beta came from. The weight cases use gamma = +-{1, 2, 4} and integer beta: feat is a small
integer, and against a dyadic unit template (4^k entries of +-2^-k) dot and nn are exact in any order, so
sim = f32(dot / sqrtf(nn)) is two correctly rounded operations and Q = weights_to_Q(sim) is predicted, not read back.

Combine. k_stats_combine is the one kernel with an approximate instruction (v_rsq_f32): mean is bit-exact and rstd
one of emulate_combine's three candidates (rsq at -1, 0, +1 ulp), the project's existing bar (test_oracle_gemm.py).

The emulators below run the kernels' lane / chunk schedules in numpy fp32 and take mutants: each must change bits of
every case that claims to cover it."""
import numpy as np
import pytest

from test_oracle_gemm import bf16_bits, bf16_val, emulate_combine, exact_bf16

F = np.float32
EPS = 1e-6

LN_D = [4, 252, 256, 260, 768, 1020, 1024]
LN_ROWS = [1, 3, 4, 5, 9]                       # the edges of 4 rows per workgroup
STATS_D = {"bf16": [8, 248, 256, 264, 768, 1016, 1024], "f32": [4, 124, 128, 132, 768, 1020, 1024]}
STATS_ROWS = [1, 2, 7, 8, 9]
STATS_BIG_ROWS = 65545                          # > 8 * 8192: the second grid stride, ending on an odd last row
STATS_BIG_D = {"bf16": 8, "f32": 4}
STATS_GRID_ROWS = 8 * 8192                      # rows of one grid stride of k_row_stats
EPC = {"bf16": 8, "f32": 4}                     # elements per 16-byte load of k_row_stats
COMBINE_PARTS = [1, 3, 5, 12, 15, 16, 64]
COMBINE_ROWS = [1, 256, 257]
CLAMP_D = 960
CLS_D = [4, 64, 192, 320, 1024]
CLS_NPART = [1, 5, 257]
CLS_N = [1, 3]
CLS_PARTS = [1, 3, 16]
W_N = [1, 3, 4, 5, 257]
W_D = [4, 252, 260, 768, 1024]
W_TOKENS = 3
LAM, BITS = 20.0, 40


# ---- operands --------------------------------------------------------------------------------------------------------

class Rows:
    """x fp32 [rows][D] (bf16 values), with the exact mean m and deviations d (float64) they were built from."""

    def __init__(self, x, m, d):
        self.x, self.m, self.d = x, m, d
        self.bits = exact_bf16(x)

    @property
    def q(self):
        return (self.d * self.d).sum(1)


def _means(rng, rows):
    m = rng.integers(1, 49, rows) / 4.0 * rng.choice([-1.0, 1.0], rows)
    odd = np.arange(1, rows, 2)
    same = m[odd] == m[odd - 1]
    m[odd[same]] = -m[odd[same]]                # a row and its pair partner never share a mean
    return m


def dense_rows(rows, D, seed=0) -> Rows:
    rng = np.random.default_rng([1, seed, rows, D])
    a = rng.integers(1, 17, (rows, D // 2)) / 4.0
    a[:, 0] = 1.0
    d = rng.permuted(np.concatenate([a, -a], 1), axis=1)
    m = _means(rng, rows)
    return Rows((m[:, None] + d).astype(F), m, d)


def coded_rows(rows, D, seed=0) -> Rows:
    rng = np.random.default_rng([2, seed, rows, D])
    s = rng.permuted(np.repeat([[1.0, -1.0]], rows, 0).repeat(D // 2, 1), axis=1)
    d = s * np.exp2(np.arange(rows) % 5 - 2.0)[:, None]
    m = _means(rng, rows)
    return Rows((m[:, None] + d).astype(F), m, d)


FAMILIES = {"dense": (dense_rows, EPS), "coded": (coded_rows, 0.0)}


def gamma_pow2(D):
    c = np.arange(D)
    return (np.where((c ^ (c >> 6)) & 1, -1.0, 1.0) * np.exp2((c * 5 + (c >> 6)) % 7 - 3.0)).astype(F)


def beta_code(D):
    """A 24-bit fp32 code by column in [-4, 4)."""
    c = np.arange(D, dtype=np.uint64)
    return (((c + 1) * 2654435761 % (1 << 24)).astype(np.float64) / 2.0 ** 21 - 4.0).astype(F)


def gamma_code(D):
    """6-bit significands, 16 exponents and a sign: distinct over 1024 columns."""
    c = np.arange(D)
    return (np.where((c >> 9) & 1, -1.0, 1.0) * (1 + (c & 31) / 32.0) * np.exp2(((c >> 5) & 15) - 8.0)).astype(F)


def beta_of_gamma(D):
    c = np.arange(D)
    return (gamma_code(D).astype(np.float64) * 2.0 * ((c + (c >> 5)) % 3 - 1)).astype(F)


def gamma_weight(D):
    c = np.arange(D)
    return (np.where((c ^ (c >> 6)) & 1, -1.0, 1.0) * np.exp2(c % 3)).astype(F)


def beta_weight(D):
    return ((np.arange(D) * 5) % 9 - 4.0).astype(F)


def ln_params(family, D):
    return (gamma_pow2(D), beta_code(D)) if family == "dense" else (gamma_code(D), beta_of_gamma(D))


def weight_params(family, D):
    return (gamma_pow2(D), beta_code(D)) if family == "dense" else (gamma_weight(D), beta_weight(D))


def template(D, seed=0):
    """A dyadic unit vector: 4^k entries of +-2^-k, the rest 0."""
    k = 1
    while 4 ** (k + 1) <= D and k < 4:
        k += 1
    rng = np.random.default_rng([3, seed, D])
    t = np.zeros(D)
    t[rng.permutation(D)[:4 ** k]] = rng.choice([-1.0, 1.0], 4 ** k) * 2.0 ** -k
    assert (t * t).sum() == 1.0
    return t.astype(F)


def int_rows(rows, D, seed=0):
    """Integer feature rows in [-8, 8] (bf16 values), none all zero."""
    rng = np.random.default_rng([4, seed, rows, D])
    x = rng.integers(-8, 9, (rows, D)).astype(F)
    x[:, 0] = np.where(x[:, 0] == 0, 3, x[:, 0])
    return x


def cls_pos(D):
    c = np.arange(D)
    return ((c * 7) % 17 - 8.0).astype(F), ((c * 3 + (c >> 4)) % 13 - 6.0).astype(F)


# ---- references (numpy fp32: +, -, *, / and sqrt are correctly rounded, as the compiled kernels' are) ----------------

def rstd_of(q, D, eps):
    var = np.asarray(q, F) / F(D)
    with np.errstate(divide="ignore"):
        return F(1.0) / np.sqrt(var + F(eps))


def ln_out(x, mean, rstd, g, b):
    """f32(f32((x - mean) rstd) gamma + beta); t gamma must be exact, so contraction does not matter."""
    t = (x - mean[:, None]) * rstd[:, None]
    tg = t * g[None, :]
    assert np.array_equal(tg.astype(np.float64), t.astype(np.float64) * g.astype(np.float64)[None, :])
    return tg + b[None, :]


def want_ln(r: Rows, g, b, eps):
    mean = r.m.astype(F)
    return ln_out(r.x, mean, rstd_of(r.q, r.x.shape[1], eps), g, b)


def want_stats(r: Rows, eps):
    return np.stack([r.m.astype(F), rstd_of(r.q, r.x.shape[1], eps)], 1)


def want_sim(feat, tmpl):
    f = feat.astype(np.float64)
    dot, nn = (f * tmpl.astype(np.float64)[None, :]).sum(1), (f * f).sum(1)
    assert np.array_equal(dot.astype(F), dot) and np.array_equal(nn.astype(F), nn) and (nn > 0).all()
    return dot.astype(F) / np.sqrt(nn.astype(F))


def want_Q(sim):
    from oracle import pf
    return pf.weights_to_Q(sim, LAM, BITS)


def cls_of(tokens, row=0, particle_stride=None):
    """The rows a weight kernel reads from tokens [n][N][D]: row 0 of every particle."""
    n, N, D = tokens.shape
    ps = N * D if particle_stride is None else particle_stride
    flat = tokens.reshape(-1)
    return np.stack([flat[p * ps + row * D:p * ps + row * D + D] for p in range(n)])


def tokens_of(cls, N):
    """[n][N][D] with the given CLS rows and NaN everywhere else."""
    t = np.full((cls.shape[0], N, cls.shape[1]), np.nan, F)
    t[:, 0] = cls
    return t


# ---- the kernels' schedules, with mutants ----------------------------------------------------------------------------

def _butterfly(s, steps):
    lanes = np.arange(s.shape[1])
    for o in steps:
        s = s + s[:, lanes ^ o]
    return s


def emulate_stats(x, kernel, mut=None, stale=0.0):
    """{mean, q} of every row by the schedule of ln_row ("ln": 64 lanes, 4-element chunks, pair sums) or of k_row_stats
    ("bf16" / "f32": 32 lanes per row, 8- / 4-element chunks summed in order, rows paired per wave), fp32 throughout.
    Mutants: drop_last_chunk, drop_last_stride (the lanes of the last, partial or full, stride), unguarded (the
    variance pass runs over the idle registers too, which hold `stale`), pair_mean (the mean of the neighbouring row
    for ln; the sum over both half-waves for k_row_stats)."""
    R, D = x.shape
    lanes, epc = (64, 4) if kernel == "ln" else (32, EPC[kernel])
    nch = D // epc
    n_i = 1024 // epc // lanes if mut == "unguarded" else -(-nch // lanes)
    xp = np.full((R, n_i * lanes * epc), stale, F)
    xp[:, :D] = x
    v = xp.reshape(R, n_i, lanes, epc)
    c = np.arange(n_i * lanes).reshape(n_i, lanes)
    live = c < nch
    if mut == "drop_last_chunk":
        live &= c != nch - 1
    if mut == "drop_last_stride":
        live &= c < lanes * ((nch - 1) // lanes)
    steps = [o for o in (32, 16, 8, 4, 2, 1) if o < lanes]
    s = np.zeros((R, lanes), F)
    for i in range(n_i):
        if kernel == "ln":
            part = (v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3])
            s = np.where(live[i], s + part, s)
        else:
            t = s
            for e in range(epc):
                t = t + v[:, i, :, e]
            s = np.where(live[i], t, s)
    tot = _butterfly(s, steps)
    assert (tot == tot[:, :1]).all()
    tot = tot[:, 0]
    partner = np.arange(R) ^ 1
    has = partner < R
    if mut == "pair_mean" and kernel != "ln":
        tot = tot + np.where(has, tot[np.minimum(partner, R - 1)], F(0))
    mean = tot / F(D)
    if mut == "pair_mean" and kernel == "ln":
        mean = np.where(has, mean[np.minimum(partner, R - 1)], mean)
    q = np.zeros((R, lanes), F)
    for i in range(n_i):
        t = q
        for e in range(epc):
            d = (v[:, i, :, e] - mean[:, None]).astype(np.float64)
            t = (d * d + t).astype(F)                                       # fmaf(d, d, q)
        q = np.where(live[i] | (mut == "unguarded"), t, q)
    q = _butterfly(q, steps)
    return mean, q[:, 0]


def in_order(x, order):
    """{mean, q} with one fp32 accumulator that takes the columns in `order` ([D] or [rows][D])."""
    R, D = x.shape
    xo = np.take_along_axis(x, np.broadcast_to(order, (R, D)), 1)
    s = np.zeros(R, F)
    for c in range(D):
        s = s + xo[:, c]
    mean = s / F(D)
    q = np.zeros(R, F)
    for c in range(D):
        d = (xo[:, c] - mean).astype(np.float64)
        q = (d * d + q).astype(F)
    return mean, q


def written_rows(rows, mut=None):
    """The rows k_row_stats writes; the mutant skip_second_stride stops after one grid stride."""
    return np.arange(min(rows, STATS_GRID_ROWS) if mut == "skip_second_stride" else rows)


def combine_no_clamp(planes, K, eps):
    sm, sq = planes[:, :, 0].sum(0, dtype=F), planes[:, :, 1].sum(0, dtype=F)
    inv_k = F(1.0) / F(K)
    mean = sm * inv_k
    var = (sq.astype(np.float64) * np.float64(inv_k) - (mean * mean).astype(np.float64)).astype(F)
    with np.errstate(invalid="ignore"):
        return mean, var, (1.0 / np.sqrt((var + F(eps)).astype(np.float64))).astype(F)


def rstd_candidates(planes, K, eps):
    """mean and the three rstd the combine may return (rsq at -1, 0, +1 ulp)."""
    out = [emulate_combine(planes, K, eps, u) for u in (-1, 0, 1)]
    return out[0][0], np.stack([o[1] for o in out])


def planes_of(r: Rows, P, plane_rows=None):
    """{sum, sumsq} of r's rows over P column blocks (sizes as even as D allows) as fp32 [P][plane_rows][2]; the spare
    rows are NaN."""
    R, D = r.x.shape
    pl = np.full((P, R if plane_rows is None else plane_rows, 2), np.nan, F)
    x = r.x.astype(np.float64)
    edges = np.linspace(0, D, P + 1).astype(int)
    for p in range(P):
        blk = x[:, edges[p]:edges[p + 1]]
        pl[p, :R, 0], pl[p, :R, 1] = blk.sum(1), (blk * blk).sum(1)
    assert np.array_equal(pl[:, :R].astype(np.float64).sum(0)[:, 0], x.sum(1))
    return pl


def constant_planes(rows, P, plane_rows):
    """Rows of one repeated bf16 value at D = 960 over P column blocks; the values are chosen below so that the fp32
    one-pass variance is negative without the clamp."""
    pl = np.full((P, plane_rows, 2), np.nan, F)
    c = CLAMP_VALUES[np.arange(rows) % len(CLAMP_VALUES)].astype(np.float64)
    n = np.diff(np.linspace(0, CLAMP_D, P + 1).astype(int)).astype(np.float64)
    pl[:, :rows, 0] = n[:, None] * c[None, :]
    pl[:, :rows, 1] = n[:, None] * (c * c)[None, :]
    return pl


def _clamp_values():
    cand = bf16_val(bf16_bits(np.linspace(0.3, 9.7, 400).astype(F))).astype(F)
    keep = []
    for P in COMBINE_PARTS:
        pl = np.stack([np.full((P, len(cand)), CLAMP_D / P) * cand, np.full((P, len(cand)), CLAMP_D / P) * cand * cand],
                      2).astype(F)
        keep.append(combine_no_clamp(pl, CLAMP_D, EPS)[1] < -F(EPS))
    return np.unique(cand[np.all(keep, 0)])[:16]


def order_planes(rows, P, plane_rows):
    """Planes whose fp32 sums depend on the order: {2^24, 1, -2^24, 1, ...} rotated by row for the sums, the same one
    step on and scaled by 2^12 for the sums of squares."""
    base = np.array([2.0 ** 24, 1.0, -2.0 ** 24, 1.0])
    pl = np.full((P, plane_rows, 2), np.nan, F)
    p, r = np.arange(P)[:, None], np.arange(rows)[None, :]
    pl[:, :rows, 0] = base[(p + r) % 4]
    pl[:, :rows, 1] = base[(p + r + 1) % 4] * 4096.0
    return pl


ORDER_D = 64
CLAMP_VALUES = _clamp_values()


def cls_stats(D):
    cls, pos = cls_pos(D)
    v = (cls + pos).astype(np.float64)
    return F(v.sum()), F((v * v).sum())


# ---- fairness proofs -------------------------------------------------------------------------------------------------

def _cases():
    """(kernel, family, D, row counts, seed) of every row set the GPU tests build."""
    for fam in FAMILIES:
        for D in LN_D:
            yield "ln", fam, D, LN_ROWS, 0
        for k in EPC:
            for D in STATS_D[k]:
                yield k, fam, D, STATS_ROWS, 0
        for D in W_D:
            yield "ln", fam, D, W_N, 1


CASES = [pytest.param(*c, id=f"{c[0]}-{c[1]}-{c[2]}-seed{c[4]}") for c in _cases()]


@pytest.mark.parametrize("kernel,family,D,row_counts,seed", CASES)
def test_statistics_are_one_value_in_any_order(kernel, family, D, row_counts, seed):
    """The kernel's schedule, plain sequential order and a random permutation per row give one bit pattern for the
    mean and q, equal to the m and the sum of d^2 the row was built from; hence one for rstd and every output."""
    rng = np.random.default_rng(D)
    for rows in row_counts:
        r = FAMILIES[family][0](rows, D, seed)
        want = (r.m.astype(F), r.q.astype(F))
        assert np.array_equal(want[1].astype(np.float64), r.q)
        for got in (emulate_stats(r.x, kernel), in_order(r.x, np.arange(D)),
                    in_order(r.x, rng.permuted(np.tile(np.arange(D), (rows, 1)), axis=1))):
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
            assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        if family == "coded":
            assert np.array_equal(rstd_of(r.q, D, 0.0), np.exp2(-(np.arange(rows) % 5 - 2.0)).astype(F))
            y = want_ln(r, *ln_params("coded", D), 0.0).astype(np.float64)
            g = gamma_code(D).astype(np.float64)
            assert np.isin(y / g[None, :], [-3, -1, 1, 3]).all()
            exact_bf16(y)


@pytest.mark.parametrize("kernel", ["bf16", "f32"])
def test_large_row_count_statistics(kernel):
    """The 65545-row case: exact in the kernel's schedule too; skipping the second grid stride leaves rows unwritten;
    summing over both half-waves changes every row but the odd last one."""
    D = STATS_BIG_D[kernel]
    r = dense_rows(STATS_BIG_ROWS, D)
    mean, q = emulate_stats(r.x, kernel)
    assert np.array_equal(mean, r.m.astype(F)) and np.array_equal(q.astype(np.float64), r.q)
    assert len(written_rows(STATS_BIG_ROWS, "skip_second_stride")) == STATS_BIG_ROWS - 9
    assert STATS_BIG_ROWS % 2 == 1 and STATS_BIG_ROWS > STATS_GRID_ROWS
    bad = emulate_stats(r.x, kernel, "pair_mean")[0] != mean
    assert bad[:-1].all() and not bad[-1]


def _bits_differ(a, b):
    return a[0].view(np.uint32) != b[0].view(np.uint32), a[1].view(np.uint32) != b[1].view(np.uint32)


@pytest.mark.parametrize("kernel,family,D,row_counts,seed", CASES)
def test_schedule_mutants_change_bits(kernel, family, D, row_counts, seed):
    """A dropped last chunk or last stride changes q of every row (and the mean, unless the lost elements sum to 0
    around it); a variance pass over the idle registers (zeroed or stale) changes q of every row wherever a lane has
    an idle register; the neighbouring row's mean (the other half-wave's sum) changes the mean of every row that has a
    neighbour, so every row count above 1 sees it."""
    eps = FAMILIES[family][1]
    for rows in row_counts:
        r = FAMILIES[family][0](rows, D, seed)
        want = emulate_stats(r.x, kernel)
        for mut in ("drop_last_chunk", "drop_last_stride"):
            got = emulate_stats(r.x, kernel, mut)
            dm, dq = _bits_differ(got, want)
            assert (dm | dq).all() and dq.all(), mut
            assert (rstd_of(got[1], D, eps) != rstd_of(r.q, D, eps)).all(), mut     # and the outputs follow
        if D < 1024:
            for stale in (0.0, 0.125):             # never a row's mean (non-zero multiples of 1/4)
                dm, dq = _bits_differ(emulate_stats(r.x, kernel, "unguarded", stale), want)
                assert not dm.any() and dq.all(), stale
        dm, _ = _bits_differ(emulate_stats(r.x, kernel, "pair_mean"), want)
        assert dm[:rows - rows % 2].all() and (rows % 2 == 0 or not dm[-1])


@pytest.mark.parametrize("D", LN_D)
def test_layernorm_outputs_name_their_column(D):
    """Coded rows: the (+, -) outputs of a column are shared with no other column within four lane strides, in fp32
    and after the bf16 rounding, so gamma or beta read from another chunk changes bits. Dense rows: a one-ulp change of
    rstd changes fp32 output bits in every row."""
    g, b = ln_params("coded", D)
    pair = np.stack([bf16_bits(g + b), bf16_bits(-g + b)], 1).astype(np.int64)
    key = pair[:, 0] * 65536 + pair[:, 1]
    for off in (1, 2, 3, 4, 64, 128, 192, 256):
        if off < D:
            assert (key[off:] != key[:-off]).all(), off
    r = dense_rows(9, D)
    g, b = ln_params("dense", D)
    rstd = rstd_of(r.q, D, EPS)
    y0 = ln_out(r.x, r.m.astype(F), rstd, g, b)
    y1 = ln_out(r.x, r.m.astype(F), np.nextafter(rstd, F(np.inf)), g, b)
    assert (y0 != y1).any(axis=1).all()


def test_rstd_is_readable_from_a_layernorm_row():
    """With gamma = 1 and beta = 0 the fp32 LayerNorm output at a column whose d is +-1 is +-rstd itself: the row
    statistics tests read the LayerNorm kernel's rstd there. Every dense row has such a column."""
    for D in sorted(set(STATS_D["bf16"] + STATS_D["f32"])):
        r = dense_rows(9, D)
        col = np.argmax(r.d == 1.0, axis=1)
        assert (r.d[np.arange(9), col] == 1.0).all()
        y = want_ln(r, np.ones(D, F), np.zeros(D, F), EPS)
        assert np.array_equal(y[np.arange(9), col], want_stats(r, EPS)[:, 1])


@pytest.mark.parametrize("P", COMBINE_PARTS)
def test_combine_planes_are_exact_and_clamped(P):
    """Dense rows as planes: the sums are exact in any plane order, so the mean is one value and rstd one of three.
    A plane read one row off, or with the wrong plane stride (the NaN spare rows), changes the result. Constant rows
    at D = 960: without the clamp the variance is below -eps and rstd is NaN; with it rstd is rsq(eps)."""
    rows, D = 257, 768
    r = dense_rows(rows, D)
    pl = planes_of(r, P, rows + 5)
    mean, cand = rstd_candidates(pl[:, :rows], D, EPS)
    assert np.array_equal(mean, (r.x.astype(np.float64).sum(1).astype(F) * (F(1) / F(D))))
    assert np.array_equal(emulate_combine(pl[::-1, :rows], D, EPS)[0], mean)
    exact = 1.0 / np.sqrt(r.q / D + EPS)
    assert np.abs(cand[1] / exact - 1).max() < 2.0 ** -12
    shifted = pl[:, :rows].copy()
    shifted[P - 1] = np.roll(shifted[P - 1], 1, axis=0)
    m2, c2 = rstd_candidates(shifted, D, EPS)
    assert ((m2 != mean) | ((c2[1] < cand[0]) | (c2[1] > cand[2]))).all()
    packed = pl.reshape(-1, 2)[:P * rows].reshape(P, rows, 2)       # plane stride = rows instead of rows + 5
    if P > 1:
        with np.errstate(invalid="ignore"):
            assert np.isnan(emulate_combine(packed, D, EPS)[0]).any()
    assert len(CLAMP_VALUES) >= 4
    cp = constant_planes(rows, P, rows + 5)[:, :rows]
    _, var, bad = combine_no_clamp(cp, CLAMP_D, EPS)
    assert (var < -F(EPS)).all() and np.isnan(bad).all()
    _, cc = rstd_candidates(cp, CLAMP_D, EPS)
    want = (1.0 / np.sqrt(np.float64(F(EPS)))).astype(F)
    assert np.isfinite(cc).all() and (cc[1] == want).all()


@pytest.mark.parametrize("P", [3, 5, 12, 16])
def test_plane_order_decides_the_sum(P):
    """The order planes: the sequential plane-order sum differs from the reversed one and from the one with two planes
    swapped, in mean or beyond the rstd candidates, on at least half of the rows each (the rows rotate the pattern)."""
    rows = 9
    pl = order_planes(rows, P, rows)
    mean, cand = rstd_candidates(pl, ORDER_D, EPS)
    assert np.isfinite(cand).all()
    swapped = pl.copy()
    swapped[[0, P - 1]] = swapped[[P - 1, 0]]
    swapped[[1, 2]] = swapped[[2, 1]]
    seen = np.zeros(rows, bool)
    for other in (pl[::-1], swapped):
        m2, c2 = rstd_candidates(other, ORDER_D, EPS)
        here = (m2 != mean) | (c2[1] < cand[0]) | (c2[1] > cand[2])
        assert here.sum() >= rows // 2
        seen |= here
    assert seen.sum() >= rows - 2


@pytest.mark.parametrize("D", CLS_D)
def test_cls_rows_are_exact(D):
    """cls + pos is an integer bf16 value per column; the sum and the sum of squares are integers below 2^24, exact in
    k_cls_stats' order (256 threads striding the columns, a wave sum, four partials) and any other."""
    cls, pos = cls_pos(D)
    v = cls + pos
    exact_bf16(v)
    assert len(np.unique(v)) > 1
    s = np.zeros(256, F)
    q = np.zeros(256, F)
    for d0 in range(0, D, 256):
        n = min(256, D - d0)
        s[:n] += v[d0:d0 + n]
        q[:n] = (v[d0:d0 + n].astype(np.float64) ** 2 + q[:n]).astype(F)
    ws = [_butterfly(a.reshape(4, 64), (32, 16, 8, 4, 2, 1))[:, 0] for a in (s, q)]
    got = [((w[0] + w[1]) + w[2]) + w[3] for w in ws]
    assert (F(got[0]), F(got[1])) == cls_stats(D)
    assert float(cls_stats(D)[1]) == float((v.astype(np.float64) ** 2).sum()) < 2 ** 24


@pytest.mark.parametrize("D", W_D)
def test_weight_operands_are_exact(D):
    """Coded CLS rows give integer features; dot and nn against the dyadic template are exact; similarities differ
    between particles; reading token row 1 (NaN) or a particle stride of D instead of N D changes feat."""
    n = 5
    r = coded_rows(n, D, seed=1)
    g, b = weight_params("coded", D)
    feat = want_ln(r, g, b, 0.0)
    assert np.array_equal(feat, np.round(feat)) and np.abs(feat).max() <= 8
    t = template(D)
    sim = want_sim(feat, t)
    assert np.isfinite(sim).all() and (np.abs(sim) <= 1).all()
    if D > 4:
        assert len(np.unique(sim)) > 1
    tok = tokens_of(r.x, W_TOKENS)
    assert np.array_equal(cls_of(tok), r.x)
    assert np.isnan(cls_of(tok, row=1)).all()
    wrong = cls_of(tok, particle_stride=D)[1:]
    assert (wrong != r.x[1:]).any(axis=1).all()                  # NaN rows, or another particle's
    Q = want_Q(sim)
    assert Q.min() >= 0 and Q.max() <= 2 ** BITS and (D == 4 or len(np.unique(Q)) > 1)
