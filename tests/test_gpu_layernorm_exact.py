"""GPU (MI355X): the LayerNorm family on exactly computable operands, through the C ABI: vpf_layernorm_*,
vpf_row_stats_*, vpf_stats_combine, vpf_cls_rows_* and vpf_cls_weight_* / vpf_cosine_weight_f32.

The operands and references come from tests/test_oracle_layernorm.py, which proves on the CPU that the bars used here
are exact arithmetic (one bit pattern for the mean, the sum of squared deviations and every output in any summation
order) and that the kernels' plausible faults change bits. Only vpf_stats_combine has an approximate instruction; its
rstd is held to the three candidates of the project's existing rsq bar.

Shapes and what they reach:
  LayerNorm / weights, D: 4 (one lane), 252 and 260 (one chunk short of and past a 64-lane stride: nch = 63, 65),
    256 (one full stride, three idle registers per lane), 768, 1020 (nch = 255) and 1024 (no idle register).
    rows / particles 1, 3, 4, 5, 9 (257 for the weights): the edges of 4 rows per workgroup.
  Row statistics, D: one 16-byte chunk, one chunk short of, at and past a 32-lane stride (bf16: 248 / 256 / 264,
    fp32: 124 / 128 / 132), 768, one chunk short of 1024, 1024. rows 1, 2, 7, 8, 9 (the half-wave pairing with and
    without an odd last row, one workgroup and two) and 65545 (the grid-stride loop's second stride, odd last row).
  Combine: parts 3 / 12 / 16 (the unrolled forms) and 1, 5, 15, 64 (the generic loop); rows 1, 256, 257 (one thread,
    one full workgroup, one thread of a second); plane_stride = rows + 5 with NaN spare rows.
  CLS rows: D 4 .. 1024 (k_cls_stats: less than one pass of 256 threads, a partial second pass at 320, four full
    passes), n_part 1, 5, 257 (the particle loop's second pass), N 1 and 3, parts 1, 3, 16.

Every output is a view inside a sentinel-filled buffer (a row stride wider than D where the entry point takes one,
spare rows before and after): the sentinel must survive outside the view and be gone inside it."""
import numpy as np
import pytest
import torch

import test_oracle_layernorm as exact    # operands and references, proven fair on the CPU there

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
NP = {"bf16": np.uint16, "f32": np.float32}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib
    assert b"gfx950" in _lib.lib().vpf_version()


def E():
    from vitparticlefiltertracker_amd import _lib
    return _lib


def run(name, *args):
    rc = getattr(E().lib(), name)(*args, E().stream_ptr())
    assert rc == 0, f"{name} returned {rc}"
    torch.cuda.synchronize()


def ubits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(ubits(a)).view(np.uint8)).to(DEV)


class Guard:
    """A [rows][cols] view (row stride ld elements) inside a buffer of sentinel bytes, `pad` spare rows before and
    after it."""

    def __init__(self, rows, cols, ld, np_dtype, sent=0xAB, pad=2):
        self.rows, self.cols, self.ld, self.pad = rows, cols, ld, pad
        self.item = np.dtype(np_dtype).itemsize
        self.buf = torch.full(((rows + 2 * pad) * ld * self.item,), sent, dtype=torch.uint8, device=DEV)
        self.sent = np.frombuffer(bytes([sent] * self.item), dtype=UINT[self.item])[0]

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.pad * self.ld * self.item

    def fill(self, values):
        v = np.ascontiguousarray(values)
        assert v.shape == (self.rows, self.cols) and v.dtype.itemsize == self.item
        t = torch.from_numpy(v.view(np.uint8).reshape(self.rows, self.cols * self.item)).to(DEV)
        self.buf.view(self.rows + 2 * self.pad, self.ld * self.item)[self.pad:self.pad + self.rows,
                                                                     :self.cols * self.item] = t
        return self

    def read(self, what, rows=None):
        """The bit patterns of the written rows [len(rows)][cols] (default: all), after checking that everything
        outside them still holds the sentinel."""
        full = self.buf.cpu().numpy().view(UINT[self.item]).reshape(self.rows + 2 * self.pad, self.ld)
        rows = np.arange(self.rows) if rows is None else np.asarray(rows)
        outside = np.ones(full.shape, dtype=bool)
        outside[(rows + self.pad)[:, None], np.arange(self.cols)[None, :]] = False
        bad = outside & (full != self.sent)
        assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the output were written; first at " \
            f"(row {np.argwhere(bad)[0][0] - self.pad}, col {np.argwhere(bad)[0][1]}) of a " \
            f"[{self.rows}][{self.cols}] view"
        return full[rows + self.pad][:, :self.cols].copy()

    def untouched(self, what):
        assert (self.buf == int(self.sent & 0xFF)).all().item(), f"{what}: the output was written"


def assert_bits(got, want, sent, what):
    want = ubits(want).reshape(got.shape)
    assert (want != sent).all(), f"{what}: an expected value equals the sentinel"
    bad = got != want
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outputs differ; first at {i}: got "
                             f"0x{int(got[i]):x}, want 0x{int(want[i]):x}")


def stored(x, dtype):
    """fp32 values that are bf16 values -> what the kernel's input holds."""
    return exact.exact_bf16(x) if dtype == "bf16" else np.asarray(x, F)


# ---- vpf_layernorm_* -------------------------------------------------------------------------------------------------

def layernorm(dtype, x_values, g, b, eps, what):
    rows, D = x_values.shape
    x = Guard(rows, D, D + 8, NP[dtype]).fill(stored(x_values, dtype))
    y = Guard(rows, D, D + 12, NP[dtype])
    run(f"vpf_layernorm_{dtype}", x.ptr, rows, D, x.ld, g.data_ptr(), b.data_ptr(), eps, y.ptr, y.ld)
    return y.read(what), y.sent


@pytest.mark.parametrize("D", exact.LN_D)
@pytest.mark.parametrize("family", ["dense", "coded"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_layernorm_bits(dtype, family, D):
    """Dense rows (eps = 1e-6) and coded rows (eps = 0): every output bit, x_stride != y_stride."""
    gen, eps = exact.FAMILIES[family]
    g, b = exact.ln_params(family, D)
    gd, bd = dev(g), dev(b)
    for rows in exact.LN_ROWS:
        r = gen(rows, D)
        want = exact.want_ln(r, g, b, eps)
        what = f"layernorm_{dtype} {family} rows={rows} D={D}"
        got, sent = layernorm(dtype, r.x, gd, bd, eps, what)
        assert_bits(got, exact.bf16_bits(want) if dtype == "bf16" else want, sent, what)


# ---- vpf_row_stats_* -------------------------------------------------------------------------------------------------

def row_stats(kernel, r, eps, what):
    rows, D = r.x.shape
    x = Guard(rows, D, D + exact.EPC[kernel], NP[kernel]).fill(stored(r.x, kernel))
    out = Guard(rows, 2, 2, F)
    run(f"vpf_row_stats_{kernel}", x.ptr, rows, D, x.ld, eps, out.ptr)
    got = out.read(what)
    assert_bits(got, exact.want_stats(r, eps), out.sent, what)
    return got


@pytest.mark.parametrize("kernel,D", [(k, D) for k in ("bf16", "f32") for D in exact.STATS_D[k]])
def test_row_stats_bits(kernel, D):
    """{mean, rstd} bit-equal on dense and coded rows; on the dense rows rstd is also the one vpf_layernorm_f32 used
    (read at a column whose deviation is 1, with gamma = 1 and beta = 0)."""
    one, zero = dev(np.ones(D, F)), dev(np.zeros(D, F))
    for rows in exact.STATS_ROWS:
        for family, (gen, eps) in exact.FAMILIES.items():
            r = gen(rows, D)
            what = f"row_stats_{kernel} {family} rows={rows} D={D}"
            got = row_stats(kernel, r, eps, what)
            if family == "dense":
                y, _ = layernorm("f32", r.x, one, zero, eps, what)
                col = np.argmax(r.d == 1.0, axis=1)
                assert np.array_equal(y[np.arange(rows), col], got[:, 1]), f"{what}: rstd differs from layernorm_f32's"


@pytest.mark.parametrize("kernel", ["bf16", "f32"])
def test_row_stats_second_grid_stride(kernel):
    """65545 rows: more than the 8 x 8192 rows of one grid stride, ending on an odd row."""
    r = exact.dense_rows(exact.STATS_BIG_ROWS, exact.STATS_BIG_D[kernel])
    row_stats(kernel, r, exact.EPS, f"row_stats_{kernel} rows={exact.STATS_BIG_ROWS}")


# ---- vpf_stats_combine -----------------------------------------------------------------------------------------------

def combine(planes, rows, D, eps, what):
    """planes fp32 [P][plane_stride][2] on the host -> {mean, rstd} bits [rows][2]."""
    P, pstride = planes.shape[:2]
    pl = Guard(P * pstride, 2, 2, F).fill(planes.reshape(-1, 2))
    out = Guard(rows, 2, 2, F)
    run("vpf_stats_combine", pl.ptr, P, pstride, rows, D, eps, out.ptr)
    got = out.read(what)
    mean, cand = exact.rstd_candidates(planes[:, :rows], D, eps)
    assert_bits(got[:, 0], mean, out.sent, what + " mean")
    rstd = got[:, 1].view(F)
    ok = (rstd[None, :] == cand).any(0)
    assert ok.all(), f"{what}: rstd of row {np.argmax(~ok)} is {rstd[np.argmax(~ok)]!r}, candidates " \
        f"{cand[:, np.argmax(~ok)]!r}"
    return rstd


@pytest.mark.parametrize("parts", exact.COMBINE_PARTS)
def test_stats_combine_bits(parts):
    """Dense rows as planes (mean bit-equal, rstd one of the three rsq candidates), constant rows at D = 960 (the clamp:
    rstd finite, a candidate of rsq(eps)) and the order-dependent planes (the sequential plane-order sum)."""
    for rows in exact.COMBINE_ROWS:
        what = f"stats_combine parts={parts} rows={rows}"
        combine(exact.planes_of(exact.dense_rows(rows, 768), parts, rows + 5), rows, 768, exact.EPS, what + " dense")
        rstd = combine(exact.constant_planes(rows, parts, rows + 5), rows, exact.CLAMP_D, exact.EPS, what + " constant")
        assert np.isfinite(rstd).all()
        combine(exact.order_planes(rows, parts, rows + 5), rows, exact.ORDER_D, exact.EPS, what + " order")


# ---- vpf_cls_rows_* --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_part", exact.CLS_NPART)
@pytest.mark.parametrize("D", exact.CLS_D)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_cls_rows_bits(dtype, D, n_part):
    """tokens[p][0][:] = cls + pos[0] bit-equal, every other token row untouched; with stats_out, plane 0 of every CLS
    row holds the exact {sum, sumsq}, planes 1.. hold 0 and every other plane row keeps its NaN."""
    cls, pos = exact.cls_pos(D)
    cd, pd = dev(cls), dev(pos)
    want = np.tile(stored(cls + pos, dtype), (n_part, 1))
    for N in exact.CLS_N:
        cls_rows = np.arange(n_part) * N
        for parts in [0] + (exact.CLS_PARTS if dtype == "bf16" else []):
            what = f"cls_rows_{dtype} D={D} n_part={n_part} N={N} parts={parts}"
            tok = Guard(n_part * N, D, D, NP[dtype])
            st = Guard(max(parts, 1) * n_part * N, 2, 2, F, sent=0xFF)
            if dtype == "bf16":
                run("vpf_cls_rows_bf16", tok.ptr, n_part, N, D, cd.data_ptr(), pd.data_ptr(),
                    st.ptr if parts else None, parts)
            else:
                run("vpf_cls_rows_f32", tok.ptr, n_part, N, D, cd.data_ptr(), pd.data_ptr())
            assert_bits(tok.read(what, cls_rows), want, tok.sent, what)
            if not parts:
                st.untouched(what)
                continue
            rows = (np.arange(parts)[:, None] * (n_part * N) + cls_rows[None, :]).reshape(-1)
            planes = np.zeros((parts, n_part, 2), F)
            planes[0] = exact.cls_stats(D)
            assert_bits(st.read(what + " planes", rows), planes.reshape(-1, 2), st.sent, what + " planes")


# ---- vpf_cls_weight_* / vpf_cosine_weight_f32 ------------------------------------------------------------------------

def tokens(cls_rows, N, dtype):
    """[n][N][D] as the kernel's input holds it: the given CLS rows, NaN in every other row."""
    tok = exact.tokens_of(cls_rows, N)
    if dtype == "f32":
        return tok
    bits = np.full(tok.shape, 0x7FC0, np.uint16)
    bits[:, 0] = exact.exact_bf16(cls_rows)
    return bits


def weigh(name, tokens, n, N, D, g, b, eps, t, feat=True, sim=True):
    """One weight launch -> (feat bits or None, sim bits or None, Q)."""
    f, s, q = Guard(n, D, D, F), Guard(n, 1, 1, F), Guard(n, 1, 1, np.int64)
    ln = () if name == "vpf_cosine_weight_f32" else (None if g is None else g.data_ptr(),
                                                      None if b is None else b.data_ptr(), eps)
    dims = (n, D) if name == "vpf_cosine_weight_f32" else (n, N, D)
    outs = (s.ptr if sim else None, q.ptr) if name == "vpf_cosine_weight_f32" else \
        (f.ptr if feat else None, s.ptr if sim else None, q.ptr)
    run(name, tokens.data_ptr(), *dims, *ln, t.data_ptr(), exact.LAM, exact.BITS, *outs)
    what = f"{name} n={n} D={D}"
    if not feat or name == "vpf_cosine_weight_f32":
        f.untouched(what + " feat")
    if not sim:
        s.untouched(what + " sim")
    return (f.read(what + " feat") if feat and name != "vpf_cosine_weight_f32" else None,
            s.read(what + " sim") if sim else None, q.read(what + " Q").view(np.int64)[:, 0], f.sent)


@pytest.mark.parametrize("D", exact.W_D)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_cls_weight_bits(dtype, D):
    """Coded CLS rows (eps = 0) under NaN token rows 1..: feat bit-equal, sim bit-equal to f32(dot / sqrtf(nn)), Q the
    oracle's function of the predicted sim, and the same Q with feat_out and sim_out NULL. Dense rows (eps = 1e-6):
    feat bit-equal."""
    name, N = f"vpf_cls_weight_{dtype}", exact.W_TOKENS
    t = exact.template(D)
    td = dev(t)
    for n in exact.W_N:
        r = exact.coded_rows(n, D, seed=1)
        g, b = exact.weight_params("coded", D)
        gd, bd = dev(g), dev(b)
        tok = dev(tokens(r.x, N, dtype))
        what = f"{name} coded n={n} D={D}"
        feat = exact.want_ln(r, g, b, 0.0)
        sim = exact.want_sim(feat, t)
        Q = exact.want_Q(sim)
        gf, gs, gq, sent = weigh(name, tok, n, N, D, gd, bd, 0.0, td)
        assert_bits(gf, feat, sent, what + " feat")
        assert_bits(gs[:, 0], sim, sent, what + " sim")
        assert np.array_equal(gq, Q), f"{what}: Q differs at particle {np.argmax(gq != Q)}"
        _, _, gq, _ = weigh(name, tok, n, N, D, gd, bd, 0.0, td, feat=False, sim=False)
        assert np.array_equal(gq, Q), f"{what}: Q differs without feat_out / sim_out"

        r = exact.dense_rows(n, D, seed=1)
        g, b = exact.weight_params("dense", D)
        tok = dev(tokens(r.x, N, dtype))
        gf, _, _, sent = weigh(name, tok, n, N, D, dev(g), dev(b), exact.EPS, td)
        assert_bits(gf, exact.want_ln(r, g, b, exact.EPS), sent, f"{name} dense n={n} D={D} feat")


@pytest.mark.parametrize("D", exact.W_D)
def test_weight_without_layernorm_bits(D):
    """The kernel without the LN: vpf_cosine_weight_f32 on integer feature rows, and vpf_cls_weight_bf16 with
    gamma = NULL on the same rows as the CLS tokens (feat_out is then the row itself)."""
    t = exact.template(D)
    td = dev(t)
    for n in exact.W_N:
        x = exact.int_rows(n, D)
        sim = exact.want_sim(x, t)
        Q = exact.want_Q(sim)
        what = f"cosine_weight_f32 n={n} D={D}"
        _, gs, gq, sent = weigh("vpf_cosine_weight_f32", dev(x), n, 1, D, None, None, 0.0, td)
        assert_bits(gs[:, 0], sim, sent, what + " sim")
        assert np.array_equal(gq, Q), f"{what}: Q differs at particle {np.argmax(gq != Q)}"
        _, _, gq, _ = weigh("vpf_cosine_weight_f32", dev(x), n, 1, D, None, None, 0.0, td, sim=False)
        assert np.array_equal(gq, Q), f"{what}: Q differs without sim_out"
        bits = tokens(x, exact.W_TOKENS, "bf16")
        what = f"cls_weight_bf16 without LN n={n} D={D}"
        gf, gs, gq, sent = weigh("vpf_cls_weight_bf16", dev(bits), n, exact.W_TOKENS, D, None, None, 0.0, td)
        assert_bits(gf, x, sent, what + " feat")
        assert_bits(gs[:, 0], sim, sent, what + " sim")
        assert np.array_equal(gq, Q), f"{what}: Q differs at particle {np.argmax(gq != Q)}"


# ---- argument contract (host-side returns: nothing launches) ---------------------------------------------------------

def test_argument_contract():
    """Every rejection of ln_launch, stats_launch, clsw_launch, vpf_stats_combine and vpf_cls_rows_* returns
    VPF_ERR_ARG and leaves the output alone; zero rows return 0 and leave it alone where the code accepts them."""
    L, s = E().lib(), E().stream_ptr()
    inf, nan = float("inf"), float("nan")
    src = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    x, g, b, t = src.data_ptr(), src.data_ptr(), src.data_ptr(), src.data_ptr()
    out = Guard(64, 64, 64, F)
    o = out.ptr
    rejected = []
    for fn in (L.vpf_layernorm_bf16, L.vpf_layernorm_f32):
        for rows, D, xs, ys in [(-1, 64, 64, 64), (4, 0, 64, 64), (4, -4, 64, 64), (4, 6, 64, 64), (4, 62, 64, 64),
                                (4, 1028, 1028, 1028), (4, 64, 60, 64), (4, 64, 64, 60)]:
            rejected.append((fn.__name__, (rows, D, xs, ys), fn(x, rows, D, xs, g, b, 1e-6, o, ys, s)))
        assert fn(x, 0, 64, 64, g, b, 1e-6, o, 64, s) == 0
    for fn, epc in ((L.vpf_row_stats_bf16, 8), (L.vpf_row_stats_f32, 4)):
        for rows, D, xs, op in [(-1, 64, 64, o), (4, 0, 64, o), (4, 64 + epc // 2, 128, o), (4, 1024 + epc, 2048, o),
                                (4, 64, 64 - epc, o), (4, 64, 64 + epc // 2, o), (4, 64, 64, None)]:
            rejected.append((fn.__name__, (rows, D, xs, op is None), fn(x, rows, D, xs, 1e-6, op, s)))
        assert fn(x, 0, 64, 64, 1e-6, o, s) == 0
    for fn in (L.vpf_cls_weight_bf16, L.vpf_cls_weight_f32):
        for n, N, D, tp, lam, bits, q in [(-1, 3, 64, t, 20.0, 40, o), (4, 0, 64, t, 20.0, 40, o),
                                          (4, 3, 0, t, 20.0, 40, o), (4, 3, 62, t, 20.0, 40, o),
                                          (4, 3, 1028, t, 20.0, 40, o), (4, 3, 64, t, 20.0, -1, o),
                                          (4, 3, 64, t, 20.0, 63, o), (4, 3, 64, t, 20.0, 40, None),
                                          (4, 3, 64, None, 20.0, 40, o), (4, 3, 64, t, -1.0, 40, o),
                                          (4, 3, 64, t, inf, 40, o), (4, 3, 64, t, nan, 40, o)]:
            rejected.append((fn.__name__, (n, N, D, tp is None, lam, bits, q is None),
                             fn(x, n, N, D, g, b, 1e-6, tp, lam, bits, o, o, q, s)))
        assert fn(x, 0, 3, 64, g, b, 1e-6, t, 20.0, 40, o, o, o, s) == 0
    for n, D, tp, lam, bits, q in [(-1, 64, t, 20.0, 40, o), (4, 62, t, 20.0, 40, o), (4, 1028, t, 20.0, 40, o),
                                   (4, 64, t, 20.0, 63, o), (4, 64, t, -1.0, 40, o), (4, 64, None, 20.0, 40, o),
                                   (4, 64, t, 20.0, 40, None)]:
        rejected.append(("vpf_cosine_weight_f32", (n, D, tp is None, lam, bits, q is None),
                         L.vpf_cosine_weight_f32(x, n, D, tp, lam, bits, o, q, s)))
    assert L.vpf_cosine_weight_f32(x, 0, 64, t, 20.0, 40, o, o, s) == 0
    for pl, parts, pstride, rows, D, eps, op in [(None, 3, 8, 8, 64, 1e-6, o), (x, 3, 8, 8, 64, 1e-6, None),
                                                 (x, 0, 8, 8, 64, 1e-6, o), (x, 65, 8, 8, 64, 1e-6, o),
                                                 (x, 3, 8, 0, 64, 1e-6, o), (x, 3, 8, -1, 64, 1e-6, o),
                                                 (x, 3, 7, 8, 64, 1e-6, o), (x, 3, 8, 8, 0, 1e-6, o),
                                                 (x, 3, 8, 8, 64, -1e-6, o), (x, 3, 8, 8, 64, nan, o),
                                                 (x + 4, 3, 8, 8, 64, 1e-6, o), (x, 3, 8, 8, 64, 1e-6, o + 4)]:
        rejected.append(("vpf_stats_combine", (pl, parts, pstride, rows, D, eps, op),
                         L.vpf_stats_combine(pl, parts, pstride, rows, D, eps, op, s)))
    for n, N, D, st, parts in [(-1, 3, 64, None, 0), (4, 0, 64, None, 0), (4, 3, 0, None, 0), (4, 3, 64, o, 0),
                               (4, 3, 64, o, 65), (4, 3, 64, o + 4, 3)]:
        rejected.append(("vpf_cls_rows_bf16", (n, N, D, st, parts),
                         L.vpf_cls_rows_bf16(o, n, N, D, g, b, st, parts, s)))
    for n, N, D in [(-1, 3, 64), (4, 0, 64), (4, 3, 0)]:
        rejected.append(("vpf_cls_rows_f32", (n, N, D), L.vpf_cls_rows_f32(o, n, N, D, g, b, s)))
    assert L.vpf_cls_rows_bf16(o, 0, 3, 64, g, b, o, 3, s) == 0
    assert L.vpf_cls_rows_f32(o, 0, 3, 64, g, b, s) == 0
    torch.cuda.synchronize()
    wrong = [(name, args, rc) for name, args, rc in rejected if rc != ERR_ARG]
    assert not wrong, wrong
    out.untouched("argument contract")
