"""GPU (MI355X): the bf16 GEMM family (vpf_gemm_bf16 on both product kernels, vpf_gemm_bf16_splitk) and vpf_gemm_f32 on
exactly computable operands, through the C ABI.

The operands and references come from tests/test_oracle_gemm.py, which proves on the CPU that the bars used here are
exact arithmetic: bf16 (or fp32) bit equality on the dense integer operands and on the coded epilogue operands, the
project's GELU bar on exact pre-activations for the GELU epilogues, and for the planes form of the LN statistics bit
equality on the coded operands and the interval its deviation bound allows on the dense ones.

Shapes (M, N, K) and what they reach (256 x 256 output tiles, 8 waves of 128 x 64, K-tiles of 64, nk = K / 64):
  (600, 520, 256)  9 tiles: the grid is not a multiple of 8 workgroups (xcd_first's r != 0 branch); 3 row panels, so
                   groups of 2 and 8 are partial (gsz < group); the M edge tile has 88 rows, so its wave row wm = 1 is
                   wholly out of range; the N edge tile is one 8-column piece (and N % 64 != 0); nk = 4.
  (300, 328, 64)   nk = 1 (the epilogue operands go out with the prologue); the N edge tile is 64 + 8 columns, so the
                   last statistics plane covers 8 columns (park_row_partial zeroes the lanes past N).
  (257, 256, 128)  an M edge tile of one row; nk = 2.
  (394, 64, 384)   N < 256 in a single column tile (every W row past 63 clamped); nk = 6; M even: the statistics planes
                   take the 16-byte DMA form (when 16-byte aligned).
  (5, 128, 320)    M < 16; nk = 5; M odd: the 4-byte DMA form.
  (300, 384, 192)  nk = 3; N % 128 == 0, for the MX8-copy instances of the producers; a 128-column N edge tile.
nk = 1 .. 6 covers every (nk % 3, nk & 1): the epilogue-operand slot and wave image regions of the deep ring, and its B
slot. The partial N tiles put the direct-store GELU epilogues (W rows staged through wperm, clamped to N - 1 - n0) and
the LN fold on both kernels.

Every output is a view of a larger buffer of sentinel bytes (row stride N + 24, spare rows); the statistics planes have
a guard in front and a spare plane and rows behind; the split-K workspace has spare elements. All of that must keep
the sentinel, and inside the view the sentinel must be gone with every bit as expected: every tile is written exactly
once, whatever the tile order."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import test_gpu_mx8 as mx8t         # the MX8 canary and quantiser helpers
import test_oracle_gemm as exact    # operands and references, proven fair on the CPU there

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0xAB
BIAS, BIAS_GELU, RES, PATCH, LN, LN_GELU = range(6)
NAMES = ["BIAS", "BIAS_GELU", "BIAS_RESIDUAL", "PATCH", "LN", "LN_GELU"]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()


def E():
    from vitparticlefiltertracker_amd import _lib
    return _lib


@contextlib.contextmanager
def tuned(kern, group=-1):
    """vpf_gemm_tune(kern, group) for the block; the per-shape defaults (0, -1) are restored whatever happens."""
    L = E().lib()
    try:
        assert L.vpf_gemm_tune(kern, group) == 0
        yield
        torch.cuda.synchronize()
    finally:
        L.vpf_gemm_tune(0, -1)


# ---- buffers ---------------------------------------------------------------------------------------------------------

def _dev_bits(bits, ld=None):
    """bf16 bits [R][C] -> device bf16 tensor; with ld a [R][C] view of rows ld elements apart."""
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)
    if ld is None:
        return t.to(DEV)
    buf = torch.zeros(bits.shape[0], ld, dtype=torch.bfloat16, device=DEV)
    buf[:, :bits.shape[1]] = t.to(DEV)
    return buf[:, :bits.shape[1]]


def _dev_f32(x, off=0):
    """fp32 array -> contiguous device tensor that starts `off` floats into its allocation (off = 2: 8 bytes in, so
    8-byte but not 16-byte aligned)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = torch.zeros(x.size + off, dtype=torch.float32, device=DEV)
    view = buf[off:]
    view.copy_(torch.from_numpy(x.reshape(-1)))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view


class OutBuf:
    """[rows][N] output view inside a sentinel-filled buffer: row stride N + 24 elements, 3 spare rows."""

    def __init__(self, rows, N, np_dtype=np.uint16):
        self.rows, self.N, self.ld = rows, N, N + 24
        self.np_dtype = np.dtype(np_dtype)
        self.buf = torch.full(((rows + 3) * self.ld * self.np_dtype.itemsize,), SENT, dtype=torch.uint8, device=DEV)
        self.sent = np.frombuffer(bytes([SENT] * self.np_dtype.itemsize), dtype=self.np_dtype)[0]

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def fill(self, values):
        """values [rows][N] (bit patterns of this buffer's width) into the view."""
        t = torch.from_numpy(np.ascontiguousarray(values).view(np.uint8).reshape(self.rows, -1)).to(DEV)
        self.buf.view(self.rows + 3, -1)[:self.rows, :t.shape[1]] = t

    def device_rows(self):
        """The view as a contiguous device bf16 tensor [rows][N]."""
        return self.buf.view(torch.bfloat16).view(self.rows + 3, self.ld)[:self.rows, :self.N].contiguous()

    def read(self, what, rows=None):
        """The bit patterns of the written rows [len(rows)][N] (default: all), after checking that everything outside
        them still holds the sentinel."""
        full = self.buf.cpu().numpy().view(self.np_dtype).reshape(self.rows + 3, self.ld)
        rows = np.arange(self.rows) if rows is None else rows
        outside = np.ones(full.shape, dtype=bool)
        outside[rows[:, None], np.arange(self.N)[None, :]] = False
        bad = outside & (full != self.sent)
        assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the output were written; first at " \
            f"(row {np.argwhere(bad)[0][0]}, col {np.argwhere(bad)[0][1]}) of a [{self.rows}][{self.N}] view"
        return full[rows][:, :self.N].copy()


class PlanesBuf:
    """Producer statistics planes [P][R][2] fp32 inside a sentinel-filled buffer: a 4-float guard in front, one spare
    plane and 3 spare rows behind."""

    def __init__(self, P, R):
        self.P, self.R = P, R
        self.n = 4 + (P + 1) * R * 2 + 6
        self.buf = torch.full((self.n * 4,), SENT, dtype=torch.uint8, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 16

    def read(self, what, rows=None):
        """float32 [P][len(rows)][2]; the guard, the spare space and the rows not in `rows` (the CLS rows of a patch
        output) must hold the sentinel."""
        raw = self.buf.cpu().numpy().view(np.uint32)
        sent = np.uint32(0xABABABAB)
        body = raw[4:4 + self.P * self.R * 2].reshape(self.P, self.R, 2)
        assert (raw[:4] == sent).all(), f"{what}: the words in front of the statistics planes were written"
        assert (raw[4 + self.P * self.R * 2:] == sent).all(), \
            f"{what}: statistics were written beyond plane {self.P - 1}"
        rows = np.arange(self.R) if rows is None else rows
        skip = np.ones(self.R, dtype=bool)
        skip[rows] = False
        assert (body[:, skip] == sent).all(), f"{what}: statistics rows of CLS tokens were written"
        got = body[:, rows]
        assert (got != sent).all(), f"{what}: {int((got == sent).sum())} statistics entries were not written"
        return got.view(np.float32)


# ---- operands on the device ------------------------------------------------------------------------------------------

class Dev:
    def __init__(self, o, strided=False):
        self.o = o
        self.lda = o.K + 8 if strided else o.K
        self.a = _dev_bits(o.a, self.lda if strided else None)
        self.w = _dev_bits(o.w)
        self.bias, self.colsum = _dev_f32(o.bias), _dev_f32(o.colsum)
        self.pos = None if o.pos is None else _dev_f32(o.pos)


BUILDERS = {"dense": exact.dense, "coded": exact.coded, "coded_planes": exact.coded_planes,
            "gcoded_planes": exact.gcoded_planes}


@functools.lru_cache(maxsize=None)
def operands(kind, M, N, K, g2="default"):
    """(CPU operands, device operands) of one case, built once."""
    if kind.startswith("gelu:"):
        o = exact.coded_gelu(M, N, K, kind[5:])
    elif g2 == "default":
        o = BUILDERS[kind](M, N, K)
    else:
        o = BUILDERS[kind](M, N, K, g2)
    return o, Dev(o)


@functools.lru_cache(maxsize=None)
def want_bits(kind, M, N, K, epi, g2="default"):
    return exact.want_bits(operands(kind, M, N, K, g2)[0], epi)


@functools.lru_cache(maxsize=None)
def pre_act(kind, M, N, K, epi):
    return exact.pre_activation(operands(kind, M, N, K)[0], epi).astype(np.float64)


# ---- comparisons -----------------------------------------------------------------------------------------------------

def assert_bits(got, want, what):
    assert (want != 0xABAB).all()
    bad = got != want
    exact.require(bad, lambda: f"{what}\n" + exact.diff_report(bad, got, want))


def assert_gelu(got, pre, what, slack=0.0):
    """The GELU bar on the exact pre-activation; the sentinel must be gone (it is a tiny negative number, inside the
    bar wherever the reference is near 0)."""
    ref, bar = exact.gelu_bar(pre, slack)
    val = exact.bf16_val(got)
    bad = ~(np.abs(val - ref) <= bar) | (got == 0xABAB)
    exact.require(bad, lambda: f"{what} (GELU bar)\n" + exact.diff_report(bad, val, ref))


def assert_interval(got, y, slack, what):
    lo, hi = exact.interval_bits(y, slack)
    val = exact.bf16_val(got)
    bad = ~((val >= lo) & (val <= hi)) | (got == 0xABAB)
    exact.require(bad, lambda: f"{what} (interval of the planes combine)\n" + exact.diff_report(bad, val, lo))


def assert_planes(pl, stored_bits, what, is_exact=True):
    """Producer planes against {sum, sumsq} of the stored bf16 values: bit-equal where those are integers (dense)."""
    want = exact.stats_planes(stored_bits)
    if is_exact:
        bad = (pl.astype(np.float64) != want).any(axis=2)
        first = tuple(np.argwhere(bad)[0]) if bad.any() else None
        assert first is None, f"{what}: {int(bad.sum())} statistics entries differ; first (plane, row) {first}: " \
            f"got {pl[first]}, want {want[first]}"
    else:
        np.testing.assert_allclose(pl, want, rtol=1e-5, atol=1e-3, err_msg=what)


# ---- launches --------------------------------------------------------------------------------------------------------

def launch(o, d, epi, what, *, stats=None, P=0, off=0, inplace=False, stats_out=False, copy8=False):
    """One vpf_gemm_bf16 call with canaries everywhere. Returns (output bits [M][N] in A's row order, producer planes
    [ceil(N/64)][M][2] or None). `stats`: the LN row statistics (default {mean, rstd}), P their plane count, `off`
    floats into their allocation."""
    M, N, K = o.M, o.N, o.K
    g2 = o.g2 if epi == PATCH else 0
    R = (M // g2) * (g2 + 1) if epi == PATCH else M
    rows = exact.patch_rows(M, g2) if epi == PATCH else None
    out = OutBuf(R, N)
    res = resbuf = None
    if epi == RES:
        if inplace:
            out.fill(o.residual)
            res = out.ptr
        else:
            resbuf = OutBuf(M, N)
            resbuf.fill(o.residual)
            res = resbuf.ptr
    st = None
    if epi in (LN, LN_GELU):
        st = _dev_f32(o.row_stats() if stats is None else stats, off)
    pl = PlanesBuf((N + 63) // 64, R) if stats_out else None
    q = s = None
    if copy8:
        qbuf = mx8t._canary_u8(R + 3, N + 128)
        q = qbuf[:R, :N]
        s = mx8t._canary_scales(N // 128, R)
    E().call("vpf_gemm_bf16", d.a.data_ptr(), d.lda, d.w.data_ptr(), d.bias.data_ptr(), res,
             None if d.pos is None or epi != PATCH else d.pos.data_ptr(), g2, None if st is None else st.data_ptr(),
             d.colsum.data_ptr() if st is not None else None, out.ptr, out.ld, M, N, K, epi, P, 0.0,
             None if pl is None else pl.ptr, None if q is None else q.data_ptr(), 0 if q is None else q.stride(0),
             None if s is None else s.data_ptr(), 0 if s is None else s.shape[1], E().stream_ptr())
    torch.cuda.synchronize()
    got = out.read(what, rows)
    if resbuf is not None:
        assert np.array_equal(resbuf.read(what + " (residual)"), o.residual), f"{what}: the residual was written"
    if copy8:
        sel = torch.from_numpy(np.arange(R) if rows is None else rows).to(DEV)
        rq, rs = mx8t.quant(out.device_rows())
        assert torch.equal(q[sel], rq[sel]), f"{what}: {int((q[sel] != rq[sel]).sum())} MX8 element codes differ"
        assert torch.equal(mx8t.ops().mx8_scale_bytes(s, R)[sel], mx8t.ops().mx8_scale_bytes(rs, R)[sel]), \
            f"{what}: MX8 scale bytes differ"
        mx8t._assert_canary(qbuf, R, N)
        mx8t._assert_scale_canary(s, R)
        if rows is not None:
            cls = torch.ones(R, dtype=torch.bool)
            cls[rows] = False
            assert bool((q[cls.to(DEV)] == mx8t.CANARY).all()), f"{what}: MX8 rows of CLS tokens were written"
    return got, None if pl is None else pl.read(what, rows)


def run_plain(kind, M, N, K, epi, what, g2="default", **kw):
    """A non-GELU epilogue on operands `kind`: bit equality (and exact planes on the dense operands)."""
    o, d = operands(kind, M, N, K, g2)
    got, pl = launch(o, d, epi, what, **kw)
    assert_bits(got, want_bits(kind, M, N, K, epi, g2), what)
    if pl is not None:
        assert_planes(pl, got, what, is_exact=(kind == "dense"))


def run_gelu(kind, M, N, K, epi, what, **kw):
    o, d = operands(kind, M, N, K)
    got, _ = launch(o, d, epi, what, **kw)
    assert_gelu(got, pre_act(kind, M, N, K, epi), what)


def g2s_of(M):
    return exact.PATCH_G2[M]


KERNELS = [0, 1, 5]   # 0: the per-shape defaults (kernel and tile group)


def _what(epi, M, N, K, kern, extra=""):
    return f"EPI_{NAMES[epi]} ({M}, {N}, {K}) kernel {kern}{' ' + extra if extra else ''}"


def all_epilogues(M, N, K, tag):
    """Every epilogue of vpf_gemm_bf16 once on the dense operands (the tile-order sweep)."""
    for epi in (BIAS, LN):
        run_plain("dense", M, N, K, epi, _what(epi, M, N, K, tag))
    run_plain("dense", M, N, K, RES, _what(RES, M, N, K, tag), inplace=True, stats_out=True)
    run_plain("dense", M, N, K, PATCH, _what(PATCH, M, N, K, tag), stats_out=True)
    for epi in (BIAS_GELU, LN_GELU):
        run_gelu("dense", M, N, K, epi, _what(epi, M, N, K, tag))


# ---- vpf_gemm_bf16: the six epilogues --------------------------------------------------------------------------------

@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("M,N,K", exact.SHAPES)
def test_epilogues_dense(M, N, K, kern):
    """All six epilogues on the dense exact operands (shapes: module docstring), on kernel 1 (k_gemm_bf16), kernel 5
    (k_gemm_pp) and the per-shape defaults: bf16 bit equality with the float64 reference rounded by the project's
    bf16 rule (residual: bf16(bf16(acc + b) + r); patch: bf16(bf16(acc + b) + pos)), the GELU bar for the two GELU
    epilogues. LN statistics as {mean, rstd}, 16-byte aligned and 8 bytes into their allocation (the 4-byte DMA form
    on even M). BIAS_RESIDUAL out of place and in place, with and without stats_out; the planes are bit-equal to the
    exact {sum, sumsq} of the stored integers, the partial last plane (N % 64 != 0) included. EPI_PATCH with every g2
    of the shape (25 and 40 at M = 600, 60 at M = 300: images across the 128-row wave and 256-row tile boundaries,
    also at partial N tiles): output and planes go to the token rows, the CLS rows of both keep the sentinel."""
    with tuned(kern):
        run_plain("dense", M, N, K, BIAS, _what(BIAS, M, N, K, kern))
        run_gelu("dense", M, N, K, BIAS_GELU, _what(BIAS_GELU, M, N, K, kern))
        for inplace in (False, True):
            for stats_out in (False, True):
                run_plain("dense", M, N, K, RES, _what(RES, M, N, K, kern, f"inplace={inplace} stats={stats_out}"),
                          inplace=inplace, stats_out=stats_out)
        for g2 in g2s_of(M):
            for stats_out in (False, True):
                run_plain("dense", M, N, K, PATCH, _what(PATCH, M, N, K, kern, f"g2={g2} stats={stats_out}"), g2=g2,
                          stats_out=stats_out)
        for off in (0, 2):
            run_plain("dense", M, N, K, LN, _what(LN, M, N, K, kern, f"stats +{4 * off} B"), off=off)
            run_gelu("dense", M, N, K, LN_GELU, _what(LN_GELU, M, N, K, kern, f"stats +{4 * off} B"), off=off)


@pytest.mark.parametrize("kern", [1, 5])
@pytest.mark.parametrize("M,N,K", exact.SHAPES)
def test_epilogues_coded(M, N, K, kern):
    """The product switched off (A = 0) and every epilogue operand naming its index: bias, colsum and pos rows coded
    by column, mean and the residual by row. Bit equality for BIAS, BIAS_RESIDUAL (in place, with planes), PATCH and
    LN; for the GELU epilogues one operand at a time carries a code from the separated set (bias; colsum; mean; rstd)
    and the output must be within the GELU bar of that code's image, which no other code's image is."""
    with tuned(kern):
        run_plain("coded", M, N, K, BIAS, _what(BIAS, M, N, K, kern, "coded"))
        run_plain("coded", M, N, K, RES, _what(RES, M, N, K, kern, "coded"), inplace=True, stats_out=True)
        run_plain("coded", M, N, K, RES, _what(RES, M, N, K, kern, "coded, out of place"))
        for g2 in g2s_of(M):
            run_plain("coded", M, N, K, PATCH, _what(PATCH, M, N, K, kern, f"coded g2={g2}"), g2=g2, stats_out=True)
        for off in (0, 2):
            run_plain("coded", M, N, K, LN, _what(LN, M, N, K, kern, f"coded, stats +{4 * off} B"), off=off)
        run_gelu("gelu:bias", M, N, K, BIAS_GELU, _what(BIAS_GELU, M, N, K, kern, "coded bias"))
        for i, which in enumerate(exact.GELU_CODED):
            run_gelu("gelu:" + which, M, N, K, LN_GELU, _what(LN_GELU, M, N, K, kern, "coded " + which),
                     off=2 * (i & 1))


@pytest.mark.parametrize("group", [0, 1, 2, 8])
@pytest.mark.parametrize("kern", [1, 5])
def test_tile_orders_write_every_tile_once(kern, group):
    """(600, 520, 256): 9 workgroups (not a multiple of 8: xcd_first's r != 0 branch) and 3 row panels (the last
    group of 2 has one panel, the only group of 8 has three: gsz < group). Under plain row-major order (0) and groups
    of 1, 2 and 8 every epilogue gives the expected bits inside a sentinel-filled buffer: every tile was written, and
    by the block that computed it."""
    M, N, K = 600, 520, 256
    with tuned(kern, group):
        all_epilogues(M, N, K, f"{kern} group {group}")


# ---- LN statistics as planes -----------------------------------------------------------------------------------------

def run_planes(M, N, K, P, kern, off):
    """LN and LN_GELU with the statistics as P planes in the planes form: coded operands (bit equality; GELU bar), and
    the dense product with the dense statistics (the interval of the combine's deviation; GELU bar widened by it)."""
    tag = f"P={P}, stats +{4 * off} B"
    o, d = operands("coded_planes", M, N, K)
    got, _ = launch(o, d, LN, _what(LN, M, N, K, kern, tag), stats=exact.planes_form(o.mean, o.rstd, K, P), P=P,
                    off=off)
    assert_bits(got, want_bits("coded_planes", M, N, K, LN), _what(LN, M, N, K, kern, "coded " + tag))
    o, d = operands("gcoded_planes", M, N, K)
    got, _ = launch(o, d, LN_GELU, _what(LN_GELU, M, N, K, kern, tag), stats=exact.planes_form(o.mean, o.rstd, K, P),
                    P=P, off=off)
    pre = pre_act("gcoded_planes", M, N, K, LN_GELU)
    assert_gelu(got, pre, _what(LN_GELU, M, N, K, kern, "coded " + tag), slack=exact.PLANES_DEV * np.abs(pre))
    o, d = operands("dense", M, N, K)
    pl = exact.planes_form(o.mean, o.rstd, K, P)
    slack = dense_slack(M, N, K)
    got, _ = launch(o, d, LN, _what(LN, M, N, K, kern, tag), stats=pl, P=P, off=off)
    assert_interval(got, pre_act("dense", M, N, K, LN), slack, _what(LN, M, N, K, kern, "dense " + tag))
    got, _ = launch(o, d, LN_GELU, _what(LN_GELU, M, N, K, kern, tag), stats=pl, P=P, off=off)
    assert_gelu(got, pre_act("dense", M, N, K, LN_GELU), _what(LN_GELU, M, N, K, kern, "dense " + tag), slack=slack)


@functools.lru_cache(maxsize=None)
def dense_slack(M, N, K):
    return exact.dense_planes_slack(operands("dense", M, N, K)[0])


@pytest.mark.parametrize("kern", [1, 5])
@pytest.mark.parametrize("M,N,K", exact.SHAPES)
def test_ln_planes(M, N, K, kern):
    """LN and LN_GELU reading P = 1, 12, 13 and 15 statistics planes (15: the most that fit next to bias and colsum),
    16-byte aligned (the 16-byte DMA form on even M, pieces dealt round-robin over the waves) and 8 bytes into their
    allocation (the 4-byte form). Row m's sum sits in plane m % P and its sumsq in plane (m + 1) % P, so a dropped
    plane or component changes the rows it decides."""
    with tuned(kern):
        for P in (1, 12, 13, 15):
            for off in (0, 2):
                run_planes(M, N, K, P, kern, off)


@pytest.mark.parametrize("kern", [1, 5])
@pytest.mark.parametrize("M,N,K", [(257, 256, 128), (300, 384, 192), (600, 520, 256)])
def test_ln_planes_wide(M, N, K, kern):
    """P = 16: the wide form of kernel 1 (kernel 5 falls back to it), whose planes land in ring slot (nk + 1) % 3 at
    the last K-step, at nk = 2, 3 and 4 (nk % 3 = 2, 0, 1). The dense product shows that the landing planes leave the
    K-tiles still in use alone."""
    with tuned(kern):
        for off in (0, 2):
            run_planes(M, N, K, 16, kern, off)


# ---- the producers' MX8 copies ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kern", [1, 5])
@pytest.mark.parametrize("M,N,K", [(300, 384, 192), (5, 128, 320)])
def test_producer_mx8_copies(M, N, K, kern):
    """The MX8-copy instances of BIAS_RESIDUAL and PATCH (N % 128 == 0) on both kernels: the bf16 bits are exact, the
    statistics planes exact, and the element codes and scale bytes equal quantize_mx8 of the stored rows; the CLS rows
    of the copy, the columns and rows around it and the scale bricks beyond the last row keep their canaries."""
    with tuned(kern):
        for kind in ("dense", "coded"):
            run_plain(kind, M, N, K, RES, _what(RES, M, N, K, kern, kind + " + MX8 copy"), inplace=True, stats_out=True,
                      copy8=True)
            run_plain(kind, M, N, K, RES, _what(RES, M, N, K, kern, kind + " + MX8 copy, out of place"), copy8=True)
            for g2 in g2s_of(M):
                run_plain(kind, M, N, K, PATCH, _what(PATCH, M, N, K, kern, f"{kind} g2={g2} + MX8 copy"), g2=g2,
                          stats_out=True, copy8=True)


# ---- vpf_gemm_bf16_splitk --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def strided(kind, M, N, K):
    o = operands(kind, M, N, K)[0]
    return o, Dev(o, strided=True)


def launch_splitk(o, d, epi, S, what, inplace=True, stats_out=False):
    M, N, K = o.M, o.N, o.K
    out = OutBuf(M, N)
    res = resbuf = None
    if epi == RES:
        if inplace:
            out.fill(o.residual)
            res = out.ptr
        else:
            resbuf = OutBuf(M, N)
            resbuf.fill(o.residual)
            res = resbuf.ptr
    st = _dev_f32(o.row_stats(), 2) if epi in (LN, LN_GELU) else None
    pl = PlanesBuf(N // 64, M) if stats_out else None
    spare = 64
    ws = torch.full(((S * M * N + spare) * 4,), SENT, dtype=torch.uint8, device=DEV)
    E().call("vpf_gemm_bf16_splitk", d.a.data_ptr(), d.lda, d.w.data_ptr(), d.bias.data_ptr(), res,
             None if st is None else st.data_ptr(), d.colsum.data_ptr() if st is not None else None, out.ptr, out.ld,
             M, N, K, epi, S, None if pl is None else pl.ptr, ws.data_ptr(), S * M * N, E().stream_ptr())
    torch.cuda.synchronize()
    tail = ws[S * M * N * 4:].cpu().numpy()
    assert (tail == SENT).all(), f"{what}: the split-K workspace was written beyond S M N elements"
    part = ws[:S * M * N * 4].cpu().numpy().view(np.float32).reshape(S, M, N).astype(np.float64)
    bad = part.sum(0) != o.acc
    exact.require(bad, lambda: f"{what}: partial planes\n" + exact.diff_report(bad, part.sum(0), o.acc))
    got = out.read(what)
    if resbuf is not None:
        assert np.array_equal(resbuf.read(what + " (residual)"), o.residual), f"{what}: the residual was written"
    return got, None if pl is None else pl.read(what)


@pytest.mark.parametrize("M,N,K", exact.SHAPES)
def test_splitk(M, N, K):
    """vpf_gemm_bf16_splitk with S = 1, 2, 3 splits (where K % (64 S) == 0) and its five epilogues on the dense and
    coded operands, with row-strided A (lda = K + 8), out and residual (row stride N + 24), the residual in place and
    out of place, with stats_out where N % 64 == 0. The fp32 partial planes sum to the exact integer product (every
    split ran its own K range, once), nothing is written past S M N workspace elements, and k_splitk_reduce's outputs
    are bit-equal (GELU: within the GELU bar) with exact statistics planes."""
    for S in (1, 2, 3):
        if K % (64 * S):
            continue
        for kind in ("dense", "coded"):
            o, d = strided(kind, M, N, K)
            for epi in (BIAS, LN):
                what = f"split-K S={S} {kind} EPI_{NAMES[epi]} ({M}, {N}, {K})"
                got, _ = launch_splitk(o, d, epi, S, what)
                assert_bits(got, want_bits(kind, M, N, K, epi), what)
            for inplace in (True, False):
                what = f"split-K S={S} {kind} EPI_BIAS_RESIDUAL ({M}, {N}, {K}) inplace={inplace}"
                got, pl = launch_splitk(o, d, RES, S, what, inplace=inplace, stats_out=(N % 64 == 0 and inplace))
                assert_bits(got, want_bits(kind, M, N, K, RES), what)
                if pl is not None:
                    assert_planes(pl, got, what, is_exact=(kind == "dense"))
        o, d = strided("dense", M, N, K)
        for epi in (BIAS_GELU, LN_GELU):
            what = f"split-K S={S} dense EPI_{NAMES[epi]} ({M}, {N}, {K})"
            got, _ = launch_splitk(o, d, epi, S, what)
            assert_gelu(got, pre_act("dense", M, N, K, epi), what)
        for which in exact.GELU_CODED:
            o, d = strided("gelu:" + which, M, N, K)
            for epi in ((BIAS_GELU, LN_GELU) if which == "bias" else (LN_GELU,)):
                what = f"split-K S={S} coded {which} EPI_{NAMES[epi]} ({M}, {N}, {K})"
                got, _ = launch_splitk(o, d, epi, S, what)
                assert_gelu(got, pre_act("gelu:" + which, M, N, K, epi), what)


# ---- vpf_gemm_f32 ----------------------------------------------------------------------------------------------------

F32_G2 = {300: 60, 129: 43, 5: 1}


@pytest.mark.parametrize("M,N,K", exact.F32_SHAPES)
def test_gemm_f32_exact(M, N, K):
    """vpf_gemm_f32 (128 x 128 tiles, K-blocks of 32) at (300, 136, 32): three row tiles with a 44-row edge, an
    8-column N edge tile, a single K-block; (129, 264, 96): a one-row M edge tile, three column tiles; (5, 128, 64).
    fp32 bit equality on the dense and coded operands for BIAS, BIAS_RESIDUAL (in place and out of place), PATCH and
    LN; the GELU epilogues against float64 at 2e-5. Outputs inside sentinel-filled buffers."""
    g2 = F32_G2[M]
    for kind in ("dense", "coded"):
        o = BUILDERS[kind](M, N, K, g2)
        a = _dev_f32(exact.bf16_val(o.a))
        w = _dev_f32(exact.bf16_val(o.w))
        bias, colsum, pos, st = _dev_f32(o.bias), _dev_f32(o.colsum), _dev_f32(o.pos), _dev_f32(o.row_stats())
        r32 = exact.bf16_val(o.residual).astype(np.float32)
        for epi in range(6):
            for inplace in ((False, True) if epi == RES else (False,)):
                what = f"f32 {kind} EPI_{NAMES[epi]} ({M}, {N}, {K}) inplace={inplace}"
                R = (M // g2) * (g2 + 1) if epi == PATCH else M
                rows = exact.patch_rows(M, g2) if epi == PATCH else None
                out = OutBuf(R, N, np.uint32)
                res = None
                if epi == RES:
                    resbuf = out if inplace else OutBuf(M, N, np.uint32)
                    resbuf.fill(r32.view(np.uint32))
                    res = resbuf.ptr
                ln = epi in (LN, LN_GELU)
                E().call("vpf_gemm_f32", a.data_ptr(), K, w.data_ptr(), bias.data_ptr(), res,
                         pos.data_ptr() if epi == PATCH else None, g2 if epi == PATCH else 0,
                         st.data_ptr() if ln else None, colsum.data_ptr() if ln else None, out.ptr, out.ld, M, N, K,
                         epi, E().stream_ptr())
                torch.cuda.synchronize()
                got = out.read(what, rows).view(np.float32)
                if epi in (BIAS_GELU, LN_GELU):
                    ref = exact.gelu64(exact.pre_activation(o, epi).astype(np.float64))
                    bad = ~(np.abs(got - ref) <= 2e-5 + 2e-5 * np.abs(ref)) | (got.view(np.uint32) == 0xABABABAB)
                    exact.require(bad, lambda: what + "\n" + exact.diff_report(bad, got, ref, (128, 128), (64, 64)))
                else:
                    want = exact.want_f32(o, epi)
                    bad = got.view(np.uint32) != want.view(np.uint32)
                    exact.require(bad, lambda: what + "\n" + exact.diff_report(
                        bad, got.view(np.uint32), want.view(np.uint32), (128, 128), (64, 64)))
