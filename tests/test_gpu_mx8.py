"""GPU (MI355X): the MX-fp8 path (BASELINE.json configs[4]) — quantiser, block-scaled GEMM
and the fp8 copies written by GEMM epilogues — through the product ops / C-ABI.

References: quantisation is bit-exact against the CPU oracle oracle/mx8.py (the rule in include/vpf.h "MX8
operands": smallest block exponent with amax * 2^-E <= 448, RNE to e4m3fn; pinned by tests/test_oracle_mx8.py);
GEMMs against float64 products of the dequantised operands (so the tolerance covers only fp32 accumulation order
and the final bf16 rounding); every fp8 copy written by an epilogue must equal vpf_quantize_mx8 of the bf16
values the same epilogue stored, bit for bit. Scale and element routing is pinned exactly: power-of-two operands
built by the CPU oracle (tests/test_oracle_mx8.py "exact-routing operands") make every output one product, compared as
bf16 bits. Outputs that are views of larger buffers are surrounded by canary bytes that must survive."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import test_oracle_mx8 as routing   # the exact-routing operand builders, proven fair on the CPU there

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()


def vpf():
    return torch.ops.vpf


def ops():
    from vitparticlefiltertracker_amd import ops as o
    return o


def E():
    from vitparticlefiltertracker_amd import _lib
    return _lib


def ref_quant(x: torch.Tensor):
    """The oracle's MX8 rule (oracle/mx8.py, pinned by tests/test_oracle_mx8.py): (uint8[rows][K] codes,
    int32[rows][K/32] scale bytes)."""
    from oracle import mx8 as omx8
    bits = x.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)
    codes, sc = omx8.quantize(bits)
    return torch.from_numpy(codes), torch.from_numpy(sc.astype(np.int32))


def quant(x: torch.Tensor):
    q, s = ops().mx8_empty(x.shape[0], x.shape[1], DEV)
    vpf().quantize_mx8_(x, 1, q, s)
    return q, s


def special_rows(K):
    """Rows exercising the block-exponent edges: zeros, subnormal bf16, mantissa 1.75 vs 1.7578 at the top,
    huge / tiny magnitudes, mixed signs."""
    rows = []
    z = torch.zeros(K)
    rows.append(z.clone())
    r = torch.zeros(K); r[::7] = 1e-39; rows.append(r)                     # bf16 subnormals
    for top in (1.75, 1.7578125, 1.0, 1.9921875):
        r = torch.linspace(-1, 1, K) * 0.3; r[5::32] = top * 2.0 ** 10; rows.append(r)
    rows.append(torch.linspace(-3e30, 3e30, K))
    rows.append(torch.linspace(-3e-30, 3e-30, K))
    return torch.stack(rows).to(torch.bfloat16)


@pytest.mark.parametrize("rows,K", [(1, 128), (77, 256), (300, 768), (64, 3072)])
def test_quantize_bit_exact(rows, K):
    g = torch.Generator().manual_seed(rows * K)
    x = (torch.randn(rows, K, generator=g) * torch.exp2(torch.randint(-20, 20, (rows, 1), generator=g).float()))
    x = torch.cat([x.to(torch.bfloat16), special_rows(K)])
    xd = x.to(DEV)
    q, s = quant(xd)
    rq, rs = ref_quant(x)
    assert torch.equal(q.cpu(), rq), f"{(q.cpu() != rq).sum().item()} element codes differ"
    assert torch.equal(ops().mx8_scale_bytes(s, x.shape[0]).cpu(), rs)
    # dequantised values are within half an e4m3 ulp (2^-4 relative) of the input, or exactly 0 below range
    deq = ops().mx8_dequantize(q, s).cpu()
    xf = x.float()
    ok = (deq - xf).abs() <= xf.abs() * 2.0 ** -4 + torch.exp2(rs.float() - 127 - 9).repeat_interleave(32, 1)
    assert bool(ok.all())


def test_quantize_strided_rows():
    """out_stride > 1 (the CLS rows of a token tensor) and a row-strided source view."""
    n, N, D = 9, 5, 256
    tok = (torch.randn(n, N, D, device=DEV)).to(torch.bfloat16)
    cls = tok.view(n, N * D)[:, :D]
    q, s = ops().mx8_empty(n * N, D, DEV)
    q.zero_(); s.zero_()
    vpf().quantize_mx8_(cls, N, q, s)
    rq, rs = ref_quant(cls.contiguous())
    assert torch.equal(q[::N].cpu(), rq)
    assert torch.equal(ops().mx8_scale_bytes(s, n * N)[::N].cpu(), rs)


def _weights(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(DEV)
    q, s = ops().mx8_empty(N, K, DEV)
    vpf().quantize_mx8_(w, 1, q, s)
    assert s.shape[1] == N
    return q, s, ops().mx8_dequantize(q, s).double()


def _acts(M, K, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * scale + 0.2).to(torch.bfloat16).to(DEV)
    q, s = quant(x)
    return x, q, s, ops().mx8_dequantize(q, s).double()


def _check(out, ref, lin, A, Wd, extra=0.0):
    """|out - ref| within: the bf16 rounding of the stored value (2^-8 relative: half an ulp, with margin), the
    bf16 rounding of the GEMM value before a residual add (2^-8 |lin|), the block-scaled MFMA's accumulation
    (measured ~1e-5 of sum |a w|; bound 2^-13), and `extra` (the GELU approximation, 2.7e-4)."""
    mag = A.abs() @ Wd.abs().t()
    bound = 2 ** -8 * (ref.abs() + lin.abs()) + 2 ** -13 * mag + extra + 1e-6
    bad = (out.double() - ref).abs() > bound
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} outside the bound; worst excess " \
        f"{((out.double() - ref).abs() - bound).max().item():.3g}"


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


@pytest.mark.parametrize("M,N,K", [(777, 256, 128), (300, 768, 768), (1024, 384, 3072), (5, 128, 256)])
@pytest.mark.parametrize("epi", ["bias", "gelu", "res"])
def test_gemm_mx8_plain_epilogues(M, N, K, epi):
    _, a8, as8, A = _acts(M, K, M + K)
    w8, ws8, Wd = _weights(N, K, N + K)
    bias = torch.randn(N, device=DEV) * 0.1
    lin = A @ Wd.t() + bias.double()
    code = {"bias": E().VPF_EPI_BIAS, "gelu": E().VPF_EPI_BIAS_GELU, "res": E().VPF_EPI_BIAS_RESIDUAL}[epi]
    out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    res = None
    if epi == "res":
        out = (torch.randn(M, N, device=DEV)).to(torch.bfloat16)
        res = out
        ref = out.double() + lin
    else:
        ref = gelu(lin) if epi == "gelu" else lin
    vpf().gemm_mx8(a8, as8, w8, ws8, bias, res, None, None, code, out)
    _check(out, ref, lin, A, Wd, 5e-4 if epi == "gelu" else 0.0)


EPS = 1e-6


class _Fold:
    """One LN-fold case: the residual stream h [M][K] (bf16) and its MX8 form, W' = MX8(W diag(gamma)), colsum of
    value(W'), b' = b + W beta; float64 views of the quantised operands for the references."""

    def __init__(self, M, K, N):
        self.M, self.K, self.N = M, K, N
        self.h, self.a8, self.as8, self.A = _acts(M, K, 7 * M + K, scale=0.8)
        g = torch.Generator().manual_seed(N)
        self.gamma = 1 + 0.2 * torch.randn(K, generator=g)
        self.beta = 0.1 * torch.randn(K, generator=g)
        self.W = torch.randn(N, K, generator=g) / math.sqrt(K)
        self.b = 0.1 * torch.randn(N, generator=g)
        Wg = (self.W * self.gamma).to(torch.bfloat16).to(DEV)
        self.w8, self.ws8 = ops().mx8_empty(N, K, DEV)
        vpf().quantize_mx8_(Wg, 1, self.w8, self.ws8)
        self.Wd = ops().mx8_dequantize(self.w8, self.ws8)
        self.colsum = self.Wd.sum(1).float().contiguous()
        self.bias = (self.b + self.W @ self.beta).to(DEV)
        self.hd = self.h.double()

    def planes(self, edges=None):
        """{sum, sumsq} of h's rows over the column blocks [edges[t], edges[t+1]) (default: K/64 blocks of 64)."""
        edges = edges or list(range(0, self.K + 1, 64))
        return torch.stack([torch.stack([self.hd[:, lo:hi].sum(1), (self.hd[:, lo:hi] ** 2).sum(1)], 1)
                            for lo, hi in zip(edges[:-1], edges[1:])]).float().contiguous()

    def row_stats(self):
        st = torch.empty(self.M, 2, device=DEV)
        vpf().row_stats(self.h, EPS, st)
        return st

    def lin(self, bias=None):
        """The fold's exact algebra on the quantised operands: rstd (value(A) W'^T - mean colsum) + b'."""
        mean = self.hd.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(self.hd.var(1, unbiased=False, keepdim=True) + EPS)
        bias = self.bias if bias is None else bias
        return rstd * (self.A @ self.Wd.double().t() - mean * self.colsum.double()) + bias.double()

    def check(self, out, gelu_epi):
        lin = self.lin()
        ref = gelu(lin) if gelu_epi else lin
        torch.testing.assert_close(out.double(), ref, rtol=2 ** -8, atol=2e-3)
        # and against LayerNorm -> GEMM in float64 on the unquantised operands: the fp8 error itself (reported bound)
        full = Fn.layer_norm(self.hd, (self.K,), self.gamma.double().to(DEV), self.beta.double().to(DEV), EPS) \
            @ self.W.double().to(DEV).t() + self.b.double().to(DEV)
        full = gelu(full) if gelu_epi else full
        rel = ((out.double() - full).norm() / full.norm()).item()
        assert rel < 0.06, rel

    def run(self, st, P, gelu_epi):
        out = torch.empty(self.M, self.N, device=DEV, dtype=torch.bfloat16)
        code = E().VPF_EPI_LN_GELU if gelu_epi else E().VPF_EPI_LN
        vpf().gemm_mx8(self.a8, self.as8, self.w8, self.ws8, self.bias, None, st, self.colsum, code, out, P, EPS)
        return out


# M = 777, 513 (odd): the 4-byte statistics DMA; M = 2, 394, 512 (even, 16-B aligned statistics): the 16-byte form the
# product runs (M = n 197 is even), with its clamp on the M edge tile (394) and on a tile shorter than one piece (2);
# K = 128: two planes, a single K-tile.
@pytest.mark.parametrize("M,K,N", [(777, 768, 2304), (513, 256, 384), (2, 256, 128), (394, 256, 384), (512, 256, 256),
                                   (394, 128, 128)])
@pytest.mark.parametrize("gelu_epi", [False, True])
@pytest.mark.parametrize("planes", [False, True])
def test_gemm_mx8_layernorm_fold(M, K, N, gelu_epi, planes):
    """LN-folded MX8 GEMM on the raw residual stream: A = MX8(h), W' = MX8(W diag(gamma)), colsum of value(W')."""
    c = _Fold(M, K, N)
    st, P = (c.planes(), K // 64) if planes else (c.row_stats(), 0)
    c.check(c.run(st, P, gelu_epi), gelu_epi)


@pytest.mark.parametrize("gelu_epi", [False, True])
@pytest.mark.parametrize("planes", [False, True])
def test_gemm_mx8_layernorm_fold_unaligned_stats(gelu_epi, planes):
    """Even M with the statistics 8 bytes into their allocation (8-B but not 16-B aligned): the 4-byte DMA form."""
    M, K, N = 394, 256, 384
    c = _Fold(M, K, N)
    st, P = (c.planes(), K // 64) if planes else (c.row_stats(), 0)
    buf = torch.empty(st.numel() + 2, device=DEV)
    view = buf[2:].view(st.shape)
    view.copy_(st)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    c.check(c.run(view, P, gelu_epi), gelu_epi)


@pytest.mark.parametrize("M", [394, 301])
@pytest.mark.parametrize("gelu_epi", [False, True])
def test_gemm_mx8_layernorm_fold_13_planes(M, gelu_epi):
    """stats_parts = 13, the most the kernel keeps in LDS: disjoint column blocks need not be 64 wide (vpf.h), so
    K = 896 as 12 blocks of 64 and one of 128. 14 planes are rejected."""
    K, N = 896, 128
    c = _Fold(M, K, N)
    st = c.planes(list(range(0, 769, 64)) + [896])
    assert st.shape[0] == 13
    c.check(c.run(st, 13, gelu_epi), gelu_epi)
    st14 = torch.cat([st, torch.zeros_like(st[:1])])
    with pytest.raises(E().VPFError):
        c.run(st14, 14, gelu_epi)


@pytest.mark.parametrize("gelu_epi", [False, True])
def test_gemm_mx8_layernorm_fold_combined_stats(gelu_epi):
    """Beyond 13 planes (ViT-L: K = 1024, 16 planes) vit.py combines them with stats_combine_ and passes {mean, rstd}
    with stats_parts = 0. At K = 768 (12 planes) both routes exist and write the same bits (vpf.h)."""
    M, N = 394, 128
    c = _Fold(M, 1024, N)
    st = torch.empty(M, 2, device=DEV)
    vpf().stats_combine_(c.planes(), 1024, EPS, st)
    c.check(c.run(st, 0, gelu_epi), gelu_epi)
    c = _Fold(M, 768, N)
    pl = c.planes()
    st = torch.empty(M, 2, device=DEV)
    vpf().stats_combine_(pl, 768, EPS, st)
    out_planes, out_comb = c.run(pl, 12, gelu_epi), c.run(st, 0, gelu_epi)
    c.check(out_planes, gelu_epi)
    c.check(out_comb, gelu_epi)
    assert torch.equal(out_planes, out_comb)


def test_gemm_mx8_q8_output_matches_quantizer():
    """FC1-style: the fp8-only output of gemm_mx8_q8_ == quantize_mx8(bf16 output of the same GEMM)."""
    M, K, N = 777, 768, 3072
    _, a8, as8, _ = _acts(M, K, 3)
    w8, ws8, _ = _weights(N, K, 4)
    bias = torch.randn(N, device=DEV) * 0.1
    out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    st = torch.stack([torch.rand(M, device=DEV) * 0.2 - 0.1, torch.rand(M, device=DEV) + 0.5], 1).contiguous()
    colsum = torch.randn(N, device=DEV)
    LNG = E().VPF_EPI_LN_GELU
    vpf().gemm_mx8(a8, as8, w8, ws8, bias, None, st, colsum, LNG, out)
    q, s = ops().mx8_empty(M, N, DEV)
    vpf().gemm_mx8_q8_(a8, as8, w8, ws8, bias, st, colsum, LNG, q, s)
    rq, rs = quant(out)
    assert torch.equal(q, rq)
    assert torch.equal(ops().mx8_scale_bytes(s, M), ops().mx8_scale_bytes(rs, M))


# ---- exact scale and element routing: operands from the CPU oracle, every output one power-of-two product ----------

def _upload(bits, lds):
    """bf16 bit rows -> the oracle's MX8 operand on the device: (codes, scale bytes) on the CPU, (q, s) uploaded."""
    from oracle import mx8 as omx8
    codes, sc = omx8.quantize(bits)
    q = torch.from_numpy(codes).to(DEV)
    s = torch.from_numpy(omx8.pack_scales(sc, lds)).to(DEV)
    return codes, sc, q, s


def _routing_cases(M, N, K, onehot):
    """(a8, as8, w8, ws8, float64 oracle product) per repetition of tests/test_oracle_mx8.py routing_pairs, which
    proves on the CPU that the product is exact in bf16 and that the repetitions select every k."""
    from oracle import mx8 as omx8
    seen = np.zeros(K, dtype=bool)
    for a_bits, _, w_bits, _, k in routing.routing_pairs(M, N, K, onehot):
        seen[k] = True
        ac, asc, a8, as8 = _upload(a_bits, (M + 63) // 64 * 64)
        wc, wsc, w8, ws8 = _upload(w_bits, N)
        yield a8, as8, w8, ws8, torch.from_numpy(omx8.gemm(ac, asc, wc, wsc))
    assert seen.all()


def _bits(t):
    return t.contiguous().cpu().view(torch.int16)


@pytest.mark.parametrize("M,N,K", routing.ROUTING_SHAPES)
@pytest.mark.parametrize("onehot", ["a", "w"])
def test_gemm_mx8_exact_routing(M, N, K, onehot):
    """One-hot x dense power-of-two operands with heterogeneous block scales (exponents over [-8, 8]): the bf16 output
    bits equal the oracle's. A one-hot A with W dense checks every W element and W scale byte, a one-hot W every A's:
    M and N edge tiles with both ring buffers used twice (K = 512), a single K-tile, an odd K-tile count with a single
    64-column tile, and M < 64."""
    bias = torch.zeros(N, device=DEV)
    for a8, as8, w8, ws8, ref in _routing_cases(M, N, K, onehot):
        out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        vpf().gemm_mx8(a8, as8, w8, ws8, bias, None, None, None, E().VPF_EPI_BIAS, out)
        want = ref.to(torch.bfloat16)
        bad = _bits(out) != _bits(want)
        assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} outputs differ; first at " \
            f"{bad.nonzero()[0].tolist()}: got {out.cpu()[bad][0].item()}, want {want[bad][0].item()}"


# The fp8-only outputs need whole scale planes (N % 128 == 0, vpf.h), so of the routing shapes only (5, 128, 256) can
# run there; (300, 384, 512) and (300, 128, 128) stand in for the rest: a partial N tile whose last valid W row is the
# clamp of the wperm16 staging, M edge tiles, four K-tiles and one.
@pytest.mark.parametrize("M,N,K", [(5, 128, 256), (300, 384, 512), (300, 128, 128)])
def test_gemm_mx8_fc1_exact_routing(M, N, K):
    """The FC1 instance (fp8-only LN + GELU output, W rows staged in wperm16 order, scale word reassembled by two
    v_perm_b32) on the one-hot A x dense W pair: {mean, rstd} = {0, 1}, colsum = bias = 0, so the epilogue is
    gelu(acc). Codes and scale bytes equal quantize_mx8 of the bf16 output of gemm_mx8 with the same arguments, whose
    scale routing test_gemm_mx8_exact_routing pins."""
    bias = torch.zeros(N, device=DEV)
    colsum = torch.zeros(N, device=DEV)
    st = torch.tensor([0.0, 1.0], device=DEV).repeat(M, 1).contiguous()
    LNG = E().VPF_EPI_LN_GELU
    for a8, as8, w8, ws8, ref in _routing_cases(M, N, K, "a"):
        out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        vpf().gemm_mx8(a8, as8, w8, ws8, bias, None, st, colsum, LNG, out)
        want = gelu(ref.to(DEV))
        assert bool(((out.double() - want).abs() <= 2 ** -8 * want.abs() + 5e-4).all())
        q, s = ops().mx8_empty(M, N, DEV)
        vpf().gemm_mx8_q8_(a8, as8, w8, ws8, bias, st, colsum, LNG, q, s)
        rq, rs = quant(out)
        assert torch.equal(q, rq), f"{int((q != rq).sum())} element codes differ"
        assert torch.equal(ops().mx8_scale_bytes(s, M), ops().mx8_scale_bytes(rs, M))


# ---- fp8-only outputs: every epilogue, edge tiles, padded outputs ------------------------------------------------

CANARY = 0xAB


def _canary_u8(rows, cols):
    return torch.full((rows, cols), CANARY, device=DEV, dtype=torch.uint8)


def _canary_scales(planes, M):
    """Scale planes with one 64-row brick more than M needs, every byte the canary."""
    lds = 64 * ((M + 63) // 64 + 1)
    return _canary_u8(planes, lds * 4).view(torch.int32)


def _assert_canary(buf, M, N):
    """Everything outside buf[:M, :N] still holds the canary bytes."""
    raw = buf.view(torch.uint8).view(buf.shape[0], -1)
    w = N * buf.element_size()
    assert bool((raw[M:] == CANARY).all()), "rows past M were written"
    assert bool((raw[:M, w:] == CANARY).all()), "columns past N were written"


def _assert_scale_canary(s, M):
    """The scale words of the bricks wholly beyond M still hold the canary."""
    tail = s[:, 64 * ((M + 63) // 64):]
    assert tail.numel() > 0 and bool((tail.contiguous().view(torch.uint8) == CANARY).all()), \
        "scale words of a brick with no row < M were written"


@pytest.mark.parametrize("M,K,N", [(300, 128, 384), (394, 384, 384), (5, 256, 128)])
@pytest.mark.parametrize("epi,planes", [("bias", False), ("gelu", False), ("ln", False), ("ln", True),
                                        ("lngelu", False), ("lngelu", True)])
def test_gemm_mx8_q8_every_epilogue(M, K, N, epi, planes):
    """gemm_mx8_q8_ (fp8-only output; store_wave_tile_q8, and the direct form for LN + GELU) == quantize_mx8 of the
    bf16 output of gemm_mx8 with the same arguments, codes and scale bytes, for all four epilogues, with the LN
    statistics as {mean, rstd} rows or as planes. The bf16 output is checked against float64 here. Three 32-column
    blocks are extreme: bias -30 (after a GELU: +-0 or tiny, the zero-amax branch of mx8_block_exp), +200 and +240
    (mantissa above 1.75: its top-binade branch). Both outputs are views of larger canary-filled buffers (row stride
    > N; scale planes one brick longer than M needs): nothing outside the views is written.
    N = 384 is the partial N tile nearest the 320 columns of the bf16-output tests: fp8 outputs need N % 128 == 0."""
    c = _Fold(M, K, N)
    ln, gelu_epi = epi in ("ln", "lngelu"), epi in ("gelu", "lngelu")
    code = {"bias": E().VPF_EPI_BIAS, "gelu": E().VPF_EPI_BIAS_GELU, "ln": E().VPF_EPI_LN,
            "lngelu": E().VPF_EPI_LN_GELU}[epi]
    bias = c.bias.clone()
    bias[:32] = -30.0
    bias[32:64] = 200.0
    bias[N - 32:] = 240.0
    st, P = (None, 0)
    if ln:
        st, P = (c.planes(), K // 64) if planes else (c.row_stats(), 0)
    colsum = c.colsum if ln else None
    obuf = _canary_u8(M + 3, (N + 64) * 2).view(torch.bfloat16)
    out = obuf[:M, :N]
    vpf().gemm_mx8(c.a8, c.as8, c.w8, c.ws8, bias, None, st, colsum, code, out, P, EPS)
    _assert_canary(obuf, M, N)
    if ln:
        lin = c.lin(bias)
        torch.testing.assert_close(out.double(), gelu(lin) if gelu_epi else lin, rtol=2 ** -8, atol=2e-3)
    else:
        lin = c.A @ c.Wd.double().t() + bias.double()
        _check(out, gelu(lin) if gelu_epi else lin, lin, c.A, c.Wd.double(), 5e-4 if gelu_epi else 0.0)
    qbuf = _canary_u8(M + 3, N + 128)
    q = qbuf[:M, :N]
    s = _canary_scales(N // 128, M)
    vpf().gemm_mx8_q8_(c.a8, c.as8, c.w8, c.ws8, bias, st, colsum, code, q, s, P, EPS)
    rq, rs = quant(out)
    assert torch.equal(q, rq), f"{int((q != rq).sum())} element codes differ"
    assert torch.equal(ops().mx8_scale_bytes(s, M), ops().mx8_scale_bytes(rs, M))
    # the extreme blocks reached the branches they are there for: 200 +- 5 scales by 2^-1, 240 +- 5 by 2^0, and the
    # GELU of -30 +- 5 is -0 in every column (scale byte 0)
    sb = ops().mx8_scale_bytes(s, M)
    assert bool((sb[:, 1] == 126).all()) and bool((sb[:, -1] == 127).all())
    if gelu_epi:
        assert bool((sb[:, 0] == 0).all())
    _assert_canary(qbuf, M, N)
    _assert_scale_canary(s, M)


@pytest.mark.parametrize("N", [320, 64])
def test_fp8_outputs_need_whole_scale_planes(N):
    """An MX8 output's scale planes cover 128 columns each (vpf.h: N % 128 == 0): N = 320 and N = 64, legal for the
    bf16 output, are rejected for the fp8-only output and for the residual producer's MX8 copy."""
    M, K = 300, 128
    a8, as8 = ops().mx8_empty(M, K, DEV)
    w8 = torch.zeros(N, K, device=DEV, dtype=torch.uint8)
    ws8 = torch.zeros(K // 128, N, device=DEV, dtype=torch.int32)
    a8.zero_(); as8.zero_()
    bias = torch.zeros(N, device=DEV)
    q = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
    s = torch.zeros(max(N // 128, 1), 320, device=DEV, dtype=torch.int32)
    with pytest.raises((E().VPFError, ValueError)):
        vpf().gemm_mx8_q8_(a8, as8, w8, ws8, bias, None, None, E().VPF_EPI_BIAS, q, s)
    h = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    planes = torch.zeros((N + 63) // 64, M, 2, device=DEV)
    with pytest.raises((E().VPFError, ValueError)):
        vpf().gemm_mx8_res_(a8, as8, w8, ws8, bias, h, planes, q, s)
    assert not bool(q.any()) and not bool(s.any()) and not bool(h.any())


def _planes_ref(y, P):
    yd = y.double()
    return torch.stack([torch.stack([yd[:, 64 * t: 64 * (t + 1)].sum(1), (yd[:, 64 * t: 64 * (t + 1)] ** 2).sum(1)], 1)
                        for t in range(P)])


def _residual_producer(M, K, N, padded=False, copy8=True):
    _, a8, as8, A = _acts(M, K, 11, scale=0.3)
    w8, ws8, Wd = _weights(N, K, 12)
    bias = torch.randn(N, device=DEV) * 0.1
    h0 = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    if padded:   # h as a row-strided view of a canary-filled buffer
        hbuf = _canary_u8(M + 3, (N + 64) * 2).view(torch.bfloat16)
        h = hbuf[:M, :N]
        h.copy_(h0)
    else:
        h = h0
    ref = h.double() + A @ Wd.t() + bias.double()
    ref0 = ref
    P = (N + 63) // 64
    planes = torch.full((P, M, 2), float("nan"), device=DEV)
    lin = A @ Wd.t() + bias.double()
    if copy8:
        q, s = ops().mx8_empty(M, N, DEV)
        vpf().gemm_mx8_res_(a8, as8, w8, ws8, bias, h, planes, q, s)
    else:   # the C ABI without the MX8 copy (any N % 64 == 0)
        E().call("vpf_gemm_mx8", a8.data_ptr(), K, as8.data_ptr(), as8.shape[1], w8.data_ptr(), ws8.data_ptr(),
                 bias.data_ptr(), h.data_ptr(), None, None, h.data_ptr(), h.stride(0), None, 0, None, 0, M, N, K,
                 E().VPF_EPI_BIAS_RESIDUAL, 0, 0.0, planes.data_ptr(), E().stream_ptr())
    _check(h, ref0, lin, A, Wd)
    torch.testing.assert_close(planes.double(), _planes_ref(h, P), rtol=2e-5, atol=2e-3)
    if copy8:
        rq, rs = quant(h)
        assert torch.equal(q, rq) and torch.equal(ops().mx8_scale_bytes(s, M), ops().mx8_scale_bytes(rs, M))
    if padded:
        _assert_canary(hbuf, M, N)


def test_gemm_mx8_residual_producer():
    """FC2-style: h += value(a8) value(w8)^T + b in place, with statistics planes and the MX8 copy of h."""
    _residual_producer(777, 3072, 768)


@pytest.mark.parametrize("M,K,N", [(300, 128, 384), (394, 384, 128)])
@pytest.mark.parametrize("padded", [False, True])
def test_gemm_mx8_residual_producer_edges(M, K, N, padded):
    """The residual producer at an M edge tile with a single K-tile and a partial N tile, and at an odd K-tile count
    with two planes; also in place on a row-strided h inside a padded buffer, which stays intact around it."""
    _residual_producer(M, K, N, padded)


@pytest.mark.parametrize("padded", [False, True])
def test_gemm_mx8_residual_producer_n320(padded):
    """N = 320 (a 64-column partial N tile, five statistics planes): the MX8 copy needs N % 128 == 0
    (test_fp8_outputs_need_whole_scale_planes), so the residual add and the planes run without it."""
    _residual_producer(300, 128, 320, padded, copy8=False)


@pytest.mark.parametrize("kern", [1, 5])
@pytest.mark.parametrize("epi,K", [("res", 768), ("res", 64), ("patch", 768)])
def test_gemm_bf16_q8_copy(epi, K, kern):
    """bf16 residual-stream producers (proj, patch embed) with the MX8 copy: equal to quantize(stored rows). On both
    bf16 kernels (vpf_gemm_tune: 1 = k_gemm_bf16, the default of these epilogues, 5 = k_gemm_pp<.., OUT8>); K = 64 is
    a single K-tile, where kernel 1 issues the epilogue-operand DMA with its prologue."""
    from vitparticlefiltertracker_amd import _lib
    L = _lib.lib()
    try:
        assert L.vpf_gemm_tune(kern, -1) == 0
        _gemm_bf16_q8_copy(epi, K)
        torch.cuda.synchronize()
    finally:
        L.vpf_gemm_tune(0, -1)


def _gemm_bf16_q8_copy(epi, K):
    D = 768
    if epi == "res":
        M = 600
        a = (torch.randn(M, K, device=DEV) * 0.5).to(torch.bfloat16)
        w = (torch.randn(D, K, device=DEV) * 0.03).to(torch.bfloat16)
        bias = torch.randn(D, device=DEV) * 0.1
        out = torch.randn(M, D, device=DEV).to(torch.bfloat16)
        rows = M
        planes = torch.empty(D // 64, rows, 2, device=DEV)
        q = torch.empty(rows, D, device=DEV, dtype=torch.uint8)
        s = _canary_scales(D // 128, rows)   # one brick more than M needs: the edge tile must leave it alone
        vpf().gemm_q8_(a, w, bias, out, None, 0, E().VPF_EPI_BIAS_RESIDUAL, out, planes, q, s)
        flat = out
        sel = torch.ones(rows, dtype=torch.bool)
    else:
        n, g2 = 3, 196
        a = (torch.randn(n * g2, K, device=DEV) * 0.5).to(torch.bfloat16)
        w = (torch.randn(D, K, device=DEV) * 0.03).to(torch.bfloat16)
        bias = torch.randn(D, device=DEV) * 0.1
        pos = torch.randn(g2 + 1, D, device=DEV) * 0.1
        tok = torch.zeros(n, g2 + 1, D, device=DEV, dtype=torch.bfloat16)
        rows = n * (g2 + 1)
        planes = torch.empty(D // 64, rows, 2, device=DEV)
        q, s = ops().mx8_empty(rows, D, DEV)
        vpf().gemm_q8_(a, w, bias, None, pos, g2, E().VPF_EPI_PATCH, tok, planes, q, s)
        flat = tok.view(rows, D)
        sel = torch.ones(rows, dtype=torch.bool)
        sel[:: g2 + 1] = False          # CLS rows: not written by the GEMM
    rq, rs = quant(flat)
    assert torch.equal(q[sel.to(DEV)], rq[sel.to(DEV)])
    assert torch.equal(ops().mx8_scale_bytes(s, rows)[sel.to(DEV)], ops().mx8_scale_bytes(rs, rows)[sel.to(DEV)])
    if epi == "res":
        _assert_scale_canary(s, rows)


def test_mx8_argument_contract():
    from vitparticlefiltertracker_amd import _lib
    x = torch.zeros(64, 100, device=DEV, dtype=torch.bfloat16)   # K % 128 != 0
    q = torch.empty(64, 128, device=DEV, dtype=torch.uint8)
    s = torch.empty(1, 64, device=DEV, dtype=torch.int32)
    with pytest.raises(_lib.VPFError):
        _lib.call("vpf_quantize_mx8", x.data_ptr(), 100, 64, 100, 1, q.data_ptr(), 128, s.data_ptr(), 64,
                  _lib.stream_ptr())
    a8, as8 = ops().mx8_empty(64, 128, DEV)
    w8, ws8 = ops().mx8_empty(96, 128, DEV)        # N = 96: scale planes need N % 64 == 0
    with pytest.raises(_lib.VPFError):
        vpf().gemm_mx8(a8, as8, w8, ws8[:, :96].contiguous(), torch.zeros(96, device=DEV), None, None, None,
                       _lib.VPF_EPI_BIAS, torch.empty(64, 96, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(_lib.VPFError):   # EPI_PATCH is not an MX8 epilogue
        w8, ws8 = ops().mx8_empty(128, 128, DEV)
        vpf().gemm_mx8(a8, as8, w8, ws8[:, :128].contiguous(), torch.zeros(128, device=DEV), None, None, None,
                       _lib.VPF_EPI_PATCH, torch.empty(64, 128, device=DEV, dtype=torch.bfloat16))


def _attention_q8(B, N, H, padded=False):
    D = H * 64
    torch.manual_seed(B * N)
    qkv = (torch.randn(B, N, 3 * D, device=DEV) * 0.7).to(torch.bfloat16)
    out = torch.empty(B, N, D, device=DEV, dtype=torch.bfloat16)
    vpf().attention(qkv, H, N, out)
    if N == 1:   # one key: the softmax weight is 1 and the output is the value row itself
        assert torch.equal(out, qkv[:, :, 2 * D:])
    if padded:   # extra rows and a row stride > D
        qbuf = _canary_u8(B * N + 3, D + 64)
        q = qbuf[:B * N, :D]
        _, s = ops().mx8_empty(B * N, D, DEV)
    else:
        q, s = ops().mx8_empty(B * N, D, DEV)
    vpf().attention_q8_(qkv, H, q, s)
    rq, rs = quant(out.view(B * N, D))
    assert torch.equal(q, rq)
    assert torch.equal(ops().mx8_scale_bytes(s, B * N), ops().mx8_scale_bytes(rs, B * N))
    if padded:
        _assert_canary(qbuf, B * N, D)


# N = 256: the kernel's ceiling (8 full strips); N = 1: a single key, 31 padded queries; N = 33: a one-query tail strip
@pytest.mark.parametrize("B,N,H", [(3, 197, 12), (2, 50, 4), (5, 256, 2), (7, 1, 2), (3, 33, 4)])
def test_attention_mx8_output_matches_quantizer(B, N, H):
    """fp8 path attention: the MX8 output == quantize_mx8 of the bf16 output of the same kernel, bit for bit."""
    _attention_q8(B, N, H)


def test_attention_mx8_padded_output():
    """q8 as a view of a larger buffer (rows past B N, ld8 > D): nothing outside the view is written."""
    _attention_q8(3, 33, 4, padded=True)


def test_attention_mx8_rejects_more_than_256_tokens():
    B, N, H = 1, 257, 2
    qkv = torch.zeros(B, N, 3 * H * 64, device=DEV, dtype=torch.bfloat16)
    q, s = ops().mx8_empty(B * N, H * 64, DEV)
    with pytest.raises(E().VPFError):
        vpf().attention_q8_(qkv, H, q, s)
