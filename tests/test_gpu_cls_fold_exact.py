"""GPU (MI355X): exact token routing, token census and fractional rescales of the folded CLS attention
(vpf_cls_attn_fold_bf16, k_cls_attn_fold<6 / 12 / 16>) on the exactly computable inputs of
tests/test_oracle_cls_fold.py (built and proven fair on the CPU there: why bit equality, one bf16 ulp and
2^-7 sum p |LNraw| are the right bars is that module's docstring), and the pieces around the kernel: the G GEMM on
vit.cls_g_weight, the V GEMM into G's storage and head_gather_ as vit.py chains them, and the argument contract.

B = 3 particles; H = 6 (lanes li >= H idle), 12, 16: the three template instances. N: 15 | 16 | 17 the chunk edge,
31 | 32 | 33 where load_chunk(c + 2) is first used, 48 | 49, 256 | 257 and 512 | 513 where the statistics prologue's
loop wraps, 197 / 577 the product shapes, 1 and 640 the limits.

Every stride is above its minimum, which the op's checks do not allow (contiguous G and out), so the probes go through
the C ABI: ldg = H D + 8, ldq = 2 D, ldo = H D + 4, plane_rows = B N + 3. The planes' pad rows, G's pad and q's pad
hold NaN; out and its pad (and a spare row) hold a sentinel, which must be gone from the output and survive in the
pad.

On the MI355X the staircase outputs sat at 0.64 to 0.83 of their bar, the same figures to three digits as the fp32
restatement on the CPU; no bar needed the widening that the restatement's ulp margins would have allowed."""
import pytest
import torch

import test_oracle_cls_fold as probe   # the builders and the bars, proven on the CPU there

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = probe.B0
SENTINEL = 5.0
ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()


def E():
    from vitparticlefiltertracker_amd import _lib
    return _lib


def vpf():
    return torch.ops.vpf


class Buffers:
    """The device buffers of one call in the padded layout, filled from a probe."""

    def __init__(self, p):
        Bp, N, D = p.tok.shape
        H = D // 64
        self.B, self.N, self.H, self.D = Bp, N, H, D
        self.ldg, self.ldq, self.ldo, self.plane_rows = H * D + 8, 2 * D, H * D + 4, Bp * N + 3
        self.tok = p.tok.to(DEV).contiguous()
        self.planes = torch.full((H, self.plane_rows, 2), float("nan"), device=DEV)
        self.planes[:, :Bp * N] = p.planes.to(DEV)
        self.G = torch.full((Bp, self.ldg), float("nan"), device=DEV, dtype=torch.bfloat16)
        self.G[:, :H * D] = p.G.reshape(Bp, H * D).to(DEV)
        self.q = torch.full((Bp, self.ldq), float("nan"), device=DEV, dtype=torch.bfloat16)
        self.q[:, :D] = p.q.to(DEV)
        self.bk = p.bk.to(DEV).contiguous()
        self.out = torch.full((Bp + 1, self.ldo), SENTINEL, device=DEV, dtype=torch.bfloat16)
        self.eps = float(p.eps)

    def args(self, **over):
        a = dict(tokens=self.tok.data_ptr(), n_part=self.B, N=self.N, H=self.H, planes=self.planes.data_ptr(),
                 plane_rows=self.plane_rows, eps=self.eps, G=self.G.data_ptr(), ldg=self.ldg, q=self.q.data_ptr(),
                 ldq=self.ldq, bk=self.bk.data_ptr(), scale=0.125, out=self.out.data_ptr(), ldo=self.ldo)
        assert set(over) <= set(a)
        a.update(over)
        return list(a.values()) + [E().stream_ptr()]

    def call(self, **over):
        return E().lib().vpf_cls_attn_fold_bf16(*self.args(**over))

    def result(self):
        """out [B][H][D] on the CPU, after checking that its pad columns and the spare row kept the sentinel."""
        torch.cuda.synchronize()
        full = self.out.cpu()
        HD_ = self.H * self.D
        assert bool((full[:, HD_:] == SENTINEL).all()) and bool((full[self.B] == SENTINEL).all()), \
            "the output's pad was written"
        return full[:self.B, :HD_].reshape(self.B, self.H, self.D).clone()


def _run(p):
    buf = Buffers(p)
    assert buf.call() == 0
    return buf.result()


def _fail(msgs, *ctx):
    assert not msgs, "\n".join([repr(ctx)] + msgs)


@pytest.mark.parametrize("N", probe.N_LIST)
@pytest.mark.parametrize("H", probe.HEADS)
def test_cls_fold_selection(H, N):
    """out[b][h] holds the bits of z[pi[b][h]] for every selection and statistics kind; with the bias c0 (the same for
    every token of a head) the output bits are the same."""
    for sel in probe.SELS:
        for stat in probe.STATS:
            p = probe.selection_probe(N, H, sel, stat)
            out = _run(p)
            _fail(probe.selection_errors(out, p), sel, stat)
            assert torch.equal(out, p.expected)
            pb = probe.selection_probe(N, H, sel, stat, True)
            outb = _run(pb)
            _fail(probe.selection_errors(outb, pb), sel, stat, "bias")
            assert torch.equal(outb.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("N", probe.N_LIST)
@pytest.mark.parametrize("H", probe.HEADS)
def test_cls_fold_census(H, N):
    """Every token ties: out[b][h][d] is one of the two bf16 neighbours of cnt / N, and 0 where cnt = 0."""
    for stat in probe.STATS:
        p = probe.census_probe(N, H, stat)
        _fail(probe.census_errors(_run(p), p), stat)


@pytest.mark.parametrize("N", probe.STAIR_N)
@pytest.mark.parametrize("H", probe.HEADS)
def test_cls_fold_staircase(H, N):
    """Fractional rescales at chunks that differ between the heads, spikes below the threshold in between: within
    2^-7 sum_t p_t |LNraw_t| of the fp64 reference (the counterpart of test_attention_bf16_rescale_branch)."""
    p = probe.staircase_probe(N, H)
    out = _run(p)
    print(f"staircase H={H} N={N}: max |out - U| / bar = {probe.staircase_ratio(out, p):.3f}")
    _fail(probe.staircase_errors(out, p))


# ---- the chain of vit.py around the kernel --------------------------------------------------------------------------

def _sigma(H):
    """[H][64] int64: the column of U_h that output dim d of head h picks, d H + (5 h + 1) % H: distinct per d, over
    all four quarters of D."""
    return torch.arange(64)[None, :] * H + ((5 * torch.arange(H) + 1) % H)[:, None]


@pytest.mark.parametrize("H,N", [(6, 197), (12, 197), (16, 197), (16, 577)])
def test_cls_fold_chain(H, N):
    """gemm(q, cls_g_weight(Wk), 0) -> cls_attn_fold_ -> gemm(U as (particle, head) rows, Wv, bv) into G's storage ->
    head_gather_, through the ops as ViTEngine chains them: Wk and q make G the selection probe's G, Wv picks one
    column of U per output dim, so x[p][64 h + d] = z[pi[p][h]][sigma(h, d)] + bv[64 h + d] bit for bit."""
    from vitparticlefiltertracker_amd.vit import cls_g_weight
    D = 64 * H
    p = probe.selection_probe(N, H, "spread", "varied")
    cols, sig = probe.score_cols(H), _sigma(H)
    Wk = torch.zeros(D, D)
    Wv = torch.zeros(D, D)
    for h in range(H):
        Wk[64 * h, cols[h]] = 64.0
        Wv[64 * h + torch.arange(64), sig[h]] = 1.0
    qall = torch.full((B, 2, D), float("nan"))
    qall[:, 0] = 0.0
    qall[:, 0, ::64] = 64.0
    q = qall.to(torch.bfloat16).to(DEV)[:, 0]                    # row stride 2 D, as the CLS rows of a token tensor
    bk = torch.zeros(D)
    bk[::64] = (torch.arange(H) % 3 + 1).float() / 32.0          # c0_h = 2, 4, 6
    bv = ((torch.arange(D) % 17) - 8).float()
    Wk, Wv, bk, bv = Wk.to(torch.bfloat16).to(DEV), Wv.to(torch.bfloat16).to(DEV), bk.to(DEV), bv.to(DEV)
    planes = torch.full((H, B * N + 3, 2), float("nan"), device=DEV)
    planes[:, :B * N] = p.planes.to(DEV)
    G = torch.empty(B, H * D, device=DEV, dtype=torch.bfloat16)
    U = torch.full((B, H * D), SENTINEL, device=DEV, dtype=torch.bfloat16)
    x = torch.full((B, 3 * D), SENTINEL, device=DEV, dtype=torch.bfloat16)
    w_g = cls_g_weight(Wk, H)
    vpf().gemm(q, w_g, torch.zeros(H * D, device=DEV), None, None, 0, None, None, 0, G)
    assert torch.equal(G.cpu().view(B, H, D), p.G), "G = gemm(q, cls_g_weight(Wk)) is not the probe's G"
    vpf().cls_attn_fold_(p.tok.to(DEV), planes, 0.0, G, q, bk, H, U)
    _fail(probe.selection_errors(U.cpu().view(B, H, D), p), "U")
    Y = G.view(B * H, D)                                         # G's storage: G is consumed by the fold
    vpf().gemm(U.view(B * H, D), Wv, bv, None, None, 0, None, None, 0, Y)
    vpf().head_gather_(Y, H, x[:, D:2 * D])
    expected = torch.stack([p.z[b, p.pi[b]].long().gather(1, sig) for b in range(B)]).float() + bv.cpu().view(1, H, 64)
    got = x.cpu()
    assert torch.equal(got[:, D:2 * D].float().view(B, H, 64), expected)
    assert bool((got[:, :D] == SENTINEL).all()) and bool((got[:, 2 * D:] == SENTINEL).all())


# ---- the argument contract, through the C ABI -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def contract():
    return Buffers(probe.census_probe(17, 6, "unit"))


def _rejected(buf, **over):
    assert buf.call(**over) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf.out == SENTINEL).all()), "a rejected call wrote the output"


def test_cls_fold_contract_ldg_too_small(contract):
    _rejected(contract, ldg=contract.H * contract.D - 8)


def test_cls_fold_contract_ldg_not_multiple_of_8(contract):
    _rejected(contract, ldg=contract.H * contract.D + 4)


def test_cls_fold_contract_ldo_too_small(contract):
    _rejected(contract, ldo=contract.H * contract.D - 4)


def test_cls_fold_contract_ldo_not_multiple_of_4(contract):
    _rejected(contract, ldo=contract.H * contract.D + 2)


def test_cls_fold_contract_ldq_too_small(contract):
    _rejected(contract, ldq=contract.D - 1)


def test_cls_fold_contract_tokens_or_g_misaligned(contract):
    """tokens and G are read in 16-byte pieces."""
    _rejected(contract, tokens=contract.tok.data_ptr() + 8)
    _rejected(contract, G=contract.G.data_ptr() + 8)
    _rejected(contract, G=contract.G.data_ptr() + 2)


def test_cls_fold_contract_planes_or_out_misaligned(contract):
    """planes are read, out is written, in 8-byte pieces."""
    _rejected(contract, planes=contract.planes.data_ptr() + 4)
    _rejected(contract, out=contract.out.data_ptr() + 4)
    _rejected(contract, out=contract.out.data_ptr() + 2)


def test_cls_fold_contract_eps_negative(contract):
    _rejected(contract, eps=-1e-6)


def test_cls_fold_contract_eps_nan(contract):
    _rejected(contract, eps=float("nan"))


def test_cls_fold_contract_no_tokens(contract):
    _rejected(contract, N=0)


def test_cls_fold_contract_no_particles(contract):
    """n_part = 0 is a valid empty call: it returns 0 and launches nothing."""
    assert contract.call(n_part=0) == 0
    torch.cuda.synchronize()
    assert bool((contract.out == SENTINEL).all())


def test_cls_fold_contract_accepts_the_layout():
    """The same buffers unchanged are accepted, and the census comes out: the rejections above are the arguments'."""
    fresh = Buffers(probe.census_probe(17, 6, "unit"))
    assert fresh.call() == 0
    _fail(probe.census_errors(fresh.result(), probe.census_probe(17, 6, "unit")))
