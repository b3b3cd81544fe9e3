"""GPU (MI355X): exact key / query routing and key census of every attention path, on the exactly computable inputs of
tests/test_oracle_attention.py (built and proven fair on the CPU there: why bit equality, one bf16 ulp and 2^-22 are
the right bars is that module's docstring).

Selection probe: out[b, i, h] must be the bits of V[b, pi(i), h]: a wrong key, query, dim, head or PV slot delivers
another row, and the message says which. Census probe: all keys tie and V counts residues, so out = cnt / N: a key
dropped at a chunk boundary, visited twice, a pad copy of key N - 1 let through the mask or a key summed into l but
not into O moves a count by one, and the message names the residue class.

B = H = 3 (9 units: not a multiple of 4, so the CLS kernel's last workgroup has waves past BH; not a multiple of 8, so
the key-streamed grid has padding workgroups; H is not a power of two). The key counts are the sizes at which the
kernels take another path:
  key-pipelined kernel (N <= 256): 8 | 9 the 8-key tail step, 16 | 17 and 40 | 41 the 16-query strip, 192 six chunks =
    one barrier group and no tail, 193 the tail chunk on a group boundary (its own wait and barrier), 197 the product
    shape, 201 a masked 16-query step, 209 a masked 32-query strip, 224 / 256 whole chunks;
  key-streamed kernel (N > 256): 257 one real key in the tail, 264 | 265 the 8-key tail step, 272 | 273 the 16-query
    strip, 330 an odd chunk count (the last group holds one chunk), 384 three full blocks, 400 the block the host adds
    for the 16-query strip, 545 / 577 / 640;
  q_rows = 1 (k_attn_cls_bf16): 63 | 64 | 65 the lane-to-key wrap, 640 its ceiling of 10 keys per lane;
  fp32: 128 | 129 the staging chunk, 577 three query passes;
  the MX8 output (N <= 256, D % 128 == 0: H = 4)."""
import pytest
import torch

import test_oracle_attention as probe   # the builders and the bars, proven on the CPU there

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H = 3, 3
SENTINEL = 5.0


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()


def vpf():
    return torch.ops.vpf


def ops():
    from vitparticlefiltertracker_amd import ops as o
    return o


def _run(qkv, heads, q_rows):
    """(out on the CPU, filled with the sentinel before the call)."""
    Bq, N, D3 = qkv.shape
    out = torch.full((Bq, N, D3 // 3), SENTINEL, device=DEV, dtype=qkv.dtype)
    vpf().attention(qkv.to(DEV), heads, q_rows, out)
    return out.cpu()


def _untouched(out, rows):
    assert bool((out[:, rows:] == SENTINEL).all()), f"rows >= {rows} were written"


def _fail(msgs):
    assert not msgs, "\n".join(msgs)


def _selection(N, kind, dtype, q_rows=None):
    qkv, expected, pi = probe.selection_probe(N, B, H, kind, 0, dtype)
    rows = N if q_rows is None else q_rows
    out = _run(qkv, H, rows)
    _fail(probe.selection_errors(out, qkv, expected, pi, rows))
    assert torch.equal(out[:, :rows], expected[:, :rows])
    _untouched(out, rows)
    return out


def _census(N, dtype, q_rows=None):
    qkv, cnt = probe.census_probe(N, B, H, dtype)
    rows = N if q_rows is None else q_rows
    out = _run(qkv, H, rows)
    _fail(probe.census_errors(out, cnt, N, rows))
    _untouched(out, rows)
    return out


@pytest.mark.parametrize("kind", probe.PERMS)
@pytest.mark.parametrize("N", probe.PIPE_N + probe.STREAM_N)
def test_attention_bf16_selection(N, kind):
    """vpf_attention_bf16, every query row: the key-pipelined kernel up to N = 256, the key-streamed one above."""
    _selection(N, kind, torch.bfloat16)


@pytest.mark.parametrize("N", probe.PIPE_N + probe.STREAM_N)
def test_attention_bf16_census(N):
    _census(N, torch.bfloat16)


@pytest.mark.parametrize("kind", probe.PERMS)
@pytest.mark.parametrize("N", probe.CLS_N)
def test_attention_cls_selection(N, kind):
    """q_rows = 1 (k_attn_cls_bf16): row 0 is V[pi(0)], the other rows keep the sentinel."""
    _selection(N, kind, torch.bfloat16, q_rows=1)


@pytest.mark.parametrize("N", probe.CLS_N)
def test_attention_cls_census(N):
    _census(N, torch.bfloat16, q_rows=1)


@pytest.mark.parametrize("kind", probe.PERMS)
@pytest.mark.parametrize("N", probe.F32_N)
def test_attention_f32_selection(N, kind):
    """vpf_attention_f32: p = expf(0) = 1 for the selected key and expf(<= -138) = 0 for the others, V / 1: fp32 bits."""
    _selection(N, kind, torch.float32)


@pytest.mark.parametrize("N", probe.F32_N)
def test_attention_f32_census(N):
    _census(N, torch.float32)


# ---- the MX8 output -------------------------------------------------------------------------------------------------

H8 = 4   # D = 256: two scale planes (the op needs D % 128 == 0, which H = 3 is not)


def _ref_quant(x):
    """The CPU oracle's MX8 rule (oracle/mx8.py, pinned by tests/test_oracle_mx8.py) on bf16 rows."""
    import numpy as np
    from oracle import mx8 as omx8
    codes, sc = omx8.quantize(x.contiguous().cpu().view(torch.int16).numpy().view(np.uint16))
    return torch.from_numpy(codes), torch.from_numpy(sc.astype(np.int32))


def _attention_q8(qkv):
    Bq, N, D3 = qkv.shape
    q, s = ops().mx8_empty(Bq * N, D3 // 3, DEV)
    vpf().attention_q8_(qkv.to(DEV), H8, q, s)
    return q, s


@pytest.mark.parametrize("kind", probe.PERMS)
@pytest.mark.parametrize("N", probe.Q8_N)
def test_attention_q8_selection(N, kind):
    """attention_q8_ (k_attn_bf16_pipe<OUT8>: 32-query strips only, the quantiser in the store): codes and scale bytes
    equal the CPU oracle quantiser applied to the expected rows V[b, pi(i), h], laid out per token [B N][64 H]."""
    qkv, expected, pi = probe.selection_probe(N, B, H8, kind)
    q, s = _attention_q8(qkv)
    rq, rs = _ref_quant(expected.view(B * N, 64 * H8))
    sb = ops().mx8_scale_bytes(s, B * N).cpu()
    bad = (q.cpu() != rq).view(B, N, H8, 64).any(-1) | (sb != rs).view(B, N, H8, 2).any(-1)
    if bool(bad.any()):   # say whether the bf16 instance of the kernel delivers the right rows at this shape
        out = _run(qkv, H8, N)
        _fail([f"MX8 output: {int(bad.sum())} (b, i, h) rows differ from quantize(V[pi(i)]), first (b, i, h) = "
               f"{bad.nonzero()[0].tolist()}; the bf16 output of the same shape:"]
              + (probe.selection_errors(out, qkv, expected, pi) or ["  is exact"]))
    assert torch.equal(q.cpu(), rq) and torch.equal(sb, rs)


@pytest.mark.parametrize("N", probe.Q8_N)
def test_attention_q8_census(N):
    """The census on the MX8 output: the bf16 output of the same shape meets the census bar, and the MX8 output is the
    quantiser (the kernel's own, bit-exact against the oracle in tests/test_gpu_mx8.py) of those bf16 rows."""
    qkv, cnt = probe.census_probe(N, B, H8)
    out = torch.empty(B, N, 64 * H8, device=DEV, dtype=torch.bfloat16)
    vpf().attention(qkv.to(DEV), H8, N, out)
    _fail(probe.census_errors(out, cnt, N))
    q, s = _attention_q8(qkv)
    rq, rs = ops().mx8_empty(B * N, 64 * H8, DEV)
    vpf().quantize_mx8_(out.view(B * N, 64 * H8), 1, rq, rs)
    assert torch.equal(q, rq), f"{int((q != rq).sum())} element codes differ"
    assert torch.equal(ops().mx8_scale_bytes(s, B * N), ops().mx8_scale_bytes(rs, B * N))
    cq, cs = _ref_quant(out.view(B * N, 64 * H8))
    assert torch.equal(q.cpu(), cq) and torch.equal(ops().mx8_scale_bytes(s, B * N).cpu(), cs)


# ---- partial q_rows -------------------------------------------------------------------------------------------------

def _partial_rows(N):
    """32 floor(N / 32) | + 1: where the host stops / starts scheduling the 16-query strip (and, at N = 400, the block
    added for it); 128 | 129: one query block of the key-streamed kernel, four strips of the key-pipelined one."""
    return [32 * (N // 32), 32 * (N // 32) + 1, 128, 129]


@pytest.mark.parametrize("N", [197, 400, 577])
def test_attention_bf16_partial_q_rows(N):
    """q_rows < N on both probes (the selection probe with every permutation kind): rows < q_rows hold the bits of the
    full call's rows (and meet the probe's bar themselves), the rest keep the sentinel."""
    for kind in probe.PERMS:
        full = _selection(N, kind, torch.bfloat16)
        for rows in _partial_rows(N):
            part = _selection(N, kind, torch.bfloat16, q_rows=rows)
            assert torch.equal(part[:, :rows], full[:, :rows]), (kind, rows)
    full = _census(N, torch.bfloat16)
    for rows in _partial_rows(N):
        part = _census(N, torch.bfloat16, q_rows=rows)
        assert torch.equal(part[:, :rows], full[:, :rows]), rows
