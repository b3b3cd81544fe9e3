"""Which K-tile's A fragments every output quadrant of the tile-walking bf16 GEMMs consumed (k_gemm_walk<EPI_LN>,
<EPI_LN_GELU>, <EPI_BIAS_GELU> and k_gemm_walk_res; csrc/gemm_bf16.hip), in exact arithmetic.

The instances that carry the 4 / 4 / 8 / 8 read order take the A0 fragments of K-tile kt + 1 from the other ring
buffer in q3 of K-tile kt, one phase after the wait that retires that half-tile, and take a tile's first A0 fragments
at the tile's top. A fragment read from the slot too early holds the half-tile staged there before (K-tile kt - 1 of the
same panel, or the previous tile's panel across a seam); a fragment carried wrongly across the tile's end holds another
K-tile's. Both show as a specific wrong integer here:

  A[m][k]   = 16 + 5 (2 kt + half) + panel % 5     kt = k // 64, half = (m % 128) // 64 (the A0 / A1 half-tile of the
                                                   row), panel = m // 256; constant over a K-tile's 64 columns
  W[n][k]   = 1 at the one column k = 64 t(n) + c(n), t(n) = n % nk, c(n) = (7 (n // nk) + n) % 64; else 0
  out[m][n] = A[m][64 t(n) + c(n)]: the code of (K-tile t(n), half, panel) as the MFMAs of that K-tile saw it.

Every column tile holds every t(n) in both of a wave's column halves, so each (quadrant, K-tile) pair is named by many
outputs. All values are integers of at most 8 bits: exact in bf16, in the fp32 accumulators and in the bf16 output.
Epilogues: bias 0; LN with {mean, rstd} = {0, 1} (the fold is fma(1, acc, fma(-0, colsum, 0)) = acc); residual 0 in
place; GELU of an integer x >= 16 is x itself in gelu_sig2 (x * rcp(1 + exp2(x (c2 x^2 + c1))): the exponent is below
-500, exp2 gives 0, rcp(1) = 1). So the expected output is an integer gather computed on the CPU, compared for
equality.

Forced walk (vpf_gemm_persistent(1, 8), asserted by gemm_persistent_grid): 12 tiles on 8 workgroups (one- and two-tile
walks, the 40-row edge panel and the 64-column edge tile), 36 tiles on 8 (walks of four and five tiles), 8 tiles on 8
(no seam). K = 128 (nk = 2: the first early read's fragments are used in the tile's last K-tile), 256 and 768."""
import contextlib
import functools

import numpy as np
import pytest
import torch

DEV = "cuda"
SENT = 0xAB
SENT16 = 0xABAB - 0x10000
BIAS_GELU, RES, LN, LN_GELU = 1, 2, 4, 5
EDGE = (3 * 256 + 40, 2 * 256 + 64)
LONG = (11 * 256 + 40, 2 * 256 + 64)
EVEN = (4 * 256, 2 * 256)


def _ops():
    from vitparticlefiltertracker_amd import _lib, ops
    return _lib, ops


@contextlib.contextmanager
def forced_walk(cap):
    L = _ops()[0].lib()
    assert L.vpf_gemm_tune(0, -1) == 0 and L.vpf_gemm_persistent(1, cap) == 0
    try:
        yield
        torch.cuda.synchronize()
    finally:
        assert L.vpf_gemm_persistent(0, 0) == 0


def code(kt, half, panel):
    return 16 + 5 * (2 * kt + half) + panel % 5


def name_of(v):
    """(K-tile, half, panel % 5) a value stands for, or None"""
    v = int(v) - 16
    return (v // 10, v // 5 % 2, v % 5) if 0 <= v < 10 * 12 else None


@functools.lru_cache(maxsize=None)
def problem(M, N, K):
    """Integer operands and the expected output (CPU, integers); the device copies are never written."""
    nk = K // 64
    m, k, n = np.arange(M)[:, None], np.arange(K)[None, :], np.arange(N)
    a = code(k // 64, m % 128 // 64, m // 256).astype(np.int64)                # [M][K]
    hot = 64 * (n % nk) + (7 * (n // nk) + n) % 64                               # [N]
    w = np.zeros((N, K), np.int64)
    w[n, hot] = 1
    want = a[:, hot]                                                             # = a @ w.T for a one-hot w
    assert want.min() >= 16 and want.max() < 256
    at, wt = (torch.from_numpy(x).to(torch.bfloat16) for x in (a, w))
    assert torch.equal(at.to(torch.int64), torch.from_numpy(a))                  # exact in bf16
    stats = torch.tensor([0.0, 1.0]).repeat(M, 1)
    dev = tuple(t.contiguous().to(DEV) for t in (at, wt, torch.zeros(N), wt.float().sum(1), stats))
    return dev, want


def run(M, N, K, epi):
    _, ops = _ops()
    (a, w, bias, colsum, stats), want = problem(M, N, K)
    ld = N + 24
    buf = torch.full(((M + 3) * ld * 2,), SENT, dtype=torch.uint8, device=DEV)
    frame = buf.view(torch.bfloat16).view(M + 3, ld)
    out = frame[:M, :N]
    if epi == RES:
        out.zero_()
        ops.gemm(a, w, bias, out, None, 0, None, None, RES, out)
    else:
        ln = epi in (LN, LN_GELU)
        ops.gemm(a, w, bias, None, None, 0, stats if ln else None, colsum if ln else None, epi, out, 0, 1e-6)
    torch.cuda.synchronize()
    bits = frame.view(torch.int16)
    assert bool((bits[:M, N:] == SENT16).all()) and bool((bits[M:] == SENT16).all()), "written outside the output view"
    return out.float().cpu().numpy(), want


@pytest.mark.gpu
@pytest.mark.parametrize("epi", [LN_GELU, BIAS_GELU, LN, RES], ids=["LN_GELU", "BIAS_GELU", "LN", "RESIDUAL"])
@pytest.mark.parametrize("K", [128, 256, 768])
@pytest.mark.parametrize("mn", [EDGE, LONG, EVEN], ids=["12tiles", "36tiles", "8tiles"])
def test_every_quadrant_consumes_its_own_k_tile(mn, K, epi):
    _, ops = _ops()
    M, N = mn
    with forced_walk(8):
        assert ops.gemm_persistent_grid(M, N, K, epi) == 8
        got, want = run(M, N, K, epi)
    bad = got != want
    if bad.any():
        i, j = (int(x[0]) for x in np.nonzero(bad))
        nk = K // 64
        pytest.fail(f"{int(bad.sum())} of {bad.size} outputs differ; first at row {i} (tile row {i % 256}, panel "
                    f"{i // 256}), column {j} (tile column {j % 256}, K-tile {j % nk}): got {got[i, j]} = (K-tile, half, "
                    f"panel % 5) {name_of(got[i, j])}, expected {want[i, j]} = {name_of(want[i, j])}; wrong rows of "
                    f"the first wrong column: {np.nonzero(bad[:, j])[0][:8].tolist()}")
