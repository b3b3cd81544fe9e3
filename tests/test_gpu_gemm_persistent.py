"""The tile-walking bf16 GEMM kernel (k_gemm_walk, csrc/gemm_bf16.hip) against the two one-tile-per-workgroup kernels.

GPU (MI355X): on seeded operands the walking kernel's output bits equal kernel 5's (k_gemm_pp) and kernel 1's
(k_gemm_bf16), for the direct-store epilogues (EPI_LN_GELU with {mean, rstd} row statistics, EPI_BIAS_GELU: FC1) and
for EPI_LN (QKV), whose pipelined image epilogue there runs on one reused 16-row group image per wave. The
vpf_gemm_persistent hook forces the kernel and caps its grid, so that a handful of tiles is walked by 8 or 16
workgroups and every seam path runs; vpf_gemm_persistent_grid says which kernel a call takes, so a case cannot pass by
silently running the old kernels. Every output is a view (row stride N + 24, 3 spare rows) of a buffer of sentinel
bytes that must survive outside the view.

Shapes (256 x 256 tiles, K-tiles of 64, nk = K / 64; workgroup b of a grid of G walks ids first(b & 7) + (b >> 3) +
j G / 8 of its XCD's range, the 8 ranges splitting the tile count as evenly as possible):
  M = 3*256 + 40, N = 2*256 + 64  12 tiles (clamped edge rows and columns: a 40-row and a 64-column edge tile). Cap 8:
                                  4 workgroups walk 2 tiles (one seam), 4 walk one (last-tile path only): the tile count
                                  is not a multiple of the grid. Cap 16: the grid shrinks to 8 too (12 & ~7), the same
                                  launch again (kept: the case is named in the kernel's specification).
  M = 4*256 + 40, N = 3*256 + 64  20 tiles, cap 16, grid 16: the XCD ranges of 3 / 2 tiles are split 2 + 1 / 1 + 1.
  M = 11*256 + 40, same N         36 tiles. Cap 8: 4 workgroups walk 5 tiles, 4 walk 4 (several seams each). Cap 16: the
                                  XCD ranges of 5 / 4 tiles are split 3 + 2 / 2 + 2.
  M = 4*256, N = 2*256            8 tiles on a grid of 8: no seam, every workgroup on the last-tile path from the start.
K = 128 (nk = 2: the two tail K-steps are the whole loop, the seam is taken in the first K-step and the aux sets
alternate every tile) and K = 768 (the encoder's). Forced mode on K = 192 (nk odd) and on stats_parts > 0 must keep the
old kernels and still match; so must the hook turned off.

Host (no GPU): the compiled kernel has no scratch and at most 256 VGPRs."""
import contextlib
import functools
import os
import re

import pytest
import torch

DEV = "cuda"
SENT = 0xAB
SENT16 = 0xABAB - 0x10000   # two sentinel bytes read as int16
BIAS, BIAS_GELU, LN, LN_GELU = 0, 1, 4, 5
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _ops():
    from vitparticlefiltertracker_amd import _lib, ops
    return _lib, ops


_ROUTING = [(0, 0, 0)]   # (kernel, mode, cap) of the enclosing routed() blocks; the bottom entry is the library's default


def _apply(kernel, mode, cap):
    L = _ops()[0].lib()
    assert L.vpf_gemm_tune(kernel, -1) == 0 and L.vpf_gemm_persistent(mode, cap) == 0


@contextlib.contextmanager
def routed(kernel=0, mode=0, cap=0):
    """vpf_gemm_tune(kernel) and vpf_gemm_persistent(mode, cap) for the block. Blocks nest: leaving one puts back the
    state of the block around it (the library's defaults outside every block), whatever happened inside."""
    _ROUTING.append((kernel, mode, cap))
    try:
        _apply(kernel, mode, cap)
        yield
        torch.cuda.synchronize()
    finally:
        _ROUTING.pop()
        _apply(*_ROUTING[-1])


@functools.lru_cache(maxsize=None)
def problem(M, N, K, parts=0):
    """Seeded operands on the device (shared by every test of the shape, never written)."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    a = (torch.rand(M, K, generator=g) * 2 - 1).to(torch.bfloat16)
    w = ((torch.rand(N, K, generator=g) * 2 - 1) * 0.05).to(torch.bfloat16)
    bias = torch.rand(N, generator=g) * 0.1
    colsum = w.float().sum(1)
    if parts:   # {sum, sumsq} planes of a's 64-column blocks
        af = a.float().view(M, parts, K // parts)
        stats = torch.stack([af.sum(2), (af * af).sum(2)], 2).transpose(0, 1).contiguous()
    else:       # {mean, rstd} rows
        stats = torch.stack([torch.rand(M, generator=g) * 0.2 - 0.1, torch.rand(M, generator=g) + 0.5], 1)
    return tuple(t.contiguous().to(DEV) for t in (a, w, bias, colsum, stats))


def run(M, N, K, epi, parts=0):
    """One vpf.gemm into a sentinel-framed output; returns the [M][N] bits after checking the frame."""
    _, ops = _ops()
    a, w, bias, colsum, stats = problem(M, N, K, parts)
    ld = N + 24
    buf = torch.full(((M + 3) * ld * 2,), SENT, dtype=torch.uint8, device=DEV)
    frame = buf.view(torch.bfloat16).view(M + 3, ld)
    out = frame[:M, :N]
    ln = epi in (LN, LN_GELU)
    ops.gemm(a, w, bias, None, None, 0, stats if ln else None, colsum if ln else None, epi, out, parts, 1e-6)
    torch.cuda.synchronize()
    bits = frame.view(torch.int16)
    assert bool((bits[:M, N:] == SENT16).all()) and bool((bits[M:] == SENT16).all()), "written outside the output view"
    return bits[:M, :N].clone()


@functools.lru_cache(maxsize=None)
def reference(M, N, K, epi, parts=0):
    """Kernel 5's and kernel 1's bits (equal: the existing suite's contract), computed once per case."""
    with routed(kernel=5):
        r5 = run(M, N, K, epi, parts)
    with routed(kernel=1):
        r1 = run(M, N, K, epi, parts)
    assert torch.equal(r5, r1), "kernels 5 and 1 differ"
    assert int((r5 == SENT16).sum()) < r5.numel() // 100, "the output was not written"
    return r5


EPIS, EPI_IDS = [LN_GELU, BIAS_GELU, LN], ["LN_GELU", "BIAS_GELU", "LN"]
EDGE = (3 * 256 + 40, 2 * 256 + 64)
TWENTY = (4 * 256 + 40, 3 * 256 + 64)
LONG = (11 * 256 + 40, 2 * 256 + 64)
EVEN = (4 * 256, 2 * 256)


@pytest.mark.gpu
@pytest.mark.parametrize("epi", EPIS, ids=EPI_IDS)
@pytest.mark.parametrize("K", [128, 768])
@pytest.mark.parametrize("mn,cap,grid", [(EDGE, 8, 8), (EDGE, 16, 8), (TWENTY, 16, 16), (LONG, 8, 8), (LONG, 16, 16),
                                         (EVEN, 8, 8)],
                         ids=["12tiles_cap8", "12tiles_cap16", "20tiles_cap16", "36tiles_cap8", "36tiles_cap16",
                              "8tiles_cap8"])
def test_walking_kernel_matches_kernels_5_and_1(mn, cap, grid, K, epi):
    _, ops = _ops()
    M, N = mn
    ref = reference(M, N, K, epi)
    with routed(mode=1, cap=cap):
        assert ops.gemm_persistent_grid(M, N, K, epi) == grid
        got = run(M, N, K, epi)
    bad = got != ref
    assert not bool(bad.any()), f"{int(bad.sum())} elements differ; first at {bad.nonzero()[0].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("epi", EPIS, ids=EPI_IDS)
def test_forced_mode_keeps_the_old_kernels_where_the_walk_cannot_run(epi):
    """nk odd (K = 192), in-kernel statistics planes (stats_parts > 0), a kernel forced by vpf_gemm_tune, the hook off,
    an epilogue the kernel does not have: grid 0, and the bits of kernels 5 and 1."""
    E, ops = _ops()
    M, N = LONG
    ln = epi != BIAS_GELU
    ref192, ref768 = reference(M, N, 192, epi), reference(M, N, 768, epi)
    ref_planes = reference(M, N, 768, epi, 12) if ln else None

    def forced():   # the hook is in forced mode right now: the walk takes the shape it can run, on the capped grid
        return ops.gemm_persistent_grid(M, N, 768, epi) == 8

    with routed(mode=1, cap=8):
        assert forced()
        assert ops.gemm_persistent_grid(M, N, 192, epi) == 0
        assert torch.equal(run(M, N, 192, epi), ref192)
        assert ops.gemm_persistent_grid(M, N, 768, BIAS) == 0
        if ln:
            assert ops.gemm_persistent_grid(M, N, 768, epi, 12) == 0
            assert torch.equal(run(M, N, 768, epi, 12), ref_planes)
        assert forced()   # still forced after the runs above
        with routed(kernel=5, mode=1, cap=8):
            assert ops.gemm_persistent_grid(M, N, 768, epi) == 0
        assert forced()   # a nested block puts the forced state back
    with routed(mode=-1, cap=8):
        assert ops.gemm_persistent_grid(M, N, 768, epi) == 0
        assert torch.equal(run(M, N, 768, epi), ref768)
    L = E.lib()
    for mode, cap in ((2, 0), (-2, 0), (1, 12), (0, -8)):
        assert L.vpf_gemm_persistent(mode, cap) == -1
    with routed(mode=1, cap=8):   # a refused call changed nothing
        assert forced()


@pytest.mark.gpu
@pytest.mark.parametrize("epi", EPIS, ids=EPI_IDS)
def test_default_routing_needs_two_tiles_per_workgroup(epi):
    """The per-shape default: EPI_LN_GELU and EPI_LN (each measured against the parent's kernel) on a grid of one
    workgroup per CU (a multiple of 8), only from two tiles per workgroup on; below that, and for EPI_BIAS_GELU (not
    measured against its default, kernel 1), the call keeps the old kernels. The default's bits equal the references."""
    _, ops = _ops()
    M, N = LONG
    ref = reference(M, N, 768, epi)
    with routed(mode=1):
        cus = ops.gemm_persistent_grid(1 << 20, 4096, 768, epi)   # 65536 tiles: the uncapped grid
    assert cus >= 8 and cus % 8 == 0
    with routed():
        big = ops.gemm_persistent_grid(2 * cus * 256, 256, 768, epi)
        assert big == (0 if epi == BIAS_GELU else cus)
        assert ops.gemm_persistent_grid((2 * cus - 1) * 256, 256, 768, epi) == 0
        assert ops.gemm_persistent_grid(M, N, 768, epi) == 0   # 36 tiles on the uncapped grid
        assert torch.equal(run(M, N, 768, epi), ref)
    with routed(cap=8):   # the default rule with a capped grid: 36 tiles >= 2 x 8
        assert ops.gemm_persistent_grid(M, N, 768, epi) == (0 if epi == BIAS_GELU else 8)
        assert torch.equal(run(M, N, 768, epi), ref)


def test_walking_kernel_compiles_without_scratch(tmp_path):
    """One workgroup per CU at 512 threads leaves a lane 256 VGPRs; a spill would put scratch traffic's vmcnt waits
    between the LDS-DMA pieces and their counted waits. Checked on the compiled gfx950 code of the three instances."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "vitparticlefiltertracker_amd", "csrc", "gemm_bf16.hip")
    out = tmp_path / "gemm_bf16.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "--cuda-device-only",
                    "-S", "-o", str(out), src], check=True, capture_output=True)
    text = out.read_text()
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        name, desc = m.group(1), m.group(2)
        if not re.search(r"\dk_gemm_walkI", name):
            continue
        seen += 1
        field = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", desc)}
        assert field["private_segment_fixed_size"] == 0, (name, "scratch")
        assert field["next_free_vgpr"] <= 256, (name, field["next_free_vgpr"])
        assert field["group_segment_fixed_size"] <= 160 * 1024, (name, field["group_segment_fixed_size"])
        body = re.search(r"^" + re.escape(name) + r":(.*?)\.Lfunc_end", text, re.S | re.M).group(1)
        assert "scratch_" not in body, name
    assert seen == 3, seen
