"""The tile-walking residual GEMM kernel (k_gemm_walk_res, csrc/gemm_bf16.hip: proj / FC2, EPI_BIAS_RESIDUAL with the
statistics planes) against the two one-tile-per-workgroup kernels.

GPU (MI355X): on seeded operands the walking kernel's output bits and plane bits equal kernel 5's (k_gemm_pp) and
kernel 1's (k_gemm_bf16), which must agree with each other first. The vpf_gemm_persistent hook forces the kernel and
caps its grid, so that a handful of tiles is walked by 8 or 16 workgroups and every seam path runs;
vpf_gemm_persistent_grid says which kernel a call takes, so a case cannot pass by running the old kernels.

Shapes and caps are test_gpu_gemm_persistent.py's (12 tiles on 8, 20 on 16, 36 on 8 and on 16, 8 on 8: no seam; a
40-row edge panel and a 64-column edge tile), K = 128 (nk = 2: the seam in the first K-step, the aux sets alternating
every tile), K = 768 (proj's nk = 12) and, on the 36-tile shape, K = 3072 (FC2's nk = 48).

Residual in place (the residual is the output view, as the engine calls it) and in a separate tensor of the same row
stride; with the planes and without (stats_out None). The output is a view (row stride N + 24, 3 spare rows) of
sentinel bytes that must survive outside it; the planes are the head of a sentinel-filled allocation whose tail must
survive. With N = 576 all 9 planes are written for all M rows (no sentinel word is left in them: the references are
checked for that, and the walk's planes equal the references bit for bit).

Operands: rand * 2 - 1 activations and residual, weights scaled by 0.05, so no partial sum of a plane cancels to zero
and the plane comparison is a comparison of real bits.

Not routed (grid 0 and the reference's bits): K = 192 (nk odd), a kernel forced by vpf_gemm_tune, mode -1; a call with
the fp8 copy (gemm_q8_) keeps the deep ring whatever the hook says and matches kernel 1's bits, the fp8 bytes included.

Host (no GPU): the compiled kernel, found by its own name, has no scratch, at most 256 VGPRs and at most 160 KiB of
LDS."""
import contextlib
import functools
import os
import re

import pytest
import torch

DEV = "cuda"
SENT = 0xAB
SENT16 = 0xABAB - 0x10000            # two sentinel bytes read as int16
SENT32 = 0xABABABAB - (1 << 32)      # four read as int32
TAIL = 64                            # sentinel floats behind the last plane
BIAS, RES, LN = 0, 2, 4
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# The per-shape default that ships: K-tile count -> routed to the walk by default.
# proj's and FC2's counts each passed their A/B against the deep ring; no other count was measured.
DEFAULT_ROUTED = {12: True, 16: False, 48: True}


def _ops():
    from vitparticlefiltertracker_amd import _lib, ops
    return _lib, ops


_ROUTING = [(0, 0, 0)]   # (kernel, mode, cap) of the enclosing routed() blocks; the bottom entry is the library's default


def _apply(kernel, mode, cap):
    L = _ops()[0].lib()
    assert L.vpf_gemm_tune(kernel, -1) == 0 and L.vpf_gemm_persistent(mode, cap) == 0


@contextlib.contextmanager
def routed(kernel=0, mode=0, cap=0):
    """vpf_gemm_tune(kernel) and vpf_gemm_persistent(mode, cap) for the block; leaving it puts back the state of the
    block around it (the library's defaults outside every block), whatever happened inside."""
    _ROUTING.append((kernel, mode, cap))
    try:
        _apply(kernel, mode, cap)
        yield
        torch.cuda.synchronize()
    finally:
        _ROUTING.pop()
        _apply(*_ROUTING[-1])


@functools.lru_cache(maxsize=None)
def problem(M, N, K):
    """Seeded operands on the device (shared by every test of the shape, never written)."""
    g = torch.Generator().manual_seed(7 + 1000 * M + 10 * N + K)
    a = (torch.rand(M, K, generator=g) * 2 - 1).to(torch.bfloat16)
    w = ((torch.rand(N, K, generator=g) * 2 - 1) * 0.05).to(torch.bfloat16)
    bias = torch.rand(N, generator=g) * 0.1
    res = (torch.rand(M, N, generator=g) * 2 - 1).to(torch.bfloat16)
    return tuple(t.contiguous().to(DEV) for t in (a, w, bias, res))


def framed(M, N):
    """An [M][N] bf16 view (row stride N + 24, 3 spare rows) of sentinel bytes, and the whole frame."""
    ld = N + 24
    buf = torch.full(((M + 3) * ld * 2,), SENT, dtype=torch.uint8, device=DEV)
    frame = buf.view(torch.bfloat16).view(M + 3, ld)
    return frame[:M, :N], frame


def run(M, N, K, inplace=True, planes=True, fp8=False):
    """One residual GEMM into a sentinel-framed output. Returns (output bits [M][N], plane bits [P][M][2] or None, and
    with fp8 the MX8 copy's two tensors) after checking everything around them."""
    _, ops = _ops()
    a, w, bias, res = problem(M, N, K)
    out, frame = framed(M, N)
    if inplace:
        out.copy_(res)
        resid = out
    else:
        resid, rframe = framed(M, N)
        resid.copy_(res)
        rbits = rframe.view(torch.int16).clone()
    P = (N + 63) // 64
    sbuf = torch.full(((P * M * 2 + TAIL) * 4,), SENT, dtype=torch.uint8, device=DEV).view(torch.float32)
    so = sbuf[:P * M * 2] if planes or fp8 else None
    extra = ()
    if fp8:
        q8, s8 = ops.mx8_empty(M, N, DEV)
        q8.zero_()
        s8.zero_()
        ops.gemm_q8_(a, w, bias, resid, None, 0, RES, out, so, q8, s8)
        extra = (q8, s8)
    elif planes:
        ops.gemm_stats_(a, w, bias, resid, None, 0, RES, out, so)
    else:
        ops.gemm(a, w, bias, resid, None, 0, None, None, RES, out)
    torch.cuda.synchronize()
    bits = frame.view(torch.int16)
    assert bool((bits[:M, N:] == SENT16).all()) and bool((bits[M:] == SENT16).all()), "written outside the output view"
    if not inplace:
        assert torch.equal(rframe.view(torch.int16), rbits), "the separate residual was written"
    sbits = sbuf.view(torch.int32)
    assert bool((sbits[P * M * 2:] == SENT32).all()), "written behind the last plane"
    if so is None:
        assert bool((sbits == SENT32).all()), "planes written without stats_out"
    return (bits[:M, :N].clone(), sbits[:P * M * 2].view(P, M, 2).clone() if so is not None else None) + extra


@functools.lru_cache(maxsize=None)
def reference(M, N, K):
    """Kernel 5's and kernel 1's output and plane bits (which must agree), in place with planes, once per shape."""
    with routed(kernel=5):
        o5, p5 = run(M, N, K)
    with routed(kernel=1):
        o1, p1 = run(M, N, K)
    assert torch.equal(o5, o1) and torch.equal(p5, p1), "kernels 5 and 1 differ"
    assert int((o5 == SENT16).sum()) < o5.numel() // 100, "the output was not written"
    assert not bool((p5 == SENT32).any()), "a plane word was not written"
    return o5, p5


EDGE = (3 * 256 + 40, 2 * 256 + 64)
TWENTY = (4 * 256 + 40, 3 * 256 + 64)
LONG = (11 * 256 + 40, 2 * 256 + 64)
EVEN = (4 * 256, 2 * 256)
SHAPES = [(EDGE, 8, 8), (EDGE, 16, 8), (TWENTY, 16, 16), (LONG, 8, 8), (LONG, 16, 16), (EVEN, 8, 8)]
SHAPE_IDS = ["12tiles_cap8", "12tiles_cap16", "20tiles_cap16", "36tiles_cap8", "36tiles_cap16", "8tiles_cap8"]
CASES = [pytest.param(mn, cap, grid, K, id=f"{sid}-K{K}") for (mn, cap, grid), sid in zip(SHAPES, SHAPE_IDS)
         for K in (128, 768)]
CASES += [pytest.param(LONG, cap, cap, 3072, id=f"36tiles_cap{cap}-K3072") for cap in (8, 16)]


def check(got, ref, planes):
    o, p = got
    ro, rp = ref
    bad = o != ro
    assert not bool(bad.any()), f"{int(bad.sum())} output elements differ; first at {bad.nonzero()[0].tolist()}"
    if planes:
        bad = p != rp
        assert not bool(bad.any()), f"{int(bad.sum())} plane words differ; first at {bad.nonzero()[0].tolist()}"
    else:
        assert p is None


@pytest.mark.gpu
@pytest.mark.parametrize("planes", [True, False], ids=["planes", "noplanes"])
@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "separate"])
@pytest.mark.parametrize("mn,cap,grid,K", CASES)
def test_walking_residual_kernel_matches_kernels_5_and_1(mn, cap, grid, K, inplace, planes):
    _, ops = _ops()
    M, N = mn
    ref = reference(M, N, K)
    with routed(mode=1, cap=cap):
        assert ops.gemm_persistent_grid(M, N, K, RES) == grid
        got = run(M, N, K, inplace, planes)
    check(got, ref, planes)


@pytest.mark.gpu
def test_forced_mode_keeps_the_old_kernels_where_the_walk_cannot_run():
    """nk odd (K = 192), a kernel forced by vpf_gemm_tune, the hook off: grid 0, and the bits of kernels 5 and 1.
    EPI_BIAS still reports 0."""
    _, ops = _ops()
    M, N = LONG
    ref192, ref768 = reference(M, N, 192), reference(M, N, 768)
    with routed(mode=1, cap=8):
        assert ops.gemm_persistent_grid(M, N, 768, RES) == 8
        assert ops.gemm_persistent_grid(M, N, 192, RES) == 0
        check(run(M, N, 192), ref192, True)
        assert ops.gemm_persistent_grid(M, N, 768, BIAS) == 0
        for kernel in (1, 5):
            with routed(kernel=kernel, mode=1, cap=8):
                assert ops.gemm_persistent_grid(M, N, 768, RES) == 0
                check(run(M, N, 768), ref768, True)
        assert ops.gemm_persistent_grid(M, N, 768, RES) == 8   # a nested block puts the forced state back
    with routed(mode=-1, cap=8):
        assert ops.gemm_persistent_grid(M, N, 768, RES) == 0
        check(run(M, N, 768), ref768, True)


@pytest.mark.gpu
def test_a_call_with_the_fp8_copy_keeps_the_deep_ring():
    """gemm_q8_ (bf16 output, planes and the MX8 copy) in forced mode: the walk has no fp8 copy, so the call runs the
    deep-ring kernel; its four outputs equal kernel 1's and its bf16 output and planes equal the references."""
    M, N = EVEN   # the MX8 copy needs N % 128 == 0
    ref = reference(M, N, 768)
    with routed(kernel=1):
        want = run(M, N, 768, fp8=True)
    with routed(mode=1, cap=8):
        assert _ops()[1].gemm_persistent_grid(M, N, 768, RES) == 8   # the same shape without the copy would walk
        got = run(M, N, 768, fp8=True)
    check(got[:2], ref, True)
    check(want[:2], ref, True)
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]), "the MX8 copy differs from kernel 1's"
    assert bool((got[2] != 0).any()) and bool((got[3] != 0).any()), "the MX8 copy was not written"


@pytest.mark.gpu
@pytest.mark.parametrize("K", [768, 1024, 3072], ids=["nk12", "nk16", "nk48"])
def test_default_routing_per_k_tile_count(K):
    """The per-shape default is decided per K-tile count (proj: nk = 12, FC2: nk = 48; nk = 16 stands for the counts
    nobody measured), each by its own A/B against the deep ring: a routed count takes the walk on a grid of one workgroup per CU from two tiles per workgroup on, a
    count that is not routed keeps the deep ring at every size. The default's bits equal the references."""
    _, ops = _ops()
    M, N = LONG
    on = DEFAULT_ROUTED[K // 64]
    ref = reference(M, N, K)
    with routed(mode=1):
        cus = ops.gemm_persistent_grid(1 << 20, 4096, K, RES)   # 65536 tiles: the uncapped grid
    assert cus >= 8 and cus % 8 == 0
    with routed():
        assert ops.gemm_persistent_grid(2 * cus * 256, 256, K, RES) == (cus if on else 0)
        assert ops.gemm_persistent_grid((2 * cus - 1) * 256, 256, K, RES) == 0
        assert ops.gemm_persistent_grid(M, N, K, RES) == 0   # 36 tiles on the uncapped grid
        assert ops.gemm_persistent_grid(2 * cus * 256, 256, K, BIAS) == 0
        check(run(M, N, K), ref, True)
    with routed(cap=8):   # the default rule with a capped grid: 36 tiles >= 2 x 8
        assert ops.gemm_persistent_grid(M, N, K, RES) == (8 if on else 0)
        check(run(M, N, K), ref, True)
        check(run(M, N, K, inplace=False, planes=False), ref, False)


def test_walking_residual_kernel_compiles_without_scratch(tmp_path):
    """One workgroup per CU at 512 threads leaves a lane 256 VGPRs; a spill would put scratch traffic's vmcnt waits
    between the LDS-DMA pieces and their counted waits. Checked on the compiled gfx950 code, found by its own name;
    the three k_gemm_walk instances are still three."""
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
    seen = walk = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        name, desc = m.group(1), m.group(2)
        walk += bool(re.search(r"\dk_gemm_walkI", name))
        if not re.search(r"\dk_gemm_walk_resE", name):
            continue
        seen += 1
        field = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", desc)}
        assert field["private_segment_fixed_size"] == 0, (name, "scratch")
        assert field["next_free_vgpr"] <= 256, (name, field["next_free_vgpr"])
        assert field["group_segment_fixed_size"] <= 160 * 1024, (name, field["group_segment_fixed_size"])
        body = re.search(r"^" + re.escape(name) + r":(.*?)\.Lfunc_end", text, re.S | re.M).group(1)
        assert "scratch_" not in body, name
    assert seen == 1, seen
    assert walk == 3, walk
