"""The K loop of the tile-walking bf16 GEMM kernels as compiled for gfx950 (csrc/gemm_bf16.hip, gemm_walk_body): the
placement of the fragment reads and of the counted waits is a property of the instruction stream, so it is checked
there and not in the source. No GPU.

The region looked at runs from the kernel's first s_barrier (the prologue's) to the first s_barrier behind the last
MFMA (the end of q3): the tile's top, the ping-pong offset barrier, the four phases and the seam. The epilogue and the
prologue's own wait lie outside it. A phase's memory part is the span between two consecutive barriers that holds the
phase's two LDS-DMA issues.

Instances with the 4 / 4 / 8 / 8 order (walk_reads_early): no scratch, at most 256 VGPRs and 160 KiB of LDS; one loop body
(64 MFMAs); no vmcnt(0) in the region and one vmcnt(8) in each of the four memory parts; the memory parts hold 4, 4, 8
and 8 ds_read_b128; no span between two consecutive barriers holds more than 8 (the tile's first A0 fragments are read
in a span of their own, in front of the offset barrier); and the early fragments reach their MFMAs in the registers
they were read into: the ds_read_b128 are asynchronous inline asm, so a register copy between the read and the
lgkmcnt wait would copy stale values; the tile-top reads and q3's reads must name the same eight register quads and
the MFMAs must take their operands from exactly those.
The instance that keeps the parent's order (EPI_BIAS_GELU: not measured) shows 12, 4, 8, 0 with three waits."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EARLY = {"k_gemm_walk<4>", "k_gemm_walk<5>", "k_gemm_walk_res"}
PARENT_ORDER = {"k_gemm_walk<1>"}


def short_name(sym):
    m = re.search(r"\dk_gemm_walkILi(\d)E", sym)
    if m:
        return f"k_gemm_walk<{m.group(1)}>"
    return "k_gemm_walk_res" if re.search(r"\dk_gemm_walk_resE", sym) else None


@pytest.fixture(scope="module")
def walk_kernels(tmp_path_factory):
    """{short name: (descriptor fields, instruction lines of the body)} of the four walk kernels"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "vitparticlefiltertracker_amd", "csrc", "gemm_bf16.hip")
    out = tmp_path_factory.mktemp("walk_loop") / "gemm_bf16.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "--cuda-device-only",
                    "-S", "-o", str(out), src], check=True, capture_output=True)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        sym, desc = m.group(1), m.group(2)
        name = short_name(sym)
        if name is None:
            continue
        field = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", desc)}
        body = re.search(r"^" + re.escape(sym) + r":(.*?)\.Lfunc_end", text, re.S | re.M).group(1)
        lines = [ln.strip() for ln in body.splitlines()]
        found[name] = (field, [ln for ln in lines if ln and ln[0] not in ".;" and not ln.split()[0].endswith(":")])
    assert set(found) == EARLY | PARENT_ORDER, sorted(found)
    return found


def loop_region(insts):
    """instructions from the first s_barrier to the first s_barrier behind the last MFMA, both included"""
    bars = [i for i, ln in enumerate(insts) if ln.startswith("s_barrier")]
    last_mfma = max(i for i, ln in enumerate(insts) if ln.startswith("v_mfma"))
    return insts[bars[0]:min(b for b in bars if b > last_mfma) + 1]


def spans(region):
    """per span between two consecutive barriers: counts of reads, LDS-DMA issues, MFMAs, vmcnt(8) and the reads' destinations"""
    out, cur = [], None
    for ln in region:
        if ln.startswith("s_barrier"):
            if cur is not None:
                out.append(cur)
            cur = dict(reads=0, dma=0, mfma=0, wait8=0, dests=[])
            continue
        if ln.startswith("ds_read_b128"):
            cur["dests"].append(re.match(r"ds_read_b128 (v\[\d+:\d+\])", ln).group(1))
        cur["reads"] += ln.startswith("ds_read_b128")
        cur["dma"] += ln.startswith("global_load_lds")
        cur["mfma"] += ln.startswith("v_mfma")
        cur["wait8"] += bool(re.match(r"s_waitcnt vmcnt\(8\)", ln))
    return out


@pytest.mark.parametrize("name", sorted(EARLY))
def test_new_order_in_the_compiled_loop(walk_kernels, name):
    field, insts = walk_kernels[name]
    assert field["private_segment_fixed_size"] == 0 and not any("scratch_" in ln for ln in insts), "scratch"
    assert field["next_free_vgpr"] <= 256, field["next_free_vgpr"]
    assert field["group_segment_fixed_size"] <= 160 * 1024, field["group_segment_fixed_size"]
    region = loop_region(insts)
    assert sum(ln.startswith("v_mfma") for ln in region) == 64, "one K-tile body of four 16-MFMA quadrants"
    assert not any(re.match(r"s_waitcnt.*vmcnt\(0\)", ln) for ln in region), "vmcnt(0) inside the K loop"
    sp = spans(region)
    assert max(s["reads"] for s in sp) <= 8, [s["reads"] for s in sp]
    memory = [s for s in sp if s["dma"]]
    assert [s["dma"] for s in memory] == [2] * 4 and all(s["mfma"] == 0 for s in memory), memory
    assert [s["wait8"] for s in memory] == [1] * 4, memory
    assert sum(s["wait8"] for s in sp) == 4, "four vmcnt(8) per K-tile body"
    assert sorted(s["reads"] for s in memory) == [4, 4, 8, 8], [s["reads"] for s in memory]
    # the four MFMA blocks read nothing, and the only other reads of the region are the tile's first A0 fragments
    assert all(s["reads"] == 0 for s in sp if s["mfma"]), sp
    assert sorted(s["reads"] for s in sp if not s["dma"] and not s["mfma"] and s["reads"]) == [8], sp
    # the tile-top reads and q3's write the same eight register quads, and the MFMAs take them from there
    top = next(s for s in sp if not s["dma"] and not s["mfma"] and s["reads"])
    early = [s for s in memory if s["reads"] == 8 and set(s["dests"]) == set(top["dests"])]
    assert len(set(top["dests"])) == 8 and len(early) == 1, (top["dests"], [s["dests"] for s in memory])
    used = {op for ln in region if ln.startswith("v_mfma") for op in re.findall(r"v\[\d+:\d+\]", ln)[1:3]}
    assert set(top["dests"]) <= used, sorted(set(top["dests"]) - used)


@pytest.mark.parametrize("name", sorted(PARENT_ORDER))
def test_unmeasured_instance_keeps_the_parent_order(walk_kernels, name):
    field, insts = walk_kernels[name]
    assert field["private_segment_fixed_size"] == 0 and field["next_free_vgpr"] <= 256
    sp = spans(loop_region(insts))
    memory = [s for s in sp if s["dma"]]
    assert sorted(s["reads"] for s in memory) == [0, 4, 8, 12], memory
    assert sum(s["wait8"] for s in sp) == 3
