"""GPU (MI355X): every launch of the bf16 and fp8 `ViTEngine` forward against its stage model (tests/engine_reference.py).

A recorder installed as `eng.timer` (eager mode; every launch of the chain goes through `_run(timer, name, fn, *args)`)
clones the `[:batch]` extent of every activation buffer before and after each launch of one `forward_weights` call:
h, x, qkv, hid_flat, stats, planes_flat, planes_cls_flat, h8, hid8, clsG, clsU, splitk_ws, Q, feat, sim. Per launch:

1. the name sequence is the one the arch, dtype and flags imply (`Reference.sequence`, written from the model);
2. the stage model's expectation, computed in fp64 from the before-snapshot and the model's ORIGINAL fp32 weights,
   against the after-snapshot of the written region, within the stage's derived tolerance (engine_reference docstring);
3. every byte of every buffer outside the written region is unchanged: rows >= n, the K | V columns during gemm_q_cls,
   h during QKV and FC1, the MX8 scale words of bricks wholly past n N. The one region vpf.h leaves unspecified, the
   scale bytes of rows >= M inside the last written brick, is exactly what the models mark `any`; the split-K
   workspace is scratch.

Cases: depth-3 archs (two full blocks, so one consumes another's planes and MX8 copy, plus the last block), sharpened
weights (tests/test_engine_reference_cpu.py shows what they buy), a 224 x 224 random frame, 64 x 64 boxes:

  ti-bf16          ViT-Ti/16 (D 192, H 3)   planes, unfused K / V last block, split-K fc2            n / batch 3 / 3
  s-bf16           ViT-S/16 (D 384, H 6)    folded CLS tail, n < batch                               3 / 5
  s-bf16-onepass   cls_fused=False, cls_splitk=False: the one-pass _cls GEMMs                        3 / 3
  s-fp8            MX8 QKV / FC1 / FC2, MX8 attention in hid8's storage, lds sized for the batch      3 / 5
  s-fp8-kv         cls_fused=False: MX8 gemm_kv on the wkv8 slice                                    2 / 2
  p14-bf16         patch 14, img 238 (N = 290), D 1024, H 16, mlp 1024: odd-patch crop with Kp padding, 16 planes,
                   streamed attention (N > 256)                                                      2 / 2
  p14-fp8          the fp8 branch with bf16 attention and the gemm_q8_ proj                          2 / 3

plus the multi-set embed, the walk-routed GEMMs inside the engine and the graph replay. The LN fold without planes
needs D > 1024, which vpf_row_stats_* and vpf_cls_weight_* refuse: a dead branch, no case.
"""
import numpy as np
import pytest
import torch

import engine_reference as er
from oracle import mx8 as omx

pytestmark = pytest.mark.gpu
DEV = "cuda"

BUFFERS = ("h", "x", "qkv", "hid_flat", "stats", "planes_flat", "planes_cls_flat", "clsG", "clsU", "splitk_ws", "Q",
           "feat", "sim")


def _np(t: torch.Tensor) -> np.ndarray:
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


class Recorder:
    """eng.timer: snapshots of every activation buffer around each launch."""

    def __init__(self, eng):
        self.eng = eng
        self.launches = []      # (name, before, after)

    def snap(self):
        torch.cuda.synchronize()
        e = self.eng
        out = {k: _np(getattr(e, k)) for k in BUFFERS if hasattr(e, k)}
        if e.fp8:
            for k, (q, s) in (("h8", e.h8), ("hid8", e.hid8)):
                out[k + "q"] = _np(q)
                out[k + "s"] = _np(s.view(torch.uint8))
        return out

    def __call__(self, name, fn, *args):
        before = self.snap()
        fn(*args)
        self.launches.append((name, before, self.snap()))


_RUNS = {}


def run_case(case):
    """(engine, Reference, recorded launches, device inputs) of the eager recorded forward, once per case."""
    if case[0] in _RUNS:
        return _RUNS[case[0]]
    from vitparticlefiltertracker_amd.vit import ViTEngine
    ref = er.make_reference(case)
    _, _, dtype, flags, n, batch = case
    eng = ViTEngine(ref.arch, ref.w, dtype, DEV, batch, **flags)
    assert eng.cls_fused == ref.cls_fused and eng.use_planes
    inputs = (torch.from_numpy(ref.frame).to(DEV), torch.from_numpy(ref.sets[0][0]).to(DEV), er.BOX,
              torch.from_numpy(ref.tmpl).to(DEV), er.LAM, er.BITS, True)
    rec = Recorder(eng)
    eng.timer = rec
    try:
        eng.forward_weights(*inputs)
    finally:
        eng.timer = None
    torch.cuda.synchronize()
    _RUNS[case[0]] = (eng, ref, rec.launches, inputs)
    return _RUNS[case[0]]


def check_launches(ref, launches, seq, n):
    assert [nm for nm, _, _ in launches] == [er.Reference.timer_name(nm) for nm, _ in seq]
    fails = []
    for i, ((name, l), (_, before, after)) in enumerate(zip(seq, launches)):
        assert sorted(before) == sorted(ref.shapes()), (sorted(before), sorted(ref.shapes()))
        for k, (shape, dt) in ref.shapes().items():
            assert before[k].shape == shape and before[k].dtype == dt, (k, before[k].shape, shape)
        for f in er.verify_launch(ref.stage(name, l, before, n), before, after):
            fails.append(f"launch {i} {name} (block {l}): {f}")
    assert not fails, "\n".join(fails)


IDS = [c[0] for c in er.CASES]


@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_every_launch_matches_its_stage_model(case):
    eng, ref, launches, _ = run_case(case)
    check_launches(ref, launches, ref.sequence(1), case[4])


@pytest.mark.parametrize("case", [c for c in er.CASES if c[2] == "fp8"], ids=[c[0] for c in er.CASES if c[2] == "fp8"])
def test_engine_mx8_weights(case):
    """The engine's MX8 weight copies are oracle.mx8.quantize of the reference's bf16 weights, bit for bit and in the
    device layout; wkv8 is the [D:] rows of wqkv8; the LN-fold colsums of the dequantised values are within gamma_K
    sum|w| of their fp64 sums."""
    from vitparticlefiltertracker_amd import ops
    eng, ref, _, _ = run_case(case)
    D = ref.D
    for l, L in enumerate(eng.layers):
        R = ref.layer(l)
        for key, rk in (("wqkv8", "qkv"), ("wproj8", "proj"), ("wfc18", "fc1"), ("wfc28", "fc2")):
            q, s = L[key]
            rows, K = R[rk]["codes"].shape
            assert tuple(q.shape) == (rows, K) and tuple(s.shape) == (K // 128, rows)
            assert np.array_equal(q.cpu().numpy(), R[rk]["codes"]), f"block {l} {key} codes"
            assert np.array_equal(s.cpu().numpy(), omx.pack_scales(R[rk]["sc"], rows)), f"block {l} {key} scale planes"
        q, s = L["wkv8"]
        assert np.array_equal(q.cpu().numpy(), R["qkv"]["codes"][D:]), f"block {l} wkv8 codes"
        assert s.is_contiguous() and np.array_equal(ops.mx8_scale_bytes(s, 2 * D).cpu().numpy(), R["qkv"]["sc"][D:])
        for key, rk in (("cqkv8", "qkv"), ("cfc18", "fc1")):
            W8 = R[rk]["W8"]
            err = np.abs(L[key].double().cpu().numpy() - W8.sum(1))
            assert (err <= er.gam(W8.shape[1]) * np.abs(W8).sum(1)).all(), f"block {l} {key}: {err.max()}"


def test_multi_set_embed():
    """embed_many with two particle sets and two boxes: both crops, the patch GEMM over all rows and the CLS rows."""
    from vitparticlefiltertracker_amd.vit import ViTEngine
    case = ("s-bf16-sets", "s", "bf16", {}, 3, 4)
    ref = er.make_reference(case)
    frame, p = er.case_inputs(3, seed=1)
    sets = [(np.ascontiguousarray(p[:, :1]), (64.0, 64.0)), (np.ascontiguousarray(p[:, 1:]), (48.0, 80.0))]
    ref.frame, ref.sets = frame, sets
    eng = ViTEngine(ref.arch, ref.w, "bf16", DEV, 4)
    rec = Recorder(eng)
    eng.timer = rec
    try:
        n = eng.embed_many(torch.from_numpy(frame).to(DEV), [torch.from_numpy(s).to(DEV) for s, _ in sets],
                           [b for _, b in sets])
    finally:
        eng.timer = None
    assert n == 3
    check_launches(ref, rec.launches, ref.sequence(2)[:4], 3)


def test_walk_routed_gemms_inside_the_engine():
    """The bf16 ViT-S case again with every GEMM that can walk routed to the tile-walking kernels (591 rows: FC1 and QKV
    have >= 8 output tiles): every recorded after-snapshot equals the default run's, bit for bit."""
    from vitparticlefiltertracker_amd import _lib, ops
    from vitparticlefiltertracker_amd.vit import ViTEngine
    case = [c for c in er.CASES if c[0] == "s-bf16"][0]
    _, ref, launches, inputs = run_case(case)
    rows = case[4] * ref.N
    # an engine of its own, started from the bytes the default run started from, so that whole snapshots compare
    eng = ViTEngine(ref.arch, ref.w, case[2], DEV, case[5], **case[3])
    for k, v in launches[0][1].items():
        t = torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v)
        getattr(eng, k).copy_(t.view(torch.bfloat16) if v.dtype == np.uint16 else t)
    rec = Recorder(eng)
    ops.gemm_persistent(1, 8)
    try:
        assert ops.gemm_persistent_grid(rows, ref.F, ref.D, _lib.VPF_EPI_LN_GELU) > 0       # FC1 walks
        assert ops.gemm_persistent_grid(rows, 3 * ref.D, ref.D, _lib.VPF_EPI_LN) > 0        # QKV walks
        eng.timer = rec
        eng.forward_weights(*inputs)
    finally:
        eng.timer = None
        ops.gemm_persistent(0, 0)
    assert [a for a, _, _ in rec.launches] == [a for a, _, _ in launches]
    for i, ((name, _, got), (_, _, want)) in enumerate(zip(rec.launches, launches)):
        for k in want:
            a, b = got[k].reshape(-1), want[k].reshape(-1)
            same = a.view(f"u{a.dtype.itemsize}") == b.view(f"u{b.dtype.itemsize}")
            assert same.all(), f"launch {i} {name}: {k} differs from the default run at {np.flatnonzero(~same)[:8]}"


@pytest.mark.parametrize("case", [c for c in er.CASES if c[0] in ("s-bf16", "s-fp8")], ids=["s-bf16", "s-fp8"])
def test_graph_replay_equals_the_eager_run(case):
    """A captured and replayed forward of the same case leaves h[:n], Q[:n] and feat[:n] equal to the eager recorded
    run, bit for bit (the buffers are cleared before the replay)."""
    eng, ref, launches, inputs = run_case(case)
    n = case[4]
    want = launches[-1][2]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.forward_weights(*inputs)       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        eng.forward_weights(*inputs)
    eng.h[:n].zero_()
    eng.Q[:n].zero_()
    eng.feat[:n].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_np(eng.h[:n]), want["h"][:n])
    assert np.array_equal(_np(eng.Q[:n]), want["Q"][:n])
    assert np.array_equal(_np(eng.feat[:n]).view(np.uint32), want["feat"][:n].view(np.uint32))
