"""CPU: the stage models of tests/engine_reference.py prove themselves before tests/test_gpu_engine_stages.py holds the
engine to them.

* Free-running. Each stage's correctly rounded expectation feeds the next stage, through the engine's own buffer
  layout (aliases included). The CLS features then meet the project's contracts against oracle/vit.py on the same
  weights: cos >= 0.999 (bf16), >= 0.99 (fp8). So the stage models compose into the ViT. This one test runs on the
  weights as make_vit_weights draws them, for which the contracts are stated (measured: >= 0.99997 bf16, >= 0.9966
  fp8); the sharpened weights of every other test amplify each rounding through the depth (0.978 bf16 and 0.78 fp8 on
  the D = 1024 arch), which is the reason the sharp check is per launch.
* Self-pass. Every stage's own rounded output passes its own check, and nothing outside the written regions moves.
* Mutants. One wrong stage, on the inputs the free run had before that stage, against the clean expectation: it must
  miss the stage check.
    bias_dropped       every GEMM that has a bias (the folded CLS attention's b'_k is a constant over the keys and
                       cancels in the softmax: no case; gemm_cls_g has no bias)
    beta_dropped       b' = b                                                            (the LN-folded GEMMs)
    colsum_unrounded   colsum from the unrounded W gamma; on the MX8 GEMMs, from W' before its quantisation. Asserted
                       on the full-size QKV / K|V / FC1 stages. The residue sum(W' - W gamma) is about 0.3 2^-9
                       sum|W'| / sqrt(K) against an allowance of gamma_K sum|W'|: the ratio falls as K^-1.5, measured
                       5 - 7 at K = 192, 1.8 - 2 at K = 384 and 0.9 at K = 1024, so the bf16 D = 1024 case cannot see
                       it and has no case; nor can the n-row _cls stages (n F elements, none near a rounding tie).
    pos_shift          pos[m % g2] for pos[1 + m % g2]                                   (gemm_patch)
    cls_nopos          the CLS row without pos[0]                                        (cls_rows)
    layer              another block's weights (l + 1; the last block takes l - 1)       (every weighted stage)
    residual_x         the residual read from x instead of h                             (proj, fc2 and their _cls forms)
    last_key, scale (1 / hd), roll_heads, neighbour (the next particle's K / V or token rows), uniform (softmax
    replaced by uniform weights), q_row1 (the CLS query read from row 1; the q_rows = 1 K / V path)
    plane_missing      the last statistics plane not summed                              (stats_combine)
    planes_unrounded   planes of the values before their bf16 rounding                   (the producers)
    scale_next_group   an MX8 scale byte read from the next 16-row group of its brick    (the MX8-fed GEMMs)
* Sharpened weights. make_vit_weights(seed 4, perturb_affine) with every attn.qkv.weight and mlp.fc1.weight multiplied
  by engine_reference.SHARPEN_QKV, SHARPEN_FC1 = 8, 8. Condition: last_key and uniform miss the check in every
  attention stage of every arch. test_attention_mutants_fail_everywhere asserts it and prints the margins (the share
  of the stage's elements that are out, and the worst error over its allowance). Measured with 8 and 8:
    uniform    0.970 - 1.000 of every stage's elements out, worst error 244 - 507 allowances;
    last_key   full attention: 0.006 - 0.089 of the elements out, worst 97 - 506 allowances; the last block's CLS
               query (n D outputs): 0.010 - 0.079 out, worst 1.9 (ViT-Ti), 15 - 151 elsewhere.
  The CLS query's margin is the thin one and it does not grow with the factor: at 12 and 16 the softmax of that one
  query is sharp enough that the last key gets no weight at all (worst 0.0 - 0.5 allowances in most cases), so 8 and 8
  stay. For the same reason the two crops of s-fp8-kv are drawn with input seed 5 (engine_reference.INPUT_SEED): with
  seed 0 its last key weighs 0.46 of an allowance.
"""
import numpy as np
import pytest
import torch

import engine_reference as er
from oracle import pf
from oracle import vit as ovit

_TRACES = {}


def trace_of(case, sharp=True):
    """[(name, l, before, checks, after)] of the free-running reference, computed once per case."""
    if (case[0], sharp) in _TRACES:
        return _TRACES[case[0], sharp]
    ref = er.make_reference(case, sharp=sharp)
    n = case[4]
    bufs = ref.alloc()
    out = []
    for name, l in ref.sequence(len(ref.sets)):
        before = {k: v.copy() for k, v in bufs.items()}
        checks = ref.stage(name, l, before, n)
        for c in checks:
            c.commit(bufs)
        out.append((name, l, before, checks, {k: v.copy() for k, v in bufs.items()}))
    _TRACES[case[0], sharp] = (ref, out)
    return ref, out


IDS = [c[0] for c in er.CASES]


@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_free_running_meets_the_cosine_contract(case):
    ref, tr = trace_of(case, sharp=False)
    n, arch = case[4], ref.arch
    feat = torch.from_numpy(tr[-1][4]["feat"][:n].astype(np.float64))
    frame, p = ref.frame, ref.sets[0][0]
    patches = pf.crop_patches(frame, p, er.BOX, arch.img_size, arch.patch, arch.patch_kp, (0.5,) * 3, (0.5,) * 3)
    want = ovit.features_from_patches(torch.from_numpy(patches), ref.w, arch).double()
    cos = torch.nn.functional.cosine_similarity(feat, want, dim=1)
    print(case[0], "min cos", cos.min().item())
    assert cos.min().item() >= (0.99 if case[2] == "fp8" else 0.999), cos


@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_every_stage_passes_its_own_check(case):
    ref, tr = trace_of(case)
    assert [er.Reference.timer_name(t[0]) for t in tr][-1] == "cls_weight"
    for name, l, before, checks, after in tr:
        fails = er.verify_launch(checks, before, after)
        assert not fails, f"{name} block {l}: " + "\n".join(fails)


# ---- mutants ---------------------------------------------------------------------------------------------------------

_MREFS = {}


def _mref(case, mutant):
    key = (case[0], mutant)
    if key not in _MREFS:
        _MREFS[key] = er.make_reference(case, mutant)
    return _MREFS[key]


def mutant_after(case, mutant, name, l, before, mod=None):
    """The buffers after a mutant of stage `name` ran on `before` (mod: a change to the inputs it reads)."""
    mref = _mref(case, mutant)
    src = mod(before) if mod is not None else before
    after = {k: v.copy() for k, v in before.items()}
    for c in mref.stage(name, l, src, case[4]):
        c.commit(after)
    return after


def misses(checks, after):
    return any(c.bad(after).any() for c in checks)


def margins(checks, after):
    """(share of elements out, worst error / allowance) over the stage's bf16 and MX8 outputs."""
    out, worst = [0.0], 0.0
    for c in checks:
        if c.kind not in ("bf16", "mx8"):
            continue
        bad = c.bad(after)
        out.append(bad.mean())
        if c.kind == "bf16":
            g = er.val_of(after[c.buf].ravel()[c.idx])
            allow = 0.5 * er.ulp16(np.maximum(np.abs(c.exp), np.abs(g))) + c.tol
            worst = max(worst, float((np.abs(g - c.exp) / allow).max()))
    return max(out), worst


GEMMS = ("gemm_patch", "gemm_qkv", "gemm_kv", "gemm_q_cls", "gemm_proj", "gemm_fc1", "gemm_fc2", "gemm_cls_v",
         "gemm_proj_cls", "gemm_fc1_cls", "gemm_fc2_cls")
LN_GEMMS = ("gemm_qkv", "gemm_kv", "gemm_q_cls", "gemm_fc1", "gemm_fc1_cls")
WEIGHTED = GEMMS[1:] + ("gemm_cls_g",)
RESIDUAL = ("gemm_proj", "gemm_fc2", "gemm_proj_cls", "gemm_fc2_cls")
ATTN = ("attention", "attention_cls")
MUTANT_CASES = [c for c in er.CASES if c[0] in ("ti-bf16", "s-bf16", "s-fp8", "s-fp8-kv", "p14-bf16", "p14-fp8")]
MIDS = [c[0] for c in MUTANT_CASES]


def _stages(case, names):
    ref, tr = trace_of(case)
    return ref, [t for t in tr if t[0] in names]


WEIGHT_MUTANTS = [("bias_dropped", GEMMS), ("beta_dropped", LN_GEMMS),
                  ("colsum_unrounded", ("gemm_qkv", "gemm_kv", "gemm_fc1")), ("pos_shift", ("gemm_patch",)),
                  ("cls_nopos", ("cls_rows",))]
# colsum_unrounded at K = 1024 in bf16 is inside the derived bound (module docstring): no case
WEIGHT_CASES = [(m, names, c) for m, names in WEIGHT_MUTANTS for c in MUTANT_CASES
                if not (m == "colsum_unrounded" and c[1] == "p14" and c[2] == "bf16")]


@pytest.mark.parametrize("mutant,names,case", WEIGHT_CASES, ids=[f"{m}-{c[0]}" for m, _, c in WEIGHT_CASES])
def test_weight_mutants_fail(mutant, names, case):
    ref, st = _stages(case, names)
    assert st
    for name, l, before, checks, _ in st:
        after = mutant_after(case, mutant, name, l, before)
        share, worst = margins(checks, after)
        print(f"{case[0]} {name} block {l} {mutant}: {share:.5f} of the elements out, worst error / allowance "
              f"{worst:.2f}")
        assert misses(checks, after), f"{mutant} passes {name} block {l}"


@pytest.mark.parametrize("case", MUTANT_CASES, ids=MIDS)
def test_another_layers_weights_fail(case):
    ref, tr = trace_of(case)
    last = ref.arch.depth - 1
    seen = 0
    for name, l, before, checks, _ in tr:
        fold = name == "attention_cls" and ref.cls_fused
        if not (name in WEIGHTED or fold):
            continue
        l2 = l - 1 if l == last else l + 1
        after = {k: v.copy() for k, v in before.items()}
        for c in ref.stage(name, l2, before, case[4]):
            c.commit(after)
        if fold:
            continue    # b'_k of another block: a constant over the keys, cancels in the softmax (module docstring)
        assert misses(checks, after), f"block {l2}'s weights pass {name} block {l}"
        seen += 1
    assert seen


@pytest.mark.parametrize("case", MUTANT_CASES, ids=MIDS)
def test_residual_from_x_fails(case):
    ref, st = _stages(case, RESIDUAL)
    for name, l, before, checks, _ in st:
        def mod(b):
            b = dict(b)
            hx = b["x"].copy()
            b["h"] = hx
            return b
        # the A operand of proj is x in both: only the residual changes; fc2 reads hid
        after = mutant_after(case, None, name, l, before, mod)
        assert misses(checks, after), f"the residual from x passes {name} block {l}"


def _fused(case):
    return er.make_reference(case).cls_fused


# q_row1 is the CLS query of the K / V path (the folded kernel takes q as its own argument): the unfused cases only
ATTN_CASES = [(m, c) for m in ("last_key", "uniform", "scale", "roll_heads", "neighbour", "q_row1")
              for c in MUTANT_CASES if not (m == "q_row1" and _fused(c))]


@pytest.mark.parametrize("mutant,case", ATTN_CASES, ids=[f"{m}-{c[0]}" for m, c in ATTN_CASES])
def test_attention_mutants_fail_everywhere(mutant, case):
    ref, st = _stages(case, ATTN)
    assert st
    seen = 0
    for name, l, before, checks, _ in st:
        fold = name == "attention_cls" and ref.cls_fused
        if mutant == "q_row1" and name != "attention_cls":
            continue       # q_rows = N reads every row: the off-by-one is the q_rows = 1 stage's
        if mutant == "roll_heads" and fold:
            continue       # G and U are per head by layout: gemm_cls_g / gemm_cls_v carry the head routing
        after = mutant_after(case, mutant, name, l, before)
        share, worst = margins(checks, after)
        print(f"{case[0]} {name} block {l} {mutant}: {share:.3f} of the elements out, worst error / allowance "
              f"{worst:.1f}")
        assert misses(checks, after), f"{mutant} passes {name} block {l}"
        seen += 1
    skipped = 1 if (mutant == "roll_heads" and ref.cls_fused) else len(st) - 1 if mutant == "q_row1" else 0
    assert seen == len(st) - skipped and seen > 0


@pytest.mark.parametrize("case", MUTANT_CASES, ids=MIDS)
def test_missing_plane_fails(case):
    ref, st = _stages(case, ("stats_combine", "stats_combine_cls"))
    assert st
    P = ref.P
    for name, l, before, checks, _ in st:
        def mod(b):
            b = dict(b)
            key = "planes_cls_flat" if name.endswith("_cls") else "planes_flat"
            rows = case[4] * (1 if name.endswith("_cls") else ref.N)
            pl = b[key].copy()
            pl[: P * rows * 2].reshape(P, rows, 2)[P - 1] = 0
            b[key] = pl
            return b
        after = mutant_after(case, None, name, l, before, mod)
        bad = checks[0].bad(after).any(axis=1)
        if not name.endswith("_cls"):
            # cls_rows writes the CLS rows' statistics into plane 0 alone: until the first proj rewrites them their
            # last plane holds zeros, and dropping it changes nothing
            bad = np.delete(bad, np.arange(case[4]) * ref.N)
        assert bad.all(), f"a missing plane passes rows of {name} block {l}"


@pytest.mark.parametrize("case", MUTANT_CASES, ids=MIDS)
def test_planes_of_unrounded_values_fail(case):
    """The producer sums its fp32 values before the bf16 rounding instead of the stored ones: 64 rounding errors of up
    to 2^-9 relative do not cancel inside gamma_64 = 72 u of the block's absolute sum."""
    ref, st = _stages(case, ("gemm_patch", "gemm_proj", "gemm_fc2", "gemm_proj_cls"))
    assert st
    for name, l, before, checks, after in st:
        hc = checks[0]
        pc = [c for c in checks if c.what.endswith(" planes")]
        assert len(pc) == 1 and hc.kind == "bf16"
        mut = {k: v.copy() for k, v in after.items()}
        v = hc.exp.reshape(hc.exp.shape[0], ref.P, 64)
        e = np.stack([v.sum(2), (v * v).sum(2)], 2).transpose(1, 0, 2)
        mut[pc[0].buf].reshape(-1)[pc[0].idx] = e.astype(np.float32)
        assert pc[0].bad(mut).any(), f"planes of the unrounded values pass {name} block {l}"


@pytest.mark.parametrize("case", [c for c in MUTANT_CASES if c[2] == "fp8"],
                         ids=[c[0] for c in MUTANT_CASES if c[2] == "fp8"])
def test_scale_byte_of_the_next_row_group_fails(case):
    ref, tr = trace_of(case)
    last = ref.arch.depth - 1
    seen = set()
    for name, l, before, checks, _ in tr:
        reads = {"gemm_qkv": "h8s", "gemm_fc1": "h8s", "gemm_kv": "h8s", "gemm_fc2": "hid8s",
                 "gemm_proj": "hid8s" if ref.N <= 256 else None}.get(name)
        if reads is None or (l == last and name != "gemm_kv"):
            continue

        def mod(b):
            b = dict(b)
            s = b[reads]
            b[reads] = np.roll(s.reshape(s.shape[0], -1, 4), -1, axis=2).reshape(s.shape)   # byte f <- byte f + 1
            return b
        after = mutant_after(case, None, name, l, before, mod)
        assert misses(checks, after), f"the next row group's scale bytes pass {name} block {l}"
        seen.add(name)
    assert {"gemm_qkv", "gemm_fc1", "gemm_fc2"} <= seen
