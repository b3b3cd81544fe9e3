"""GPU (one MI355X): Tracker and MultiTracker are one frame loop (tracker._TargetLoop), Tracker its K = 1 case. The
checkpoint schema of both classes, literally; one source for both classes' checkpoint arrays; a second `init` equals a
new tracker; the per-frame launch sequence of both classes and of two targets; a held target keeps its templates in the
batched update. ViT-Ti/16 bf16, 64 particles, the tinted synthetic 224 x 224 clip, at most 4 tracked frames per test:
what can go wrong here is host logic, not a tile edge.

Feature sets: A = ESS-gated resampling, constant velocity, the angle row, the colour cue, a template update; B = the
colour cue with its surround ring, the occlusion gate, re-detection, the mode estimate, a template update. (The gate is
not combined with resample.ess_threshold, so they cannot be one set.) Both targets are tinted into one colour bin each,
so under B's gate (the default threshold 0.05) a particle on a visible target scores a peak near 1 (0.96 to 0.99 on
these frames), while on an all-black frame every box sample falls in colour bin 0, where the templates are empty: rho = 0
and the colour weight alone is e^-20 = 2.1e-9 for every particle (SPEC S13). Each test asserts the held / not-held
frames it relies on before anything else."""
import json

import numpy as np
import pytest
import torch

import s13_reference as R13

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P_L, D, BINS, SEED = 64, 192, 4, 77
BOXES = [R13.FOLLOW["box"], (8, 8, 48, 40)]             # two sizes: each target has its own box and mode window
TINT_2 = ((0, 64), (192, 256), (128, 192))
BOXES_2 = [(84, 82, 56, 60), (150, 20, 40, 48)]         # the second init's
OUTPUTS = ("last_held", "last_peak", "last_evidence", "held_frames", "lost", "last_searched", "last_reacquired",
           "last_mean", "last_mode_index", "last_mode_mass", "last_ess", "last_resampled", "last_velocity",
           "last_rotation")
PER_TARGET = ("pf_frame", "particles_soa", "template", "box_wh", "carry", "velocity_soa", "rotation_soa",
              "color_template", "held_frames", "anchor")


def _cfg(features, seed=SEED):
    from vitparticlefiltertracker_amd import load_config
    cfg = {"model": {"arch": "vit_tiny_patch16_224", "dtype": "bf16", "weights": {"seed": 3}},
           "particles": {"num": P_L, "seed": seed}}
    color = {"bins": BINS, "grid": 8}
    if features == "A":
        cfg["particles"].update(motion_model="constant_velocity", rotation_std=0.02)
        cfg["resample"] = {"ess_threshold": 0.5}
        cfg["likelihood"] = {"color": color, "template_update": 0.1}
    elif features == "B":
        cfg["likelihood"] = {"color": color, "color_surround": {}, "occlusion": {}, "redetect": {},
                             "template_update": 0.1}
        cfg["estimate"] = {"method": "mode"}
    else:
        assert features == "default"
    return load_config(cfg)


def _tracker(kind, features, **kw):
    """kind: "single", or the number of targets of a MultiTracker."""
    from vitparticlefiltertracker_amd import MultiTracker, Tracker
    if kind == "single":
        return Tracker(_cfg(features), device=DEV, **kw)
    return MultiTracker(_cfg(features), n_objects=kind, device=DEV, **kw)


def _init(tr, kind, frame, boxes=BOXES):
    tr.init(frame, boxes[0]) if kind == "single" else tr.init(frame, boxes[:kind])


def _arrays_equal(a, b, tag):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), tag


@pytest.fixture(scope="module")
def clip():
    """The tinted clip, with a second, static target painted over BOXES[1] in another tint (one colour bin at 4 bins per
    channel, like the moving target's), so that under B both targets stand out from the noise background."""
    from vitparticlefiltertracker_amd.frames import synthetic_clip
    frames = synthetic_clip(6, target_range=R13.TINT).copy()
    x, y, w, h = BOXES[1]
    rng = np.random.default_rng(5)
    frames[:, y:y + h, x:x + w] = np.stack([rng.integers(lo, hi, (h, w), dtype=np.uint8) for lo, hi in TINT_2], axis=-1)
    return frames


# ------------------------------------------------------------------ 1. the checkpoint schema, literal
def _schema(features, K):
    """key -> (numpy dtype, shape) of state_dict(); K None: a Tracker. `config` is checked apart."""
    lead = () if K is None else (K,)
    nb = BINS ** 3
    s = {"format": (np.int64, ()), "frame_index": (np.int64, ()), "pf_frame": (np.int64, lead),
         "particles_soa": (np.float32, lead + (3, P_L)), "template": (np.float32, lead + (D,)),
         "box_wh": (np.float64, lead + (2,)), "frame_hw": (np.int64, (2,))}
    if K is not None:
        s["n_objects"] = (np.int64, ())
    if features == "A":
        s.update(carry=(np.int64, lead + (P_L,)), velocity_soa=(np.float32, lead + (2, P_L)),
                 rotation_soa=(np.float32, lead + (1, P_L)), color_template=(np.float32, lead + (nb,)))
    if features == "B":
        s.update(color_template=(np.float32, lead + (nb,)), held_frames=(np.int64, lead),
                 anchor=(np.float64, lead + (3,)))
    return s


@pytest.mark.parametrize("features", ["default", "A", "B"])
def test_checkpoint_schema_is_the_literal_table(clip, features):
    for kind, K in (("single", None), (2, 2)):
        tr = _tracker(kind, features)
        _init(tr, kind, clip[0])
        for f in clip[1:3]:
            tr.track(f)
        sd = tr.state_dict()
        want = _schema(features, K)
        assert set(sd) == set(want) | {"config"}, (kind, sorted(sd))
        for key, (dtype, shape) in want.items():
            v = np.asarray(sd[key])
            assert v.dtype == dtype and v.shape == shape, (kind, key, v.dtype, v.shape)
        assert int(sd["format"]) == 3 and int(sd["frame_index"]) == 2
        assert np.asarray(sd["pf_frame"]).tolist() == (2 if K is None else [2] * K)
        assert np.asarray(sd["box_wh"]).tolist() == ([64.0, 64.0] if K is None else [[64.0, 64.0], [48.0, 40.0]])
        assert np.asarray(sd["frame_hw"]).tolist() == [224, 224]
        config = np.asarray(sd["config"])
        assert config.shape == () and config.dtype.kind == "U"
        fingerprint = json.loads(str(config))
        assert fingerprint == tr.config_fingerprint()
        assert fingerprint.get("n_objects") == K and ("n_objects" in fingerprint) == (K is not None)
        if features == "default":
            assert not set(fingerprint) & {"ess_threshold", "motion_model", "rotation_std", "color", "color_surround",
                                           "occlusion", "redetect", "estimate"}


# ------------------------------------------------------------------ 2. one checkpoint, two classes' arrays
@pytest.mark.parametrize("features", ["A", "B"])
def test_one_target_checkpoint_arrays_are_the_trackers(clip, features):
    sds = {}
    for kind in ("single", 1):
        tr = _tracker(kind, features)
        _init(tr, kind, clip[0])
        for f in clip[1:4]:
            tr.track(f)
        sds[kind] = tr.state_dict()
    one, many = sds["single"], sds[1]
    assert set(many) == set(one) | {"n_objects"} and int(many["n_objects"]) == 1
    assert set(one) - {"format", "frame_index", "frame_hw", "config"} <= set(PER_TARGET)
    for key in set(one) - {"config"}:
        _arrays_equal(one[key], np.squeeze(many[key], 0) if key in PER_TARGET else many[key], key)


# ------------------------------------------------------------------ 3. a second init equals a new tracker
def _run(tr, kind, frames):
    """Per frame: the estimates and every frame output; then the checkpoint arrays."""
    rec = []
    for f in frames:
        rec.append((tr.track(f), {name: getattr(tr, name) for name in OUTPUTS}))
    return rec, tr.state_dict()


@pytest.mark.parametrize("features", ["A", "B"])
@pytest.mark.parametrize("kind", ["single", 2])
def test_second_init_equals_a_new_tracker(clip, kind, features):
    again = _tracker(kind, features, use_graph=True)
    _init(again, kind, clip[0])
    for f in clip[1:3]:
        again.track(f)
    assert again._graph is not None
    _init(again, kind, clip[3], BOXES_2)
    assert again._graph is None and again.frame_index == 0        # the captured graph read the first init's templates
    templates = [t.data_ptr() for t in again.templates + again.color_templates]
    fresh = _tracker(kind, features, use_graph=True)
    _init(fresh, kind, clip[3], BOXES_2)
    for t_a, t_f in zip(again.templates + again.color_templates, fresh.templates + fresh.color_templates):
        assert torch.equal(t_a.view(torch.int32), t_f.view(torch.int32))
    got, got_sd = _run(again, kind, clip[4:6])
    want, want_sd = _run(fresh, kind, clip[4:6])
    # the new graph reads, and the updates wrote in place, the buffers that the second init made
    assert again._graph is not None and [t.data_ptr() for t in again.templates + again.color_templates] == templates
    for k, (g, w) in enumerate(zip(got, want), start=1):
        assert g == w, f"frame {k} after the second init"
    assert set(got_sd) == set(want_sd)
    for key in got_sd:
        _arrays_equal(got_sd[key], want_sd[key], key)


# ------------------------------------------------------------------ 4. the launch sequence
def _launches(tr, frame):
    from vitparticlefiltertracker_amd.vit import KernelTimer
    tr.engine.timer = KernelTimer()
    tr.track(frame)
    names = [name for name, _, _ in tr.engine.timer.pending]
    tr.engine.timer = None
    return names


@pytest.mark.parametrize("features", ["default", "B"])
def test_launch_sequence_of_both_classes_and_of_two_targets(clip, features):
    """A frame's timed launches: crop_patches per target, the patch GEMM and encoder (`body`), then per target
    cls_weight and, under B, color_weight_surround. With a template update (B) on a frame that is not held, the
    features pass of the K estimate crops follows: crop_patches per target and the same body; on a held frame (B: an
    all-black image) nothing follows."""
    tail = ["cls_weight"] + (["color_weight_surround"] if features == "B" else [])
    seen = {}
    for kind in ("single", 1, 2):
        tr = _tracker(kind, features, use_graph=False)
        _init(tr, kind, clip[0])
        seen[kind] = [_launches(tr, clip[1])]
        not_held = False if features == "B" else None            # None: no gate
        assert tr.last_held is not_held if kind == "single" else tr.last_held == [not_held] * kind
        if features == "B":
            seen[kind].append(_launches(tr, np.zeros_like(clip[1])))
            assert tr.last_held is True if kind == "single" else tr.last_held == [True] * kind
    assert seen["single"] == seen[1]
    first = seen["single"][0]
    body = first[1:first.index("cls_weight")]
    assert "crop_patches" not in body and "cls_weight" not in body and "gemm_patch" in body and len(body) > 12
    for kind, K in (("single", 1), (2, 2)):
        forward = ["crop_patches"] * K + body + tail * K
        update = ["crop_patches"] * K + body if features == "B" else []
        assert seen[kind][0] == forward + update, (kind, seen[kind][0])
        if features == "B":
            assert seen[kind][1] == forward, (kind, seen[kind][1])


# ------------------------------------------------------------------ 5. a held target keeps its templates in the batch
def test_held_target_keeps_its_templates_in_the_batched_update(clip):
    """Target 0's surroundings are blanked, target 1 (on the static background, away from it) stays visible: target 0 is
    held and keeps both templates' bits, target 1's template moves, though the update's feature pass covers both."""
    mt = _tracker(2, "B")
    _init(mt, 2, clip[0])
    frame = clip[1].copy()
    frame[64:184, 64:184] = 0           # target 0's box (80..144, moving 2 px a frame) and every particle's around it
    before = [[t.clone() for t in ts] for ts in (mt.templates, mt.color_templates)]
    mt.track(frame)
    assert mt.last_held == [True, False]
    for ts, was in zip((mt.templates, mt.color_templates), before):
        assert torch.equal(ts[0].view(torch.int32), was[0].view(torch.int32))
    assert not torch.equal(mt.templates[1].view(torch.int32), before[0][1].view(torch.int32))
