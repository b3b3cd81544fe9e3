"""GPU (one MI355X): SPEC S13 end to end — a ParticleFilter driven by the colour cue alone FOLLOWS the tinted target,
bit for bit with the numpy reference (tests/s13_reference.py); the Tracker and MultiTracker with `likelihood.color`
(ViT-Ti, fp32) multiply the cue into the ViT weight exactly, with and without the captured graph and with the angle row;
the histogram template's update and checkpoint; and the default tracker left as it was."""
import numpy as np
import pytest
import torch

import s10_reference as R10
import s13_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K40 = 40
HW = (224, 224)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def tinted():
    from vitparticlefiltertracker_amd.frames import synthetic_clip
    return synthetic_clip(R.FOLLOW["frames"], target_range=R.TINT)


# ------------------------------------------------------------------ the colour-only filter loop follows the target
def test_colour_only_filter_follows_the_target_and_equals_the_reference(tinted):
    """ParticleFilter + ops.color_weight (combine = 0), P = 256, the configuration's defaults, 23 tracked frames of the
    tinted clip: predicted rows, Q, ancestors and resampled rows equal the reference's every frame, the estimates to
    1e-12, and so the DEVICE's estimates stay within the host test's bound of the true centre (112 + 2 k, 112 + k)."""
    from vitparticlefiltertracker_amd import ops
    from vitparticlefiltertracker_amd.particle_filter import ParticleFilter
    F = R.FOLLOW
    bx, by, bw, bh = F["box"]
    ref = R.follow(tinted)
    pf = ParticleFilter(F["P"], (bx + 0.5 * bw, by + 0.5 * bh, 1.0), F["motion_std"], F["scale_range"], F["seed"], DEV,
                        frame_size=F["frame_size"], lam=20.0, weight_bits=F["K"])
    ws = ops.rgba_workspace(HW, DEV)
    one = torch.tensor([[bx + 0.5 * bw], [by + 0.5 * bh], [1.0]], device=DEV)
    hist = torch.empty(1, 512, device=DEV, dtype=torch.int32)
    f0 = torch.from_numpy(tinted[0]).to(DEV)
    torch.ops.vpf.color_weight(f0, ws, True, one, None, [float(bw), float(bh)], list(HW), 32, 8, None, 0.0, 0, False,
                               hist, None, None)
    tmpl = (hist[0].to(torch.float32) / 1024.0).contiguous()
    assert np.array_equal(bits(tmpl.cpu().numpy()), bits(R.template(tinted[0], F["box"], None, 32, 8)))
    Q = torch.empty(F["P"], device=DEV, dtype=torch.int64)
    dist = []
    for k, want in enumerate(ref, start=1):
        fd = torch.from_numpy(tinted[k]).to(DEV)
        pf.predict(k)
        assert np.array_equal(bits(pf.particles_soa.cpu().numpy()), bits(want["pred"])), f"frame {k}: predicted rows"
        torch.ops.vpf.color_weight(fd, ws, True, pf.particles_soa, None, [float(bw), float(bh)], list(HW), 32, 8, tmpl,
                                   20.0, F["K"], False, None, None, Q)
        assert np.array_equal(Q.cpu().numpy(), want["Lc"]), f"frame {k}: Q"
        pf.set_weights(Q)
        est = pf.step()
        r = want["r"]
        assert np.array_equal(pf.last_ancestors.cpu().numpy(), r["anc"]), f"frame {k}: ancestors"
        assert np.array_equal(bits(pf.particles_soa.cpu().numpy()), bits(r["states"])), f"frame {k}: resampled rows"
        np.testing.assert_allclose(est, want["est"], rtol=1e-12)
        tx, ty = R.truth(k)
        dist.append(float(np.hypot(est[0] - tx, est[1] - ty)))
    print("device run, truth distance per frame:", [round(v, 2) for v in dist])
    assert len(dist) == 23 and max(dist) <= R.FOLLOW_BOUND_PX < 16.0


# ------------------------------------------------------------------ Tracker / MultiTracker (ViT-Ti, fp32)
P_T, BOX, SEED = 64, (80, 80, 64, 64), 99
T_ROT = {"rotation_std": 0.05, "rotation_range": [-1.0, 1.2]}
COLOR = {"bins": 8, "grid": 32, "lambda": 20.0}


def _cfg(color=COLOR, seed=SEED, alpha=0.0, rot=False, drop_key=False):
    from vitparticlefiltertracker_amd import load_config
    lk = {"template_update": alpha}
    if not drop_key:
        lk["color"] = color
    return load_config({"model": {"arch": "vit_tiny_patch16_224", "dtype": "fp32", "weights": {"seed": 3}},
                        "particles": {"num": P_T, "seed": seed, **(T_ROT if rot else {})}, "likelihood": lk})


def _rows(pf):
    return pf._state.cpu().numpy()


def _record(tr, est):
    return {"est": est, "state": _rows(tr.pf), "anc": tr.pf.last_ancestors.cpu().numpy().copy(),
            "ct": None if tr.color_template is None else tr.color_template.cpu().numpy().copy()}


def _same(a, b, tag):
    assert a["est"] == b["est"], tag
    assert np.array_equal(a["anc"], b["anc"]), f"{tag}: ancestors"
    assert np.array_equal(bits(a["state"]), bits(b["state"])), f"{tag}: state"


def _track_all(cfg, clip, n, use_graph=True):
    from vitparticlefiltertracker_amd import Tracker
    tr = Tracker(cfg, device=DEV, use_graph=use_graph)
    tr.init(clip[0], BOX)
    return [_record(tr, tr.track(f)) for f in clip[1:1 + n]]


@pytest.fixture(scope="module")
def tracked(tinted):
    """The uninterrupted six-frame run through track() with the colour cue (graph on, fixed templates)."""
    return _track_all(_cfg(), tinted, 6)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_tracker_weights_are_the_exact_product(tinted, tracked, use_graph):
    """Four frames step by step: tr.pf.Q is (Qvit Lc_ref) >> K exactly, with Qvit from a separate forward of the same
    predicted states without the cue and Lc_ref the reference's; ancestors and states follow the reference from that Q;
    and track() of the same frames agrees, with the graph and without it."""
    from vitparticlefiltertracker_amd import Tracker
    tr = Tracker(_cfg(), device=DEV, use_graph=use_graph)
    tr.init(tinted[0], BOX)
    t_ref = R.template(tinted[0], BOX, None, 32, 8)
    assert np.array_equal(bits(tr.color_template.cpu().numpy()), bits(t_ref)) and tr.color_template.shape == (512,)
    c = _cfg()["particles"]
    cx, cy = BOX[0] + 0.5 * BOX[2], BOX[1] + 0.5 * BOX[3]
    ref = R10.Filter(P_T, (cx, cy, 1.0), c["motion_std"], c["scale_range"], SEED, HW, K40, R10.SYSTEMATIC, None)
    for k, f in enumerate(tinted[1:5], start=1):
        tr._upload(f)
        tr.frame_index += 1
        tr.pf.predict(tr.frame_index)
        ref.predict(k)
        tr.weigh()
        Q = tr.pf.Q.cpu().numpy().copy()
        pred = tr.pf.particles_soa.cpu().numpy().copy()
        assert np.array_equal(bits(pred), bits(ref.particles)), f"frame {k}: predicted state"
        tr.engine.forward_weights(tr._frame_dev, tr.pf.particles_soa, tr.box_wh, tr.template, tr.lam, tr.bits)
        Qvit = tr.engine.Q[:P_T].cpu().numpy().copy()
        Lc = R.color_weights(f, pred, None, (64.0, 64.0), t_ref, 32, 8, 20.0, K40)
        assert Q.tolist() == R.combine(Qvit, Lc, K40), f"frame {k}: Q is not the exact product"
        assert not np.array_equal(Q, Qvit) and (Q <= Qvit).all()
        est = tr.pf.estimate()
        anc = tr.pf.resample().cpu().numpy()
        r = ref.update(Q)
        assert np.array_equal(anc, r["anc"]), f"frame {k}: ancestors"
        assert np.array_equal(bits(_rows(tr.pf)), bits(r["states"])), f"frame {k}: resampled state"
        np.testing.assert_allclose(est, R10.estimate(r, P_T), rtol=1e-12)
        _same(_record(tr, est), tracked[k - 1], f"frame {k} against track()")
    assert np.array_equal(bits(tr.color_template.cpu().numpy()), bits(t_ref)), "alpha = 0 changed the template"
    for rec in tracked:
        assert np.array_equal(bits(rec["ct"]), bits(t_ref)), "alpha = 0 changed the template"


def test_cue_uses_the_angle_row(tinted):
    """With rotation_std the cue takes S12's coordinates: Q is the exact product with the reference's rotated Lc, which
    differs from the unrotated call's on the same states."""
    from vitparticlefiltertracker_amd import Tracker
    tr = Tracker(_cfg(rot=True), device=DEV)
    tr.init(tinted[0], BOX, angle=0.2)
    t_ref = R.template(tinted[0], BOX, np.float32(0.2), 32, 8)
    assert np.array_equal(bits(tr.color_template.cpu().numpy()), bits(t_ref))
    assert not np.array_equal(t_ref, R.template(tinted[0], BOX, None, 32, 8))
    f = tinted[1]
    tr._upload(f)
    tr.frame_index += 1
    tr.pf.predict(tr.frame_index)
    tr.weigh()
    Q = tr.pf.Q.cpu().numpy().copy()
    pred, ang = tr.pf.particles_soa.cpu().numpy().copy(), tr.pf.rotation.cpu().numpy().copy()
    tr.engine.forward_weights(tr._frame_dev, tr.pf.particles_soa, tr.box_wh, tr.template, tr.lam, tr.bits,
                              angles=tr.pf.rotation_soa)
    Qvit = tr.engine.Q[:P_T].cpu().numpy().copy()
    Lc_rot = R.color_weights(f, pred, ang, (64.0, 64.0), t_ref, 32, 8, 20.0, K40)
    assert Q.tolist() == R.combine(Qvit, Lc_rot, K40)
    Qu = torch.empty(P_T, device=DEV, dtype=torch.int64)
    torch.ops.vpf.color_weight(None, tr.engine.rgba, False, tr.pf.particles_soa, None, [64.0, 64.0], list(HW), 32, 8,
                               tr.color_template, 20.0, K40, False, None, None, Qu)
    assert np.array_equal(Qu.cpu().numpy(), R.color_weights(f, pred, None, (64.0, 64.0), t_ref, 32, 8, 20.0, K40))
    assert not np.array_equal(Qu.cpu().numpy(), Lc_rot), "the cue ignored the angle row"
    est = tr.track(tinted[2])
    assert tr.last_rotation is not None and all(np.isfinite(est))


def test_multitracker_targets_equal_their_own_trackers(tinted):
    """Two targets, each with its own box, seed and histogram template, alpha = 0.25 so both templates move too: every
    frame's estimates, rows, ancestors and colour templates are the two single trackers', and a checkpoint resumes."""
    from vitparticlefiltertracker_amd import MultiTracker, Tracker
    boxes = [BOX, (60, 70, 48, 56)]
    mt = MultiTracker(_cfg(alpha=0.25), n_objects=2, device=DEV)
    mt.init(tinted[0], boxes)
    trs = [Tracker(_cfg(alpha=0.25, seed=SEED + k), device=DEV) for k in range(2)]
    for tr, bx in zip(trs, boxes):
        tr.init(tinted[0], bx)
    assert not torch.equal(mt.color_templates[0], mt.color_templates[1])
    assert mt.color_template is mt.color_templates and len(mt.color_template) == 2
    for i, f in enumerate(tinted[1:4], start=1):
        ests = mt.track(f)
        for k, tr in enumerate(trs):
            assert tr.track(f) == ests[k], f"frame {i} target {k}"
            assert np.array_equal(bits(_rows(mt.pfs[k])), bits(_rows(tr.pf))), f"frame {i} target {k}"
            assert torch.equal(mt.pfs[k].last_ancestors, tr.pf.last_ancestors)
            assert torch.equal(mt.color_templates[k].view(torch.int32), tr.color_template.view(torch.int32))
    sd = mt.state_dict()
    assert sd["color_template"].shape == (2, 512)
    mt2 = MultiTracker(_cfg(alpha=0.25), n_objects=2, device=DEV)
    mt2.load_state_dict(sd)
    assert mt2.track(tinted[4]) == mt.track(tinted[4])
    for a, b in zip(mt.color_templates, mt2.color_templates):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError):
        MultiTracker(_cfg(color=None, alpha=0.25), n_objects=2, device=DEV).load_state_dict(sd)


def test_template_update_follows_the_three_operation_rule(tinted):
    """alpha = 0.25: after every frame color_template is fp32(fp32(0.75) t) + fp32(fp32(0.25) p), p the histogram of the
    estimate's box (fp32 of the fp64 estimate) on that frame, bit for bit, with no renormalisation."""
    from vitparticlefiltertracker_amd import Tracker
    tr = Tracker(_cfg(alpha=0.25), device=DEV)
    tr.init(tinted[0], BOX)
    t = R.template(tinted[0], BOX, None, 32, 8)
    for k, f in enumerate(tinted[1:4], start=1):
        est = tr.track(f)
        st = np.array([[est[0]], [est[1]], [est[2]]], np.float32)
        p = R.normalised(R.histograms(f, st, None, (64.0, 64.0), 32, 8), 32)[0]
        t = R.blend(t, p, 0.25)
        assert np.array_equal(bits(tr.color_template.cpu().numpy()), bits(t)), f"frame {k}"
    assert abs(float(t.sum()) - 1.0) < 1e-5 and not np.array_equal(t, R.template(tinted[0], BOX, None, 32, 8))


# ------------------------------------------------------------------ checkpoints
FINGERPRINT_KEYS = {"arch", "dtype", "weights_seed", "weights_crc32", "mean", "std", "P", "motion_std", "scale_range",
                    "seed", "lambda", "weight_bits", "template_update", "rank", "world_size"}
STATE_KEYS = {"format", "frame_index", "pf_frame", "particles_soa", "template", "box_wh", "frame_hw", "config"}


def test_checkpoint_resumes_bit_exact_and_the_kinds_refuse_each_other(tmp_path, tinted):
    from vitparticlefiltertracker_amd import Tracker
    a = Tracker(_cfg(alpha=0.25), device=DEV)
    a.init(tinted[0], BOX)
    for f in tinted[1:3]:
        a.track(f)
    path = a.save_checkpoint(str(tmp_path / "colour"))
    with np.load(path) as z:
        assert set(z.files) == STATE_KEYS | {"color_template"} and z["color_template"].shape == (512,)
        assert np.array_equal(bits(z["color_template"]), bits(a.color_template.cpu().numpy()))
    assert set(a.config_fingerprint()) == FINGERPRINT_KEYS | {"color"} and a.config_fingerprint()["color"] == COLOR
    b = Tracker(_cfg(alpha=0.25), device=DEV)
    b.load_checkpoint(path)
    assert b.frame_index == 2
    for i, f in enumerate(tinted[3:5], start=3):
        ea, eb = a.track(f), b.track(f)
        _same(_record(a, ea), _record(b, eb), f"frame {i} after resume")
        assert torch.equal(a.color_template.view(torch.int32), b.color_template.view(torch.int32))
    d = Tracker(_cfg(color=None, alpha=0.25), device=DEV)
    for other in (d, Tracker(_cfg(color={"grid": 16}, alpha=0.25), device=DEV)):
        with pytest.raises(ValueError):
            other.load_checkpoint(path)
    d.init(tinted[0], BOX)
    d.track(tinted[1])
    dpath = d.save_checkpoint(str(tmp_path / "plain"))
    with pytest.raises(ValueError):
        Tracker(_cfg(alpha=0.25), device=DEV).load_checkpoint(dpath)


# ------------------------------------------------------------------ the default path
def test_default_path_is_untouched(tinted):
    """`color: null` equals a configuration without the key: state-dict keys, fingerprint, and four frames of Q,
    ancestors and states; its engine timer shows no color_weight launch (the colour tracker's shows one per frame, next
    to crop_patches)."""
    from vitparticlefiltertracker_amd import Tracker
    from vitparticlefiltertracker_amd.vit import KernelTimer
    runs = []
    for cfg in (_cfg(color=None), _cfg(drop_key=True)):
        tr = Tracker(cfg, device=DEV)
        tr.init(tinted[0], BOX)
        assert tr.color is None and tr.color_template is None
        rec = []
        for f in tinted[1:5]:
            tr._upload(f)
            tr.frame_index += 1
            tr.pf.predict(tr.frame_index)
            tr.weigh()
            Q = tr.pf.Q.cpu().numpy().copy()
            est = tr.pf.step()
            rec.append({**_record(tr, est), "Q": Q})
        assert set(tr.state_dict()) == STATE_KEYS and set(tr.config_fingerprint()) == FINGERPRINT_KEYS
        runs.append((rec, tr.config_fingerprint(), tr))
    assert runs[0][1] == runs[1][1]
    for k, (x, y) in enumerate(zip(runs[0][0], runs[1][0]), start=1):
        _same(x, y, f"frame {k}")
        assert np.array_equal(x["Q"], y["Q"])
    for color, want in ((None, 0), (COLOR, 1)):
        tr = Tracker(_cfg(color=color), device=DEV, use_graph=False)
        tr.init(tinted[0], BOX)
        tr.engine.timer = KernelTimer()
        tr.track(tinted[1])
        s = tr.engine.timer.summary()
        tr.engine.timer = None
        assert s["crop_patches"]["launches"] == 1 and s["cls_weight"]["launches"] == 1
        assert s.get("color_weight", {"launches": 0})["launches"] == want, sorted(s)
