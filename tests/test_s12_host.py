"""CPU: SPEC S12 (rotated particle boxes) — that the reference of the GPU tests (tests/s12_reference.py) means something
(the quarter-turn identity, the reduction to S3 at a = 0, its single-rounding fmaf) and the host logic: the angle
predict's rules, the configuration keys, the fingerprint and state dict at the defaults, the spinning clip, the chunk."""
import ctypes
import math
import types

import numpy as np
import pytest

import s10_reference as R10
import s11_reference as R11
import s12_reference as R
from oracle import pf as opf
from vitparticlefiltertracker_amd import config as C

f32 = np.float32
HALF_PI = f32(math.pi / 2)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ the reference means something
def _frame(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


QUARTER = [((60.0, 50.0, 1.0), (40.0, 30.0)), ((64.5, 47.25, 1.37), (64.0, 48.0)), ((20.0, 80.0, 2.0), (64.0, 64.0))]


@pytest.mark.parametrize("state,box", QUARTER)
def test_quarter_turn_identity(state, box):
    """Frame F 96 x 128, G = rot90(F, -1): the crop of G at centre (H - yc, xc) with a = pi/2 is the unrotated (S3) crop
    of F at (xc, yc), within 0.05 raw units: the fixed sincos is within 2^-23 of (0, 1) there, four fp32 roundings of
    coordinates below 256 move a sample by < 1e-4 px and a bilinear value by at most 255 per px per axis. With
    a = -pi/2 the crops differ by more than 100 somewhere, which pins the sign. The largest box has a 64 px
    half-extent and leaves the frame, so the zero border takes part."""
    H, W, S = 96, 128, 32
    F = _frame(H, W)
    G = np.ascontiguousarray(np.rot90(F, -1))
    assert G.shape == (W, H, 3)
    xc, yc, sc = state
    c, s = R.sincos_angle(HALF_PI)
    assert abs(float(c)) <= 2.0 ** -23 and abs(1.0 - float(s)) <= 2.0 ** -23
    pf = np.array([[xc], [yc], [sc]], np.float32)
    pg = np.array([[H - yc], [xc], [sc]], np.float32)
    want = R.bilinear(F, *R.s3_coords(pf, box, S))[0]
    got = R.crop_raw(G, pg, np.array([HALF_PI]), box, S)[0]
    worst = float(np.abs(got - want).max())
    print(f"quarter turn {state} {box}: largest difference {worst:.3e}")
    assert worst <= 0.05
    other = R.crop_raw(G, pg, np.array([-HALF_PI]), box, S)[0]
    assert float(np.abs(other - want).max()) > 100.0


def test_zero_angle_reproduces_s3_coordinates():
    """a = 0: the sample coordinates are within 1e-5 px of SPEC S3's (not asserted bit-equal: S12 subtracts half the box
    from the offset, S3 from the centre, and the fixed sincos gives (1 - 2^-23, -4.2e-8) at u = 0, not (1, 0)).
    1e-5 px is less than one ulp (1.53e-5) of a coordinate in [128, 256), so that bound is asserted on states whose
    samples stay below 128 px (the quarter-turn test's frame is 96 x 128), where an ulp is at most 7.6e-6. The states
    that reach 256 px are held to what the arithmetic allows there: the two orders differ in 3 + 5 roundings of at most
    half an ulp (2^-16) each, 4 ulp in all, plus (|1 - c| + |s|) times the half-extent (at most 1.7e-7 * 64 px)."""
    S = 32
    c0, s0 = R.sincos_angle(0.0)
    assert abs(1.0 - float(c0)) <= 2.0 ** -23 and abs(float(s0)) <= 2.0 ** -24
    small = np.array([[60.0, 64.5, 20.0, 90.3], [50.0, 47.25, 80.0, 7.9], [1.0, 1.37, 1.1, 0.5]], np.float32)
    large = np.array([[160.0, 111.3, 200.7], [150.0, 190.2, 60.0], [1.37, 2.0, 0.77]], np.float32)
    for p, limit, bound in ((small, 128.0, 1e-5), (large, 256.0, 4 * 2.0 ** -16 + 1.7e-7 * 64)):
        for box in ((40.0, 30.0), (64.0, 48.0), (64.0, 64.0)):
            sx, sy = R.sample_coords(p, np.zeros(p.shape[1], np.float32), box, S)
            rx, ry = R.s3_coords(p, box, S)
            assert max(np.abs(sx).max(), np.abs(sy).max()) < limit
            worst = max(float(np.abs(sx - rx).max()), float(np.abs(sy - ry).max()))
            print(f"a = 0, box {box}, coordinates below {limit:.0f}: largest difference {worst:.3e} px")
            assert worst <= bound


def test_reference_fmaf_vec_is_libm_fmaf():
    """The crop's vectorised fmaf against libm's, on random operands and on sums that sit next to an fp32 rounding tie
    (where rounding to fp64 first and then to fp32 would round twice)."""
    rng = np.random.default_rng(5)
    a = rng.uniform(0, 255, 4000).astype(np.float32)
    b = np.full(4000, opf.norm_affine([0.5] * 3, [0.5] * 3)[0][0], np.float32)
    c = np.full(4000, -1.0, np.float32)
    a = np.concatenate([a, np.full(3, f32(1 + 2.0 ** -12)), rng.standard_normal(1000).astype(np.float32)])
    b = np.concatenate([b, np.full(3, f32(1 + 2.0 ** -12)), rng.standard_normal(1000).astype(np.float32)])
    c = np.concatenate([c, np.array([2.0 ** -60, -2.0 ** -60, 0.0], np.float32),
                        (rng.standard_normal(1000) * 1e-3).astype(np.float32)])
    want = np.array([R11.fmaf(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    got = R.fmaf_vec(a, b, c)
    assert np.array_equal(bits(got), bits(want))
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert not np.array_equal(bits(twice), bits(want))      # the set does hold double-rounding cases


# ------------------------------------------------------------------ the angle predict's rules
def test_predict_with_zero_std_leaves_the_bits():
    a = np.array([0.0, -0.3, 1.25, -1.5, 1.5], np.float32)
    b = a.copy()
    R.predict_angle(b, 7, 99, 3, 0.0, -1.5, 1.5)
    assert np.array_equal(bits(a), bits(b))


def test_angle_noise_is_its_own_draw():
    """n5 of counter (i, k, 0, 2) equals none of n0..n4 (counters (i, k, 0, 0) and (i, k, 0, 1)) for the same (i, k)."""
    for gi, frame, seed in [(0, 1, 1234), (5, 3, (1 << 40) + 77), (4095, 200, 2 ** 63 + 5)]:
        n5 = R.angle_noise(gi, frame, seed)
        assert np.isfinite(n5)
        assert all(bits(n5) != bits(v) for v in R11.noise(gi, frame, seed))


def test_both_clamps_fire():
    n, lo, hi = 64, -0.4, 0.9
    a = np.zeros(n, np.float32)
    a[::2], a[1::2] = lo, hi
    R.predict_angle(a, 0, 11, 1, 0.5, lo, hi)
    assert a.min() == f32(lo) and a.max() == f32(hi)
    assert (a == f32(lo)).sum() > 4 and (a == f32(hi)).sum() > 4 and ((a > f32(lo)) & (a < f32(hi))).sum() > 4


def test_reference_converges_on_a_peaked_likelihood():
    """The recursion of the GPU convergence test, on the CPU first: from a = 0 with sigma_a = 0.1 and the likelihood
    floor(2^40 exp(-(a - 0.6)^2 / (2 0.05^2))), 12 frames; the angle estimate ends within 0.1 rad of 0.6 — here with room
    to spare (0.03) for the seed the GPU test uses."""
    est = R.run_convergence(R.CONV_SEED)
    print(f"seed {R.CONV_SEED}: angle estimates {[round(v, 4) for v in est]}")
    assert abs(est[-1] - 0.6) < 0.03


# ------------------------------------------------------------------ configuration
def test_config_defaults_and_accepts_rotation(tmp_path):
    d = C.load_config()
    assert d["particles"]["rotation_std"] is None
    assert d["particles"]["rotation_range"] == [-math.pi / 2, math.pi / 2]
    assert d["input"]["angle0"] == 0.0 and d["input"]["angles"] is None
    p = tmp_path / "c.yaml"
    p.write_text("particles: {rotation_std: 0.05, rotation_range: [-1.0, 2.0]}\ninput: {angle0: 1.5}\n")
    d = C.load_config(str(p))
    assert d["particles"]["rotation_std"] == 0.05 and d["particles"]["rotation_range"] == [-1.0, 2.0]
    assert C.check_rotation(0, [-math.pi, math.pi]) == (0.0, [-math.pi, math.pi])
    assert C.check_rotation(None, "ignored") == (None, [-math.pi / 2, math.pi / 2])
    # without rotation_std the other keys are not read
    C.load_config({"particles": {"rotation_range": [5, 1]}, "input": {"angle0": 9.0}})
    C.load_config({"particles": {"rotation_std": 0.1}, "input": {"bboxes": [[1, 1, 8, 8], [2, 2, 8, 8]],
                                                                  "angles": [0.0, 0.2]}})


@pytest.mark.parametrize("part,inp", [
    ({"rotation_range": [-3.2, 1.0]}, {}), ({"rotation_range": [-1.0, 3.2]}, {}),      # outside +-pi
    ({"rotation_range": [0.5, 0.5]}, {}), ({"rotation_range": [1.0, -1.0]}, {}),       # amin >= amax
    ({"rotation_range": [0.0]}, {}), ({"rotation_range": [0.0, float("nan")]}, {}),
    ({"rotation_std": -0.1}, {}), ({"rotation_std": float("nan")}, {}), ({"rotation_std": float("inf")}, {}),
    ({"rotation_std": True}, {}), ({"rotation_std": "0.1"}, {}),
    ({}, {"angle0": 1.6}), ({"rotation_range": [0.1, 1.0]}, {}),                       # angle0 outside the range
    ({}, {"bboxes": [[1, 1, 8, 8]], "angles": [0.0, 0.1]}), ({}, {"bboxes": [[1, 1, 8, 8]], "angles": [2.0]}),
    ({}, {"angles": [0.0]}),
])
def test_config_rejects(part, inp):
    with pytest.raises(ValueError):
        C.load_config({"particles": {"rotation_std": 0.1, **part}, "input": inp})


def test_fingerprint_and_state_dict_have_no_new_key_at_the_defaults():
    import torch
    from vitparticlefiltertracker_amd import tracker as T
    base = T._fingerprint(C.load_config(), "vit_base_patch16_224", "00000000", 0, 1)
    assert set(base) == {"arch", "dtype", "weights_seed", "weights_crc32", "mean", "std", "P", "motion_std",
                         "scale_range", "seed", "lambda", "weight_bits", "template_update", "rank", "world_size"}
    rot = T._fingerprint(C.load_config({"particles": {"rotation_std": 0.05}}), "vit_base_patch16_224", "00000000", 0, 1)
    assert set(rot) - set(base) == {"rotation_std", "rotation_range"}
    assert rot["rotation_std"] == 0.05 and rot["rotation_range"] == [-math.pi / 2, math.pi / 2]
    assert {k: rot[k] for k in base} == base

    def sd(rotation_soa):
        pf = types.SimpleNamespace(frame=2, particles_soa=torch.zeros(3, 4), height=8, width=8, ess_threshold=None,
                                   velocity_soa=None, rotation_soa=rotation_soa)
        stub = types.SimpleNamespace(pf=pf, frame_index=2, template=torch.zeros(4), box_wh=(4.0, 4.0),
                                     config_fingerprint=lambda: base)
        return T.Tracker.state_dict(stub)
    keys = {"format", "frame_index", "pf_frame", "particles_soa", "template", "box_wh", "frame_hw", "config"}
    assert set(sd(None)) == keys
    with_row = sd(torch.full((1, 4), 0.25))
    assert set(with_row) == keys | {"rotation_soa"} and with_row["rotation_soa"].shape == (1, 4)


# ------------------------------------------------------------------ the spinning clip
def test_clip_without_spin_is_todays_bytes():
    from vitparticlefiltertracker_amd.frames import synthetic_clip, target_angle
    a, b = synthetic_clip(5), synthetic_clip(5, spin=0.0)
    assert a.tobytes() == b.tobytes()
    assert synthetic_clip(3, 64, 80, (10, 12, 16, 20), 3, (1, 2)).tobytes() == \
        synthetic_clip(3, 64, 80, (10, 12, 16, 20), 3, (1, 2), spin=0.0).tobytes()
    assert target_angle(4, 0.07) == pytest.approx(0.28) and target_angle(9, 0.0) == 0.0


def test_spinning_clip_turns_the_texture_with_s12s_sign():
    """Frame 0 of a spinning clip is the plain clip's; in frame t the target is the texture turned by spin * t about its
    box centre: the S12 crop of that frame at the true centre and angle gives the texture back (bilinear resampling twice:
    close, not equal), and the crop at the opposite angle does not."""
    from vitparticlefiltertracker_amd.frames import synthetic_clip, target_angle, target_box
    plain, spun = synthetic_clip(6), synthetic_clip(6, spin=0.1)
    assert np.array_equal(plain[0], spun[0]) and not np.array_equal(plain[5], spun[5])
    bg_mask = np.ones(plain.shape[1:3], bool)
    bg_mask[40:200, 40:200] = False
    assert np.array_equal(plain[5][bg_mask], spun[5][bg_mask])          # the background is untouched
    x, y, w, h = target_box(5)
    p = np.array([[x + 0.5 * w], [y + 0.5 * h], [1.0]], np.float32)
    tex = plain[5][y:y + h, x:x + w].astype(np.float32)
    ang = target_angle(5, 0.1)
    inner = (slice(8, -8), slice(8, -8))
    good = R.crop_raw(spun[5], p, np.array([ang], np.float32), (w, h), w)[0]
    bad = R.crop_raw(spun[5], p, np.array([-ang], np.float32), (w, h), w)[0]
    # white-noise texture resampled twice: the error of the right angle is a fraction of the wrong angle's
    e_good, e_bad = np.abs(good - tex)[inner].mean(), np.abs(bad - tex)[inner].mean()
    print(f"mean |crop - texture|: true angle {e_good:.2f}, opposite angle {e_bad:.2f}")
    assert e_good < 0.6 * e_bad


def test_box_corners_follow_the_sign():
    from vitparticlefiltertracker_amd.frames import box_corners, draw_quad
    c = box_corners((10, 20, 8, 4), math.pi / 2)            # centre (14, 22); +x turns to +y
    np.testing.assert_allclose(c, [(16, 18), (16, 26), (12, 26), (12, 18)], atol=1e-12)
    np.testing.assert_allclose(box_corners((10, 20, 8, 4)), [(10, 20), (18, 20), (18, 24), (10, 24)])
    img = draw_quad(np.zeros((40, 40, 3), np.uint8), box_corners((10, 10, 20, 10), 0.5), thickness=1)
    assert img[..., 0].any() and not img[..., 1].any() and img[0, 0, 0] == 0
    draw_quad(np.zeros((8, 8, 3), np.uint8), box_corners((-50, -50, 200, 200), 0.3))     # clipped, no error


# ------------------------------------------------------------------ the chunk
def test_chunk_words_for_four_and_six_rows():
    from vitparticlefiltertracker_amd.particle_filter import chunk_words, shard_views
    import torch
    assert chunk_words(10, 4) == 60 and chunk_words(11, 4) == 66          # 24 B per particle, already 8-B aligned
    assert chunk_words(10, 6) == 80 and chunk_words(11, 6) == 88          # 32 B per particle
    assert chunk_words(11, 3) == 56 and chunk_words(11, 5) == 78          # the odd-row chunks pad, as before
    for rows in (4, 6):
        Q, st = shard_views(torch.zeros(chunk_words(7, rows), dtype=torch.int32), 7, rows)
        assert Q.shape == (7,) and st.shape == (rows, 7)


def test_libvpf_exports_the_s12_entry_points():
    from vitparticlefiltertracker_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vpf_predict_angle", "vpf_crop_patches_rot_bf16", "vpf_crop_patches_rot_f32"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
