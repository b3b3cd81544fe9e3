"""CPU: SPEC S15 (occlusion gate) — the configuration key and every rejection, the fingerprint and state dict at the
default, that the reference of the GPU tests (tests/s15_reference.py) means something (gate_q, the step on both sides of
the boundary, the held step, the device-order sums), and the behaviour: the gated reference recursion HOLDS through the
occluded frames and comes back, while today's recursion with the same template update is lost."""
import math
import types

import numpy as np
import pytest

import s10_reference as R10
import s13_reference as R13
import s15_reference as R
from vitparticlefiltertracker_amd import config as C

K40 = 40


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ configuration
def test_config_default_is_null_and_a_mapping_gets_its_defaults():
    assert C.load_config()["likelihood"]["occlusion"] is None
    assert C.load_config({"likelihood": {"occlusion": None}})["likelihood"]["occlusion"] is None
    assert C.load_config({"likelihood": {"occlusion": {}}})["likelihood"]["occlusion"] == R.DEFAULTS
    got = C.load_config({"likelihood": {"occlusion": {"threshold": 1, "noise_gain": 1, "max_hold": 0}}})
    got = got["likelihood"]["occlusion"]
    assert got == {"threshold": 1.0, "noise_gain": 1.0, "max_hold": 0}
    assert isinstance(got["threshold"], float) and isinstance(got["noise_gain"], float) and type(got["max_hold"]) is int
    ok = C.load_config({"likelihood": {"occlusion": {"threshold": 0.2}}, "resample": {"method": "stratified"}})
    assert ok["likelihood"]["occlusion"]["threshold"] == 0.2


@pytest.mark.parametrize("bad", [{"threshold": 0.0}, {"threshold": -0.1}, {"threshold": 1.5}, {"threshold": True},
                                 {"threshold": float("nan")}, {"threshold": float("inf")}, {"threshold": "0.05"},
                                 {"threshold": None}, {"noise_gain": 0.5}, {"noise_gain": float("inf")},
                                 {"noise_gain": float("nan")}, {"noise_gain": True}, {"noise_gain": "2"},
                                 {"max_hold": -1}, {"max_hold": 2.0}, {"max_hold": True}, {"max_hold": "30"},
                                 {"treshold": 0.05}, {"threshold": 0.05, "relative": True}, 0.05, [0.05, 2.0], "on",
                                 True])
def test_config_rejects_anything_else(bad):
    with pytest.raises(ValueError):
        C.load_config({"likelihood": {"occlusion": bad}})


def test_config_rejects_the_gate_with_the_ess_gate():
    with pytest.raises(ValueError, match="ess_threshold"):
        C.load_config({"likelihood": {"occlusion": {}}, "resample": {"ess_threshold": 0.5}})
    assert C.load_config({"resample": {"ess_threshold": 0.5}})["likelihood"]["occlusion"] is None


def test_fingerprint_and_state_dict_have_no_new_key_at_the_default():
    import torch
    from vitparticlefiltertracker_amd import tracker as T
    base = T._fingerprint(C.load_config(), "vit_base_patch16_224", "00000000", 0, 1)
    assert set(base) == {"arch", "dtype", "weights_seed", "weights_crc32", "mean", "std", "P", "motion_std",
                         "scale_range", "seed", "lambda", "weight_bits", "template_update", "rank", "world_size"}
    null = C.load_config({"likelihood": {"occlusion": None}})
    assert T._fingerprint(null, "vit_base_patch16_224", "00000000", 0, 1) == base
    occ = T._fingerprint(C.load_config({"likelihood": {"occlusion": {"max_hold": 3}}}), "vit_base_patch16_224",
                         "00000000", 0, 1)
    assert set(occ) - set(base) == {"occlusion"}
    assert occ["occlusion"] == {"threshold": 0.05, "noise_gain": 2.0, "max_hold": 3}
    assert {k: occ[k] for k in base} == base
    assert "occlusion_threshold" not in T._resample_args(C.load_config())
    args = T._resample_args(C.load_config({"likelihood": {"occlusion": {"max_hold": 3}}}))
    assert args["occlusion_threshold"] == 0.05 and args["occlusion_max_hold"] == 3

    def sd(occlusion):
        pf = types.SimpleNamespace(frame=2, particles_soa=torch.zeros(3, 4), height=8, width=8, ess_threshold=None,
                                   velocity_soa=None, rotation_soa=None, held_frames=4)
        stub = types.SimpleNamespace(pf=pf, frame_index=2, template=torch.zeros(4), box_wh=(4.0, 4.0), color=None,
                                     color_template=None, occlusion=occlusion, config_fingerprint=lambda: base)
        return T.Tracker.state_dict(stub)
    keys = {"format", "frame_index", "pf_frame", "particles_soa", "template", "box_wh", "frame_hw", "config"}
    assert set(sd(None)) == keys
    held = sd(R.DEFAULTS)
    assert set(held) == keys | {"held_frames"} and int(held["held_frames"]) == 4


# ------------------------------------------------------------------ the reference
def test_gate_q_is_the_exact_floor():
    from fractions import Fraction
    from vitparticlefiltertracker_amd.config import occlusion_gate_q
    for theta in (0.05, 1.0, 0.5, 1e-13, 0.3, 2.0 ** -40, 2.0 ** -41):
        for K in (0, 1, 40, 51, 61):
            q = R.gate_q(theta, K)
            assert isinstance(q, int) and q == occlusion_gate_q(theta, K)
            assert Fraction(q) <= Fraction(theta) * 2 ** K < Fraction(q + 1)
    assert R.gate_q(1.0, K40) == 1 << K40 and R.gate_q(2.0 ** -41, K40) == 0 and R.gate_q(0.05, K40) == 54975581388


def _case(P, seed, zero=False):
    rng = np.random.default_rng(seed)
    Q = np.zeros(P, np.int64) if zero else rng.integers(0, (1 << K40) + 1, P, dtype=np.int64)
    return Q, rng.uniform(0, 224, (3, P)).astype(np.float32)


@pytest.mark.parametrize("method", [R10.SYSTEMATIC, R10.STRATIFIED])
@pytest.mark.parametrize("zero", [False, True])
def test_step_without_a_gate_is_s10s_step(method, zero):
    """gate_q = 0 never holds: the result is s10_reference.step(tau = None)'s, on random and on all-zero weights (the
    uniform resample), and the device-order sums agree with its fsum sums to 1e-12."""
    Q, p = _case(300, 5, zero)
    got = R.step(Q, p, 77, 3, method, K40, 0)
    want = R10.step(Q, p, 77, 3, method, None, K40)
    assert got["held"] is False and got["resampled"] is True
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(got[k], v), k
        else:
            assert got[k] == v, k
    np.testing.assert_allclose(got["tree"], want["sums"], rtol=1e-12)
    np.testing.assert_allclose(R.estimate(got, 300), R10.estimate(want, 300), rtol=1e-12)


def test_held_step_returns_its_inputs_and_the_plain_tree_mean():
    Q, p = _case(1500, 6)
    Q >>= 20                                   # every weight far below the gate
    keep = p.copy()
    r = R.step(Q, p, 77, 3, R10.SYSTEMATIC, K40, R.gate_q(0.05, K40))
    assert r["held"] is True and r["resampled"] is False
    assert r["T"] == int(Q.sum()) and r["m"] == int(Q.max()) and r["ess"] == R10.ess(Q)
    assert np.array_equal(r["anc"], np.arange(1500)) and r["anc"].dtype == np.int32
    assert np.array_equal(bits(r["states"]), bits(keep)) and np.array_equal(bits(p), bits(keep))
    assert r["carry"].tolist() == [R10.identity(K40)] * 1500
    est = R.estimate(r, 1500)
    assert est == tuple(s / 1500.0 for s in R.tree_sums([1] * 1500, keep))
    np.testing.assert_allclose(est, keep.astype(np.float64).mean(axis=1), rtol=1e-12)
    # all-zero weights under a gate are held, not uniformly resampled
    z = R.step(np.zeros(64, np.int64), p[:, :64].copy(), 1, 1, R10.SYSTEMATIC, K40, 1)
    assert z["held"] is True and z["T"] == 0 and np.array_equal(z["anc"], np.arange(64))


def test_tree_sums_follow_the_lane_order():
    """On values whose fp64 sum depends on the order, tree_sums is the lane-then-halving order, not the index order."""
    P = 2050
    v = np.zeros((1, P), np.float32)
    v[0, 0], v[0, 1024], v[0, 2048] = 1.0, 2.0 ** -53, 2.0 ** -53       # lane 0's three terms: 2^40, 2^-13, 2^-13
    w = [1 << 40] * P
    assert R.tree_sums(w, v)[0] == 2.0 ** 40                            # (2^40 + 2^-13) + 2^-13: two ties to even
    assert math.fsum(float(1 << 40) * float(x) for x in v[0]) == 2.0 ** 40 + 2.0 ** -12
    rng = np.random.default_rng(2)
    x = rng.uniform(0, 224, (3, 5000)).astype(np.float32)
    q = rng.integers(0, 1 << 40, 5000)
    want = [math.fsum(float(a) * float(b) for a, b in zip(q, x[c])) for c in range(3)]
    np.testing.assert_allclose(R.tree_sums(q, x), want, rtol=1e-13)


def test_the_boundary_is_an_integer_comparison():
    Q, p = _case(100, 8)
    m = int(Q.max())
    at = R.step(Q, p, 5, 2, R10.SYSTEMATIC, K40, m)            # m == gate_q: not held
    below = R.step(Q, p, 5, 2, R10.SYSTEMATIC, K40, m + 1)     # m == gate_q - 1: held
    assert at["held"] is False and below["held"] is True and at["m"] == below["m"] == m
    assert not np.array_equal(at["anc"], below["anc"])


def test_filter_widens_only_the_predict_after_a_held_frame():
    from oracle import pf as opf
    std, rng_ = (3.0, 2.5, 0.03), (0.6, 1.8)
    f = R.Filter(50, (100.0, 90.0, 1.0), std, rng_, 9, (224, 224), K40, R10.SYSTEMATIC, 1000, 2.5)
    plain = np.empty((3, 50), np.float32)
    plain[0], plain[1], plain[2] = 100.0, 90.0, 1.0
    f.predict(1)
    opf.predict(plain, 0, 9, 1, std, 224, 224, rng_)
    assert np.array_equal(bits(f.particles), bits(plain))
    assert f.update(np.full(50, 999, np.int64))["held"] and f.held_frames == 1
    f.predict(2)
    wide = plain.copy()
    opf.predict(wide, 0, 9, 2, (7.5, 6.25, 0.03), 224, 224, rng_)
    opf.predict(plain, 0, 9, 2, std, 224, 224, rng_)
    assert np.array_equal(bits(f.particles), bits(wide)) and not np.array_equal(bits(wide[:2]), bits(plain[:2]))
    assert np.array_equal(bits(wide[2]), bits(plain[2]))            # the scale's sigma is not gained
    assert not f.update(np.full(50, 1000, np.int64))["held"] and f.held_frames == 0
    assert R.gained((0.1, 0.3, 0.02), 3.0) == (float(np.float32(0.1) * np.float32(3.0)),
                                               float(np.float32(0.3) * np.float32(3.0)), 0.02)


# ------------------------------------------------------------------ the behaviour run
@pytest.fixture(scope="module")
def runs():
    clip = R.occluded_clip()
    return clip, R.follow_occluded(clip), R.follow_occluded(clip, theta=None)


def test_occluder_hides_the_target_only_in_its_frames():
    from vitparticlefiltertracker_amd.frames import synthetic_clip
    clip, plain = R.occluded_clip(), synthetic_clip(R.FRAMES, target_range=R13.TINT)
    changed = [k for k in range(R.FRAMES) if not np.array_equal(clip[k], plain[k])]
    assert changed == list(R.OCCLUDED) == list(range(9, 16))
    k = 12
    tx, ty = (int(v) for v in R13.truth(k))
    diff = np.argwhere((clip[k] != plain[k]).any(axis=2))
    assert diff.min(axis=0).tolist()[0] >= ty - 40 and diff.max(axis=0).tolist()[0] < ty + 40
    assert diff.min(axis=0).tolist()[1] >= tx - 40 and diff.max(axis=0).tolist()[1] < tx + 40


def test_gate_holds_through_the_occluder_and_recovers(runs):
    """The gated reference run: held exactly in the occluded frames; the peak separates visible from hidden frames by
    more than 10 x on either side of theta; after the occluder the worst distance stays within 1.5 x the measured
    4.08 px (< 16 px, a quarter of the box); the control (no gate, the same alpha = 0.3) ends more than half a box away;
    the gated template still scores rho >= 0.9 against the init template (measured: 0.9991; the control's 0.3746)."""
    clip, gated, control = runs
    assert len(gated) == len(control) == R.FRAMES - 1
    held = [k for k, g in enumerate(gated, start=1) if g["held"]]
    print("gated  : dist", [round(g["dist"], 2) for g in gated])
    print("gated  : peak", [round(g["peak"], 4) for g in gated])
    print("control: dist", [round(g["dist"], 2) for g in control])
    print("control: peak", [round(g["peak"], 4) for g in control])
    assert held == list(R.OCCLUDED)
    assert not any(g["held"] for g in control)
    vis = min(g["peak"] for k, g in enumerate(gated, start=1) if k not in R.OCCLUDED)
    hid = max(g["peak"] for k, g in enumerate(gated, start=1) if k in R.OCCLUDED)
    print("min visible peak", vis, "max hidden peak", hid)
    assert vis >= 10 * R.THETA and R.THETA >= 10 * hid
    after = [g["dist"] for g in gated[R.OCCLUDED[-1]:]]
    assert len(after) == 16
    print("worst distance after the occluder", max(after), "control's last", control[-1]["dist"])
    assert R.GATED_BOUND_PX == 1.5 * R.GATED_WORST_PX < 16.0
    assert max(after) <= R.GATED_WORST_PX                 # the recorded measurement is this reference's
    assert max(after) <= R.GATED_BOUND_PX
    assert control[-1]["dist"] > 32.0
    # a held frame keeps the template's bits; a visible frame moves them
    for k in R.OCCLUDED:
        assert np.array_equal(bits(gated[k - 1]["t"]), bits(gated[k - 2]["t"])), k
    assert not np.array_equal(bits(gated[15]["t"]), bits(gated[14]["t"]))
    t0 = R13.template(clip[0], R13.FOLLOW["box"], None, 32, 8)
    h0 = np.round(t0 * 1024).astype(np.int64)[None]
    rho_g, rho_c = float(R13.rho(h0, gated[-1]["t"], 32)[0]), float(R13.rho(h0, control[-1]["t"], 32)[0])
    print("template rho against the init template: gated", rho_g, "control", rho_c)
    assert rho_g >= 0.9 and abs(rho_g - R.GATED_TEMPLATE_RHO) < 5e-4 and rho_c < 0.9


def test_frames_before_the_occluder_are_todays(runs):
    """Until the first held frame the gated run is the ungated one bit for bit (a frame that is not held writes what
    today's step writes), and the first eight frames never come near the gate."""
    _, gated, control = runs
    for k in range(8):
        assert gated[k]["est"] == control[k]["est"] and np.array_equal(gated[k]["r"]["anc"], control[k]["r"]["anc"])
        assert np.array_equal(bits(gated[k]["t"]), bits(control[k]["t"]))
