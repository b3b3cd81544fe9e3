"""CPU: SPEC S17 (mode estimate) — the `estimate` key and every rejection, `estimate: null` leaving the configuration, the
fingerprint and main.py's output as they were, the window helper, the reference's own properties (tests/s17_reference.py:
the density does not depend on the order of j, a bimodal cloud's mean lies outside both windows while the mode lies
inside the heavier one, the window's edge, ties, non-finite states), what _read_estimate() makes of the statistics, and
the measured constants of the twin run."""
import copy
import types

import numpy as np
import pytest

import s15_reference as R15
import s17_reference as R
from vitparticlefiltertracker_amd import config as C

f32 = np.float32
ARCH = "vit_base_patch16_224"


# ------------------------------------------------------------------ configuration
def test_config_default_is_null_and_null_changes_nothing():
    base = C.load_config()
    assert base["estimate"] is None and C.DEFAULTS["estimate"] is None
    for same in ({"estimate": None}, {"estimate": {}}, {"estimate": {"method": "mean"}},
                 {"estimate": {"method": "mean", "window": 0.25}}):
        assert C.load_config(same) == base, same
    rest = copy.deepcopy(base)
    del rest["estimate"]
    on = C.load_config({"estimate": {"method": "mode"}})
    assert on.pop("estimate") == {"method": "mode", "window": 0.5} and on == rest


def test_config_mapping_gets_its_defaults_and_combines_with_everything():
    got = C.load_config({"estimate": {"method": "mode", "window": 1}})["estimate"]
    assert got == {"method": "mode", "window": 1.0} and isinstance(got["window"], float)
    assert C.check_estimate({"method": "mode"}) == {"method": "mode", "window": R.DEFAULTS["window"]}
    assert C.ESTIMATE_DEFAULTS == R.DEFAULTS
    cfg = C.load_config({"estimate": {"method": "mode", "window": 0.75},
                         "likelihood": {"occlusion": {}, "redetect": {}, "color": {}, "color_surround": {},
                                        "template_update": 0.3},
                         "resample": {"method": "stratified"},
                         "particles": {"motion_model": "constant_velocity", "rotation_std": 0.05}})
    assert cfg["estimate"]["window"] == 0.75
    assert C.load_config({"estimate": {"method": "mode"}, "resample": {"ess_threshold": 0.5}})["estimate"] is not None


@pytest.mark.parametrize("bad", [{"method": "median"}, {"method": None}, {"method": True}, {"method": 1},
                                 {"window": 0}, {"window": 0.0}, {"window": -0.5}, {"window": True},
                                 {"window": float("nan")}, {"window": float("inf")}, {"window": "0.5"}, {"window": None},
                                 {"windw": 0.5}, {"method": "mode", "iterations": 3}, 3, [0.5], "mode", True])
def test_config_rejects_anything_else(bad):
    with pytest.raises(ValueError):
        C.load_config({"estimate": bad})


def test_window_is_one_fp32_rounding_of_the_fp64_product():
    assert C.estimate_window(None, (64.0, 64.0)) is None
    assert C.estimate_window({"method": "mode", "window": 0.5}, (64, 48)) == (32.0, 24.0)
    for omega, box in ((0.1, (63.0, 17.5)), (1.0 / 3.0, (100.0, 7.0)), (2.5, (1e-3, 1e4))):
        got = C.estimate_window({"method": "mode", "window": omega}, box)
        want = R.window(omega, box)
        assert got == (float(want[0]), float(want[1])) and all(v == float(f32(v)) for v in got)
        assert got[0] == float(f32(omega * box[0]))


# ------------------------------------------------------------------ fingerprint, state dict, main.py
def test_fingerprint_gains_the_key_only_when_it_is_set_and_the_two_kinds_refuse_each_other():
    import json
    from vitparticlefiltertracker_amd import tracker as T
    base = T._fingerprint(C.load_config(), ARCH, "00000000", 0, 1)
    assert "estimate" not in base
    for same in ({"estimate": None}, {"estimate": {}}, {"estimate": {"method": "mean", "window": 2.0}}):
        assert T._fingerprint(C.load_config(same), ARCH, "00000000", 0, 1) == base
    legacy = C.load_config()
    del legacy["estimate"]                      # a configuration dict from before the key existed
    assert T._fingerprint(legacy, ARCH, "00000000", 0, 1) == base
    on = T._fingerprint(C.load_config({"estimate": {"method": "mode"}}), ARCH, "00000000", 0, 1)
    assert set(on) - set(base) == {"estimate"} and on["estimate"] == {"method": "mode", "window": 0.5}
    assert {k: on[k] for k in base} == base
    wide = T._fingerprint(C.load_config({"estimate": {"method": "mode", "window": 0.75}}), ARCH, "00000000", 0, 1)
    assert "mode_window" not in T._resample_args(C.load_config({"estimate": {"method": "mode"}}))

    def sd(fp):
        return {"format": np.int64(T.CHECKPOINT_FORMAT), "config": np.array(json.dumps(fp, sort_keys=True))}
    T._check_fingerprint(sd(on), on)
    T._check_fingerprint(sd(base), base)
    for saved, mine in ((on, base), (base, on), (on, wide)):
        with pytest.raises(ValueError, match="estimate"):
            T._check_fingerprint(sd(saved), mine)


def test_state_dict_has_no_new_key():
    import torch
    from vitparticlefiltertracker_amd import tracker as T
    pf = types.SimpleNamespace(frame=2, particles_soa=torch.zeros(3, 4), height=8, width=8, ess_threshold=None,
                               velocity_soa=None, rotation_soa=None, held_frames=0, anchor=None)
    keys = None
    for est in (None, {"method": "mode", "window": 0.5}):
        stub = types.SimpleNamespace(pf=pf, frame_index=2, template=torch.zeros(4), box_wh=(4.0, 4.0), color=None,
                                     color_template=None, occlusion=None, redetect=None, estimate=est,
                                     config_fingerprint=lambda: {})
        got = set(T.Tracker.state_dict(stub))
        assert keys is None or got == keys
        keys = got


def test_main_output_gains_the_mode_fields_only_with_the_flag():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "vpf_main", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "main.py"))
    main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(main)
    assert main._mode_record(0.5, (1.0, 2.0, 1.25)) == {"mode_mass": 0.5, "mean_x": 1.0, "mean_y": 2.0,
                                                        "mean_scale": 1.25}
    assert main._mode_record(None, None) == {"mode_mass": None, "mean_x": None, "mean_y": None, "mean_scale": None}
    assert main._mode_text(0.5, (100.0, 20.5, 1.25)) == "  mass=0.5000  mean_x=  100.00  mean_y=   20.50  mean_scale= 1.250"
    assert "n/a" in main._mode_text(None, None)


# ------------------------------------------------------------------ the reference's own properties
def _cloud(P, seed=0, span=200.0):
    rng = np.random.default_rng(seed)
    st = np.empty((3, P), np.float32)
    st[:2] = rng.uniform(0.0, span, (2, P))
    st[2] = rng.uniform(0.6, 1.8, P)
    Q = rng.integers(0, 1 << 40, P, dtype=np.int64)
    return Q, st


def test_density_is_invariant_under_a_permutation_of_j():
    Q, st = _cloud(300)
    hx, hy = f32(20.0), f32(12.5)
    D = R.density(Q, st[0], st[1], hx, hy)
    brute = [sum(int(Q[j]) for j in range(300) if abs(f32(st[0, i] - st[0, j])) <= hx
                 and abs(f32(st[1, i] - st[1, j])) <= hy) for i in range(300)]
    assert D.tolist() == brute
    perm = np.random.default_rng(1).permutation(300)
    Dp = R.density(Q[perm], st[0][perm], st[1][perm], hx, hy)
    assert np.array_equal(Dp, D[perm])
    # the seeds unchanged, only the order the j are added in: the same integers
    for i in (0, 17, 299):
        m = R.in_window(st[0, i], st[1, i], st[0][perm], st[1][perm], hx, hy)
        assert sum(int(q) for q, k in zip(Q[perm], m) if k) == int(D[i])


def test_bimodal_mean_lies_outside_both_windows_and_the_mode_inside_the_heavier():
    rng = np.random.default_rng(3)
    P, hx, hy = 400, f32(32.0), f32(32.0)
    a, b = (100.0, 120.0), (340.0, 300.0)
    st = np.empty((3, P), np.float32)
    st[0] = np.where(np.arange(P) % 2 == 0, a[0], b[0]) + rng.normal(0, 4, P)
    st[1] = np.where(np.arange(P) % 2 == 0, a[1], b[1]) + rng.normal(0, 4, P)
    st[2] = 1.0
    Q = np.where(np.arange(P) % 2 == 0, 2 << 30, 3 << 30).astype(np.int64)       # the cluster at b is the heavier
    T = int(Q.sum())
    mean = tuple(s / float(T) for s in R15.tree_sums(Q, st))
    for c in (a, b):
        assert abs(mean[0] - c[0]) > 2 * hx and abs(mean[1] - c[1]) > 2 * hy
    r = R.mode(Q, st, hx, hy, False)
    assert r["i"] % 2 == 1 and abs(r["est"][0] - b[0]) <= hx and abs(r["est"][1] - b[1]) <= hy
    assert np.hypot(r["est"][0] - b[0], r["est"][1] - b[1]) < 2.0
    assert 0.55 < r["Tm"] / T <= 0.6 + 1e-12                                   # 3 / 5 of the posterior at the most
    # with every weight 1 the clusters tie in count: the smallest index wins, which is in the cluster at a
    u = R.mode(Q, st, hx, hy, True)
    assert u["Tm"] == int(u["D"].max()) and u["i"] == int(np.flatnonzero(u["D"] == u["D"].max())[0])


def test_window_edge_is_inclusive_one_ulp_beyond_is_out_and_zero_counts_coincident_only():
    hx = f32(8.0)
    x = np.array([100.0, 108.0, np.nextafter(f32(108.0), f32(200.0)), 100.0, 92.0], np.float32)
    y = np.full(5, 50.0, np.float32)
    Q = [1, 10, 100, 1000, 10000]
    D = R.density(Q, x, y, hx, f32(0.0))
    assert D.tolist() == [11011, 1111, 110, 11011, 11001]
    assert R.density(Q, x, y, f32(0.0), f32(0.0)).tolist() == [1001, 10, 100, 1001, 10000]


def test_ties_take_the_smallest_index_and_non_finite_states_are_in_no_window():
    st = np.array([[5.0, 5.0, 70.0, 70.0], [5.0, 5.0, 9.0, 9.0], [1.0, 1.0, 1.0, 1.0]], np.float32)
    r = R.mode([3, 3, 3, 3], st, f32(1.0), f32(1.0), False)
    assert r["D"].tolist() == [6, 6, 6, 6] and r["i"] == 0 and r["Tm"] == 6 and r["est"] == (5.0, 5.0, 1.0)
    bad = st.copy()
    bad[0, 0], bad[1, 1] = np.nan, np.inf
    r = R.mode([3, 3, 3, 3], bad, f32(1.0), f32(1.0), False)
    assert r["D"].tolist() == [0, 0, 6, 6] and r["i"] == 2 and r["est"] == (70.0, 9.0, 1.0)
    bad[0, 2:] = -np.inf
    r = R.mode([3, 3, 3, 3], bad, f32(1.0), f32(1.0), False)
    assert not r["D"].any() and r["i"] == 0 and r["Tm"] == 0 and r["est"] is None
    assert R.out_words(r).tolist() == [0] * 8


def test_out_words_layout():
    Q, st = _cloud(70, seed=5)
    full = np.vstack([st, st[:2] * f32(0.01)])
    r = R.mode(Q, full, f32(30.0), f32(30.0), False)
    o = R.out_words(r)
    assert o[0] == r["i"] and o[1] == r["Tm"] and len(r["sums"]) == 5 and o[7] == 0
    assert o[2:7].view(np.float64).tolist() == r["sums"]


# ------------------------------------------------------------------ what _read_estimate makes of the statistics
class _NoWait:
    def synchronize(self):
        pass


def _fake_filter(P=16, extra=0, cv=False, rot=False, window=(8.0, 8.0)):
    import torch
    from vitparticlefiltertracker_amd.particle_filter import ParticleFilter
    f = ParticleFilter.__new__(ParticleFilter)
    f.P, f.bits, f._gate, f._adaptive, f._extra, f._cv, f._rot, f._vstats = P, 40, False, False, extra, cv, rot, 4
    f.redetect, f.mode_window = None, window
    f._mstats = 4 + (4 if extra else 0)
    f._stats_pin, f._stats_evt = torch.zeros(f._mstats + 8, dtype=torch.int64), _NoWait()
    f._est = f._mean = f._mode_index = f._mode_mass = f._vel = f._ang = None
    return f


def test_read_estimate_returns_the_mode_and_keeps_the_mean():
    import torch
    f = _fake_filter(extra=3, cv=True, rot=True)
    T, Tm = 1 << 20, 3 << 18
    f._stats_pin[0] = T
    f._stats_pin[1:4] = torch.tensor([v * T for v in (100.0, 80.0, 1.5)], dtype=torch.float64).view(torch.int64)
    f._stats_pin[5:8] = torch.tensor([v * T for v in (2.0, -1.0, 0.25)], dtype=torch.float64).view(torch.int64)
    f._stats_pin[8], f._stats_pin[9] = 11, Tm
    f._stats_pin[10:16] = torch.tensor([v * Tm for v in (40.0, 30.0, 1.25, 4.0, -3.0, 0.5)],
                                       dtype=torch.float64).view(torch.int64)
    assert f._read_estimate() == (40.0, 30.0, 1.25)
    assert f.last_mean == (100.0, 80.0, 1.5) and f.last_mode_index == 11 and f.last_mode_mass == 0.75
    assert f.last_velocity == (4.0, -3.0) and f.last_rotation == 0.5
    # Tm == 0: every state non-finite; S6's mean (whatever it holds) is what remains
    f._est = None
    f._stats_pin[9] = 0
    assert f._read_estimate() == (100.0, 80.0, 1.5) == f.last_mean
    assert f.last_mode_mass == 0.0 and f.last_velocity == (2.0, -1.0) and f.last_rotation == 0.25
    # T == 0: the weights count as 1 and the mass is Tm / P
    f._est = None
    f._stats_pin[0], f._stats_pin[9] = 0, 4
    f._stats_pin[10:13] = torch.tensor([160.0, 120.0, 5.0], dtype=torch.float64).view(torch.int64)
    assert f._read_estimate() == (40.0, 30.0, 1.25) and f.last_mode_mass == 0.25


def test_without_the_window_the_outputs_are_none_and_the_window_is_checked():
    from vitparticlefiltertracker_amd.particle_filter import ParticleFilter
    f = _fake_filter(window=None)
    f._stats_pin[0] = 4
    f._read_estimate()
    assert f.last_mean is None and f.last_mode_index is None and f.last_mode_mass is None
    g = ParticleFilter.__new__(ParticleFilter)
    g.mode_window = None
    for bad in ((1.0,), (1.0, -1.0), (float("nan"), 1.0), (1.0, float("inf")), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="mode_window"):
            g.set_mode_window(bad)
    g.set_mode_window((0.1, 0.0))
    assert g.mode_window == (float(f32(0.1)), 0.0)


# ------------------------------------------------------------------ the behaviour run's constants
def test_twin_run_constants():
    import s13_reference as R13
    import s16_reference as R16
    hx, hy = R.window(R.OMEGA, R13.FOLLOW["box"][2:])
    assert (hx, hy) == (32.0, 32.0)
    assert R.MODE_BOUND_PX == 1.5 * 2.75 < 0.25 * 64 and R.MODE_BOUND_PX < min(hx, hy)
    assert min(R.MEAN_NEAREST_PX.values()) > 2 * max(hx, hy)
    clip = R.twin_clip()
    base = R16.jump_clip()
    assert np.array_equal(clip[:R16.REAPPEAR], base[:R16.REAPPEAR])
    bx, by, bw, bh = R13.FOLLOW["box"]
    for k in (R16.REAPPEAR, R16.FRAMES - 1):
        (ax, ay), (tx, ty) = R.copies(k)
        assert np.hypot(ax - tx, ay - ty) >= 200.0
        twin = clip[k, int(ty) - bh // 2:int(ty) + bh // 2, int(tx) - bw // 2:int(tx) + bw // 2]
        real = clip[k, int(ay) - bh // 2:int(ay) + bh // 2, int(ax) - bw // 2:int(ax) + bw // 2]
        assert np.array_equal(twin, real) and np.array_equal(twin, clip[0, by:by + bh, bx:bx + bw])
        changed = np.any(clip[k] != base[k], axis=2)
        assert changed.sum() > 0 and not changed[:int(ty) - bh // 2].any() and not changed[int(ty) + bh // 2:].any()
