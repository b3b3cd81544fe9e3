"""CPU: SPEC S16 (re-detection) — the configuration key and every rejection, the fingerprint and state dict at the
default and with the key, the lattice helper against hand values, that the reference of the GPU tests
(tests/s16_reference.py) scatters what S16 promises (one particle per cell, disjoint ordered y-strata, every coordinate
inside the frame), and the streak logic: which frames search, what a held search frame returns, what ends the search."""
import types

import numpy as np
import pytest

import s16_reference as R
from vitparticlefiltertracker_amd import config as C

f32 = np.float32
K40 = 40


def _lk(redetect, occlusion="default", **more):
    lk = {"redetect": redetect, **more}
    if occlusion is not None:
        lk["occlusion"] = {} if occlusion == "default" else occlusion
    return {"likelihood": lk}


# ------------------------------------------------------------------ configuration
def test_config_default_is_null_and_a_mapping_gets_its_defaults():
    assert C.load_config()["likelihood"]["redetect"] is None
    assert C.load_config(_lk(None))["likelihood"]["redetect"] is None
    assert C.load_config(_lk(None, occlusion=None))["likelihood"]["redetect"] is None
    assert C.load_config(_lk({}))["likelihood"]["redetect"] == {"after": None, "threshold": None}
    got = C.load_config(_lk({"after": 1, "threshold": 1}))["likelihood"]["redetect"]
    assert got == {"after": 1, "threshold": 1.0} and type(got["after"]) is int and isinstance(got["threshold"], float)
    assert C.load_config(_lk({"after": None, "threshold": None}))["likelihood"]["redetect"] == \
        {"after": None, "threshold": None}
    assert C.load_config(_lk({"after": 40}))["likelihood"]["redetect"]["after"] == 40     # past max_hold is allowed


def test_config_allows_every_other_feature_beside_it():
    cfg = C.load_config({"likelihood": {"occlusion": {"threshold": 0.2}, "redetect": {"threshold": 0.1}, "color": {},
                                        "color_surround": {}},
                         "resample": {"method": "stratified"},
                         "particles": {"motion_model": "constant_velocity", "rotation_std": 0.05}})
    assert cfg["likelihood"]["redetect"] == {"after": None, "threshold": 0.1}
    assert C.load_config({**_lk({"after": 2}), "particles": {"motion_model": "random_walk"}})


@pytest.mark.parametrize("bad", [{"after": 0}, {"after": -1}, {"after": 2.0}, {"after": True}, {"after": "3"},
                                 {"threshold": 0.0}, {"threshold": -0.1}, {"threshold": 1.5}, {"threshold": True},
                                 {"threshold": float("nan")}, {"threshold": float("inf")}, {"threshold": "0.05"},
                                 {"afer": 3}, {"after": 3, "region": [0, 0, 10, 10]}, 3, [3, 0.05], "on", True])
def test_config_rejects_anything_else(bad):
    with pytest.raises(ValueError):
        C.load_config(_lk(bad))


def test_config_rejects_the_search_without_the_gate_and_with_the_ess_gate():
    with pytest.raises(ValueError, match="occlusion"):
        C.load_config(_lk({}, occlusion=None))
    with pytest.raises(ValueError, match="occlusion"):
        C.load_config(_lk({"after": 2}, occlusion=None))
    with pytest.raises(ValueError, match="ess_threshold"):
        C.load_config({**_lk({}), "resample": {"ess_threshold": 0.5}})
    assert C.check_redetect(None, None) is None
    with pytest.raises(ValueError):
        C.check_redetect({}, None)


def test_after_null_means_lost():
    occ = C.load_config(_lk({}, occlusion={"max_hold": 3}))["likelihood"]
    assert C.redetect_after(occ["redetect"], occ["occlusion"]) == 4 == R.search_after(None, 3)
    occ = C.load_config(_lk({"after": 2}, occlusion={"max_hold": 3}))["likelihood"]
    assert C.redetect_after(occ["redetect"], occ["occlusion"]) == 2 == R.search_after(2, 3)


# ------------------------------------------------------------------ fingerprint / state dict
def test_fingerprint_and_state_dict_gain_the_key_only_when_it_is_set():
    import torch
    from vitparticlefiltertracker_amd import tracker as T
    arch = "vit_base_patch16_224"
    gated = C.load_config(_lk(None, occlusion={"max_hold": 3}))
    base = T._fingerprint(gated, arch, "00000000", 0, 1)
    assert "redetect" not in base
    dropped = C.load_config({"likelihood": {"occlusion": {"max_hold": 3}}})       # the key not given at all
    assert T._fingerprint(dropped, arch, "00000000", 0, 1) == base
    assert "redetect" not in T._fingerprint(C.load_config(), arch, "00000000", 0, 1)
    assert "redetect" not in T._resample_args(gated) and "redetect" not in T._resample_args(C.load_config())
    on = C.load_config(_lk({"after": 2}, occlusion={"max_hold": 3}))
    fp = T._fingerprint(on, arch, "00000000", 0, 1)
    assert set(fp) - set(base) == {"redetect"} and fp["redetect"] == {"after": 2, "threshold": None}
    assert {k: fp[k] for k in base} == base
    empty = T._fingerprint(C.load_config(_lk({}, occlusion={"max_hold": 3})), arch, "00000000", 0, 1)
    assert empty["redetect"] == {"after": None, "threshold": None}
    assert T._resample_args(on)["redetect"] == {"after": 2, "threshold": None}

    def sd(redetect, fingerprint):
        pf = types.SimpleNamespace(frame=2, particles_soa=torch.zeros(3, 4), height=8, width=8, ess_threshold=None,
                                   velocity_soa=None, rotation_soa=None, held_frames=4, anchor=(1.5, 2.5, 1.25))
        stub = types.SimpleNamespace(pf=pf, frame_index=2, template=torch.zeros(4), box_wh=(4.0, 4.0), color=None,
                                     color_template=None, occlusion=on["likelihood"]["occlusion"], redetect=redetect,
                                     config_fingerprint=lambda: fingerprint)
        return T.Tracker.state_dict(stub)
    keys = {"format", "frame_index", "pf_frame", "particles_soa", "template", "box_wh", "frame_hw", "config",
            "held_frames"}
    plain, search = sd(None, base), sd(on["likelihood"]["redetect"], fp)
    assert set(plain) == keys and set(search) == keys | {"anchor"}
    assert search["anchor"].dtype == np.float64 and search["anchor"].tolist() == [1.5, 2.5, 1.25]
    # a checkpoint of either kind is refused by a tracker of the other, and by one with another `after`
    T._check_fingerprint(search, fp)
    T._check_fingerprint(plain, base)
    for saved, mine in ((search, base), (plain, fp), (search, empty)):
        with pytest.raises(ValueError, match="redetect"):
            T._check_fingerprint(saved, mine)


def test_confidence_output_gains_the_flags_only_with_the_key():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "vpf_main", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "main.py"))
    main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(main)
    assert main._conf_record(0.5, 0.25, False, False) == {"peak": 0.5, "evidence": 0.25, "held": False, "lost": False}
    assert main._conf_record(0.5, 0.25, True, False, (True, False)) == \
        {"peak": 0.5, "evidence": 0.25, "held": True, "lost": False, "searched": True, "reacquired": False}
    old = main._conf_text(0.5, 0.25, True, False)
    assert old == "  peak= 0.5000  evidence= 0.2500  held=1  lost=0"
    assert main._conf_text(0.5, 0.25, True, False, (True, False)) == old + "  searched=1  reacquired=0"
    off = types.SimpleNamespace(redetect=None)
    assert main._search_of(off) is None and main._search_of(off, 1) is None
    one = types.SimpleNamespace(redetect={}, last_searched=True, last_reacquired=True)
    many = types.SimpleNamespace(redetect={}, last_searched=[False, True], last_reacquired=[False, False])
    assert main._search_of(one) == (True, True) and main._search_of(many, 1) == (True, False)


# ------------------------------------------------------------------ the lattice
@pytest.mark.parametrize("P,W,H,gx", [(4096, 224, 224, 64), (8192, 1920, 1080, 121), (1, 224, 224, 1), (1, 37, 11, 2),
                                      (1000, 224, 224, 32), (7, 11, 37, 2), (1024, 11, 37, 18), (255, 37, 11, 30),
                                      (1 << 24, 224, 224, 4096)])
def test_redetect_lattice_against_hand_values(P, W, H, gx):
    """gx by hand: 4096 = 64^2; 8192 * 1920 / 1080 = 14563.6 and 120^2 = 14400 < 14563.6 <= 121^2 = 14641; P = 1 on a
    wide frame: 37 / 11 = 3.4 needs gx = 2; 31^2 = 961 < 1000 <= 32^2; W < H: 7 * 11 / 37 = 2.08 -> 2 (1 < 2.08 <= 4),
    1024 * 11 / 37 = 304.4 -> 18 (17^2 = 289 < 304.4 <= 324); 255 * 37 / 11 = 857.7 -> 30 (29^2 = 841 < 857.7 <= 900)."""
    got = C.redetect_lattice(P, W, H)
    assert got[0] == gx and gx * gx * H >= P * W and (gx == 1 or (gx - 1) ** 2 * H < P * W)
    assert type(got[0]) is int
    assert f32(got[1]) == f32(1.0) / f32(gx) and got[1] == float(f32(got[1]))
    assert f32(got[2]) == f32(1.0) / f32(P) and got[2] == float(f32(got[2]))
    ref = R.lattice(P, W, H) if P <= 8192 else (gx, f32(1.0) / f32(gx), f32(1.0) / f32(P))
    assert (ref[0], float(ref[1]), float(ref[2])) == got
    with pytest.raises(ValueError):
        C.redetect_lattice(0, W, H)


# ------------------------------------------------------------------ the reference scatter's own properties
@pytest.mark.parametrize("P,S", [(64, 224), (1024, 448), (4096, 224)])
def test_reference_scatter_puts_one_particle_in_every_cell(P, S):
    """P = gx gy on a square frame (gx = gy = sqrt P): every (x-stratum, band) cell holds exactly one particle, for
    three frames' draws. A cell is [c, c + 1) (S - 1) / gx by [b, b + 1) (S - 1) / gx, evaluated in fp64."""
    gx = R.lattice(P, S, S)[0]
    assert gx * gx == P
    for frame in (1, 12, 16):
        u0, u1 = R.draws(0, P, 1234, frame)
        x, y = R.cell_xy(np.arange(P), u0, u1, P, S, S)
        col = np.floor(x.astype(np.float64) * gx / (S - 1.0)).astype(np.int64)
        band = np.floor(y.astype(np.float64) * gx / (S - 1.0)).astype(np.int64)
        assert col.min() >= 0 and col.max() == gx - 1 and band.min() >= 0 and band.max() == gx - 1
        assert len(set(zip(col.tolist(), band.tolist()))) == P, f"frame {frame}: a cell holds two particles"
        assert np.array_equal(col, np.arange(P) % gx) and np.array_equal(band, np.arange(P) // gx)


@pytest.mark.parametrize("P,W,H", [(1, 224, 224), (7, 37, 11), (255, 224, 224), (257, 37, 11), (1000, 1920, 1080),
                                   (1000, 11, 37)])
def test_reference_scatter_y_strata_are_disjoint_and_in_order(P, W, H):
    """Any P: particle i's y lies in its own stratum [i, i + 1] (H - 1) / P (fp64 bounds), so the strata are disjoint
    and ordered; every run of gx consecutive particles takes each x-stratum once; everything is inside the frame. The
    bounds are the exact strata, with no slack for y's own fp32 rounding: these sizes and draws (seed 1234, frames 3 and
    16) meet them without exception. A draw within an ulp of a stratum's edge can round past it (seed 99, frame 3 at
    P = 255 does, by 5.5e-6 px); the order of the y's is kept even then, every operation being monotone."""
    gx = R.lattice(P, W, H)[0]
    i = np.arange(P)
    for frame in (3, 16):
        u0, u1 = R.draws(0, P, 1234, frame)
        x, y = R.cell_xy(i, u0, u1, P, W, H)
        yd, xd = y.astype(np.float64), x.astype(np.float64)
        assert np.all(yd >= i * (H - 1.0) / P) and np.all(yd <= (i + 1) * (H - 1.0) / P)
        assert np.all(np.diff(yd) >= 0.0)
        c = i % gx
        assert np.all(xd >= c * (W - 1.0) / gx) and np.all(xd <= (c + 1) * (W - 1.0) / gx)
        assert x.min() >= 0.0 and x.max() <= W - 1 and y.min() >= 0.0 and y.max() <= H - 1


@pytest.mark.parametrize("P,W,H", [(7, 37, 11), (255, 224, 224), (1000, 1920, 1080), (1000, 11, 37), (1 << 24, 224, 224),
                                   (3, 1, 1)])
def test_reference_scatter_stays_inside_the_frame_at_the_adversarial_draws(P, W, H):
    """u one ulp below 1 in the last column (c = gx - 1) and the last stratum (i = P - 1), and the smallest u in the
    first: x in [0, W - 1] and y in [0, H - 1] (the clamp carries it where the rounded products overshoot)."""
    gx = C.redetect_lattice(P, W, H)[0]
    top, low = np.nextafter(f32(1.0), f32(0.0)), f32(2.0 ** -24)
    idx = np.array([0, min(gx, P) - 1, ((P - gx) // gx) * gx + gx - 1 if P >= gx else P - 1, P - 1], np.int64)
    assert idx.max() == P - 1 and (P < gx or np.all(idx[1:3] % gx == gx - 1))
    for u in (top, low):
        uu = np.full(idx.shape, u, np.float32)
        if P <= 8192:
            x, y = R.cell_xy(idx, uu, uu, P, W, H)
        else:       # the reference's own lattice loop is for small P: the same arithmetic with the helper's gx
            inv_gx, inv_P = f32(1.0) / f32(gx), f32(1.0) / f32(P)
            wm1, hm1 = f32(W) - f32(1.0), f32(H) - f32(1.0)
            x = np.minimum(np.maximum((((idx % gx).astype(np.float32) + uu) * inv_gx) * wm1, f32(0.0)), wm1)
            y = np.minimum(np.maximum(((idx.astype(np.float32) + uu) * inv_P) * hm1, f32(0.0)), hm1)
        assert x.dtype == np.float32 and y.dtype == np.float32
        assert np.all((x >= 0.0) & (x <= f32(W) - f32(1.0))), (x, W)
        assert np.all((y >= 0.0) & (y <= f32(H) - f32(1.0))), (y, H)


def test_reference_search_predict_keeps_s2s_scale_row_and_zeroes_the_velocity():
    from oracle import pf as opf
    P, seed, frame = 300, 77, 9
    rng = np.random.default_rng(0)
    p = np.empty((5, P), np.float32)
    p[:2] = rng.uniform(0, 200, (2, P))
    p[2] = rng.uniform(0.6, 1.8, P)
    p[3:] = rng.normal(0, 3, (2, P))
    walk = np.ascontiguousarray(p[:3]).copy()
    opf.predict(walk, 0, seed, frame, (4.0, 4.0, 0.02), 224, 224, (0.5, 2.0))
    three = np.ascontiguousarray(p[:3]).copy()
    R.predict_search(p, 0, P, seed, frame, 0.02, 224, 224, (0.5, 2.0))
    R.predict_search(three, 0, P, seed, frame, 0.02, 224, 224, (0.5, 2.0))
    assert np.array_equal(p[2].view(np.uint32), walk[2].view(np.uint32))
    assert np.array_equal(p[:3].view(np.uint32), three.view(np.uint32))
    assert not p[3:].view(np.uint32).any()
    assert not np.array_equal(p[0], walk[0])
    shard = np.ascontiguousarray(walk[:, 100:180]).copy()
    R.predict_search(shard, 100, P, seed, frame + 1, 0.02, 224, 224, (0.5, 2.0))
    whole = walk.copy()
    R.predict_search(whole, 0, P, seed, frame + 1, 0.02, 224, 224, (0.5, 2.0))
    assert np.array_equal(shard.view(np.uint32), whole[:, 100:180].view(np.uint32))


# ------------------------------------------------------------------ the streak logic, with a fake filter
class _NoWait:
    def synchronize(self):
        pass


def _fake_filter(redetect, max_hold, P=16):
    """A ParticleFilter without a device: the attributes _read_estimate() reads, the statistics written by hand."""
    import torch
    from vitparticlefiltertracker_amd.particle_filter import ParticleFilter
    occ = C.check_occlusion({"max_hold": max_hold})
    f = ParticleFilter.__new__(ParticleFilter)
    f.P, f.bits, f._gate, f._adaptive, f._extra, f._cv, f._rot, f._vstats = P, K40, True, True, 0, False, False, 8
    f.occlusion_max_hold = max_hold
    f.redetect = C.check_redetect(redetect, occ)
    f.search_after = C.redetect_after(f.redetect, occ)
    f._stats_pin, f._stats_evt = torch.zeros(8, dtype=torch.int64), _NoWait()
    f.held_frames, f._searched, f._reacquired, f._est, f.anchor = 0, None, None, None, (50.0, 60.0, 1.0)
    return f


def _frame(f, T, search, held, state):
    """What predict + _settle leave behind for one frame: the search flag, and the 64-B statistics of a frame whose
    device sums are `state` times the divisor (T, or P when held)."""
    import torch
    f._searched, f._est = search, None
    d = float(f.P) if held or not T else float(T)
    f._stats_pin[0] = T
    f._stats_pin[1:4] = torch.tensor([v * d for v in state], dtype=torch.float64).view(torch.int64)
    f._stats_pin[4:5] = torch.tensor([1.0], dtype=torch.float64).view(torch.int64)
    f._stats_pin[5], f._stats_pin[6], f._stats_pin[7] = int(not held), 1 << 30, int(held)
    return f._read_estimate()


@pytest.mark.parametrize("redetect,max_hold,A", [({"after": 2}, 30, 2), ({}, 3, 4)])
def test_streak_decides_the_search_and_a_held_search_frame_returns_the_anchor(redetect, max_hold, A):
    """visible, then held frames until two search frames were held, then a search frame that is not held, then two
    ordinary frames. The frames that search are exactly those whose predict sees held_frames >= A (A = after, or
    max_hold + 1: the frames at whose predict `lost` is up); a held search frame returns the anchor, the last estimate
    returned by a frame that was not a search frame (a held ordinary frame's plain mean included), and the filter
    stays `lost`-consistent; the search frame that is not held returns its own estimate, sets last_reacquired, clears
    the streak, and the next predict is ordinary."""
    from vitparticlefiltertracker_amd.tracker import _search_frame
    f = _fake_filter(redetect, max_hold)
    assert f.search_after == A
    assert _search_frame(None, f) is False
    plan = ["visible"] + ["held"] * (A + 2) + ["visible", "visible", "held"]
    searched, expect_anchor = [], None
    for k, kind in enumerate(plan, start=1):
        search = _search_frame(f.redetect, f)
        assert search == (f.held_frames >= A)
        if redetect == {}:
            assert search == bool(f.lost)
        searched.append(search)
        held = kind == "held"
        state = (100.0 + k, 80.0 + k, 1.0 + k / 64.0)         # exact in fp64 after the multiply and the divide
        before = f.held_frames
        got = _frame(f, 1 << 20, search, held, state)
        assert f.last_searched is search and f.last_held is held and f.last_reacquired is (search and not held)
        if search and held:
            assert got == expect_anchor and got != state, f"frame {k}: a held search frame returns the anchor"
        else:
            assert got == state, f"frame {k}"
        if not search:
            expect_anchor = state
        assert f.anchor == expect_anchor
        assert f.held_frames == (before + 1 if held else 0)
        assert f._read_estimate() == got and f.held_frames == (before + 1 if held else 0)   # read once per frame
    first = 1 + A + 1          # frame 1 visible, A held frames, then the predict that sees the streak
    assert [k for k, s in enumerate(searched, start=1) if s] == [first, first + 1, first + 2]
    assert plan[first + 1] == "visible" and searched[first + 2:] == [False, False]
    assert f.held_frames == 1 and f.last_reacquired is False


def test_search_needs_the_key():
    from vitparticlefiltertracker_amd.particle_filter import ParticleFilter
    f = ParticleFilter.__new__(ParticleFilter)
    f.redetect = None
    with pytest.raises(ValueError, match="redetect"):
        f.predict(3, 1.0, search=True)
