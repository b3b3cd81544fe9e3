"""CPU: SPEC S11 (constant-velocity motion model) — the config keys, the shard-chunk layout with five state rows, the
Python reference (tests/s11_reference.py) against the S2 oracle and on a moving target, and the new entry points'
argument checks. No compute calls (no GPU here)."""
import math
import os

import numpy as np
import pytest
import torch

import s10_reference as R10
import s11_reference as R
from oracle import pf as opf
from vitparticlefiltertracker_amd import config as C


# ------------------------------------------------------------------ config
def test_config_defaults_and_accepts_the_model(tmp_path):
    p = C.load_config()["particles"]
    assert (p["motion_model"], p["velocity_std"], p["velocity_decay"], p["velocity_max"]) == \
        ("random_walk", [1.0, 1.0], 1.0, 64.0)
    p = C.load_config({"particles": {"motion_model": "constant_velocity", "velocity_std": [0.5, 0], "velocity_decay": 0,
                                     "velocity_max": 8}})["particles"]
    assert p["motion_model"] == "constant_velocity" and p["velocity_std"] == [0.5, 0]
    f = tmp_path / "c.yaml"
    f.write_text("particles: {motion_model: constant_velocity, velocity_std: [2.0, 3.0], velocity_decay: 0.9}\n")
    p = C.load_config(str(f))["particles"]
    assert p["velocity_std"] == [2.0, 3.0] and p["velocity_decay"] == 0.9 and p["velocity_max"] == 64.0
    # the three velocity_* keys are read only under constant_velocity
    C.load_config({"particles": {"velocity_max": -1}})


@pytest.mark.parametrize("bad", [
    {"motion_model": "brownian"}, {"motion_model": None}, {"motion_model": ""},
    {"velocity_std": [1.0]}, {"velocity_std": [1.0, 1.0, 1.0]}, {"velocity_std": 1.0}, {"velocity_std": [-0.1, 1.0]},
    {"velocity_std": [1.0, float("nan")]}, {"velocity_std": [float("inf"), 1.0]}, {"velocity_std": ["a", 1.0]},
    {"velocity_decay": -0.01}, {"velocity_decay": 1.01}, {"velocity_decay": float("nan")}, {"velocity_decay": "x"},
    {"velocity_max": 0}, {"velocity_max": -3.0}, {"velocity_max": float("inf")}, {"velocity_max": float("nan")},
])
def test_config_rejects(bad):
    with pytest.raises(ValueError):
        C.load_config({"particles": {"motion_model": "constant_velocity", **bad}})


# ------------------------------------------------------------------ the chunk layout with five rows
def _fill_and_read(P, world, rows):
    """Fill every rank's chunk through shard_views with Q_i = 1000 + i, row c of particle i = 100 c + i; gather; read
    every particle's Q and rows back in global order through global_view (equal shards) or compact_index."""
    from vitparticlefiltertracker_amd.particle_filter import (chunk_words, compact_index, compact_view, global_view,
                                                              shard_range, shard_views)
    n_max = -(-P // world)
    cw = chunk_words(n_max, rows)
    assert cw % 2 == 0 and cw >= (2 + rows) * n_max
    allc = torch.full((world * cw,), -7, dtype=torch.int32)
    for r in range(world):
        b, n = shard_range(P, world, r)
        Q, st = shard_views(allc[r * cw:(r + 1) * cw], n, rows)
        assert Q.shape == (n,) and st.shape == (rows, n)
        Q.copy_(torch.arange(b, b + n) + 1000)
        for c in range(rows):
            st[c].copy_((torch.arange(b, b + n) + 100 * c).float())
    if P % world == 0:
        Qv, qs, Pv, ld, ps, nsh = global_view(allc, world, n_max, rows)
    else:
        glob = torch.index_select(allc, 0, compact_index(P, world, rows))
        assert glob.numel() == (2 + rows) * P
        Qv, qs, Pv, ld, ps, nsh = compact_view(glob, P, rows)
    assert P % nsh == 0 and ld >= nsh
    if P > nsh:
        assert qs >= nsh and ps >= (rows - 1) * ld + nsh
    gotQ = [int(Qv[(i // nsh) * qs + i % nsh]) for i in range(P)]
    got = [[float(Pv[(i // nsh) * ps + c * ld + i % nsh]) for i in range(P)] for c in range(rows)]
    assert gotQ == [1000 + i for i in range(P)]
    assert got == [[float(100 * c + i) for i in range(P)] for c in range(rows)]
    return (Qv, qs, Pv, ld, ps, nsh)


@pytest.mark.parametrize("P,world", [(10, 3), (8, 2), (9, 3), (7, 1)])
def test_layout_reads_back_every_particle_with_five_rows(P, world):
    """(10, 3): shards 3 / 3 / 4 in padded chunks, compacted. (8, 2), (9, 3): equal shards (9 / 3: an odd 5-row chunk,
    padded). With 5 rows the chunk is Q | x | y | s | vx | vy, 28 B per particle."""
    from vitparticlefiltertracker_amd.particle_filter import chunk_words
    _fill_and_read(P, world, 5)
    assert chunk_words(4, 5) * 4 == 28 * 4 and chunk_words(3, 5) == 22


@pytest.mark.parametrize("P,world", [(10, 3), (8, 2), (9, 3)])
def test_layout_with_three_rows_is_the_default_layout(P, world):
    from vitparticlefiltertracker_amd.particle_filter import (chunk_words, compact_index, compact_view, global_view,
                                                              shard_views)
    explicit = _fill_and_read(P, world, 3)
    n = -(-P // world)
    assert [chunk_words(m) for m in range(1, 9)] == [chunk_words(m, 3) for m in range(1, 9)] == \
        [5 * m + (m & 1) for m in range(1, 9)]
    chunk = torch.arange(chunk_words(n), dtype=torch.int32)
    for a, b in zip(shard_views(chunk, n), shard_views(chunk, n, 3)):
        assert a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype
    assert shard_views(chunk, n)[1].shape == (3, n)
    assert torch.equal(compact_index(P, world), compact_index(P, world, 3))
    allc = torch.zeros(world * chunk_words(n), dtype=torch.int32)
    dflt = global_view(allc, world, n) if P % world == 0 else compact_view(torch.zeros(5 * P, dtype=torch.int32), P)
    assert dflt[1] == explicit[1] and dflt[3:] == explicit[3:]
    assert dflt[3:] == ((n, chunk_words(n), n) if P % world == 0 else (P, 3 * P, P))


# ------------------------------------------------------------------ the reference itself
MS, SR = (3.0, 2.0, 0.03), (0.6, 1.8)


def test_reference_with_zero_velocity_is_s2():
    """sigma_v = 0, d = 1, zero velocities: rows 0-2 equal oracle.pf.predict bit for bit, rows 3-4 stay 0."""
    n, gb, frame, seed = 64, 5, 3, (1 << 40) + 77
    rng = np.random.default_rng(0)
    p = np.zeros((5, n), np.float32)
    p[0], p[1] = rng.uniform(0, 223, n), rng.uniform(0, 223, n)
    p[2] = rng.uniform(0.6, 1.8, n)
    p[0, :16:2], p[0, 1:16:2], p[1, :16:2], p[1, 1:16:2] = 0.0, 223.0, 223.0, 0.0   # on the borders: about half clamp
    ref = np.ascontiguousarray(p[:3])
    opf.predict(ref, gb, seed, frame, MS, 224, 224, SR)
    R.predict_cv(p, gb, seed, frame, MS, (0.0, 0.0), 1.0, 64.0, 224, 224, SR)
    assert np.array_equal(p[:3].view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(p[3:].view(np.uint32), np.zeros((2, n), np.uint32))
    assert (ref[:2] == 0).any() and (ref[:2] == 223).any()


def test_reference_fmaf_rounds_once():
    """a * b + c where rounding the exact sum to fp64 first and then to fp32 differs from rounding once."""
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)     # a b = 1 + 2^-11 + 2^-24 exactly
    c = np.float32(2.0 ** -60)
    assert R.fmaf(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)  # just above the tie: up
    assert np.float32(float(a) * float(b) + float(c)) == np.float32(1 + 2.0 ** -11)   # the tie, to even: down


def _likelihood(x, y, tx, ty):
    return [int(math.floor(math.exp(-((float(a) - tx) ** 2 + (float(b) - ty) ** 2) / (2.0 * 6.0 ** 2)) * 2.0 ** 40))
            for a, b in zip(x, y)]


@pytest.mark.parametrize("seed", [1234, 7, 99])
def test_reference_follows_a_target_the_random_walk_loses(seed):
    """A property of S11's rule: a target moving 8 px/frame, sigma = (2, 2, 0), sigma_v = (0.5, 0.5), d = 1, vmax = 64,
    256 particles, a Gaussian likelihood of width 6 px, systematic resample every frame, 24 frames. Over the last 8
    frames the constant-velocity filter stays within 16 px with vx in [6, 10] and T != 0; the random walk ends more
    than 60 px away."""
    P, K, frames, W = 256, 40, 24, 512
    ms, sr = (2.0, 2.0, 0.0), (0.5, 2.0)
    cv = R.Filter(P, (40.0, 256.0, 1.0), ms, sr, seed, (W, W), K, (0.5, 0.5), 1.0, 64.0)
    rw = np.empty((3, P), np.float32)
    rw[0], rw[1], rw[2] = 40.0, 256.0, 1.0
    err_cv, vxs, Ts, err_rw = [], [], [], []
    for k in range(1, frames + 1):
        tx, ty = 40.0 + 8.0 * k, 256.0
        cv.predict(k)
        r = cv.update(_likelihood(cv.state[0], cv.state[1], tx, ty))
        ex, ey, _ = R10.estimate(r, P)
        err_cv.append(math.hypot(ex - tx, ey - ty))
        vxs.append(R.velocity(r, P)[0])
        Ts.append(r["T"])
        opf.predict(rw, 0, seed, k, ms, W, W, sr)
        q = R10.step(_likelihood(rw[0], rw[1], tx, ty), rw, seed, k, R10.SYSTEMATIC, None, K)
        rx, ry, _ = R10.estimate(q, P)
        err_rw.append(math.hypot(rx - tx, ry - ty))
        rw = q["states"]
    print(f"seed {seed}: cv err max(last 8) = {max(err_cv[-8:]):.3f} px, vx in [{min(vxs[-8:]):.3f}, "
          f"{max(vxs[-8:]):.3f}], rw err at the last frame = {err_rw[-1]:.3f} px")
    assert max(err_cv[-8:]) < 16.0, err_cv
    assert all(6.0 <= v <= 10.0 for v in vxs[-8:]), vxs
    assert all(T != 0 for T in Ts[-8:]), Ts
    assert err_rw[-1] > 60.0, err_rw


# ------------------------------------------------------------------ the C ABI
def _lib():
    from vitparticlefiltertracker_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_libvpf_exports_the_s11_entry_points():
    import ctypes
    _lib_mod = _lib()
    L = ctypes.CDLL(_lib_mod.LIB_PATH)
    for name in ("vpf_predict_cv", "vpf_gather_rows", "vpf_weighted_sums"):
        assert hasattr(L, name), name
        assert name in _lib_mod.SIGNATURES


def test_c_abi_rejects_bad_s11_arguments_before_any_launch():
    L = _lib().lib()
    fake = 4096                                          # never dereferenced: validation fails first
    inf, nan = float("inf"), float("nan")

    def predict(n=8, ld=8, gb=0, svx=1.0, svy=1.0, d=1.0, vmax=64.0):
        return L.vpf_predict_cv(fake, n, ld, gb, 1, 1, 1.0, 1.0, 0.1, svx, svy, d, vmax, 224.0, 224.0, 0.5, 2.0, None)
    assert predict(n=-1) == -1 and predict(ld=7) == -1 and predict(gb=-1) == -1 and predict(gb=(1 << 32) - 4) == -1
    assert predict(d=-0.5) == -1 and predict(d=1.5) == -1 and predict(d=nan) == -1
    assert predict(svx=-1.0) == -1 and predict(svy=-1.0) == -1 and predict(svx=inf) == -1 and predict(svy=nan) == -1
    assert predict(vmax=0.0) == -1 and predict(vmax=-1.0) == -1 and predict(vmax=inf) == -1 and predict(vmax=nan) == -1

    def gather(n_slots=8, ld=8, ps=40, nsh=8, P=16, n_rows=2, out_ld=8):
        return L.vpf_gather_rows(fake, n_slots, fake, ld, ps, nsh, P, n_rows, fake, out_ld, None)
    assert gather(n_slots=-1) == -1 and gather(out_ld=7) == -1
    assert gather(P=0) == -1 and gather(P=17) == -1 and gather(P=1 << 31) == -1 and gather(nsh=0) == -1
    assert gather(ld=7) == -1 and gather(n_rows=0) == -1 and gather(n_rows=9) == -1
    assert gather(ps=15) == -1 and gather(n_rows=8, ps=63) == -1          # shards overlap the rows

    def sums(qs=8, ld=8, ps=40, nsh=8, P=16, n_rows=2):
        return L.vpf_weighted_sums(fake, qs, fake, ld, ps, nsh, P, n_rows, fake, None)
    assert sums(P=0) == -1 and sums(P=17) == -1 and sums(P=1 << 31) == -1 and sums(nsh=0) == -1
    assert sums(ld=7) == -1 and sums(n_rows=0) == -1 and sums(n_rows=4) == -1
    assert sums(qs=7) == -1 and sums(ps=15) == -1
