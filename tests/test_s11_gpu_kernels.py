"""GPU (MI355X): the SPEC S11 kernels — vpf_predict_cv bit for bit against the Python reference
(tests/s11_reference.py), vpf_gather_rows cell by cell, vpf_weighted_sums against vpf_estimate_resample's statistics
and math.fsum. Run: python -m pytest tests -m gpu."""
import math

import numpy as np
import pytest
import torch

import s11_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
W, H = 320, 224
MS, SR, VMAX = (3.0, 2.0, 0.03), (0.6, 1.8), 16.0


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()
    assert torch.cuda.is_available()


def vpf():
    return torch.ops.vpf


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ vpf_predict_cv
def _state(n, seed=0):
    """Five rows with, cyclically over the index, particles on both borders of both axes, velocities at +-vmax and at
    +-3 vmax (no step of noise brings those back inside, so the velocity clamp fires whatever d > 0 is), velocities
    that push a border particle further out, and scales at both ends of the range."""
    rng = np.random.default_rng(seed + n)
    p = np.empty((5, n), np.float32)
    p[0], p[1] = rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)
    p[2] = rng.uniform(SR[0], SR[1], n)
    p[3], p[4] = rng.uniform(-VMAX, VMAX, n), rng.uniform(-VMAX, VMAX, n)
    i = np.arange(n)
    for k, (row, val) in enumerate([(0, 0.0), (0, W - 1.0), (1, 0.0), (1, H - 1.0), (2, SR[0]), (2, SR[1]),
                                    (3, VMAX), (3, -VMAX), (4, 3 * VMAX), (4, -3 * VMAX), (3, 3 * VMAX),
                                    (3, -3 * VMAX)]):
        p[row, i % 16 == k] = val
    p[3, i % 16 == 0], p[3, i % 16 == 1] = -VMAX, VMAX          # on the x borders, moving outwards
    p[4, i % 16 == 2], p[4, i % 16 == 3] = -VMAX, VMAX
    return p


def _gpu_predict_cv(p, gb, seed, frame, sv, d, ld=None):
    n = p.shape[1]
    if ld is None:
        t = torch.from_numpy(p.copy()).to(DEV)
        vpf().predict_cv_(t, gb, seed, frame, list(MS), list(sv), d, VMAX, float(W), float(H), list(SR))
        return t.cpu().numpy()
    from vitparticlefiltertracker_amd import _lib
    buf = torch.full((5, ld), -5.0, device=DEV)
    buf[:, :n] = torch.from_numpy(p).to(DEV)
    _lib.call("vpf_predict_cv", buf.data_ptr(), n, ld, gb, seed, frame, MS[0], MS[1], MS[2], sv[0], sv[1], d, VMAX,
              float(W), float(H), SR[0], SR[1], _lib.stream_ptr())
    out = buf.cpu().numpy()
    assert np.all(out[:, n:] == -5.0), "columns past n were written"
    return np.ascontiguousarray(out[:, :n])


def _ref_predict_cv(p, gb, seed, frame, sv, d):
    q = p.copy()
    R.predict_cv(q, gb, seed, frame, MS, sv, d, VMAX, W, H, SR)
    return q


@pytest.mark.parametrize("d,sv", [(0.0, (1.0, 0.5)), (0.5, (1.0, 0.5)), (1.0, (1.0, 0.5)), (1.0, (0.0, 0.0))])
@pytest.mark.parametrize("n,gb,ld", [(1, 0, None), (255, 0, None), (257, 1000, 300), (1000, 7, None)])
def test_predict_cv_equals_reference(n, gb, ld, d, sv):
    """n: one particle; a ragged last wave; one particle into a second block (with global_begin != 0 and ld > n, through
    the C ABI); four blocks. Every decay and a zero velocity noise; with 255 particles and more every clamp fires."""
    seed, frame = (1 << 40) + 31 * n, 6
    p = _state(n)
    ref = _ref_predict_cv(p, gb, seed, frame, sv, d)
    got = _gpu_predict_cv(p, gb, seed, frame, sv, d, ld)
    for c, name in enumerate(("x", "y", "s", "vx", "vy")):
        assert np.array_equal(bits(got[c]), bits(ref[c])), f"row {name}: {np.flatnonzero(got[c] != ref[c])[:8]}"
    if n >= 255:
        for row, lo, hi in ((0, 0.0, W - 1.0), (1, 0.0, H - 1.0), (2, SR[0], SR[1])):
            assert (ref[row] == np.float32(lo)).any() and (ref[row] == np.float32(hi)).any(), f"row {row}: no clamp"
        if d > 0.0:
            for row in (3, 4):
                assert (ref[row] == VMAX).any() and (ref[row] == -VMAX).any(), f"row {row}: no clamp"
        # a particle clamped at the border keeps its velocity
        assert (ref[3][ref[0] == 0.0] < 0).any() and (ref[3][ref[0] == W - 1.0] > 0).any()


def test_predict_cv_does_not_depend_on_the_sharding():
    n, seed, frame, sv, d = 1000, 99, 4, (1.0, 0.5), 0.75
    p = _state(n, seed=1)
    whole = _gpu_predict_cv(p, 0, seed, frame, sv, d)
    a = _gpu_predict_cv(np.ascontiguousarray(p[:, :333]), 0, seed, frame, sv, d)
    b = _gpu_predict_cv(np.ascontiguousarray(p[:, 333:]), 333, seed, frame, sv, d)
    assert np.array_equal(bits(np.concatenate([a, b], axis=1)), bits(whole))
    assert not np.array_equal(bits(_gpu_predict_cv(np.ascontiguousarray(p[:, 333:]), 0, seed, frame, sv, d)),
                              bits(whole[:, 333:]))


@pytest.mark.parametrize("n", [1, 257, 1000])
def test_predict_cv_with_zero_velocity_is_predict(n):
    """sigma_v = 0, d = 1, zero velocities: rows 0-2 are vpf_predict's bits, rows 3-4 stay 0."""
    seed, frame, gb = 5, 2, 11
    p = _state(n, seed=2)
    p[3:] = 0.0
    got = _gpu_predict_cv(p, gb, seed, frame, (0.0, 0.0), 1.0)
    t = torch.from_numpy(np.ascontiguousarray(p[:3])).to(DEV)
    vpf().predict_(t, gb, seed, frame, list(MS), float(W), float(H), list(SR))
    assert np.array_equal(bits(got[:3]), bits(t.cpu().numpy()))
    assert np.array_equal(bits(got[3:]), np.zeros((2, n), np.uint32))


# ------------------------------------------------------------------ vpf_gather_rows
SENT = -12345.0


def _gather_case(flat, ld, ps, nsh, P, n_rows, rng):
    """Random ancestors with repeats, 0 and P - 1 among them; the whole slot range and two sub-ranges of it. Written
    cells are exact; every other cell of the output keeps the sentinel."""
    n_slots = max(P, 5)
    anc = rng.integers(0, P, n_slots).astype(np.int32)
    anc[0], anc[-1], anc[n_slots // 2] = P - 1, 0, anc[(n_slots // 2) - 1]
    anc_d = torch.from_numpy(anc).to(DEV)
    flat_d = torch.from_numpy(flat).to(DEV)
    for b, e in {(0, n_slots), (1, n_slots - 1), (n_slots // 3, n_slots // 3 + 1)}:
        cnt, out_ld = e - b, e - b + 3
        out = torch.full((n_rows + 1, out_ld), SENT, device=DEV)
        vpf().gather_rows(anc_d[b:e], flat_d, ld, ps, nsh, P, n_rows, out)
        got = out.cpu().numpy()
        a = anc[b:e].astype(np.int64)
        for c in range(n_rows):
            want = flat[(a // nsh) * ps + c * ld + a % nsh]
            assert np.array_equal(bits(got[c, :cnt]), bits(want)), (b, e, c)
        assert np.all(got[:n_rows, cnt:] == SENT) and np.all(got[n_rows] == SENT), (b, e)


@pytest.mark.parametrize("n_rows", [1, 2, 8])
@pytest.mark.parametrize("P", [1, 33, 1000])
def test_gather_rows_one_shard(P, n_rows):
    rng = np.random.default_rng(P + n_rows)
    flat = rng.standard_normal(n_rows * P).astype(np.float32)
    _gather_case(flat, P, n_rows * P, P, P, n_rows, rng)


@pytest.mark.parametrize("n_rows", [1, 2, 8])
def test_gather_rows_three_padded_shards(n_rows):
    """n_shard = 4, ld = 5 (a padded row), p_stride = 45 > 2 ld + n_shard (and >= 7 ld + n_shard for eight rows): every
    cell of the buffer holds its own value, so a wrong stride reads a wrong number."""
    nsh, ld, ps, G = 4, 5, 45, 3
    flat = np.arange(G * ps, dtype=np.float32) + 0.5
    _gather_case(flat, ld, ps, nsh, G * nsh, n_rows, np.random.default_rng(n_rows))


@pytest.mark.parametrize("n_rows", [1, 2])
def test_gather_rows_compacted_view(n_rows):
    """P = 10 over 3 ranks (3 / 3 / 4): the five-row chunks compacted into the global order; the velocity rows start at
    the particle view + 3 ld."""
    from vitparticlefiltertracker_amd.particle_filter import (chunk_words, compact_index, compact_view, shard_range,
                                                              shard_views)
    P, world = 10, 3
    cw = chunk_words(4, 5)
    allc = torch.zeros(world * cw, dtype=torch.int32)
    for r in range(world):
        b, n = shard_range(P, world, r)
        _, st = shard_views(allc[r * cw:(r + 1) * cw], n, 5)
        for c in range(5):
            st[c].copy_((torch.arange(b, b + n) + 100 * c).float())
    glob = torch.index_select(allc, 0, compact_index(P, world, 5))
    _, _, Pv, ld, ps, nsh = compact_view(glob, P, 5)
    vel = Pv[3 * ld:].numpy().copy()
    assert vel[:P].tolist() == [300.0 + i for i in range(P)] and vel[ld:ld + P].tolist() == [400.0 + i for i in range(P)]
    _gather_case(vel, ld, ps, nsh, P, n_rows, np.random.default_rng(n_rows))


# ------------------------------------------------------------------ vpf_weighted_sums
def _weights(kind, P, rng):
    Q = np.zeros(P, np.int64)
    if kind == "random":
        Q = rng.integers(0, (1 << 40) + 1, P, dtype=np.int64)
    elif kind == "onehot":
        Q[P // 3] = 12345
    else:
        assert kind == "zero"
    return Q


def _sums(view, P, n_rows):
    out = torch.full((4,), -1, device=DEV, dtype=torch.int64)
    vpf().weighted_sums(*view, P, n_rows, out)
    return out.cpu()


@pytest.mark.parametrize("kind", ["random", "onehot", "zero"])
@pytest.mark.parametrize("P", [1, 33, 1025, 5000])
def test_weighted_sums_over_the_states_are_estimate_resamples_statistics(P, kind):
    """P: one particle; a ragged wave; one past the tree's 1024 stride; several strides. The four words are
    vpf_estimate_resample's stats_out[0..3] as bits (zero weights: the plain sums of the T == 0 rule)."""
    rng = np.random.default_rng(P + len(kind))
    Q = torch.from_numpy(_weights(kind, P, rng)).to(DEV)
    p = torch.from_numpy(rng.uniform(0, 224, (3, P)).astype(np.float32)).to(DEV)
    stats = torch.empty(4, device=DEV, dtype=torch.int64)
    vpf().estimate_resample(Q, P, p.view(-1), P, 3 * P, P, P, 77, 3, 0, P, torch.empty(P, device=DEV, dtype=torch.int32),
                            torch.empty(3, P, device=DEV), torch.empty(P, device=DEV, dtype=torch.int64), stats)
    assert torch.equal(_sums((Q, P, p.view(-1), P, 3 * P, P), P, 3), stats.cpu())
    # fewer rows: the same leading sums, zeros after them
    two = _sums((Q, P, p.view(-1), P, 3 * P, P), P, 2)
    assert torch.equal(two[:3], stats.cpu()[:3]) and int(two[3]) == 0


@pytest.mark.parametrize("kind", ["random", "onehot", "zero"])
@pytest.mark.parametrize("P", [33, 1026])
def test_weighted_sums_over_velocity_rows(P, kind):
    """T exact, the two sums within 1e-12 relative of math.fsum, the unused word 0, and the same bits from one shard
    and from three gathered five-row chunks of the same data.
    The velocities are uniform over [-4, 12) px/frame (a target moving at +4): both signs occur, and the sums stay
    well conditioned (sum |t| / |sum t| <= 4 or so), so the relative bound means what it means for S6's positive
    states: the tree's error is at most (P / 1024 + 11) roundings of 2^-53 each on sum |t|, under 1e-14 relative."""
    from vitparticlefiltertracker_amd.particle_filter import chunk_words, global_view, shard_views
    rng = np.random.default_rng(3 * P + len(kind))
    Q = _weights(kind, P, rng)
    st = rng.uniform(0, 224, (5, P)).astype(np.float32)
    st[3:] = rng.uniform(-4, 12, (2, P)).astype(np.float32)
    assert (st[3:] < 0).any()
    one = torch.from_numpy(st).to(DEV)
    got1 = _sums((torch.from_numpy(Q).to(DEV), P, one.view(-1)[3 * P:], P, 5 * P, P), P, 2)
    G, n = 3, P // 3
    cw = chunk_words(n, 5)
    allc = torch.zeros(G * cw, dtype=torch.int32)
    for r in range(G):
        Qv, pv = shard_views(allc[r * cw:(r + 1) * cw], n, 5)
        Qv.copy_(torch.from_numpy(Q[r * n:(r + 1) * n].copy()))
        pv.copy_(torch.from_numpy(st[:, r * n:(r + 1) * n].copy()))
    Qv, qs, Pv, ld, ps, nsh = global_view(allc.to(DEV), G, n, 5)
    got3 = _sums((Qv, qs, Pv[3 * ld:], ld, ps, nsh), P, 2)
    assert torch.equal(got1, got3), "the sums depend on the shard count"
    T = int(Q.sum())
    assert int(got1[0]) == T and int(got1[3]) == 0
    w = [int(q) for q in Q] if T else [1] * P
    want = [math.fsum(float(q) * float(v) for q, v in zip(w, st[c])) for c in (3, 4)]
    np.testing.assert_allclose(got1[1:3].view(torch.float64).numpy(), want, rtol=1e-12, atol=0)
