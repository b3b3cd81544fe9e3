"""GPU (MI355X): SPEC S16's search predict, vpf_predict_search / torch.ops.vpf.predict_search_, bit for bit against the
Python reference (tests/s16_reference.py) on the smallest shapes that can go wrong: one particle, a ragged wave, one
block exactly, one particle into a second block, four blocks; square, tiny and HD frames; ld > n, shards, both row
counts; and every rejection of the C ABI. Run: python -m pytest tests -m gpu."""
import numpy as np
import pytest
import torch

import s16_reference as R
from oracle import pf as opf

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIG_S, SR = 0.03, (0.6, 1.8)
CANARY = -5.0
FRAMES = [(224, 224), (37, 11), (1920, 1080)]       # (W, H)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()
    assert torch.cuda.is_available()


def vpf():
    return torch.ops.vpf


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _state(n, rows, seed=0):
    """Rows x | y | s (| vx | vy): positions anywhere (the search must not read them), scales across and at both ends
    of the range, non-zero velocities with NaNs and infinities among them."""
    rng = np.random.default_rng(seed + 7 * n + rows)
    p = np.empty((rows, n), np.float32)
    p[0], p[1] = rng.uniform(-50, 2500, n), rng.uniform(-50, 2500, n)
    p[2] = rng.uniform(SR[0], SR[1], n)
    p[2, np.arange(n) % 8 == 1], p[2, np.arange(n) % 8 == 2] = SR[0], SR[1]
    if rows == 5:
        p[3], p[4] = rng.uniform(-16, 16, n) + 17.0, rng.uniform(-16, 16, n) - 17.0
        p[3, np.arange(n) % 4 == 0], p[4, np.arange(n) % 4 == 1] = np.nan, -np.inf
    return p


def _lattice(P, W, H):
    from vitparticlefiltertracker_amd.config import redetect_lattice
    return redetect_lattice(P, W, H)


def _gpu_search(p, gb, P, seed, frame, W, H, ld=None, total_rows=None):
    """Through the op (ld None), or through the C ABI on a [total_rows][ld] buffer of canaries whose first rows hold
    p: the columns past n and the rows past p's must keep the canary."""
    rows, n = p.shape
    gx, inv_gx, inv_P = _lattice(P, W, H)
    if ld is None:
        t = torch.from_numpy(p.copy()).to(DEV)
        vpf().predict_search_(t, gb, P, seed, frame, SIG_S, float(W), float(H), list(SR), gx, inv_gx, inv_P)
        return t.cpu().numpy()
    from vitparticlefiltertracker_amd import _lib
    total_rows = total_rows or rows
    buf = torch.full((total_rows, ld), CANARY, device=DEV)
    buf[:rows, :n] = torch.from_numpy(p).to(DEV)
    _lib.call("vpf_predict_search", buf.data_ptr(), n, ld, gb, P, rows, seed, frame, SIG_S, float(W), float(H), SR[0],
              SR[1], gx, inv_gx, inv_P, _lib.stream_ptr())
    out = buf.cpu().numpy()
    assert np.all(out[:, n:] == CANARY), "columns past n were written"
    assert np.all(out[rows:] == CANARY), "rows past the state's were written"
    return np.ascontiguousarray(out[:rows, :n])


def _ref_search(p, gb, P, seed, frame, W, H):
    q = p.copy()
    R.predict_search(q, gb, P, seed, frame, SIG_S, W, H, SR)
    return q


def _same(got, ref, tag=""):
    for c, name in enumerate(("x", "y", "s", "vx", "vy")[:ref.shape[0]]):
        assert np.array_equal(bits(got[c]), bits(ref[c])), f"{tag} row {name}: {np.flatnonzero(bits(got[c]) != bits(ref[c]))[:8]}"


@pytest.mark.parametrize("rows", [3, 5])
@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("P", [1, 7, 255, 256, 257, 1000])
def test_predict_search_equals_reference(P, W, H, rows):
    """The whole set in one call through the op. The scale row equals oracle.pf.predict's for the same seed and frame
    (the bits an ordinary predict gives it); with five rows the velocity words are exactly 0x00000000, from non-zero,
    NaN and infinite inputs; every coordinate is inside the frame."""
    seed, frame = (1 << 40) + 31 * P + W, 12
    p = _state(P, rows)
    got = _gpu_search(p, 0, P, seed, frame, W, H)
    _same(got, _ref_search(p, 0, P, seed, frame, W, H))
    walk = np.ascontiguousarray(p[:3]).copy()
    opf.predict(walk, 0, seed, frame, (4.0, 4.0, SIG_S), W, H, SR)
    assert np.array_equal(bits(got[2]), bits(walk[2])), "the scale row is not S2's step"
    assert got[0].min() >= 0.0 and got[0].max() <= W - 1 and got[1].min() >= 0.0 and got[1].max() <= H - 1
    if rows == 5:
        assert not bits(got[3:]).any(), "velocity words are not +0.0f"
    if P >= 255:
        assert (walk[2] == np.float32(SR[0])).any() and (walk[2] == np.float32(SR[1])).any(), "no scale clamp fired"


@pytest.mark.parametrize("rows,total_rows", [(3, 3), (3, 6), (5, 6)])
@pytest.mark.parametrize("P,gb,n,ld", [(1000, 300, 257, 300), (257, 1, 255, 256), (7, 2, 3, 64), (1000, 999, 1, 2)])
def test_shard_inside_the_set_with_padding_through_the_c_abi(P, gb, n, ld, rows, total_rows):
    """A shard [gb, gb + n) strictly inside [0, P), ld > n: canaries in the padding columns and in the rows past the
    state's (the angle row of a six-row chunk; the velocity rows when the three-row instance runs) stay untouched."""
    W, H = 224, 224
    assert 0 < gb and gb + n <= P and ld > n and (gb + n < P or n == 1)
    seed, frame = 77, 5
    p = _state(n, rows, seed=3)
    got = _gpu_search(p, gb, P, seed, frame, W, H, ld=ld, total_rows=total_rows)
    _same(got, _ref_search(p, gb, P, seed, frame, W, H))


@pytest.mark.parametrize("rows", [3, 5])
@pytest.mark.parametrize("W,H", [(224, 224), (1920, 1080)])
def test_three_shard_calls_equal_one_whole_call(W, H, rows):
    """Only the global index enters: [0, 333) + [333, 667) + [667, 1000) equal the whole call bit for bit; a shard given
    the wrong global_begin does not."""
    P, seed, frame = 1000, 99, 4
    p = _state(P, rows, seed=1)
    whole = _gpu_search(p, 0, P, seed, frame, W, H)
    parts = [_gpu_search(np.ascontiguousarray(p[:, a:b]), a, P, seed, frame, W, H)
             for a, b in ((0, 333), (333, 667), (667, 1000))]
    assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(whole))
    moved = _gpu_search(np.ascontiguousarray(p[:, 333:667]), 0, P, seed, frame, W, H)
    assert not np.array_equal(bits(moved[:2]), bits(whole[:2, 333:667]))


def test_two_frames_differ_and_the_same_frame_repeats():
    P, seed, W, H = 1000, 5, 224, 224
    p = _state(P, 3, seed=2)
    a, again, b = (_gpu_search(p, 0, P, seed, f, W, H) for f in (8, 8, 9))
    assert np.array_equal(bits(a), bits(again))
    assert (a[0] != b[0]).mean() > 0.99 and (a[1] != b[1]).mean() > 0.99
    other = _gpu_search(p, 0, P, seed + 1, 8, W, H)
    assert (a[0] != other[0]).mean() > 0.99
    # the lattice itself does not move: the same cells, other offsets inside them
    gx = R.lattice(P, W, H)[0]
    for r in (a, b, other):
        assert np.array_equal(np.floor(r[0].astype(np.float64) * gx / (W - 1.0)).astype(int), np.arange(P) % gx)


def test_op_refuses_what_it_cannot_run():
    gx, inv_gx, inv_P = _lattice(16, 224, 224)
    args = (0, 16, 1, 1, SIG_S, 224.0, 224.0, list(SR), gx, inv_gx, inv_P)
    with pytest.raises(Exception):
        vpf().predict_search_(torch.zeros(3, 16), *args)                    # a CPU tensor
    with pytest.raises(ValueError):
        vpf().predict_search_(torch.zeros(4, 16, device=DEV), *args)        # rows not 3 or 5
    with pytest.raises(ValueError):
        vpf().predict_search_(torch.zeros(3, 16, device=DEV, dtype=torch.float64), *args)


def test_c_abi_rejections_launch_nothing():
    """Every rejection returns VPF_ERR_ARG (-1) and leaves the buffer as it was; n == 0 returns 0 and launches
    nothing."""
    from vitparticlefiltertracker_amd import _lib
    n, ld, P = 16, 32, 64
    gx, inv_gx, inv_P = _lattice(P, 224, 224)
    buf = torch.full((5, ld), CANARY, device=DEV)
    fn = _lib.lib().vpf_predict_search

    def call(n=n, ld=ld, gb=0, P=P, rows=3, gx=gx):
        return fn(buf.data_ptr(), n, ld, gb, P, rows, 9, 3, SIG_S, 224.0, 224.0, SR[0], SR[1], gx, inv_gx, inv_P,
                  _lib.stream_ptr())
    bad = [dict(rows=4), dict(rows=0), dict(rows=6), dict(rows=-3), dict(P=0), dict(P=-1), dict(P=(1 << 24) + 1),
           dict(gb=P - n + 1), dict(gb=P), dict(gb=-1), dict(n=-1), dict(n=ld + 1), dict(gx=0), dict(gx=-2),
           dict(gx=1 << 32), dict(n=P + 1, ld=P + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(n=0) == 0 and call(n=0, gb=P) == 0
    torch.cuda.synchronize()
    assert torch.all(buf == CANARY), "a rejected call or n == 0 wrote to the buffer"
    assert call(P=1 << 24, gb=(1 << 24) - n) == 0 and call(rows=5, gb=P - n) == 0      # the edges that are allowed
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.all(out[:, n:] == CANARY) and np.all(out[:, :n] != CANARY)
