"""GPU (MI355X): SPEC S13's kernel — vpf_color_weight's counts, scores and weights bit for bit against the numpy
reference (tests/s13_reference.py) for every bins x grid, with S3 and S12 coordinates, boxes inside, across and
outside the frame, under maximal same-address contention, combined in place against Python integers, on a prefilled
workspace, on a sub-range, and every argument check. Run: python -m pytest tests -m gpu."""
import math
import random

import numpy as np
import pytest
import torch

import s13_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
K40 = 40
H1, W1, BOX1 = 40, 48, (20.0, 14.0)          # a 48 x 40 frame, a non-square template box
PI = math.pi


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()
    assert torch.cuda.is_available()


def vpf():
    return torch.ops.vpf


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _states(n, seed=1):
    """n finite states on the 48 x 40 frame. The first ten by hand: inside; across the left, right, top and bottom
    edges; wholly outside (every tap in the zero border); the scales 0.5 and 2.0; a corner; fractional coordinates.
    The rest random, centres up to 12 px outside the frame."""
    hand = np.array([[24.0, 20.0, 1.0], [2.0, 20.0, 1.0], [46.0, 18.0, 1.0], [24.0, 3.0, 1.0], [24.0, 38.0, 1.0],
                     [-40.0, -40.0, 1.0], [24.0, 20.0, 0.5], [24.0, 20.0, 2.0], [47.0, 39.0, 1.37], [20.5, 17.25, 0.77]],
                    np.float32)
    rng = np.random.default_rng(seed)
    rnd = np.stack([rng.uniform(-12, W1 + 12, n), rng.uniform(-12, H1 + 12, n), rng.uniform(0.5, 2.0, n)], 1)
    return np.ascontiguousarray(np.concatenate([hand, rnd.astype(np.float32)])[:n].T)


def _angles(n):
    return np.resize(np.array([0.0, 0.3, -0.3, PI / 2, -PI / 2], np.float32), n)


def gpu_color(frame, p, ang, box, C, B, tmpl=None, lam=20.0, K=K40, combine=False, Q0=None, pad=0, ws=None,
              fill=True, want_hist=True):
    """vpf.color_weight on particles float32[3][n] stored with row stride n + pad; returns (hist, rho, Q) as numpy
    (None where not asked for)."""
    from vitparticlefiltertracker_amd import ops
    n, nb = p.shape[1], B ** 3
    store = torch.full((3, n + pad), 7.0, device=DEV)
    store[:, :n] = torch.from_numpy(p)
    view = store[:, :n]
    assert view.stride(0) == n + pad
    fd = torch.from_numpy(frame).to(DEV)
    ws = ops.rgba_workspace(frame.shape[:2], DEV) if ws is None else ws
    hist = torch.full((n, nb), -1, device=DEV, dtype=torch.int32) if want_hist else None
    rho = torch.full((n,), -5.0, device=DEV) if tmpl is not None else None
    Q = None
    if tmpl is not None:
        Q = torch.from_numpy(np.asarray(Q0, np.int64)).to(DEV) if Q0 is not None else \
            torch.full((n,), -1, device=DEV, dtype=torch.int64)
    vpf().color_weight(fd if fill else None, ws, fill, view, None if ang is None else torch.from_numpy(ang).to(DEV),
                       [float(box[0]), float(box[1])], [frame.shape[0], frame.shape[1]], C, B,
                       None if tmpl is None else torch.from_numpy(tmpl).to(DEV), float(lam), K, combine, hist, rho, Q)
    torch.cuda.synchronize()
    assert (store[:, n:] == 7.0).all()
    return (None if hist is None else hist.cpu().numpy().astype(np.int64), None if rho is None else rho.cpu().numpy(),
            None if Q is None else Q.cpu().numpy())


def _check(frame, p, ang, box, C, B, tmpl, lam=20.0, K=K40, pad=0, tag=""):
    h_ref = R.histograms(frame, p, ang, box, C, B)
    r_ref = R.rho(h_ref, tmpl, C)
    q_ref = R.weights(r_ref, lam, K)
    h, r, q = gpu_color(frame, p, ang, box, C, B, tmpl, lam, K, pad=pad)
    bad = np.flatnonzero((h != h_ref).any(axis=1))
    assert bad.size == 0, f"{tag}: histograms differ, first particles {bad[:8]}"
    assert (h.sum(axis=1) == C * C).all()
    assert np.array_equal(bits(r), bits(r_ref)), f"{tag}: rho differs at {np.flatnonzero(bits(r) != bits(r_ref))[:8]}"
    assert np.array_equal(q, q_ref), f"{tag}: Q differs at {np.flatnonzero(q != q_ref)[:8]}"
    return h_ref, r_ref, q_ref


# ------------------------------------------------------------------ counts, scores, weights
@pytest.mark.parametrize("rot", [False, True], ids=["s3", "s12"])
@pytest.mark.parametrize("C", [8, 32, 64])
@pytest.mark.parametrize("B", [4, 8, 16])
def test_color_weight_equals_reference(B, C, rot):
    """67 particles (row stride 80) on the 48 x 40 frame, box 20 x 14: grid 8 has fewer samples than threads, grid 64
    sixteen per thread; bins 4 and 8 count into a histogram per wave, bins 16 into one. The template is particle 0's own
    histogram: its score is exactly 1.0f and its weight 2^K; the wholly outside box counts every sample in bin 0."""
    frame = _frame(H1, W1, 10 * B + C)
    p = _states(67)
    ang = _angles(67) if rot else None
    tmpl = R.normalised(R.histograms(frame, p[:, :1], None if ang is None else ang[:1], BOX1, C, B), C)[0]
    h, r, q = _check(frame, p, ang, BOX1, C, B, tmpl, pad=13, tag=f"B {B} C {C} rot {rot}")
    assert bits(r[:1])[0] == bits(np.float32(1.0)) and q[0] == 1 << K40
    assert h[5, 0] == C * C and len(set(q.tolist())) > 2      # the weights vary (64 samples in 4096 bins: 9 values)


@pytest.mark.parametrize("n", [1, 3])
def test_small_batches(n):
    frame = _frame(H1, W1, n)
    p = _states(10)[:, 7:7 + n].copy()
    tmpl = R.template(frame, (14.0, 13.0, 20.0, 14.0), None, 32, 8)
    _check(frame, p, None, BOX1, 32, 8, tmpl, pad=5, tag=f"n {n}")
    _check(frame, p, _angles(n) + np.float32(0.1), BOX1, 32, 8, tmpl, pad=5, tag=f"n {n} rotated")


@pytest.mark.parametrize("B,C", [(16, 64), (8, 64), (4, 8)])
def test_single_colour_frame_counts_exactly_under_contention(B, C):
    """Every sample of a box inside a one-colour frame lands in ONE bin: C^2 atomic adds on one LDS address (bins 16)
    or on one address per wave (bins 4, 8). A box across the edge splits between that bin, bin 0 and the blends."""
    frame = np.empty((H1, W1, 3), np.uint8)
    frame[...] = (200, 100, 50)
    p = _states(10)
    tmpl = R.normalised(R.histograms(frame, p[:, :1], None, BOX1, C, B), C)[0]
    h, r, q = _check(frame, p, None, BOX1, C, B, tmpl, tag=f"B {B} C {C}")
    sh = 8 - (B.bit_length() - 1)
    one = ((200 >> sh) * B + (100 >> sh)) * B + (50 >> sh)
    assert h[0, one] == C * C and h[6, one] == C * C and h[5, 0] == C * C
    assert r[0] == 1.0 and r[6] == 1.0 and r[5] == 0.0 and q[0] == 1 << K40


def test_histograms_only_without_a_template():
    frame = _frame(H1, W1, 3)
    p, ang = _states(12), _angles(12)
    h, r, q = gpu_color(frame, p, ang, BOX1, 16, 4, None)
    assert r is None and q is None and np.array_equal(h, R.histograms(frame, p, ang, BOX1, 16, 4))


# ------------------------------------------------------------------ states beyond the int range
FAR_HW, FAR_BOX, FAR_C, FAR_B = (24, 32), (10.0, 8.0), 8, 4
FAR_STATES = np.ascontiguousarray(np.array(
    [[16.0, 12.0, 1.0], [3e9, 12.0, 1.0], [10.5, 9.25, 1.2], [16.0, -3e9, 1.0], [np.inf, 12.0, 1.0], [20.0, 14.0, 0.8],
     [16.0, -np.inf, 1.0], [14.0, 10.0, 1.0]], np.float32).T)
FAR_ORDINARY, FAR_HUGE, FAR_INF = [0, 2, 5, 7], [1, 3], [4, 6]


@pytest.mark.parametrize("rot", [False, True], ids=["s3", "s12"])
def test_states_beyond_the_int_range_count_padding_only(rot):
    """SPEC S3's last paragraph, for the cue: a coordinate of +-3e9 converts to a saturated int, every tap (the second
    one's index wraps) is clamped into the zero border, and all C^2 samples fall in bin 0 (closed form: the numpy
    reference's float -> int conversion is not defined there). A +-inf coordinate gives NaN values, whose bins are the
    device's conversion of NaN: only the count is asserted. The ordinary particles between them are the reference's
    counts exactly: no state disturbs a neighbour. The op raises on a non-zero status."""
    frame = _frame(*FAR_HW, 31)
    ang = np.full(8, 0.3, np.float32) if rot else None
    CC = FAR_C * FAR_C
    ref = R.histograms(frame, FAR_STATES[:, FAR_ORDINARY].copy(), None if ang is None else ang[FAR_ORDINARY], FAR_BOX,
                       FAR_C, FAR_B)
    assert (ref[:, 0] < CC).all(), "an ordinary box counts only bin 0: the case tests nothing"
    h, _, _ = gpu_color(frame, FAR_STATES, ang, FAR_BOX, FAR_C, FAR_B, None, pad=3)
    assert np.array_equal(h[FAR_ORDINARY], ref)
    assert (h[FAR_HUGE, 0] == CC).all() and not h[FAR_HUGE, 1:].any()
    assert (h[FAR_INF].sum(axis=1) == CC).all() and (h[FAR_INF] >= 0).all()


# ------------------------------------------------------------------ the combination, in place
@pytest.mark.parametrize("K", [40, 1, 0, 61])
def test_combine_in_place_equals_python_integers(K):
    """Q <- (Q Lc) >> K against Python integers. Lv takes 0, 1, 2^K - 1, 2^K and random values against every Lc the
    cue produces here: 2^K (the template's own box), 0 (lambda 1e6 on any rho < 1) and, at lambda 20, values in
    between (at K = 1, lambda 0.5 gives w in [0.6, 1) and so Lc = 1 = 2^K - 1)."""
    frame = _frame(H1, W1, 40 + K)
    p = np.ascontiguousarray(np.repeat(_states(10)[:, :5], 10, axis=1))          # 5 boxes x 10 values of Lv
    tmpl = R.normalised(R.histograms(frame, p[:, :1], None, BOX1, 32, 8), 32)[0]
    rnd = random.Random(K)
    edge = [0, 1, max((1 << K) - 1, 0), 1 << K] + [rnd.randrange(0, (1 << K) + 1) for _ in range(6)]
    Lv = np.array(edge * 5, np.int64)
    seen = set()
    for lam in (20.0, 1e6, 0.5, 0.0):
        Lc = R.color_weights(frame, p, None, BOX1, tmpl, 32, 8, lam, K)
        seen |= set(Lc.tolist())
        _, _, q = gpu_color(frame, p, None, BOX1, 32, 8, tmpl, lam, K, combine=True, Q0=Lv, want_hist=False)
        assert q.tolist() == R.combine(Lv, Lc, K), f"lambda {lam}"
        _, _, q0 = gpu_color(frame, p, None, BOX1, 32, 8, tmpl, lam, K, combine=False, Q0=Lv, want_hist=False)
        assert np.array_equal(q0, Lc)
    assert {0, 1 << K} <= seen and (K != 40 or len(seen) > 4) and (K != 1 or 1 in seen)


# ------------------------------------------------------------------ workspace reuse, sub-ranges
def test_prefilled_workspace_equals_a_fresh_one():
    """fill_ws = 0 after crop_patches on the same frame (the tracker's case; the frame pointer is NULL) equals
    fill_ws = 1."""
    from vitparticlefiltertracker_amd import ops
    frame = _frame(H1, W1, 77)
    p, ang = _states(20), _angles(20)
    tmpl = R.template(frame, (14.0, 13.0, 20.0, 14.0), None, 32, 8)
    ws = ops.rgba_workspace(frame.shape[:2], DEV)
    ws.fill_(0x00FFFFFF)                                        # stale contents the crop must replace
    out = torch.empty(20 * 4, 768, device=DEV)
    vpf().crop_patches(torch.from_numpy(frame).to(DEV), ws, torch.from_numpy(p).to(DEV), list(BOX1), 32, 16,
                       [1.0, 1.0, 1.0, 0.0, 0.0, 0.0], out)
    for a in (None, ang):
        fresh = gpu_color(frame, p, a, BOX1, 32, 8, tmpl)
        reused = gpu_color(frame, p, a, BOX1, 32, 8, tmpl, ws=ws, fill=False)
        assert np.array_equal(reused[0], fresh[0]) and np.array_equal(bits(reused[1]), bits(fresh[1]))
        assert np.array_equal(reused[2], fresh[2])
        assert np.array_equal(fresh[0], R.histograms(frame, p, a, BOX1, 32, 8))


def test_sub_range_equals_the_rows_of_the_full_call():
    """Shard independence: a call on columns [23, 50) of the same storage (pointer offset, smaller n, same row stride)
    gives the full call's rows, so no bit depends on how the particles are split over ranks."""
    from vitparticlefiltertracker_amd import ops
    frame = _frame(H1, W1, 5)
    p, ang = _states(67), _angles(67)
    tmpl = R.template(frame, (14.0, 13.0, 20.0, 14.0), None, 16, 16)
    pd, ad = torch.from_numpy(p).to(DEV), torch.from_numpy(ang).to(DEV)
    fd, ws, td = torch.from_numpy(frame).to(DEV), ops.rgba_workspace(frame.shape[:2], DEV), torch.from_numpy(tmpl).to(DEV)

    def run(lo, hi):
        n = hi - lo
        hist = torch.empty(n, 4096, device=DEV, dtype=torch.int32)
        rho, Q = torch.empty(n, device=DEV), torch.empty(n, device=DEV, dtype=torch.int64)
        vpf().color_weight(fd, ws, True, pd[:, lo:hi], ad[lo:hi], list(BOX1), [H1, W1], 16, 16, td, 20.0, K40, False,
                           hist, rho, Q)
        return hist.cpu().numpy(), rho.cpu().numpy(), Q.cpu().numpy()
    full, part = run(0, 67), run(23, 50)
    for f, s in zip(full, part):
        assert np.array_equal(f[23:50], s)
    assert np.array_equal(full[2], R.color_weights(frame, p, ang, BOX1, tmpl, 16, 16, 20.0, K40))


# ------------------------------------------------------------------ argument checks
def test_argument_checks_return_err_arg_and_launch_nothing():
    from vitparticlefiltertracker_amd import _lib, ops
    L = _lib.lib()
    n, nb = 4, 512
    fd = torch.zeros(H1, W1, 3, device=DEV, dtype=torch.uint8)
    ws = ops.rgba_workspace((H1, W1), DEV)
    ws.fill_(-1)
    pd = torch.from_numpy(_states(n)).to(DEV)
    td = torch.full((nb,), 1.0 / nb, device=DEV)
    hist = torch.full((n, nb), -1, device=DEV, dtype=torch.int32)
    rho = torch.full((n,), -5.0, device=DEV)
    Q = torch.full((n,), -1, device=DEV, dtype=torch.int64)
    good = dict(frame=fd.data_ptr(), H=H1, W=W1, ws=ws.data_ptr(), fill=1, p=pd.data_ptr(), ld=n, ang=None, n=n,
                w0=20.0, h0=14.0, grid=32, bins=8, tmpl=td.data_ptr(), lam=20.0, bits=K40, combine=0,
                hist=hist.data_ptr(), rho=rho.data_ptr(), Q=Q.data_ptr())

    def call(**over):
        a = {**good, **over}
        return L.vpf_color_weight(a["frame"], a["H"], a["W"], a["ws"], a["fill"], a["p"], a["ld"], a["ang"], a["n"],
                                  a["w0"], a["h0"], a["grid"], a["bins"], a["tmpl"], a["lam"], a["bits"], a["combine"],
                                  a["hist"], a["rho"], a["Q"], _lib.stream_ptr())
    bad = [dict(bins=5), dict(bins=32), dict(bins=0), dict(grid=24), dict(grid=128), dict(grid=4), dict(lam=-1.0),
           dict(lam=float("nan")), dict(lam=float("inf")), dict(bits=-1), dict(bits=62), dict(ld=n - 1), dict(n=-1),
           dict(ws=None), dict(frame=None), dict(p=None), dict(Q=None), dict(tmpl=None, hist=None), dict(H=0),
           dict(W=0), dict(H=65536, W=65536)]
    for over in bad:
        assert call(**over) == -1, over
    assert call(n=0, ld=0, p=None) == 0                       # nothing to do: no launch either
    torch.cuda.synchronize()
    assert (ws == -1).all() and (hist == -1).all() and (rho == -5.0).all() and (Q == -1).all(), "a refused call launched"
    assert call() == 0 and call(frame=None, fill=0) == 0 and call(tmpl=None, Q=None) == 0
    torch.cuda.synchronize()
    assert (hist.sum(dim=1) == 1024).all() and (Q >= 0).all()
    # the op's own checks
    with pytest.raises(ValueError):
        vpf().color_weight(fd, ws, True, pd, None, [20.0, 14.0], [H1, W1], 32, 5, td, 20.0, K40, False, hist, rho, Q)
    with pytest.raises(ValueError):
        vpf().color_weight(None, ws, True, pd, None, [20.0, 14.0], [H1, W1], 32, 8, td, 20.0, K40, False, hist, rho, Q)
    with pytest.raises(ValueError):
        vpf().color_weight(fd, ws[:100], True, pd, None, [20.0, 14.0], [H1, W1], 32, 8, td, 20.0, K40, False, hist, rho, Q)


# ------------------------------------------------------------------ degenerate scales, angles outside the circle
@pytest.mark.parametrize("rot", [False, True], ids=["s3", "s12"])
@pytest.mark.parametrize("C,B", [(8, 4), (32, 8)])
def test_degenerate_scales_and_angles_outside_the_circle(C, B, rot):
    """Scale 0: all C^2 samples are the one point (x - 0.5, y - 0.5), here the pixel (20, 17), so they fill ONE bin, the
    bin of that pixel's bytes (closed form), and the reference agrees. Scales -1 and -1.37 (mirrored grids) and, with an
    angle row, the angles -0.0, +-1e-9, +-2 pi, 7 pi / 2, +-100, +-1e6 and +-3e38: the reference's counts, rho bits and Q.
    A NaN scale or a NaN angle: the values are NaN and their bins the device's conversion of NaN, so only the count's
    sum C^2 and non-negative counts are asserted. The ordinary particles in between are exact."""
    import crop_rot_cases as K
    frame = _frame(H1, W1, 60 + C)
    kinds, p, ang = K.color_states(rot)
    fin = [i for i, k in enumerate(kinds) if k != "nan"]
    nan = [i for i, k in enumerate(kinds) if k == "nan"]
    assert len(nan) == (2 if rot else 1)
    tmpl = R.template(frame, (14.0, 13.0, 20.0, 14.0), None, C, B)
    h_ref = R.histograms(frame, np.ascontiguousarray(p[:, fin]), None if ang is None else ang[fin], BOX1, C, B)
    r_ref = R.rho(h_ref, tmpl, C)
    q_ref = R.weights(r_ref, 20.0, K40)
    zero = fin.index(kinds.index("zero"))
    one = K.one_pixel_bin(frame, 20, 17, B)
    assert h_ref[zero, one] == C * C and h_ref[zero].sum() == C * C
    if rot:
        a0 = fin.index(kinds.index("angle"))
        row = lambda a: h_ref[a0 + K.ANGLES.index(a)].tobytes()
        assert all(row(a) == row(0.0) for a in K.SAME_AS_ZERO) and all(row(a) != row(0.0) for a in K.NOT_ZERO)
    h, r, q = gpu_color(frame, p, ang, BOX1, C, B, tmpl, pad=3)
    assert h[kinds.index("zero"), one] == C * C
    bad = np.flatnonzero((h[fin] != h_ref).any(axis=1))
    assert bad.size == 0, f"histograms differ at finite particles {[fin[i] for i in bad[:8]]} ({[kinds[fin[i]] for i in bad[:8]]})"
    assert np.array_equal(bits(r[fin]), bits(r_ref)), np.flatnonzero(bits(r[fin]) != bits(r_ref))[:8]
    assert np.array_equal(q[fin], q_ref)
    assert (h[nan].sum(axis=1) == C * C).all() and (h[nan] >= 0).all()
