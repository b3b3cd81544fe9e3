"""GPU (MI355X): SPEC S14's kernel — vpf_color_weight_surround's box and ring counts, both scores and the combined
weight bit for bit against the numpy reference (tests/s14_reference.py): the smallest and largest grid, one bin per lane
and the single-histogram path, S3 and S12 coordinates, with and without the ViT weight; rings in the zero padding, out
of the frame on all sides, and a non-finite state; the box's outputs against vpf_color_weight's; the histogram-only
form, n == 0 and every argument check. Run: python -m pytest tests -m gpu."""
import math
import random

import numpy as np
import pytest
import torch

import s13_reference as R13
import s14_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
K40 = 40
H1, W1, BOX1 = 40, 48, (20.0, 14.0)          # a 48 x 40 frame, a non-square template box
TBOX = (14.0, 13.0, 20.0, 14.0)              # the template's box, inside the frame
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


def _frame(seed):
    return np.random.default_rng(seed).integers(0, 256, (H1, W1, 3), dtype=np.uint8)


# five states: fractional and inside; at the frame's corner (the ring mostly zero padding); scale 2 (box 40 x 28, the
# doubled box 80 x 56: the ring leaves the 48 x 40 frame on all sides); a non-finite one (Q = 0); across the left edge
STATES5 = np.ascontiguousarray(np.array([[20.5, 17.25, 0.77], [47.0, 39.0, 1.0], [24.0, 20.0, 2.0],
                                         [np.nan, 20.0, 1.0], [2.0, 20.0, 1.37]], np.float32).T)
ANGLES5 = np.array([0.3, -PI / 2, 0.0, 0.2, -0.3], np.float32)
FINITE5 = [0, 1, 2, 4]


def _to(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def gpu_surround(frame, p, ang, box, C, B, tmpl, lam_c=20.0, lam_s=10.0, K=K40, combine=False, Q0=None, pad=0,
                 want=("h", "hs")):
    """vpf.color_weight_surround on particles float32[3][n] stored with row stride n + pad; a dict of numpy results."""
    from vitparticlefiltertracker_amd import ops
    n, nb = p.shape[1], B ** 3
    store = torch.full((3, n + pad), 7.0, device=DEV)
    store[:, :n] = torch.from_numpy(p)
    view = store[:, :n]
    assert n == 0 or pad == 0 or view.stride(0) == n + pad
    ws = ops.rgba_workspace(frame.shape[:2], DEV)
    h = torch.full((n, nb), -1, device=DEV, dtype=torch.int32) if "h" in want else None
    hs = torch.full((n, nb), -1, device=DEV, dtype=torch.int32) if "hs" in want else None
    rho = rho_s = Q = None
    if tmpl is not None:
        rho, rho_s = torch.full((n,), -5.0, device=DEV), torch.full((n,), -5.0, device=DEV)
        Q = _to(Q0, np.int64) if Q0 is not None else torch.full((n,), -1, device=DEV, dtype=torch.int64)
    vpf().color_weight_surround(_to(frame), ws, True, view, _to(ang), [float(box[0]), float(box[1])],
                                [frame.shape[0], frame.shape[1]], C, B, _to(tmpl), float(lam_c), float(lam_s), K,
                                combine, h, hs, rho, rho_s, Q)
    torch.cuda.synchronize()
    assert (store[:, n:] == 7.0).all()
    out = {"h": h, "hs": hs, "rho": rho, "rho_s": rho_s, "Q": Q}
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _check(frame, p, ang, box, C, B, tmpl, lam_c, lam_s, combine, pad, tag):
    n = p.shape[1]
    ref = R.cue(frame, p, ang, box, tmpl, C, B, lam_c, lam_s, K40)
    rnd = random.Random(C * B + n)
    Lv = [0, 1 << K40, (1 << K40) - 1] + [rnd.randrange(0, (1 << K40) + 1) for _ in range(n)]
    Lv = Lv[:n]
    want = R.combine(Lv if combine else None, ref["Lc"], ref["Ls"], K40)
    got = gpu_surround(frame, p, ang, box, C, B, tmpl, lam_c, lam_s, K40, combine, Q0=Lv, pad=pad)
    for key, cnt in (("h", C * C), ("hs", 3 * C * C // 4)):
        bad = np.flatnonzero((got[key] != ref[key]).any(axis=1))
        assert bad.size == 0, f"{tag}: {key} differs at particles {bad[:8]}"
        assert (got[key].sum(axis=1) == cnt).all()
    for key in ("rho", "rho_s"):
        assert np.array_equal(bits(got[key]), bits(ref[key])), \
            f"{tag}: {key} differs at {np.flatnonzero(bits(got[key]) != bits(ref[key]))[:8]}: {got[key]} {ref[key]}"
    assert got["Q"].tolist() == want, f"{tag}: Q differs"
    return ref, got, want


# ------------------------------------------------------------------ counts, scores, weights
@pytest.mark.parametrize("combine", [False, True], ids=["colour-only", "combined"])
@pytest.mark.parametrize("rot", [False, True], ids=["s3", "s12"])
@pytest.mark.parametrize("C,B", [(8, 4), (8, 16), (64, 4), (64, 16), (32, 8)])
def test_surround_equals_reference(C, B, rot, combine):
    """Five particles, row stride 8. C = 8: 64 + 48 samples, fewer than the workgroup's threads; C = 64: 28 per thread.
    B = 4: one bin per lane of the scoring waves, a histogram pair per wave; B = 16: one pair, 2 x 16 KiB. The corner
    and scale-2 rings count zero padding into bin 0; the non-finite state has rho_s = NaN and Q = 0."""
    frame = _frame(10 * B + C)
    ang = ANGLES5 if rot else None
    tmpl = R13.template(frame, TBOX, None if ang is None else np.float32(0.3), C, B)
    ref, got, want = _check(frame, STATES5, ang, BOX1, C, B, tmpl, 20.0, 10.0, combine, pad=3,
                            tag=f"C {C} B {B} rot {rot} combine {combine}")
    assert np.isnan(got["rho_s"][3]) and got["Q"][3] == 0
    assert ref["hs"][1, 0] > 3 * C * C // 8, "the corner ring is not mostly padding"
    assert ref["hs"][2, 0] >= 3 * C * C // 16, "the scale-2 ring does not leave the frame"
    if rot is False and combine is False:
        assert len({want[i] for i in FINITE5}) > 1, "every weight equal: the case tests nothing"


@pytest.mark.parametrize("rot", [False, True], ids=["s3", "s12"])
def test_many_particles_on_the_uncovered_grid(rot):
    """40 particles (row stride 53) at C = 16, B = 8: hand-placed edge states and random ones up to 12 px outside."""
    rng = np.random.default_rng(3)
    n = 40
    rnd = np.stack([rng.uniform(-12, W1 + 12, n), rng.uniform(-12, H1 + 12, n), rng.uniform(0.5, 2.0, n)]).astype(np.float32)
    p = np.ascontiguousarray(np.concatenate([STATES5, rnd], axis=1)[:, :n])
    ang = np.resize(np.array([0.0, 0.3, -0.3, PI / 2, -PI / 2], np.float32), n) if rot else None
    frame = _frame(77)
    tmpl = R13.template(frame, TBOX, None, 16, 8)
    ref, got, want = _check(frame, p, ang, BOX1, 16, 8, tmpl, 20.0, 10.0, True, pad=13, tag=f"n 40 rot {rot}")
    assert len(set(ref["Ls"].tolist())) > 10


FAR_HW, FAR_BOX, FAR_C, FAR_B = (24, 32), (10.0, 8.0), 8, 4
FAR_STATES = np.ascontiguousarray(np.array(
    [[16.0, 12.0, 1.0], [3e9, 12.0, 1.0], [10.5, 9.25, 1.2], [16.0, -3e9, 1.0], [np.inf, 12.0, 1.0], [20.0, 14.0, 0.8],
     [16.0, -np.inf, 1.0], [14.0, 10.0, 1.0]], np.float32).T)
FAR_ORDINARY, FAR_HUGE, FAR_INF = [0, 2, 5, 7], [1, 3], [4, 6]


@pytest.mark.parametrize("rot", [False, True], ids=["s3", "s12"])
def test_states_beyond_the_int_range_count_padding_only(rot):
    """SPEC S3's last paragraph, for both grids of the cue: at a coordinate of +-3e9 every tap of the box and of the
    ring is clamped into the zero border, so all C^2 and all 3 C^2 / 4 samples fall in bin 0 (closed form: the numpy
    reference's float -> int conversion is not defined there); at +-inf the values are NaN and only the counts'
    sums are asserted. The ordinary particles between them are the reference's counts exactly. The op raises on a
    non-zero status."""
    frame = np.random.default_rng(31).integers(0, 256, (*FAR_HW, 3), dtype=np.uint8)
    ang = np.full(8, 0.3, np.float32) if rot else None
    CC, RC = FAR_C * FAR_C, 3 * FAR_C * FAR_C // 4
    p_ord, a_ord = FAR_STATES[:, FAR_ORDINARY].copy(), None if ang is None else ang[FAR_ORDINARY]
    ref = R.histograms(frame, p_ord, a_ord, FAR_BOX, FAR_C, FAR_B)
    ref_s = R.ring_histograms(frame, p_ord, a_ord, FAR_BOX, FAR_C, FAR_B)
    assert (ref[:, 0] < CC).all(), "an ordinary box counts only bin 0: the case tests nothing"
    got = gpu_surround(frame, FAR_STATES, ang, FAR_BOX, FAR_C, FAR_B, None, pad=3)
    h, hs = got["h"], got["hs"]
    assert np.array_equal(h[FAR_ORDINARY], ref) and np.array_equal(hs[FAR_ORDINARY], ref_s)
    assert (h[FAR_HUGE, 0] == CC).all() and not h[FAR_HUGE, 1:].any()
    assert (hs[FAR_HUGE, 0] == RC).all() and not hs[FAR_HUGE, 1:].any()
    assert (h[FAR_INF].sum(axis=1) == CC).all() and (hs[FAR_INF].sum(axis=1) == RC).all()
    assert (h[FAR_INF] >= 0).all() and (hs[FAR_INF] >= 0).all()


def test_exact_anchors_on_the_device():
    """A one-colour frame: a box and ring inside it fall in the template's single bin: rho = rho_s = 1 and
    Q = floor(fixed_expf(-lambda_s) 2^K); the same ring against a template that shares no bin: rho_s = +0, Ls = 2^K,
    Q = Lc; a ring wholly in the padding: rho_s = +0 too."""
    frame = np.empty((H1, W1, 3), np.uint8)
    frame[...] = (200, 100, 50)
    p = np.ascontiguousarray(np.array([[24.0, 20.0, 0.5], [-200.0, -200.0, 1.0]], np.float32).T)
    tmpl = R13.template(frame, TBOX, None, 16, 8)
    e = int(R.opf.weights_to_Q(np.array([0.0], np.float32), 10.0, K40)[0])
    got = gpu_surround(frame, p, None, BOX1, 16, 8, tmpl)
    assert bits(got["rho_s"]).tolist() == [bits(np.float32(1.0))[0], 0] and got["rho"][0] == 1.0
    assert got["Q"].tolist() == [e, int(R13.weights(got["rho"][1:], 20.0, K40)[0])]
    other = np.zeros(512, np.float32)
    other[3] = 1.0
    got = gpu_surround(frame, p, None, BOX1, 16, 8, other)
    assert bits(got["rho_s"]).tolist() == [0, 0] and bits(got["rho"]).tolist() == [0, 0]
    assert got["Q"].tolist() == [int(R13.weights(np.zeros(1, np.float32), 20.0, K40)[0])] * 2


# ------------------------------------------------------------------ against vpf_color_weight
@pytest.mark.parametrize("rot", [False, True], ids=["s3", "s12"])
@pytest.mark.parametrize("C,B", [(8, 16), (64, 4), (32, 8)])
def test_box_outputs_equal_color_weight_and_lambda_zero_equals_its_q(C, B, rot):
    """The box's histogram and rho are vpf_color_weight's on the same inputs, bit for bit (the non-finite state
    included); at lambda_s = 0 the final Q is its Q on every finite state, combined and colour only."""
    from vitparticlefiltertracker_amd import ops
    frame = _frame(C + B)
    ang = ANGLES5 if rot else None
    tmpl = R13.template(frame, TBOX, None, C, B)
    Lv = [1 << K40, 12345678901, (1 << K40) - 1, 1 << K40, 0x5A5A5A5A5A]
    for combine in (False, True):
        got = gpu_surround(frame, STATES5, ang, BOX1, C, B, tmpl, 20.0, 0.0, K40, combine, Q0=Lv)
        n, nb = 5, B ** 3
        h = torch.full((n, nb), -1, device=DEV, dtype=torch.int32)
        rho, Q = torch.full((n,), -5.0, device=DEV), _to(Lv, np.int64)
        vpf().color_weight(_to(frame), ops.rgba_workspace((H1, W1), DEV), True, _to(STATES5), _to(ang), list(BOX1),
                           [H1, W1], C, B, _to(tmpl), 20.0, K40, combine, h, rho, Q)
        torch.cuda.synchronize()
        assert np.array_equal(got["h"], h.cpu().numpy())
        assert np.array_equal(bits(got["rho"]), bits(rho.cpu().numpy()))
        assert np.array_equal(got["Q"][FINITE5], Q.cpu().numpy()[FINITE5])
        assert got["Q"][3] == 0 and np.isnan(got["rho_s"][3])


# ------------------------------------------------------------------ histogram-only form, n == 0, argument checks
def test_histograms_only_without_a_template():
    frame = _frame(3)
    for ang in (None, ANGLES5):
        for want in (("h", "hs"), ("hs",), ("h",)):
            got = gpu_surround(frame, STATES5, ang, BOX1, 16, 4, None, want=want)
            assert got["rho"] is None and got["Q"] is None
            if "h" in want:
                assert np.array_equal(got["h"], R.histograms(frame, STATES5, ang, BOX1, 16, 4))
            if "hs" in want:
                assert np.array_equal(got["hs"], R.ring_histograms(frame, STATES5, ang, BOX1, 16, 4))


def test_argument_checks_return_err_arg_and_launch_nothing():
    from vitparticlefiltertracker_amd import _lib, ops
    L = _lib.lib()
    n, nb = 4, 512
    fd = torch.zeros(H1, W1, 3, device=DEV, dtype=torch.uint8)
    ws = ops.rgba_workspace((H1, W1), DEV)
    ws.fill_(-1)
    pd = _to(STATES5[:, [0, 1, 2, 4]])
    td = torch.full((nb,), 1.0 / nb, device=DEV)
    h = torch.full((n, nb), -1, device=DEV, dtype=torch.int32)
    hs = torch.full((n, nb), -1, device=DEV, dtype=torch.int32)
    rho, rho_s = torch.full((n,), -5.0, device=DEV), torch.full((n,), -5.0, device=DEV)
    Q = torch.full((n,), -1, device=DEV, dtype=torch.int64)
    good = dict(frame=fd.data_ptr(), H=H1, W=W1, ws=ws.data_ptr(), fill=1, p=pd.data_ptr(), ld=n, ang=None, n=n,
                w0=20.0, h0=14.0, grid=32, bins=8, tmpl=td.data_ptr(), lam=20.0, lam_s=10.0, bits=K40, combine=0,
                h=h.data_ptr(), hs=hs.data_ptr(), rho=rho.data_ptr(), rho_s=rho_s.data_ptr(), Q=Q.data_ptr())

    def call(**over):
        a = {**good, **over}
        return L.vpf_color_weight_surround(a["frame"], a["H"], a["W"], a["ws"], a["fill"], a["p"], a["ld"], a["ang"],
                                           a["n"], a["w0"], a["h0"], a["grid"], a["bins"], a["tmpl"], a["lam"],
                                           a["lam_s"], a["bits"], a["combine"], a["h"], a["hs"], a["rho"], a["rho_s"],
                                           a["Q"], _lib.stream_ptr())
    bad = [dict(bins=5), dict(bins=32), dict(bins=0), dict(grid=24), dict(grid=128), dict(grid=4), dict(lam=-1.0),
           dict(lam=float("nan")), dict(lam=float("inf")), dict(lam_s=-1.0), dict(lam_s=float("nan")),
           dict(lam_s=float("inf")), dict(bits=-1), dict(bits=62), dict(ld=n - 1), dict(n=-1), dict(ws=None),
           dict(frame=None), dict(p=None), dict(Q=None), dict(tmpl=None, h=None, hs=None), dict(H=0), dict(W=0),
           dict(H=65536, W=65536)]
    for over in bad:
        assert call(**over) == -1, over
    assert call(n=0, ld=0, p=None) == 0                       # nothing to do: no launch either
    torch.cuda.synchronize()
    for t, v in ((ws, -1), (h, -1), (hs, -1), (rho, -5.0), (rho_s, -5.0), (Q, -1)):
        assert (t == v).all(), "a refused call launched"
    assert call() == 0 and call(frame=None, fill=0) == 0 and call(tmpl=None, Q=None, h=None) == 0
    assert call(h=None, hs=None, rho=None, rho_s=None) == 0   # every optional output absent
    torch.cuda.synchronize()
    assert (h.sum(dim=1) == 1024).all() and (hs.sum(dim=1) == 768).all() and (Q >= 0).all()
    # the op: n == 0 and its own checks
    e = torch.empty(3, 0, device=DEV)
    vpf().color_weight_surround(fd, ws, True, e, None, [20.0, 14.0], [H1, W1], 32, 8, td, 20.0, 10.0, K40, False, None,
                                None, None, None, Q[:0])
    args = ([20.0, 14.0], [H1, W1])
    with pytest.raises(ValueError):
        vpf().color_weight_surround(fd, ws, True, pd, None, *args, 32, 5, td, 20.0, 10.0, K40, False, h, hs, rho, rho_s, Q)
    with pytest.raises(ValueError):
        vpf().color_weight_surround(None, ws, True, pd, None, *args, 32, 8, td, 20.0, 10.0, K40, False, h, hs, rho, rho_s, Q)
    with pytest.raises(ValueError):
        vpf().color_weight_surround(fd, ws[:100], True, pd, None, *args, 32, 8, td, 20.0, 10.0, K40, False, h, hs, rho,
                                    rho_s, Q)
    with pytest.raises(ValueError):
        vpf().color_weight_surround(fd, ws, True, pd, None, *args, 32, 8, td, 20.0, 10.0, K40, False, h, hs[:1], rho,
                                    rho_s, Q)
    with pytest.raises(ValueError):
        vpf().color_weight_surround(fd, ws, True, pd, None, *args, 32, 8, td, 20.0, 10.0, K40, False, h, hs, rho,
                                    rho_s[:2], Q)


# ------------------------------------------------------------------ degenerate scales, angles outside the circle
@pytest.mark.parametrize("rot", [False, True], ids=["s3", "s12"])
@pytest.mark.parametrize("C,B", [(8, 4), (32, 8)])
def test_degenerate_scales_and_angles_outside_the_circle(C, B, rot):
    """test_s13_gpu_kernels.py's degenerate states through both grids of the cue. Scale 0: the box's C^2 samples and the
    ring's 3 C^2 / 4 (the doubled box of a zero box is the same point) all fall in the bin of the pixel (20, 17)
    (closed form), and the reference agrees. Scales -1 and -1.37 and, with an angle row, every angle outside the
    circle: the reference's counts, rho and rho_s bits and Q. A NaN scale or a NaN angle: rho_s is NaN and Q == 0. The
    ordinary particles in between are exact."""
    import crop_rot_cases as K
    frame = _frame(60 + C)
    kinds, p, ang = K.color_states(rot)
    fin = [i for i, k in enumerate(kinds) if k != "nan"]
    nan = [i for i, k in enumerate(kinds) if k == "nan"]
    assert len(nan) == (2 if rot else 1)
    tmpl = R13.template(frame, TBOX, None, C, B)
    ref = R.cue(frame, np.ascontiguousarray(p[:, fin]), None if ang is None else ang[fin], BOX1, tmpl, C, B, 20.0, 10.0,
                K40)
    want = R.combine(None, ref["Lc"], ref["Ls"], K40)
    zero, one = fin.index(kinds.index("zero")), K.one_pixel_bin(frame, 20, 17, B)
    assert ref["h"][zero, one] == C * C and ref["hs"][zero, one] == 3 * C * C // 4
    if rot:
        a0 = fin.index(kinds.index("angle"))
        row = lambda a: ref["hs"][a0 + K.ANGLES.index(a)].tobytes()
        assert all(row(a) == row(0.0) for a in K.SAME_AS_ZERO) and all(row(a) != row(0.0) for a in K.NOT_ZERO)
    got = gpu_surround(frame, p, ang, BOX1, C, B, tmpl, 20.0, 10.0, K40, False, pad=3)
    z = kinds.index("zero")
    assert got["h"][z, one] == C * C and got["hs"][z, one] == 3 * C * C // 4
    for key in ("h", "hs"):
        bad = np.flatnonzero((got[key][fin] != ref[key]).any(axis=1))
        assert bad.size == 0, f"{key} differs at finite particles {[fin[i] for i in bad[:8]]}"
    for key in ("rho", "rho_s"):
        assert np.array_equal(bits(got[key][fin]), bits(ref[key])), key
    assert got["Q"][fin].tolist() == want
    assert np.isnan(got["rho_s"][nan]).all() and (got["Q"][nan] == 0).all()
    assert (got["h"][nan].sum(axis=1) == C * C).all() and (got["hs"][nan].sum(axis=1) == 3 * C * C // 4).all()
