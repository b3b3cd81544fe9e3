"""GPU (MI355X): the unrotated crop (SPEC S3; vpf_crop_patches_f32 / _bf16, csrc/crop.hip) bit for bit against
oracle.pf.crop_patches, the bf16 output as its RNE rounding: both kernel forms and every store width, every workgroup
split, windows on either side of the LDS budget (the branch asserted from tests/crop_reference.py's geometry), windows
cut by the frame, the degenerate states of S3's last paragraph mixed into ordinary batches, closed forms that do not go
through the oracle, and ld > n and the rejections through the C ABI. Every output is pre-filled with 7.0 and is a
leading view of a buffer whose tail rows hold -9.0 and must survive. Run: python -m pytest tests -m gpu."""
import numpy as np
import pytest
import torch

import crop_reference as C
from oracle import pf as opf

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL, GUARD, GUARD_ROWS = 7.0, -9.0, 5
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()
    assert torch.cuda.is_available()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bf16_rne(x):
    """The bf16 bit patterns (uint16) of finite fp32 values, round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _norm_ab(mean, std):
    a, b = opf.norm_affine(mean, std)
    return [float(v) for v in a] + [float(v) for v in b]


def _frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _host(t):
    """fp32 values, or the uint16 bit patterns of a bf16 tensor."""
    return t.cpu().numpy() if t.dtype == torch.float32 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def _guard_intact(buf, rows, tag):
    tail = _host(buf[rows:])
    want = np.float32(GUARD) if buf.dtype == torch.float32 else bf16_rne(np.float32(GUARD))
    assert tail.shape[0] == GUARD_ROWS and np.all(tail == want), f"{tag}: rows past the output's end were written"


def _gpu_crop(frame, p, box, S, patch, kp, dtype, mean=MEAN, std=STD):
    """The op on a sentinel-filled leading view of a guarded buffer: fp32 values or bf16 bit patterns [n g^2][kp]."""
    from vitparticlefiltertracker_amd import ops
    n, g = p.shape[1], S // patch
    rows = n * g * g
    buf = torch.full((rows + GUARD_ROWS, kp), GUARD, device=DEV, dtype=dtype)
    out = buf[:rows]
    out.fill_(SENTINEL)
    torch.ops.vpf.crop_patches(torch.from_numpy(frame).to(DEV), ops.rgba_workspace(frame.shape[:2], DEV),
                               torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(DEV),
                               [float(box[0]), float(box[1])], S, patch, _norm_ab(mean, std), out)
    _guard_intact(buf, rows, f"S={S} patch={patch} kp={kp} {dtype}")
    return _host(out)


def _assert_rows(got, ref, dtype, S, patch, tag, rows=None):
    """got == ref (fp32 bits), or got == RNE(ref) (bf16 bits), over `rows` (default: all); names the first bad cell."""
    want = bits(ref) if dtype == torch.float32 else bf16_rne(ref)
    have = bits(got) if dtype == torch.float32 else got
    sel = np.arange(ref.shape[0]) if rows is None else np.asarray(rows)
    bad = np.argwhere(have[sel] != want[sel])
    if bad.size:
        r, c = int(sel[bad[0][0]]), int(bad[0][1])
        raise AssertionError(f"{tag} {dtype}: {len(bad)} cells differ from the reference, first at "
                             f"{C.where(r, c, S, patch)}: got bits {int(have[r, c]):#x}, want {int(want[r, c]):#x}")


def _check(frame, p, box, S, patch, kp, tag, mean=MEAN, std=STD):
    """Both dtypes against the oracle; the padding columns exactly +0 over the sentinel. Returns the reference."""
    ref = opf.crop_patches(frame, p, box, S, patch, kp, mean, std)
    K = 3 * patch * patch
    assert not bits(ref[:, K:]).any()
    for dtype in DTYPES:
        got = _gpu_crop(frame, p, box, S, patch, kp, dtype, mean, std)
        _assert_rows(got, ref, dtype, S, patch, tag)
        assert not got[:, K:].view(np.uint32 if dtype == torch.float32 else np.uint16).any(), f"{tag}: padding not +0"
    return ref


def _particle_rows(idx, g2):
    return (np.asarray(idx).reshape(-1, 1) * g2 + np.arange(g2).reshape(1, -1)).reshape(-1)


# ------------------------------------------------------------------ a. every form and store width
H1, W1, BOX1 = 96, 128, (40.0, 30.0)
SIX = np.array([[60.0, 64.5, -40.0, W1 - 1.0, 30.0, 100.0],         # test_s12_gpu_kernels.py's SIX
                [50.0, 47.25, -40.0, H1 - 1.0, 70.0, 20.0],
                [1.0, 1.37, 0.5, 2.0, 0.5, 1.37]], np.float32)
FORMS = [(32, 16, 768, "lds8"), (16, 8, 192, "lds8"), (32, 8, 256, "row"), (28, 14, 640, "row"), (28, 7, 192, "row"),
         (24, 12, 448, "row")]


@pytest.mark.parametrize("S,patch,kp,form", FORMS)
def test_crop_every_form_and_store_width(S, patch, kp, form):
    """(32, 16, 768) and (16, 8, 192): the 8-pixel form, 16-B stores. (32, 8, 256): patch % 8 == 0 but Kp > 3 patch^2,
    so the per-row kernel with 64 padding columns. (28, 14, 640): per-row, bf16 pairs. (28, 7, 192): odd patch, element
    stores. (24, 12, 448): per-row. Six particles: the far corner, (-40, -40) entirely in the border (its rows hold b_c
    only), the scales 0.5, 1.37 and 2; all staged."""
    assert C.kernel_form(patch, kp) == form
    assert C.window(SIX, BOX1, S, H1, W1)["staged"].all()
    ref = _check(_frame(H1, W1, S + patch), SIX, BOX1, S, patch, kp, f"S={S} patch={patch} kp={kp}")
    g2, pp = (S // patch) ** 2, patch * patch
    _, b = opf.norm_affine(MEAN, STD)
    border = ref[2 * g2:3 * g2, : 3 * pp].reshape(g2, 3, pp)
    assert all(np.all(border[:, c] == b[c]) for c in range(3))
    assert len({ref[k * g2:(k + 1) * g2].tobytes() for k in range(6)}) == 6


# ------------------------------------------------------------------ b. every split share
@pytest.mark.parametrize("n", [6, 1023, 1024, 2047, 2048])
def test_crop_every_split_share(n):
    """The 8-pixel form's launch shapes on both sides of each threshold: four workgroups per particle (n = 6, 1023),
    two (1024, 2047), one (2048, the production launch), at S = 16, patch = 8. Centres in and around the frame, scales
    over [0.5, 2]."""
    rng = np.random.default_rng(n)
    p = np.stack([rng.uniform(-10, W1 + 10, n), rng.uniform(-10, H1 + 10, n), rng.uniform(0.5, 2.0, n)]).astype(np.float32)
    assert C.kernel_form(8, 192) == "lds8" and C.split_of(n) == {6: 4, 1023: 4, 1024: 2, 2047: 2, 2048: 1}[n]
    assert C.window(p, (24.0, 18.0), 16, H1, W1)["staged"].all()
    _check(_frame(H1, W1, 11), p, (24.0, 18.0), 16, 8, 192, f"n={n}")


# ------------------------------------------------------------------ c. the LDS budget
BUDGET = [((100.0, 100.0), (79.5, 129.25), (80, 128)), ((100.5, 100.5), (76.5, 134.25), (77, 133))]


@pytest.mark.parametrize("patch,kp", [(16, 768), (8, 256)])
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("centre,box,sides", BUDGET)
def test_crop_window_at_and_over_the_lds_budget(centre, box, sides, transpose, patch, kp):
    """Frame 200 x 200, S = 32, scale 1. An 80 x 128 window is exactly CROP_LDS_DW = 10240 dwords, the last size that is
    staged; a 77 x 133 window is 10241, the first that takes the global taps; and their transposes. The branch is
    asserted from the restated geometry. A small staged particle rides along on each side."""
    H = W = 200
    if transpose:
        centre, box, sides = centre[::-1], box[::-1], sides[::-1]
    p = np.array([[30.0, centre[0], 150.0], [40.0, centre[1], 160.0], [0.25, 1.0, 0.25]], np.float32)
    w = C.window(p, box, 32, H, W)
    assert (w["wx"][1], w["wy"][1]) == sides and w["px"][1] == sides[0] * sides[1]
    assert w["staged"].tolist() == [True, sides[0] * sides[1] <= C.CROP_LDS_DW, True]
    assert w["px"][1] - C.CROP_LDS_DW == (0 if sides[0] * sides[1] == 10240 else 1)
    _check(_frame(H, W, 3), p, box, 32, patch, kp, f"window {sides}")


# ------------------------------------------------------------------ d. windows cut by the frame
@pytest.mark.parametrize("S,patch,kp", [(16, 8, 192), (28, 7, 192)])
def test_crop_windows_cut_by_the_frame(S, patch, kp):
    """Boxes hanging over each edge and each corner: the window starts in the left / top border (cx0 = -1, cy0 = -1) or
    ends in the right / bottom one (cx1 = W, cy1 = H), asserted. Then centres 10^6 px off each side (past the staging
    bound, global taps) and 2 x 10^5 px off (staged: a window one border column or row wide): every tap is padding, so
    every value is exactly b_c."""
    H, W, box = H1, W1, BOX1
    xs = [0.0, W, W / 2, W / 2, 0.0, W, 0.0, W]
    ys = [H / 2, H / 2, 0.0, H, 0.0, 0.0, H, H]
    far = [(-1e6, 50.0), (W + 1e6, 50.0), (50.0, -1e6), (50.0, H + 1e6),
           (-2e5, 50.0), (W + 2e5, 50.0), (50.0, -2e5), (50.0, H + 2e5)]
    p = np.array([xs + [f[0] for f in far], ys + [f[1] for f in far], [1.0] * 16], np.float32)
    w = C.window(p, box, S, H, W)
    assert w["cx0"][[0, 4, 6]].tolist() == [-1] * 3 and w["cx1"][[1, 5, 7]].tolist() == [W] * 3
    assert w["cy0"][[2, 4, 5]].tolist() == [-1] * 3 and w["cy1"][[3, 6, 7]].tolist() == [H] * 3
    assert w["staged"].tolist() == [True] * 8 + [False] * 4 + [True] * 4
    assert (np.minimum(w["wx"], w["wy"])[8:] == 1).all()
    assert w["cx0"][8:10].tolist() == [-1, W] and w["cy0"][10:12].tolist() == [-1, H]
    ref = _check(_frame(H, W, 21), p, box, S, patch, kp, "cut windows")
    g2, pp = (S // patch) ** 2, patch * patch
    _, b = opf.norm_affine(MEAN, STD)
    want = np.repeat(b, pp)
    assert np.array_equal(bits(ref[8 * g2:, : 3 * pp]), bits(np.broadcast_to(want, (8 * g2, 3 * pp))))
    assert all(ref[k * g2:(k + 1) * g2, : 3 * pp].std() > 0.1 for k in range(8))     # the first eight see the frame


# ------------------------------------------------------------------ e. degenerate states
ORD = [(60.0, 50.0, 1.0), (64.5, 47.25, 1.37), (100.0, 20.0, 0.5), (30.0, 70.0, 2.0)]
INF, NAN = float("inf"), float("nan")
DEGENERATE = [
    ("zero", (64.3, 47.7, 0.0)), ("ord", ORD[0]),
    ("mirror", (60.0, 50.0, -1.0)), ("mirror", (5.0, 4.0, -1.37)), ("ord", ORD[1]),      # near the top-left corner
    ("far", (3e9, 50.0, 1.0)), ("far", (-3e9, 50.0, 1.0)), ("far", (60.0, -3e9, 1.0)), ("far", (60.0, 3e9, 1.0)),
    ("ord", ORD[2]),
    ("nan", (NAN, 50.0, 1.0)), ("nan", (INF, 50.0, 1.0)), ("nan", (-INF, 50.0, 1.0)), ("ord", ORD[3]),
    ("nan", (60.0, NAN, 1.0)), ("nan", (60.0, INF, 1.0)), ("nan", (60.0, -INF, 1.0)), ("ord", ORD[0]),
    ("nan", (60.0, 50.0, NAN)), ("nan", (60.0, 50.0, INF)), ("nan", (60.0, 50.0, -INF)), ("ord", ORD[1]),
]


@pytest.mark.parametrize("S,patch,kp", [(32, 16, 768), (32, 8, 256), (28, 7, 192)])
def test_crop_degenerate_states_between_ordinary_particles(S, patch, kp):
    """SPEC S3's last paragraph, one call: scale 0 (every sample at (x - 0.5, y - 0.5): one value per channel, the
    oracle's), scale -1 and -1.37 (mirrored crops, the oracle's; one near the top-left corner), |x| = 3 x 10^9 and
    |y| = 3 x 10^9 (every tap is padding: exactly b_c, in closed form), NaN, +inf and -inf in x, y and s in turn (every
    value column NaN, any NaN pattern in bf16; padding columns +0). The ordinary particles between them are the
    oracle's bits: no state disturbs another particle's rows. A coordinate of 2^31 or more, +inf included, converts to
    INT_MAX, so its second tap's index is the wrapping INT_MAX + 1 (next_px in crop.hip)."""
    kinds = [k for k, _ in DEGENERATE]
    p = np.array([s for _, s in DEGENERATE], np.float32).T.copy()
    frame = _frame(H1, W1, 33)
    w = C.window(p, BOX1, S, H1, W1)
    staged_want = [k in ("zero", "mirror", "ord") for k in kinds]
    assert w["staged"].tolist() == staged_want
    zero = kinds.index("zero")
    assert (w["wx"][zero], w["wy"][zero]) == (2, 2)
    mirrored = [i for i, k in enumerate(kinds) if k == "mirror"]
    assert (w["wx"][mirrored] > 30).all() and w["cx0"][mirrored[1]] == -1 and w["cy0"][mirrored[1]] == -1
    g2, pp = (S // patch) ** 2, patch * patch
    K = 3 * pp
    # the reference: the oracle on the in-range states only (its conversions are defined there), b_c in closed form
    inr = [i for i, k in enumerate(kinds) if k in ("zero", "mirror", "ord")]
    far = [i for i, k in enumerate(kinds) if k == "far"]
    nan = [i for i, k in enumerate(kinds) if k == "nan"]
    ref = np.zeros((len(kinds) * g2, kp), np.float32)
    ref[_particle_rows(inr, g2)] = opf.crop_patches(frame, np.ascontiguousarray(p[:, inr]), BOX1, S, patch, kp, MEAN, STD)
    _, b = opf.norm_affine(MEAN, STD)
    ref[_particle_rows(far, g2), :K] = np.repeat(b, pp)
    zr = ref[zero * g2:(zero + 1) * g2, :K].reshape(g2, 3, pp)
    assert all(np.unique(zr[:, c]).size == 1 for c in range(3)) and np.unique(zr).size == 3
    finite = _particle_rows(inr + far, g2)
    nan_rows = _particle_rows(nan, g2)
    for dtype in DTYPES:
        got = _gpu_crop(frame, p, BOX1, S, patch, kp, dtype)
        _assert_rows(got, ref, dtype, S, patch, "finite states", rows=finite)
        gn = got[nan_rows]
        isnan = np.isnan(gn[:, :K]) if dtype == torch.float32 else (gn[:, :K] & 0x7FFF) > 0x7F80
        bad = np.argwhere(~isnan)
        assert bad.size == 0, f"{dtype}: a non-finite state's value is not NaN at " \
                              f"{C.where(int(nan_rows[bad[0][0]]), int(bad[0][1]), S, patch)}"
        assert not gn[:, K:].view(np.uint32 if dtype == torch.float32 else np.uint16).any(), "padding of NaN rows not +0"


@pytest.mark.parametrize("S,patch,kp", [(32, 16, 768), (28, 14, 640)])
@pytest.mark.parametrize("box", [(-56.0, 42.0), (56.0, -42.0), (-56.0, -42.0)])
def test_crop_negative_box_side_is_the_mirrored_crop(S, patch, kp, box):
    """A negative w0 or h0 mirrors that axis only; with scale -1 on top the other axis is the mirrored one. Particles in
    the middle, near the top-left corner (the window reaches the border on both sides) and near the bottom-right."""
    p = np.array([[60.0, 5.0, 64.5, 124.0, 30.0], [50.0, 4.0, 47.25, 93.0, 70.0], [1.0, 1.37, -1.0, -1.37, 0.5]], np.float32)
    w = C.window(p, box, S, H1, W1)
    assert w["staged"].all() and (w["wx"] >= 20).all() and (w["wy"] >= 14).all()
    assert w["cx0"][1] == -1 and w["cy0"][1] == -1 and w["cx1"][3] == W1 and w["cy1"][3] == H1
    frame = _frame(H1, W1, 44)
    ref = _check(frame, p, box, S, patch, kp, f"box {box}")
    # the mirror, stated without the oracle's negative step: particle 0 equals the upright crop with that axis reversed
    # (56 / S and 42 / S are exact for both S, so both grids' coordinates are computed without rounding)
    up = opf.crop_patches(frame, p[:, :1], (abs(box[0]), abs(box[1])), S, patch, kp, MEAN, STD)
    g = S // patch

    def image(m):
        return m[:, : 3 * patch * patch].reshape(g, g, 3, patch, patch).transpose(2, 0, 3, 1, 4).reshape(3, S, S)
    want = image(up)[:, :: (-1 if box[1] < 0 else 1), :: (-1 if box[0] < 0 else 1)]
    assert np.array_equal(bits(image(ref[: g * g])), bits(want))


# ------------------------------------------------------------------ f. closed forms independent of the oracle
@pytest.mark.parametrize("S,patch,kp", [(32, 16, 768), (32, 8, 256), (28, 7, 192)])
def test_crop_equals_the_closed_forms(S, patch, kp):
    """A frame whose bytes encode the position, mean 0 (out = fp32(v a_c), one rounding, computed in fp64): the identity
    crop, half-pixel shifts in x and in y (the mean of two neighbours), scale 2 (the mean of four) and scale -1 (the
    identity crop flipped in both axes), at four origins, two of them hanging over the frame. Each is exact in fp32, so
    a mistake shared by the kernel and the oracle cannot pass."""
    frame = C.position_frame(80, 300)
    origins = [(40, 8), (250, 3), (-5, -7), (290, 70)]
    p, want = C.closed_forms(frame, S, patch, kp, STD, origins)
    assert C.window(p, (S, S), S, 80, 300)["staged"].all()
    for dtype in DTYPES:
        got = _gpu_crop(frame, p, (float(S), float(S)), S, patch, kp, dtype, mean=(0.0, 0.0, 0.0))
        _assert_rows(got, want, dtype, S, patch, "closed forms")


# ------------------------------------------------------------------ g. C ABI
@pytest.mark.parametrize("name,dtype", [("vpf_crop_patches_f32", torch.float32), ("vpf_crop_patches_bf16", torch.bfloat16)])
@pytest.mark.parametrize("S,patch,kp", [(32, 16, 768), (28, 7, 192)])
def test_crop_c_abi_reads_only_the_first_n_columns(S, patch, kp, name, dtype):
    """ld = 9 > n = 6: the columns past n hold NaN and are not read (the output is the 6-particle reference), and no
    row past the output's end is written."""
    import ctypes
    from vitparticlefiltertracker_amd import _lib, ops
    n, ld, g = 6, 9, S // patch
    frame = _frame(H1, W1, 5)
    buf = torch.full((3, ld), float("nan"), device=DEV)
    buf[:, :n] = torch.from_numpy(SIX).to(DEV)
    rows = n * g * g
    out = torch.full((rows + GUARD_ROWS, kp), GUARD, device=DEV, dtype=dtype)
    out[:rows].fill_(SENTINEL)
    ab = np.array(_norm_ab(MEAN, STD), np.float32)
    fd = torch.from_numpy(frame).to(DEV)
    ws = ops.rgba_workspace((H1, W1), DEV)
    _lib.call(name, fd.data_ptr(), H1, W1, ws.data_ptr(), buf.data_ptr(), ld, n, BOX1[0], BOX1[1], S, patch, kp,
              ab.ctypes.data_as(ctypes.c_void_p), out.data_ptr(), _lib.stream_ptr())
    _guard_intact(out, rows, name)
    ref = opf.crop_patches(frame, SIX, BOX1, S, patch, kp, MEAN, STD)
    _assert_rows(_host(out[:rows]), ref, dtype, S, patch, f"{name} ld={ld}")


@pytest.mark.parametrize("name", ["vpf_crop_patches_f32", "vpf_crop_patches_bf16"])
def test_crop_c_abi_rejects_bad_arguments(name):
    from vitparticlefiltertracker_amd import _lib
    fn = getattr(_lib.lib(), name)
    fake = 4096                                          # never dereferenced: validation fails first
    S, patch, kp, n = 32, 8, 256, 6

    def crop(frame=fake, H=H1, W=W1, ws=fake, particles=fake, ld=9, n=n, S=S, patch=patch, kp=kp, norm=fake, out=fake):
        return fn(frame, H, W, ws, particles, ld, n, 40.0, 30.0, S, patch, kp, norm, out, None)
    assert crop(H=0) == -1 and crop(W=0) == -1 and crop(n=-1) == -1 and crop(ld=n - 1) == -1
    assert crop(S=S + 1) == -1 and crop(S=0) == -1 and crop(S=-32) == -1 and crop(patch=0) == -1
    assert crop(kp=kp + 4) == -1 and crop(kp=3 * patch * patch - 8) == -1
    assert crop(frame=None) == -1 and crop(ws=None) == -1 and crop(norm=None) == -1
    assert crop(particles=None) == -1 and crop(out=None) == -1
    assert crop(n=0, particles=None, out=None) == 0      # nothing to read or write: no launch
