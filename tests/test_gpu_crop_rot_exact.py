"""GPU (MI355X): the rotated crop (SPEC S12; vpf_crop_patches_rot_f32 / _bf16, RotGrid in csrc/crop.hip) bit for bit
against s12_reference.crop_patches_rot, the bf16 output as its RNE rounding, on the footing tests/test_gpu_crop_exact.py
gives the upright grid: both kernel forms and every store width, every workgroup split on both sides of each threshold,
windows at the last staged and the first unstaged size (the branch asserted from crop_reference.rot_window, the
kernel's widened window), windows cut by each frame edge, the staging bound M = 2^18 with frame content on both sides
(for the upright grid too), the degenerate states of S3's last paragraph with a non-finite angle among them, angles far
outside [-pi, pi], and the C ABI. The inputs live in tests/crop_rot_cases.py; tests/test_crop_host.py shows on the CPU
which one-line mutants of the crop each of them tells from the real thing. Every output is pre-filled with 7.0 and is a
leading view of a buffer whose tail rows hold -9.0 and must survive. Run: python -m pytest tests -m gpu."""
import numpy as np
import pytest
import torch

import crop_reference as C
import crop_rot_cases as K
import s12_reference as R
from oracle import pf as opf

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL, GUARD, GUARD_ROWS = 7.0, -9.0, 5
DTYPES = [torch.float32, torch.bfloat16]
H1, W1, BOX1 = K.H1, K.W1, K.BOX1


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()
    assert torch.cuda.is_available()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _norm_ab(mean=MEAN, std=STD):
    a, b = opf.norm_affine(mean, std)
    return [float(v) for v in a] + [float(v) for v in b]


def _host(t):
    """fp32 values, or the uint16 bit patterns of a bf16 tensor."""
    return t.cpu().numpy() if t.dtype == torch.float32 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def _guard_intact(buf, rows, tag):
    tail = _host(buf[rows:])
    want = np.float32(GUARD) if buf.dtype == torch.float32 else R.bf16_rne(np.float32(GUARD))
    assert tail.shape[0] == GUARD_ROWS and np.all(tail == want), f"{tag}: rows past the output's end were written"


def _guarded(rows, kp, dtype):
    buf = torch.full((rows + GUARD_ROWS, kp), GUARD, device=DEV, dtype=dtype)
    buf[:rows].fill_(SENTINEL)
    return buf


def _gpu_crop(frame, p, ang, box, S, patch, kp, dtype, upright=False):
    """The op on a sentinel-filled leading view of a guarded buffer: fp32 values or bf16 bit patterns [n g^2][kp]."""
    from vitparticlefiltertracker_amd import ops
    n, g = p.shape[1], S // patch
    rows = n * g * g
    buf = _guarded(rows, kp, dtype)
    fd, ws = torch.from_numpy(frame).to(DEV), ops.rgba_workspace(frame.shape[:2], DEV)
    pd = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(DEV)
    if upright:
        torch.ops.vpf.crop_patches(fd, ws, pd, [float(box[0]), float(box[1])], S, patch, _norm_ab(), buf[:rows])
    else:
        torch.ops.vpf.crop_patches_rot(fd, ws, pd, torch.from_numpy(np.ascontiguousarray(ang, np.float32)).to(DEV),
                                       [float(box[0]), float(box[1])], S, patch, _norm_ab(), buf[:rows])
    _guard_intact(buf, rows, f"S={S} patch={patch} kp={kp} {dtype}")
    return _host(buf[:rows])


def _assert_rows(got, ref, dtype, S, patch, tag, rows=None):
    """got == ref (fp32 bits), or got == RNE(ref) (bf16 bits), over `rows` (default: all); names the first bad cell."""
    want = bits(ref) if dtype == torch.float32 else R.bf16_rne(ref)
    have = bits(got) if dtype == torch.float32 else got
    sel = np.arange(ref.shape[0]) if rows is None else np.asarray(rows)
    bad = np.argwhere(have[sel] != want[sel])
    if bad.size:
        r, c = int(sel[bad[0][0]]), int(bad[0][1])
        raise AssertionError(f"{tag} {dtype}: {len(bad)} cells differ from the reference, first at "
                             f"{C.where(r, c, S, patch)}: got bits {int(have[r, c]):#x}, want {int(want[r, c]):#x}")


def _padding_is_zero(got, K3, dtype, tag):
    assert not got[:, K3:].view(np.uint32 if dtype == torch.float32 else np.uint16).any(), f"{tag}: padding not +0"


def _particle_rows(idx, g2):
    return (np.asarray(idx).reshape(-1, 1) * g2 + np.arange(g2).reshape(1, -1)).reshape(-1)


def _window(c):
    return C.rot_window(c["p"], c["ang"], c["box"], c["S"], c["H"], c["W"])


def _check(c, patch, kp, tag):
    """A case whose every state is finite and in range, both dtypes against the reference; the padding columns exactly
    +0 over the sentinel. Returns the reference."""
    frame = K.frame(c["H"], c["W"], c["seed"])
    ref = R.crop_patches_rot(frame, c["p"], c["ang"], c["box"], c["S"], patch, kp, MEAN, STD)
    K3 = 3 * patch * patch
    assert not bits(ref[:, K3:]).any()
    for dtype in DTYPES:
        got = _gpu_crop(frame, c["p"], c["ang"], c["box"], c["S"], patch, kp, dtype)
        _assert_rows(got, ref, dtype, c["S"], patch, tag)
        _padding_is_zero(got, K3, dtype, tag)
    return ref


def _b_rows(patch):
    """b_c in every value column: the row of a crop whose every tap is padding."""
    _, b = opf.norm_affine(MEAN, STD)
    return np.repeat(np.asarray(b, np.float32), patch * patch)


# ------------------------------------------------------------------ a. every form and store width
@pytest.mark.parametrize("S,patch,kp,form", K.FORMS)
def test_rot_every_form_and_store_width(S, patch, kp, form):
    """(32, 16, 768) and (16, 8, 192): the 8-pixel form, 16-B stores. (32, 8, 256): the per-row kernel with 64 padding
    columns. (28, 14, 640): per-row, bf16 pairs. (28, 7, 192): odd patch, element stores. (24, 12, 448): per-row. Six
    particles at 0, +-pi/2, pi, 0.3 and -2.5: the far corner, (-40, -40) wholly in the border (b_c only), the scales 0.5,
    1.37 and 2; all staged."""
    c = K.forms(S)
    assert C.kernel_form(patch, kp) == form and _window(c)["staged"].all()
    ref = _check(c, patch, kp, f"S={S} patch={patch} kp={kp}")
    g2, K3 = (S // patch) ** 2, 3 * patch * patch
    assert np.array_equal(bits(ref[2 * g2:3 * g2, :K3]), bits(np.broadcast_to(_b_rows(patch), (g2, K3))))
    assert len({ref[k * g2:(k + 1) * g2].tobytes() for k in range(6)}) == 6


# ------------------------------------------------------------------ b. every split share
@pytest.mark.parametrize("n", K.SPLITS)
def test_rot_every_split_share(n):
    """The 8-pixel form's launch shapes on both sides of each threshold: four workgroups per particle (n = 6, 1023),
    two (1024, 2047), one (2048), at S = 16, patch = 8; every angle in [-pi, pi], all staged."""
    c = K.splits(n)
    assert C.kernel_form(8, 192) == "lds8" and C.split_of(n) == {6: 4, 1023: 4, 1024: 2, 2047: 2, 2048: 1}[n]
    assert _window(c)["staged"].all()
    _check(c, 8, 192, f"n={n}")


# ------------------------------------------------------------------ c. the LDS budget
@pytest.mark.parametrize("patch,kp", [(16, 768), (14, 640)])
@pytest.mark.parametrize("variant", K.BUDGET_VARIANTS)
@pytest.mark.parametrize("over", [False, True], ids=["at", "over"])
@pytest.mark.parametrize("pair", sorted(K.BUDGET))
def test_rot_window_at_and_over_the_lds_budget(pair, over, variant, patch, kp):
    """Frame 200 x 200, scale 1, box (side, 0.75 side) about (100, 100), S = 32 on the 8-pixel form. At 0.3: side 92.0
    has a 108 x 94 window, staged; 92.25 has 110 x 94 = 10340 > CROP_LDS_DW dwords, global taps. At pi/4: 80.75 has
    100 x 100, 81.0 has 102 x 102. On the per-row form S = 28, whose same windows belong to the sides 92.5 / 92.75 and
    81.25 / 81.5. Each as it is, with the sides swapped and the angle pi/2 - a (the same window walked along the other
    axis), and with the sides swapped and the angle -a (the window transposed). The sides and the branch come from the
    kernel's widened window, restated. A small staged particle rides along on each side."""
    c = K.budget(pair, over, variant, 2 * patch)
    w = _window(c)
    assert (w["wx"][1], w["wy"][1]) == c["sides"]
    assert w["staged"].tolist() == [True, not over, True] and (w["px"][1] > C.CROP_LDS_DW) == over
    _check(c, patch, kp, f"side {c['side']} window {c['sides']}")


# ------------------------------------------------------------------ d. windows cut by the frame
@pytest.mark.parametrize("S,patch,kp", [(16, 8, 192), (28, 7, 192)])
def test_rot_windows_cut_by_the_frame(S, patch, kp):
    """Boxes at 0.3 and at -2.5 hanging over each edge and each corner of the 96 x 128 frame: the window starts in the
    left / top border (cx0 = -1, cy0 = -1) or ends in the right / bottom one (cx1 = W, cy1 = H), asserted. Then centres
    10^6 px off each side (past the staging bound, global taps) and 2 x 10^5 px off (staged: a window one border column
    or row wide): every tap is padding, so these eight rows are exactly b_c."""
    c = K.cut(S)
    H, W = c["H"], c["W"]
    w = _window(c)
    for off in (0, 8):
        e = {k: [off + i for i in v] for k, v in K.CUT_EDGES.items()}
        assert (w["cx0"][e["left"]] == -1).all() and (w["cx1"][e["right"]] == W).all()
        assert (w["cy0"][e["top"]] == -1).all() and (w["cy1"][e["bottom"]] == H).all()
    assert w["staged"].tolist() == [True] * 16 + [False] * 4 + [True] * 4
    assert (np.minimum(w["wx"], w["wy"])[16:] == 1).all()
    assert w["cx0"][20:22].tolist() == [-1, W] and w["cy0"][22:24].tolist() == [-1, H]
    ref = _check(c, patch, kp, "cut windows")
    g2, K3 = (S // patch) ** 2, 3 * patch * patch
    assert np.array_equal(bits(ref[16 * g2:, :K3]), bits(np.broadcast_to(_b_rows(patch), (8 * g2, K3))))
    assert all(ref[k * g2:(k + 1) * g2, :K3].std() > 0.1 for k in range(16))         # the first sixteen see the frame


# ------------------------------------------------------------------ e. the staging bound
@pytest.fixture(scope="module")
def bound_frame():
    c = K.bound()
    return K.frame(c["H"], c["W"], c["seed"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("grid", ["rot", "upright"])
def test_staging_bound_with_frame_content_on_both_sides(grid, dtype, bound_frame):
    """An 8 x 262200 frame, box (12, 8), S = 16: xc = 262110 has M = |xc| + |yc| + |bw| + |bh| = 262134 and is the last
    staged magnitude, xc = 262120 has M = 2^18 and takes the global taps; both windows lie inside the frame, so both
    rows are frame content read at the coarsest coordinates the LDS taps ever see (ulp 2^-6 px). Two ordinary particles
    ride along. For RotGrid at 0.3 against s12_reference, for UprightGrid against the oracle."""
    c = K.bound()
    H, W = K.BOUND_HW
    S, patch, kp = K.BOUND_S, 8, 192
    w = _window(c) if grid == "rot" else C.window(c["p"], c["box"], S, H, W)
    m = np.abs(c["p"][0]) + np.abs(c["p"][1]) + np.abs(c["p"][2] * np.float32(c["box"][0])) \
        + np.abs(c["p"][2] * np.float32(c["box"][1]))
    assert m.dtype == np.float32 and (m[1], m[3]) == K.BOUND_M and K.BOUND_M[1] == C.M_BOUND
    assert w["staged"].tolist() == [True, True, True, False]
    assert (w["cx0"] >= 0).all() and (w["cx1"] < W).all() and (w["wx"][[1, 3]] == (16 if grid == "rot" else 14)).all()
    if grid == "rot":
        ref = R.crop_patches_rot(bound_frame, c["p"], c["ang"], c["box"], S, patch, kp, MEAN, STD)
    else:
        ref = opf.crop_patches(bound_frame, c["p"], c["box"], S, patch, kp, MEAN, STD)
    g2 = (S // patch) ** 2
    assert all(ref[k * g2:(k + 1) * g2].std() > 0.5 for k in range(4)), "a row does not see the frame"
    got = _gpu_crop(bound_frame, c["p"], c["ang"], c["box"], S, patch, kp, dtype, upright=grid == "upright")
    _assert_rows(got, ref, dtype, S, patch, f"staging bound, {grid}")


# ------------------------------------------------------------------ f. degenerate states
def _assert_nan_rows(got, nan_rows, K3, dtype, S, patch):
    gn = got[nan_rows]
    isnan = np.isnan(gn[:, :K3]) if dtype == torch.float32 else (gn[:, :K3] & 0x7FFF) > 0x7F80
    bad = np.argwhere(~isnan)
    assert bad.size == 0, f"{dtype}: a non-finite state's value is not NaN at " \
                          f"{C.where(int(nan_rows[bad[0][0]]), int(bad[0][1]), S, patch)}"
    _padding_is_zero(gn, K3, dtype, "NaN rows")


@pytest.mark.parametrize("S,patch,kp", [(32, 16, 768), (32, 8, 256), (28, 7, 192)])
def test_rot_degenerate_states_between_ordinary_particles(S, patch, kp):
    """SPEC S3's last paragraph through the rotated grid, one call, angles mixed: scale 0 (every sample at
    (x - 0.5, y - 0.5): one value per channel, a 4 x 4 window), scale -1 and -1.37 (mirrored grids, one near the
    top-left corner), |x| and |y| = 3 x 10^9 at five angles (every tap is padding: exactly b_c), NaN, +inf and -inf in
    x, y, s and the ANGLE in turn (every value column NaN, any NaN pattern in bf16; padding columns +0). A non-finite
    angle with a finite state is the one degenerate state of bounded magnitude: only make_window's `wx >= 1` keeps it
    from being staged. The ordinary particles in between are the reference's bits."""
    c = K.degenerate(S)
    kinds = K.DEG_KINDS
    w = _window(c)
    assert w["staged"].tolist() == [k in K.IN_RANGE_KINDS for k in kinds]
    zero = kinds.index("zero")
    assert (w["wx"][zero], w["wy"][zero]) == (4, 4)
    mirrored = [i for i, k in enumerate(kinds) if k == "mirror"]
    assert (w["wx"][mirrored] > 30).all() and w["cx0"][mirrored[1]] == -1 and w["cy0"][mirrored[1]] == -1
    na = [i for i, k in enumerate(kinds) if k == "nan_angle"]
    assert (w["m"][na] < C.M_BOUND).all() and (w["wx"][na] == -c["W"]).all() and (w["wy"][na] == -c["H"]).all()
    g2, K3 = (S // patch) ** 2, 3 * patch * patch
    inr, far = c["inr"], [i for i, k in enumerate(kinds) if k == "far"]
    nan = [i for i, k in enumerate(kinds) if k in ("nan", "nan_angle")]
    assert len(far) == 6 and len(nan) == 12 and len(inr) + len(far) + len(nan) == len(kinds)
    frame = K.frame(c["H"], c["W"], c["seed"])
    ref = np.zeros((len(kinds) * g2, kp), np.float32)
    ref[_particle_rows(inr, g2)] = R.crop_patches_rot(frame, np.ascontiguousarray(c["p"][:, inr]), c["ang"][inr],
                                                      c["box"], S, patch, kp, MEAN, STD)
    ref[_particle_rows(far, g2), :K3] = _b_rows(patch)
    zr = ref[zero * g2:(zero + 1) * g2, :K3].reshape(g2, 3, patch * patch)
    assert all(np.unique(zr[:, ch]).size == 1 for ch in range(3)) and np.unique(zr).size == 3
    finite, nan_rows = _particle_rows(inr + far, g2), _particle_rows(nan, g2)
    for dtype in DTYPES:
        got = _gpu_crop(frame, c["p"], c["ang"], c["box"], S, patch, kp, dtype)
        _assert_rows(got, ref, dtype, S, patch, "finite states", rows=finite)
        _padding_is_zero(got[finite], K3, dtype, "finite states")
        _assert_nan_rows(got, nan_rows, K3, dtype, S, patch)


@pytest.mark.parametrize("S,patch,kp", [(32, 16, 768), (32, 8, 256), (28, 7, 192)])
@pytest.mark.parametrize("box", K.NEG_BOXES)
def test_rot_negative_box_sides(S, patch, kp, box):
    """A negative w0 or h0 mirrors that axis of the grid, with scale -1 and -1.37 on top: the corner extremes come out of
    RotGrid::taps' min / max in another order. In the middle, near the top-left corner (the window reaches the border
    on both sides) and near the bottom-right."""
    c = K.negative_box(S, box)
    w = _window(c)
    assert w["staged"].all() and (w["wx"] >= 20).all() and (w["wy"] >= 14).all()
    assert w["cx0"][1] == -1 and w["cy0"][1] == -1 and w["cx1"][3] == c["W"] and w["cy1"][3] == c["H"]
    _check(c, patch, kp, f"box {box}")


# ------------------------------------------------------------------ g. angles outside [-pi, pi]
@pytest.mark.parametrize("S,patch,kp", [(32, 16, 768), (28, 7, 192)])
def test_rot_angles_outside_the_circle(S, patch, kp):
    """One call with the angles 0, -0.0, -1e-9, 1e-9, +-2 pi, 7 pi / 2, +-100, +-1e6 and +-3e38 on an ordinary state and on
    one across the left edge. The reduction u = a fp32(1 / 2 pi), u -= floorf(u) rounds to 1.0 for -1e-9 (read as 0 by
    the quadrant's & 3), keeps 4 fraction bits at 1e6 and is 0 at 3e38. On the reference: -1e-9, -0.0, 2 pi and +-3e38
    give a = 0's rows bit for bit, 100 and 1e6 do not."""
    c = K.angles(S)
    w = _window(c)
    n = len(K.ANGLES)
    assert w["staged"].all() and (w["cx0"][n:] == -1).all() and (w["cx0"][:n] > 0).all()
    ref = _check(c, patch, kp, "angles")
    g2 = (S // patch) ** 2
    for s in range(len(K.ANGLE_STATES)):
        row = lambda a: ref[(s * n + K.ANGLES.index(a)) * g2:(s * n + K.ANGLES.index(a) + 1) * g2].tobytes()
        assert all(row(a) == row(0.0) for a in K.SAME_AS_ZERO) and all(row(a) != row(0.0) for a in K.NOT_ZERO)


# ------------------------------------------------------------------ h. C ABI
ROT_ABI = [("vpf_crop_patches_rot_f32", torch.float32), ("vpf_crop_patches_rot_bf16", torch.bfloat16)]


@pytest.mark.parametrize("name,dtype", ROT_ABI)
@pytest.mark.parametrize("S,patch,kp", [(32, 16, 768), (28, 7, 192)])
def test_rot_c_abi_reads_only_the_first_n_columns(S, patch, kp, name, dtype):
    """ld = 9 > n = 6: the state columns and the angles past n hold NaN and are not read (the output is the 6-particle
    reference), and no row past the output's end is written."""
    import ctypes
    from vitparticlefiltertracker_amd import _lib, ops
    n, ld, g = 6, 9, S // patch
    frame = K.frame(H1, W1, 5)
    buf = torch.full((3, ld), float("nan"), device=DEV)
    buf[:, :n] = torch.from_numpy(K.SIX).to(DEV)
    ang = torch.full((ld,), float("nan"), device=DEV)
    ang[:n] = torch.from_numpy(K.SIX_ANGLES).to(DEV)
    rows = n * g * g
    out = _guarded(rows, kp, dtype)
    ab = np.array(_norm_ab(), np.float32)
    fd = torch.from_numpy(frame).to(DEV)
    ws = ops.rgba_workspace((H1, W1), DEV)
    _lib.call(name, fd.data_ptr(), H1, W1, ws.data_ptr(), buf.data_ptr(), ld, ang.data_ptr(), n, BOX1[0], BOX1[1], S,
              patch, kp, ab.ctypes.data_as(ctypes.c_void_p), out.data_ptr(), _lib.stream_ptr())
    _guard_intact(out, rows, name)
    ref = R.crop_patches_rot(frame, K.SIX, K.SIX_ANGLES, BOX1, S, patch, kp, MEAN, STD)
    got = _host(out[:rows])
    _assert_rows(got, ref, dtype, S, patch, f"{name} ld={ld}")
    _padding_is_zero(got, 3 * patch * patch, dtype, name)


@pytest.mark.parametrize("name,dtype", ROT_ABI)
def test_rot_c_abi_rejects_bad_arguments(name, dtype):
    """Every rejection of crop_launch and the rotated entry points' own (angles == NULL with n > 0), with pointers that
    are never dereferenced; a rejected call and n = 0 with null pointers launch nothing: a real workspace and output
    handed to them keep their fill."""
    from vitparticlefiltertracker_amd import _lib, ops
    fn = getattr(_lib.lib(), name)
    fake = 4096                                          # never dereferenced: validation fails first
    S, patch, kp, n = 32, 8, 256, 6

    def crop(frame=fake, H=H1, W=W1, ws=fake, particles=fake, ld=9, angles=fake, n=n, S=S, patch=patch, kp=kp, norm=fake,
             out=fake):
        return fn(frame, H, W, ws, particles, ld, angles, n, 40.0, 30.0, S, patch, kp, norm, out, None)
    assert crop(H=0) == -1 and crop(W=0) == -1 and crop(n=-1) == -1 and crop(ld=n - 1) == -1
    assert crop(S=S + 1) == -1 and crop(S=0) == -1 and crop(S=-32) == -1 and crop(patch=0) == -1
    assert crop(kp=kp + 4) == -1 and crop(kp=3 * patch * patch - 8) == -1
    assert crop(frame=None) == -1 and crop(ws=None) == -1 and crop(norm=None) == -1
    assert crop(particles=None) == -1 and crop(out=None) == -1 and crop(angles=None) == -1
    assert crop(H=65536, W=65536) == -1
    # nothing to read or write: returns 0 and launches nothing, not even the workspace fill
    ws = ops.rgba_workspace((H1, W1), DEV)
    ws.fill_(-1)
    out = _guarded(n * 16, kp, dtype)
    fd = torch.zeros(H1, W1, 3, device=DEV, dtype=torch.uint8)
    ab = np.array(_norm_ab(), np.float32)
    assert crop(frame=fd.data_ptr(), ws=ws.data_ptr(), norm=ab.ctypes.data, n=0, particles=None, angles=None,
                out=None) == 0
    assert crop(frame=fd.data_ptr(), ws=ws.data_ptr(), norm=ab.ctypes.data, angles=None, out=out.data_ptr()) == -1
    torch.cuda.synchronize()
    assert (ws == -1).all(), "a call with nothing to do filled the workspace"
    _guard_intact(out, n * 16, name)
    assert (out[:n * 16] == SENTINEL).all()
