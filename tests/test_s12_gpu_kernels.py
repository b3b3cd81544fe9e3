"""GPU (MI355X): the SPEC S12 kernels — vpf_crop_patches_rot_f32 bit for bit against the numpy reference
(tests/s12_reference.py) and _bf16 as its RNE rounding, on every kernel form, store width, launch shape and on the
global-tap branch; vpf_predict_angle bit for bit. Run: python -m pytest tests -m gpu."""
import math

import numpy as np
import pytest
import torch

import s12_reference as R
from oracle import pf as opf

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
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


def _norm_ab():
    a, b = opf.norm_affine(MEAN, STD)
    return [float(v) for v in a] + [float(v) for v in b]


def _frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _gpu_crop(frame, p, ang, box, S, patch, kp, dtype):
    from vitparticlefiltertracker_amd import ops
    n, g = p.shape[1], S // patch
    fd = torch.from_numpy(frame).to(DEV)
    out = torch.full((n * g * g, kp), 7.0, device=DEV, dtype=dtype)      # padding columns must be overwritten with 0
    vpf().crop_patches_rot(fd, ops.rgba_workspace(frame.shape[:2], DEV), torch.from_numpy(p).to(DEV),
                           torch.from_numpy(ang).to(DEV), [float(box[0]), float(box[1])], S, patch, _norm_ab(), out)
    return out.cpu().numpy() if dtype == torch.float32 else out.view(torch.int16).cpu().numpy().view(np.uint16)


def _check(frame, p, ang, box, S, patch, tag=""):
    kp = -(-3 * patch * patch // 64) * 64
    ref = R.crop_patches_rot(frame, p, ang, box, S, patch, kp, MEAN, STD)
    got = _gpu_crop(frame, p, ang, box, S, patch, kp, torch.float32)
    bad = np.flatnonzero((bits(got) != bits(ref)).any(axis=1))
    assert bad.size == 0, f"{tag}: fp32 rows differ, first {bad[:8]} (row = particle * g*g + patch)"
    assert not ref[:, 3 * patch * patch:].any() and not got[:, 3 * patch * patch:].any()
    got16 = _gpu_crop(frame, p, ang, box, S, patch, kp, torch.bfloat16)
    assert np.array_equal(got16, R.bf16_rne(ref)), f"{tag}: bf16 is not the RNE rounding of the fp32 reference"
    return ref


# ------------------------------------------------------------------ vpf_crop_patches_rot_*
H1, W1, BOX1 = 96, 128, (40.0, 30.0)
SIX = np.array([[60.0, 64.5, -40.0, W1 - 1.0, 30.0, 100.0],
                [50.0, 47.25, -40.0, H1 - 1.0, 70.0, 20.0],
                [1.0, 1.37, 0.5, 2.0, 0.5, 1.37]], np.float32)
SIX_ANGLES = np.array([0.0, PI / 2, -PI / 2, PI, 0.3, -2.5], np.float32)


@pytest.mark.parametrize("S,patch", [(32, 16), (32, 8), (28, 14), (28, 7), (24, 12)])
def test_crop_rot_equals_reference(S, patch):
    """(32, 16) and (32, 8): the 8-pixel form with 16-B stores. (28, 14): the per-row form with bf16 pairs and ViT-L's
    Kp = 640. (28, 7): odd patch, element stores. (24, 12): Kp = 448. Six particles: the angles 0, +-pi/2, pi, 0.3 and
    -2.5, one centre at (-40, -40) whose every tap is in the zero border (its rows hold b_c only), one on the frame's
    far corner, the scales 0.5, 1.37 and 2.0. Kp is 3 patch^2 rounded up to 64; the padding columns are zero."""
    frame = _frame(H1, W1, S + patch)
    assert (R.tap_bbox_pixels(SIX, SIX_ANGLES, BOX1, S, H1, W1) <= R.CROP_LDS_DW).all()     # all staged in LDS
    ref = _check(frame, SIX, SIX_ANGLES, BOX1, S, patch, f"S={S} patch={patch}")
    g2, pp = (S // patch) ** 2, patch * patch
    _, b = opf.norm_affine(MEAN, STD)
    border = ref[2 * g2:3 * g2, : 3 * pp].reshape(g2, 3, pp)
    assert all(np.all(border[:, c] == b[c]) for c in range(3))
    assert len({ref[k * g2:(k + 1) * g2].tobytes() for k in range(6)}) == 6


@pytest.mark.parametrize("S,patch", [(32, 16), (28, 14)])
def test_crop_rot_window_over_the_lds_budget_takes_the_global_taps(S, patch):
    """Frame 160 x 200, a 110 x 110 box at pi/4 in its middle: the bounding box of its samples' taps, clipped to the
    frame, holds more than CROP_LDS_DW pixels (asserted from the reference's geometry), so the workgroup reads the
    taps from global memory; the second particle of the call is staged. Both kernel forms."""
    H, W, box = 160, 200, (110.0, 110.0)
    p = np.array([[100.0, 60.0], [80.0, 50.0], [1.0, 0.5]], np.float32)
    ang = np.array([PI / 4, PI / 4], np.float32)
    px = R.tap_bbox_pixels(p, ang, box, S, H, W)
    assert px[0] > R.CROP_LDS_DW and px[1] <= R.CROP_LDS_DW, px
    _check(_frame(H, W, 3), p, ang, box, S, patch, "over budget")


@pytest.mark.parametrize("n", [6, 1024, 2048])
def test_crop_rot_every_split_share(n):
    """The 8-pixel form's launch shapes: four workgroups per particle (n = 6), two (n = 1024), one (n = 2048), at
    S = 16, patch = 8. Centres in and around the frame, every angle in [-pi, pi], scales over [0.5, 2]."""
    rng = np.random.default_rng(n)
    p = np.stack([rng.uniform(-10, W1 + 10, n), rng.uniform(-10, H1 + 10, n), rng.uniform(0.5, 2.0, n)]).astype(np.float32)
    ang = rng.uniform(-PI, PI, n).astype(np.float32)
    _check(_frame(H1, W1, 11), p, ang, (24.0, 18.0), 16, 8, f"n={n}")


FAR = np.array([[60.0, 3e9, 64.5, 30.0, np.inf, 100.0],
                [50.0, 40.0, 47.25, -3e9, 40.0, 20.0],
                [1.0, 1.0, 1.37, 1.0, 1.0, 0.5]], np.float32)
FAR_ORDINARY, FAR_HUGE, FAR_INF = [0, 2, 5], [1, 3], 4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("S,patch", [(16, 8), (14, 7)])
def test_crop_rot_states_beyond_the_int_range(S, patch, dtype):
    """SPEC S3's last paragraph through the rotated grid, at angle 0.3, on the 8-pixel form (16, 8) and the per-row
    form with an odd patch (14, 7): a coordinate of +-3e9 converts to a saturated int and every tap (the second one's
    index wraps) is clamped into the zero border, so the row holds b_c exactly; x = +inf gives NaN everywhere. The
    ordinary particles between them are the reference's bits, the padding columns +0."""
    frame = _frame(H1, W1, S)
    ang = np.full(6, 0.3, np.float32)
    g2, pp = (S // patch) ** 2, patch * patch
    kp = -(-3 * pp // 64) * 64
    ref = R.crop_patches_rot(frame, FAR[:, FAR_ORDINARY].copy(), ang[FAR_ORDINARY], BOX1, S, patch, kp, MEAN, STD)
    _, b = opf.norm_affine(MEAN, STD)
    want_b = np.repeat(np.asarray(b, np.float32), pp)
    if dtype == torch.bfloat16:
        ref, want_b = R.bf16_rne(ref), R.bf16_rne(want_b)
        as_float = lambda u16: (u16.astype(np.uint32) << 16).view(np.float32)
    else:
        ref, want_b = bits(ref), bits(want_b)
        as_float = lambda u32: u32.view(np.float32)
    got = _gpu_crop(frame, FAR, ang, BOX1, S, patch, kp, dtype)
    got = got if dtype == torch.bfloat16 else bits(got)
    rows = got.reshape(6, g2, kp)
    assert np.array_equal(rows[FAR_ORDINARY].reshape(-1, kp), ref)
    assert (rows[FAR_HUGE, :, :3 * pp] == want_b).all()
    assert np.isnan(as_float(np.ascontiguousarray(rows[FAR_INF, :, :3 * pp]))).all()
    assert not rows[:, :, 3 * pp:].any(), "padding columns are not +0"


@pytest.mark.parametrize("S,patch", [(32, 8), (28, 7)])
def test_crop_rot_c_abi_reads_only_the_first_n_columns(S, patch):
    """ld > n through the C ABI: the columns past n hold NaN and are not read (the output is the n-particle
    reference), and the output and the angle row have no cell past their end written."""
    import ctypes
    from vitparticlefiltertracker_amd import _lib, ops
    n, ld, g = 6, 9, S // patch
    kp = -(-3 * patch * patch // 64) * 64
    frame = _frame(H1, W1, 5)
    buf = torch.full((3, ld), float("nan"), device=DEV)
    buf[:, :n] = torch.from_numpy(SIX).to(DEV)
    ang = torch.full((ld,), float("nan"), device=DEV)
    ang[:n] = torch.from_numpy(SIX_ANGLES).to(DEV)
    rows = n * g * g
    out = torch.full((rows + 4, kp), -9.0, device=DEV)
    ab = np.array(_norm_ab(), np.float32)
    fd = torch.from_numpy(frame).to(DEV)
    ws = ops.rgba_workspace((H1, W1), DEV)
    _lib.call("vpf_crop_patches_rot_f32", fd.data_ptr(), H1, W1, ws.data_ptr(), buf.data_ptr(), ld, ang.data_ptr(), n,
              BOX1[0], BOX1[1], S, patch, kp, ab.ctypes.data_as(ctypes.c_void_p), out.data_ptr(), _lib.stream_ptr())
    got = out.cpu().numpy()
    ref = R.crop_patches_rot(frame, SIX, SIX_ANGLES, BOX1, S, patch, kp, MEAN, STD)
    assert np.array_equal(bits(got[:rows]), bits(ref)) and np.all(got[rows:] == -9.0)
    L = _lib.lib()
    fake = 4096                                          # never dereferenced: validation fails first

    def crop(H=H1, W=W1, ld=ld, n=n, S=S, patch=patch, kp=kp, angles=fake):
        return L.vpf_crop_patches_rot_f32(fake, H, W, fake, fake, ld, angles, n, 40.0, 30.0, S, patch, kp, fake, fake,
                                          None)
    assert crop(H=0) == -1 and crop(W=0) == -1 and crop(n=-1) == -1 and crop(ld=n - 1) == -1
    assert crop(S=S + 1) == -1 and crop(patch=0) == -1 and crop(kp=kp + 4) == -1 and crop(kp=3 * patch * patch - 8) == -1
    assert crop(angles=None) == -1


# ------------------------------------------------------------------ vpf_predict_angle
LO, HI = -1.25, 0.75


def _angles(n, seed=0):
    """Angles over the range with, cyclically over the index, both range ends (from which half the draws clamp)."""
    a = np.random.default_rng(seed + n).uniform(LO, HI, n).astype(np.float32)
    i = np.arange(n)
    a[i % 4 == 0], a[i % 4 == 1] = LO, HI
    return a


@pytest.mark.parametrize("sig", [0.0, 0.1])
@pytest.mark.parametrize("n,gb,ld", [(1, 0, None), (255, 0, None), (257, 1000, 300), (1000, 7, None)])
def test_predict_angle_equals_reference(n, gb, ld, sig):
    """n: one particle; a ragged last wave; one particle into a second block (global_begin != 0, a longer buffer whose
    cells past n stay as they were); four blocks. sigma_a = 0 keeps every bit; with 0.1 both clamps fire."""
    seed, frame = (1 << 40) + 31 * n, 6
    a = _angles(n)
    ref = a.copy()
    R.predict_angle(ref, gb, seed, frame, sig, LO, HI)
    buf = torch.full((ld or n,), -5.0, device=DEV)
    buf[:n] = torch.from_numpy(a).to(DEV)
    vpf().predict_angle_(buf[:n], gb, seed, frame, sig, [LO, HI])
    got = buf.cpu().numpy()
    assert np.all(got[n:] == -5.0), "cells past n were written"
    assert np.array_equal(bits(got[:n]), bits(ref)), np.flatnonzero(got[:n] != ref)[:8]
    if sig == 0.0:
        assert np.array_equal(bits(ref), bits(a))
    elif n >= 255:
        inner = (ref > np.float32(LO)) & (ref < np.float32(HI))
        assert (ref == np.float32(LO)).sum() > n // 16 and (ref == np.float32(HI)).sum() > n // 16 and inner.sum() > n // 2
        assert not np.array_equal(bits(ref), bits(a))


def test_predict_angle_does_not_depend_on_the_sharding_or_the_other_rows_draws():
    n, seed, frame = 1000, 99, 4
    a = _angles(n, seed=1)

    def run(x, gb):
        t = torch.from_numpy(x.copy()).to(DEV)
        vpf().predict_angle_(t, gb, seed, frame, 0.1, [LO, HI])
        return t.cpu().numpy()
    whole = run(a, 0)
    assert np.array_equal(bits(np.concatenate([run(a[:333], 0), run(a[333:], 333)])), bits(whole))
    assert not np.array_equal(bits(run(a[333:], 0)), bits(whole[333:]))


def test_predict_angle_c_abi_rejects_bad_arguments():
    from vitparticlefiltertracker_amd import _lib
    L = _lib.lib()
    fake = 4096                                          # never dereferenced: validation fails first
    inf, nan = float("inf"), float("nan")

    def predict(n=8, gb=0, sig=0.1, lo=-1.0, hi=1.0):
        return L.vpf_predict_angle(fake, n, gb, 1, 1, sig, lo, hi, None)
    assert predict(n=0) == 0
    assert predict(n=-1) == -1 and predict(gb=-1) == -1 and predict(gb=(1 << 32) - 4) == -1
    assert predict(sig=-0.1) == -1 and predict(sig=inf) == -1 and predict(sig=nan) == -1
    assert predict(lo=-3.2) == -1 and predict(hi=3.2) == -1 and predict(lo=-inf) == -1 and predict(hi=inf) == -1
    assert predict(lo=0.5, hi=0.5) == -1 and predict(lo=1.0, hi=-1.0) == -1
    assert predict(lo=nan) == -1 and predict(hi=nan) == -1
    assert predict(n=0, lo=-PI, hi=PI) == 0              # the whole circle, as fp32(pi), is a valid range
