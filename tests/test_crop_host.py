"""CPU: tests/crop_reference.py against the oracle and against itself. The closed forms (crops known from integer
arithmetic on a position-encoding frame) anchor oracle.pf.crop_patches beyond the identity crop of test_oracle_pf.py, a
mirrored crop included; the window geometry reproduces the two windows on either side of the LDS budget and contains
every tap of every sample, for mirrored grids too."""
import numpy as np
import pytest

import crop_reference as C
from oracle import pf as opf

STD = (0.229, 0.224, 0.225)
ORIGINS = [(40, 8), (250, 3), (-5, -7), (290, 70)]      # inside; across the x = 256 wrap; over the top-left; bottom-right


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("S,patch,kp", [(32, 16, 768), (32, 8, 256), (28, 7, 192)])
def test_oracle_crop_equals_the_closed_forms(S, patch, kp):
    """Identity, half-pixel shifts in x and in y, the 2 x 2 mean at scale 2 and the mirrored crop at scale -1, at four
    origins (two hang over the frame: the zero padding is part of the closed form). Bit for bit."""
    frame = C.position_frame(80, 300)
    p, want = C.closed_forms(frame, S, patch, kp, STD, ORIGINS)
    got = opf.crop_patches(frame, p, (S, S), S, patch, kp, (0.0, 0.0, 0.0), STD)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{len(bad)} cells differ, first at {C.where(*bad[0], S, patch)}"
    pp = patch * patch
    assert want[:, : 3 * pp].any() and not want[:, 3 * pp:].any()
    n = len(C.CLOSED_CASES)
    g2 = (S // patch) ** 2
    blocks = {want[k * g2:(k + 1) * g2].tobytes() for k in range(n)}      # the five cases are five different crops
    assert len(blocks) == n


def test_closed_form_flip_is_the_identity_crop_reversed():
    frame = C.position_frame(80, 300)
    _, ident = C.closed_case(frame, "identity", 40, 8, 32)
    (x, y, s), flip = C.closed_case(frame, "flip", 40, 8, 32)
    assert (x, y, s) == (56.0, 24.0, -1.0)
    assert np.array_equal(flip, ident[::-1, ::-1]) and not np.array_equal(flip, ident)
    assert np.array_equal(ident[3, 5], frame[8 + 3, 40 + 5])


def test_window_reproduces_the_two_budget_geometries():
    """Frame 200 x 200, S = 32, scale 1: an 80 x 128 window is exactly CROP_LDS_DW dwords, the last staged size; a
    77 x 133 window is one dword more, the first that takes the global taps. And their transposes."""
    for centre, box, sides in [((100.0, 100.0), (79.5, 129.25), (80, 128)), ((100.5, 100.5), (76.5, 134.25), (77, 133))]:
        for t in (False, True):
            b = box[::-1] if t else box
            c = centre[::-1] if t else centre
            w = C.window(np.array([[c[0]], [c[1]], [1.0]], np.float32), b, 32, 200, 200)
            want = sides[::-1] if t else sides
            assert (w["wx"][0], w["wy"][0]) == want, (centre, box, t, w["wx"], w["wy"])
            assert w["px"][0] == want[0] * want[1] and w["staged"][0] == (want[0] * want[1] <= C.CROP_LDS_DW)
    assert 80 * 128 == C.CROP_LDS_DW and 77 * 133 == C.CROP_LDS_DW + 1


@pytest.mark.parametrize("box", [(40.0, 30.0), (-40.0, 30.0), (300.0, 200.0)])
def test_window_contains_every_tap_of_every_sample(box):
    """For states in and around the frame with scales in [-2.5, 2.5] (zero included): every sample's floor lies in
    [ix_lo, ix_hi - 1], so both taps of each axis are in the window, and a mirrored grid's window is as wide as the
    upright one's (its sides are never below 2)."""
    rng = np.random.default_rng(7)
    n, S, H, W = 4000, 32, 96, 128
    p = np.stack([rng.uniform(-60, W + 60, n), rng.uniform(-60, H + 60, n), rng.uniform(-2.5, 2.5, n)]).astype(np.float32)
    p[2, :8] = [0.0, -0.0, 1.0, -1.0, 2.5, -2.5, 1e-30, -1e-30]
    w = C.window(p, box, S, H, W)
    fx, fy = C.sample_floors(p, box, S)
    assert (fx.min(1) >= w["ix_lo"]).all() and (fx.max(1) + 1 <= w["ix_hi"]).all()
    assert (fy.min(1) >= w["iy_lo"]).all() and (fy.max(1) + 1 <= w["iy_hi"]).all()
    assert (fx.min(1) == w["ix_lo"]).all() and (fx.max(1) + 1 == w["ix_hi"]).all()      # and it is tight
    assert (w["ix_hi"] - w["ix_lo"] >= 1).all() and (w["wx"] >= 1).all() and (w["wy"] >= 1).all()
    neg = p[2] < 0
    assert neg.sum() > n // 3 and (w["ix_hi"] - w["ix_lo"])[neg].max() > 50


def test_window_guard_for_states_outside_the_int_range_and_non_finite_ones():
    """Nothing is staged for |x| or |y| >= 2^18, NaN or inf in any of x, y, s; the clamped window is still a valid one
    (sides >= 1): no conversion is out of range."""
    inf, nan = np.inf, np.nan
    p = np.array([[3e9, -3e9, 50.0, 1e6, 50.0, nan, inf, -inf, 50.0, 50.0, 50.0, 50.0, 50.0, 50.0, 2e5, 50.0],
                  [50.0, 50.0, -3e9, 50.0, -1e6, 50.0, 50.0, 50.0, nan, inf, -inf, 50.0, 50.0, 50.0, 50.0, 50.0],
                  [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, nan, inf, -inf, 1.0, 1.0]], np.float32)
    w = C.window(p, (40.0, 30.0), 32, 96, 128)
    assert not w["staged"][:14].any() and w["staged"][14:].all()
    assert (w["wx"] >= 1).all() and (w["wy"] >= 1).all() and (w["px"] <= 98 * 130).all()
    assert w["wx"][14] == 1 and w["cx0"][14] == 128                       # 2 x 10^5 px to the right: one border column


def test_kernel_form_and_split():
    assert C.kernel_form(16, 768) == "lds8" and C.kernel_form(8, 192) == "lds8"
    assert C.kernel_form(8, 256) == "row" and C.kernel_form(14, 640) == "row" and C.kernel_form(7, 192) == "row"
    assert [C.split_of(n) for n in (6, 1023, 1024, 2047, 2048)] == [4, 4, 2, 2, 1]
