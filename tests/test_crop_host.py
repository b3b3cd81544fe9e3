"""CPU: tests/crop_reference.py against the oracle and against itself. The closed forms (crops known from integer
arithmetic on a position-encoding frame) anchor oracle.pf.crop_patches beyond the identity crop of test_oracle_pf.py, a
mirrored crop included; the window geometry reproduces the two windows on either side of the LDS budget and contains
every tap of every sample, for mirrored grids too.

The rotated grid (SPEC S12): crop_reference.rot_window restates RotGrid::taps + make_window. A hunt over 55 000 states
per grid size looks for a tap outside the unclamped window and prints the largest excess of an interior sample's floor
over the corner samples' floors; the budget pairs, the staging-bound pair and the non-finite states are re-derived; and
every input of tests/test_gpu_crop_rot_exact.py (tests/crop_rot_cases.py) is run through a model of what the kernel
reads, with and without the one-line mutants of crop_reference.MUTANTS. Mutant -> the cases that are meant to catch it
(each asserted to change at least one output bit there):
  1 s -> -s                              forms, splits n = 6, budget, cut, bound, degenerate, negative box
  2 ex and ey swapped                    the same
  3 half box taken from the centre       the same
  4 floorf omitted from the reduction    angles (+3e38: the quadrant's conversion saturates; the negative angles round
                                         differently); the six ordinary angles of `forms` do not catch it
  5 a window from two opposite corners   forms, budget, cut, degenerate, negative box
  6 second tap clamp(i) + 1              cut (a window ending in the right or bottom border: the index leaves it)"""
import numpy as np
import pytest

import crop_reference as C
import crop_rot_cases as K
import s12_reference as R12
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


# ============================================================================================== the rotated grid
def _hunt_states(n, box, rng):
    """n states with M = |x| + |y| + |bw| + |bh| up to just under 2^18: centres of every magnitude from 1 to 1.2 x 10^5
    with both signs, scales over [-3, 3] (0, -0, +-1e-30, +-1 and +-3 among them), and every class of angle: uniform over
    [-pi, pi], the multiples of pi / 4, -1e-9 and its like, and the out-of-range ones."""
    mag = lambda: rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(0.0, 5.11, n)
    p = np.stack([mag(), mag(), rng.uniform(-3.0, 3.0, n)]).astype(np.float32)
    near = rng.random(n) < 0.4                                        # in and around a frame
    p[0, near], p[1, near] = rng.uniform(-60, 190, near.sum()), rng.uniform(-60, 160, near.sum())
    edge = rng.random(n) < 0.15                                       # on either side of the staging bound
    p[0, edge] = rng.choice([-1.0, 1.0], edge.sum()) * rng.uniform(2.0e5, 2.62e5, edge.sum())
    p[1, edge] = rng.uniform(-2000.0, 2000.0, edge.sum())
    p[2, :10] = [0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 3.0, -3.0, 0.5, -0.5]
    p[0, :10], p[1, :10] = rng.uniform(0, 128, 10), rng.uniform(0, 96, 10)
    special = np.array(K.ANGLES + [1e-9, -1e-9, -0.0, 50.0, -50.0, 4 * K.PI, -7 * K.PI / 2], np.float32)
    cls = rng.integers(0, 4, n)
    ang = rng.uniform(-K.PI, K.PI, n)
    ang = np.where(cls == 1, rng.integers(-8, 9, n) * (K.PI / 4), ang)
    ang = np.where(cls == 2, rng.choice(special, n), ang).astype(np.float32)
    ang = np.where(cls == 3, rng.uniform(-60.0, 60.0, n).astype(np.float32), ang).astype(np.float32)
    ang[:3] = [-1e-9, -0.0, 2 * K.PI]
    return p, ang


HUNT_BOXES = [(40.0, 30.0), (-40.0, 30.0), (300.0, -200.0), (9000.0, 7000.0)]


@pytest.mark.parametrize("S", [16, 28, 32])
def test_rot_window_contains_every_tap_of_every_sample(S, capsys):
    """The containment hunt: for every state of bounded magnitude (the only ones a window is staged for), both taps of
    every sample lie inside the tap range [ix_lo, ix_hi] x [iy_lo, iy_hi] BEFORE any clamp, so win_tap's clamp changes
    no staged tap. The one-pixel margin is for the amount by which an interior sample's floor may exceed the corner
    samples' floors: it must be <= 1, and is printed."""
    H, W = 96, 128
    excess, checked, staged, m_max = 0, 0, 0, 0.0
    for k, box in enumerate(HUNT_BOXES):
        for chunk in range(4):
            p, ang = _hunt_states(3500, box, np.random.default_rng(1000 * S + 10 * k + chunk))
            coords = R12.sample_coords(p, ang, box, S)
            w = C.rot_window(p, ang, box, S, H, W, coords=coords)
            ok = w["m"] < C.M_BOUND
            assert w["staged"][~ok].sum() == 0
            fx, fy = C.rot_sample_floors(p, ang, box, S, coords=coords)
            for f, lo, hi in ((fx, w["ix_lo"], w["ix_hi"]), (fy, w["iy_lo"], w["iy_hi"])):
                fmin, fmax = f.min(1)[ok], f.max(1)[ok]
                assert (fmin >= lo[ok]).all() and (fmax + 1 <= hi[ok]).all()
                # the corner samples' floors are lo + 1 and hi - 2
                excess = max(excess, int(((lo[ok] + 1) - fmin).max()), int((fmax - (hi[ok] - 2)).max()))
            checked += int(ok.sum())
            staged += int(w["staged"].sum())
            m_max = max(m_max, float(w["m"][ok].max()))
            assert (w["wx"] >= 1).all() and (w["wy"] >= 1).all()
    assert checked >= 50000 and staged > checked // 2 and 2.6e5 < m_max < 2.0 ** 18, (checked, staged, m_max)
    with capsys.disabled():
        print(f"\n[rot window hunt] S={S}: {checked} states with M < 2^18 ({staged} staged), largest excess of an "
              f"interior sample's floor over the corner samples' floors: {excess} px")
    assert 0 <= excess <= 1


@pytest.mark.parametrize("S", [32, 28])
@pytest.mark.parametrize("variant", K.BUDGET_VARIANTS)
@pytest.mark.parametrize("pair", sorted(K.BUDGET))
def test_rot_window_reproduces_the_budget_pairs(pair, variant, S):
    """Frame 200 x 200, box (side, 0.75 side), centre (100, 100), scale 1, S = 32. At 0.3: side 92.0 gives a 108 x 94
    window (10152 dwords, staged), 92.25 a 110 x 94 one (10340, global taps). At pi / 4: 80.75 gives 100 x 100 and 81.0
    gives 102 x 102 (that box makes the WINDOW square). At S = 28 the same windows belong to the sides 92.5 / 92.75 and
    81.25 / 81.5. Re-derived here in fp64 from the geometry, not from rot_window: the corner samples are the box's
    corners pulled in by half a step, turned, minus the half pixel. Swapping the box's sides and turning by pi/2 - a
    keeps the footprint ("quarter"); swapping them and turning by -a transposes it."""
    a, ratio, sides_in, sides_over, widths = K.BUDGET[pair]
    assert widths[32] == {"0.3": (92.0, 92.25), "pi/4": (80.75, 81.0)}[pair]
    for over, side, sides in ((False, widths[S][0], sides_in), (True, widths[S][1], sides_over)):
        c = K.budget(pair, over, variant, S)
        assert c["box"] == ((side, ratio * side) if variant == "plain" else (ratio * side, side))
        w = C.rot_window(c["p"], c["ang"], c["box"], S, 200, 200)
        hx, hy = (0.5 * (S - 1) / S * abs(b) for b in c["box"])
        t = float(c["ang"][1])
        ex, ey = abs(np.cos(t)) * hx + abs(np.sin(t)) * hy, abs(np.sin(t)) * hx + abs(np.cos(t)) * hy
        want = tuple(int((np.floor(99.5 + e) + 2) - (np.floor(99.5 - e) - 1) + 1) for e in (ex, ey))
        assert want == c["sides"] == (sides[::-1] if variant == "transposed" else sides)
        assert (w["wx"][1], w["wy"][1]) == want and w["px"][1] == want[0] * want[1]
        assert w["staged"].tolist() == [True, not over, True] and (w["px"][1] > C.CROP_LDS_DW) == over
    assert 108 * 94 == 10152 and 110 * 94 == 10340 and 100 * 100 <= C.CROP_LDS_DW < 102 * 102


def test_rot_window_bound_pair():
    """H, W = 8, 262200, box (12, 8), S = 16, angle 0.3, yc = 4: xc = 262110 has M = 262134 and is staged, xc = 262120
    has M = 262144 = 2^18 and is not; both windows are 16 x 10 and inside the frame's columns. The upright grid's pair,
    at the same states, is 14 x 10."""
    c = K.bound()
    H, W = K.BOUND_HW
    w = C.rot_window(c["p"], c["ang"], c["box"], c["S"], H, W)
    assert (w["m"][1], w["m"][3]) == K.BOUND_M and K.BOUND_M[1] == C.M_BOUND
    assert w["staged"].tolist() == [True, True, True, False]
    assert (w["wx"][[1, 3]] == 16).all() and (w["wy"][[1, 3]] == 10).all()
    assert (w["cx0"] >= 0).all() and (w["cx1"] < W).all() and w["cx1"][3] == 262127
    u = C.window(c["p"], c["box"], c["S"], H, W)
    assert u["staged"].tolist() == [True, True, True, False]
    assert (u["wx"][[1, 3]] == 14).all() and (u["wy"][[1, 3]] == 10).all() and (u["cx1"] < W).all()


def test_rot_window_of_non_finite_states():
    """NaN or +-inf in x, y or s is never staged (M is not below the bound). A non-finite ANGLE with a finite state has a
    finite M, and only the guard's `wx >= 1` keeps it unstaged: every corner coordinate is NaN, fminf / fmaxf keep their
    +inf / -inf seeds, the tap range is (+inf, -inf) and clamps to cx0 = W, cx1 = -1: a window of side -W. (Folding the
    corners without the seeds would give NaN bounds, which clamp_f sends to -2: a staged 1 x 1 window at (-1, -1). The
    kernel's fold has the seeds.) Every window whose corners are not all NaN has sides >= 1."""
    c = K.degenerate(32)
    H, W = c["H"], c["W"]
    w = C.rot_window(c["p"], c["ang"], c["box"], 32, H, W)
    kinds = np.array(K.DEG_KINDS)
    assert w["staged"].tolist() == [k in K.IN_RANGE_KINDS for k in kinds]
    na = kinds == "nan_angle"
    assert na.sum() == 3 and (w["m"][na] < C.M_BOUND).all()
    assert (w["ix_lo"][na] == np.inf).all() and (w["ix_hi"][na] == -np.inf).all()
    assert (w["cx0"][na] == W).all() and (w["cx1"][na] == -1).all() and (w["cy0"][na] == H).all() and (w["cy1"][na] == -1).all()
    assert (w["wx"][na] == -W).all() and (w["wy"][na] == -H).all()
    cx, cy = C.rot_corners(c["p"], c["ang"], c["box"], 32)
    some = ~np.isnan(cx).all(1)
    assert (w["wx"][some] >= 1).all()
    assert (w["wy"][~np.isnan(cy).all(1)] >= 1).all()
    assert not np.isfinite(w["m"][(kinds == "nan")]).any()
    zero = K.DEG_KINDS.index("zero")
    assert (w["wx"][zero], w["wy"][zero]) == (4, 4)                  # scale 0: one sample point, the margin around it


def test_sincos2pi_any_equals_the_oracle_routine():
    rng = np.random.default_rng(5)
    us = np.concatenate([rng.random(2000).astype(np.float32), np.float32([0.0, 0.25, 0.5, 0.75, 1.0, 2.0 ** -24])])
    import ctypes
    for u in us:
        c, s = ctypes.c_float(), ctypes.c_float()
        opf.lib().orc_sincos2pi(float(u), ctypes.byref(c), ctypes.byref(s))
        got = C.sincos2pi_any(u)
        assert (bits(np.float32(got[0])), bits(np.float32(got[1]))) == (bits(np.float32(c.value)), bits(np.float32(s.value)))
    # u = 1.0 (the reduction of a = -1e-9 rounds to it) is read as u = 0: the quadrant is taken mod 4
    assert [bits(v) for v in C.sincos2pi_any(1.0)] == [bits(v) for v in C.sincos2pi_any(0.0)]
    u = np.float32(-1e-9) * R12.INV_2PI
    assert np.float32(u - np.floor(u)) == np.float32(1.0)


# ------------------------------------------------------------------ the GPU cases, on the CPU
def _gpu_cases():
    cases = {f"forms S={S}": K.forms(S) for S in sorted({f[0] for f in K.FORMS})}
    cases["splits n=6"] = K.splits(6)
    for pair in sorted(K.BUDGET):
        for over in (False, True):
            for v in K.BUDGET_VARIANTS:
                for S in (32, 28):
                    cases[f"budget {pair} {'over' if over else 'at'} {v} S={S}"] = K.budget(pair, over, v, S)
    cases.update({f"cut S={S}": K.cut(S) for S in (16, 28)})
    cases["bound"] = K.bound()
    cases.update({f"degenerate S={S}": K.degenerate(S) for S in (32, 28)})
    cases.update({f"negative box {b} S={S}": K.negative_box(S, b) for b in K.NEG_BOXES for S in (32, 28)})
    cases.update({f"angles S={S}": K.angles(S) for S in (32, 28)})
    return cases


GPU_CASES = _gpu_cases()


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_rot_case_discriminates_its_mutants(name):
    """On the case's finite in-range states: the model of what the kernel reads (S12's coordinates, the restated window
    as a flat array, win_tap's clamp) equals s12_reference.crop_raw bit for bit, and every mutant the case is meant to
    catch changes at least one bit of the normalised output."""
    c = GPU_CASES[name]
    frame = K.frame(c["H"], c["W"], c["seed"])
    p, ang = np.ascontiguousarray(c["p"][:, c["inr"]]), c["ang"][c["inr"]]
    ref = R12.crop_raw(frame, p, ang, c["box"], c["S"])
    a, b = opf.norm_affine((0.485, 0.456, 0.406), STD)
    norm = lambda v: R12.fmaf_vec(v, a.reshape(1, 1, 1, 3), b.reshape(1, 1, 1, 3))
    assert np.array_equal(bits(C.rot_crop_model(frame, p, ang, c["box"], c["S"])), bits(ref))
    want = bits(norm(ref))
    for m in c["catches"]:
        got = bits(norm(C.rot_crop_model(frame, p, ang, c["box"], c["S"], mutant=m)))
        assert (got != want).any(), f"{name}: mutant {m} ({C.MUTANTS[m]}) changes no output bit"


def test_every_mutant_is_caught_by_a_named_case():
    caught = {m: sorted(n for n, c in GPU_CASES.items() if m in c["catches"]) for m in C.MUTANTS}
    assert all(caught[m] for m in C.MUTANTS), caught
    assert any(n.startswith("angles") for n in caught[4]) and any(n.startswith("cut") for n in caught[6])
    assert any(n.startswith("budget") for n in caught[5])


def test_rot_cut_windows_and_far_centres():
    """The cut case's branches: which frame edge cuts which window, global taps 10^6 px off, one staged border column
    or row 2 x 10^5 px off."""
    for S in (16, 28):
        c = K.cut(S)
        H, W = c["H"], c["W"]
        w = C.rot_window(c["p"], c["ang"], c["box"], S, H, W)
        for off in (0, 8):
            e = {k: [off + i for i in v] for k, v in K.CUT_EDGES.items()}
            assert (w["cx0"][e["left"]] == -1).all() and (w["cx1"][e["right"]] == W).all()
            assert (w["cy0"][e["top"]] == -1).all() and (w["cy1"][e["bottom"]] == H).all()
        assert w["staged"].tolist() == [True] * 16 + [False] * 4 + [True] * 4
        assert (np.minimum(w["wx"], w["wy"])[16:] == 1).all()
        assert w["cx0"][20:22].tolist() == [-1, W] and w["cy0"][22:24].tolist() == [-1, H]


def test_rot_angle_rows_on_the_reference():
    """-1e-9 (u rounds to 1.0), -0.0, 2 pi and +-3e38 (u - floor(u) = 0) give a = 0's crop bit for bit; 100 and 1e6 do
    not."""
    c = K.angles(32)
    ref = R12.crop_raw(K.frame(c["H"], c["W"], c["seed"]), c["p"], c["ang"], c["box"], 32)
    n = len(K.ANGLES)
    for s in range(len(K.ANGLE_STATES)):
        row = lambda a: ref[s * n + K.ANGLES.index(a)].tobytes()
        assert all(row(a) == row(0.0) for a in K.SAME_AS_ZERO) and all(row(a) != row(0.0) for a in K.NOT_ZERO)
        assert ref[s * n].std() > 1.0
