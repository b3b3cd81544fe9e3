"""The inputs of tests/test_gpu_crop_rot_exact.py (the rotated crop, SPEC S12, on the device), kept apart from it so that
tests/test_crop_host.py can show on the CPU what each of them exercises: the branch from crop_reference.rot_window, and
which one-line mutants of the crop (crop_reference.MUTANTS) change at least one output bit on its inputs. A case is a
dict: the frame's H, W and seed, the box, S, particles float32[3][n], angles float32[n], `inr` (the indices of the finite
in-range states, the ones a reference can be computed for) and `catches` (the mutants it is meant to catch)."""
import math

import numpy as np

PI = math.pi
INF, NAN = float("inf"), float("nan")
H1, W1, BOX1 = 96, 128, (40.0, 30.0)
SIX = np.array([[60.0, 64.5, -40.0, W1 - 1.0, 30.0, 100.0],         # test_s12_gpu_kernels.py's six states and angles
                [50.0, 47.25, -40.0, H1 - 1.0, 70.0, 20.0],
                [1.0, 1.37, 0.5, 2.0, 0.5, 1.37]], np.float32)
SIX_ANGLES = np.array([0.0, PI / 2, -PI / 2, PI, 0.3, -2.5], np.float32)
FORMS = [(32, 16, 768, "lds8"), (16, 8, 192, "lds8"), (32, 8, 256, "row"), (28, 14, 640, "row"), (28, 7, 192, "row"),
         (24, 12, 448, "row")]


def frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _case(H, W, seed, box, S, p, ang, catches, inr=None):
    p = np.ascontiguousarray(np.asarray(p, np.float32))
    ang = np.ascontiguousarray(np.asarray(ang, np.float32))
    assert p.shape == (3, ang.shape[0])
    return dict(H=H, W=W, seed=seed, box=box, S=S, p=p, ang=ang, catches=tuple(catches),
                inr=list(range(p.shape[1])) if inr is None else list(inr))


# ------------------------------------------------------------------ a. forms
def forms(S):
    """The six states: quarter turns, 0.3 and -2.5; scales 0.5, 1.37 and 2; one box wholly in the border."""
    return _case(H1, W1, 100 + S, BOX1, S, SIX, SIX_ANGLES, catches=(1, 2, 3, 5))


# ------------------------------------------------------------------ b. splits
SPLITS = (6, 1023, 1024, 2047, 2048)
SPLIT_BOX = (24.0, 18.0)


def splits(n):
    rng = np.random.default_rng(n)
    p = np.stack([rng.uniform(-10, W1 + 10, n), rng.uniform(-10, H1 + 10, n), rng.uniform(0.5, 2.0, n)])
    return _case(H1, W1, 11, SPLIT_BOX, 16, p, rng.uniform(-PI, PI, n), catches=(1, 2, 3) if n == 6 else ())


# ------------------------------------------------------------------ c. the LDS budget
# angle, height / width of the box, the two window sizes (the last staged one and the first unstaged one), and per S the
# box's width that has each of them, on a 200 x 200 frame, centre (100, 100), scale 1. S = 28 draws its corner samples
# in by a larger half step than S = 32, so the same windows belong to slightly larger boxes.
BUDGET = {"0.3": (0.3, 0.75, (108, 94), (110, 94), {32: (92.0, 92.25), 28: (92.5, 92.75)}),
          "pi/4": (PI / 4, 0.75, (100, 100), (102, 102), {32: (80.75, 81.0), 28: (81.25, 81.5)})}
BUDGET_HW = 200


BUDGET_VARIANTS = ("plain", "quarter", "transposed")


def budget(pair, over, variant, S=32):
    """Particle 1 is the one at the budget; the small ones on either side are staged. "quarter": the box's sides
    swapped and the angle pi/2 - a, the same footprint (and window) walked along the other axis. "transposed": the
    sides swapped and the angle -a, the footprint mirrored in the diagonal, so the window's sides swap."""
    a, ratio, sides_in, sides_over, widths = BUDGET[pair]
    side, sides = (widths[S][1], sides_over) if over else (widths[S][0], sides_in)
    box = (side, ratio * side)
    if variant == "quarter":
        a, box = PI / 2 - a, box[::-1]
    elif variant == "transposed":
        a, box, sides = -a, box[::-1], sides[::-1]
    else:
        assert variant == "plain"
    p = [[30.0, 100.0, 150.0], [40.0, 100.0, 160.0], [0.25, 1.0, 0.25]]
    c = _case(BUDGET_HW, BUDGET_HW, 3, box, S, p, [a] * 3, catches=(1, 2, 3, 5))
    c["sides"], c["over"], c["side"] = sides, over, side
    return c


# ------------------------------------------------------------------ d. windows cut by the frame
CUT_EDGES = dict(left=[0, 4, 6], right=[1, 5, 7], top=[2, 4, 5], bottom=[3, 6, 7])      # indices into the 8 positions


def cut(S):
    """Eight positions (each edge, each corner) at the angles 0.3 and -2.5 (particles k and 8 + k), then centres 10^6 px
    off each side (past the staging bound: global taps) and 2 x 10^5 px off (staged: one border column or row)."""
    H, W = H1, W1
    xs = [0.0, W, W / 2, W / 2, 0.0, W, 0.0, W]
    ys = [H / 2, H / 2, 0.0, H, 0.0, 0.0, H, H]
    far = [(-1e6, 50.0), (W + 1e6, 50.0), (50.0, -1e6), (50.0, H + 1e6),
           (-2e5, 50.0), (W + 2e5, 50.0), (50.0, -2e5), (50.0, H + 2e5)]
    p = [xs + xs + [f[0] for f in far], ys + ys + [f[1] for f in far], [1.0] * 24]
    ang = [0.3] * 8 + [-2.5] * 8 + [0.3, -2.5] * 4
    return _case(H, W, 21, BOX1, S, p, ang, catches=(1, 2, 3, 5, 6))


# ------------------------------------------------------------------ e. the staging bound
BOUND_HW, BOUND_BOX, BOUND_S = (8, 262200), (12.0, 8.0), 16
BOUND_P = [[100.0, 262110.0, 131000.5, 262120.0], [4.25, 4.0, 3.5, 4.0], [1.0, 1.0, 1.0, 1.0]]
BOUND_M = (262134.0, 262144.0)                    # |xc| + |yc| + |bw| + |bh| of particles 1 and 3: under and at 2^18


def bound():
    """A thin frame wide enough to have content on both sides of M = 2^18: particle 1 is the last staged magnitude,
    particle 3 the first that takes the global taps; a coordinate's ulp there is 2^-6 px."""
    return _case(*BOUND_HW, 18, BOUND_BOX, BOUND_S, BOUND_P, [0.3] * 4, catches=(1, 2, 3))


# ------------------------------------------------------------------ f. degenerate states
ORD = [(60.0, 50.0, 1.0), (64.5, 47.25, 1.37), (100.0, 20.0, 0.5), (30.0, 70.0, 2.0)]
DEGENERATE = [
    ("zero", (64.3, 47.7, 0.0), 0.3), ("ord", ORD[0], 0.0),
    ("mirror", (60.0, 50.0, -1.0), 0.3), ("mirror", (5.0, 4.0, -1.37), -2.5), ("ord", ORD[1], PI / 2),
    ("far", (3e9, 50.0, 1.0), 0.3), ("far", (-3e9, 50.0, 1.0), -2.5), ("far", (60.0, -3e9, 1.0), PI / 4),
    ("far", (60.0, 3e9, 1.0), 0.0), ("far", (3e9, -3e9, 1.0), PI), ("far", (-3e9, 3e9, 1.37), -PI / 2),
    ("ord", ORD[2], -0.3),
    ("nan", (NAN, 50.0, 1.0), 0.3), ("nan", (INF, 50.0, 1.0), 0.0), ("nan", (-INF, 50.0, 1.0), -2.5), ("ord", ORD[3], 0.3),
    ("nan", (60.0, NAN, 1.0), 0.0), ("nan", (60.0, INF, 1.0), 0.3), ("nan", (60.0, -INF, 1.0), PI / 4), ("ord", ORD[0], -2.5),
    ("nan", (60.0, 50.0, NAN), 0.3), ("nan", (60.0, 50.0, INF), -2.5), ("nan", (60.0, 50.0, -INF), 0.0), ("ord", ORD[1], PI),
    ("nan_angle", ORD[0], NAN), ("nan_angle", ORD[1], INF), ("nan_angle", ORD[3], -INF), ("ord", ORD[2], 0.3),
]
DEG_KINDS = [k for k, _, _ in DEGENERATE]
IN_RANGE_KINDS = ("zero", "mirror", "ord")


def degenerate(S):
    p = np.array([s for _, s, _ in DEGENERATE], np.float32).T
    inr = [i for i, k in enumerate(DEG_KINDS) if k in IN_RANGE_KINDS]
    return _case(H1, W1, 33, BOX1, S, p, [a for _, _, a in DEGENERATE], catches=(1, 2, 3, 5), inr=inr)


NEG_BOXES = [(-56.0, 42.0), (56.0, -42.0), (-56.0, -42.0)]


def negative_box(S, box):
    """Mirrored grids through RotGrid::taps' min / max: a negative w0 or h0, with scale -1 and -1.37 on top; in the
    middle, near the top-left corner and near the bottom-right one."""
    p = [[60.0, 5.0, 64.5, 124.0, 30.0], [50.0, 4.0, 47.25, 93.0, 70.0], [1.0, 1.37, -1.0, -1.37, 0.5]]
    return _case(H1, W1, 44, box, S, p, [0.3, -2.5, 0.0, PI / 2, -0.3], catches=(1, 2, 3, 5))


# ------------------------------------------------------------------ g. angles
ANGLES = [0.0, -0.0, -1e-9, 1e-9, 2 * PI, -2 * PI, 7 * PI / 2, 100.0, -100.0, 1e6, -1e6, 3e38, -3e38]
ANGLE_STATES = [(60.0, 50.0, 1.0), (2.0, 47.25, 1.37)]          # an ordinary state, and one across the left edge
SAME_AS_ZERO = [-1e-9, -0.0, 2 * PI, 3e38, -3e38]               # rows equal to a = 0's, bit for bit
NOT_ZERO = [100.0, 1e6]                                         # rows that differ from a = 0's


def angles(S):
    """Every angle on both states: particle s * len(ANGLES) + k has state s and angle k."""
    p = np.array([st for st in ANGLE_STATES for _ in ANGLES], np.float32).T
    return _case(H1, W1, 55, BOX1, S, p, ANGLES * len(ANGLE_STATES), catches=(4,))


# ------------------------------------------------------------------ the colour cues (SPEC S13, S14) on the same states
def color_states(rot):
    """(kinds, particles float32[3][n], angles float32[n] or None) on the 48 x 40 frame: scale 0 (its one sample point
    is the pixel (20, 17)), the mirrored scales -1 and -1.37 (one near the top-left corner), with an angle row every
    angle of ANGLES on one state, a NaN scale and (with an angle row) a NaN angle, ordinary particles in
    between."""
    rows = [("ord", (24.0, 20.0, 1.0), 0.3), ("zero", (20.5, 17.5, 0.0), -2.5), ("ord", (20.5, 17.25, 0.77), 0.0),
            ("mirror", (24.0, 20.0, -1.0), 0.3), ("mirror", (5.0, 4.0, -1.37), -2.5), ("ord", (46.0, 18.0, 1.0), PI / 2)]
    if rot:
        rows += [("angle", (24.0, 20.0, 1.0), a) for a in ANGLES]
    rows += [("nan", (24.0, 20.0, float("nan")), 0.3), ("ord", (2.0, 20.0, 1.37), -0.3)]
    if rot:
        rows += [("nan", (24.0, 20.0, 1.0), float("nan")), ("ord", (24.0, 38.0, 1.0), 0.3)]
    kinds = [k for k, _, _ in rows]
    p = np.ascontiguousarray(np.array([s for _, s, _ in rows], np.float32).T)
    return kinds, p, (np.array([a for _, _, a in rows], np.float32) if rot else None)


def one_pixel_bin(frame, x, y, B):
    """The bin of the pixel (x, y) itself, from its bytes."""
    q = frame[y, x].astype(np.int64) >> (8 - (B.bit_length() - 1))
    return int((q[0] * B + q[1]) * B + q[2])
