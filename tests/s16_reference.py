"""SPEC S16 (re-detection: a global search once the target is lost) restated in Python ints and numpy: the reference of
tests/test_s16_*.py, on top of s15_reference (the gate, the device-order sums), s11 / s12_reference (the constant-
velocity and angle predicts), s13_reference (the colour cue of the behaviour run) and oracle.pf (Philox, S2's predict).
Every fp32 operation of the scatter is one numpy float32 operation (one rounding each)."""
import numpy as np

import s10_reference as R10
import s11_reference as R11
import s12_reference as R12
import s13_reference as R13
import s15_reference as R15
from oracle import pf as opf

f32 = np.float32
P_MAX = 1 << 24


# ---------------------------------------------------------------------------------------------- the lattice
def lattice(P: int, W: int, H: int):
    """(gx, inv_gx, inv_P): gx the smallest integer >= 1 with gx^2 H >= P W, found by counting up in Python integers;
    inv_gx = fp32(1) / fp32(gx), inv_P = fp32(1) / fp32(P)."""
    gx = 1
    while gx * gx * H < P * W:
        gx += 1
    return gx, f32(1.0) / f32(gx), f32(1.0) / f32(P)


def cell_xy(i: np.ndarray, u0: np.ndarray, u1: np.ndarray, P: int, W: int, H: int):
    """x, y float32[n] of the particles with global indices i (int64[n]) and in-cell offsets u0, u1 (float32[n]):
    x = clamp(((fp32(i mod gx) + u0) inv_gx) Wm1, 0, Wm1), y = clamp(((fp32(i) + u1) inv_P) Hm1, 0, Hm1)."""
    assert P <= P_MAX and u0.dtype == np.float32 and u1.dtype == np.float32
    gx, inv_gx, inv_P = lattice(P, W, H)
    wm1, hm1 = f32(W) - f32(1.0), f32(H) - f32(1.0)
    c = (np.asarray(i, np.int64) % gx).astype(np.float32)
    x = ((c + u0) * inv_gx) * wm1
    y = ((np.asarray(i, np.int64).astype(np.float32) + u1) * inv_P) * hm1
    assert x.dtype == np.float32 and y.dtype == np.float32
    return np.minimum(np.maximum(x, f32(0.0)), wm1), np.minimum(np.maximum(y, f32(0.0)), hm1)


def draws(gbegin: int, n: int, seed: int, frame: int):
    """u0, u1 float32[n] = uniform(r0), uniform(r1) of Philox counter (i, frame, 0, 3), i = gbegin .. gbegin + n - 1."""
    seed &= (1 << 64) - 1
    key = (seed & 0xFFFFFFFF, seed >> 32)
    u = np.empty((2, n), np.float32)
    for j in range(n):
        r = opf.philox4x32_10((gbegin + j, frame, 0, 3), key)
        u[0, j], u[1, j] = R11.uniform01(r[0]), R11.uniform01(r[1])
    return u[0], u[1]


def predict_search(p: np.ndarray, gbegin: int, P: int, seed: int, frame: int, sig_s, W: int, H: int,
                   scale_range) -> None:
    """SPEC S16's search predict, in place on float32[3][n] or float32[5][n], the shard [gbegin, gbegin + n) of P: the
    scale row is S2's own step (oracle.pf.predict on a copy: x and y of that copy are dropped), x and y the lattice's,
    the velocity rows +0."""
    assert p.dtype == np.float32 and p.shape[0] in (3, 5)
    n = p.shape[1]
    assert gbegin >= 0 and gbegin + n <= P
    walk = np.ascontiguousarray(p[:3]).copy()
    opf.predict(walk, gbegin, seed, frame, (0.0, 0.0, sig_s), W, H, scale_range)
    u0, u1 = draws(gbegin, n, seed, frame)
    p[0], p[1] = cell_xy(np.arange(gbegin, gbegin + n), u0, u1, P, W, H)
    p[2] = walk[2]
    if p.shape[0] == 5:
        p[3:5] = f32(0.0)


# ---------------------------------------------------------------------------------------------- the recursion
def search_after(after, max_hold: int) -> int:
    """A: `after`, or max_hold + 1 (the filter is `lost`) when it is None."""
    return max_hold + 1 if after is None else after


class Filter:
    """The S16 recursion of one target over every state row (x, y, s, [vx, vy], [a]): the predict is the search iff
    held_frames >= A, else S15's (the gained sigmas after a held frame) under either motion model; the angle row's
    predict follows either; the gate of a search frame is gq_search. `returned` is what step() / track() report: the
    anchor on a held search frame. cv = (velocity_std, decay, vmax) or None; rot = (rotation_std, (amin, amax)) or
    None."""

    def __init__(self, P, init_state, motion_std, scale_range, seed, frame_size, K, method, gq, gain, A, gq_search,
                 cv=None, rot=None):
        self.P, self.K, self.method, self.seed = P, K, method, seed
        self.gq, self.gain, self.A, self.gq_search = gq, gain, A, gq_search
        self.motion_std, self.scale_range, self.cv, self.rot = motion_std, scale_range, cv, rot
        self.height, self.width = frame_size
        rows = 3 + (2 if cv else 0) + (1 if rot else 0)
        assert len(init_state) == rows
        self.state = np.zeros((rows, P), np.float32)
        for c, v in enumerate(init_state):
            self.state[c] = v
        self.frame = 0
        self.held_frames = 0
        self.searched = False
        self.anchor = tuple(float(v) for v in init_state[:3])

    @property
    def particles(self):
        return self.state[:3]

    def predict(self, frame=None):
        self.frame = self.frame + 1 if frame is None else frame
        self.searched = self.held_frames >= self.A
        nh = 5 if self.cv else 3
        head = np.ascontiguousarray(self.state[:nh])
        if self.searched:
            predict_search(head, 0, self.P, self.seed, self.frame, self.motion_std[2], self.width, self.height,
                           self.scale_range)
        else:
            std = R15.gained(self.motion_std, self.gain) if self.held_frames > 0 else self.motion_std
            if self.cv:
                R11.predict_cv(head, 0, self.seed, self.frame, std, self.cv[0], self.cv[1], self.cv[2], self.width,
                               self.height, self.scale_range)
            else:
                opf.predict(head, 0, self.seed, self.frame, std, self.width, self.height, self.scale_range)
        self.state[:nh] = head
        if self.rot:
            R12.predict_angle(self.state[-1], 0, self.seed, self.frame, self.rot[0], *self.rot[1])

    def update(self, L) -> dict:
        """One frame under the frame's gate: s15_reference.step on x | y | s; every row gathered by its ancestors; `xtree`:
        the extra rows' device-order sums over the same weights (every weight 1 when held or T == 0); `est`, `extras`:
        the device's estimates; `returned`: the anchor on a held search frame, else `est`."""
        gq = self.gq_search if self.searched else self.gq
        r = R15.step(L, np.ascontiguousarray(self.state[:3]), self.seed, self.frame, self.method, self.K, gq)
        w = [int(q) for q in L] if r["T"] and not r["held"] else [1] * self.P
        r["xtree"] = R15.tree_sums(w, self.state[3:]) if self.state.shape[0] > 3 else []
        r["state"] = np.ascontiguousarray(self.state[:, r["anc"]])
        assert np.array_equal(r["state"][:3].view(np.uint32), r["states"].view(np.uint32))
        d = float(r["T"]) if r["T"] and not r["held"] else float(self.P)
        r["est"] = R15.estimate(r, self.P)
        r["extras"] = tuple(s / d for s in r["xtree"])
        r["searched"] = self.searched
        r["reacquired"] = self.searched and not r["held"]
        if not self.searched:
            self.anchor = r["est"]
        r["returned"] = self.anchor if self.searched and r["held"] else r["est"]
        self.state = r["state"].copy()
        self.held_frames = self.held_frames + 1 if r["held"] else 0
        return r


# ---------------------------------------------------------------------------------------------- the behaviour run
# s13_reference's colour-only follow run (likelihood.lambda = 0) on a 448 x 448 frame: synthetic_clip's background and
# tinted 64 x 64 texture; through frame 8 the target moves as s13_reference.truth, it is absent in frames 9..15, and
# from frame 16 it is at (360, 330), about 300 px from where it vanished, moving (-2, -1) per frame.
SIDE = 448
FRAMES = 28                      # frames 0..27
ABSENT = tuple(range(9, 16))
REAPPEAR = 16
JUMP_TO, JUMP_VELOCITY = (360, 330), (-2, -1)
P_RUN = 1024
THETA, GAIN, ALPHA, MAX_HOLD, AFTER = 0.05, 2.0, 0.3, 30, 3
SEEDS = (1234, 1, 2)
# Measured with this reference on the CPU (recorded in DESIGN.md §14), P = 1024, after = 3, theta = theta_r = 0.05:
#   1. frames 9..15 are held (12..15 as search frames); the first frame that is not held is 16, the first visible one,
#      for each of the seeds 1234, 1 and 2; the test requires it within 2 frames of the reappearance.
#   2. the worst distance to the true centre over the frames from 4 after the re-acquisition on (20..27) is 3.46 px
#      (seed 1234, frame 23), 3.15 px (seed 1) and 3.38 px (seed 2); frame 16's own estimate is 1.81 px away; the bound is 1.5 x the largest, and must itself be < 16 px (a
#      quarter of the box side).
#   3. the control (redetect None, everything else the same): held in every frame from 9 on, `lost` not raised within
#      the clip (the streak reaches 19 <= max_hold), and the plain mean is 316.43 px from the true centre in
#      frame 16 and 291.90 px in frame 27, the last.
REACQUIRE_WITHIN = 2
SEARCH_WORST_PX = {1234: 3.46, 1: 3.15, 2: 3.38}
SEARCH_BOUND_PX = 1.5 * max(SEARCH_WORST_PX.values())
CONTROL_FINAL_PX = 291.90
CONTROL_MIN_PX = 200.0


def truth(k: int):
    """The target's true centre in frame k; None while it is absent."""
    if k < ABSENT[0]:
        return R13.truth(k)
    if k < REAPPEAR:
        return None
    return (float(JUMP_TO[0] + JUMP_VELOCITY[0] * (k - REAPPEAR)), float(JUMP_TO[1] + JUMP_VELOCITY[1] * (k - REAPPEAR)))


def jump_clip(frames: int = FRAMES) -> np.ndarray:
    """uint8[frames][448][448][3]. Frames 0..8 are synthetic_clip's own; the background of the later ones is the same
    generator's first draw, the texture the one synthetic_clip blitted into frame 0."""
    from vitparticlefiltertracker_amd.frames import synthetic_clip
    bx, by, bw, bh = R13.FOLLOW["box"]
    head = synthetic_clip(ABSENT[0], SIDE, SIDE, target_range=R13.TINT)
    bg = np.random.default_rng(7).integers(0, 256, size=(SIDE, SIDE, 3), dtype=np.uint8)
    tex = head[0, by:by + bh, bx:bx + bw].copy()
    mask = np.ones((SIDE, SIDE), bool)
    mask[by:by + bh, bx:bx + bw] = False
    assert np.array_equal(head[0][mask], bg[mask]), "synthetic_clip's background recipe changed"
    clip = np.empty((frames, SIDE, SIDE, 3), np.uint8)
    for k in range(frames):
        if k < ABSENT[0]:
            clip[k] = head[k]
            continue
        clip[k] = bg
        if k >= REAPPEAR:
            cx, cy = (int(v) for v in truth(k))
            clip[k, cy - bh // 2:cy + bh // 2, cx - bw // 2:cx + bw // 2] = tex
    return clip


def distance(est, k: int):
    t = truth(k)
    return None if t is None else float(np.hypot(est[0] - t[0], est[1] - t[1]))


def follow_jump(clip, redetect=True, after=AFTER, theta_r=None, seed=None, P=P_RUN, frames=None, cv=None, rot=None,
                color=None):
    """The reference run of the colour-only tracker under the gate and, unless `redetect` is False (the control), the
    search. Per tracked frame a dict: L, pred (every predicted row), r (Filter.update's result), est (the device's),
    returned, dist (of `returned`; None while the target is absent), held, searched, reacquired, streak, peak, evidence,
    t (the colour template after the frame). With `rot` the cue and the template crops take the angle row (S12's
    coordinates), the template update the frame's angle estimate."""
    c = {**R13.DEFAULTS, **(color or {})}
    F = R13.FOLLOW
    bx, by, bw, bh = F["box"]
    K = F["K"]
    gq = R15.gate_q(THETA, K)
    A = search_after(after, MAX_HOLD) if redetect else (1 << 62)
    t = R13.template(clip[0], (bx, by, bw, bh), 0.0 if rot else None, c["grid"], c["bins"])
    init = (bx + 0.5 * bw, by + 0.5 * bh, 1.0) + ((0.0, 0.0) if cv else ()) + ((0.0,) if rot else ())
    ref = Filter(P, init, F["motion_std"], F["scale_range"], F["seed"] if seed is None else seed, (SIDE, SIDE), K,
                 R10.SYSTEMATIC, gq, GAIN, A, gq if theta_r is None else R15.gate_q(theta_r, K), cv, rot)
    out = []
    for k in range(1, len(clip) if frames is None else frames + 1):
        ref.predict(k)
        pred = ref.state.copy()
        L = R13.color_weights(clip[k], pred[:3], pred[-1] if rot else None, (bw, bh), t, c["grid"], c["bins"],
                              c["lambda"], K)
        r = ref.update(L)
        if ALPHA > 0.0 and not r["held"]:
            st = np.array([[r["est"][0]], [r["est"][1]], [r["est"][2]]], np.float32)
            ang = np.array([r["extras"][-1]], np.float32) if rot else None
            p = R13.normalised(R13.histograms(clip[k], st, ang, (bw, bh), c["grid"], c["bins"]), c["grid"])[0]
            t = R13.blend(t, p, ALPHA)
        out.append({"L": L, "pred": pred, "r": r, "est": r["est"], "returned": r["returned"],
                    "dist": distance(r["returned"], k), "held": r["held"], "searched": r["searched"] if redetect else None,
                    "reacquired": r["reacquired"] if redetect else None, "streak": ref.held_frames,
                    "peak": float(r["m"]) / float(1 << K), "evidence": float(r["T"]) / (float(P) * float(1 << K)),
                    "t": t.copy()})
    return out


if __name__ == "__main__":      # the measurements quoted above
    import time
    clip = jump_clip()
    for s in SEEDS:
        t0 = time.time()
        run = follow_jump(clip, seed=s)
        first = next(k for k, f in enumerate(run, start=1) if k >= ABSENT[0] and not f["held"])
        late = {k: f["dist"] for k, f in enumerate(run, start=1) if k >= first + 4}
        print(f"seed {s}: held {[k for k, f in enumerate(run, start=1) if f['held']]} searched "
              f"{[k for k, f in enumerate(run, start=1) if f['searched']]} first not held {first} "
              f"dist there {run[first - 1]['dist']:.2f} worst from {first + 4} on {max(late.values()):.2f} "
              f"(frame {max(late, key=late.get)})  [{time.time() - t0:.1f} s]")
    ctl = follow_jump(clip, redetect=False)
    print(f"control: held {[k for k, f in enumerate(ctl, start=1) if f['held']]} streak {ctl[-1]['streak']} "
          f"final dist {ctl[-1]['dist']:.2f} at frame {REAPPEAR} {ctl[REAPPEAR - 1]['dist']:.2f}")
