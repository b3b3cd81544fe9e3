"""SPEC S17 (mode estimate: the local weighted mean of the posterior's densest cluster) restated in Python ints and numpy
float32, one rounding per operation: the reference of tests/test_s17_*.py, on top of s15_reference (the device-order
sums) and s16_reference (the recursion with the gate and the search, and the jump clip of the behaviour run).

Measured with this reference on the CPU (`python tests/s17_reference.py`; recorded in DESIGN.md §15), the twin run:
the jump clip with a second, identical copy of the tinted texture standing at TWIN_AT from the reappearance frame on,
colour-only, redetect on, P = 1024, omega = 0.5 (hx = hy = 32 px), alpha = 0.3, seeds 1234, 1 and 2:
  1. frames 9..15 are held (12..15 as search frames) and frame 16, the reappearance, is the first that is not, for each
     seed: the recursion up to there is s16_reference's.
  2. the mode run (condition): from frame 16 on every returned estimate lies inside the window (|dx| <= 32, |dy| <= 32) of
     the nearer copy's centre, for each seed; the copy it reports changes from the target's to the twin's in frame 22
     (seed 1234), 17 (seed 1) and 19 (seed 2), as the feature does not promise which. Its worst distance to the nearer
     copy's centre over frames 16..27 is 2.63 px (seed 1234, frame 21), 2.75 px (seed 1, frame 17) and 2.56 px (seed 2,
     frame 18); frame 16's own is 1.92 / 1.03 / 1.59 px. The bound is 1.5 x the largest, 4.125 px, and must itself be
     < 16 px (a quarter of the box side).
  3. the control (condition): frame 16's SPEC S6 mean, (243.5, 243.6) / (240.8, 239.6) / (249.4, 246.4), is 145.03 /
     149.60 / 138.67 px from the nearer copy: on the background between them, farther than 2 max(hx, hy) = 64 px from
     both. The mean-reporting tracker with the same seeds returns it (and learns it: alpha = 0.3) and stays more than
     100 px from either copy through frame 19 (20 for seed 2).
  4. the mode mass Tm / T in frame 16 is 0.512 / 0.498 / 0.532: half the posterior is elsewhere.
"""
import numpy as np

import s10_reference as R10
import s13_reference as R13
import s15_reference as R15
import s16_reference as R16

f32 = np.float32
DEFAULTS = {"method": "mean", "window": 0.5}


# ---------------------------------------------------------------------------------------------- the definition
def window(omega: float, box_wh):
    """(hx, hy) = (fp32(omega w0), fp32(omega h0)): an fp64 product rounded once to fp32."""
    return f32(float(omega) * float(box_wh[0])), f32(float(omega) * float(box_wh[1]))


def in_window(xa, ya, x: np.ndarray, y: np.ndarray, hx, hy) -> np.ndarray:
    """in(a, j) for every j: fabsf(x_a - x_j) <= hx and fabsf(y_a - y_j) <= hy, one rounded fp32 subtraction per axis,
    inclusive; False where anything is NaN (inf - inf included). xa, ya: scalars, or columns for a block of seeds."""
    assert x.dtype == np.float32 and y.dtype == np.float32
    with np.errstate(invalid="ignore"):
        dx = np.abs(np.asarray(xa, np.float32) - x)
        dy = np.abs(np.asarray(ya, np.float32) - y)
        assert dx.dtype == np.float32 and dy.dtype == np.float32
        return (dx <= f32(hx)) & (dy <= f32(hy))


def density(w, x: np.ndarray, y: np.ndarray, hx, hy) -> np.ndarray:
    """D_i = sum_j w_j in(i, j), int64[P]: an exact integer sum (the caller keeps sum w <= 2^62), here in blocks of 256
    seeds by an int64 matrix product."""
    wv = np.array([int(q) for q in w], np.int64)
    assert sum(int(q) for q in w) <= 1 << 62
    P = len(wv)
    D = np.empty(P, np.int64)
    for b in range(0, P, 256):
        m = in_window(x[b:b + 256, None], y[b:b + 256, None], x[None, :], y[None, :], hx, hy)
        D[b:b + 256] = m.astype(np.int64) @ wv
    return D


def mode(Q, states: np.ndarray, hx, hy, uniform: bool) -> dict:
    """SPEC S17 of one frame: states float32[3 + n_extra][P] as predicted, Q the frame's global weights; `uniform` (T == 0
    or the frame is held): every weight counts as 1. D, i* (largest D, smallest index), Tm = D_i*, `sums`: the device-
    order fp64 sums of every row over the weights w_j in(i*, j), a particle outside the window contributing +0 whatever
    its state holds; `est`: sums / Tm, or None when Tm == 0 (the caller keeps SPEC S6's mean)."""
    states = np.ascontiguousarray(states, np.float32)
    P = states.shape[1]
    w = [1] * P if uniform else [int(q) for q in Q]
    x, y = states[0], states[1]
    D = density(w, x, y, hx, hy)
    i = int(np.argmax(D))                       # numpy's argmax returns the first maximum: the smallest index
    assert D[i] == D.max() and not (D[:i] == D[i]).any()
    m = in_window(x[i], y[i], x, y, hx, hy)
    wm = [q if k else 0 for q, k in zip(w, m)]
    sums = R15.tree_sums(wm, np.where(m[None, :], states, f32(0.0)))
    Tm = sum(wm)
    assert Tm == int(D[i])
    return {"D": D, "i": i, "Tm": Tm, "sums": sums, "est": tuple(s / float(Tm) for s in sums) if Tm else None}


def out_words(r: dict) -> np.ndarray:
    """vpf_mode_estimate's out int64[8] for mode()'s result."""
    o = np.zeros(8, np.int64)
    o[0], o[1] = r["i"], r["Tm"]
    o[2:2 + len(r["sums"])] = np.array(r["sums"], np.float64).view(np.int64)
    return o


# ---------------------------------------------------------------------------------------------- the recursion
class Filter(R16.Filter):
    """s16_reference.Filter reporting the mode: the recursion (predict, gate, resample, streak) is untouched; `est` and
    `extras` become the window's, `mean` / `mean_extras` keep SPEC S6's, the anchor remembers what was returned."""

    def __init__(self, *args, window_px, **kw):
        super().__init__(*args, **kw)
        self.hx, self.hy = window_px

    def update(self, L) -> dict:
        pred, anchor = self.state.copy(), self.anchor
        r = super().update(L)
        uniform = r["held"] or r["T"] == 0
        m = mode(L, pred, self.hx, self.hy, uniform)
        r["mean"], r["mean_extras"], r["mode"] = r["est"], r["extras"], m
        r["mass"] = float(m["Tm"]) / (float(self.P) if uniform else float(r["T"]))
        if m["est"] is not None:
            r["est"], r["extras"] = m["est"][:3], m["est"][3:]
        self.anchor = anchor if self.searched else r["est"]
        r["returned"] = self.anchor if self.searched and r["held"] else r["est"]
        return r


# ---------------------------------------------------------------------------------------------- the behaviour run
# s16_reference's jump clip; from the reappearance frame (16) on a second copy of the same tinted texture stands still
# at TWIN_AT, more than 200 px from the returning target, which moves from (360, 330) by (-2, -1) per frame.
TWIN_AT = (120, 150)
OMEGA = 0.5
SEEDS = R16.SEEDS
FIRST = R16.REAPPEAR            # the first frame that is not held, for each seed (measured)
MODE_WORST_PX = {1234: 2.63, 1: 2.75, 2: 2.56}
MODE_BOUND_PX = 1.5 * max(MODE_WORST_PX.values())
MEAN_NEAREST_PX = {1234: 145.03, 1: 149.60, 2: 138.67}   # frame FIRST's S6 mean to the nearer copy (the control)


def copies(k: int):
    """The centres of the two copies in frame k >= REAPPEAR: the returning target's, the twin's."""
    return R16.truth(k), (float(TWIN_AT[0]), float(TWIN_AT[1]))


def twin_clip(frames: int = R16.FRAMES) -> np.ndarray:
    clip = R16.jump_clip(frames).copy()
    bx, by, bw, bh = R13.FOLLOW["box"]
    tex = clip[0, by:by + bh, bx:bx + bw].copy()
    cx, cy = TWIN_AT
    assert min(np.hypot(cx - t[0], cy - t[1]) for t in (R16.truth(k) for k in range(R16.REAPPEAR, frames))) >= 200.0
    for k in range(R16.REAPPEAR, frames):
        clip[k, cy - bh // 2:cy + bh // 2, cx - bw // 2:cx + bw // 2] = tex
    return clip


def offsets(est, k: int):
    """(|dx|, |dy|, distance) of `est` to the nearer copy's centre in frame k, and that copy's index."""
    d = [(abs(est[0] - c[0]), abs(est[1] - c[1]), float(np.hypot(est[0] - c[0], est[1] - c[1]))) for c in copies(k)]
    n = 0 if d[0][2] <= d[1][2] else 1
    return d[n], n


def follow_twin(clip, report_mode: bool, seed=None, P=R16.P_RUN, frames=None, cv=None, rot=None, omega=OMEGA):
    """s16_reference.follow_jump's colour-only run under the gate and the search, reporting the mode (report_mode) or the
    mean: per tracked frame a dict: L, pred, r (the filter's result), est, returned, held, searched, reacquired, streak,
    peak, evidence, t (the colour template after the frame), and with the mode: mean, mass, index."""
    c = dict(R13.DEFAULTS)
    F = R13.FOLLOW
    bx, by, bw, bh = F["box"]
    K = F["K"]
    gq = R15.gate_q(R16.THETA, K)
    A = R16.search_after(R16.AFTER, R16.MAX_HOLD)
    t = R13.template(clip[0], (bx, by, bw, bh), 0.0 if rot else None, c["grid"], c["bins"])
    init = (bx + 0.5 * bw, by + 0.5 * bh, 1.0) + ((0.0, 0.0) if cv else ()) + ((0.0,) if rot else ())
    args = (P, init, F["motion_std"], F["scale_range"], F["seed"] if seed is None else seed, (R16.SIDE, R16.SIDE), K,
            R10.SYSTEMATIC, gq, R16.GAIN, A, gq, cv, rot)
    ref = Filter(*args, window_px=window(omega, (bw, bh))) if report_mode else R16.Filter(*args)
    out = []
    for k in range(1, len(clip) if frames is None else frames + 1):
        ref.predict(k)
        pred = ref.state.copy()
        L = R13.color_weights(clip[k], pred[:3], pred[-1] if rot else None, (bw, bh), t, c["grid"], c["bins"],
                              c["lambda"], K)
        r = ref.update(L)
        if R16.ALPHA > 0.0 and not r["held"]:
            st = np.array([[r["est"][0]], [r["est"][1]], [r["est"][2]]], np.float32)
            ang = np.array([r["extras"][-1]], np.float32) if rot else None
            p = R13.normalised(R13.histograms(clip[k], st, ang, (bw, bh), c["grid"], c["bins"]), c["grid"])[0]
            t = R13.blend(t, p, R16.ALPHA)
        out.append({"L": L, "pred": pred, "r": r, "est": r["est"], "returned": r["returned"], "held": r["held"],
                    "searched": r["searched"], "reacquired": r["reacquired"], "streak": ref.held_frames,
                    "peak": float(r["m"]) / float(1 << K), "evidence": float(r["T"]) / (float(P) * float(1 << K)),
                    "t": t.copy(), "mean": r.get("mean"), "mass": r.get("mass"),
                    "index": r["mode"]["i"] if report_mode else None})
    return out


if __name__ == "__main__":      # the measurements quoted above
    import time
    clip = twin_clip()
    hx, hy = window(OMEGA, R13.FOLLOW["box"][2:])
    print("twin at", TWIN_AT, "window", float(hx), float(hy))
    for s in SEEDS:
        t0 = time.time()
        run = follow_twin(clip, True, seed=s)
        first = next(k for k, f in enumerate(run, start=1) if k >= R16.ABSENT[0] and not f["held"])
        off = {k: offsets(f["returned"], k) for k, f in enumerate(run, start=1) if k >= first}
        ok = all(o[0][0] <= hx and o[0][1] <= hy for o in off.values())
        worst = max(off, key=lambda k: off[k][0][2])
        mean0 = run[first - 1]["mean"]
        dm = [float(np.hypot(mean0[0] - c[0], mean0[1] - c[1])) for c in copies(first)]
        print(f"seed {s}: first not held {first}; mode inside the window on every frame: {ok}; worst distance "
              f"{off[worst][0][2]:.2f} px (frame {worst}); copy per frame {[o[1] for o in off.values()]}; mass "
              f"{[round(f['mass'], 3) for f in run[first - 1:]]}")
        print(f"   frame {first}: mode distance {off[first][0][2]:.2f}, S6 mean of the same frame "
              f"({mean0[0]:.1f}, {mean0[1]:.1f}) is {dm[0]:.2f} / {dm[1]:.2f} px from the copies "
              f"(needs > {2 * max(hx, hy):.0f})  [{time.time() - t0:.1f} s]")
        ctl = follow_twin(clip, False, seed=s)
        cf = next(k for k, f in enumerate(ctl, start=1) if k >= R16.ABSENT[0] and not f["held"])
        co = {k: offsets(f["returned"], k)[0][2] for k, f in enumerate(ctl, start=1) if k >= cf}
        print(f"   mean-reporting twin: first not held {cf}, distance to the nearer copy per frame "
              f"{[round(v, 1) for v in co.values()]}")
