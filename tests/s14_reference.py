"""SPEC S14 (colour cue with a surround ring) restated in numpy: the reference of tests/test_s14_*.py, built on
s13_reference (bins, the pinned sum, the box's histogram, the template) and s12_reference (sample coordinates, the
bilinear value). Every fp32 operation is one numpy float32 operation. The ring is the C x C sample grid of the box
doubled about its centre, without its central C/2 x C/2 samples; it is scored against the TARGET's template and the
resemblance is penalised: Ls = weights_to_Q(1 - min(rho_s, 1), lambda_s, K)."""
import numpy as np

import s10_reference as R10
import s12_reference as R12
import s13_reference as R13
from oracle import pf as opf

f32 = np.float32
DEFAULTS = {"lambda": 10.0}
RATIO = 2               # fixed (SPEC S14): the outer box is the box doubled


def ring_mask(C: int) -> np.ndarray:
    """bool[C(oy)][C(ox)]: True on the ring, ox or oy outside [C/4, 3C/4); 3 C^2 / 4 samples."""
    o = np.arange(C)
    inner = (o >= C // 4) & (o < 3 * C // 4)
    return ~(inner.reshape(C, 1) & inner.reshape(1, C))


def ring_count(C: int) -> int:
    return 3 * C * C // 4


def finite_states(particles, angles) -> np.ndarray:
    ok = np.isfinite(np.asarray(particles, np.float32)).all(axis=0)
    return ok if angles is None else ok & np.isfinite(np.asarray(angles, np.float32).reshape(-1))


def _bins(frame, particles, angles, box_wh, C: int, B: int) -> np.ndarray:
    """int[n][C][C]: every sample's bin for the box box_wh. A non-finite state's samples all have NaN values, which
    the kernel's (int) conversion turns into 0: bin 0."""
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    particles = np.asarray(particles, np.float32)
    n = particles.shape[1]
    ok = finite_states(particles, angles)
    safe = np.where(ok.reshape(1, n), particles, f32(1.0)).astype(np.float32)
    if angles is None:
        sx, sy = R12.s3_coords(safe, box_wh, C)
        sx, sy = np.broadcast_to(sx, (n, C, C)), np.broadcast_to(sy, (n, C, C))
    else:
        ang = np.where(ok, np.asarray(angles, np.float32).reshape(-1), f32(0.0)).astype(np.float32)
        sx, sy = R12.sample_coords(safe, ang, box_wh, C)
    b = R13.bin_index(R12.bilinear(frame, sx, sy), B).reshape(n, C, C)
    b[~ok] = 0
    return b


def _count(b: np.ndarray, B: int) -> np.ndarray:
    return np.stack([np.bincount(row, minlength=B ** 3) for row in b]).astype(np.int64)


def histograms(frame, particles, angles, box_wh, C: int, B: int) -> np.ndarray:
    """S13's h int64[n][B^3] (the box's C x C samples); equal to s13_reference.histograms on finite states."""
    n = np.asarray(particles).shape[1]
    return _count(_bins(frame, particles, angles, box_wh, C, B).reshape(n, C * C), B)


def ring_histograms(frame, particles, angles, box_wh, C: int, B: int) -> np.ndarray:
    """hs int64[n][B^3]: the bin counts of the ring's 3 C^2 / 4 samples. The outer grid is S3's / S12's with
    (w0, h0) -> (2 w0, 2 h0), the doubling exact in fp32."""
    outer = (f32(RATIO) * f32(box_wh[0]), f32(RATIO) * f32(box_wh[1]))
    b = _bins(frame, particles, angles, outer, C, B)
    return _count(b[:, ring_mask(C)], B)


def rho_lanes_over(h: np.ndarray, t: np.ndarray, den: int) -> np.ndarray:
    """S13's pinned sum over term_b = sqrt(fp32(fp32(fp32(h_b) / fp32(den)) t_b)): float32[n][64] after the butterfly."""
    t = np.asarray(t, np.float32)
    n, nb = h.shape
    assert t.shape == (nb,) and nb % 64 == 0
    p = h.astype(np.float32) / f32(den)
    term = np.sqrt(p * t.reshape(1, nb)).reshape(n, nb // 64, 64)
    assert term.dtype == np.float32
    acc = np.zeros((n, 64), np.float32)
    for r in range(nb // 64):
        acc = acc + term[:, r]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    assert acc.dtype == np.float32
    return acc


def rho_s(hs, t, C: int, finite=None) -> np.ndarray:
    """rho_s float32[n]: the ring's Bhattacharyya coefficient against the template; NaN for a non-finite state."""
    r = np.ascontiguousarray(rho_lanes_over(hs, t, ring_count(C))[:, 0])
    if finite is not None:
        r[~np.asarray(finite, bool)] = np.float32("nan")
    return r


def surround_weights(rs: np.ndarray, lam_s: float, K: int) -> np.ndarray:
    """Ls = floor(fixed_expf(lam_s (min(sim_s, 1) - 1)) 2^K) with sim_s = 1.0f - fminf(rho_s, 1.0f); 0 for a non-finite
    rho_s (fminf would drop the NaN, so it is kept by hand)."""
    rs = np.asarray(rs, np.float32)
    with np.errstate(invalid="ignore"):
        sim = np.where(np.isfinite(rs), f32(1.0) - np.fmin(rs, f32(1.0)), np.float32("nan")).astype(np.float32)
    return opf.weights_to_Q(sim, lam_s, K)


def combine(Lv, Lc, Ls, K: int):
    """L = (((Lv Lc) >> K) Ls) >> K, or (Lc Ls) >> K without the ViT weight (Lv None): exact Python integers."""
    if Lv is None:
        return [(int(c) * int(s)) >> K for c, s in zip(Lc, Ls)]
    return [(((int(v) * int(c)) >> K) * int(s)) >> K for v, c, s in zip(Lv, Lc, Ls)]


def cue(frame, particles, angles, box_wh, t, C, B, lam_c, lam_s, K) -> dict:
    """Everything the kernel reports for one call: h, hs, rho, rho_s, Lc, Ls (numpy arrays)."""
    h = histograms(frame, particles, angles, box_wh, C, B)
    hs = ring_histograms(frame, particles, angles, box_wh, C, B)
    r = R13.rho(h, t, C)
    rs = rho_s(hs, t, C, finite_states(particles, angles))
    return {"h": h, "hs": hs, "rho": r, "rho_s": rs, "Lc": R13.weights(r, lam_c, K),
            "Ls": surround_weights(rs, lam_s, K)}


# ---------------------------------------------------------------------------------------------- the follow-the-target run
# S13's FOLLOW set-up (colour only, the tinted 24-frame clip) with the ring at lambda_s = 10. Measured on the CPU with
# this reference, 2026-10-20 (recorded in DESIGN.md): the scale estimate stays within FOLLOW_SCALE_DEV of 1 (S13 alone
# drifts by 0.18) and the worst frame is FOLLOW_WORST_PX from the true centre (S13 alone: 3.69 px). Each bound is the
# measured value x 1.5 and must stay below 0.06 (a third of S13's drift) and below S13's FOLLOW_BOUND_PX.
FOLLOW = R13.FOLLOW
FOLLOW_LAMBDA_S = 10.0
FOLLOW_SCALE_DEV = 0.0189       # max |s_hat - 1| over frames 1..23 (frame estimates in [0.9983, 1.0189]), 2026-10-20
FOLLOW_WORST_PX = 1.43          # worst-frame distance to the true centre, 2026-10-20
FOLLOW_SCALE_BOUND = 1.5 * FOLLOW_SCALE_DEV
FOLLOW_BOUND_PX = 1.5 * FOLLOW_WORST_PX


def follow(clip, lam_s=FOLLOW_LAMBDA_S, color=None):
    """s13_reference.follow with L = (Lc Ls) >> K: a list of per-frame dicts {L, Lc, Ls, pred, r, est, dist}."""
    c = {**R13.DEFAULTS, **(color or {})}
    F = FOLLOW
    bx, by, bw, bh = F["box"]
    t = R13.template(clip[0], F["box"], None, c["grid"], c["bins"])
    ref = R10.Filter(F["P"], (bx + 0.5 * bw, by + 0.5 * bh, 1.0), F["motion_std"], F["scale_range"], F["seed"],
                     F["frame_size"], F["K"], R10.SYSTEMATIC, None)
    out = []
    for k in range(1, len(clip)):
        ref.predict(k)
        pred = ref.particles.copy()
        q = cue(clip[k], pred, None, (bw, bh), t, c["grid"], c["bins"], c["lambda"], lam_s, F["K"])
        L = np.array(combine(None, q["Lc"], q["Ls"], F["K"]), np.int64)
        r = ref.update(L)
        r = dict(r, states=r["states"].copy())      # the filter predicts in place on the array it returned
        est = R10.estimate(r, F["P"])
        tx, ty = R13.truth(k)
        out.append({"L": L, "Lc": q["Lc"], "Ls": q["Ls"], "pred": pred, "r": r, "est": est,
                    "dist": float(np.hypot(est[0] - tx, est[1] - ty))})
    return out
