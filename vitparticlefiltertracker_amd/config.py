"""Configuration surface: the `config.yaml` schema the reference names but does not ship.

The reference's only statement about configuration is "configure the tracking parameters in the
`config.yaml` file" (/root/reference/README.md:42); the key set below is the build's contract
 and SPEC.md gives each value its meaning.
"""
from __future__ import annotations

import copy
import dataclasses
import math
import os
from typing import Any, Dict, Optional

import yaml


@dataclasses.dataclass(frozen=True)
class ViTArch:
    """A ViT architecture: image size, patch, width, depth, heads, MLP width, LayerNorm eps."""

    name: str
    img_size: int
    patch: int
    dim: int
    depth: int
    heads: int
    mlp: int
    ln_eps: float = 1e-6

    @property
    def grid(self) -> int:
        return self.img_size // self.patch

    @property
    def n_patches(self) -> int:
        return self.grid * self.grid

    @property
    def tokens(self) -> int:
        return self.n_patches + 1

    @property
    def head_dim(self) -> int:
        return self.dim // self.heads

    @property
    def patch_k(self) -> int:
        return 3 * self.patch * self.patch

    @property
    def patch_kp(self) -> int:
        """Patch-GEMM K padded to the 64-deep K-step of the HIP GEMM (SPEC S3)."""
        return (self.patch_k + 63) // 64 * 64

    def gflop_per_crop(self) -> float:
        """Algorithmic FLOPs of one crop's forward (SURVEY.md §8d formula), in GFLOP."""
        n, N, D, L, H, hd, F = self.n_patches, self.tokens, self.dim, self.depth, self.heads, self.head_dim, self.mlp
        f = 2 * (n * self.patch_k * D + L * (N * D * 3 * D + 2 * H * N * N * hd + N * D * D + 2 * N * D * F))
        return f / 1e9

    def gflop_per_crop_executed(self, cls_fused: bool = True) -> float:
        """FLOPs of the work the product path performs per crop, in GFLOP: the full forward of blocks 0..L-2, and for
        the last block only what its CLS row needs (vit.py ViTEngine.encoder: the final LayerNorm reads nothing else).
        cls_fused (csrc/cls_attn.hip): the CLS query (2 D^2), G = W'_k^T q per head (2 D^2 useful), the folded
        attention's scores and weighted row sum over N tokens (4 N D H), W'_v per head (2 D^2 useful), proj (2 D^2),
        fc1 / fc2 (4 D F). Otherwise K and V for every row (4 N D^2), the CLS query, its attention (4 H N hd) and
        the CLS row's proj / MLP. The block-diagonal GEMMs' discarded products are not counted."""
        n, N, D, L, H, hd, F = self.n_patches, self.tokens, self.dim, self.depth, self.heads, self.head_dim, self.mlp
        full_block = N * D * 3 * D + 2 * H * N * N * hd + N * D * D + 2 * N * D * F
        if cls_fused:
            last = D * D + D * D + 2 * N * D * H + D * D + D * D + 2 * D * F
        else:
            last = 2 * N * D * D + D * D + 2 * H * N * hd + D * D + 2 * D * F
        f = 2 * (n * self.patch_k * D + (L - 1) * full_block + last)
        return f / 1e9

    def gflop_per_crop_mx8(self) -> float:
        """FLOPs per crop that the fp8 path (model.dtype: fp8) runs on block-scaled MX8 MFMA, in GFLOP: QKV, FC1 and FC2
        of blocks 0..L-2, and their proj when N <= 256 (the attention then writes MX8; vit.py ViTEngine.encoder). The
        patch embedding, the attention and the last block stay bf16."""
        N, D, L, F = self.tokens, self.dim, self.depth, self.mlp
        per_block = N * D * 3 * D + 2 * N * D * F + (N * D * D if N <= 256 else 0)
        return 2 * (L - 1) * per_block / 1e9


ARCHS: Dict[str, ViTArch] = {
    "vit_tiny_patch16_224": ViTArch("vit_tiny_patch16_224", 224, 16, 192, 12, 3, 768),
    "vit_small_patch16_224": ViTArch("vit_small_patch16_224", 224, 16, 384, 12, 6, 1536),
    "vit_base_patch16_224": ViTArch("vit_base_patch16_224", 224, 16, 768, 12, 12, 3072),
    "vit_large_patch14_336": ViTArch("vit_large_patch14_336", 336, 14, 1024, 24, 16, 4096),
}


DEFAULTS: Dict[str, Any] = {
    "model": {
        "arch": "vit_base_patch16_224",
        "dtype": "bf16",                 # bf16 (product) | fp8 (MX-fp8 encoder GEMMs, configs[4]) | fp32 (parity)
        "weights": {"seed": 0},
        "mean": [0.5, 0.5, 0.5],
        "std": [0.5, 0.5, 0.5],
    },
    "particles": {
        "num": 4096,
        "motion_std": [4.0, 4.0, 0.02],
        "scale_range": [0.5, 2.0],
        "seed": 1234,
        "motion_model": "random_walk",   # random_walk (SPEC S2) | constant_velocity (SPEC S11: a (vx, vy) per particle)
        "velocity_std": [1.0, 1.0],      # constant_velocity only: px/frame of velocity noise added per frame
        "velocity_decay": 1.0,           # constant_velocity only: d in [0, 1], v <- d * v + noise
        "velocity_max": 64.0,            # constant_velocity only: |vx|, |vy| <= this, px/frame
        "rotation_std": None,            # SPEC S12: None (axis-aligned boxes) or radians/frame of angle noise, >= 0
        "rotation_range": [-math.pi / 2, math.pi / 2],   # rotation_std only: angles are clamped to [amin, amax]
    },
    "likelihood": {"lambda": 20.0, "weight_bits": 40,
                   "template_update": 0.0,      # alpha: t <- normalise((1 - alpha) t + alpha f(estimate)); 0 = fixed
                   "color": None,               # SPEC S13: None (the ViT cue alone) or {bins, grid, lambda}: a colour-
                                                # histogram cue per particle, multiplied into the ViT weight
                   "color_surround": None,      # SPEC S14 (needs `color`): None or {lambda}: the ring around the box
                                                # scored against the same template, its resemblance penalised
                   "occlusion": None,           # SPEC S15: None or {threshold, noise_gain, max_hold}: hold the filter
                                                # while the frame's peak likelihood is below the threshold
                   "redetect": None,            # SPEC S16 (needs `occlusion`): None or {after, threshold}: after that
                                                # many held frames, search the whole frame for the target
                   "tokens": None},             # SPEC S18: None or {lambda}: the patch tokens of each particle scored
                                                # row by row against a spatial template, multiplied into the weight
    "resample": {"method": "systematic",        # systematic (SPEC S7) | stratified (SPEC S10)
                 "ess_threshold": None},        # tau in (0, 1]: resample only when N_eff < tau * P; None: every frame
    "input": {"source": "synthetic", "frames": 32, "height": 224, "width": 224,
              "bbox0": [80, 80, 64, 64], "seed": 7,
              "bboxes": None,                 # several targets (SPEC S9): [[x, y, w, h], ...]; main.py -> MultiTracker
              "angle0": 0.0,                  # SPEC S12 (particles.rotation_std only): bbox0's angle in radians
              "angles": None,                 # SPEC S12: one angle per box of `bboxes` (null: all 0)
              "target_range": None},          # synthetic source: [[rlo, rhi], [glo, ghi], [blo, bhi]] tints the target
    "distributed": {"world_size": 1},
    "estimate": None,                         # SPEC S17: None (SPEC S6's mean) or {method: mean | mode, window}
}


RESAMPLE_METHODS = ("systematic", "stratified")


def check_ess_threshold(tau) -> Optional[float]:
    """resample.ess_threshold (SPEC S10): None (resample every frame) or a float tau in (0, 1]."""
    if tau is None:
        return None
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not (math.isfinite(tau) and 0.0 < tau <= 1.0):
        raise ValueError(f"resample.ess_threshold must be null or a number in (0, 1] (SPEC S10), got {tau!r}")
    return float(tau)


MOTION_MODELS = ("random_walk", "constant_velocity")


def _number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)


def check_motion_model(model, velocity_std, velocity_decay, velocity_max):
    """particles.motion_model and, under constant_velocity (SPEC S11; otherwise they are not read), velocity_std =
    [svx, svy] finite and >= 0, velocity_decay in [0, 1], velocity_max finite and > 0. Returns the values as
    (model, [svx, svy], decay, vmax) floats."""
    if model not in MOTION_MODELS:
        raise ValueError(f"particles.motion_model must be one of {MOTION_MODELS} (SPEC S2, S11), got {model!r}")
    if model != "constant_velocity":
        return str(model), [1.0, 1.0], 1.0, 64.0
    if not isinstance(velocity_std, (list, tuple)) or len(velocity_std) != 2 \
            or not all(_number(v) and v >= 0 for v in velocity_std):
        raise ValueError(f"particles.velocity_std must be two finite numbers >= 0 (SPEC S11), got {velocity_std!r}")
    if not (_number(velocity_decay) and 0.0 <= velocity_decay <= 1.0):
        raise ValueError(f"particles.velocity_decay must be a number in [0, 1] (SPEC S11), got {velocity_decay!r}")
    if not (_number(velocity_max) and velocity_max > 0.0):
        raise ValueError(f"particles.velocity_max must be a finite number > 0 (SPEC S11), got {velocity_max!r}")
    return str(model), [float(v) for v in velocity_std], float(velocity_decay), float(velocity_max)


def check_rotation(rotation_std, rotation_range, angles=()):
    """particles.rotation_std (SPEC S12): None (no angle row; rotation_range is then not read) or sigma_a finite and
    >= 0 in radians per frame, with rotation_range = [amin, amax], -pi <= amin < amax <= pi, and every initial angle of
    `angles` inside the range. Returns (sigma_a or None, [amin, amax]) as floats."""
    if rotation_std is None:
        return None, [-math.pi / 2, math.pi / 2]
    if not (_number(rotation_std) and rotation_std >= 0):
        raise ValueError(f"particles.rotation_std must be null or a finite number >= 0 (SPEC S12), got {rotation_std!r}")
    if not isinstance(rotation_range, (list, tuple)) or len(rotation_range) != 2 \
            or not all(_number(v) for v in rotation_range) \
            or not -math.pi <= rotation_range[0] < rotation_range[1] <= math.pi:
        raise ValueError("particles.rotation_range must be [amin, amax] with -pi <= amin < amax <= pi (SPEC S12), got "
                         f"{rotation_range!r}")
    amin, amax = float(rotation_range[0]), float(rotation_range[1])
    for a in angles:
        if not (_number(a) and amin <= a <= amax):
            raise ValueError(f"initial angle {a!r} is outside particles.rotation_range [{amin}, {amax}] (SPEC S12)")
    return float(rotation_std), [amin, amax]


COLOR_DEFAULTS = {"bins": 8, "grid": 32, "lambda": 20.0}
COLOR_BINS = (4, 8, 16)
COLOR_GRIDS = (8, 16, 32, 64)


def check_color(color) -> Optional[Dict[str, Any]]:
    """likelihood.color (SPEC S13): None (no colour cue) or a mapping with the sub-keys `bins` (B per channel, one of
    4, 8, 16; default 8), `grid` (C x C samples per particle, C one of 8, 16, 32, 64; default 32) and `lambda` (finite
    and >= 0; default 20.0). Anything else, unknown sub-keys included, is refused. Returns None or the full mapping
    {"bins": int, "grid": int, "lambda": float}."""
    if color is None:
        return None
    if not isinstance(color, dict):
        raise ValueError(f"likelihood.color must be null or a mapping (SPEC S13), got {color!r}")
    unknown = sorted(set(color) - set(COLOR_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"likelihood.color: unknown key(s) {unknown}; known: {sorted(COLOR_DEFAULTS)} (SPEC S13)")
    c = {**COLOR_DEFAULTS, **color}
    if isinstance(c["bins"], bool) or not isinstance(c["bins"], int) or c["bins"] not in COLOR_BINS:
        raise ValueError(f"likelihood.color.bins must be one of {COLOR_BINS} (SPEC S13), got {c['bins']!r}")
    if isinstance(c["grid"], bool) or not isinstance(c["grid"], int) or c["grid"] not in COLOR_GRIDS:
        raise ValueError(f"likelihood.color.grid must be one of {COLOR_GRIDS} (SPEC S13), got {c['grid']!r}")
    if not (_number(c["lambda"]) and c["lambda"] >= 0):
        raise ValueError(f"likelihood.color.lambda must be finite and >= 0 (SPEC S13), got {c['lambda']!r}")
    return {"bins": int(c["bins"]), "grid": int(c["grid"]), "lambda": float(c["lambda"])}


COLOR_SURROUND_DEFAULTS = {"lambda": 10.0}


def check_color_surround(surround, color) -> Optional[Dict[str, Any]]:
    """likelihood.color_surround (SPEC S14): None (no surround cue) or a mapping with the single sub-key `lambda`
    (finite and >= 0; default 10.0). It needs `likelihood.color` (already normalised: `color`), whose bins and grid it
    shares; the ring's ratio is fixed at 2. Returns None or {"lambda": float}."""
    if surround is None:
        return None
    if not isinstance(surround, dict):
        raise ValueError(f"likelihood.color_surround must be null or a mapping (SPEC S14), got {surround!r}")
    unknown = sorted(set(surround) - set(COLOR_SURROUND_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"likelihood.color_surround: unknown key(s) {unknown}; known: "
                         f"{sorted(COLOR_SURROUND_DEFAULTS)} (SPEC S14)")
    s = {**COLOR_SURROUND_DEFAULTS, **surround}
    if not (_number(s["lambda"]) and s["lambda"] >= 0):
        raise ValueError(f"likelihood.color_surround.lambda must be finite and >= 0 (SPEC S14), got {s['lambda']!r}")
    if color is None:
        raise ValueError("likelihood.color_surround needs likelihood.color: the ring is scored against the colour "
                         "cue's template, with its bins and grid (SPEC S14)")
    return {"lambda": float(s["lambda"])}


OCCLUSION_DEFAULTS = {"threshold": 0.05, "noise_gain": 2.0, "max_hold": 30}


def check_occlusion(occlusion, ess_threshold=None) -> Optional[Dict[str, Any]]:
    """likelihood.occlusion (SPEC S15): None (no gate) or a mapping with the sub-keys `threshold` (theta, finite, in
    (0, 1]; default 0.05), `noise_gain` (g, finite, >= 1; default 2.0) and `max_hold` (an integer >= 0; default 30).
    Anything else, unknown sub-keys and bools for numbers included, is refused, and so is the gate together with
    resample.ess_threshold: a held frame under the ESS gate would need the prior-weighted estimate over the global
    carry, which the gathered chunk does not hold. Returns None or the full mapping
    {"threshold": float, "noise_gain": float, "max_hold": int}."""
    if occlusion is None:
        return None
    if not isinstance(occlusion, dict):
        raise ValueError(f"likelihood.occlusion must be null or a mapping (SPEC S15), got {occlusion!r}")
    unknown = sorted(set(occlusion) - set(OCCLUSION_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"likelihood.occlusion: unknown key(s) {unknown}; known: {sorted(OCCLUSION_DEFAULTS)} "
                         "(SPEC S15)")
    o = {**OCCLUSION_DEFAULTS, **occlusion}
    if not (_number(o["threshold"]) and 0.0 < o["threshold"] <= 1.0):
        raise ValueError(f"likelihood.occlusion.threshold must be a number in (0, 1] (SPEC S15), got "
                         f"{o['threshold']!r}")
    if not (_number(o["noise_gain"]) and o["noise_gain"] >= 1.0):
        raise ValueError(f"likelihood.occlusion.noise_gain must be finite and >= 1 (SPEC S15), got "
                         f"{o['noise_gain']!r}")
    if isinstance(o["max_hold"], bool) or not isinstance(o["max_hold"], int) or o["max_hold"] < 0:
        raise ValueError(f"likelihood.occlusion.max_hold must be an integer >= 0 (SPEC S15), got {o['max_hold']!r}")
    if ess_threshold is not None:
        raise ValueError("likelihood.occlusion cannot be combined with resample.ess_threshold: a held frame under the "
                         "ESS gate needs the prior-weighted estimate over the global carry (SPEC S15, out of scope)")
    return {"threshold": float(o["threshold"]), "noise_gain": float(o["noise_gain"]), "max_hold": int(o["max_hold"])}


def occlusion_gate_q(theta: float, bits: int) -> int:
    """SPEC S15: gate_q = floor(theta 2^K), exact (theta's own fp64 value times a power of two, in integers)."""
    from fractions import Fraction
    return int(Fraction(float(theta)) * (1 << int(bits)))


REDETECT_DEFAULTS = {"after": None, "threshold": None}


def check_redetect(redetect, occlusion) -> Optional[Dict[str, Any]]:
    """likelihood.redetect (SPEC S16): None (no search) or a mapping, `{}` included, with the sub-keys `after` (None: the
    search starts when the filter is `lost`, held_frames >= max_hold + 1; or an integer >= 1: when held_frames >= after)
    and `threshold` (theta_r, the gate of a search frame: None, meaning occlusion.threshold, or finite and in (0, 1]).
    Anything else, unknown sub-keys and bools for numbers included, is refused, and so is the key without
    likelihood.occlusion (already normalised: `occlusion`), whose gate and streak it runs on. Returns None or the full
    mapping {"after": int or None, "threshold": float or None}."""
    if redetect is None:
        return None
    if not isinstance(redetect, dict):
        raise ValueError(f"likelihood.redetect must be null or a mapping (SPEC S16), got {redetect!r}")
    unknown = sorted(set(redetect) - set(REDETECT_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"likelihood.redetect: unknown key(s) {unknown}; known: {sorted(REDETECT_DEFAULTS)} "
                         "(SPEC S16)")
    r = {**REDETECT_DEFAULTS, **redetect}
    if r["after"] is not None and (isinstance(r["after"], bool) or not isinstance(r["after"], int) or r["after"] < 1):
        raise ValueError(f"likelihood.redetect.after must be null or an integer >= 1 (SPEC S16), got {r['after']!r}")
    if r["threshold"] is not None and not (_number(r["threshold"]) and 0.0 < r["threshold"] <= 1.0):
        raise ValueError(f"likelihood.redetect.threshold must be null or a number in (0, 1] (SPEC S16), got "
                         f"{r['threshold']!r}")
    if occlusion is None:
        raise ValueError("likelihood.redetect needs likelihood.occlusion: the search starts from the gate's streak of "
                         "held frames and ends by its decision (SPEC S16)")
    return {"after": None if r["after"] is None else int(r["after"]),
            "threshold": None if r["threshold"] is None else float(r["threshold"])}


def redetect_after(redetect, occlusion) -> int:
    """SPEC S16: A, the streak of held frames from which the predict is the search: `after`, or max_hold + 1 (the
    filter is `lost`) when it is null."""
    return int(occlusion["max_hold"]) + 1 if redetect["after"] is None else int(redetect["after"])


def redetect_lattice(P: int, W: int, H: int):
    """SPEC S16: (gx, inv_gx, inv_P) of the search lattice over a W x H frame: gx the smallest integer >= 1 with
    gx^2 H >= P W (Python integers: exact), inv_gx = fp32(1) / fp32(gx) and inv_P = fp32(1) / fp32(P), one IEEE
    division each, returned as floats that hold the fp32 values."""
    import numpy as np
    P, W, H = int(P), int(W), int(H)
    if P < 1 or W < 1 or H < 1:
        raise ValueError(f"redetect_lattice: P, W, H must be >= 1, got {(P, W, H)}")
    gx = max(1, math.isqrt((P * W) // H))
    while gx * gx * H < P * W:
        gx += 1
    while gx > 1 and (gx - 1) * (gx - 1) * H >= P * W:
        gx -= 1
    one = np.float32(1.0)
    return gx, float(one / np.float32(gx)), float(one / np.float32(P))


TOKENS_DEFAULTS = {"lambda": 20.0}


def check_tokens(tokens) -> Optional[Dict[str, Any]]:
    """likelihood.tokens (SPEC S18): None (no patch-token cue) or a mapping, `{}` included, with the single sub-key
    `lambda` (finite and >= 0; default 20.0). Anything else, unknown sub-keys and a bool for the number included, is
    refused. Returns None or {"lambda": float}."""
    if tokens is None:
        return None
    if not isinstance(tokens, dict):
        raise ValueError(f"likelihood.tokens must be null or a mapping (SPEC S18), got {tokens!r}")
    unknown = sorted(set(tokens) - set(TOKENS_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"likelihood.tokens: unknown key(s) {unknown}; known: {sorted(TOKENS_DEFAULTS)} (SPEC S18)")
    t = {**TOKENS_DEFAULTS, **tokens}
    if not (_number(t["lambda"]) and t["lambda"] >= 0):
        raise ValueError(f"likelihood.tokens.lambda must be finite and >= 0 (SPEC S18), got {t['lambda']!r}")
    return {"lambda": float(t["lambda"])}


ESTIMATE_DEFAULTS = {"method": "mean", "window": 0.5}
ESTIMATE_METHODS = ("mean", "mode")


def check_estimate(estimate) -> Optional[Dict[str, Any]]:
    """estimate (SPEC S17): None (SPEC S6's weighted mean, nothing else) or a mapping, `{}` included, with the sub-keys
    `method` (`mean`, the default and the same as None, or `mode`: the local weighted mean of the posterior's densest
    cluster) and `window` (omega, finite and > 0; default 0.5: the window's half-width in units of the template box's
    side). Anything else, unknown sub-keys and bools for numbers included, is refused. Returns None (also for method
    `mean`, whose window is checked and then not used) or {"method": "mode", "window": float}."""
    if estimate is None:
        return None
    if not isinstance(estimate, dict):
        raise ValueError(f"estimate must be null or a mapping (SPEC S17), got {estimate!r}")
    unknown = sorted(set(estimate) - set(ESTIMATE_DEFAULTS), key=str)
    if unknown:
        raise ValueError(f"estimate: unknown key(s) {unknown}; known: {sorted(ESTIMATE_DEFAULTS)} (SPEC S17)")
    e = {**ESTIMATE_DEFAULTS, **estimate}
    if not isinstance(e["method"], str) or e["method"] not in ESTIMATE_METHODS:
        raise ValueError(f"estimate.method must be one of {ESTIMATE_METHODS} (SPEC S17), got {e['method']!r}")
    if not (_number(e["window"]) and e["window"] > 0.0):
        raise ValueError(f"estimate.window must be a finite number > 0 (SPEC S17), got {e['window']!r}")
    if e["method"] == "mean":
        return None
    return {"method": "mode", "window": float(e["window"])}


def estimate_window(estimate, box_wh):
    """SPEC S17: (hx, hy) = (fp32(omega w0), fp32(omega h0)) of a target's template box, each an fp64 product rounded
    once to fp32, returned as floats that hold the fp32 values; None without the mode estimate."""
    if estimate is None:
        return None
    import numpy as np
    return (float(np.float32(estimate["window"] * float(box_wh[0]))),
            float(np.float32(estimate["window"] * float(box_wh[1]))))


def check_target_range(tr):
    """input.target_range: None or three [lo, hi] integer pairs with 0 <= lo < hi <= 256, one per channel (R, G, B):
    the synthetic target's texture is mapped into [lo, hi) per channel (frames.synthetic_clip). Returns None or a tuple
    of three (lo, hi) tuples."""
    if tr is None:
        return None
    ok = isinstance(tr, (list, tuple)) and len(tr) == 3 and all(
        isinstance(r, (list, tuple)) and len(r) == 2
        and all(isinstance(v, int) and not isinstance(v, bool) for v in r) and 0 <= r[0] < r[1] <= 256 for r in tr)
    if not ok:
        raise ValueError("input.target_range must be null or [[rlo, rhi], [glo, ghi], [blo, bhi]] with integers "
                         f"0 <= lo < hi <= 256, got {tr!r}")
    return tuple((int(r[0]), int(r[1])) for r in tr)


def _merge(base: Dict[str, Any], over: Dict[str, Any]) -> Dict[str, Any]:
    out = copy.deepcopy(base)
    for k, v in (over or {}).items():
        if isinstance(v, dict) and isinstance(out.get(k), dict):
            out[k] = _merge(out[k], v)
        else:
            out[k] = copy.deepcopy(v)
    return out


def load_config(cfg: Optional[Any] = None) -> Dict[str, Any]:
    """Accept a path to a YAML file, a dict (partial is fine) or None; return the full config dict."""
    if cfg is None:
        user = {}
    elif isinstance(cfg, (str, os.PathLike)):
        with open(cfg, "r") as fh:
            user = yaml.safe_load(fh) or {}
    elif isinstance(cfg, dict):
        user = cfg
    else:
        raise TypeError(f"config must be a path, dict or None, got {type(cfg).__name__}")
    out = _merge(DEFAULTS, user)
    arch = out["model"]["arch"]
    if arch not in ARCHS:
        raise ValueError(f"unknown model.arch {arch!r}; known: {sorted(ARCHS)}")
    if out["model"]["dtype"] not in ("bf16", "fp8", "fp32"):
        raise ValueError("model.dtype must be 'bf16', 'fp8' or 'fp32'")
    lam = float(out["likelihood"]["lambda"])
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("likelihood.lambda must be finite and >= 0 (SPEC S5)")
    if not 0.0 <= float(out["likelihood"]["template_update"]) <= 1.0:
        raise ValueError("likelihood.template_update must be in [0, 1]")
    out["likelihood"]["color"] = check_color(out["likelihood"]["color"])      # SPEC S13: None or the full mapping
    out["likelihood"]["color_surround"] = check_color_surround(out["likelihood"]["color_surround"],
                                                               out["likelihood"]["color"])     # SPEC S14
    out["likelihood"]["occlusion"] = check_occlusion(out["likelihood"]["occlusion"],
                                                     out["resample"]["ess_threshold"])          # SPEC S15
    out["likelihood"]["redetect"] = check_redetect(out["likelihood"]["redetect"],
                                                   out["likelihood"]["occlusion"])              # SPEC S16
    out["likelihood"]["tokens"] = check_tokens(out["likelihood"].get("tokens"))                 # SPEC S18
    out["estimate"] = check_estimate(out.get("estimate"))                                       # SPEC S17
    check_target_range(out["input"].get("target_range"))
    if out["resample"]["method"] not in RESAMPLE_METHODS:
        raise ValueError(f"resample.method must be one of {RESAMPLE_METHODS} (SPEC S7, S10)")
    check_ess_threshold(out["resample"]["ess_threshold"])
    p = out["particles"]
    check_motion_model(p["motion_model"], p["velocity_std"], p["velocity_decay"], p["velocity_max"])
    boxes = out["input"].get("bboxes")
    if boxes is not None:
        if not isinstance(boxes, (list, tuple)) or not boxes:
            raise ValueError("input.bboxes must be a non-empty list of [x, y, w, h] boxes (or null)")
        for b in boxes:
            if not isinstance(b, (list, tuple)) or len(b) != 4 or not all(math.isfinite(float(v)) for v in b) \
                    or float(b[2]) <= 0 or float(b[3]) <= 0:
                raise ValueError(f"input.bboxes: {b!r} is not an [x, y, w, h] box with w, h > 0")
    if p["rotation_std"] is not None:       # SPEC S12; with the default none of these keys is read
        angles = out["input"].get("angles")
        if angles is not None and (not isinstance(angles, (list, tuple)) or boxes is None or len(angles) != len(boxes)):
            raise ValueError("input.angles must be null or one angle per box of input.bboxes (SPEC S12)")
        check_rotation(p["rotation_std"], p["rotation_range"], [out["input"].get("angle0", 0.0)] + list(angles or []))
    return out


def arch_of(cfg: Dict[str, Any]) -> ViTArch:
    return ARCHS[cfg["model"]["arch"]]
