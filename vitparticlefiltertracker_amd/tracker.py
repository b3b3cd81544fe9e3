"""`Tracker` — the per-frame loop the reference drives from main.py ("integrates the Vision Transformer
(ViT) architecture with a Particle Filter to achieve precise object position tracking",
/root/reference/README.md:3; "provide the input data ... configure ... config.yaml ... output the tracked
positions", README.md:42). SPEC.md S8 / SURVEY.md §8a H13-H14.

    t = Tracker("config.yaml")        # or a dict, or None for the defaults
    t.init(frame0, (x, y, w, h))      # template feature from the bbox crop (H13)
    for f in frames: x, y, s = t.track(f)

`MultiTracker(cfg, K)` follows K targets the same way: `init(frame0, boxes)`, `track(f)` -> K estimates. Both are
`_TargetLoop`, the one frame loop over K targets below (one filter per target, one batched ViT pass over every target's
particles); `Tracker` is its K = 1 case with scalar results, `MultiTracker` has a list with one entry per target
wherever `Tracker` has a value. Everything that follows is said once, for one target, and holds per target.

Per frame: predict (eager launch; its frame index is a kernel argument) -> [HIP graph replay: crop+ViT
-> final LN -> cosine -> Q] -> (world > 1: one all-gather of the shard chunks) -> estimate + resample on the
device (vpf_estimate_resample). The only host synchronisation is reading the 32-B estimate statistics.
With `particles.motion_model: constant_velocity` (SPEC S11) every particle also carries a velocity: predict is
vpf_predict_cv, the velocity rows ride in the same all-gather, and `last_velocity` is the frame's velocity estimate.
With `particles.rotation_std` (SPEC S12) every particle carries an angle: vpf_predict_angle follows the motion model's
predict, the crop in the graph is vpf_crop_patches_rot_*, the angle row rides in the same all-gather, `init` takes the
box's initial angle and `last_rotation` is the frame's angle estimate.
With `likelihood.color` (SPEC S13) a colour-histogram cue multiplies the ViT weight: vpf_color_weight follows
vpf_cls_weight inside the graph, `init` takes the box's histogram as `color_template` (updated with the CLS template
under `likelihood.template_update`, kept in checkpoints). With the default `null` none of this exists.
With `likelihood.color_surround` (SPEC S14) that launch is vpf_color_weight_surround: the same cue fused with one over
the ring around the box, scored against the same template and penalised; no new state.
With `likelihood.tokens` (SPEC S18) a patch-token cue multiplies the CLS weight: vpf_token_weight follows vpf_cls_weight
inside the graph (before the colour launch) and scores every patch-token row of a particle's crop against its own row
of `token_template` (f32[N-1][D], taken at `init` from the same forward as the CLS template, updated with it, kept in
checkpoints); `last_token_sim` holds the frame's mean cosines. With the default `null` none of this exists.
With `likelihood.occlusion` (SPEC S15) the estimate + resample call is vpf_estimate_resample_gate: a frame whose peak
likelihood is below the threshold is held (decided on the device: plain-mean estimate, no resample), its template
updates are skipped and the next frame's position noise is widened; `last_held`, `last_peak`, `last_evidence`,
`held_frames` and `lost` report it. With the default `null` none of this exists.
With `likelihood.redetect` (SPEC S16) a frame whose streak of held frames has reached `after` (default: `lost`) is
predicted by vpf_predict_search instead: the particles are scattered over the whole frame and gated with the search
threshold; the first such frame that is not held collapses them onto the target and tracking resumes. While the search
is held `track()` returns the last estimate from before it; `last_searched` and `last_reacquired` report it. With the
default `null` none of this exists.
With `estimate: {method: mode}` (SPEC S17) vpf_mode_estimate follows the estimate + resample call: `track()` returns the
local weighted mean of the posterior's densest cluster (window: `estimate.window` x the template box), which is also
what the template update and the search's anchor then use; `last_mean` keeps SPEC S6's mean, `last_mode_index` and
`last_mode_mass` report the cluster. With the default `null` none of this exists.
"""
from __future__ import annotations

import os
from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .config import arch_of, estimate_window, load_config
from .particle_filter import ParticleFilter, shard_range
from .vit import ViTEngine
from .weights import make_vit_weights


def weights_digest(weights) -> str:
    """crc32 over every weight tensor's bytes (sorted names, fp32): the configuration fingerprint records it, so a
    checkpoint taken with one weight set is refused by a tracker built with another, whether the weights came from
    the seed or from the `weights=` argument."""
    import zlib
    crc = 0
    for name in sorted(weights):
        t = weights[name].detach().to("cpu", torch.float32).contiguous()
        crc = zlib.crc32(name.encode(), crc)
        crc = zlib.crc32(t.numpy().tobytes(), crc)
    return f"{crc:08x}"


# 3: the fingerprint includes the weights' crc32 (round 4 added it to format 2 without a bump: ADVICE r4)
CHECKPOINT_FORMAT = 3


def _stage_frame(self, frame) -> torch.Tensor:
    """Frame -> the device frame buffer `self._frame_dev` (Tracker and MultiTracker): a device tensor is copied on the
    device; a pinned uint8[H][W][3] tensor (frames.prefetch) is copied asynchronously; anything else goes through a
    pinned staging buffer `self._frame_host` and an asynchronous copy guarded by the event `self._h2d_done`, so the host
    never blocks on the H2D copy of the frame it just submitted. A new frame shape drops the captured graph."""
    if isinstance(frame, torch.Tensor) and frame.is_cuda:
        src = frame.to(torch.uint8)
        if self._frame_dev is None or self._frame_dev.shape != src.shape:
            self._frame_dev = torch.empty_like(src)
            self._graph = None
        self._frame_dev.copy_(src)
        return self._frame_dev
    if (isinstance(frame, torch.Tensor) and frame.dtype == torch.uint8 and frame.dim() == 3
            and frame.shape[2] == 3 and frame.is_contiguous() and frame.is_pinned()):
        # frames.prefetch() output: already staged in pinned memory, copy straight from it
        if self._frame_dev is None or self._frame_dev.shape != frame.shape:
            self._frame_dev = torch.empty(frame.shape, dtype=torch.uint8, device=self.device)
            self._graph = None
        self._frame_dev.copy_(frame, non_blocking=True)
        return self._frame_dev
    arr = np.ascontiguousarray(frame.cpu().numpy() if isinstance(frame, torch.Tensor) else frame, dtype=np.uint8)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("frame must be uint8[H][W][3]")
    if self._frame_dev is None or tuple(self._frame_dev.shape) != arr.shape:
        self._frame_dev = torch.empty(arr.shape, dtype=torch.uint8, device=self.device)
        self._graph = None
    # the pinned staging buffer is sized independently: the device frame may have come from a pinned or
    # device tensor of this shape, which never touches it
    if self._frame_host is None or tuple(self._frame_host.shape) != arr.shape:
        # the previous async copy may still read the old buffer: finish it before dropping it
        if self._frame_host is not None:
            torch.cuda.current_stream(self.device).synchronize()
        self._frame_host = torch.empty(arr.shape, dtype=torch.uint8).pin_memory()
    elif self._h2d_done is not None:
        # reusing the staging buffer: the last frame's H2D copy must have finished reading it
        self._h2d_done.synchronize()
    self._frame_host.numpy()[...] = arr
    self._frame_dev.copy_(self._frame_host, non_blocking=True)
    if self._h2d_done is None:
        self._h2d_done = torch.cuda.Event()
    self._h2d_done.record()
    return self._frame_dev


class _LazyDigest:
    """`weights_digest` of the tracker's weights. Weights built from the seed: computed on first use (a checkpoint save /
    load) from a rebuild (make_vit_weights is deterministic) and cached, since the crc32 converts every weight to a host
    fp32 copy (~1.2 GB for ViT-L/14) that a tracker which never checkpoints should not pay. Weights passed
    in: digested at construction (`_set_weights_digest`) and not referenced afterwards, so the caller can free them and
    a later change to the caller's tensors cannot make the recorded crc describe other weights than the engine's copy
    (ADVICE r5)."""

    def _set_weights_digest(self, weights) -> None:
        self._digest = weights_digest(weights) if weights is not None else None

    @property
    def weights_digest(self) -> str:
        if self._digest is None:
            self._digest = weights_digest(make_vit_weights(self.arch, seed=int(self.cfg["model"]["weights"]["seed"])))
        return self._digest


def _fingerprint(cfg, arch_name: str, digest: str, rank: int, world_size: int) -> dict:
    """Every configuration value a tracking frame's arithmetic depends on: a checkpoint records these and
    a resume under any other value is refused instead of drifting from the original run."""
    m, p, lk = cfg["model"], cfg["particles"], cfg["likelihood"]
    # SPEC S10: recorded only when non-default, so checkpoints of the default configuration keep their fingerprint
    rs = {k: v for k, v in (("resample_method", str(cfg["resample"]["method"])),
                            ("ess_threshold", cfg["resample"]["ess_threshold"]))
          if v not in ("systematic", None)}
    if "ess_threshold" in rs:
        rs["ess_threshold"] = float(rs["ess_threshold"])
    if p["motion_model"] == "constant_velocity":    # SPEC S11: likewise absent under the default random walk
        rs.update(motion_model="constant_velocity", velocity_std=[float(v) for v in p["velocity_std"]],
                  velocity_decay=float(p["velocity_decay"]), velocity_max=float(p["velocity_max"]))
    if p["rotation_std"] is not None:               # SPEC S12: likewise absent without the angle row
        rs.update(rotation_std=float(p["rotation_std"]), rotation_range=[float(v) for v in p["rotation_range"]])
    if lk.get("color") is not None:                 # SPEC S13: likewise absent without the colour cue
        rs.update(color={"bins": int(lk["color"]["bins"]), "grid": int(lk["color"]["grid"]),
                         "lambda": float(lk["color"]["lambda"])})
    if lk.get("color_surround") is not None:        # SPEC S14: likewise absent without the surround ring
        rs.update(color_surround={"lambda": float(lk["color_surround"]["lambda"])})
    if lk.get("tokens") is not None:                # SPEC S18: likewise absent without the patch-token cue
        rs.update(tokens={"lambda": float(lk["tokens"]["lambda"])})
    if lk.get("occlusion") is not None:             # SPEC S15: likewise absent without the occlusion gate
        rs.update(occlusion={"threshold": float(lk["occlusion"]["threshold"]),
                             "noise_gain": float(lk["occlusion"]["noise_gain"]),
                             "max_hold": int(lk["occlusion"]["max_hold"])})
    if lk.get("redetect") is not None:              # SPEC S16: likewise absent without the search
        rs.update(redetect={"after": lk["redetect"]["after"], "threshold": lk["redetect"]["threshold"]})
    if cfg.get("estimate") is not None:             # SPEC S17: likewise absent without the mode estimate
        rs.update(estimate={"method": str(cfg["estimate"]["method"]), "window": float(cfg["estimate"]["window"])})
    return {**rs, "arch": arch_name, "dtype": str(m["dtype"]), "weights_seed": int(m["weights"]["seed"]),
            "weights_crc32": digest,
            "mean": [float(v) for v in m["mean"]], "std": [float(v) for v in m["std"]],
            "P": int(p["num"]), "motion_std": [float(v) for v in p["motion_std"]],
            "scale_range": [float(v) for v in p["scale_range"]], "seed": int(p["seed"]),
            "lambda": float(lk["lambda"]), "weight_bits": int(lk["weight_bits"]),
            "template_update": float(lk["template_update"]), "rank": rank, "world_size": world_size}


def _resample_args(cfg) -> dict:
    """ParticleFilter's SPEC S10 arguments from the config's `resample` section and its SPEC S11 (motion model) and
    S12 (angle row) arguments from `particles`."""
    p = cfg["particles"]
    occ = cfg["likelihood"].get("occlusion")
    gate = {} if occ is None else {"occlusion_threshold": occ["threshold"], "occlusion_max_hold": occ["max_hold"]}
    if cfg["likelihood"].get("redetect") is not None:       # SPEC S16
        gate["redetect"] = cfg["likelihood"]["redetect"]
    return {"resample_method": cfg["resample"]["method"], "ess_threshold": cfg["resample"]["ess_threshold"],
            "motion_model": p["motion_model"], "velocity_std": p["velocity_std"],
            "velocity_decay": p["velocity_decay"], "velocity_max": p["velocity_max"],
            "rotation_std": p["rotation_std"], "rotation_range": p["rotation_range"], **gate}


def _hold_gain(occlusion, pf) -> float:
    """SPEC S15: the position-noise gain of the next predict: g when the filter's last frame was held, else 1."""
    return occlusion["noise_gain"] if occlusion is not None and pf.held_frames > 0 else 1.0


def _search_frame(redetect, pf) -> bool:
    """SPEC S16: whether the next predict is the search: the streak of held frames the host already read has reached
    A (`after`, or max_hold + 1). No device read-back."""
    return redetect is not None and pf.held_frames >= pf.search_after


def _init_angle(cfg, angle) -> Optional[float]:
    """SPEC S12: the initial angle of a target as fp32-exact float, checked against particles.rotation_range; None
    without the angle row (an angle other than 0 is then an error: the tracker has nowhere to keep it)."""
    from .config import check_rotation
    p = cfg["particles"]
    if p["rotation_std"] is None:
        if float(angle) != 0.0:
            raise ValueError("an initial angle needs particles.rotation_std (SPEC S12)")
        return None
    check_rotation(p["rotation_std"], p["rotation_range"], [angle])
    return float(np.float32(angle))


def _full_state(cfg, cx: float, cy: float, angle: Optional[float]):
    """ParticleFilter's initial state in row order: (x, y, 1), zero velocities under constant_velocity, the angle."""
    cv = (0.0, 0.0) if cfg["particles"]["motion_model"] == "constant_velocity" else ()
    return (cx, cy, 1.0) + cv + (() if angle is None else (angle,))


def _angle_row(angle: Optional[float], device) -> Optional[torch.Tensor]:
    """One crop's angle row f32[1] for the engine (None: the unrotated crop)."""
    return None if angle is None else torch.tensor([angle], dtype=torch.float32, device=device)


def _check_fingerprint(sd: dict, mine: dict) -> None:
    import json
    fmt = int(sd["format"])
    if fmt == 1:
        raise ValueError("checkpoint format 1 (rounds 1-2) records only P, rank, world size, seed and arch; format "
                         f"{CHECKPOINT_FORMAT} also checks every value the tracking arithmetic depends on (dtype, lambda, "
                         "motion, weights, ...): re-create the checkpoint with this version")
    if fmt not in (2, CHECKPOINT_FORMAT):
        raise ValueError(f"unknown checkpoint format {fmt}")
    saved = json.loads(str(sd["config"]))
    # format 2 is format 3 without the bump (round 4 added the crc to format 2's fingerprint): such a file carries the
    # crc and is checked like format 3; a format-2 file written before that lacks it and is refused
    if fmt == 2 and "weights_crc32" not in saved:
        raise ValueError("this format-2 checkpoint predates the weights' crc32 in the fingerprint, which format "
                         f"{CHECKPOINT_FORMAT} checks so that a resume with other weights is refused: re-create the "
                         "checkpoint with this version")
    diff = sorted(k for k in set(saved) | set(mine) if saved.get(k) != mine.get(k))
    if diff:
        raise ValueError("checkpoint was written by a tracker with another configuration or rank layout: "
                         + ", ".join(f"{k} {saved.get(k)!r} != {mine.get(k)!r}" for k in diff))


def _sd_particles_soa(sd: dict) -> np.ndarray:
    """A checkpoint's particle states in the SoA layout (float32[3][P_l], [K][3][P_l] for a MultiTracker). Since round 6
    the key is `particles_soa`: `ParticleFilter.particles` became the [P_l][3] view in round 5, and one name for two
    shapes invited misreads. Files of earlier rounds store the same SoA array under `particles`."""
    a = sd["particles_soa"] if "particles_soa" in sd else sd["particles"]
    return np.ascontiguousarray(a, dtype=np.float32)


def _checkpoint_file(path: str, rank: int, world_size: int) -> str:
    """`<path>.rank<r>of<G>.npz` with several ranks, `<path>.npz` with one; a path that already names this rank's
    file (what save_checkpoint returned) is taken as is, so save -> load round-trips either way."""
    suffix = f".rank{rank}of{world_size}.npz" if world_size > 1 else ".npz"
    return path if path.endswith(suffix) else path + suffix


def _blend_template(t: torch.Tensor, f: torch.Tensor, alpha: float) -> None:
    """SPEC S9 in place on the device: t <- g / |g|, g = (1 - alpha) t + alpha f / |f| (fp32)."""
    g = (1.0 - alpha) * t + alpha * (f / f.norm())
    t.copy_(g / g.norm())


def _blend_token_template(t: torch.Tensor, u: torch.Tensor, alpha: float) -> None:
    """SPEC S18 in place on the device, per row: t_j <- g_j / |g_j|, g_j = (1 - alpha) t_j + alpha u_j (fp32), u_j the
    unit token rows of the update's crop; a row whose g_j is zero stays zero."""
    g = (1.0 - alpha) * t + alpha * u
    nrm = g.norm(dim=1, keepdim=True)
    t.copy_(g / torch.where(nrm > 0, nrm, torch.ones_like(nrm)))


def _blend_color_template(t: torch.Tensor, p: torch.Tensor, alpha: float) -> None:
    """SPEC S13 in place on the device: t_b <- fp32(fp32(1 - alpha) t_b) + fp32(fp32(alpha) p_b), three separately
    rounded fp32 operations (three elementwise launches, nothing fused), no renormalisation."""
    om, al = float(np.float32(1.0 - alpha)), float(np.float32(alpha))
    a = t * om
    b = p * al
    torch.add(a, b, out=t)


def _dist_info(rank, world_size, group):
    if rank is not None and world_size is not None:
        return int(rank), int(world_size), group
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group), group
    return 0, 1, None


class _Target(NamedTuple):
    """One target's checkpointed state: its filter, CLS template, template box, histogram template (or None) and
    token template (or None)."""
    pf: ParticleFilter
    template: torch.Tensor
    box_wh: Tuple[float, float]
    color_template: Optional[torch.Tensor]
    token_template: Optional[torch.Tensor] = None


def _restore_streak(pf: ParticleFilter, v) -> None:
    pf.held_frames = int(v)


def _restore_anchor(pf: ParticleFilter, v) -> None:
    pf.anchor = tuple(float(x) for x in v)


# The checkpoint entries that exist only with their feature: (key, dtype, present(tracker, filter 0), value(target),
# restore(filter, value) or None for a device tensor, which is copied in place). Every entry is per target: the
# value's own shape for a Tracker, a leading [K] for a MultiTracker. getattr: a tracker-like object without a feature's
# attribute has that feature off.
_OPTIONAL_ENTRIES = (
    # SPEC S10: the weights carried over skipped resamples, [P_l]
    ("carry", np.int64, lambda tr, pf: pf.ess_threshold is not None, lambda t: t.pf.carry, None),
    # SPEC S11: the velocity rows, [2][P_l]
    ("velocity_soa", np.float32, lambda tr, pf: pf.velocity_soa is not None, lambda t: t.pf.velocity_soa, None),
    # SPEC S12: the angle row, [1][P_l]
    ("rotation_soa", np.float32, lambda tr, pf: pf.rotation_soa is not None, lambda t: t.pf.rotation_soa, None),
    # SPEC S13: the histogram template, [bins^3]
    ("color_template", np.float32, lambda tr, pf: getattr(tr, "color", None) is not None,
     lambda t: t.color_template, None),
    # SPEC S18: the token template, [N-1][D]
    ("token_template", np.float32, lambda tr, pf: getattr(tr, "tokens", None) is not None,
     lambda t: t.token_template, None),
    # SPEC S15: the streak (and with it the next predict's gain), a scalar
    ("held_frames", np.int64, lambda tr, pf: getattr(tr, "occlusion", None) is not None,
     lambda t: t.pf.held_frames, _restore_streak),
    # SPEC S16: what a held search frame returns, [3]
    ("anchor", np.float64, lambda tr, pf: getattr(tr, "redetect", None) is not None,
     lambda t: t.pf.anchor, _restore_anchor),
)
_PER_TARGET = ("pf_frame", "particles_soa", "particles", "template", "box_wh") + tuple(e[0] for e in _OPTIONAL_ENTRIES)


def _state_dict(tr, targets: Sequence[_Target], multi: bool) -> dict:
    """The state between frames of a tracker's targets as numpy arrays: each target's shard of the particles as
    `particles_soa` (float32[3][P_l], the SoA storage; `ParticleFilter.particles` is its [P_l][3] view) after the last
    resample (so Q is zero), its filter's frame counter, template and template box, then the frame size, the frame index
    and the configuration fingerprint (JSON), plus `_OPTIONAL_ENTRIES`. The motion noise and the resample word are
    counter-based (seed, frame index, global particle index: SPEC S1/S2), so a tracker with the same configuration
    that loads this continues bit for bit. `multi`: the MultiTracker form, with `n_objects` and a leading [K] on every
    per-target entry; otherwise the one target's entries as they are."""
    import json

    def per_target(value, dtype):
        vals = [value(t) for t in targets]
        return np.stack([np.asarray(v.cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype) for v in vals])
    pf0 = targets[0].pf
    sd = {"format": np.int64(CHECKPOINT_FORMAT), **({"n_objects": np.int64(len(targets))} if multi else {}),
          "frame_index": np.int64(tr.frame_index), "pf_frame": per_target(lambda t: t.pf.frame, np.int64),
          "particles_soa": per_target(lambda t: t.pf.particles_soa, np.float32),
          "template": per_target(lambda t: t.template, np.float32),
          "box_wh": per_target(lambda t: t.box_wh, np.float64),
          "frame_hw": np.array([pf0.height, pf0.width], np.int64),
          "config": np.array(json.dumps(tr.config_fingerprint(), sort_keys=True))}
    for key, dtype, present, value, _ in _OPTIONAL_ENTRIES:
        if present(tr, pf0):
            sd[key] = per_target(value, dtype)
    return sd if multi else {k: v[0] if k in _PER_TARGET else v for k, v in sd.items()}


class _TargetLoop(_LazyDigest):
    """The frame loop over K targets (SPEC S9), which `MultiTracker` exposes with list-valued
    results and `Tracker` as its K = 1 case with scalar ones: one ParticleFilter per target, and ONE batched ViT
    forward over every target's particles per frame (crops with each target's own template box, one patch GEMM /
    encoder / final LN over all K*P crops, cosine weights against each target's own template), captured into one HIP
    graph. Target k's particle stream is seeded with particles.seed + k. With likelihood.template_update = alpha > 0
    every target's template is updated from its own estimate after each frame (one batched feature pass over the K
    estimate crops). Several ranks: every target's particles are sharded by index range over the ranks, each rank runs
    the ViT over its K x P/G crops, and each target's filter does its own chunk all-gather + global estimate /
    resample, so every rank returns the same K estimates, bit-identical to one rank."""

    _init_args = "frame, bboxes"

    def __init__(self, cfg, n_objects: int, device, rank, world_size, group, use_graph: bool, weights):
        self.cfg = load_config(cfg)
        if not torch.cuda.is_available():
            raise _lib.VPFError(f"{type(self).__name__} runs on the HIP device only; the CPU restatement is oracle/ "
                                "(tests)")
        if n_objects < 1:
            raise ValueError("n_objects >= 1")
        self.rank, self.world_size, self.group = _dist_info(rank, world_size, group)
        if device is None:
            local = int(os.environ.get("LOCAL_RANK", self.rank % max(1, torch.cuda.device_count())))
            device = torch.device("cuda", local)
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        c = self.cfg
        self.arch = arch_of(c)
        self.K = int(n_objects)
        self.P = int(c["particles"]["num"])
        _, self.n_local = shard_range(self.P, self.world_size, self.rank)   # rank r: [floor(rP/G), floor((r+1)P/G))
        w = weights if weights is not None else make_vit_weights(self.arch, seed=int(c["model"]["weights"]["seed"]))
        self._set_weights_digest(weights)
        self.engine = ViTEngine(self.arch, w, c["model"]["dtype"], self.device, max(1, self.K * self.n_local),
                                c["model"]["mean"], c["model"]["std"])
        self.lam = float(c["likelihood"]["lambda"])
        self.bits = int(c["likelihood"]["weight_bits"])
        self.template_alpha = float(c["likelihood"]["template_update"])
        self.color = c["likelihood"]["color"]       # SPEC S13: None, or {bins, grid, lambda} of the colour cue
        self.color_surround = c["likelihood"]["color_surround"]    # SPEC S14: None, or {lambda} of the surround ring
        self.tokens = c["likelihood"]["tokens"]     # SPEC S18: None, or {lambda} of the patch-token cue
        self.occlusion = c["likelihood"]["occlusion"]   # SPEC S15: None, or {threshold, noise_gain, max_hold}
        self.redetect = c["likelihood"]["redetect"]     # SPEC S16: None, or {after, threshold}
        self.estimate = c["estimate"]                   # SPEC S17: None, or {method: mode, window}
        self.use_graph = bool(use_graph)
        self.pfs: List[ParticleFilter] = []
        self.templates: List[torch.Tensor] = []
        self.boxes: List[Tuple[float, float]] = []
        self.color_templates: List[torch.Tensor] = []          # target k's histogram template, f32[bins^3] (SPEC S13)
        self._token_templates: List[torch.Tensor] = []         # target k's token template, f32[N-1][D] (SPEC S18)
        self._frame_dev: Optional[torch.Tensor] = None
        self._frame_host: Optional[torch.Tensor] = None
        self._h2d_done: Optional[torch.cuda.Event] = None
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._weighed = False      # whether a frame has been weighed since init / load: the engine's outputs are a frame's
        self.frame_index = 0

    # ------------------------------------------------------------------ frames
    def _upload(self, frame) -> torch.Tensor:
        return _stage_frame(self, frame)

    def _require_init(self) -> None:
        if not self.pfs:
            raise RuntimeError(f"call init({self._init_args}) first")

    # ------------------------------------------------------------------ H13
    def _place_filters(self, frame_hw, states=None) -> None:
        """Every target's filter on a frame of `frame_hw`, all particles at states[k] (default (0, 0, 1): a checkpoint
        load overwrites them), with the mode window of `self.boxes[k]`. Filters are built once, target k's seeded with
        particles.seed + k, and reused from then on: a second init or a load resets them, which leaves them as a new
        filter would be."""
        c, p = self.cfg, self.cfg["particles"]
        if not self.pfs:
            self.pfs = [ParticleFilter(self.P, (0.0, 0.0, 1.0), p["motion_std"], p["scale_range"], int(p["seed"]) + k,
                                       self.device, frame_hw, self.lam, self.bits, self.rank, self.world_size,
                                       self.group, **_resample_args(c),
                                       mode_window=estimate_window(self.estimate, self.boxes[k]))
                        for k in range(self.K)]
        for k, pf in enumerate(self.pfs):
            pf.height, pf.width = int(frame_hw[0]), int(frame_hw[1])
            pf.set_mode_window(estimate_window(self.estimate, self.boxes[k]))
            pf.reset((0.0, 0.0, 1.0) if states is None else states[k])
        self._graph = None
        self._weighed = False

    def _init(self, frame, bboxes: Sequence, angles: Optional[Sequence[float]] = None) -> None:
        """Every target's template from its box (x, y, w, h) cropped at scale 1, and its particles reset to the box
        centre. `angles` (SPEC S12, with particles.rotation_std): one initial angle per box in radians, default all 0;
        the box is turned by it about its centre, and the template crop and every particle start there."""
        if len(bboxes) != self.K:
            raise ValueError(f"expected {self.K} boxes")
        if angles is not None and len(angles) != self.K:
            raise ValueError(f"expected {self.K} angles")
        c = self.cfg
        angs = [_init_angle(c, a) for a in (angles if angles is not None else [0.0] * self.K)]
        fd = self._upload(frame)
        self.boxes = [(float(bw), float(bh)) for _, _, bw, bh in bboxes]
        self.templates, self.color_templates, self._token_templates, states = [], [], [], []
        for (bx, by, _, _), (bw, bh), ang in zip(bboxes, self.boxes, angs):
            cx, cy = float(bx) + 0.5 * bw, float(by) + 0.5 * bh
            one = torch.tensor([[cx], [cy], [1.0]], dtype=torch.float32, device=self.device)
            if self.tokens is not None:     # SPEC S18: the token rows of the forward pass that gives the CLS template
                f, u = self.engine.features_many(fd, [one], [(bw, bh)], [_angle_row(ang, self.device)],
                                                 want_tokens=True)
                f = f[0].clone()
                self._token_templates.append(u[0].contiguous())
            else:
                f = self.engine.features(fd, one, (bw, bh), _angle_row(ang, self.device))[0].clone()
            self.templates.append((f / f.norm()).contiguous())
            if self.color is not None:      # SPEC S13: the init box's histogram at scale 1, turned by the initial angle
                self.color_templates.append(self.engine.color_histograms(
                    fd, one, (bw, bh), self.color, _angle_row(ang, self.device))[0].contiguous())
            states.append(_full_state(c, cx, cy, ang))
        self._place_filters((fd.shape[0], fd.shape[1]), states)
        self.frame_index = 0

    # ------------------------------------------------------------------ H14
    def _forward(self) -> None:
        eng = self.engine
        n = eng.embed_many(self._frame_dev, [pf.particles_soa for pf in self.pfs], self.boxes,
                           [pf.rotation_soa for pf in self.pfs])
        eng.encoder(n)
        for k, pf in enumerate(self.pfs):
            eng.weights_from_tokens(self.n_local, self.templates[k], self.lam, self.bits, row0=k * self.n_local)
            if self.tokens is not None:     # SPEC S18: directly after cls_weight, which pins the order of the floors
                eng.token_weights(self.n_local, self._token_templates[k], self.tokens["lambda"], self.bits,
                                  row0=k * self.n_local)
            if self.color is not None:      # SPEC S13: one call per target, its own box and histogram template
                eng.color_weights(self.n_local, pf.particles_soa, self.boxes[k], self.color, self.color_templates[k],
                                  self.bits, pf.rotation_soa, row0=k * self.n_local, surround=self.color_surround)

    def _capture(self) -> None:
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._forward()   # warm-up outside capture
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        # thread_local: RCCL's watchdog thread queries events while a capture runs (multi-GPU); "global" would
        # invalidate the capture on that, the capture itself only involves this thread's stream
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._forward()
        self._graph = g

    def weigh(self) -> None:
        """Crop + ViT + weights of every target's predicted particles on the uploaded frame (graph replay when
        enabled); each filter's Q is set."""
        if self.use_graph:
            if self._graph is None:
                self._capture()
            self._graph.replay()
        else:
            self._forward()
        for k, pf in enumerate(self.pfs):
            pf.set_weights(self.engine.Q[k * self.n_local:(k + 1) * self.n_local])
        self._weighed = True

    def _step(self) -> List[Tuple[float, float, float]]:
        """Every target's estimate + resample on the device, all enqueued before the host reads any estimate (one
        wait), then the template updates, which crop at the estimates on this frame and do not read the particles."""
        for pf in self.pfs:
            pf._settle()
            pf._commit()
        ests = [pf._read_estimate() for pf in self.pfs]
        if self.template_alpha > 0.0:
            self._update_templates(ests)
        return ests

    def _track(self, frame) -> List[Tuple[float, float, float]]:
        self._require_init()
        fd = self._upload(frame)
        self.frame_index += 1
        for pf in self.pfs:
            # a frame of another size: predict clamps to the new bounds (the graph was dropped by _upload)
            pf.height, pf.width = int(fd.shape[0]), int(fd.shape[1])
            pf.predict(self.frame_index, _hold_gain(self.occlusion, pf), _search_frame(self.redetect, pf))
        self.weigh()
        return self._step()

    def _blend_templates(self, targets: Sequence[int], states, alpha: Optional[float], angles: Sequence) -> None:
        """SPEC S9 for the chosen targets: t_k <- normalise((1 - alpha) t_k + alpha f_k / |f_k|), f_k the CLS feature
        of the crop at states[k] = (x, y, scale) of the current frame with target k's box, turned with the angle row
        (SPEC S12) by angles[k] (None: the frame's angle estimate); with the colour cue (SPEC S13) the crop's histogram
        is blended into the histogram template without renormalisation; with the token cue (SPEC S18) the crop's unit
        token rows, taken from the same forward pass, are blended into the token template row by row. One batched
        feature pass over all K crops (a crop's features do not depend on the batch); nothing is launched for no
        target. In place, so the captured graph keeps reading the same buffers; every rank computes the same bits (same
        estimates, same kernels)."""
        if not targets:
            return
        a = self.template_alpha if alpha is None else float(alpha)
        sets = [torch.tensor([[st[0]], [st[1]], [st[2]]], dtype=torch.float32, device=self.device) for st in states]
        angs = [_angle_row(None if pf.rotation_soa is None else pf.last_rotation if ang is None else ang, self.device)
                for pf, ang in zip(self.pfs, angles)]
        if self.tokens is not None:
            f, u = self.engine.features_many(self._frame_dev, sets, self.boxes, angs, want_tokens=True)
        else:
            f = self.engine.features_many(self._frame_dev, sets, self.boxes, angs)
        for k in targets:
            _blend_template(self.templates[k], f[k], a)
            if self.tokens is not None:
                _blend_token_template(self._token_templates[k], u[k], a)
            if self.color is not None:
                p = self.engine.color_histograms(self._frame_dev, sets[k], self.boxes[k], self.color, angs[k])[0]
                _blend_color_template(self.color_templates[k], p, a)

    def _update_templates(self, states, alpha: Optional[float] = None) -> None:
        """The template update of every target from states[k] (`_blend_templates`), except that a target whose last
        frame was held (SPEC S15) keeps both its templates' bits."""
        self._blend_templates([k for k, pf in enumerate(self.pfs) if not pf.last_held], states, alpha, [None] * self.K)

    # ------------------------------------------------------------------ checkpoint / resume
    def _load(self, sd: dict) -> None:
        """A MultiTracker-form state dict (`_state_dict`) into this tracker. The templates are written in place once
        they exist: a captured graph reads these buffers."""
        _check_fingerprint(sd, self.config_fingerprint())
        self.boxes = [tuple(float(v) for v in b) for b in sd["box_wh"]]
        if not self.templates:
            self.templates = [torch.empty(self.arch.dim, dtype=torch.float32, device=self.device)
                              for _ in range(self.K)]
            if self.color is not None:
                self.color_templates = [torch.empty(int(self.color["bins"]) ** 3, dtype=torch.float32,
                                                    device=self.device) for _ in range(self.K)]
            if self.tokens is not None:
                self._token_templates = [torch.empty(self.arch.tokens - 1, self.arch.dim, dtype=torch.float32,
                                                     device=self.device) for _ in range(self.K)]
        self._place_filters(tuple(int(v) for v in sd["frame_hw"]))
        soa = _sd_particles_soa(sd)
        for k, t in enumerate(self._targets()):
            t.pf.particles_soa.copy_(torch.from_numpy(np.ascontiguousarray(soa[k])))
            t.pf.frame = int(sd["pf_frame"][k])
            t.template.copy_(torch.from_numpy(np.ascontiguousarray(sd["template"][k], dtype=np.float32)))
            for key, dtype, present, value, restore in _OPTIONAL_ENTRIES:
                if present(self, t.pf):
                    v = np.asarray(sd[key][k], dtype=dtype)
                    if restore is None:
                        value(t).copy_(torch.from_numpy(np.ascontiguousarray(v)))
                    else:
                        restore(t.pf, v)
        self.frame_index = int(sd["frame_index"])

    def _targets(self) -> List[_Target]:
        return [_Target(pf, self.templates[k], self.boxes[k], self.color_templates[k] if self.color_templates else None,
                        self._token_templates[k] if self._token_templates else None)
                for k, pf in enumerate(self.pfs)]

    def _checkpoint_file(self, path: str) -> str:
        return _checkpoint_file(path, self.rank, self.world_size)

    def save_checkpoint(self, path: str) -> str:
        """np.savez of state_dict() (no pickled objects); with several ranks each writes `<path>.rank<r>of<G>.npz`.
        Returns the file written (load_checkpoint accepts it, or the base path)."""
        path = self._checkpoint_file(path)
        np.savez(path, **self.state_dict())
        return path

    def load_checkpoint(self, path: str) -> None:
        path = self._checkpoint_file(path)
        with np.load(path, allow_pickle=False) as z:
            self.load_state_dict({k: z[k] for k in z.files})


class MultiTracker(_TargetLoop):
    """Several targets in one frame loop (`_TargetLoop`): every result is a list with one entry per target. With one
    target it reproduces Tracker bit for bit."""

    def __init__(self, cfg=None, n_objects: int = 1, device=None, use_graph: bool = True, weights=None,
                 rank: Optional[int] = None, world_size: Optional[int] = None, group=None):
        super().__init__(cfg, n_objects, device, rank, world_size, group, use_graph, weights)

    init, track, step, update_templates = (_TargetLoop._init, _TargetLoop._track, _TargetLoop._step,
                                           _TargetLoop._update_templates)

    @property
    def color_template(self) -> Optional[List[torch.Tensor]]:
        """SPEC S13: every target's histogram template (f32[bins^3] each; `color_templates`), None without
        likelihood.color; the single tracker's attribute of the same name holds one tensor."""
        return None if self.color is None else self.color_templates

    @property
    def token_templates(self) -> Optional[List[torch.Tensor]]:
        """SPEC S18: every target's token template (f32[N-1][D] each), None without likelihood.tokens; the single
        tracker's `token_template` holds one tensor."""
        return None if self.tokens is None else self._token_templates

    def config_fingerprint(self) -> dict:
        """Tracker's fingerprint and the target count."""
        return {**_fingerprint(self.cfg, self.arch.name, self.weights_digest, self.rank, self.world_size),
                "n_objects": self.K}

    def state_dict(self) -> dict:
        """`_state_dict` of every target: particles_soa [K][3][P_l], templates [K][D], template boxes [K][2], ..."""
        self._require_init()
        return _state_dict(self, self._targets(), multi=True)

    def load_state_dict(self, sd: dict) -> None:
        if "n_objects" not in sd:
            raise ValueError("this checkpoint was written by a single-target Tracker")
        self._load(sd)


def _first(name: str, doc: str) -> property:
    """A Tracker's view of its one target: element 0 of the K-target list `name`, None before there is one."""
    return property(lambda self: (getattr(self, name) or (None,))[0], doc=doc)


class Tracker(_TargetLoop):
    """One target: `_TargetLoop` with K = 1 and scalar results (`pf`, `template`, `box_wh`, `color_template` and the
    frame outputs are its one target's; all None before `init`)."""

    _init_args = "frame, bbox"

    def __init__(self, cfg=None, device=None, rank: Optional[int] = None, world_size: Optional[int] = None,
                 group=None, use_graph: bool = True, weights=None):
        super().__init__(cfg, 1, device, rank, world_size, group, use_graph, weights)

    pf = _first("pfs", "The target's ParticleFilter.")
    template = _first("templates", "The unit CLS template, f32[D].")
    box_wh = _first("boxes", "The template box (w, h): a particle of scale s stands for an s w x s h box (SPEC S3).")
    color_template = _first("color_templates", "SPEC S13: the histogram template, f32[bins^3]; None without the cue.")

    token_template = _first("_token_templates", "SPEC S18: the token template, f32[N-1][D]; None without the cue.")

    def init(self, frame, bbox, angle: float = 0.0) -> None:
        """Template from the bbox (x, y, w, h) crop at scale 1; particles reset to the bbox centre. With
        particles.rotation_std (SPEC S12) the box is turned by `angle` radians about its centre: the template crop and
        every particle start there."""
        self._init(frame, [bbox], [angle])

    def track(self, frame) -> Tuple[float, float, float]:
        return self._track(frame)[0]

    def update_template(self, state, alpha: Optional[float] = None, angle: Optional[float] = None) -> None:
        """`_blend_templates` of the target from `state`, turned by `angle` (default: the frame's angle estimate;
        ignored without the angle row). Unlike the update inside `track`, this blends after a held frame too."""
        self._blend_templates([0], [state], alpha, [angle])

    def config_fingerprint(self) -> dict:
        """Every configuration value a tracking frame's arithmetic depends on: a checkpoint records
        these and a resume under any other value is refused instead of drifting from the original run."""
        return _fingerprint(self.cfg, self.arch.name, self.weights_digest, self.rank, self.world_size)

    def state_dict(self) -> dict:
        """`_state_dict` of the one target, its entries without a leading axis and no `n_objects`."""
        if self.pf is None:
            raise RuntimeError("call init(frame, bbox) first")
        target = _Target(self.pf, self.template, self.box_wh, getattr(self, "color_template", None),
                         getattr(self, "token_template", None))
        return _state_dict(self, [target], multi=False)

    def load_state_dict(self, sd: dict) -> None:
        if "n_objects" in sd:
            raise ValueError("this checkpoint was written by a MultiTracker")
        self._load({k: np.asarray(v)[None] if k in _PER_TARGET else v for k, v in sd.items()})

    def box(self, state) -> Tuple[float, float, float, float]:
        """(x, y, w, h) of the box a state (centre x, y, scale) stands for (SPEC S3: scale x template size)."""
        x, y, s = (float(v) for v in state)
        w, h = s * self.box_wh[0], s * self.box_wh[1]
        return x - 0.5 * w, y - 0.5 * h, w, h

    def run(self, frames: Iterable) -> np.ndarray:
        return np.array([self.track(f) for f in frames], dtype=np.float64)


# The frame outputs, forwarded from each target's ParticleFilter after `track`: a list with one entry per target on a
# MultiTracker, the target's own value on a Tracker (None before `init`).
_FRAME_OUTPUTS = {
    "last_held": "Whether the last tracked frame was held (SPEC S15; None unless likelihood.occlusion is set).",
    "last_peak": "max_i L_i / 2^K of the last tracked frame, the gate's statistic (SPEC S15; None without the gate).",
    "last_evidence": "The last tracked frame's mean likelihood T / (P 2^K) (SPEC S15; None without the gate).",
    "lost": "held_frames > likelihood.occlusion.max_hold: a flag, the tracker goes on holding (SPEC S15; None without "
            "the gate).",
    "last_searched": "Whether the last tracked frame's predict was the search (SPEC S16; None unless "
                     "likelihood.redetect is set).",
    "last_reacquired": "Whether the last tracked frame was searched and not held: the target was found again (SPEC "
                       "S16; None without the search).",
    "last_mean": "SPEC S6's weighted mean (x, y, scale) of the last tracked frame, which `track()` no longer returns "
                 "under the mode estimate (SPEC S17; None unless estimate.method is mode).",
    "last_mode_index": "The global index of the particle whose window holds the most weight (SPEC S17; None without "
                       "the mode estimate).",
    "last_mode_mass": "The share of the posterior inside the reported window, Tm / T (SPEC S17; None without the mode "
                      "estimate).",
    "last_ess": "N_eff of the last tracked frame's posterior weights (SPEC S10; None unless adaptive resampling is on).",
    "last_resampled": "Whether the last tracked frame resampled (always, unless resample.ess_threshold gates it: SPEC "
                      "S10).",
    "last_velocity": "The velocity estimate (vx, vy) in px/frame of the last tracked frame (SPEC S11; None unless "
                     "particles.motion_model is constant_velocity).",
    "last_rotation": "The angle estimate in radians of the last tracked frame (SPEC S12; None unless "
                     "particles.rotation_std is set).",
}


def _frame_output(name: str, doc: str, per_target=None) -> None:
    """The frame output `name` as a property of both classes; `per_target(tracker)` (default: the filters' attribute
    of that name) produces the per-target list, and a Tracker takes its element 0."""
    if per_target is None:
        def per_target(self):
            return [getattr(pf, name) for pf in self.pfs]
    setattr(MultiTracker, name, property(per_target, doc="Per target: " + doc))
    setattr(Tracker, name, property(lambda self: (per_target(self) or [None])[0], doc=doc))


for _name, _doc in _FRAME_OUTPUTS.items():
    _frame_output(_name, _doc)
# a filter counts its streak from 0 with or without the gate; a tracker reports it only with the gate
_frame_output("held_frames", "Consecutive held frames up to the last tracked one (SPEC S15; None without the gate).",
              lambda self: [pf.held_frames if self.occlusion is not None else None for pf in self.pfs])
# the engine's buffer of the last weighed frame: target k's slice, this rank's shard; the next frame overwrites it, a
# template update's forward does not touch it, and before the first frame after init or a checkpoint load it holds nothing
_frame_output("last_token_sim", "The last tracked frame's mean patch-token cosine sim_p of every local particle, a "
              "device tensor f32[P_l] that the next frame overwrites (SPEC S18; None unless likelihood.tokens is set, and "
              "until a frame has been tracked since init or a checkpoint load).",
              lambda self: [self.engine.tok_sim[k * self.n_local:(k + 1) * self.n_local]
                            if self.tokens is not None and self._weighed else None for k in range(len(self.pfs))])
