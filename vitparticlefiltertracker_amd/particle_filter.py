"""`ParticleFilter` — the reference's "Particle Filter ... probabilistic algorithms for accurate state
estimation" (/root/reference/README.md:8), SPEC.md S2/S5-S7, on the HIP path.

Particles are sharded by index across ranks (rank r owns [floor(r*P/G), floor((r+1)*P/G)); shards
differ by at most one particle when G does not divide P); one process per GPU.
Per frame the only cross-device traffic is ONE fixed-size all-gather of the shard chunks (weight Q_i int64 +
state x, y, s fp32 = 20 B per particle; 80 KB at 4096 particles, 1.3 MB at configs[4]'s 65536; every chunk is sized
for the largest shard; the constant-velocity model of SPEC S11 adds vx, vy: 28 B; SPEC S12's angle row adds 4 B to
either). Every rank then holds the global
weights and states, and one device call (vpf_estimate_resample) computes on each rank:

  * the weight-normalisation sum T and the estimate sums (SPEC S6), in one fixed-order tree over the GLOBAL
    index, so every rank and every world size gets the same bits;
  * the inclusive CDF and, from the resample word drawn on the device, the exact systematic-resample ancestors
    of the slots this rank owns (SPEC S7): identical to the single-process oracle for any G.

No host planning sits between the weights and the resample; the host reads only the 32-B statistics (the
estimate it returns). The collective runs on torch.distributed (backend "nccl" = RCCL over xGMI on the GPU box;
"gloo" in CPU tests of the layout and when several ranks share one GPU). With G = 1 there is no collective.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import ops  # noqa: F401

vpf = torch.ops.vpf

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr: Sequence[int], key: Sequence[int]) -> List[int]:
    """Host Philox4x32-10 (SPEC S1) for the per-frame resample offset word."""
    c0, c1, c2, c3 = (int(v) & _MASK for v in ctr)
    k0, k1 = (int(v) & _MASK for v in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> 32) ^ c3 ^ k1) & _MASK, p0 & _MASK
    return [c0, c1, c2, c3]


def resample_word(seed: int, frame: int) -> int:
    seed &= (1 << 64) - 1
    return philox4x32_10((0, frame, 1, 0), (seed & _MASK, seed >> 32))[0]


def position(j: int, T: int, P: int, U: int) -> int:
    """SPEC S7: pos_j = floor((j*T + floor(U*T/2^32)) / P) (Python ints: exact)."""
    u = (U * T) >> 32
    return (j * T + u) // P


def slot_range(offset: int, shard_T: int, T: int, P: int, U: int) -> Tuple[int, int]:
    """Slots j whose position falls in [offset, offset + shard_T): a contiguous range (pos is monotone)."""
    def first_at_least(v: int) -> int:
        lo, hi = 0, P
        while lo < hi:
            mid = (lo + hi) // 2
            if position(mid, T, P, U) >= v:
                hi = mid
            else:
                lo = mid + 1
        return lo
    return first_at_least(offset), first_at_least(offset + shard_T)


def shard_range(P: int, world: int, rank: int) -> Tuple[int, int]:
    """(begin, n) of rank `rank`'s particles: [floor(rank P / world), floor((rank + 1) P / world)).
    Equal shards when world divides P; otherwise the sizes differ by one. Needs 1 <= world <= P."""
    if not 1 <= world <= P or not 0 <= rank < world:
        raise ValueError(f"need 1 <= world_size <= particles and 0 <= rank < world_size (P={P}, world={world}, "
                         f"rank={rank})")
    b, e = rank * P // world, (rank + 1) * P // world
    return b, e - b


def plan_resample(stats, P: int, n_local, U: int):
    """Host plan of the exact systematic resample (SPEC S7) for the per-shard entry point vpf_resample, from the
    shards' (T_r, ...) statistics: (uniform, T, offsets, slot ranges per rank). `n_local`: the shard size (equal
    shards) or the list of shard sizes. ParticleFilter itself runs the device-resident vpf_estimate_resample and
    needs no plan."""
    world = len(stats)
    T_r = [s[0] for s in stats]
    uniform = sum(T_r) == 0
    if uniform:
        T_r = list(n_local) if isinstance(n_local, (list, tuple)) else [n_local] * world
    T = sum(T_r)
    offsets = [sum(T_r[:r]) for r in range(world)]
    ranges = [slot_range(offsets[r], T_r[r], T, P, U) for r in range(world)]
    return uniform, T, offsets, ranges


def _all_gather_into(out: torch.Tensor, inp: torch.Tensor, group=None) -> None:
    """all_gather_into_tensor on the group's backend. RCCL ("nccl") takes the device tensors directly, on the
    current stream. gloo (CPU tests; several ranks sharing one GPU) exchanges host copies."""
    import torch.distributed as dist
    if inp.is_cuda and dist.get_backend(group) == "gloo":
        host = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(host, inp.cpu(), group=group)
        out.copy_(host)
    else:
        dist.all_gather_into_tensor(out, inp, group=group)


def chunk_words(n: int, rows: int = 3) -> int:
    """int32 words of one shard chunk: Q int64[n] | `rows` fp32[n] state rows (x | y | s; SPEC S11's five rows add
    vx | vy), padded to a multiple of 8 bytes."""
    return (2 + rows) * n + ((rows * n) & 1)


def shard_views(chunk: torch.Tensor, n: int, rows: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Q int64[n], particles f32[rows][n]) as views into one shard chunk (int32[chunk_words(n, rows)]): the filter's
    state lives in the chunk, so the all-gather sends it as is (no packing)."""
    return chunk[: 2 * n].view(torch.int64), chunk[2 * n: (2 + rows) * n].view(torch.float32).view(rows, n)


def global_view(allc: torch.Tensor, world: int, n: int, rows: int = 3):
    """Kernel arguments of vpf_estimate_resample for `world` gathered chunks of n particles each (allc:
    int32[world * chunk_words(n, rows)]): (Q view, q_stride, particle view, ld, p_stride, n_shard). Rows past the
    third (SPEC S11's velocity) start at particle view + 3 * ld, with the same ld and p_stride."""
    cw = chunk_words(n, rows)
    return allc.view(torch.int64), cw // 2, allc[2 * n:].view(torch.float32), n, cw, n


def compact_index(P: int, world: int, rows: int = 3) -> torch.Tensor:
    """Unequal shards (world does not divide P): int32-word indices into the gathered chunks (world slots of
    chunk_words(ceil(P / world), rows) words; rank r's slot holds its shard_views layout for its own n_r) that read
    out the global arrays in particle order: Q int64[P] as 2P words, then the `rows` state rows fp32[P] (x | y | s).
    One index_select of the gathered buffer with it gives the one-shard layout that vpf_estimate_resample reads as
    (Q, P, x|y|s, P, rows * P, P)."""
    cw = chunk_words(-(-P // world), rows)
    q, st = [], [[] for _ in range(rows)]
    for r in range(world):
        _, n = shard_range(P, world, r)
        base = r * cw
        q.append(torch.arange(base, base + 2 * n))
        for c in range(rows):
            st[c].append(torch.arange(base + (2 + c) * n, base + (3 + c) * n))
    return torch.cat(q + [t for row in st for t in row])


def compact_view(glob: torch.Tensor, P: int, rows: int = 3):
    """vpf_estimate_resample's arguments over the compacted global arrays (glob: int32[(2 + rows) P], compact_index
    order)."""
    return glob[: 2 * P].view(torch.int64), P, glob[2 * P:].view(torch.float32), P, rows * P, P


class ParticleFilter:
    """H1, H10-H12. API: predict(), update(features, template), estimate(), resample(),
    attributes `particles` (float32[P_local][3] on the device: one (x, y, scale) row per particle, §8b's shape) and
    `Q` (int64[P_local]). The storage is SoA, `particles_soa` (float32[3][P_local]); `particles` is its transposed view.

    `Q` and `particles_soa` are views into one shard chunk (`shard_views`). Per frame (`step`, or estimate() then
    resample()): world > 1 all-gathers the chunks (20 B per particle, one fixed-size RCCL collective), then ONE
    device call, vpf_estimate_resample, computes the estimate sums, the CDF, the resample word and the ancestors
    of this rank's slots over the global set. The resample is enqueued before the host waits for the 32-B
    statistics, so the only host synchronisation of a frame is that read.

    Adaptive resampling (SPEC S10): `resample_method="stratified"` and / or `ess_threshold=tau` in (0, 1] switch the
    frame to vpf_weight_prior (the carried weights times the frame's likelihood, on the local shard, before the
    all-gather) and vpf_estimate_resample_ex, which decides on the device whether N_eff < tau * P and either resamples
    with the scheme's positions or keeps every particle and carries its weight into the next frame. `carry`
    (int64[P_local]) holds the carried weights, `last_ess` / `last_resampled` the frame's N_eff and decision (read
    with the estimate: 64 B instead of 32 B, same single wait). With the defaults none of this exists (`carry is
    None`) and the frame launches exactly vpf_estimate_resample.

    Constant-velocity motion (SPEC S11): `motion_model="constant_velocity"` gives every particle a velocity. The chunk
    then holds five state rows, x | y | s | vx | vy (28 B per particle with Q, still ONE all-gather): `particles_soa`
    stays the [3][P_local] view of the first three (the crop and the captured ViT graph read it), `velocity_soa` is the
    [2][P_local] view of the last two and `velocity` its [P_local][2] transpose. predict() launches vpf_predict_cv; the
    frame adds vpf_weighted_sums over the velocity rows (the velocity estimate `last_velocity`, read with the state
    estimate in the same single wait) and vpf_gather_rows (the slots take their ancestors' velocities). With the
    default `random_walk` none of this exists (`velocity_soa is None`).

    Rotated boxes (SPEC S12): `rotation_std=sigma_a` (radians per frame) appends one more row, the angle `a`, last:
    x | y | s | [vx | vy] | a (24 B per particle with Q, 32 B with the velocity; still ONE all-gather). `rotation_soa` is
    its [1][P_local] view, `rotation` the [P_local] row. predict() adds vpf_predict_angle after the motion model's kernel
    (angles are clamped to `rotation_range`, not wrapped); the frame's vpf_weighted_sums and vpf_gather_rows run over all
    extra rows in one call each, and `last_rotation` is the angle estimate, read in the same single wait. The crop
    (vpf_crop_patches_rot_*) reads the row. With the default None none of this exists (`rotation_soa is None`).

    Occlusion gate (SPEC S15): `occlusion_threshold=theta` in (0, 1] switches the frame to vpf_estimate_resample_gate
    (and vpf_weighted_sums_gate for the extra rows) on the adaptive path's buffers: when the frame's largest weight is
    below gate_q = floor(theta 2^K) the frame is held, decided on the device: the estimate is the particles' plain
    mean, nothing is resampled and the states stay. `last_held`, `last_peak` (max L_i / 2^K) and `last_evidence` (the
    mean likelihood) are read with the estimate in the same single wait; `held_frames` counts the consecutive held
    frames and `lost` is held_frames > `occlusion_max_hold`. The caller widens the next predict's position noise after
    a hold (`predict(frame, gain)`). Not combined with `ess_threshold`. With the default None none of this exists.

    Re-detection (SPEC S16): `redetect={after, threshold}` (needs the occlusion gate). The caller asks for the search
    predict (`predict(frame, gain, search=True)`) once `held_frames >= search_after`: vpf_predict_search scatters the
    particles over the whole frame on a jittered lattice in the global index (the scale row steps as ever, the
    velocities are zeroed, the angle row's predict follows unchanged), and that frame's gate runs with
    `search_gate_q` = floor(theta_r 2^K). A search frame that is not held is an ordinary frame: the resample collapses
    the lattice onto the target. On a held search frame the plain mean of the scattered cloud is the frame centre, so
    estimate() / step() return the `anchor` instead: the (x, y, s) returned by the last frame that was not a search
    frame. `last_searched` / `last_reacquired` report it. With the default None none of this exists.

    Mode estimate (SPEC S17): `mode_window=(hx, hy)` in pixels (fp32 values, finite and >= 0). After the estimate +
    resample call the frame enqueues vpf_mode_estimate over the same global weights and predicted states (the resample
    writes elsewhere): the all-pairs density D_i of every particle's window, its arg-max i* and the windowed sums over
    every state row, written behind the other statistics, so the pinned copy and the single wait stay one. estimate() /
    step() then return the local weighted mean of the densest cluster, `last_velocity` / `last_rotation` its extra rows;
    SPEC S6's mean is kept as `last_mean`, with `last_mode_index` = i* and `last_mode_mass` = Tm / T, the share of the
    posterior inside the window. The resample does not read the estimate: ancestors and states are a mean filter's. With
    the default None none of this exists."""

    def __init__(self, num_particles: int, init_state=(0.0, 0.0, 1.0), motion_std=(4.0, 4.0, 0.02),
                 scale_range=(0.5, 2.0), seed: int = 1234, device=None, frame_size=(224, 224),
                 lam: float = 20.0, weight_bits: int = 40, rank: int = 0, world_size: int = 1,
                 group: Optional[object] = None, resample_method: str = "systematic",
                 ess_threshold: Optional[float] = None, motion_model: str = "random_walk",
                 velocity_std=(1.0, 1.0), velocity_decay: float = 1.0, velocity_max: float = 64.0,
                 rotation_std: Optional[float] = None, rotation_range=(-math.pi / 2, math.pi / 2),
                 occlusion_threshold: Optional[float] = None, occlusion_max_hold: int = 30,
                 redetect: Optional[dict] = None, mode_window: Optional[Sequence[float]] = None):
        from .config import (RESAMPLE_METHODS, check_ess_threshold, check_motion_model, check_occlusion,
                             check_redetect, check_rotation, occlusion_gate_q, redetect_after)
        self.motion_model, self.velocity_std, self.velocity_decay, self.velocity_max = check_motion_model(
            motion_model, velocity_std, velocity_decay, velocity_max)
        self._cv = self.motion_model == "constant_velocity"
        self.rotation_std, self.rotation_range = check_rotation(rotation_std, rotation_range)
        self._rot = self.rotation_std is not None
        self._extra = (2 if self._cv else 0) + (1 if self._rot else 0)     # state rows past x | y | s
        rows = 3 + self._extra
        if resample_method not in RESAMPLE_METHODS:
            raise ValueError(f"resample_method must be one of {RESAMPLE_METHODS} (SPEC S7, S10)")
        self.resample_method = str(resample_method)
        self.ess_threshold = check_ess_threshold(ess_threshold)
        occ = None if occlusion_threshold is None else check_occlusion(
            {"threshold": occlusion_threshold, "max_hold": occlusion_max_hold}, self.ess_threshold)
        self.occlusion_threshold = None if occ is None else occ["threshold"]
        self.occlusion_max_hold = None if occ is None else occ["max_hold"]
        self._gate = occ is not None
        self.redetect = check_redetect(redetect, occ)           # SPEC S16: None, or {after, threshold}
        self.begin, self.n_local = shard_range(int(num_particles), int(world_size), int(rank))
        if weight_bits + max(1, (num_particles - 1).bit_length()) > 62:
            raise ValueError("weight_bits + ceil(log2 P) must be <= 62 (SPEC S5)")
        if not (math.isfinite(float(lam)) and float(lam) >= 0.0):
            raise ValueError("lam must be finite and >= 0 (SPEC S5)")
        self.P = int(num_particles)
        self.rank, self.world_size, self.group = int(rank), int(world_size), group
        n = self.n_local
        n_max = -(-self.P // self.world_size)     # every rank's chunk has the largest shard's size (fixed-size gather)
        self.motion_std = [float(v) for v in motion_std]
        self.scale_range = [float(v) for v in scale_range]
        self.seed = int(seed)
        self.lam, self.bits = float(lam), int(weight_bits)
        self.height, self.width = int(frame_size[0]), int(frame_size[1])
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._chunk = torch.zeros(chunk_words(n_max, rows), device=self.device, dtype=torch.int32)
        self.Q, self._state = shard_views(self._chunk, n, rows)     # every state row; [:3] is x | y | s
        self.particles_soa = self._state[:3]
        self.velocity_soa: Optional[torch.Tensor] = self._state[3:5] if self._cv else None
        self.rotation_soa: Optional[torch.Tensor] = self._state[rows - 1:] if self._rot else None   # SPEC S12: [1][P_l]
        self._cidx = None
        if self.world_size > 1:
            self._allc = torch.zeros(self.world_size * chunk_words(n_max, rows), device=self.device,
                                     dtype=torch.int32)
            if self.P % self.world_size == 0:
                self._gview = global_view(self._allc, self.world_size, n, rows)
            else:   # unequal shards: the gathered chunks are compacted into the global order first (_settle)
                self._cidx = compact_index(self.P, self.world_size, rows).to(self.device)
                self._glob = torch.empty((2 + rows) * self.P, device=self.device, dtype=torch.int32)
                self._gview = compact_view(self._glob, self.P, rows)
        else:
            self._gview = (self.Q, n, self._state.view(-1), n, rows * n, n)
        self._cdf = torch.empty(self.P, device=self.device, dtype=torch.int64)
        self._states_all = torch.empty(rows, n, device=self.device, dtype=torch.float32)   # the resampled rows
        self._states = self._states_all[:3]
        self._anc = torch.empty(n, device=self.device, dtype=torch.int32)
        # SPEC S10 (a non-default scheme or an ESS gate): the per-slot carry of this rank's shard and 64-B statistics
        self._adaptive = self.resample_method != "systematic" or self.ess_threshold is not None or self._gate
        self.gate_q = occlusion_gate_q(self.occlusion_threshold, self.bits) if self._gate else None
        self.held_frames = 0                                    # SPEC S15: consecutive held frames
        # SPEC S16: the streak from which the predict is the search, and a search frame's gate
        self.search_after = None if self.redetect is None else redetect_after(self.redetect, occ)
        self.search_gate_q = None if self.redetect is None else occlusion_gate_q(
            occ["threshold"] if self.redetect["threshold"] is None else self.redetect["threshold"], self.bits)
        self._frame_gate_q = self.gate_q                        # this frame's gate: search_gate_q on a search frame
        self._searched: Optional[bool] = None                   # this frame's predict was the search
        self._reacquired: Optional[bool] = None
        self.anchor: Optional[Tuple[float, float, float]] = None
        self.carry: Optional[torch.Tensor] = None
        if self._adaptive:
            self.carry = torch.empty(n, device=self.device, dtype=torch.int64)
            self._carry_out = torch.empty(n, device=self.device, dtype=torch.int64)
        self._prior_applied = False                             # Q already holds the posterior weights (S10 rule 1)
        # SPEC S11 / S12: the extra rows' statistics {T, sum Q vx, sum Q vy, sum Q a} (those rows that exist, in row
        # order, then 0) follow the state's in the same buffer and copy
        self._vstats = 8 if self._adaptive else 4
        n_stats = self._vstats + (4 if self._extra else 0)
        # SPEC S17: the mode estimate's 8 words {i*, Tm, six sums} follow them, and the density has a workspace
        self.mode_window = None
        self.set_mode_window(mode_window)
        self._mstats = n_stats
        if self.mode_window is not None:
            n_stats += 8
            self._dens = torch.empty(self.P, device=self.device, dtype=torch.int64)
        self._stats_dev = torch.zeros(n_stats, device=self.device, dtype=torch.int64)
        self._stats_pin = torch.zeros(n_stats, dtype=torch.int64).pin_memory()
        self._stats_evt = torch.cuda.Event()
        self.frame = 0
        self.last_ancestors: Optional[torch.Tensor] = None
        self._settled = False                                   # estimate / resample of the current Q computed
        self._est: Optional[Tuple[float, float, float]] = None  # its host value once read
        self._ess: Optional[float] = None
        self._resampled: Optional[bool] = None
        self._vel: Optional[Tuple[float, float]] = None
        self._ang: Optional[float] = None
        self._held: Optional[bool] = None
        self._peak: Optional[float] = None
        self._evidence: Optional[float] = None
        self._mean: Optional[Tuple[float, float, float]] = None
        self._mode_index: Optional[int] = None
        self._mode_mass: Optional[float] = None
        self.reset(init_state)

    def set_mode_window(self, window: Optional[Sequence[float]]) -> None:
        """SPEC S17: the window half-widths (hx, hy) in pixels, rounded to fp32; finite and >= 0. A filter built without
        a window has no room for the mode statistics and cannot be given one later, nor the reverse."""
        if (window is None) != (self.mode_window is None) and hasattr(self, "_mstats"):
            raise ValueError("mode_window: a filter is built with or without the mode estimate (SPEC S17)")
        if window is None:
            return
        w = tuple(float(np.float32(v)) for v in window)
        if len(w) != 2 or not all(math.isfinite(v) and v >= 0.0 for v in w):
            raise ValueError(f"mode_window must be two finite numbers >= 0 (SPEC S17), got {window!r}")
        self.mode_window = w
        self._settled = False

    # ------------------------------------------------------------------ state
    @property
    def particles(self) -> torch.Tensor:
        """The particles as float32[P_local][3] rows (x, y, scale): SURVEY.md §8b's `.particles [P, 3]`, so
        `particles[:, 0]` is every particle's x. A transposed VIEW of the SoA storage `particles_soa` (float32[3][P_local],
        the layout the kernels and the all-gathered chunk use); writes through it land in the filter's state."""
        return self.particles_soa.t()

    @particles.setter
    def particles(self, value) -> None:
        """Assign [P_local][3] states (x, y, scale per row): copied into the SoA storage."""
        v = torch.as_tensor(value, dtype=torch.float32, device=self.device)
        if tuple(v.shape) != (self.n_local, 3):
            raise ValueError(f"particles: expected shape ({self.n_local}, 3), got {tuple(v.shape)}")
        self.particles_soa.copy_(v.t())
        self._settled = False

    @property
    def states(self) -> torch.Tensor:
        """Alias of `particles` ([P_local][3] view)."""
        return self.particles_soa.t()

    @property
    def velocity(self) -> Optional[torch.Tensor]:
        """SPEC S11: the particles' velocities as float32[P_local][2] rows (vx, vy) in px/frame, a transposed view of
        `velocity_soa`; None under the random walk."""
        return None if self.velocity_soa is None else self.velocity_soa.t()

    @property
    def rotation(self) -> Optional[torch.Tensor]:
        """SPEC S12: the particles' angles in radians as float32[P_local], a view of `rotation_soa`'s row; None without
        `rotation_std`."""
        return None if self.rotation_soa is None else self.rotation_soa[0]

    def reset(self, state) -> None:
        """Every particle at `state`: (x, y, s), or every state row in row order (x, y, s, [vx, vy], [a]: SPEC S11,
        S12); rows not given are 0."""
        state = tuple(float(v) for v in state)
        rows = self._state.shape[0]
        if len(state) not in (3, rows):
            names = "(x, y, s" + (", vx, vy" if self._cv else "") + (", a" if self._rot else "") + ")"
            raise ValueError("reset: state is (x, y, s)" + (f" or {names}" if rows > 3 else ""))
        for row, v in zip(self._state, state + (0.0,) * (rows - len(state))):
            row.fill_(v)
        self.Q.zero_()
        if self.carry is not None:
            self.carry.fill_(1 << (self.bits + 1))
        self._prior_applied = False
        self.frame = 0
        self.held_frames = 0
        if self.redetect is not None:   # SPEC S16: the anchor before any tracked frame is the initial state
            self.anchor = state[:3]
            self._frame_gate_q = self.gate_q
        self._settled = False

    def predict(self, frame: Optional[int] = None, gain: float = 1.0, search: bool = False) -> None:
        """H1: counter-based random walk (SPEC S2), or the constant-velocity model (SPEC S11), for frame index
        `frame` (default: next frame). `gain` (SPEC S15, the frame after a hold): the position sigmas of this call are
        fp32(sigma_x) * fp32(gain) and fp32(sigma_y) * fp32(gain), one rounded fp32 multiply each; every other sigma
        is unchanged. gain = 1 passes the configured values as they are. `search` (SPEC S16, needs `redetect`): the
        search predict replaces the motion model's for this frame (x, y scattered over the frame, the scale stepped as
        ever, velocities zeroed; the gain has nothing left to act on), and the frame's gate is `search_gate_q`."""
        if search and self.redetect is None:
            raise ValueError("predict(search=True) needs redetect (SPEC S16)")
        self.frame = self.frame + 1 if frame is None else int(frame)
        if self.redetect is not None:
            self._searched = bool(search)
            self._frame_gate_q = self.search_gate_q if search else self.gate_q
        std = self.motion_std
        if gain != 1.0:
            g = np.float32(gain)
            std = [float(np.float32(std[0]) * g), float(np.float32(std[1]) * g), std[2]]
        if search:
            from .config import redetect_lattice
            gx, inv_gx, inv_P = redetect_lattice(self.P, self.width, self.height)
            vpf.predict_search_(self._state[:5] if self._cv else self.particles_soa, self.begin, self.P, self.seed,
                                self.frame, self.motion_std[2], float(self.width), float(self.height),
                                self.scale_range, gx, inv_gx, inv_P)
        elif self._cv:
            vpf.predict_cv_(self._state[:5], self.begin, self.seed, self.frame, std, self.velocity_std,
                            self.velocity_decay, self.velocity_max, float(self.width), float(self.height),
                            self.scale_range)
        else:
            vpf.predict_(self.particles_soa, self.begin, self.seed, self.frame, std, float(self.width),
                         float(self.height), self.scale_range)
        if self._rot:   # SPEC S12: the angle row's own kernel, after either motion model's
            vpf.predict_angle_(self.rotation_soa, self.begin, self.seed, self.frame, self.rotation_std,
                               self.rotation_range)
        self._settled = False

    def update(self, features: torch.Tensor, template: torch.Tensor) -> torch.Tensor:
        """H10 from explicit features [n][D] fp32 (LN'd CLS) and a unit template [D]: sets Q."""
        n, D = features.shape
        if n != self.n_local:
            raise ValueError(f"update: expected {self.n_local} feature rows, got {n}")
        vpf.cosine_weight(features.to(torch.float32).contiguous(), template.to(torch.float32).contiguous(),
                          self.lam, self.bits, self.Q, None)
        self._prior_applied = False
        self._settled = False
        return self.Q

    def set_weights(self, Q: torch.Tensor) -> None:
        if Q.data_ptr() != self.Q.data_ptr():
            self.Q.copy_(Q)
        self._prior_applied = False
        self._settled = False

    # ------------------------------------------------------------------ H11 + H12 on the device
    def _settle(self) -> None:
        """Enqueue (world > 1: the chunk all-gather, then) vpf_estimate_resample for the current weights and the
        32-B statistics' copy to pinned host memory. No host synchronisation."""
        if self._settled:
            return
        if self._adaptive and not self._prior_applied:
            vpf.weight_prior_(self.Q, self.carry, self.bits)    # likelihood -> posterior weights, on the local shard
            self._prior_applied = True
        if self.world_size > 1:
            _all_gather_into(self._allc, self._chunk, self.group)
            if self._cidx is not None:
                torch.index_select(self._allc, 0, self._cidx, out=self._glob)
        Qv, qs, Pv, ld, ps, nsh = self._gview
        method = (_lib.VPF_RESAMPLE_STRATIFIED if self.resample_method == "stratified"
                  else _lib.VPF_RESAMPLE_SYSTEMATIC)
        if self._extra and self._gate:    # SPEC S15: the same held decision, from the same tree, picks their sums
            vpf.weighted_sums_gate(Qv, qs, Pv[3 * ld:], ld, ps, nsh, self.P, self._extra, self._frame_gate_q,
                                   self._stats_dev[self._vstats:])
        elif self._extra:  # SPEC S11 / S12: the extra rows' estimate, over the same weights and tree as the state's
            vpf.weighted_sums(Qv, qs, Pv[3 * ld:], ld, ps, nsh, self.P, self._extra, self._stats_dev[self._vstats:])
        if self._gate:
            vpf.estimate_resample_gate(Qv, qs, Pv, ld, ps, nsh, self.P, self.seed, self.frame, self.begin,
                                       self.begin + self.n_local, self._anc, self._states, self._cdf, self._stats_dev,
                                       method, self.bits, self._frame_gate_q, self._carry_out)
        elif self._adaptive:
            vpf.estimate_resample_ex(Qv, qs, Pv, ld, ps, nsh, self.P, self.seed, self.frame, self.begin,
                                     self.begin + self.n_local, self._anc, self._states, self._cdf, self._stats_dev,
                                     method, -1.0 if self.ess_threshold is None else self.ess_threshold, self.bits,
                                     self._carry_out)
        else:
            vpf.estimate_resample(Qv, qs, Pv, ld, ps, nsh, self.P, self.seed, self.frame, self.begin,
                                  self.begin + self.n_local, self._anc, self._states, self._cdf, self._stats_dev)
        if self._extra:    # the slots take their ancestors' extra rows (a skipped resample: their own)
            vpf.gather_rows(self._anc, Pv[3 * ld:], ld, ps, nsh, self.P, self._extra, self._states_all[3:])
        if self.mode_window is not None:    # SPEC S17: the same weights and predicted states; T / held from the call above
            vpf.mode_estimate(Qv, qs, Pv, ld, ps, nsh, self.P, self._extra, self.mode_window[0], self.mode_window[1],
                              self._stats_dev, self._gate, self._dens, self._stats_dev[self._mstats:])
        self._stats_pin.copy_(self._stats_dev, non_blocking=True)
        self._stats_evt.record()
        self._settled = True
        self._est = None

    def _commit(self) -> None:
        """Enqueue the resample computed by _settle: this rank's slots take their ancestors' states."""
        self._state.copy_(self._states_all)
        self.last_ancestors = self._anc.clone()
        if self._adaptive:
            self.carry.copy_(self._carry_out)
        self.Q.zero_()
        self._prior_applied = False
        self._settled = False

    def _read_estimate(self) -> Tuple[float, float, float]:
        """SPEC S6 from the settled statistics (waits for their D2H copy): sum Q*state / T, or the plain mean
        when T == 0. The sums are the same bits on every rank and for every world size."""
        if self._est is None:
            self._stats_evt.synchronize()
            T = int(self._stats_pin[0])
            sx, sy, ss = self._stats_pin[1:4].view(torch.float64).tolist()
            held = self._gate and bool(int(self._stats_pin[7]))
            d = float(T) if T and not held else float(self.P)
            self._est = (sx / d, sy / d, ss / d)
            mode = None
            if getattr(self, "mode_window", None) is not None:  # SPEC S17: the windowed sums over Tm; Tm == 0: S6's mean
                m = self._stats_pin[self._mstats: self._mstats + 8]
                tm = int(m[1])
                self._mean, self._mode_index, self._mode_mass = self._est, int(m[0]), float(tm) / d
                if tm:
                    mode = [v / float(tm) for v in m[2:8].view(torch.float64).tolist()]
                    self._est = tuple(mode[:3])
            if self._gate:      # SPEC S15; read once per settled frame, so the streak counts frames
                self._held = held
                self._peak = float(int(self._stats_pin[6])) / float(1 << self.bits)
                self._evidence = float(T) / (float(self.P) * float(1 << self.bits))
                self.held_frames = self.held_frames + 1 if held else 0
            if self.redetect is not None:       # SPEC S16: a held search frame reports the anchor, not the frame centre
                self._reacquired = bool(self._searched) and not held
                if not self._searched:
                    self.anchor = self._est
                elif held:
                    self._est = self.anchor
            if self._adaptive:
                self._ess = float(self._stats_pin[4:5].view(torch.float64)[0])
                self._resampled = bool(int(self._stats_pin[5]))
            else:
                self._resampled = True
            if self._extra:
                ext = self._stats_pin[self._vstats + 1: self._vstats + 1 + self._extra].view(torch.float64).tolist()
                if self._cv:
                    self._vel = (ext[0] / d, ext[1] / d)
                if self._rot:
                    self._ang = ext[-1] / d
                if mode is not None:        # SPEC S17: the window's own velocity and angle
                    if self._cv:
                        self._vel = (mode[3], mode[4])
                    if self._rot:
                        self._ang = mode[3 + self._extra - 1]
        return self._est

    @property
    def last_held(self) -> Optional[bool]:
        """SPEC S15: whether the last estimate() / step() frame was held (its largest weight below the gate); None
        without `occlusion_threshold`."""
        return self._held

    @property
    def last_peak(self) -> Optional[float]:
        """SPEC S15: max_i L_i / 2^K of the last frame, the statistic the gate compares with theta (the same bits on
        every rank); None without `occlusion_threshold`."""
        return self._peak

    @property
    def last_evidence(self) -> Optional[float]:
        """SPEC S15: the last frame's mean likelihood float(T) / (float(P) 2^K); None without `occlusion_threshold`."""
        return self._evidence

    @property
    def lost(self) -> Optional[bool]:
        """SPEC S15: held_frames > occlusion_max_hold. A flag only: the filter goes on holding; the caller re-inits.
        None without `occlusion_threshold`."""
        return self.held_frames > self.occlusion_max_hold if self._gate else None

    @property
    def last_searched(self) -> Optional[bool]:
        """SPEC S16: whether the last frame's predict was the search; None without `redetect`."""
        return self._searched

    @property
    def last_reacquired(self) -> Optional[bool]:
        """SPEC S16: whether the last estimate() / step() frame was searched and not held: the target was found and the
        resample collapsed the lattice onto it; None without `redetect`."""
        return self._reacquired

    @property
    def last_mean(self) -> Optional[Tuple[float, float, float]]:
        """SPEC S17: SPEC S6's weighted mean of the last estimate() / step(), which a mode filter no longer returns
        (on a held search frame too: the cloud's plain mean, not the anchor); None without `mode_window`."""
        return self._mean

    @property
    def last_mode_index(self) -> Optional[int]:
        """SPEC S17: i*, the global index of the particle whose window holds the most weight (the smallest such index);
        None without `mode_window`."""
        return self._mode_index

    @property
    def last_mode_mass(self) -> Optional[float]:
        """SPEC S17: Tm / T in fp64, the share of the posterior inside the reported window (Tm / P on a frame whose
        weights count as 1): near 1 for a single hump, lower the more weight lies elsewhere; None without
        `mode_window`."""
        return self._mode_mass

    @property
    def last_rotation(self) -> Optional[float]:
        """SPEC S12: the angle estimate sum Q_i a_i / T in radians of the last estimate() / step() (a linear mean: the
        row is clamped, not wrapped; the same bits on every rank); None without `rotation_std`."""
        return self._ang

    @property
    def last_velocity(self) -> Optional[Tuple[float, float]]:
        """SPEC S11: the velocity estimate (vx, vy) = sum Q_i v_i / T in px/frame of the last estimate() / step()
        (the same bits on every rank); None under the random walk."""
        return self._vel

    @property
    def last_ess(self) -> Optional[float]:
        """SPEC S10: N_eff = (sum Q)^2 / sum Q^2 of the posterior weights of the last estimate() / step() (the same
        bits on every rank); None on the default path, which does not compute it."""
        return self._ess

    @property
    def last_resampled(self) -> Optional[bool]:
        """Whether the last estimate() / step() frame's resample ran (SPEC S10 rule 4) or was skipped; the default
        path resamples every frame (True)."""
        return self._resampled

    def estimate(self) -> Tuple[float, float, float]:
        """SPEC S6: weighted mean state of the current particles and weights."""
        self._settle()
        return self._read_estimate()

    def resample(self) -> torch.Tensor:
        """SPEC S7 systematic resample; returns the global ancestor indices of this rank's slots."""
        self._settle()
        self._commit()
        return self.last_ancestors

    def step(self) -> Tuple[float, float, float]:
        """estimate() then resample() of one frame, with the resample enqueued before the host waits for the
        estimate (Tracker.track)."""
        self._settle()
        self._commit()
        return self._read_estimate()
