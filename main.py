"""`python main.py [--config config.yaml]` — the entry point the reference documents (README.md:34-38):
read the config, feed frames to the Tracker, print the tracked positions (README.md:42).

Several targets (README.md:46-50, SPEC S9): `input.bboxes: [[x, y, w, h], ...]` runs a MultiTracker (one batched ViT
pass over every target's particles); each frame then prints and records one position per target, --video-out
draws every box, and --checkpoint / --resume save and restore every target.

Multi-GPU: `torchrun --nproc-per-node G --master-addr 127.0.0.1 main.py` shards the particles over G GPUs.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys
import time


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "config.yaml"))
    ap.add_argument("--frames", type=int, default=None, help="override input.frames")
    ap.add_argument("--out", default=None, help="write positions as JSON here")
    ap.add_argument("--video-out", default=None,
                    help="write the frames with the tracked box drawn: a .y4m file, or a directory of frames")
    ap.add_argument("--frame-format", default="ppm", choices=["ppm", "png", "jpg"],
                    help="image format of the --video-out directory's frames (png / jpg through Pillow)")
    ap.add_argument("--checkpoint", default=None,
                    help="save the tracker state (np.savez; per rank with several GPUs) here after the last frame")
    ap.add_argument("--checkpoint-every", type=int, default=0, help="also save every N frames")
    ap.add_argument("--resume", default=None,
                    help="continue from a checkpoint: the source's frames up to its frame index are skipped")
    ap.add_argument("--ess", action="store_true",
                    help="append each frame's effective sample size N_eff and whether it resampled (SPEC S10; needs "
                         "resample.ess_threshold or resample.method: stratified, otherwise N_eff is not computed) to the "
                         "printed line and to the --out records")
    ap.add_argument("--velocity", action="store_true",
                    help="append each frame's velocity estimate vx, vy in px/frame (SPEC S11; needs "
                         "particles.motion_model: constant_velocity, otherwise n/a) to the printed line and to the "
                         "--out records")
    ap.add_argument("--rotation", action="store_true",
                    help="append each frame's angle estimate in radians (SPEC S12; needs particles.rotation_std, "
                         "otherwise n/a) to the printed line and to the --out records")
    ap.add_argument("--confidence", action="store_true",
                    help="append each frame's peak likelihood, mean likelihood (evidence), held and lost flags (SPEC "
                         "S15; needs likelihood.occlusion, otherwise n/a) to the printed line and to the --out records")
    ap.add_argument("--mode", action="store_true",
                    help="append each frame's mode mass (the share of the posterior inside the reported window) and the "
                         "weighted mean that the mode estimate replaces (SPEC S17; needs estimate.method: mode, otherwise "
                         "n/a) to the printed line and to the --out records")
    ap.add_argument("--dist-timeout", type=float, default=120.0,
                    help="seconds: bound on the multi-GPU rendezvous and on any collective (vpf.distributed)")
    args = ap.parse_args(argv)

    import torch
    import torch.distributed as dist
    from vitparticlefiltertracker_amd import MultiTracker, Tracker, load_config
    from vitparticlefiltertracker_amd.frames import iter_frames, prefetch, synthetic_clip

    cfg = load_config(args.config)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not dist.is_initialized():
        from vitparticlefiltertracker_amd.distributed import init_distributed
        dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(dev)
        # RCCL bound to this rank's GPU eagerly (device_id), a bounded rendezvous and one probe collective (as bench.py)
        init_distributed("nccl", dev, args.dist_timeout)
    inp = cfg["input"]
    n = args.frames or int(inp["frames"])
    if inp["source"] == "synthetic":
        src = iter_frames(synthetic_clip(n, inp["height"], inp["width"], tuple(inp["bbox0"]), inp["seed"],
                                         target_range=inp.get("target_range")))   # SPEC S13: a tinted target
    else:
        src = itertools.islice(iter_frames(inp["source"]), n)
    frames = prefetch(src, depth=2)   # decode + pin on a host thread, overlapped with the GPU frame loop
    # one loop for both forms: `input.bboxes` runs a MultiTracker over its K boxes, otherwise a Tracker follows `bbox0`
    boxes = inp.get("bboxes")
    single = boxes is None
    rotating = cfg["particles"]["rotation_std"] is not None      # SPEC S12: the boxes carry an angle
    if single:
        tr = Tracker(cfg)
        boxes, angles0 = [inp["bbox0"]], [inp["angle0"]] if rotating else None
    else:
        tr = MultiTracker(cfg, n_objects=len(boxes))
        angles0 = [float(a) for a in (inp.get("angles") or [0.0] * len(boxes))] if rotating else None
    first = next(frames)
    start = 1
    if args.resume:
        tr.load_checkpoint(args.resume)
        for _ in range(tr.frame_index):       # frames 1 .. frame_index were tracked before the checkpoint
            if next(frames, None) is None:
                raise SystemExit(f"--resume: the checkpoint is at frame {tr.frame_index}, past the end of the input")
        start = tr.frame_index + 1
    elif single:
        tr.init(first, boxes[0], angles0[0] if rotating else 0.0)
    else:
        tr.init(first, boxes, angles0)
    emit, close = _sink(args, tr.rank)
    if not args.resume:
        emit(0, first, boxes, angles0)
    t0 = time.perf_counter()
    out = []
    for k, f in enumerate(frames, start=start):
        ests = [tr.track(f)] if single else tr.track(f)
        fields = [_flag_fields(args, tr, None if single else i) for i in range(len(ests))]
        out.append(_frame_record(k, ests, fields, single))
        # the box sizes being tracked (restored from the checkpoint after --resume), not the config's
        emit(k, f, [_box(st, (0.0, 0.0, w, h)) for st, (w, h) in zip(ests, tr.boxes)],
             [tr.last_rotation] if single else tr.last_rotation)
        if tr.rank == 0:
            print(_frame_line(k, ests, fields, single), flush=True)
        if args.checkpoint and args.checkpoint_every > 0 and k % args.checkpoint_every == 0:
            tr.save_checkpoint(args.checkpoint)
    if args.checkpoint:
        tr.save_checkpoint(args.checkpoint)
    close()
    dt = time.perf_counter() - t0
    if tr.rank == 0:
        what = f"{len(out)} frames" if single else f"{len(out)} frames x {len(boxes)} targets"
        print(f"{what} in {dt:.3f} s ({len(out) / max(dt, 1e-9):.2f} frames/s)", file=sys.stderr)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)
    if dist.is_initialized():
        dist.destroy_process_group()
    return 0


def _flag_fields(args, tr, i=None):
    """(record fields, text) that --ess --velocity --rotation --confidence --mode add to the last tracked frame of a
    Tracker, or of target i of a MultiTracker, in that order; each flag is consulted here and nowhere else."""
    at = (lambda v: v) if i is None else (lambda v: v[i])
    rec, text = {}, ""
    if args.ess:
        ess, resampled = at(tr.last_ess), at(tr.last_resampled)
        rec.update(ess=ess, resampled=resampled)
        text += _ess_text(ess, resampled)
    if args.velocity:
        rec.update(_vel_record(at(tr.last_velocity)))
        text += _vel_text(at(tr.last_velocity))
    if args.rotation:
        rec.update(angle=at(tr.last_rotation))
        text += _angle_text(at(tr.last_rotation))
    if args.confidence:
        conf = (at(tr.last_peak), at(tr.last_evidence), at(tr.last_held), at(tr.lost), _search_of(tr, i))
        rec.update(_conf_record(*conf))
        text += _conf_text(*conf)
    if args.mode:
        rec.update(_mode_record(at(tr.last_mode_mass), at(tr.last_mean)))
        text += _mode_text(at(tr.last_mode_mass), at(tr.last_mean))
    return rec, text


def _frame_record(k, ests, fields, single) -> dict:
    """Frame k's --out record from every target's estimate and `_flag_fields`: the one target's fields beside
    `frame` for a single target, a `targets` list under `input.bboxes`."""
    targets = [{"x": x, "y": y, "scale": s, **rec} for (x, y, s), (rec, _) in zip(ests, fields)]
    return {"frame": k, **targets[0]} if single else {"frame": k, "targets": targets}


def _frame_line(k, ests, fields, single) -> str:
    """Frame k's printed line: `x= y= scale=` for a single target, one `[i] x= y= s=` segment per target under
    `input.bboxes`, each followed by its `_flag_fields` text."""
    if single:
        (x, y, s), (_, text) = ests[0], fields[0]
        return f"frame {k:4d}  x={x:8.2f}  y={y:8.2f}  scale={s:6.3f}" + text
    return f"frame {k:4d}  " + "  ".join(f"[{i}] x={x:8.2f} y={y:8.2f} s={s:6.3f}" + text
                                         for i, ((x, y, s), (_, text)) in enumerate(zip(ests, fields)))


def _sink(args, rank):
    """(emit(k, rgb, boxes, angles), close()) for --video-out: the frame with every box drawn (turned by its angle where
    one is given: SPEC S12), as .y4m or image frames."""
    from vitparticlefiltertracker_amd.frames import Y4MWriter, box_corners, draw_box, draw_quad
    if not args.video_out or rank != 0:
        return (lambda k, rgb, boxes, angles=None: None), (lambda: None)
    writer = Y4MWriter(args.video_out) if args.video_out.lower().endswith(".y4m") else None
    if writer is None:
        os.makedirs(args.video_out, exist_ok=True)

    def emit(k, rgb, boxes, angles=None):
        img = rgb.numpy() if hasattr(rgb, "numpy") else rgb
        for b, a in zip(boxes, angles or [None] * len(boxes)):
            img = draw_box(img, b) if a is None else draw_quad(img, box_corners(b, a))
        if writer is not None:
            writer.write(img)
        else:
            _write_frame(args, k, img)
    return emit, (writer.close if writer is not None else (lambda: None))


def _write_frame(args, k, img) -> None:
    """Frame k of a --video-out directory in --frame-format (PPM with numpy; PNG / JPEG through Pillow)."""
    from vitparticlefiltertracker_amd.frames import write_image_pil, write_ppm
    path = os.path.join(args.video_out, f"frame_{k:05d}.{args.frame_format}")
    if args.frame_format == "ppm":
        write_ppm(path, img)
    else:
        write_image_pil(path, img)


def _ess_text(ess, resampled) -> str:
    """--ess: the frame's N_eff (n/a on the default path, which does not compute it) and its resample decision."""
    return f"  ess={'n/a' if ess is None else format(ess, '.2f'):>9}  resampled={int(bool(resampled))}"


def _vel_record(vel) -> dict:
    """--velocity: the frame's velocity estimate as record fields (null under the random walk)."""
    return {"vx": None if vel is None else vel[0], "vy": None if vel is None else vel[1]}


def _vel_text(vel) -> str:
    """--velocity: the frame's velocity estimate in px/frame (n/a under the random walk, which has none)."""
    vx, vy = ("n/a", "n/a") if vel is None else (format(vel[0], ".2f"), format(vel[1], ".2f"))
    return f"  vx={vx:>7}  vy={vy:>7}"


def _angle_text(angle) -> str:
    """--rotation: the frame's angle estimate in radians (n/a without particles.rotation_std, which has none)."""
    return f"  angle={'n/a' if angle is None else format(angle, '.3f'):>7}"


def _search_of(tr, i=None):
    """--confidence: (last_searched, last_reacquired) of a Tracker, or of target i of a MultiTracker, when
    likelihood.redetect is set (SPEC S16); None otherwise: the output is then SPEC S15's, byte for byte."""
    if tr.redetect is None:
        return None
    return (tr.last_searched, tr.last_reacquired) if i is None else (tr.last_searched[i], tr.last_reacquired[i])


def _conf_record(peak, evidence, held, lost, search=None) -> dict:
    """--confidence: the frame's SPEC S15 outputs as record fields (null without likelihood.occlusion), and SPEC S16's
    two flags when likelihood.redetect is set (`search`: _search_of's pair)."""
    rec = {"peak": peak, "evidence": evidence, "held": held, "lost": lost}
    if search is not None:
        rec.update(searched=search[0], reacquired=search[1])
    return rec


def _conf_text(peak, evidence, held, lost, search=None) -> str:
    """--confidence: peak and mean likelihood and the held / lost flags (n/a without likelihood.occlusion); with
    likelihood.redetect also the searched / reacquired flags (SPEC S16)."""
    if peak is None:
        return "  peak=    n/a  evidence=    n/a  held=n/a  lost=n/a"
    more = "" if search is None else f"  searched={int(search[0])}  reacquired={int(search[1])}"
    return f"  peak={peak:7.4f}  evidence={evidence:7.4f}  held={int(held)}  lost={int(lost)}" + more


def _mode_record(mass, mean) -> dict:
    """--mode: the frame's SPEC S17 outputs as record fields (null without the mode estimate)."""
    mx, my, ms = (None, None, None) if mean is None else mean
    return {"mode_mass": mass, "mean_x": mx, "mean_y": my, "mean_scale": ms}


def _mode_text(mass, mean) -> str:
    """--mode: the share of the posterior inside the reported window and SPEC S6's mean (n/a without estimate.method:
    mode, which computes neither)."""
    if mass is None:
        return "  mass=   n/a  mean_x=     n/a  mean_y=     n/a  mean_scale=   n/a"
    return f"  mass={mass:6.4f}  mean_x={mean[0]:8.2f}  mean_y={mean[1]:8.2f}  mean_scale={mean[2]:6.3f}"


def _box(state, bbox0):
    """(x, y, w, h) of a state (centre, scale) for a target whose frame-0 box is bbox0 (SPEC S3)."""
    x, y, s = (float(v) for v in state)
    w, h = s * float(bbox0[2]), s * float(bbox0[3])
    return x - 0.5 * w, y - 0.5 * h, w, h


if __name__ == "__main__":
    sys.exit(main())
