"""Timing of the patch-token cue (SPEC S18), which bench.py cannot enable.

    python tools/token_timing.py [--particles 4096] [--arch vit_base_patch16_224] [--dtype bf16] [--frames 8]

In one process: the KernelTimer time of `token_weight` per frame (eager), `row_stats` over the same n x N rows of the
same buffer beside it (it reads the same bytes: the reference), and the frame time of the graph-replayed tracker with
the cue on and off. Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from vitparticlefiltertracker_amd import Tracker, load_config                     # noqa: E402
from vitparticlefiltertracker_amd.frames import synthetic_clip                      # noqa: E402
from vitparticlefiltertracker_amd.vit import KernelTimer                            # noqa: E402


def frame_ms(tr, clip, warmup):
    tr.init(clip[0], (80, 80, 64, 64))
    for f in clip[1:1 + warmup]:
        tr.track(f)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f in clip[1 + warmup:]:
        tr.track(f)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / (len(clip) - 1 - warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=4096)
    ap.add_argument("--arch", default="vit_base_patch16_224")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    clip = synthetic_clip(1 + a.warmup + a.frames)

    def cfg(tokens):
        return load_config({"model": {"arch": a.arch, "dtype": a.dtype}, "particles": {"num": a.particles},
                            "likelihood": {"tokens": tokens}})
    out = {"particles": a.particles, "arch": a.arch, "dtype": a.dtype}
    tr = Tracker(cfg({}), use_graph=False)
    tr.init(clip[0], (80, 80, 64, 64))
    for f in clip[1:1 + a.warmup]:
        tr.track(f)
    eng = tr.engine
    eng.timer = KernelTimer()
    n, N, D = a.particles, eng.arch.tokens, eng.arch.dim
    for f in clip[1 + a.warmup:]:
        tr.track(f)
        eng.timer("row_stats_all_rows", torch.ops.vpf.row_stats, eng.h[:n].view(n * N, D), eng.arch.ln_eps,
                  eng.stats[: n * N])
    s = eng.timer.summary()
    eng.timer = None
    out["token_weight_ms"] = s["token_weight"]["avg_ms"]
    out["row_stats_same_rows_ms"] = s["row_stats_all_rows"]["avg_ms"]
    out["cls_weight_ms"] = s["cls_weight"]["avg_ms"]
    out["token_bytes_gb"] = n * (N - 1) * D * eng.h.element_size() / 1e9
    del tr, eng
    out["frame_ms_tokens_on"] = frame_ms(Tracker(cfg({})), clip, a.warmup)
    out["frame_ms_tokens_off"] = frame_ms(Tracker(cfg(None)), clip, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
