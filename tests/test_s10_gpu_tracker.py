"""GPU (one MI355X): SPEC S10 end to end — the Tracker / MultiTracker with `resample.method: stratified` and an ESS
threshold on real HIP kernels (ViT-Ti, bf16, 6 frames): replayed through the Python-int reference, sharded over ranks,
resumed from a checkpoint, and per target.

LAM / TAU: with the seeded random weights the cosines are all close to 1, so lambda = 20 (the default) gives nearly
flat likelihoods (N_eff ~ 0.93 P after one frame) that sharpen as they accumulate in the carry; tau = 0.92 then skips
the first frame and resamples the second. Measured on the MI355X at P = 100 (particle seed 99, weight seed 3,
synthetic_clip(7)): N_eff = 93.5, 89.3, 93.9, 87.1, 95.2, 88.4 and flags skip, resample, skip, resample, skip,
resample. (lambda = 100 and above resample every frame at any tau >= 0.5; lambda = 20 with tau = 0.5 never does in 6
frames.)"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import s10_reference as R

pytestmark = pytest.mark.gpu

FRAMES = 6
LAM, TAU, METHOD = 20.0, 0.92, R.STRATIFIED
P0, BOX = 100, (80, 80, 64, 64)


def _cfg(P=P0, seed=99, method=METHOD, tau=TAU):
    from vitparticlefiltertracker_amd import load_config
    return load_config({"model": {"arch": "vit_tiny_patch16_224", "dtype": "bf16", "weights": {"seed": 3}},
                        "particles": {"num": P, "seed": seed}, "likelihood": {"lambda": LAM},
                        "resample": {"method": method, "ess_threshold": tau}})


def _frame(tr, f):
    """One tracked frame's record: estimate, flag, ess, this rank's likelihood weights (as the engine left them),
    ancestors, states and carry."""
    est = tr.track(f)
    return {"est": est, "flag": tr.last_resampled, "ess": tr.last_ess,
            "L": tr.engine.Q[: tr.n_local].cpu().numpy().copy(), "anc": tr.pf.last_ancestors.cpu().numpy().copy(),
            "parts": tr.pf.particles_soa.cpu().numpy().copy(), "carry": tr.pf.carry.cpu().numpy().copy()}


def _run(tr, clip):
    tr.init(clip[0], BOX)
    return [_frame(tr, f) for f in clip[1:]]


def _same(a, b, sl=slice(None), tag=""):
    assert a["est"] == b["est"] and a["flag"] == b["flag"], tag
    assert R.f64_bits(a["ess"]) == R.f64_bits(b["ess"]), tag
    assert np.array_equal(a["anc"], b["anc"][sl]), f"{tag}: ancestors"
    assert np.array_equal(a["parts"].view(np.uint32), b["parts"][:, sl].view(np.uint32)), f"{tag}: states"
    assert np.array_equal(a["carry"], b["carry"][sl]), f"{tag}: carry"


@pytest.fixture(scope="module")
def single():
    """The single-rank gated run every test here compares against (computed once)."""
    from vitparticlefiltertracker_amd import Tracker
    from vitparticlefiltertracker_amd.frames import synthetic_clip
    return _run(Tracker(_cfg(), device="cuda:0"), synthetic_clip(FRAMES + 1))


def test_tracker_replays_through_the_reference(single):
    """The engine's likelihood weights of every frame, replayed through the S10 recursion in Python ints: flags, ess
    bits, ancestors, states and carries bit for bit, estimates to 1e-12; the run holds a skip and a resample."""
    c = _cfg()["particles"]
    cx, cy = BOX[0] + 0.5 * BOX[2], BOX[1] + 0.5 * BOX[3]
    ref = R.Filter(P0, (cx, cy, 1.0), c["motion_std"], c["scale_range"], c["seed"], (224, 224), 40, METHOD, TAU)
    for k, got in enumerate(single, start=1):
        ref.predict(k)
        r = ref.update(got["L"])
        assert got["flag"] == r["resampled"], f"frame {k}"
        assert R.f64_bits(got["ess"]) == R.f64_bits(r["ess"]), f"frame {k}"
        assert np.array_equal(got["anc"], r["anc"]), f"frame {k}: ancestors"
        assert np.array_equal(got["parts"].view(np.uint32), r["states"].view(np.uint32)), f"frame {k}: states"
        assert np.array_equal(got["carry"], r["carry"]), f"frame {k}: carry"
        np.testing.assert_allclose(got["est"], R.estimate(r, P0), rtol=1e-12)
    flags = [g["flag"] for g in single]
    assert True in flags and False in flags, flags


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vitparticlefiltertracker_amd import Tracker
        from vitparticlefiltertracker_amd.frames import synthetic_clip
        tr = Tracker(_cfg(), device="cuda:0", rank=rank, world_size=world)
        q.put((rank, _run(tr, synthetic_clip(FRAMES + 1))))
    except Exception as e:  # report instead of hanging the parent
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_gated_tracker_equals_single_rank(world, single):
    """P = 100 over 2 ranks (equal shards) and 3 (33 / 33 / 34, compacted after the gather), gloo on one GPU: every
    rank takes the single-rank run's decisions and gets its estimates, ess, ancestors, states and carries bit for bit
    (the carry is per slot and local: it never crosses ranks)."""
    from vitparticlefiltertracker_amd.particle_filter import shard_range
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        assert not isinstance(out[r], str), out[r]
        b, n = shard_range(P0, world, r)
        for k, (got, ref) in enumerate(zip(out[r], single), start=1):
            _same(got, ref, slice(b, b + n), f"rank {r} frame {k}")
            assert np.array_equal(got["L"], ref["L"][b:b + n]), f"rank {r} frame {k}: likelihood weights"


def test_checkpoint_after_a_skipped_frame_resumes_bit_exact(tmp_path, single):
    """Save after a frame whose resample was skipped (the carry is not the identity there), load into a fresh
    tracker, continue: the rest of the run equals the uninterrupted one bit for bit."""
    from vitparticlefiltertracker_amd import Tracker
    from vitparticlefiltertracker_amd.frames import synthetic_clip
    clip = synthetic_clip(FRAMES + 1)
    k = next(i for i, g in enumerate(single, start=1) if not g["flag"] and i > 1)     # a skipped frame, not the first
    a = Tracker(_cfg(), device="cuda:0")
    a.init(clip[0], BOX)
    for f in clip[1:k + 1]:
        a.track(f)
    assert a.last_resampled is False and not np.all(a.pf.carry.cpu().numpy() == R.identity(40))
    path = a.save_checkpoint(str(tmp_path / "ck"))
    with np.load(path) as z:
        assert "carry" in z.files and np.array_equal(z["carry"], single[k - 1]["carry"])
    b = Tracker(_cfg(), device="cuda:0")
    b.load_checkpoint(path)
    assert b.frame_index == k
    for i, f in enumerate(clip[k + 1:], start=k + 1):
        _same(_frame(b, f), single[i - 1], tag=f"frame {i} after resume")
    # a tracker with another threshold (or the default configuration) refuses the file
    for other in (_cfg(tau=0.5), _cfg(method="systematic", tau=None)):
        with pytest.raises(ValueError):
            Tracker(other, device="cuda:0").load_checkpoint(path)


def test_default_checkpoint_has_no_carry_and_the_old_fingerprint():
    from vitparticlefiltertracker_amd import Tracker
    from vitparticlefiltertracker_amd.frames import synthetic_clip
    clip = synthetic_clip(2)
    tr = Tracker(_cfg(method="systematic", tau=None), device="cuda:0")
    tr.init(clip[0], BOX)
    tr.track(clip[1])
    assert tr.pf.carry is None and tr.last_resampled is True and tr.last_ess is None
    sd = tr.state_dict()
    assert "carry" not in sd
    assert not {"resample_method", "ess_threshold"} & set(tr.config_fingerprint())


def test_multitracker_targets_equal_their_own_trackers():
    """SPEC S9 under S10: target k of a two-target MultiTracker equals a single-target Tracker with seed + k and its
    box — estimates, flags, ess, states and its own carry, bit for bit."""
    from vitparticlefiltertracker_amd import MultiTracker, Tracker
    from vitparticlefiltertracker_amd.frames import synthetic_clip
    P, boxes = 64, [(80, 80, 64, 64), (60, 70, 48, 56)]
    clip = synthetic_clip(FRAMES + 1)
    mt = MultiTracker(_cfg(P), n_objects=2, device="cuda:0")
    mt.init(clip[0], boxes)
    trs = [Tracker(_cfg(P, seed=99 + k), device="cuda:0") for k in range(2)]
    for tr, bx in zip(trs, boxes):
        tr.init(clip[0], bx)
    for i, f in enumerate(clip[1:], start=1):
        ests = mt.track(f)
        for k, tr in enumerate(trs):
            assert tr.track(f) == ests[k], f"frame {i} target {k}"
            assert mt.last_resampled[k] == tr.last_resampled, f"frame {i} target {k}"
            assert R.f64_bits(mt.last_ess[k]) == R.f64_bits(tr.last_ess)
            assert torch.equal(mt.pfs[k].particles_soa, tr.pf.particles_soa)
            assert torch.equal(mt.pfs[k].carry, tr.pf.carry)
            assert torch.equal(mt.pfs[k].last_ancestors, tr.pf.last_ancestors)


def test_main_reads_the_keys_and_reports_ess(tmp_path, capsys):
    """main.py takes resample.method / resample.ess_threshold from the YAML; --ess appends N_eff and the decision to
    the printed line and the --out records, and without it the records are the plain ones."""
    import json
    import main as vpf_main
    cpath = tmp_path / "config.yaml"
    cpath.write_text("model: {arch: vit_tiny_patch16_224, dtype: bf16, weights: {seed: 3}}\n"
                     f"particles: {{num: {P0}, seed: 99}}\n"
                     f"resample: {{method: stratified, ess_threshold: {TAU}}}\n"
                     "input: {source: synthetic, frames: 4}\n")
    plain, rich = tmp_path / "plain.json", tmp_path / "rich.json"
    assert vpf_main.main(["--config", str(cpath), "--out", str(plain)]) == 0
    text_plain = capsys.readouterr().out
    assert vpf_main.main(["--config", str(cpath), "--out", str(rich), "--ess"]) == 0
    text_rich = capsys.readouterr().out
    a, b = json.loads(plain.read_text()), json.loads(rich.read_text())
    assert all(set(r) == {"frame", "x", "y", "scale"} for r in a) and "ess" not in text_plain
    assert [{k: r[k] for k in ("frame", "x", "y", "scale")} for r in b] == a
    assert all(0.0 < r["ess"] <= P0 and isinstance(r["resampled"], bool) for r in b)
    assert text_rich.count("ess=") == len(b) == 3 and text_rich.count("resampled=") == 3
