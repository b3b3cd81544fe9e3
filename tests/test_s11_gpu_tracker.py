"""GPU (one MI355X): SPEC S11 end to end — the ParticleFilter, Tracker and MultiTracker with
`particles.motion_model: constant_velocity` on real HIP kernels, replayed through the Python reference
(tests/s11_reference.py), sharded over ranks (gloo on one GPU), resumed from a checkpoint and driven by main.py; and the
default random walk left as it was."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import s10_reference as R10
import s11_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K40 = 40
INIT, MS, SR, HW = (100.0, 90.0, 1.0), (3.0, 2.0, 0.03), (0.6, 1.8), (224, 224)
CV = {"motion_model": "constant_velocity", "velocity_std": (1.0, 0.5), "velocity_decay": 0.9, "velocity_max": 3.0}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pf(P, seed, **kw):
    from vitparticlefiltertracker_amd.particle_filter import ParticleFilter
    return ParticleFilter(P, INIT, MS, SR, seed, DEV, frame_size=HW, lam=20.0, weight_bits=K40, **{**CV, **kw})


def _ref(P, seed, method=R10.SYSTEMATIC, tau=None):
    return R.Filter(P, INIT, MS, SR, seed, HW, K40, CV["velocity_std"], CV["velocity_decay"], CV["velocity_max"],
                    method, tau)


def _injected(P, k, rng):
    """Frame k's likelihood weights: flat on odd frames (N_eff ~ P), concentrated on even ones (N_eff << P)."""
    if k % 2:
        return rng.integers((1 << 40) - (1 << 30), (1 << 40) + 1, P, dtype=np.int64)
    L = rng.integers(0, 1 << 20, P, dtype=np.int64)
    L[rng.integers(0, P, 3)] = 1 << 40
    return L


def _state5(pf):
    return torch.cat([pf.particles_soa, pf.velocity_soa]).cpu().numpy()


# ------------------------------------------------------------------ ParticleFilter against the reference recursion
@pytest.mark.parametrize("method,tau", [(R10.SYSTEMATIC, None), (R10.STRATIFIED, None), (R10.SYSTEMATIC, 0.5)])
def test_particle_filter_recursion_equals_reference(method, tau):
    """P = 300, 8 frames of injected weights: the five-row state after predict and after the resample, the ancestors,
    the estimate and the velocity estimate (1e-12) follow the reference; vmax = 3 with sigma_v = 1 makes the velocity
    clamp fire along the way. The gated run holds frames of both kinds."""
    P, seed = 300, 321
    f = _pf(P, seed, resample_method=method, ess_threshold=tau)
    ref = _ref(P, seed, method, tau)
    assert f.velocity_soa.shape == (2, P) and f.velocity.shape == (P, 2) and f.particles_soa.shape == (3, P)
    assert f.velocity_soa.data_ptr() == f.particles_soa.data_ptr() + 3 * P * 4 and f.last_velocity is None
    assert not f.velocity_soa.any()
    rng = np.random.default_rng(3)
    flags, clamped = [], False
    for k in range(1, 9):
        L = _injected(P, k, rng)
        f.predict()
        ref.predict()
        assert np.array_equal(bits(_state5(f)), bits(ref.state)), f"frame {k}: predicted state"
        clamped |= bool((np.abs(ref.state[3:]) == CV["velocity_max"]).any())
        f.set_weights(torch.from_numpy(L).to(DEV))
        if k % 4 == 0:
            est = f.estimate()
            vel = f.last_velocity
            anc = f.resample().cpu().numpy()
        else:
            est = f.step()
            vel = f.last_velocity
            anc = f.last_ancestors.cpu().numpy()
        r = ref.update(L)
        flags.append(f.last_resampled)
        assert f.last_resampled == r["resampled"], f"frame {k}"
        assert np.array_equal(anc, r["anc"]), f"frame {k}: ancestors"
        assert np.array_equal(bits(_state5(f)), bits(r["state"])), f"frame {k}: resampled state"
        np.testing.assert_allclose(est, R10.estimate(r, P), rtol=1e-12)
        np.testing.assert_allclose(vel, R.velocity(r, P), rtol=1e-12)
    assert clamped
    assert set(flags) == ({True, False} if tau is not None else {True}), flags
    # reset: velocities back to 0, or to the two extra values
    f.reset((1.0, 2.0, 1.0))
    assert not f.velocity_soa.any() and f.particles_soa[1].eq(2.0).all()
    f.reset((1.0, 2.0, 1.0, -0.5, 0.25))
    assert f.velocity_soa[0].eq(-0.5).all() and f.velocity_soa[1].eq(0.25).all()
    with pytest.raises(ValueError):
        f.reset((1.0, 2.0))


def test_zero_weights_give_the_plain_mean_velocity():
    P = 300
    f = _pf(P, 5)
    f.predict()
    v = f.velocity_soa.cpu().numpy().astype(np.float64)
    f.set_weights(torch.zeros(P, dtype=torch.int64, device=DEV))
    f.step()
    import math
    assert v.any()
    np.testing.assert_allclose(f.last_velocity, [math.fsum(row) / P for row in v], rtol=1e-12)


def test_default_path_is_untouched():
    from vitparticlefiltertracker_amd.particle_filter import ParticleFilter, chunk_words
    P = 100
    f = ParticleFilter(P, INIT, MS, SR, 321, DEV, frame_size=HW, lam=20.0, weight_bits=K40)
    assert f.velocity_soa is None and f.velocity is None and f.last_velocity is None
    assert f._chunk.numel() == chunk_words(P) == 5 * P and f._stats_dev.numel() == 4
    assert f.particles_soa.data_ptr() == f._chunk.data_ptr() + 8 * P
    f.predict()
    f.set_weights(torch.arange(P, dtype=torch.int64, device=DEV))
    f.step()
    assert f.last_velocity is None
    with pytest.raises(ValueError):
        f.reset((1.0, 2.0, 1.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        ParticleFilter(P, INIT, MS, SR, 321, DEV, motion_model="brownian")
    with pytest.raises(ValueError):
        ParticleFilter(P, INIT, MS, SR, 321, DEV, motion_model="constant_velocity", velocity_max=0.0)


# ------------------------------------------------------------------ several ranks (gloo on one GPU)
MR_FRAMES = 4


def _mr_run(f, P):
    """Four frames of injected weights (the same global arrays on every rank, this rank's slice injected)."""
    rng = np.random.default_rng(17)
    out = []
    for k in range(1, MR_FRAMES + 1):
        L = _injected(P, k, rng)
        f.predict()
        f.set_weights(torch.from_numpy(L[f.begin:f.begin + f.n_local].copy()).to(DEV))
        est = f.step()
        out.append({"est": est, "vel": f.last_velocity, "flag": f.last_resampled, "state": _state5(f),
                    "anc": f.last_ancestors.cpu().numpy().copy()})
    return out


def _mr_worker(rank, world, port, P, kw, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _mr_run(_pf(P, 321, rank=rank, world_size=world, **kw), P)))
    except Exception as e:  # report instead of hanging the parent
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("world,P,kw", [(2, 64, {}), (3, 10, {"resample_method": R10.STRATIFIED, "ess_threshold": 0.5})])
def test_sharded_filter_equals_single_rank(world, P, kw):
    """World 2 (P = 64, equal shards) and world 3 (P = 10: shards 3 / 3 / 4, the five-row chunks compacted after the
    gather; stratified with a gate, so skipped frames occur): every rank's slots hold the single-rank filter's five rows
    and ancestors bit for bit, and every rank reports its estimate and velocity estimate bits."""
    from vitparticlefiltertracker_amd.particle_filter import shard_range
    single = _mr_run(_pf(P, 321, **kw), P)
    if kw:
        assert {g["flag"] for g in single} == {True, False}
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mr_worker, args=(r, world, port, P, kw, q)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        out = dict(q.get(timeout=240) for _ in procs)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert not isinstance(out[r], str), out[r]
        b, n = shard_range(P, world, r)
        for k, (got, ref) in enumerate(zip(out[r], single), start=1):
            tag = f"rank {r} frame {k}"
            assert got["est"] == ref["est"] and got["vel"] == ref["vel"] and got["flag"] == ref["flag"], tag
            assert np.array_equal(got["anc"], ref["anc"][b:b + n]), f"{tag}: ancestors"
            assert np.array_equal(bits(got["state"]), bits(ref["state"][:, b:b + n])), f"{tag}: state"


# ------------------------------------------------------------------ Tracker / MultiTracker (ViT-Ti, fp32)
P_T, BOX, SEED = 64, (80, 80, 64, 64), 99
T_CV = {"motion_model": "constant_velocity", "velocity_std": [1.0, 0.5], "velocity_decay": 0.9, "velocity_max": 6.0}


def _cfg(cv=True, seed=SEED, **over):
    from vitparticlefiltertracker_amd import load_config
    return load_config({"model": {"arch": "vit_tiny_patch16_224", "dtype": "fp32", "weights": {"seed": 3}},
                        "particles": {"num": P_T, "seed": seed, **(T_CV if cv else {}), **over}})


def _record(tr, est):
    return {"est": est, "vel": tr.last_velocity, "state": _state5(tr.pf),
            "anc": tr.pf.last_ancestors.cpu().numpy().copy()}


def _same(a, b, tag):
    assert a["est"] == b["est"] and a["vel"] == b["vel"], tag
    assert np.array_equal(a["anc"], b["anc"]), f"{tag}: ancestors"
    assert np.array_equal(bits(a["state"]), bits(b["state"])), f"{tag}: state"


@pytest.fixture(scope="module")
def clip():
    from vitparticlefiltertracker_amd.frames import synthetic_clip
    return synthetic_clip(7)


@pytest.fixture(scope="module")
def tracked(clip):
    """The uninterrupted six-frame constant-velocity run through track() that the tests here compare against."""
    from vitparticlefiltertracker_amd import Tracker
    tr = Tracker(_cfg(), device=DEV)
    tr.init(clip[0], BOX)
    return [_record(tr, tr.track(f)) for f in clip[1:]]


def test_tracker_frames_equal_the_reference(clip, tracked):
    """Four frames step by step: the predicted state is the reference's predict, and from the weights the forward
    produced the resampled five rows and the ancestors are the reference's; the estimates to 1e-12; and track() of the
    same frames returns what estimate() gives here."""
    from vitparticlefiltertracker_amd import Tracker
    tr = Tracker(_cfg(), device=DEV)
    tr.init(clip[0], BOX)
    assert tr.last_velocity is None
    c = _cfg()["particles"]
    cx, cy = BOX[0] + 0.5 * BOX[2], BOX[1] + 0.5 * BOX[3]
    ref = R.Filter(P_T, (cx, cy, 1.0), c["motion_std"], c["scale_range"], SEED, HW, K40, c["velocity_std"],
                   c["velocity_decay"], c["velocity_max"])
    for k, f in enumerate(clip[1:5], start=1):
        tr._upload(f)
        tr.frame_index += 1
        tr.pf.predict(tr.frame_index)
        ref.predict(k)
        tr.weigh()
        Q = tr.pf.Q.cpu().numpy().copy()
        assert np.array_equal(bits(_state5(tr.pf)), bits(ref.state)), f"frame {k}: predicted state"
        est = tr.pf.estimate()
        vel = tr.last_velocity
        anc = tr.pf.resample().cpu().numpy()
        r = ref.update(Q)
        assert np.array_equal(anc, r["anc"]), f"frame {k}: ancestors"
        assert np.array_equal(bits(_state5(tr.pf)), bits(r["state"])), f"frame {k}: resampled state"
        np.testing.assert_allclose(est, R10.estimate(r, P_T), rtol=1e-12)
        np.testing.assert_allclose(vel, R.velocity(r, P_T), rtol=1e-12)
        _same(_record(tr, est), tracked[k - 1], f"frame {k} against track()")


def test_multitracker_targets_equal_their_own_trackers(clip):
    from vitparticlefiltertracker_amd import MultiTracker, Tracker
    boxes = [BOX, (60, 70, 48, 56)]
    mt = MultiTracker(_cfg(), n_objects=2, device=DEV)
    mt.init(clip[0], boxes)
    trs = [Tracker(_cfg(seed=SEED + k), device=DEV) for k in range(2)]
    for tr, bx in zip(trs, boxes):
        tr.init(clip[0], bx)
    for i, f in enumerate(clip[1:5], start=1):
        ests = mt.track(f)
        for k, tr in enumerate(trs):
            assert tr.track(f) == ests[k], f"frame {i} target {k}"
            assert mt.last_velocity[k] == tr.last_velocity and tr.last_velocity is not None, f"frame {i} target {k}"
            assert np.array_equal(bits(_state5(mt.pfs[k])), bits(_state5(tr.pf))), f"frame {i} target {k}"
            assert torch.equal(mt.pfs[k].last_ancestors, tr.pf.last_ancestors)
    sd = mt.state_dict()
    assert sd["velocity_soa"].shape == (2, 2, P_T) and sd["particles_soa"].shape == (2, 3, P_T)
    mt2 = MultiTracker(_cfg(), n_objects=2, device=DEV)
    mt2.load_state_dict(sd)
    assert mt2.track(clip[5]) == mt.track(clip[5]) and mt2.last_velocity == mt.last_velocity
    for a, b in zip(mt.pfs, mt2.pfs):
        assert np.array_equal(bits(_state5(a)), bits(_state5(b)))


# ------------------------------------------------------------------ checkpoints
FINGERPRINT_KEYS = {"arch", "dtype", "weights_seed", "weights_crc32", "mean", "std", "P", "motion_std", "scale_range",
                    "seed", "lambda", "weight_bits", "template_update", "rank", "world_size"}
STATE_KEYS = {"format", "frame_index", "pf_frame", "particles_soa", "template", "box_wh", "frame_hw", "config"}


def test_checkpoint_resumes_bit_exact_and_the_models_refuse_each_other(tmp_path, clip, tracked):
    from vitparticlefiltertracker_amd import Tracker
    a = Tracker(_cfg(), device=DEV)
    a.init(clip[0], BOX)
    for f in clip[1:4]:
        a.track(f)
    path = a.save_checkpoint(str(tmp_path / "cv"))
    with np.load(path) as z:
        assert set(z.files) == STATE_KEYS | {"velocity_soa"}
        assert z["velocity_soa"].shape == (2, P_T) and z["particles_soa"].shape == (3, P_T)
        assert np.array_equal(bits(z["velocity_soa"]), bits(tracked[2]["state"][3:]))
    assert set(a.config_fingerprint()) == FINGERPRINT_KEYS | {"motion_model", "velocity_std", "velocity_decay",
                                                              "velocity_max"}
    b = Tracker(_cfg(), device=DEV)
    b.load_checkpoint(path)
    assert b.frame_index == 3
    for i, f in enumerate(clip[4:7], start=4):
        _same(_record(b, b.track(f)), tracked[i - 1], f"frame {i} after resume")
    # the default model, and another velocity noise, refuse the file; a default checkpoint is refused the other way
    d = Tracker(_cfg(cv=False), device=DEV)
    for other in (d, Tracker(_cfg(velocity_std=[2.0, 0.5]), device=DEV)):
        with pytest.raises(ValueError):
            other.load_checkpoint(path)
    d.init(clip[0], BOX)
    d.track(clip[1])
    assert d.last_velocity is None and d.pf.velocity_soa is None
    assert set(d.config_fingerprint()) == FINGERPRINT_KEYS and set(d.state_dict()) == STATE_KEYS
    assert d.state_dict()["particles_soa"].shape == (3, P_T)
    dpath = d.save_checkpoint(str(tmp_path / "rw"))
    with pytest.raises(ValueError):
        Tracker(_cfg(), device=DEV).load_checkpoint(dpath)
    d2 = Tracker(_cfg(cv=False), device=DEV)
    d2.load_checkpoint(dpath)
    assert d2.track(clip[2]) == d.track(clip[2])


# ------------------------------------------------------------------ main.py
def test_main_reads_the_keys_and_reports_velocity(tmp_path, capsys):
    import json
    import main as vpf_main
    head = "model: {arch: vit_tiny_patch16_224, dtype: bf16, weights: {seed: 3}}\ninput: {source: synthetic, frames: 4}\n"
    cv, rw = tmp_path / "cv.yaml", tmp_path / "rw.yaml"
    cv.write_text(head + "particles: {num: 64, seed: 99, motion_model: constant_velocity, velocity_std: [1.0, 0.5]}\n")
    rw.write_text(head + "particles: {num: 64, seed: 99}\n")
    plain, rich = tmp_path / "plain.json", tmp_path / "rich.json"
    assert vpf_main.main(["--config", str(cv), "--out", str(plain)]) == 0
    text_plain = capsys.readouterr().out
    assert vpf_main.main(["--config", str(cv), "--out", str(rich), "--velocity"]) == 0
    text_rich = capsys.readouterr().out
    a, b = json.loads(plain.read_text()), json.loads(rich.read_text())
    assert all(set(r) == {"frame", "x", "y", "scale"} for r in a) and "vx=" not in text_plain
    assert [{k: r[k] for k in ("frame", "x", "y", "scale")} for r in b] == a
    assert all(isinstance(r["vx"], float) and isinstance(r["vy"], float) for r in b)
    assert text_rich.count("vx=") == len(b) == 3 and "n/a" not in text_rich
    assert vpf_main.main(["--config", str(rw), "--velocity"]) == 0
    text_rw = capsys.readouterr().out
    assert text_rw.count("vx=    n/a") == 3 and text_rw.count("vy=    n/a") == 3
