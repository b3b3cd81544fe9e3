"""GPU (one MI355X): SPEC S16 end to end. The colour-only Tracker (likelihood.lambda = 0, ViT-Ti, P = 1024) on the jump
clip (tests/s16_reference.py: the target vanishes in frame 9 and reappears 300 px away in frame 16) reproduces
follow_jump bit for bit, so the DEVICE searches from frame 12 on, reports the anchor while the search is held and is
back on the target in the first visible frame, while the same tracker without `redetect` holds for ever; the same under
constant velocity plus an angle row; per target in a MultiTracker; a checkpoint on a held search frame; 2 and 3 ranks
over gloo; and `redetect: null` left as SPEC S15."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import s13_reference as R13
import s16_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOX = R13.FOLLOW["box"]
CV = {"motion_model": "constant_velocity", "velocity_std": [1.0, 1.0], "velocity_decay": 1.0, "velocity_max": 64.0}
ROT = {"rotation_std": 0.05, "rotation_range": [-1.0, 1.2]}
P_CV, N_CV = 256, 13                # the constant-velocity + angle run: frames 1..13, the search starts in 12
FIRST_SEARCH = R.ABSENT[0] + R.AFTER


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cfg(redetect="default", seed=R13.FOLLOW["seed"], P=R.P_RUN, drop_key=False, particles=None):
    from vitparticlefiltertracker_amd import load_config
    lk = {"lambda": 0.0, "template_update": R.ALPHA, "color": {},
          "occlusion": {"threshold": R.THETA, "noise_gain": R.GAIN, "max_hold": R.MAX_HOLD}}
    if not drop_key:
        lk["redetect"] = {"after": R.AFTER} if redetect == "default" else redetect
    return load_config({"model": {"arch": "vit_tiny_patch16_224", "dtype": "bf16", "weights": {"seed": 3}},
                        "particles": {"num": P, "seed": seed, **(particles or {})}, "likelihood": lk})


def _record(tr, est):
    return {"est": est, "state": tr.pf._state.cpu().numpy().copy(), "anc": tr.pf.last_ancestors.cpu().numpy().copy(),
            "ct": tr.color_template.cpu().numpy().copy(), "t": tr.template.cpu().numpy().copy(), "held": tr.last_held,
            "peak": tr.last_peak, "evidence": tr.last_evidence, "streak": tr.held_frames, "lost": tr.lost,
            "searched": tr.last_searched, "reacquired": tr.last_reacquired, "anchor": tr.pf.anchor,
            "vel": tr.last_velocity, "rot": tr.last_rotation}


FLAGS = ("held", "peak", "evidence", "streak", "searched", "reacquired", "anchor", "vel", "rot")


def _same(a, b, tag):
    assert a["est"] == b["est"], tag
    assert np.array_equal(a["anc"], b["anc"]) and np.array_equal(bits(a["state"]), bits(b["state"])), tag
    assert np.array_equal(bits(a["ct"]), bits(b["ct"])) and np.array_equal(bits(a["t"]), bits(b["t"])), tag
    assert tuple(a[k] for k in FLAGS) == tuple(b[k] for k in FLAGS), tag


def _track(cfg, clip, n, box=BOX, **kw):
    from vitparticlefiltertracker_amd import Tracker
    tr = Tracker(cfg, device=DEV, **kw)
    tr.init(clip[0], box)
    return tr, [_record(tr, tr.track(f)) for f in clip[1:1 + n]]


def _against_reference(got, want, k):
    """One frame of a device run against follow_jump's, bit for bit."""
    r = want["r"]
    tag = f"frame {k}"
    assert got["held"] is want["held"] and got["streak"] == want["streak"], f"{tag}: held"
    assert got["searched"] is want["searched"] and got["reacquired"] is want["reacquired"], f"{tag}: search flags"
    assert got["peak"] == want["peak"] and got["evidence"] == want["evidence"], f"{tag}: peak / evidence"
    assert got["est"] == want["returned"], f"{tag}: returned estimate"
    assert np.array_equal(got["anc"], r["anc"]), f"{tag}: ancestors"
    assert np.array_equal(bits(got["state"]), bits(r["state"])), f"{tag}: states"
    assert np.array_equal(bits(got["ct"]), bits(want["t"])), f"{tag}: colour template"


@pytest.fixture(scope="module")
def clip():
    return R.jump_clip()


@pytest.fixture(scope="module")
def reference(clip):
    return R.follow_jump(clip)


@pytest.fixture(scope="module")
def tracked(clip):
    """The uninterrupted searching run of the whole clip through track() (graph on)."""
    return _track(_cfg(), clip, R.FRAMES - 1)[1]


# ------------------------------------------------------------------ the behaviour run
def test_tracker_reproduces_the_reference_and_finds_the_target_again(clip, reference, tracked):
    """Every frame equals follow_jump's: states, ancestors, held flags, peak, returned estimate, colour template, the
    search flags. Independently, on the device's own numbers: (1) the first frame that is not held after the target
    vanished comes within 2 frames of its reappearance; (2) from 4 frames after it the estimate stays within the bound
    measured on the CPU (1.5 x the worst of three seeds, < 16 px); and while the search is held track() returns the
    anchor, the estimate of frame 11, not the frame centre."""
    assert len(tracked) == len(reference) == R.FRAMES - 1
    for k, (got, want) in enumerate(zip(tracked, reference), start=1):
        _against_reference(got, want, k)
        assert got["lost"] is False
    held = [k for k, g in enumerate(tracked, start=1) if g["held"]]
    searched = [k for k, g in enumerate(tracked, start=1) if g["searched"]]
    assert held[0] == R.ABSENT[0] and held == list(range(held[0], held[-1] + 1))
    first = held[-1] + 1
    print("device run: held", held, "searched", searched, "first not held", first)
    assert R.REAPPEAR <= first <= R.REAPPEAR + R.REACQUIRE_WITHIN
    assert searched == list(range(FIRST_SEARCH, first + 1))
    assert [k for k, g in enumerate(tracked, start=1) if g["reacquired"]] == [first]
    dist = {k: R.distance(g["est"], k) for k, g in enumerate(tracked, start=1)}
    print("device run, truth distance per frame:", {k: None if v is None else round(v, 2) for k, v in dist.items()})
    assert max(v for k, v in dist.items() if k >= first + 4) <= R.SEARCH_BOUND_PX < 16.0
    for k in range(FIRST_SEARCH, first):                        # held search frames report the anchor
        assert tracked[k - 1]["est"] == tracked[FIRST_SEARCH - 2]["est"] == tracked[k - 1]["anchor"], f"frame {k}"
        centre = tracked[k - 1]["state"][:2].astype(np.float64).mean(axis=1)
        assert np.hypot(*(centre - 223.5)) < 20.0 and np.hypot(centre[0] - tracked[k - 1]["est"][0],
                                                               centre[1] - tracked[k - 1]["est"][1]) > 100.0
        assert np.array_equal(bits(tracked[k - 1]["ct"]), bits(tracked[k - 2]["ct"])), "template moved on a held frame"
    # the search frames' clouds cover the frame; the re-acquired one has collapsed onto the target: a box farther than
    # one box side (64 px) from the target's centre does not overlap it, so the survivors span less than two sides
    assert np.ptp(tracked[FIRST_SEARCH - 1]["state"][0]) > 400.0 and np.ptp(tracked[first - 1]["state"][0]) < 128.0


def test_control_without_the_search_holds_for_ever_and_redetect_null_is_s15(clip):
    """(3) The same configuration with `redetect: null`: held in every frame from 9 on, `lost` not raised within the
    clip, and the final plain mean more than 200 px from the truth. It is SPEC S15's run, bit for bit
    (follow_jump(redetect=False) is s15_reference's recursion), and so is a configuration without the key; no S16
    output, fingerprint entry or state-dict key exists."""
    want = R.follow_jump(clip, redetect=False)
    runs = []
    for cfg in (_cfg(redetect=None), _cfg(drop_key=True)):
        tr, rec = _track(cfg, clip, R.FRAMES - 1)
        assert tr.redetect is None and tr.pf.redetect is None and tr.pf.anchor is None and tr.pf.search_after is None
        assert tr.last_searched is None and tr.last_reacquired is None
        assert "redetect" not in tr.config_fingerprint() and "anchor" not in tr.state_dict()
        runs.append((tr, rec))
    (ta, ra), (tb, rb) = runs
    assert ta.config_fingerprint() == tb.config_fingerprint() and set(ta.state_dict()) == set(tb.state_dict())
    for k, (a, b, w) in enumerate(zip(ra, rb, want), start=1):
        _same(a, b, f"frame {k}")
        _against_reference(a, w, k)
    assert [k for k, g in enumerate(ra, start=1) if g["held"]] == list(range(R.ABSENT[0], R.FRAMES))
    assert not any(g["lost"] for g in ra) and ra[-1]["streak"] == R.FRAMES - R.ABSENT[0] <= R.MAX_HOLD
    final = R.distance(ra[-1]["est"], R.FRAMES - 1)
    print("control, final distance:", round(final, 2), "at the reappearance:", round(R.distance(ra[15]["est"], 16), 2))
    assert final > R.CONTROL_MIN_PX


def test_eager_tracker_equals_the_graph(clip, tracked):
    _, eager = _track(_cfg(), clip, R.REAPPEAR + 1, use_graph=False)
    for k, (a, b) in enumerate(zip(eager, tracked), start=1):
        _same(a, b, f"frame {k}")


def test_search_under_constant_velocity_and_an_angle_row(clip):
    """constant_velocity + rotation_std, P = 256, frames 1..13 (the search starts in 12): all six state rows, the
    returned estimate, the velocity and angle estimates and the colour template equal the reference; on the search
    frames both velocity rows are +0 (every word), so the velocity estimate is (0, 0), and the angle row was
    predicted as ever."""
    cv = (CV["velocity_std"], CV["velocity_decay"], CV["velocity_max"])
    rot = (ROT["rotation_std"], ROT["rotation_range"])
    want = R.follow_jump(clip, P=P_CV, frames=N_CV, cv=cv, rot=rot)
    tr, got = _track(_cfg(P=P_CV, particles={**CV, **ROT}), clip, N_CV)
    assert tr.pf._state.shape[0] == 6
    for k, (g, w) in enumerate(zip(got, want), start=1):
        _against_reference(g, w, k)
        assert g["vel"] == w["r"]["extras"][:2] and g["rot"] == w["r"]["extras"][2], f"frame {k}: velocity / angle"
    assert [k for k, g in enumerate(got, start=1) if g["searched"]] == [FIRST_SEARCH, FIRST_SEARCH + 1]
    for k in (FIRST_SEARCH, FIRST_SEARCH + 1):
        assert not bits(got[k - 1]["state"][3:5]).any() and got[k - 1]["vel"] == (0.0, 0.0), f"frame {k}"
        assert np.array_equal(bits(got[k - 1]["state"][5]), bits(want[k - 1]["pred"][5]))
        assert not np.array_equal(bits(got[k - 1]["state"][5]), bits(got[k - 2]["state"][5]))
    assert bits(got[FIRST_SEARCH - 2]["state"][3:5]).any()


# ------------------------------------------------------------------ MultiTracker
def test_multitracker_searches_per_target(clip, tracked):
    """Two targets; target 0 is the one that jumps, target 1 sits on the static background. Target 0 equals the single
    tracker's searching run, target 1 its own single-target run (seed + 1), and it never searches."""
    from vitparticlefiltertracker_amd import MultiTracker
    box1, n = (8, 8, 48, 48), R.REAPPEAR + 2
    mt = MultiTracker(_cfg(), n_objects=2, device=DEV)
    mt.init(clip[0], [BOX, box1])
    _, solo = _track(_cfg(seed=R13.FOLLOW["seed"] + 1), clip, n, box=box1)
    for k in range(1, n + 1):
        ests = mt.track(clip[k])
        for t, want in ((0, tracked[k - 1]), (1, solo[k - 1])):
            tag = f"frame {k} target {t}"
            assert ests[t] == want["est"], tag
            assert np.array_equal(bits(mt.pfs[t]._state.cpu().numpy()), bits(want["state"])), tag
            assert np.array_equal(bits(mt.color_templates[t].cpu().numpy()), bits(want["ct"])), tag
            assert (mt.last_held[t], mt.last_peak[t], mt.held_frames[t], mt.last_searched[t], mt.last_reacquired[t]) == \
                (want["held"], want["peak"], want["streak"], want["searched"], want["reacquired"]), tag
            assert mt.pfs[t].anchor == want["anchor"], tag
        assert mt.last_searched == [FIRST_SEARCH <= k <= R.REAPPEAR, False], f"frame {k}"
        assert mt.last_held[1] is False
    sd = mt.state_dict()
    assert sd["anchor"].shape == (2, 3) and sd["anchor"].dtype == np.float64
    mt2 = MultiTracker(_cfg(), n_objects=2, device=DEV)
    mt2.load_state_dict(sd)
    assert [pf.anchor for pf in mt2.pfs] == [pf.anchor for pf in mt.pfs]
    assert mt2.track(clip[n + 1]) == mt.track(clip[n + 1])


# ------------------------------------------------------------------ checkpoint
def test_checkpoint_on_a_held_search_frame_resumes_bit_exact(tmp_path, clip, tracked):
    from vitparticlefiltertracker_amd import Tracker
    a, rec = _track(_cfg(), clip, FIRST_SEARCH + 1)             # frames 12, 13: searched and held
    assert a.last_searched is True and a.last_held is True and a.held_frames == R.AFTER + 2
    path = a.save_checkpoint(str(tmp_path / "search"))
    with np.load(path) as z:
        assert "anchor" in z.files and z["anchor"].dtype == np.float64
        assert tuple(z["anchor"].tolist()) == tracked[FIRST_SEARCH - 2]["est"] == rec[-1]["est"]
    assert a.config_fingerprint()["redetect"] == {"after": R.AFTER, "threshold": None}
    b = Tracker(_cfg(), device=DEV)
    b.load_checkpoint(path)
    assert b.frame_index == FIRST_SEARCH + 1 and b.held_frames == R.AFTER + 2 and b.pf.anchor == a.pf.anchor
    for k in range(FIRST_SEARCH + 2, R.REAPPEAR + 4):           # two more held search frames, then the recovery
        _same(_record(b, b.track(clip[k])), tracked[k - 1], f"frame {k} after resume")
    plain = Tracker(_cfg(redetect=None), device=DEV)
    for other in (plain, Tracker(_cfg(redetect={"after": R.AFTER + 1}), device=DEV),
                  Tracker(_cfg(redetect={"after": R.AFTER, "threshold": 0.1}), device=DEV)):
        with pytest.raises(ValueError, match="redetect"):
            other.load_checkpoint(path)
    plain.init(clip[0], BOX)
    plain.track(clip[1])
    ppath = plain.save_checkpoint(str(tmp_path / "plain"))
    with pytest.raises(ValueError, match="redetect"):
        Tracker(_cfg(), device=DEV).load_checkpoint(ppath)


def test_search_threshold_of_its_own_gates_only_the_search_frames(clip, tracked):
    """theta_r = 1.0 (no frame's peak reaches 2^K... unless a weight is exactly 1): every search frame is held, the
    visible ones included, so the search goes on; the frames before the first search frame equal the default run's."""
    _, rec = _track(_cfg(redetect={"after": R.AFTER, "threshold": 1.0}), clip, R.REAPPEAR + 2)
    for k in range(1, FIRST_SEARCH):
        _same(rec[k - 1], tracked[k - 1], f"frame {k}")
    assert all(g["searched"] and g["held"] for g in rec[FIRST_SEARCH - 1:])
    assert all(g["peak"] < 1.0 for g in rec[FIRST_SEARCH - 1:])
    assert rec[R.REAPPEAR - 1]["peak"] > R.THETA            # the target is in view, only theta_r keeps the frame held
    assert all(g["est"] == tracked[FIRST_SEARCH - 2]["est"] for g in rec[FIRST_SEARCH - 1:])


# ------------------------------------------------------------------ 2 and 3 ranks sharing the GPU over gloo
N_RANKED = R.REAPPEAR + 2


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, clip, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vitparticlefiltertracker_amd import Tracker
        tr = Tracker(_cfg(), device=DEV, rank=rank, world_size=world)
        tr.init(clip[0], BOX)
        q.put((rank, [_record(tr, tr.track(f)) for f in clip[1:1 + N_RANKED]]))
    except Exception as e:  # report instead of hanging the parent
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_equal_the_single_rank_run(world, clip, tracked):
    """2 ranks (equal shards) and 3 ranks (1024 = 341 + 341 + 342: the compacted gather) share cuda:0 and exchange
    through gloo, through the hold, the search and the re-acquisition (frames 1..18): each rank scatters its own shard
    from global indices, so its states are the single-rank run's shard, and its estimate, anchor, streak and flags are
    that run's bits."""
    from vitparticlefiltertracker_amd.particle_filter import shard_range
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, clip[:N_RANKED + 1], q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        out = dict(q.get(timeout=240) for _ in procs)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    for r in range(world):
        assert not isinstance(out[r], str), out[r]
        b, n = shard_range(R.P_RUN, world, r)
        for k, (got, want) in enumerate(zip(out[r], tracked), start=1):
            tag = f"rank {r} frame {k}"
            assert got["est"] == want["est"], tag
            assert tuple(got[f] for f in FLAGS) == tuple(want[f] for f in FLAGS), tag
            assert np.array_equal(got["anc"], want["anc"][b:b + n]), tag
            assert np.array_equal(bits(got["state"]), bits(want["state"][:, b:b + n])), tag
            assert np.array_equal(bits(got["ct"]), bits(want["ct"])) and np.array_equal(bits(got["t"]), bits(want["t"]))
    assert [g["searched"] for g in out[0]] == [FIRST_SEARCH <= k <= R.REAPPEAR for k in range(1, N_RANKED + 1)]
