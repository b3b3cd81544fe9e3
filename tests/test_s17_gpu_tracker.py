"""GPU (one MI355X): SPEC S17 end to end. ParticleFilter with a bimodal posterior (the mode equals the reference, the mean
is kept, the resample is a mean filter's); the colour-only Tracker on the twin clip (tests/s17_reference.py: the jump
clip with a second identical copy of the target from the reappearance on) reproduces follow_twin bit for bit, returns
an estimate inside the window of a copy from the first frame that is not held, while SPEC S6's mean of that frame lies
on the background between the copies; 2 ranks over gloo; per target in a MultiTracker; a checkpoint mid-run; and
`estimate: null` left as SPEC S16."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import s13_reference as R13
import s15_reference as R15
import s16_reference as R16
import s17_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOX = R13.FOLLOW["box"]
f32 = np.float32
FIRST_SEARCH = R16.ABSENT[0] + R16.AFTER
N_SHORT = R16.REAPPEAR + 3          # frames 1..19: the hold, the search, the re-acquisition and three bimodal frames


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cfg(estimate="mode", seed=R13.FOLLOW["seed"], P=R16.P_RUN, drop_key=False, alpha=R16.ALPHA):
    from vitparticlefiltertracker_amd import load_config
    cfg = {"model": {"arch": "vit_tiny_patch16_224", "dtype": "bf16", "weights": {"seed": 3}},
           "particles": {"num": P, "seed": seed},
           "likelihood": {"lambda": 0.0, "template_update": alpha, "color": {}, "redetect": {"after": R16.AFTER},
                          "occlusion": {"threshold": R16.THETA, "noise_gain": R16.GAIN, "max_hold": R16.MAX_HOLD}}}
    if not drop_key:
        cfg["estimate"] = {"method": "mode", "window": R.OMEGA} if estimate == "mode" else estimate
    return load_config(cfg)


def _record(tr, est):
    return {"est": est, "state": tr.pf._state.cpu().numpy().copy(), "anc": tr.pf.last_ancestors.cpu().numpy().copy(),
            "ct": tr.color_template.cpu().numpy().copy(), "t": tr.template.cpu().numpy().copy(), "held": tr.last_held,
            "peak": tr.last_peak, "evidence": tr.last_evidence, "streak": tr.held_frames,
            "searched": tr.last_searched, "reacquired": tr.last_reacquired, "anchor": tr.pf.anchor,
            "mean": tr.last_mean, "mass": tr.last_mode_mass, "index": tr.last_mode_index}


FLAGS = ("held", "peak", "evidence", "streak", "searched", "reacquired", "anchor", "mean", "mass", "index")


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
    r = want["r"]
    tag = f"frame {k}"
    assert got["held"] is want["held"] and got["streak"] == want["streak"], f"{tag}: held"
    assert got["searched"] is want["searched"] and got["reacquired"] is want["reacquired"], f"{tag}: search flags"
    assert got["peak"] == want["peak"] and got["evidence"] == want["evidence"], f"{tag}: peak / evidence"
    assert got["est"] == want["returned"], f"{tag}: returned estimate"
    assert got["mean"] == want["mean"] and got["mass"] == want["mass"] and got["index"] == want["index"], f"{tag}: mode"
    assert np.array_equal(got["anc"], r["anc"]), f"{tag}: ancestors"
    assert np.array_equal(bits(got["state"]), bits(r["state"])), f"{tag}: states"
    assert np.array_equal(bits(got["ct"]), bits(want["t"])), f"{tag}: colour template"


@pytest.fixture(scope="module")
def clip():
    return R.twin_clip()


@pytest.fixture(scope="module")
def reference(clip):
    return R.follow_twin(clip, True)


@pytest.fixture(scope="module")
def tracked(clip):
    """The uninterrupted mode-reporting run of the whole clip through track() (graph on)."""
    return _track(_cfg(), clip, R16.FRAMES - 1)[1]


# ------------------------------------------------------------------ ParticleFilter
def _bimodal(P, rows, seed=0):
    rng = np.random.default_rng(seed)
    st = np.empty((rows, P), np.float32)
    heavy = np.arange(P) % 3 == 0                   # a third of the particles at b carry most of the weight
    a, b = (60.0, 70.0), (160.0, 150.0)
    st[0] = np.where(heavy, b[0], a[0]) + rng.normal(0, 3, P)
    st[1] = np.where(heavy, b[1], a[1]) + rng.normal(0, 3, P)
    st[2] = rng.uniform(0.8, 1.2, P)
    st[3:] = rng.normal(0, 1, (rows - 3, P))
    # the heavy third holds about 0.6 of the weight: the mean lies 0.4 of the way from b to a, outside both windows
    Q = np.where(heavy, rng.integers(1 << 39, 1 << 40, P), rng.integers(1 << 37, 3 << 37, P)).astype(np.int64)
    return Q, st, a, b


@pytest.mark.parametrize("kw,rows", [({}, 3), ({"motion_model": "constant_velocity", "rotation_std": 0.05}, 6),
                                     ({"resample_method": "stratified", "ess_threshold": 0.5}, 3),
                                     ({"occlusion_threshold": 0.5}, 3), ({"occlusion_threshold": 1.0}, 3)])
def test_filter_reports_the_mode_keeps_the_mean_and_resamples_as_a_mean_filter(kw, rows):
    """set_weights with a bimodal Q (P = 1000: the tree's tail): estimate() equals the reference's mode, last_mean
    SPEC S6's mean, the extra rows' estimates are the window's; the states, ancestors and statistics after step() are a
    mode_window=None filter's, bit for bit. occlusion_threshold 1.0 holds the frame: every weight counts as 1."""
    from vitparticlefiltertracker_amd.particle_filter import ParticleFilter
    P, hx, hy = 1000, f32(16.0), f32(12.0)
    Q, st, a, b = _bimodal(P, rows)
    made = []
    for window in ((float(hx), float(hy)), None):
        pf = ParticleFilter(P, (0.0,) * rows, seed=9, device=DEV, frame_size=(224, 224), mode_window=window, **kw)
        pf._state.copy_(torch.from_numpy(st))
        pf.frame = 5
        pf.set_weights(torch.from_numpy(Q).to(DEV))
        made.append(pf)
    mode, mean = made
    held = kw.get("occlusion_threshold") == 1.0
    uniform = held
    # a first frame's carry is the identity: the posterior weights are Q itself
    ref = R.mode(Q, st, hx, hy, uniform)
    T = int(Q.sum())
    tree = R15.tree_sums([1] * P if uniform else Q, st)
    d = float(P) if uniform else float(T)
    want_mean = tuple(s / d for s in tree[:3])
    est_mean = mean.estimate()
    est = mode.estimate()
    assert est_mean == want_mean == mode.last_mean and mean.last_mean is None and mean.last_mode_index is None
    assert est == ref["est"][:3] and mode.last_mode_index == ref["i"] and mode.last_mode_mass == ref["Tm"] / d
    assert mode.last_held is (held if "occlusion_threshold" in kw else None)
    if not uniform:
        assert abs(est[0] - b[0]) <= hx and abs(est[1] - b[1]) <= hy and mode.last_mode_mass > 0.5
        for c in (a, b):
            assert abs(want_mean[0] - c[0]) > hx and abs(want_mean[1] - c[1]) > hy
    if rows == 6:
        assert mode.last_velocity == ref["est"][3:5] and mode.last_rotation == ref["est"][5]
        assert mean.last_velocity == tuple(s / d for s in tree[3:5]) and mean.last_rotation == tree[5] / d
    assert mode.step() == est and mean.step() == est_mean
    assert torch.equal(mode.last_ancestors, mean.last_ancestors)
    assert np.array_equal(bits(mode._state.cpu().numpy()), bits(mean._state.cpu().numpy()))
    assert torch.equal(mode._stats_pin[:mode._mstats], mean._stats_pin)
    assert mode.last_ess == mean.last_ess and mode.last_resampled == mean.last_resampled
    if mode.carry is not None:
        assert torch.equal(mode.carry, mean.carry)
    # the next frame, from the resampled cloud: T == 0 (no weights set) counts every particle once
    for pf in made:
        pf.predict()
    st2 = mode._state.cpu().numpy()
    assert np.array_equal(bits(st2), bits(mean._state.cpu().numpy()))
    if "ess_threshold" not in kw:       # (under the ESS gate the posterior is the carry times zero: also T == 0)
        r2 = R.mode(None, st2, hx, hy, True)
        assert mode.estimate() == r2["est"][:3] and mode.last_mode_mass == r2["Tm"] / float(P)
        assert mode.last_mean == mean.estimate()


def test_window_can_be_changed_but_not_added():
    from vitparticlefiltertracker_amd.particle_filter import ParticleFilter
    P = 300
    Q, st, _, _ = _bimodal(P, 3, seed=2)
    pf = ParticleFilter(P, (0.0, 0.0, 1.0), device=DEV, mode_window=(4.0, 4.0))
    pf._state.copy_(torch.from_numpy(st))
    for w in ((4.0, 4.0), (20.0, 0.5)):
        pf.set_mode_window(w)
        pf.set_weights(torch.from_numpy(Q).to(DEV))
        assert pf.estimate() == R.mode(Q, st, f32(w[0]), f32(w[1]), False)["est"]
    with pytest.raises(ValueError, match="mode_window"):
        pf.set_mode_window(None)
    with pytest.raises(ValueError, match="mode_window"):
        ParticleFilter(P, (0.0, 0.0, 1.0), device=DEV).set_mode_window((1.0, 1.0))


# ------------------------------------------------------------------ the behaviour run
def test_tracker_reproduces_the_reference_and_reports_a_copy_not_the_background(clip, reference, tracked):
    """Every frame equals follow_twin's: states, ancestors, flags, the returned estimate, the mean, the mass, i*, the
    colour template (which learnt the returned estimate). On the device's own numbers: from the first frame that is not
    held on, the estimate lies inside the window of the nearer copy's centre, and within the bound measured on the CPU
    (1.5 x the worst of three seeds, < 16 px); that first frame's SPEC S6 mean lies farther than 2 max(hx, hy) from both
    copies; held search frames return the anchor."""
    assert len(tracked) == len(reference) == R16.FRAMES - 1
    for k, (got, want) in enumerate(zip(tracked, reference), start=1):
        _against_reference(got, want, k)
    hx, hy = R.window(R.OMEGA, BOX[2:])
    held = [k for k, g in enumerate(tracked, start=1) if g["held"]]
    first = held[-1] + 1
    assert first == R.FIRST and held == list(range(R16.ABSENT[0], first))
    off = {k: R.offsets(g["est"], k) for k, g in enumerate(tracked, start=1) if k >= first}
    print("device run: nearer copy and distance per frame", {k: (o[1], round(o[0][2], 2)) for k, o in off.items()})
    print("device run: mode mass per frame", {k: round(g["mass"], 3) for k, g in enumerate(tracked, start=1)})
    for k, (o, _) in off.items():
        assert o[0] <= hx and o[1] <= hy, f"frame {k}: the estimate left the window of both copies"
        assert o[2] <= R.MODE_BOUND_PX < 16.0, f"frame {k}"
    mean = tracked[first - 1]["mean"]
    dist = [float(np.hypot(mean[0] - c[0], mean[1] - c[1])) for c in R.copies(first)]
    print("device run: SPEC S6 mean of frame", first, mean, "distances", dist)
    assert min(dist) > 2.0 * max(hx, hy)
    assert tracked[first - 1]["mass"] < 0.75                     # the diagnostic says so: weight lies elsewhere
    assert all(g["mass"] > 0.9 for g in tracked[:R16.ABSENT[0] - 1])     # one hump while the target is followed
    for k in range(FIRST_SEARCH, first):
        assert tracked[k - 1]["est"] == tracked[FIRST_SEARCH - 2]["est"] == tracked[k - 1]["anchor"], f"frame {k}"
        assert tracked[k - 1]["mean"] != tracked[k - 1]["est"]


def test_estimate_null_is_the_mean_tracker_bit_for_bit(clip):
    """`estimate: null`, `estimate: {method: mean}` and no key at all: SPEC S16's run (s16_reference's recursion on the
    twin clip, follow_twin(report_mode=False)), no S17 output, fingerprint entry or launch: the statistics buffer has
    its old size and no density workspace exists."""
    want = R.follow_twin(clip, False, frames=N_SHORT)
    runs = []
    for cfg in (_cfg(estimate=None), _cfg(estimate={"method": "mean", "window": 0.25}), _cfg(drop_key=True)):
        tr, rec = _track(cfg, clip, N_SHORT)
        assert tr.estimate is None and tr.pf.mode_window is None and not hasattr(tr.pf, "_dens")
        assert tr.pf._stats_dev.numel() == 8 and "estimate" not in tr.config_fingerprint()
        assert tr.last_mean is None and tr.last_mode_index is None and tr.last_mode_mass is None
        runs.append((tr, rec))
    for k in range(1, N_SHORT + 1):
        for _, rec in runs[1:]:
            _same(rec[k - 1], runs[0][1][k - 1], f"frame {k}")
        got, w = runs[0][1][k - 1], want[k - 1]
        assert got["est"] == w["returned"] and np.array_equal(got["anc"], w["r"]["anc"]), f"frame {k}"
        assert np.array_equal(bits(got["state"]), bits(w["r"]["state"])), f"frame {k}"
        assert np.array_equal(bits(got["ct"]), bits(w["t"])), f"frame {k}"
    assert set(runs[0][0].state_dict()) == set(runs[2][0].state_dict())


def test_fixed_template_mode_tracker_resamples_as_the_mean_tracker(clip):
    """template_update = 0: nothing follows the report, so the mode tracker's states and ancestors are the mean
    tracker's in every frame, and its last_mean is what that tracker returns (a held search frame aside: the anchor)."""
    _, a = _track(_cfg(alpha=0.0), clip, N_SHORT)
    _, b = _track(_cfg(estimate=None, alpha=0.0), clip, N_SHORT)
    differ = 0
    for k, (m, n) in enumerate(zip(a, b), start=1):
        assert np.array_equal(m["anc"], n["anc"]) and np.array_equal(bits(m["state"]), bits(n["state"])), f"frame {k}"
        assert (m["held"], m["peak"], m["searched"]) == (n["held"], n["peak"], n["searched"]), f"frame {k}"
        if not (m["searched"] and m["held"]):
            assert m["mean"] == n["est"], f"frame {k}"
        differ += m["est"] != n["est"]
    assert differ >= 3


def test_eager_tracker_equals_the_graph(clip, tracked):
    _, eager = _track(_cfg(), clip, N_SHORT, use_graph=False)
    for k, (a, b) in enumerate(zip(eager, tracked), start=1):
        _same(a, b, f"frame {k}")


# ------------------------------------------------------------------ MultiTracker
def test_multitracker_equals_two_trackers(clip, tracked):
    """K = 2: target 0 is the twin clip's, target 1 a smaller box on the static background with its own window (omega x
    its own box). Each equals its single tracker (seed + k), per-target outputs included."""
    from vitparticlefiltertracker_amd import MultiTracker
    box1, n = (8, 8, 48, 40), R16.REAPPEAR + 2
    mt = MultiTracker(_cfg(), n_objects=2, device=DEV)
    mt.init(clip[0], [BOX, box1])
    assert mt.pfs[0].mode_window == (32.0, 32.0) and mt.pfs[1].mode_window == (24.0, 20.0)
    _, solo = _track(_cfg(seed=R13.FOLLOW["seed"] + 1), clip, n, box=box1)
    for k in range(1, n + 1):
        ests = mt.track(clip[k])
        for t, want in ((0, tracked[k - 1]), (1, solo[k - 1])):
            tag = f"frame {k} target {t}"
            assert ests[t] == want["est"], tag
            assert np.array_equal(bits(mt.pfs[t]._state.cpu().numpy()), bits(want["state"])), tag
            assert np.array_equal(bits(mt.color_templates[t].cpu().numpy()), bits(want["ct"])), tag
            assert (mt.last_mean[t], mt.last_mode_mass[t], mt.last_mode_index[t], mt.last_held[t]) == \
                (want["mean"], want["mass"], want["index"], want["held"]), tag
            assert mt.pfs[t].anchor == want["anchor"], tag
    sd = mt.state_dict()
    mt2 = MultiTracker(_cfg(), n_objects=2, device=DEV)
    mt2.load_state_dict(sd)
    assert [pf.mode_window for pf in mt2.pfs] == [pf.mode_window for pf in mt.pfs]
    assert mt2.track(clip[n + 1]) == mt.track(clip[n + 1]) and mt2.last_mean == mt.last_mean


# ------------------------------------------------------------------ checkpoint
def test_checkpoint_mid_run_resumes_bit_exact(tmp_path, clip, tracked):
    from vitparticlefiltertracker_amd import Tracker
    a, _ = _track(_cfg(), clip, R16.REAPPEAR)                   # saved on the first bimodal frame
    path = a.save_checkpoint(str(tmp_path / "mode"))
    with np.load(path) as z:
        keys = set(z.files)
    assert a.config_fingerprint()["estimate"] == {"method": "mode", "window": R.OMEGA}
    b = Tracker(_cfg(), device=DEV)
    b.load_checkpoint(path)
    assert b.pf.mode_window == a.pf.mode_window == (32.0, 32.0) and b.pf.anchor == a.pf.anchor
    for k in range(R16.REAPPEAR + 1, R16.REAPPEAR + 4):
        _same(_record(b, b.track(clip[k])), tracked[k - 1], f"frame {k} after resume")
    plain = Tracker(_cfg(estimate=None), device=DEV)
    wide = Tracker(_cfg(estimate={"method": "mode", "window": 0.75}), device=DEV)
    for other in (plain, wide):
        with pytest.raises(ValueError, match="estimate"):
            other.load_checkpoint(path)
    plain.init(clip[0], BOX)
    plain.track(clip[1])
    ppath = plain.save_checkpoint(str(tmp_path / "plain"))
    with np.load(ppath) as z:
        assert set(z.files) == keys, "the mode estimate adds no state"
    with pytest.raises(ValueError, match="estimate"):
        Tracker(_cfg(), device=DEV).load_checkpoint(ppath)


# ------------------------------------------------------------------ 2 ranks sharing the GPU over gloo
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
        q.put((rank, [_record(tr, tr.track(f)) for f in clip[1:1 + N_SHORT]]))
    except Exception as e:  # report instead of hanging the parent
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_the_single_rank_run(clip, tracked):
    """2 ranks (equal shards: the two-shard global view, the layout one rank never sees) share cuda:0 and exchange
    through gloo: each computes the whole density on its gathered view, so its estimate, mean, mass and i* are the
    single-rank run's bits, and its states that run's shard."""
    world = 2
    from vitparticlefiltertracker_amd.particle_filter import shard_range
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, clip[:N_SHORT + 1], q)) for r in range(world)]
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
        b, n = shard_range(R16.P_RUN, world, r)
        for k, (got, want) in enumerate(zip(out[r], tracked), start=1):
            tag = f"rank {r} frame {k}"
            assert got["est"] == want["est"], tag
            assert tuple(got[f] for f in FLAGS) == tuple(want[f] for f in FLAGS), tag
            assert np.array_equal(got["anc"], want["anc"][b:b + n]), tag
            assert np.array_equal(bits(got["state"]), bits(want["state"][:, b:b + n])), tag
            assert np.array_equal(bits(got["ct"]), bits(want["ct"])), tag
