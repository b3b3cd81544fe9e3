"""GPU (MI355X): SPEC S18, the patch-token cue, through ViTEngine, Tracker and MultiTracker (ViT-Ti unless said).

The cue reads rows 1 .. N-1 of `engine.h` after `encoder`: the last block updates the CLS rows only, so they hold the
residual stream that entered it. The stage test pins that against the oracle in all three dtypes; the rest runs the
tracker: self-score, fp32 parity with the reference tracker (tests/token_reference.py), following the stock clip, the
default path untouched, graph = eager, MultiTracker = Trackers, checkpoint / resume, held frames, two ranks."""
import os

import numpy as np
import pytest
import torch

import token_reference as R
from oracle import pf
from test_gpu_multirank import _free_port, _run as _rank_run     # the multi-rank launcher's pieces, as they are
from vitparticlefiltertracker_amd.config import ARCHS, load_config
from vitparticlefiltertracker_amd.frames import synthetic_clip
from vitparticlefiltertracker_amd.weights import make_vit_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TI, SM = "vit_tiny_patch16_224", "vit_small_patch16_224"
BOX = (80, 80, 64, 64)
K = 40
# the fp32 feature bar of tests/test_gpu_vit_tracker.py::test_vit_features_vs_oracle: rtol 1e-4, atol 1e-4 max|ref|
FP32_RTOL = 1e-4


def _cfg(P=64, dtype="bf16", tokens={}, alpha=0.0, arch=TI, drop_key=False, lam=20.0, **lk):
    c = {"model": {"arch": arch, "dtype": dtype, "weights": {"seed": 0}}, "particles": {"num": P, "seed": 1234},
         "likelihood": {"lambda": lam, "weight_bits": K, "template_update": alpha, "tokens": tokens, **lk}}
    if drop_key:
        del c["likelihood"]["tokens"]
    return load_config(c)


@pytest.fixture(scope="module")
def clip():
    return synthetic_clip(9)


def _frame(tr, f):
    """One frame in pieces: (Q before the resample, estimates)."""
    tr._upload(f)
    tr.frame_index += 1
    for p in tr.pfs:
        p.height, p.width = int(f.shape[0]), int(f.shape[1])
        p.predict(tr.frame_index)
    tr.weigh()
    Qs = [p.Q.cpu().numpy().copy() for p in tr.pfs]
    return Qs, tr._step()


# ------------------------------------------------------------------ stage: the patch rows survive the last block
@pytest.mark.parametrize("name,dtype", [(TI, "fp32"), (TI, "bf16"), (SM, "fp8")])
def test_patch_rows_after_the_encoder_are_the_last_blocks_input(name, dtype):
    from vitparticlefiltertracker_amd.vit import ViTEngine
    arch = ARCHS[name]
    w = make_vit_weights(arch, seed=4, perturb_affine=True)
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)
    p = np.array([[60.0, 112.5, 170.25], [100.0, 90.5, 141.0], [0.8, 1.0, 1.5]], np.float32)
    eng = ViTEngine(arch, w, dtype, DEV, 3)
    n = eng.embed_many(torch.from_numpy(frame).to(DEV), [torch.from_numpy(p).to(DEV)], [(64.0, 64.0)])
    eng.encoder(n)
    got = eng.h[:3, 1:].double().cpu()
    ref = R.token_rows(frame, p, (64.0, 64.0), w, arch).double()
    assert got.shape == ref.shape == (3, arch.tokens - 1, arch.dim)
    if dtype == "fp32":
        torch.testing.assert_close(got, ref, rtol=FP32_RTOL, atol=FP32_RTOL * ref.abs().max().item())
    else:
        cos = torch.nn.functional.cosine_similarity(got, ref, dim=2)
        print(name, dtype, "min row cosine", cos.min().item())
        assert cos.min().item() >= (0.999 if dtype == "bf16" else 0.99), cos.min()


# ------------------------------------------------------------------ self-score
@pytest.mark.parametrize("name,dtype", [(TI, "fp32"), (TI, "bf16"), (SM, "fp8")])
def test_the_init_crop_scores_one_on_every_token(name, dtype, clip):
    """One particle at exactly the init state on frame 0: the same crop and the same rows as the template's (a crop's
    features do not depend on the batch), so every sim_pj >= 1 - 2e-6."""
    from vitparticlefiltertracker_amd import Tracker
    tr = Tracker(_cfg(8, dtype, arch=name), device=DEV)
    tr.init(clip[0], BOX)
    arch = ARCHS[name]
    assert tr.token_template.shape == (arch.tokens - 1, arch.dim) and tr.token_template.dtype == torch.float32
    torch.testing.assert_close(tr.token_template.norm(dim=1), torch.ones(arch.tokens - 1, device=DEV), rtol=0, atol=1e-6)
    one = torch.tensor([[112.0], [112.0], [1.0]], device=DEV)
    eng = tr.engine
    n = eng.embed_many(tr._frame_dev, [one], [tr.box_wh])
    eng.encoder(n)
    ts = torch.empty(1, arch.tokens - 1, device=DEV)
    sim = torch.empty(1, device=DEV)
    Q = torch.empty(1, device=DEV, dtype=torch.int64)
    torch.ops.vpf.token_weight(eng.h[:1], eng.ng, eng.nb, arch.ln_eps, tr.token_template, 20.0, K, False, Q, None, ts, sim)
    assert ts.min().item() >= 1 - 2e-6, ts.min().item()
    assert sim.item() >= 1 - 2e-6 and Q.item() >= pf.weights_to_Q(np.array([1 - 2e-6], np.float32), 20.0, K)[0]


# ------------------------------------------------------------------ fp32 parity with the reference tracker, one frame
def test_fp32_frame_matches_the_reference_tracker(clip):
    from vitparticlefiltertracker_amd import Tracker
    cfg = _cfg(64, "fp32")
    arch = ARCHS[TI]
    w = make_vit_weights(arch, seed=0)
    tr = Tracker(cfg, device=DEV, weights=w)
    ot = R.TokenOracleTracker(cfg, w, arch)
    tr.init(clip[0], BOX)
    ot.init(clip[0], BOX)
    tt = torch.from_numpy(ot.token_template).double()
    torch.testing.assert_close(tr.token_template.double().cpu(), tt, rtol=FP32_RTOL, atol=FP32_RTOL * tt.abs().max().item())
    (Q,), (est,) = _frame(tr, clip[1])
    e_ref = ot.track(clip[1])
    sim = tr.last_token_sim.cpu().numpy()
    ref = ot.last_token_sim
    print("token sim: device", sim[:4], "reference", ref[:4], "max err", np.abs(sim - ref).max())
    np.testing.assert_allclose(sim, ref, rtol=FP32_RTOL, atol=FP32_RTOL * np.abs(ref).max())
    Lv = pf.weights_to_Q(tr.engine.sim[:64].cpu().numpy(), 20.0, K)
    Lt = pf.weights_to_Q(sim, 20.0, K)
    assert np.array_equal(Q, R.combine_Q(Lv, Lt, K))
    np.testing.assert_allclose(np.array(est), np.array(e_ref), rtol=1e-4)


# ------------------------------------------------------------------ following
def test_bf16_tracker_follows_the_stock_clip(clip):
    """The configuration of the CPU follow test (tests/test_token_host.py): ViT-Ti weights seed 0, P = 256, seed 1234,
    lambda = lambda_t = 20, K = 40; within 2 px of the truth on each of the 8 frames (the reference stays <= 0.54)."""
    from vitparticlefiltertracker_amd import Tracker
    on, s = R.follow(Tracker(_cfg(256), device=DEV), clip)
    off, _ = R.follow(Tracker(_cfg(256, tokens=None), device=DEV), clip)
    print("tokens: {}  :", [round(d, 3) for d in on], "scale", s)
    print("tokens: null:", [round(d, 3) for d in off])
    assert len(on) == 8 and max(on) <= 2.0, on


# ------------------------------------------------------------------ off means off
def test_null_is_the_unconfigured_tracker(clip):
    from vitparticlefiltertracker_amd import Tracker
    from vitparticlefiltertracker_amd.vit import KernelTimer
    names, recs = [], []
    for cfg in (_cfg(tokens=None), _cfg(drop_key=True), _cfg()):
        tr = Tracker(cfg, device=DEV, use_graph=False)
        tr.init(clip[0], BOX)
        tr.engine.timer = KernelTimer()
        (Q,), (est,) = _frame(tr, clip[1])
        names.append([n for n, _, _ in tr.engine.timer.pending])
        tr.engine.timer.summary()
        tr.engine.timer = None
        recs.append((Q, est, tr))
    assert "token_weight" not in names[0] and names[0] == names[1]
    i = names[2].index("cls_weight")
    assert names[2][i + 1] == "token_weight" and names[2][:i + 1] + names[2][i + 2:] == names[0]
    assert np.array_equal(recs[0][0], recs[1][0]) and recs[0][1] == recs[1][1]
    for _, _, tr in recs[:2]:
        assert tr.tokens is None and tr.token_template is None and tr.last_token_sim is None
        assert "tokens" not in tr.config_fingerprint() and "token_template" not in tr.state_dict()
    assert recs[0][2].config_fingerprint() == recs[1][2].config_fingerprint()
    assert set(recs[0][2].state_dict()) == set(recs[1][2].state_dict())
    on = recs[2][2]
    assert on.config_fingerprint()["tokens"] == {"lambda": 20.0} and "token_template" in on.state_dict()
    assert on.last_token_sim.shape == (64,)
    on.init(clip[0], BOX)                               # no frame weighed yet: nothing to report
    assert on.last_token_sim is None


def test_lambda_zero_leaves_the_tokens_as_the_only_vit_cue(clip):
    from vitparticlefiltertracker_amd import Tracker
    tr = Tracker(_cfg(lam=0.0), device=DEV)
    tr.init(clip[0], BOX)
    (Q,), _ = _frame(tr, clip[1])
    assert np.array_equal(Q, pf.weights_to_Q(tr.last_token_sim.cpu().numpy(), 20.0, K))


# ------------------------------------------------------------------ graph replay = eager
def test_graph_replay_equals_eager(clip):
    from vitparticlefiltertracker_amd import Tracker
    runs = []
    for use_graph in (True, False):
        tr = Tracker(_cfg(alpha=0.1), device=DEV, use_graph=use_graph)
        tr.init(clip[0], BOX)
        runs.append([_frame(tr, f) for f in clip[1:4]] + [tr.token_template.cpu().numpy()])
    for (Qg, eg), (Qe, ee) in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(Qg[0], Qe[0]) and eg == ee
    assert np.array_equal(runs[0][3], runs[1][3])


# ------------------------------------------------------------------ MultiTracker
def test_multitracker_targets_equal_single_trackers(clip):
    from vitparticlefiltertracker_amd import MultiTracker, Tracker
    boxes = [BOX, (40, 50, 48, 48)]
    mt = MultiTracker(_cfg(alpha=0.1), n_objects=2, device=DEV)
    mt.init(clip[0], boxes)
    assert len(mt.token_templates) == 2 and not torch.equal(mt.token_templates[0], mt.token_templates[1])
    multi = [_frame(mt, f) for f in clip[1:3]]
    for k, box in enumerate(boxes):
        cfg = _cfg(alpha=0.1)
        cfg["particles"]["seed"] += k
        tr = Tracker(cfg, device=DEV)
        tr.init(clip[0], box)
        for i, f in enumerate(clip[1:3]):
            (Q,), (est,) = _frame(tr, f)
            assert np.array_equal(Q, multi[i][0][k]), f"target {k} frame {i + 1}: Q"
            assert est == multi[i][1][k], f"target {k} frame {i + 1}: estimate"
        assert torch.equal(tr.pf.particles_soa, mt.pfs[k].particles_soa)
        assert torch.equal(tr.token_template, mt.token_templates[k])
        assert torch.equal(tr.last_token_sim, mt.last_token_sim[k])
    assert MultiTracker(_cfg(tokens=None), n_objects=2, device=DEV).token_templates is None


# ------------------------------------------------------------------ checkpoint
def test_checkpoint_resumes_bit_exact_and_the_kinds_refuse_each_other(tmp_path, clip):
    from vitparticlefiltertracker_amd import Tracker

    def run(tr, frames):
        return [(tr.track(f), tr.pf.particles_soa.cpu().numpy().copy(), tr.token_template.cpu().numpy().copy())
                for f in frames]
    a = Tracker(_cfg(alpha=0.1), device=DEV)
    a.init(clip[0], BOX)
    t0 = a.token_template.clone()
    run(a, clip[1:3])
    assert not torch.equal(a.token_template, t0), "alpha > 0 updates the token template"
    path = a.save_checkpoint(str(tmp_path / "tok"))
    with np.load(path) as z:
        assert z["token_template"].shape == (196, 192) and z["token_template"].dtype == np.float32
    ref = run(a, clip[3:5])
    b = Tracker(_cfg(alpha=0.1), device=DEV)
    b.load_checkpoint(path)
    assert b.last_token_sim is None
    got = run(b, clip[3:5])
    assert b.last_token_sim is not None
    for k, (r, g) in enumerate(zip(ref, got), start=3):
        assert r[0] == g[0], f"frame {k}: estimate"
        assert np.array_equal(r[1].view(np.uint32), g[1].view(np.uint32)), f"frame {k}: particles"
        assert np.array_equal(r[2].view(np.uint32), g[2].view(np.uint32)), f"frame {k}: token_template"
    plain = Tracker(_cfg(alpha=0.1, tokens=None), device=DEV)
    with pytest.raises(ValueError, match="tokens"):
        plain.load_checkpoint(path)
    plain.init(clip[0], BOX)
    plain.track(clip[1])
    ppath = plain.save_checkpoint(str(tmp_path / "plain"))
    with pytest.raises(ValueError, match="tokens"):
        Tracker(_cfg(alpha=0.1), device=DEV).load_checkpoint(ppath)
    # alpha = 0 leaves the bits untouched
    c = Tracker(_cfg(), device=DEV)
    c.init(clip[0], BOX)
    t0 = c.token_template.clone()
    c.track(clip[1])
    assert torch.equal(c.token_template, t0)


# ------------------------------------------------------------------ held frame
def test_a_held_frame_keeps_the_token_template(clip):
    """With the occlusion gate (SPEC S15) a frame without the target is held and leaves token_template's bits unchanged;
    the next frame with the target updates it again. The token cue's weights are far smaller than the CLS cue's (a
    particle half a pixel off scores exp(-10)), so the gate's threshold is placed for them: on the CPU reference
    (P = 256) the peak likelihood of the clip's frames is >= 6e-5 and that of the noise frame 4.8e-9; 5e-7 lies two
    orders from either."""
    from vitparticlefiltertracker_amd import Tracker
    tr = Tracker(_cfg(256, alpha=0.1, occlusion={"threshold": 5e-7}), device=DEV)
    tr.init(clip[0], BOX)
    tr.track(clip[1])
    assert tr.last_held is False
    t1 = tr.token_template.clone()
    noise = np.random.default_rng(1).integers(0, 256, clip[0].shape, dtype=np.uint8)
    tr.track(noise)
    assert tr.last_held is True and torch.equal(tr.token_template, t1)
    tr.track(clip[2])
    assert tr.last_held is False and not torch.equal(tr.token_template, t1)


# ------------------------------------------------------------------ two ranks over gloo on one GPU
def _tok_worker(rank, world, port, P, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vitparticlefiltertracker_amd import Tracker
        tr = Tracker(_cfg(P), device="cuda:0", rank=rank, world_size=world)
        q.put((rank, _rank_run(tr, synthetic_clip(3))))
    except Exception as e:  # report instead of hanging the parent
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_the_single_rank_run():
    import torch.multiprocessing as mp
    from vitparticlefiltertracker_amd import Tracker
    from vitparticlefiltertracker_amd.particle_filter import shard_range
    world, P = 2, 64
    ref = _rank_run(Tracker(_cfg(P), device="cuda:0"), synthetic_clip(3))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tok_worker, args=(r, world, port, P, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        assert not isinstance(out[r], str), out[r]
        b, n = shard_range(P, world, r)
        for k, ((est, anc, parts), (est1, anc1, parts1)) in enumerate(zip(out[r], ref), start=1):
            assert est == est1, f"rank {r} frame {k}: estimate {est} vs single rank {est1}"
            assert np.array_equal(anc, anc1[b:b + n]), f"rank {r} frame {k}: ancestors"
            assert np.array_equal(parts.view(np.uint32), parts1[:, b:b + n].view(np.uint32)), f"rank {r} frame {k}"
