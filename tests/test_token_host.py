"""CPU: SPEC S18 (patch-token likelihood) — the `likelihood.tokens` key and every rejection, `tokens: null` leaving the
fingerprint and a checkpoint's key set as they were, the exact-case generators being fair (every fp32 summation order
gives the same bits, so bit equality is a fair bar for the kernel), and the reason the cue exists, on the reference alone:
the CPU oracle filter follows the stock synthetic clip with the token cue and does not with the CLS cue."""
import types

import numpy as np
import pytest

import token_reference as R
from vitparticlefiltertracker_amd import config as C

ARCH = "vit_tiny_patch16_224"


# ------------------------------------------------------------------ config
def test_tokens_key_accepted_forms():
    assert C.load_config()["likelihood"]["tokens"] is None
    assert C.DEFAULTS["likelihood"]["tokens"] is None
    assert C.load_config({"likelihood": {"tokens": None}})["likelihood"]["tokens"] is None
    assert C.load_config({"likelihood": {"tokens": {}}})["likelihood"]["tokens"] == {"lambda": 20.0}
    for lam, want in ((0, 0.0), (0.0, 0.0), (7, 7.0), (12.5, 12.5), (1e30, 1e30)):
        got = C.load_config({"likelihood": {"tokens": {"lambda": lam}}})["likelihood"]["tokens"]
        assert got == {"lambda": want} and type(got["lambda"]) is float
    assert C.check_tokens(None) is None and C.check_tokens({}) == {"lambda": 20.0}


@pytest.mark.parametrize("bad", [True, False, 0, 20.0, "on", [], [20.0], {"lam": 1.0}, {"lambda": 1.0, "mask": None},
                                 {"lambda": True}, {"lambda": False}, {"lambda": "20"}, {"lambda": None},
                                 {"lambda": [1.0]}, {"lambda": -1e-9}, {"lambda": -1}, {"lambda": float("nan")},
                                 {"lambda": float("inf")}, {"lambda": -float("inf")}, {1: 2.0}])
def test_tokens_key_rejected_forms(bad):
    with pytest.raises(ValueError, match="likelihood.tokens"):
        C.load_config({"likelihood": {"tokens": bad}})


def test_tokens_combine_with_every_other_key():
    c = C.load_config({"particles": {"motion_model": "constant_velocity", "rotation_std": 0.01},
                       "likelihood": {"lambda": 0, "tokens": {"lambda": 5}, "color": {}, "color_surround": {},
                                      "occlusion": {}, "redetect": {}, "template_update": 0.1},
                       "estimate": {"method": "mode"}, "resample": {"method": "stratified"}})
    assert c["likelihood"]["tokens"] == {"lambda": 5.0} and c["likelihood"]["lambda"] == 0
    c = C.load_config({"likelihood": {"tokens": {}}, "resample": {"ess_threshold": 0.5}})
    assert c["likelihood"]["tokens"] == {"lambda": 20.0}


def test_null_leaves_the_fingerprint_and_the_two_kinds_refuse_each_other():
    import json
    from vitparticlefiltertracker_amd import tracker as T
    base = T._fingerprint(C.load_config(), ARCH, "00000000", 0, 1)
    assert "tokens" not in base
    assert T._fingerprint(C.load_config({"likelihood": {"tokens": None}}), ARCH, "00000000", 0, 1) == base
    legacy = C.load_config()
    del legacy["likelihood"]["tokens"]              # a configuration dict from before the key existed
    assert T._fingerprint(legacy, ARCH, "00000000", 0, 1) == base
    assert json.dumps(T._fingerprint(legacy, ARCH, "00000000", 0, 1), sort_keys=True) == json.dumps(base, sort_keys=True)
    on = T._fingerprint(C.load_config({"likelihood": {"tokens": {}}}), ARCH, "00000000", 0, 1)
    assert set(on) - set(base) == {"tokens"} and on["tokens"] == {"lambda": 20.0}
    assert {k: on[k] for k in base} == base
    other = T._fingerprint(C.load_config({"likelihood": {"tokens": {"lambda": 5}}}), ARCH, "00000000", 0, 1)

    def sd(fp):
        return {"format": np.int64(T.CHECKPOINT_FORMAT), "config": np.array(json.dumps(fp, sort_keys=True))}
    T._check_fingerprint(sd(on), on)
    T._check_fingerprint(sd(base), base)
    for saved, mine in ((on, base), (base, on), (on, other)):
        with pytest.raises(ValueError, match="tokens"):
            T._check_fingerprint(sd(saved), mine)


def test_checkpoint_key_set_gains_token_template_only_with_the_cue():
    import torch
    from vitparticlefiltertracker_amd import tracker as T
    pf = types.SimpleNamespace(frame=2, particles_soa=torch.zeros(3, 4), height=8, width=8, ess_threshold=None,
                               velocity_soa=None, rotation_soa=None, held_frames=0, anchor=None)

    def stub(**kw):
        return types.SimpleNamespace(pf=pf, frame_index=2, template=torch.zeros(4), box_wh=(4.0, 4.0), color=None,
                                     color_template=None, occlusion=None, redetect=None, estimate=None,
                                     config_fingerprint=lambda: {}, **kw)
    absent = T.Tracker.state_dict(stub())                               # a tracker from before the key existed
    null = T.Tracker.state_dict(stub(tokens=None, token_template=None))
    assert set(null) == set(absent) and "token_template" not in null
    tt = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    on = T.Tracker.state_dict(stub(tokens={"lambda": 20.0}, token_template=tt))
    assert set(on) - set(absent) == {"token_template"}
    assert on["token_template"].dtype == np.float32 and np.array_equal(on["token_template"], tt.numpy())
    assert "token_template" in T._PER_TARGET


# ------------------------------------------------------------------ the exact cases are fair
ORDERS = ("seq", "rev", "pair", "lanes")


@pytest.mark.parametrize("n,N,D,m", [(3, 5, 768, 1), (2, 197, 192, 2), (2, 2, 4, 1), (3, 3, 260, 2), (2, 4, 1024, 3)])
def test_exact_case_has_one_fp32_value_under_every_summation_order(n, N, D, m):
    tok, T, sim, sim_p = R.exact_case(n, N, D, seed=N + D, m=m)
    assert np.all(tok[:, 0] == np.float32(1e30))
    assert np.array_equal(R.bf16_round(tok[:, 1:]), tok[:, 1:]), "the rows are exact in bf16 too"
    assert len({T[j].tobytes() for j in range(N - 1)}) == N - 1, "distinct template rows"
    got = [R.eval_f32(tok, T, o) for o in ORDERS]
    for s, sp in got:
        assert np.array_equal(s.view(np.uint32), sim.astype(np.float32).view(np.uint32))
        assert np.array_equal(sp.view(np.uint32), sim_p.view(np.uint32))
    assert np.array_equal(sim.astype(np.float32).astype(np.float64), sim)
    # and the fp64 reference agrees: the values are exact, not merely order-independent
    _, s64, sp64 = R.sims_ref(tok[:, 1:], T)
    assert np.array_equal(s64, sim)
    np.testing.assert_allclose(sp64, sim_p, rtol=2.0 ** -23)
    # routing: pairing token row j with another template row changes the value
    if N > 2:
        swapped, _ = R.eval_f32(tok, np.roll(T, 1, axis=0), "seq")
        assert not np.array_equal(swapped, sim.astype(np.float32))


@pytest.mark.parametrize("n,N,D", [(3, 5, 256), (2, 3, 1024), (2, 4, 16)])
def test_exact_ln_case_normalises_to_signs(n, N, D):
    tok, T, sim, sim_p = R.exact_ln_case(n, N, D, seed=D)
    rows = tok[:, 1:].astype(np.float64)
    assert np.all(rows.mean(-1) == 0) and np.all(rows.var(-1) == rows[..., 0] ** 2)
    g, s64, _ = R.sims_ref(tok[:, 1:], T, np.ones(D), np.zeros(D), eps=0.0)
    assert np.array_equal(np.abs(g), np.ones_like(g))
    assert np.array_equal(s64, sim)
    signs = np.sign(tok).astype(np.float32)
    signs[:, 0] = 1e30
    for o in ORDERS:
        s, sp = R.eval_f32(signs, T, o)
        assert np.array_equal(s.view(np.uint32), sim.astype(np.float32).view(np.uint32))
        assert np.array_equal(sp.view(np.uint32), sim_p.view(np.uint32))


def test_weight_of_the_exact_cases_is_exact():
    """A token equal to its template row: sim 1, Lt = 2^K; S5's form otherwise (oracle weights_to_Q)."""
    from oracle import pf
    assert pf.weights_to_Q(np.array([1.0, 1.5, np.nan, np.inf, -np.inf], np.float32), 20.0, 40).tolist() == \
        [2 ** 40, 2 ** 40, 0, 0, 0]
    assert R.combine_Q([2 ** 40, 12345, 0], [2 ** 40, 2 ** 39, 2 ** 40], 40).tolist() == [2 ** 40, 6172, 0]


# ------------------------------------------------------------------ following, on the reference alone
@pytest.fixture(scope="module")
def follow_runs():
    from vitparticlefiltertracker_amd.config import ARCHS
    from vitparticlefiltertracker_amd.frames import synthetic_clip
    from vitparticlefiltertracker_amd.weights import make_vit_weights
    from oracle.tracker import OracleTracker
    arch = ARCHS[ARCH]
    w = make_vit_weights(arch, seed=0)
    clip = synthetic_clip(9)
    base = {"model": {"arch": ARCH, "weights": {"seed": 0}}, "particles": {"num": 256, "seed": 1234},
            "likelihood": {"lambda": 20.0, "weight_bits": 40}}
    tok = R.follow(R.TokenOracleTracker(C.load_config({**base, "likelihood": {**base["likelihood"], "tokens": {}}}),
                                        w, arch), clip)
    cls = R.follow(OracleTracker(C.load_config(base), w, arch), clip)
    return tok, cls


def test_reference_filter_follows_with_the_token_cue_and_not_with_cls(follow_runs):
    """Stock synthetic_clip(9) (target moving (2, 1) px per frame), ViT-Ti weights seed 0, P = 256, seed 1234,
    lambda = lambda_t = 20, K = 40. Measured on the oracle: the token tracker stays within 0.54 px on every frame; a
    filter that does not follow is 17.9 px off by frame 8 (the target's own travel) and the CLS-only filter 18.7."""
    (tok, s_tok), (cls, _) = follow_runs
    print("token cue:", [round(d, 3) for d in tok], "scale", s_tok)
    print("CLS only :", [round(d, 3) for d in cls])
    assert len(tok) == 8 and max(tok) <= 2.0, tok
    assert cls[-1] > 10.0, cls
