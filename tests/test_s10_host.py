"""CPU: SPEC S10 (adaptive resampling) — the config keys, the library's new exports, and the Python-int reference
(tests/s10_reference.py) checked by hand on tiny cases. No compute calls (no GPU here)."""
import ctypes
import os

import numpy as np
import pytest

import s10_reference as R
from vitparticlefiltertracker_amd import config as C


def test_config_accepts_stratified_and_a_threshold(tmp_path):
    d = C.load_config()
    assert d["resample"] == {"method": "systematic", "ess_threshold": None}
    d = C.load_config({"resample": {"method": "stratified", "ess_threshold": 0.5}})
    assert d["resample"] == {"method": "stratified", "ess_threshold": 0.5}
    assert C.load_config({"resample": {"ess_threshold": 1}})["resample"]["ess_threshold"] == 1
    p = tmp_path / "c.yaml"
    p.write_text("resample: {method: stratified, ess_threshold: 0.25}\n")
    assert C.load_config(str(p))["resample"] == {"method": "stratified", "ess_threshold": 0.25}


@pytest.mark.parametrize("tau", [0, 1.5, "x", -0.5, float("nan"), True])
def test_config_rejects_bad_thresholds(tau):
    with pytest.raises(ValueError):
        C.load_config({"resample": {"ess_threshold": tau}})


@pytest.mark.parametrize("method", ["residual", "multinomial", "", None])
def test_config_rejects_other_methods(method):
    with pytest.raises(ValueError):
        C.load_config({"resample": {"method": method}})


def test_libvpf_exports_the_s10_entry_points():
    from vitparticlefiltertracker_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vpf_weight_prior", "vpf_estimate_resample_ex"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES


def test_c_abi_rejects_bad_s10_arguments_before_any_launch():
    from vitparticlefiltertracker_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    fake = 4096                                          # never dereferenced: validation fails first
    assert L.vpf_weight_prior(fake, fake, -1, 40, None) == -1
    assert L.vpf_weight_prior(fake, fake, 8, 62, None) == -1
    ex = L.vpf_estimate_resample_ex

    def call(P=16, method=0, tau=0.5, bits=40):
        return ex(fake, 8, fake, 8, 24, 8, P, 1, 1, 0, 8, fake, fake, 8, fake, fake, method, tau, bits, fake, None)
    assert call(P=0) == -1 and call(P=17) == -1                 # vpf_estimate_resample's own checks
    assert call(method=2) == -1 and call(method=-1) == -1
    assert call(tau=0.0) == -1 and call(tau=1.5) == -1 and call(tau=float("nan")) == -1
    assert call(bits=62) == -1 and call(bits=-1) == -1


def test_reference_ess_by_hand():
    for P in (1, 7, 1000):
        assert R.ess([1 << 40] * P) == float(P)            # all equal: T^2 / (P q^2) = P, exactly
        assert R.ess([5] * P) == float(P)
        one = [0] * P
        one[P // 2] = 12345
        assert R.ess(one) == 1.0
    assert R.ess([0, 0, 0]) == 0.0
    assert R.ess([3, 1]) == 16.0 / 10.0
    # the gate: T == 0 and a disabled gate resample; all-equal weights skip at any tau <= 1
    assert R.gate([0, 0], 2, 0.5) and R.gate([7, 7], 2, None)
    assert not R.gate([7, 7], 2, 1.0) and not R.gate([7, 7], 2, 0.5)
    assert R.gate([7, 0], 2, 0.75) and not R.gate([7, 0], 2, 0.5)


@pytest.mark.parametrize("K", [1, 40, 51, 61])
def test_reference_identity_carry_keeps_the_likelihood(K):
    rng = np.random.default_rng(K)
    L = [0, 1, 1 << K, (1 << K) - 1] + [int(v) for v in rng.integers(0, (1 << K) + 1, 50)]
    assert R.weight_prior(L, [R.identity(K)] * len(L), K) == L
    # a carry of 2^K halves (floor), a carry of 1 leaves nothing of a weight <= 2^K
    assert R.weight_prior(L, [1 << K] * len(L), K) == [v >> 1 for v in L]
    assert R.weight_prior(L, [1] * len(L), K) == [0] * len(L)


@pytest.mark.parametrize("P,T", [(1, 5), (7, 3), (100, 1 << 46), (1000, (1 << 50) + 12345), (33, 33)])
def test_reference_stratified_positions(P, T):
    for frame in (1, 2):
        pos = R.positions(T, P, 99, frame, R.STRATIFIED)
        assert all(a <= b for a, b in zip(pos, pos[1:]))
        for j, p in enumerate(pos):
            assert j * T <= p * P + (P - 1) and p * P <= (j + 1) * T, (j, p)   # jT/P - 1 < p <= (j+1)T/P
            assert 0 <= p < T
    # the per-slot words differ from slot to slot and from the systematic word
    ws = {R.word(99, 1, j, R.STRATIFIED) for j in range(16)}
    assert len(ws) == 16 and R.word(99, 1, 0, R.SYSTEMATIC) not in ws


def test_reference_skip_carry_is_normalised_to_the_top_bit():
    K = 40
    st = np.zeros((3, 4), np.float32)
    r = R.step([1 << 30, 3 << 28, 1, 0], st, 1, 1, R.SYSTEMATIC, 0.01, K)
    assert not r["resampled"] and list(r["anc"]) == [0, 1, 2, 3]
    assert list(r["carry"]) == [1 << 40, 3 << 38, 1 << 10, 0] and 1 << K <= max(r["carry"]) < 1 << (K + 1)
    r = R.step([0, 0, 0, 0], st, 1, 1, R.STRATIFIED, 0.01, K)
    assert r["resampled"] and list(r["carry"]) == [R.identity(K)] * 4 and r["ess"] == 0.0
    assert list(r["anc"]) == [0, 1, 2, 3]                       # uniform fallback: pos_j = j + floor(u_j / P) = j
