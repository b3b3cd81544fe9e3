"""GPU (MI355X): the SPEC S10 kernels (vpf_weight_prior, vpf_estimate_resample_ex) and the ParticleFilter's adaptive
path, bit for bit against the Python-int reference (tests/s10_reference.py). Run: python -m pytest tests -m gpu."""
import numpy as np
import pytest
import torch

import s10_reference as R
from oracle import pf as opf

pytestmark = pytest.mark.gpu

DEV = "cuda"
K40 = 40
METHODS = {R.SYSTEMATIC: 0, R.STRATIFIED: 1}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()
    assert torch.cuda.is_available()


def vpf():
    return torch.ops.vpf


@pytest.mark.parametrize("K,n", [(40, 1000), (51, 1000), (40, 257), (51, 1)])
def test_weight_prior_equals_python_ints(K, n):
    """Q = (L * C) >> (K + 1) from the 128-bit product: L over [0, 2^K] with both ends, carries over [0, 2^(K+1)] with
    the identity, 2^K and 1 — products from 0 up to 2^(2K+1) (103 bits at K = 51), so both the hi and the lo word
    feed the shifted result."""
    rng = np.random.default_rng(K + n)
    L = rng.integers(0, (1 << K) + 1, n, dtype=np.int64)
    Cy = rng.integers(0, (1 << (K + 1)) + 1, n, dtype=np.int64)
    edge_l = [0, 1 << K, (1 << K) - 1, 1, 1 << K, 1 << K, 1 << K, 0, 12345]
    edge_c = [R.identity(K), R.identity(K), R.identity(K), R.identity(K), 1 << K, 1, R.identity(K) - 1, 0, 1]
    m = min(n, len(edge_l))
    L[:m], Cy[:m] = edge_l[:m], edge_c[:m]
    Q = torch.from_numpy(L.copy()).to(DEV)
    vpf().weight_prior_(Q, torch.from_numpy(Cy).to(DEV), K)
    ref = R.weight_prior(L, Cy, K)
    assert Q.cpu().tolist() == ref
    assert max(ref) <= 1 << K


def _weights(kind: str, P: int, rng) -> np.ndarray:
    Q = np.zeros(P, np.int64)
    if kind == "random":        # up to 2^40: the squares' low words overflow, so lo -> hi carries occur
        Q = rng.integers(0, (1 << 40) + 1, P, dtype=np.int64)
    elif kind == "full":        # S2 = P * 2^80 lives in the hi word alone; ess == P, skipped at any tau <= 1
        Q[:] = 1 << 40
    elif kind == "onehot":
        Q[P // 3] = 12345
    elif kind == "two":
        Q[P // 3] = (1 << 40) - 7
        Q[(2 * P) // 3] = 3 << 20
    else:
        assert kind == "zero"
    return Q


def _run_ex(view, P, seed, frame, b, n, method, tau, K):
    anc = torch.full((n,), -1, device=DEV, dtype=torch.int32)
    st = torch.empty(3, n, device=DEV)
    cdf = torch.empty(P, device=DEV, dtype=torch.int64)
    stats = torch.full((8,), -1, device=DEV, dtype=torch.int64)
    carry = torch.full((n,), -1, device=DEV, dtype=torch.int64)
    vpf().estimate_resample_ex(*view, P, seed, frame, b, b + n, anc, st, cdf, stats, METHODS[method],
                               -1.0 if tau is None else tau, K, carry)
    return anc.cpu().numpy(), st.cpu().numpy(), cdf.cpu().numpy(), stats.cpu(), carry.cpu().numpy()


@pytest.mark.parametrize("kind", ["random", "full", "onehot", "zero", "two"])
@pytest.mark.parametrize("P", [1, 33, 1000, 4097, 5000])
def test_estimate_resample_ex_equals_reference(P, kind):
    """P: one particle; a ragged wave; just under one 1024 stride; the 4096-element scan chunk crossed (4097, 5000).
    For both schemes, the gate disabled / 0.5 / 1.0 and G in {1, 2} gathered shard chunks (where 2 divides P): anc,
    states, carry_out, T, the ess bits, the flag and m equal the reference bit for bit, the sums to 1e-12."""
    from vitparticlefiltertracker_amd.particle_filter import chunk_words, global_view, shard_views
    rng = np.random.default_rng(1000 * P + len(kind))
    Q = _weights(kind, P, rng)
    p = rng.uniform(0, 224, (3, P)).astype(np.float32)
    seed, frame = (1 << 40) + 17 * P, 9
    views = {}
    for G in (1, 2):
        if P % G:
            continue
        n = P // G
        cw = chunk_words(n)
        allc = torch.zeros(G * cw, dtype=torch.int32)
        for r in range(G):
            Qv, pv = shard_views(allc[r * cw:(r + 1) * cw], n)
            Qv.copy_(torch.from_numpy(Q[r * n:(r + 1) * n].copy()))
            pv.copy_(torch.from_numpy(p[:, r * n:(r + 1) * n].copy()))
        views[G] = global_view(allc.to(DEV), G, n)
    flags = set()
    for method in (R.SYSTEMATIC, R.STRATIFIED):
        for tau in (None, 0.5, 1.0):
            ref = R.step(Q, p, seed, frame, method, tau, K40)
            flags.add(ref["resampled"])
            for G, view in views.items():
                n = P // G
                for r in range(G):
                    b = r * n
                    anc, st, cdf, stats, carry = _run_ex(view, P, seed, frame, b, n, method, tau, K40)
                    tag = f"{method} tau={tau} G={G} shard {r}"
                    assert np.array_equal(anc, ref["anc"][b:b + n]), tag
                    assert np.array_equal(st.view(np.uint32), ref["states"][:, b:b + n].view(np.uint32)), tag
                    assert np.array_equal(carry, ref["carry"][b:b + n]), tag
                    assert int(stats[0]) == ref["T"], tag
                    assert int(stats[4]) == R.f64_bits(ref["ess"]), (tag, stats[4:5].view(torch.float64), ref["ess"])
                    assert int(stats[5]) == int(ref["resampled"]) and int(stats[6]) == ref["m"], tag
                    assert int(stats[7]) == 0
                    np.testing.assert_allclose(stats[1:4].view(torch.float64).numpy(), ref["sums"], rtol=1e-12)
                    assert np.array_equal(cdf, np.cumsum(Q)), tag
    if kind == "full":
        assert flags == {True, False}          # ess == P: skipped under both thresholds, resampled without a gate
    if kind in ("onehot", "zero"):
        assert flags == ({True} if P > 1 or kind == "zero" else {True, False})


@pytest.mark.parametrize("P,kind", [(1, "random"), (1000, "random"), (4097, "zero"), (5000, "two"), (5000, "random")])
def test_ex_without_gate_equals_estimate_resample(P, kind):
    """Systematic with the gate disabled: anc, states, cdf and stats_out[0..3] are vpf_estimate_resample's bits."""
    rng = np.random.default_rng(P)
    Q = _weights(kind, P, rng)
    p = rng.uniform(0, 224, (3, P)).astype(np.float32)
    Qd, pd = torch.from_numpy(Q).to(DEV), torch.from_numpy(p).to(DEV)
    view = (Qd, P, pd.view(-1), P, 3 * P, P)
    seed, frame = 77, 3
    anc0 = torch.empty(P, device=DEV, dtype=torch.int32)
    st0 = torch.empty(3, P, device=DEV)
    cdf0 = torch.empty(P, device=DEV, dtype=torch.int64)
    stats0 = torch.empty(4, device=DEV, dtype=torch.int64)
    vpf().estimate_resample(*view, P, seed, frame, 0, P, anc0, st0, cdf0, stats0)
    anc, st, cdf, stats, carry = _run_ex(view, P, seed, frame, 0, P, R.SYSTEMATIC, None, K40)
    assert np.array_equal(anc, anc0.cpu().numpy())
    assert np.array_equal(st.view(np.uint32), st0.cpu().numpy().view(np.uint32))
    assert np.array_equal(cdf, cdf0.cpu().numpy())
    assert torch.equal(stats[:4], stats0.cpu())
    assert int(stats[5]) == 1 and np.array_equal(carry, np.full(P, R.identity(K40)))


def test_stratified_counts_are_within_two_of_expectation():
    """Each stratum holds one position, so n_i differs from P Q_i / T by less than 2 (systematic: less than 1)."""
    P = 5000
    rng = np.random.default_rng(11)
    Q = rng.integers(0, (1 << 40) + 1, P, dtype=np.int64)
    Q[rng.random(P) < 0.5] >>= 12
    p = np.zeros((3, P), np.float32)
    view = (torch.from_numpy(Q).to(DEV), P, torch.from_numpy(p).to(DEV).view(-1), P, 3 * P, P)
    T = int(Q.sum())
    expect = Q.astype(np.float64) * P / T
    for method, bound in ((R.STRATIFIED, 2.0), (R.SYSTEMATIC, 1.0)):
        anc = _run_ex(view, P, 5, 2, 0, P, method, None, K40)[0]
        counts = np.bincount(anc, minlength=P)
        assert np.abs(counts - expect).max() < bound, method


def _pf(P, seed, **kw):
    from vitparticlefiltertracker_amd.particle_filter import ParticleFilter
    return ParticleFilter(P, (100.0, 90.0, 1.0), (3.0, 2.0, 0.03), (0.6, 1.8), seed, DEV, frame_size=(224, 224),
                          lam=20.0, weight_bits=K40, **kw)


@pytest.mark.parametrize("method", [R.SYSTEMATIC, R.STRATIFIED])
def test_particle_filter_gated_recursion_equals_reference(method):
    """8 frames of injected likelihoods at P = 100, tau = 0.5, alternating flat (ess = P: skip, the weights carry)
    and concentrated (ess << P: resample). Flags, ess, carries, ancestors, states and estimates follow the reference
    recursion, and both branches occur."""
    P, seed, tau = 100, 321, 0.5
    f = _pf(P, seed, resample_method=method, ess_threshold=tau)
    assert f.carry is not None and f.carry.cpu().tolist() == [R.identity(K40)] * P
    ref = R.Filter(P, (100.0, 90.0, 1.0), (3.0, 2.0, 0.03), (0.6, 1.8), seed, (224, 224), K40, method, tau)
    rng = np.random.default_rng(3)
    flags = []
    for k in range(1, 9):
        if k % 2:
            L = rng.integers((1 << 40) - (1 << 30), (1 << 40) + 1, P, dtype=np.int64)       # flat
        else:
            L = rng.integers(0, 1 << 20, P, dtype=np.int64)                                 # concentrated
            L[rng.integers(0, P, 3)] = 1 << 40
        f.predict()
        ref.predict()
        assert np.array_equal(f.particles_soa.cpu().numpy().view(np.uint32), ref.particles.view(np.uint32))
        f.set_weights(torch.from_numpy(L).to(DEV))
        if k % 4 == 0:
            est = f.estimate()
            anc = f.resample().cpu().numpy()
        else:
            est = f.step()
            anc = f.last_ancestors.cpu().numpy()
        r = ref.update(L)
        flags.append(f.last_resampled)
        assert f.last_resampled == r["resampled"], f"frame {k}"
        assert R.f64_bits(f.last_ess) == R.f64_bits(r["ess"]), f"frame {k}"
        assert np.array_equal(anc, r["anc"]), f"frame {k}: ancestors"
        assert np.array_equal(f.particles_soa.cpu().numpy().view(np.uint32), r["states"].view(np.uint32)), f"frame {k}"
        assert f.carry.cpu().tolist() == [int(c) for c in r["carry"]], f"frame {k}: carry"
        np.testing.assert_allclose(est, R.estimate(r, P), rtol=1e-12)
    assert True in flags and False in flags, flags
    f.reset((1.0, 2.0, 1.0))
    assert f.carry.cpu().tolist() == [R.identity(K40)] * P


def test_particle_filter_defaults_keep_the_plain_path():
    """Default arguments: no carry, 32-B statistics, and the frame's results are vpf_estimate_resample's (the oracle's
    S7 ancestors), as before S10."""
    P, seed = 100, 321
    f = _pf(P, seed)
    assert f.carry is None and f._stats_dev.numel() == 4 and f._stats_pin.numel() == 4
    assert f.last_ess is None
    states = np.empty((3, P), np.float32)
    states[0], states[1], states[2] = 100.0, 90.0, 1.0
    rng = np.random.default_rng(4)
    for k in range(1, 4):
        f.predict()
        opf.predict(states, 0, seed, k, (3.0, 2.0, 0.03), 224, 224, (0.6, 1.8))
        Q = rng.integers(0, 1 << 40, P, dtype=np.int64)
        f.set_weights(torch.from_numpy(Q).to(DEV))
        est = f.step()
        anc = opf.resample(Q, opf.resample_U(seed, k))
        np.testing.assert_allclose(est, opf.estimate(Q, states), rtol=1e-12)
        assert np.array_equal(f.last_ancestors.cpu().numpy(), anc)
        states = np.ascontiguousarray(states[:, anc])
        assert np.array_equal(f.particles_soa.cpu().numpy().view(np.uint32), states.view(np.uint32))
        assert f.last_resampled is True and f.last_ess is None
