"""GPU (MI355X): the SPEC S15 kernels (vpf_estimate_resample_gate, vpf_weighted_sums_gate) bit for bit against the
Python-int reference (tests/s15_reference.py): both sides of the integer boundary, every size at which the tree, the
thread tail or the 4096-element scan block changes path, one and four (padded) shards, every slot range, both schemes.
The states are small integers and halves; the sums are compared with the reference's device-order sums bit for bit and,
on weights that are multiples of 2^20, with the exact integer sums (no order can round those).
Run: python -m pytest tests -m gpu."""
import numpy as np
import pytest
import torch

import s10_reference as R10
import s15_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
K40 = 40
METHODS = {R10.SYSTEMATIC: 0, R10.STRATIFIED: 1}
SEED, FRAME = (1 << 41) + 12345, 7


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()
    assert torch.cuda.is_available()


def vpf():
    return torch.ops.vpf


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _states(P, rows, rng):
    """Small integers and halves: every product with a weight, and every partial sum of the coarse-weight cases, is
    exact."""
    return (rng.integers(0, 32, (rows, P)) * 0.5).astype(np.float32)


def _weights(P, rng, peak_at, coarse=False):
    """Random in [0, 2^40] (coarse: multiples of 2^20), the unique maximum 2^40 - 3 (coarse: 2^40) at `peak_at`."""
    if coarse:
        Q = rng.integers(0, 1 << 20, P, dtype=np.int64) << 20
        Q[peak_at] = 1 << 40
    else:
        Q = rng.integers(0, (1 << 40) - 3, P, dtype=np.int64)
        Q[peak_at] = (1 << 40) - 3
    return Q


def _layout(Q, p, G, pad):
    """The global view of Q int64[P] and rows float32[R][P] as G shards; pad > 0: q_stride, ld and p_stride larger than
    they need be, the gaps filled with values that would show if read (NaN, a huge weight)."""
    P, R_ = Q.shape[0], p.shape[0]
    n = P // G
    assert n * G == P
    ld = n + (3 if pad else 0)
    qs = n + (5 if pad else 0)
    ps = R_ * ld + (7 if pad else 0)
    Qb = np.full((G - 1) * qs + n + (pad and 2), 1 << 60, np.int64)
    pb = np.full((G - 1) * ps + (R_ - 1) * ld + n + (pad and 2), np.nan, np.float32)
    for r in range(G):
        Qb[r * qs: r * qs + n] = Q[r * n:(r + 1) * n]
        for c in range(R_):
            pb[r * ps + c * ld: r * ps + c * ld + n] = p[c, r * n:(r + 1) * n]
    return torch.from_numpy(Qb).to(DEV), qs, torch.from_numpy(pb).to(DEV), ld, ps, n


def _run_gate(view, P, b, e, method, gq, K=K40, seed=SEED, frame=FRAME):
    n = e - b
    anc = torch.full((max(n, 1),), -1, device=DEV, dtype=torch.int32)
    st = torch.full((3, max(n, 1)), -7.0, device=DEV)
    cdf = torch.full((P,), -1, device=DEV, dtype=torch.int64)
    stats = torch.full((8,), -1, device=DEV, dtype=torch.int64)
    carry = torch.full((max(n, 1),), -1, device=DEV, dtype=torch.int64)
    vpf().estimate_resample_gate(*view, P, seed, frame, b, e, anc, st, cdf, stats, METHODS[method], K, gq, carry)
    return anc.cpu().numpy(), st.cpu().numpy(), cdf.cpu().numpy(), stats.cpu(), carry.cpu().numpy()


def _check(got, ref, Q, b, e, tag):
    anc, st, cdf, stats, carry = got
    n = e - b
    assert np.array_equal(anc[:n], ref["anc"][b:e]), tag
    assert np.array_equal(bits32(st[:, :n]), bits32(ref["states"][:, b:e])), tag
    assert np.array_equal(carry[:n], ref["carry"][b:e]), tag
    if n == 0:      # an empty slot range writes no slot
        assert anc[0] == -1 and carry[0] == -1 and (st == -7.0).all(), tag
    assert int(stats[0]) == ref["T"], tag
    assert [int(v) for v in stats[1:4]] == [R10.f64_bits(s) for s in ref["tree"]], tag
    assert int(stats[4]) == R10.f64_bits(ref["ess"]), tag
    assert int(stats[5]) == int(ref["resampled"]) and int(stats[6]) == ref["m"], tag
    assert int(stats[7]) == int(ref["held"]), tag
    if not ref["held"]:
        assert np.array_equal(cdf, np.cumsum(Q)), tag


def _slot_ranges(P):
    return sorted({(0, P), (P // 3, max(P // 3, (2 * P) // 3)), (P // 2, P // 2)})


@pytest.mark.parametrize("P", [1, 64, 1000, 1024, 1025, 4097])
def test_gate_equals_reference_on_both_sides_of_the_boundary(P):
    """One shard. The maximum m at index 0 and at P - 1; gate_q one above m (held), equal to m and one below (not held);
    both schemes; the slot ranges [0, P), an interior one and an empty one. Everything the call writes equals the
    reference; a held call's states_out are the slots' own states, its anc their own indices, its carry the identity."""
    rng = np.random.default_rng(P)
    p = _states(P, 3, rng)
    held = set()
    for peak_at in sorted({0, P - 1}):
        Q = _weights(P, rng, peak_at)
        m = int(Q.max())
        assert int(Q.argmax()) == peak_at and (Q == m).sum() == 1
        view = _layout(Q, p, 1, 0)
        for method in METHODS:
            for gq in (m + 1, m, m - 1):
                ref = R.step(Q, p, SEED, FRAME, method, K40, gq)
                assert ref["held"] == (gq == m + 1)
                held.add(ref["held"])
                for b, e in _slot_ranges(P):
                    got = _run_gate(view, P, b, e, method, gq)
                    _check(got, ref, Q, b, e, f"P={P} peak@{peak_at} {method} gate_q=m{gq - m:+d} slots [{b}, {e})")
                    if ref["held"]:
                        assert np.array_equal(got[0][:e - b], np.arange(b, e))
                        assert np.array_equal(bits32(got[1][:, :e - b]), bits32(p[:, b:e]))
                        assert (got[4][:e - b] == R10.identity(K40)).all() and int(got[3][7]) == 1
    assert held == {True, False}


@pytest.mark.parametrize("P", [1024, 4096])
def test_gate_over_four_padded_shards(P):
    """Four gathered shards with q_stride, ld and p_stride larger than the shard (the gaps hold NaN and 2^60, which any
    read would show), the maximum the last element of the last shard; every shard's slot range, an interior range
    across a shard boundary and an empty one; the result is the one-shard reference's."""
    rng = np.random.default_rng(P + 4)
    p = _states(P, 3, rng)
    Q = _weights(P, rng, P - 1)
    m = int(Q.max())
    view = _layout(Q, p, 4, 1)
    one = _layout(Q, p, 1, 0)
    n = P // 4
    for method in METHODS:
        for gq in (m + 1, m, m - 1):
            ref = R.step(Q, p, SEED, FRAME, method, K40, gq)
            for b, e in [(r * n, (r + 1) * n) for r in range(4)] + [(n - 5, 2 * n + 9), (n, n)]:
                _check(_run_gate(view, P, b, e, method, gq), ref, Q, b, e,
                       f"P={P} {method} gate_q=m{gq - m:+d} [{b}, {e})")
            a, c = _run_gate(view, P, 0, P, method, gq), _run_gate(one, P, 0, P, method, gq)
            assert np.array_equal(a[0], c[0]) and np.array_equal(bits32(a[1]), bits32(c[1]))
            assert torch.equal(a[3], c[3]) and np.array_equal(a[4], c[4])


@pytest.mark.parametrize("P", [1, 1000, 4097])
def test_coarse_weights_give_the_exact_integer_sums(P):
    """Weights that are multiples of 2^20 and states in halves: every partial sum is an integer below 2^53 in units of
    2^19, so the fp64 sums equal the exact integer sums in any order; held, they are the plain sums of the states."""
    rng = np.random.default_rng(P + 1)
    p = _states(P, 3, rng)
    Q = _weights(P, rng, P // 2, coarse=True)
    view = _layout(Q, p, 1, 0)
    twice = np.round(p.astype(np.float64) * 2).astype(np.int64)
    for gq, held in ((1 << 40, False), (0, False)):      # the maximum is 2^40 == gate_q: not held
        stats = _run_gate(view, P, 0, P, R10.SYSTEMATIC, gq)[3]
        want = [sum(int(q) * int(v) for q, v in zip(Q, twice[c])) / 2.0 for c in range(3)]
        assert stats[1:4].view(torch.float64).tolist() == want and int(stats[7]) == int(held)
    Qlow = Q >> 1                                   # the maximum 2^39: held under gate_q = 2^40
    stats = _run_gate(_layout(Qlow, p, 1, 0), P, 0, P, R10.SYSTEMATIC, 1 << 40)[3]
    assert int(stats[7]) == 1 and int(stats[0]) == int(Qlow.sum()) and int(stats[6]) == 1 << 39
    assert stats[1:4].view(torch.float64).tolist() == [float(twice[c].sum()) / 2.0 for c in range(3)]


@pytest.mark.parametrize("P", [1, 1000, 4097])
def test_all_zero_weights(P):
    """T == 0: with gate_q = 0 the frame is not held and resamples uniformly, as vpf_estimate_resample_ex does; with
    gate_q = 1 it is held (m = 0 < 1), not uniformly resampled (the uniform resample's ancestors are the identity too:
    the flags tell the two apart). The sums are the every-weight-1 ones either way."""
    rng = np.random.default_rng(P + 2)
    p = _states(P, 3, rng)
    Q = np.zeros(P, np.int64)
    view = _layout(Q, p, 1, 0)
    for method in METHODS:
        for gq in (0, 1):
            ref = R.step(Q, p, SEED, FRAME, method, K40, gq)
            assert ref["held"] == bool(gq) and ref["T"] == 0
            got = _run_gate(view, P, 0, P, method, gq)
            _check(got, ref, Q, 0, P, f"P={P} {method} gate_q={gq}")
            assert got[3][1:4].view(torch.float64).tolist() == [float(p[c].astype(np.float64).sum()) for c in range(3)]


@pytest.mark.parametrize("P,kind", [(1, "random"), (1000, "random"), (1025, "random"), (4097, "zero"),
                                    (4097, "random")])
def test_gate_q_zero_is_estimate_resample_ex_without_its_gate(P, kind):
    """gate_q = 0 never holds: anc, states, carry, the CDF and stats[0..6] are vpf_estimate_resample_ex(ess_tau = -1)'s
    bits for both schemes, and so are they at any gate_q <= m; that call's own stats[7] stays 0."""
    rng = np.random.default_rng(P + 3)
    p = _states(P, 3, rng)
    Q = np.zeros(P, np.int64) if kind == "zero" else _weights(P, rng, P // 2)
    view = _layout(Q, p, 1, 0)
    for method in METHODS:
        anc0 = torch.full((P,), -1, device=DEV, dtype=torch.int32)
        st0 = torch.empty(3, P, device=DEV)
        cdf0 = torch.empty(P, device=DEV, dtype=torch.int64)
        stats0 = torch.full((8,), -1, device=DEV, dtype=torch.int64)
        carry0 = torch.empty(P, device=DEV, dtype=torch.int64)
        vpf().estimate_resample_ex(*view, P, SEED, FRAME, 0, P, anc0, st0, cdf0, stats0, METHODS[method], -1.0, K40,
                                   carry0)
        assert int(stats0[7]) == 0
        for gq in (0,) if kind == "zero" else (0, 1, int(Q.max())):
            anc, st, cdf, stats, carry = _run_gate(view, P, 0, P, method, gq)
            assert np.array_equal(anc, anc0.cpu().numpy()) and np.array_equal(bits32(st), bits32(st0.cpu().numpy()))
            assert np.array_equal(cdf, cdf0.cpu().numpy()) and np.array_equal(carry, carry0.cpu().numpy())
            assert torch.equal(stats[:7], stats0.cpu()[:7]) and int(stats[7]) == 0 and int(stats[5]) == 1


def _run_sums(view, P, n_rows, gq=None):
    out = torch.full((4,), -1, device=DEV, dtype=torch.int64)
    if gq is None:
        vpf().weighted_sums(*view, P, n_rows, out)
    else:
        vpf().weighted_sums_gate(*view, P, n_rows, gq, out)
    return out.cpu()


@pytest.mark.parametrize("G,pad", [(1, 0), (4, 1)])
@pytest.mark.parametrize("n_rows", [1, 2, 3])
def test_weighted_sums_gate_on_both_sides_of_the_boundary(n_rows, G, pad):
    """1, 2 and 3 extra rows: not held (gate_q = m, m - 1, 0) the output is vpf_weighted_sums' bits and the reference's
    device-order sums; held (gate_q = m + 1) out[0] is still the true T and the sums are the every-weight-1 ones, the
    rows not given 0; over three rows it is vpf_estimate_resample_gate's stats[0..3] on either side."""
    P = 4096 if G == 4 else 1025
    rng = np.random.default_rng(10 * n_rows + G)
    rows = _states(P, n_rows, rng)
    Q = _weights(P, rng, P - 1)
    m = int(Q.max())
    view = _layout(Q, rows, G, pad)
    pad3 = np.zeros((3, P), np.float32)
    pad3[:n_rows] = rows
    plain = _run_sums(view, P, n_rows)
    assert [int(v) for v in plain] == [int(Q.sum())] + [R10.f64_bits(s) for s in R.tree_sums(Q, pad3)]
    for gq in (m, m - 1, 0):
        assert torch.equal(_run_sums(view, P, n_rows, gq), plain), gq
    held = _run_sums(view, P, n_rows, m + 1)
    want = [float(pad3[c].astype(np.float64).sum()) for c in range(3)]
    assert int(held[0]) == int(Q.sum()) and held[1:4].view(torch.float64).tolist() == want
    assert [int(v) for v in held[1:4]] == [R10.f64_bits(s) for s in R.tree_sums([1] * P, pad3)]
    if n_rows == 3:
        for gq in (m, m + 1):
            stats = _run_gate(view, P, 0, P, R10.SYSTEMATIC, gq)[3]
            assert torch.equal(stats[:4], _run_sums(view, P, 3, gq)), gq
    zero = _layout(np.zeros(P, np.int64), rows, G, pad)
    for gq in (0, 1):                             # T == 0: the uniform sums whether held or not
        z = _run_sums(zero, P, n_rows, gq)
        assert int(z[0]) == 0 and z[1:4].view(torch.float64).tolist() == want


def test_bad_arguments_are_refused():
    """VPF_ERR_ARG (the binding raises) for gate_q outside [0, 2^bits], bits outside [0, 61] and an unknown method; the
    valid extremes pass. Nothing is launched for a refused call: the outputs keep their fill."""
    from vitparticlefiltertracker_amd._lib import VPFError
    P = 64
    rng = np.random.default_rng(0)
    Q, p = _weights(P, rng, 3), _states(P, 3, rng)
    view = _layout(Q, p, 1, 0)

    def call(method, bits, gq):
        anc = torch.full((P,), -1, device=DEV, dtype=torch.int32)
        st = torch.empty(3, P, device=DEV)
        cdf = torch.empty(P, device=DEV, dtype=torch.int64)
        stats = torch.full((8,), -1, device=DEV, dtype=torch.int64)
        carry = torch.empty(P, device=DEV, dtype=torch.int64)
        vpf().estimate_resample_gate(*view, P, 1, 1, 0, P, anc, st, cdf, stats, method, bits, gq, carry)
        return stats.cpu(), anc.cpu()
    for method, bits, gq in ((0, K40, -1), (0, K40, (1 << K40) + 1), (1, 10, 1025), (0, -1, 0), (0, 62, 0), (2, K40, 0),
                             (-1, K40, 0)):
        with pytest.raises(VPFError):
            call(method, bits, gq)
    stats, anc = call(0, K40, 1 << K40)
    assert int(stats[7]) == 1 and np.array_equal(anc.numpy(), np.arange(P))
    stats, _ = call(1, 61, 0)
    assert int(stats[7]) == 0
    out = torch.full((4,), -1, device=DEV, dtype=torch.int64)
    for n_rows, gq in ((3, -1), (3, (1 << 61) + 1), (0, 0), (4, 0)):
        with pytest.raises((VPFError, ValueError)):
            vpf().weighted_sums_gate(*view, P, n_rows, gq, out)
    assert out.cpu().tolist() == [-1] * 4
