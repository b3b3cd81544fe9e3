"""GPU (MI355X): vpf_mode_estimate (SPEC S17) bit for bit against the Python-int reference (tests/s17_reference.py): `out`
(i*, Tm and the bits of the six fp64 sums) and the whole density `dens_ws`, at every size where a wave, a seed block (512
seeds), an LDS tile (128 entries) or a j-chunk of several tiles (P > 5792) ends; 2 and 3 padded shards; the window's
inclusive edge; ties; a 2^62 density; the uniform-weight frames (T == 0, a held frame); non-finite states; 0..3 extra
rows; refused arguments; one graph capture and replay.
Run: python -m pytest tests -m gpu."""
import numpy as np
import pytest
import torch

import s17_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from vitparticlefiltertracker_amd import _lib, ops  # noqa: F401
    assert b"gfx950" in _lib.lib().vpf_version()
    assert torch.cuda.is_available()


def vpf():
    return torch.ops.vpf


def _cloud(P, rows=3, seed=0, K=40, span=300.0):
    """A few clusters on a quarter-pixel grid (so that pairs also sit exactly on a window's edge) plus a uniform
    background; scales and extra rows in sixteenths; weights anywhere in [0, 2^K)."""
    rng = np.random.default_rng(seed)
    st = np.empty((rows, P), np.float32)
    c = rng.uniform(0.2 * span, 0.8 * span, (4, 2))
    k = rng.integers(0, 5, P)
    for a in range(2):
        v = np.where(k < 4, c[np.minimum(k, 3), a] + rng.normal(0, 6, P), rng.uniform(0, span, P))
        st[a] = np.round(v * 4) / 4
    st[2:] = rng.integers(8, 32, (rows - 2, P)) / 16.0
    return rng.integers(0, 1 << K, P, dtype=np.int64), st


def _layout(Q, p, G, pad):
    """The global view of Q int64[P] and rows float32[R][P] as G shards; pad: q_stride, ld and p_stride larger than they
    need be, the gaps filled with values that would show if read (NaN states, a 2^60 weight)."""
    P, rows = Q.shape[0], p.shape[0]
    n = P // G
    assert n * G == P
    ld = n + (3 if pad else 0)
    qs = n + (5 if pad else 0)
    ps = rows * ld + (7 if pad else 0)
    Qb = np.full((G - 1) * qs + n + (2 if pad else 0), 1 << 60, np.int64)
    pb = np.full((G - 1) * ps + (rows - 1) * ld + n + (2 if pad else 0), np.nan, np.float32)
    for r in range(G):
        Qb[r * qs: r * qs + n] = Q[r * n:(r + 1) * n]
        for c in range(rows):
            pb[r * ps + c * ld: r * ps + c * ld + n] = p[c, r * n:(r + 1) * n]
    return torch.from_numpy(Qb).to(DEV), qs, torch.from_numpy(pb).to(DEV), ld, ps, n


def _stats(T, held=0, fill=-1):
    """The statistics block an estimate + resample call leaves: T at [0], the held flag at [7]; the rest is not read."""
    s = np.full(8, fill, np.int64)
    s[0], s[7] = T, held
    return torch.from_numpy(s).to(DEV)


def _run(view, P, n_extra, hx, hy, stats, gate=False):
    dens = torch.full((P,), -1, device=DEV, dtype=torch.int64)
    out = torch.full((8,), -1, device=DEV, dtype=torch.int64)
    vpf().mode_estimate(*view, P, n_extra, float(hx), float(hy), stats, gate, dens, out)
    return out.cpu().numpy(), dens.cpu().numpy()


def _check(got, ref, tag=""):
    out, dens = got
    assert np.array_equal(dens, ref["D"]), f"{tag}: density"
    assert out.tolist() == R.out_words(ref).tolist(), f"{tag}: out"


@pytest.mark.parametrize("P", [1, 63, 64, 65, 127, 128, 129, 257, 512, 513, 1000, 6001])
def test_edge_sizes(P):
    """One shard, three rows. 64: a wave; 128: an LDS tile; 512: a seed block; 6001: the first sizes at which a j-chunk
    holds more than one tile (two, the last chunk one)."""
    Q, st = _cloud(P, seed=P)
    hx, hy = f32(9.25), f32(7.0)
    ref = R.mode(Q, st, hx, hy, False)
    assert P < 64 or 1 < np.unique(ref["D"]).size
    _check(_run(_layout(Q, st, 1, 0), P, 0, hx, hy, _stats(int(Q.sum()))), ref, f"P={P}")


@pytest.mark.parametrize("n_extra", [0, 3])
def test_padded_shards_equal_one_shard(n_extra):
    P = 1002
    Q, st = _cloud(P, rows=3 + n_extra, seed=7)
    hx, hy = f32(12.0), f32(12.0)
    ref = R.mode(Q, st, hx, hy, False)
    one = _run(_layout(Q, st, 1, 0), P, n_extra, hx, hy, _stats(int(Q.sum())))
    _check(one, ref, "one shard")
    for G in (2, 3):
        got = _run(_layout(Q, st, G, 1), P, n_extra, hx, hy, _stats(int(Q.sum())))
        _check(got, ref, f"{G} shards")
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1])


def test_window_edge_is_inclusive_and_zero_counts_coincident_particles_only():
    hx = f32(8.0)
    x = np.array([100.0, 108.0, np.nextafter(f32(108.0), f32(200.0)), 100.0, 92.0], np.float32)
    st = np.stack([x, np.full(5, 50.0, np.float32), np.ones(5, np.float32)])
    Q = np.array([1, 10, 100, 1000, 10000], np.int64)
    for a, b, D in ((hx, f32(0.0), [11011, 1111, 110, 11011, 11001]), (f32(0.0), hx, [1001, 10, 100, 1001, 10000]),
                    (f32(0.0), f32(0.0), [1001, 10, 100, 1001, 10000])):
        ref = R.mode(Q, st, a, b, False)
        assert ref["D"].tolist() == D
        _check(_run(_layout(Q, st, 1, 0), 5, 0, a, b, _stats(int(Q.sum()))), ref, f"hx={a} hy={b}")
        swapped = np.ascontiguousarray(st[[1, 0, 2]])          # the same on the y axis
        _check(_run(_layout(Q, swapped, 1, 0), 5, 0, b, a, _stats(int(Q.sum()))), R.mode(Q, swapped, b, a, False))


def test_ties_take_the_smallest_index():
    P = 700
    Q, st = _cloud(P // 2, seed=11)
    Q, st = np.concatenate([Q, Q]), np.concatenate([st, st], axis=1)       # particle i + 350 duplicates particle i
    hx, hy = f32(10.0), f32(10.0)
    ref = R.mode(Q, st, hx, hy, False)
    assert ref["i"] < P // 2 and ref["D"][ref["i"] + P // 2] == ref["D"][ref["i"]]
    got = _run(_layout(Q, st, 1, 0), P, 0, hx, hy, _stats(int(Q.sum())))
    _check(got, ref)
    flipped = np.ascontiguousarray(st[:, ::-1])                            # the other copy now comes first
    rf = R.mode(Q[::-1].copy(), flipped, hx, hy, False)
    assert rf["i"] == P // 2 - 1 - ref["i"]
    _check(_run(_layout(Q[::-1].copy(), flipped, 1, 0), P, 0, hx, hy, _stats(int(Q.sum()))), rf)


def test_density_accumulates_in_64_bits():
    """K = 50, P = 4096, every particle at one point with Q = 2^50: D_i = 2^62 for every i, which neither a 32-bit nor
    an fp32 / fp64 accumulator of odd multiples holds; one more unit of weight on one particle shows in the last bit."""
    P, K = 4096, 50
    st = np.stack([np.full(P, 123.25, np.float32), np.full(P, 45.5, np.float32), np.full(P, 1.5, np.float32)])
    Q = np.full(P, 1 << K, np.int64)
    out, dens = _run(_layout(Q, st, 1, 0), P, 0, f32(0.0), f32(0.0), _stats(1 << 62))
    assert (dens == 1 << 62).all() and out[0] == 0 and out[1] == 1 << 62
    assert out[2:5].view(np.float64).tolist() == [123.25 * 2.0 ** 62, 45.5 * 2.0 ** 62, 1.5 * 2.0 ** 62]
    assert not out[5:].any()
    Q[1:] -= 1
    Q[0] = (1 << K) - 1 + 4095 - 2                         # the sum is 2^62 - 3: odd, above 2^53
    ref = R.mode(Q, st, f32(0.0), f32(0.0), False)
    assert ref["Tm"] == (1 << 62) - 3
    _check(_run(_layout(Q, st, 1, 0), P, 0, f32(0.0), f32(0.0), _stats(ref["Tm"])), ref)


def test_uniform_weights_when_t_is_zero_or_the_frame_is_held():
    P = 777
    Q, st = _cloud(P, rows=5, seed=23)
    hx, hy = f32(11.0), f32(11.0)
    T = int(Q.sum())
    view = _layout(Q, st, 1, 0)
    weighted, uniform = R.mode(Q, st, hx, hy, False), R.mode(Q, st, hx, hy, True)
    assert weighted["i"] != uniform["i"] and uniform["Tm"] == int(uniform["D"].max()) <= P
    _check(_run(view, P, 2, hx, hy, _stats(0)), uniform, "T == 0")
    _check(_run(view, P, 2, hx, hy, _stats(0), gate=True), uniform, "T == 0, gated")
    _check(_run(view, P, 2, hx, hy, _stats(T, held=1), gate=True), uniform, "held")
    _check(_run(view, P, 2, hx, hy, _stats(T, held=0), gate=True), weighted, "gated, not held")
    _check(_run(view, P, 2, hx, hy, _stats(T, held=1), gate=False), weighted, "no gate: [7] is not read")
    _check(_run(view, P, 2, hx, hy, _stats(T)[:4].contiguous(), gate=False), weighted, "the 32-B statistics")
    # the statistics as vpf_estimate_resample_gate itself leaves them, on the same stream, on either side of its gate
    m = int(Q.max())
    for gq, ref in ((m + 1, uniform), (m, weighted)):
        stats = torch.full((8,), -1, device=DEV, dtype=torch.int64)
        vpf().estimate_resample_gate(*view, P, 99, 3, 0, P, torch.empty(P, device=DEV, dtype=torch.int32),
                                     torch.empty(3, P, device=DEV), torch.empty(P, device=DEV, dtype=torch.int64),
                                     stats, 0, 40, gq, torch.empty(P, device=DEV, dtype=torch.int64))
        _check(_run(view, P, 2, hx, hy, stats, gate=True), ref, f"gate_q = m{gq - m:+d}")
        assert int(stats[7]) == int(gq > m)


def test_non_finite_states_are_in_no_window():
    P = 300
    Q, st = _cloud(P, seed=31)
    hx, hy = f32(15.0), f32(15.0)
    clean = R.mode(Q, st, hx, hy, False)
    bad = st.copy()
    i = clean["i"]
    bad[0, i], bad[1, (i + 1) % P], bad[0, (i + 2) % P], bad[1, (i + 3) % P] = np.nan, np.inf, -np.inf, np.nan
    bad[0, 7], bad[1, 7] = np.inf, np.inf
    ref = R.mode(Q, bad, hx, hy, False)
    assert ref["i"] != i and ref["D"][i] == 0 and ref["D"][7] == 0 and all(np.isfinite(ref["sums"]))
    _check(_run(_layout(Q, bad, 1, 0), P, 0, hx, hy, _stats(int(Q.sum()))), ref)
    for fill in (np.nan, np.inf):
        gone = bad.copy()
        gone[0] = fill
        out, dens = _run(_layout(Q, gone, 1, 0), P, 0, hx, hy, _stats(int(Q.sum())))
        assert not dens.any() and not out.any(), "every state non-finite: Tm == 0, i* == 0, every sum +0"
        _check((out, dens), R.mode(Q, gone, hx, hy, False))
    # a non-finite scale inside the window is summed as SPEC S6 sums it; outside the window it is not read
    far = st.copy()
    far[2, (np.flatnonzero(~R.in_window(st[0, i], st[1, i], st[0], st[1], hx, hy))[0])] = np.nan
    _check(_run(_layout(Q, far, 1, 0), P, 0, hx, hy, _stats(int(Q.sum()))), R.mode(Q, far, hx, hy, False))
    assert R.mode(Q, far, hx, hy, False)["sums"] == clean["sums"]
    near = st.copy()
    near[2, i] = np.nan
    rn = R.mode(Q, near, hx, hy, False)
    assert rn["sums"][:2] == clean["sums"][:2] and np.isnan(rn["sums"][2])
    _check(_run(_layout(Q, near, 1, 0), P, 0, hx, hy, _stats(int(Q.sum()))), rn)


@pytest.mark.parametrize("n_extra", [0, 1, 2, 3])
def test_extra_rows(n_extra):
    P = 1300
    Q, st = _cloud(P, rows=6, seed=41)
    hx, hy = f32(13.5), f32(9.0)
    ref = R.mode(Q, st[:3 + n_extra], hx, hy, False)
    out, dens = _run(_layout(Q, st, 1, 0), P, n_extra, hx, hy, _stats(int(Q.sum())))
    _check((out, dens), ref, f"n_extra={n_extra}")
    assert not out[5 + n_extra:].any() and (n_extra == 0 or out[4 + n_extra] != 0)
    if n_extra:                # the extra rows' sums are vpf_weighted_sums' over the masked weights
        m = R.in_window(st[0, ref["i"]], st[1, ref["i"]], st[0], st[1], hx, hy)
        Qm = np.where(m, Q, 0)
        ws = torch.full((4,), -1, device=DEV, dtype=torch.int64)
        Qd, qs, pd, ld, ps, n = _layout(Qm, st, 1, 0)
        vpf().weighted_sums(Qd, qs, pd[3 * ld:], ld, ps, n, P, n_extra, ws)
        assert ws.cpu().numpy().tolist() == [ref["Tm"]] + out[5:8].tolist()


def test_bad_arguments_are_refused():
    from vitparticlefiltertracker_amd import _lib
    from vitparticlefiltertracker_amd._lib import VPFError
    P = 64
    Q, st = _cloud(P, rows=4, seed=51)
    view = _layout(Q, st, 1, 0)
    for hx, hy in ((float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("-inf")), (-1.0, 1.0),
                   (1.0, -0.5)):
        dens = torch.full((P,), -1, device=DEV, dtype=torch.int64)
        out = torch.full((8,), -1, device=DEV, dtype=torch.int64)
        with pytest.raises(VPFError):
            vpf().mode_estimate(*view, P, 0, hx, hy, _stats(1), False, dens, out)
        assert (dens == -1).all() and (out == -1).all(), "a refused call launches nothing"
    for n_extra in (-1, 2, 4):                  # the view holds four rows: one extra row at the most
        with pytest.raises((VPFError, ValueError)):
            _run(view, P, n_extra, 1.0, 1.0, _stats(1))
    _run(view, P, 1, 0.0, 0.0, _stats(1))       # the valid extremes pass
    Qd, qs, pd, ld, ps, n = view
    stats, dens, out = _stats(1), torch.zeros(P, device=DEV, dtype=torch.int64), torch.zeros(8, device=DEV,
                                                                                            dtype=torch.int64)
    raw = _lib.lib().vpf_mode_estimate

    def rc(P_=P, n_=n, ld_=ld, nx=0, hx=1.0, hy=1.0, q=Qd.data_ptr(), o=out.data_ptr()):
        return raw(q, qs, pd.data_ptr(), ld_, ps, n_, P_, nx, hx, hy, stats.data_ptr(), 0, dens.data_ptr(), o,
                   _lib.stream_ptr())
    assert rc() == 0
    assert rc(P_=0) == -1 and rc(P_=-1) == -1 and rc(P_=63) == -1 and rc(ld_=n - 1) == -1 and rc(n_=0) == -1
    assert rc(nx=4) == -1 and rc(nx=-1) == -1 and rc(q=0) == -1 and rc(o=0) == -1
    torch.cuda.synchronize()


def test_graph_replay_equals_the_eager_call():
    P = 1500
    Q, st = _cloud(P, rows=5, seed=61)
    Q2, st2 = _cloud(P, rows=5, seed=62)
    hx, hy = f32(10.0), f32(14.0)
    Qd, qs, pd, ld, ps, n = _layout(Q, st, 1, 0)
    stats = _stats(int(Q.sum()))
    dens = torch.full((P,), -1, device=DEV, dtype=torch.int64)
    out = torch.full((8,), -1, device=DEV, dtype=torch.int64)

    def call():
        vpf().mode_estimate(Qd, qs, pd, ld, ps, n, P, 2, float(hx), float(hy), stats, False, dens, out)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    eager = (out.cpu().numpy(), dens.cpu().numpy())
    _check(eager, R.mode(Q, st, hx, hy, False), "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for Qn, stn in ((Q2, st2), (Q, st)):        # new inputs in the captured buffers; stale outputs
        Qd.copy_(torch.from_numpy(Qn))
        pd.copy_(torch.from_numpy(stn.reshape(-1)))
        stats.copy_(_stats(int(Qn.sum())))
        dens.fill_(-5)
        out.fill_(-5)
        g.replay()
        got = (out.cpu().numpy(), dens.cpu().numpy())
        _check(got, R.mode(Qn, stn, hx, hy, False), "replay")
    assert np.array_equal(got[0], eager[0]) and np.array_equal(got[1], eager[1])
