"""CPU: exactly computable attention inputs (shared with tests/test_gpu_attention_exact.py, which imports this module),
the proof that the bars set on them are fair, and the proof that those bars reject a wrong kernel.

Attention is out[b, i, h] = softmax_j(q_i . k_j / 8) v_j per unit u = (b, h) = b H + h, head dim 64, on
qkv [B][N][3 * 64 H] (include/vpf.h). Gaussian inputs against a tolerance see a wrong key, a pad row let through
the mask or a key counted in l but not in O only when a heavy softmax weight happens to sit on the faulty position.
Two input families make every output exact instead, so such a fault is a gross difference with a name.

Selection probe. Per unit (its own generator): K rows are random +-1 sign vectors, pi is a permutation of 0..N-1,
Q row i = 64 K[pi(i)], V is random normal rounded to the compute type. Every value is exact in bf16. The score of key
pi(i) is 64 * 64 = 4096, every other score is lower by 64 (64 - <k, k'>). Expected: out[b, i, h] == V[b, pi(i), h] bit
for bit. Why equality is a fair bar for kernels that compute in fp32 with bf16 probabilities:
  * the builder asserts (fp64) that the gap to the best other key, in the kernels' exp2 domain (x 0.125 log2 e), is
    >= 200 for every query. Every other probability is then exp2(-gap) <= 2^-200: 0 in fp32 (subnormals end at
    2^-149) and in bf16, against whatever running maximum is current once the selected key has been seen;
  * the selected key's probability is exp2 of the residual fma(s, c, -round(m c)) with s = m = 4096 and
    c = 0.125 log2 e: at most the rounding error of m c, |m c| 2^-24 = 2^-24 * 739 (and 0 where 4096 c is exact), so
    p = 1 +- 1e-4: it packs to bf16 1.0, and l, whether summed from the fp32 or from the bf16 probabilities, is
    1 +- 1e-4;
  * O = 1.0 * V + 0 * (finite rows) = V exactly in fp32, and O (1 / l) = V (1 +- 1e-4) rounds back to the bf16 value V
    (half a bf16 ulp is 2^-9 = 2e-3 relative). The fp32 kernel divides V by 1.0: bit-equal in fp32.
  * before the selected key's tile arrives the running maximum is some other key's score, at least 200 lower: on
    arrival the lazy rescale (key-pipelined kernel, 16-query strip) or the speculative-max redo (key-streamed kernel:
    the probabilities overflow, the step sum is not <= 256) fires with alpha = exp2(<= -200) = 0 and wipes l and O,
    which were finite. Keys after it never move the maximum.
Three permutation kinds (random, identity, reversal): every key is selected exactly once per unit, and each key
position is selected by a query of the first strip and by one of the last.

Census probe. Every Q row is +2 in all dims, every K row -2: every score is exactly -256 (-32 after the 1/8 scale), all
keys tie, every probability is exp2(0) = 1. V[u][j][d] = 1 if (j + u) % 64 == d else 0, so
out[u][i][d] = cnt / N with cnt = #{j < N : (j + u) % 64 == d}. l = N and O = cnt are exact integers in fp32 whatever
the order of summation; what remains is one reciprocal, one multiply and one bf16 rounding, so a bf16 output is one of
the two bf16 neighbours of cnt / N: |out - cnt / N| < ulp_bf16(cnt / N) (and exactly 0 where cnt = 0). The fp32 kernel
does one fp32 division: |out - cnt / N| <= 2^-22 cnt / N. A dropped key, a doubled key or a pad copy of key N - 1 let
through the mask moves some cnt by 1 (>= 10 % of the value at N <= 640); a zero or garbage pad row scores 0 against
-32 and takes the whole softmax.

The fault models at the end of this module run an fp64 attention with one defect each and show that the bars above
reject it at every tested N > 1; DETECTED_BY records which probe does."""
import functools
import math

import pytest
import torch

HD = 64
LOG2E = 1.4426950408889634

# key counts per path of tests/test_gpu_attention_exact.py (the boundaries are explained there)
PIPE_N = [1, 8, 9, 16, 17, 33, 40, 41, 50, 192, 193, 197, 201, 209, 224, 256]        # key-pipelined kernel
STREAM_N = [257, 264, 265, 272, 273, 288, 300, 330, 384, 400, 545, 577, 640]          # key-streamed kernel
CLS_N = [1, 63, 64, 65, 197, 577, 640]                                                # q_rows = 1
F32_N = [1, 128, 129, 257, 577]
Q8_N = [1, 33, 197, 256]
ALL_N = sorted(set(PIPE_N + STREAM_N + CLS_N + F32_N + Q8_N))
PERMS = ["random", "identity", "reversal"]
MIN_GAP = 200.0


# ---- builders -------------------------------------------------------------------------------------------------------

def _gen(tag, N, u, seed):
    return torch.Generator().manual_seed(((seed * 7919 + tag) * 4099 + N) * 1009 + u)


@functools.lru_cache(maxsize=None)
def selection_probe(N, B, H, kind="random", seed=0, dtype=torch.bfloat16):
    """(qkv [B][N][3 * 64 H] in `dtype`, expected [B][N][64 H] in `dtype`, pi [B][H][N] int64): out[b, i, h] must be
    the bits of V[b, pi[b, h, i], h]. Deterministic from the arguments; the tensors are shared, do not write them."""
    assert kind in PERMS and dtype in (torch.bfloat16, torch.float32)
    D = HD * H
    qkv = torch.empty(B, N, 3, H, HD, dtype=torch.float32)
    pi = torch.empty(B, H, N, dtype=torch.int64)
    for u in range(B * H):
        g = _gen(1, N, u, seed)
        b, h = divmod(u, H)
        k = torch.randint(0, 2, (N, HD), generator=g).float() * 2 - 1
        v = torch.randn(N, HD, generator=g).to(dtype).float()
        p = {"random": torch.randperm(N, generator=g), "identity": torch.arange(N),
             "reversal": torch.arange(N - 1, -1, -1)}[kind]
        qkv[b, :, 0, h] = 64.0 * k[p]
        qkv[b, :, 1, h] = k
        qkv[b, :, 2, h] = v
        pi[b, h] = p
    q, k = qkv[:, :, 0].double().transpose(1, 2), qkv[:, :, 1].double().transpose(1, 2)   # [B][H][N][64]
    s = q @ k.transpose(-1, -2)
    sel = s.gather(-1, pi[..., None])
    assert bool((sel == 4096.0).all())
    if N > 1:   # the precondition of bit equality: every other key at least MIN_GAP below, in the exp2 domain
        other = s.scatter(-1, pi[..., None], -math.inf).amax(-1, keepdim=True)
        gap = ((sel - other) * 0.125 * LOG2E).min().item()
        assert gap >= MIN_GAP, f"selection probe N={N} B={B} H={H} {kind} seed={seed}: gap {gap:.1f} < {MIN_GAP}"
    v = qkv[:, :, 2]                                                                      # [B][N][H][64]
    idx = pi.transpose(1, 2)[..., None].expand(B, N, H, HD)
    expected = v.gather(1, idx).reshape(B, N, D).to(dtype)
    out = qkv.reshape(B, N, 3 * D).to(dtype)
    assert torch.equal(out.float(), qkv.reshape(B, N, 3 * D))       # every input is exact in `dtype`
    return out, expected, pi


def census_counts(N, B, H):
    """cnt [B][H][64] int64: cnt[b, h, d] = #{j < N : (j + b H + h) % 64 == d}."""
    j = torch.arange(N)[None, :] + torch.arange(B * H)[:, None]
    return torch.nn.functional.one_hot(j % HD, HD).sum(1).reshape(B, H, HD)


@functools.lru_cache(maxsize=None)
def census_probe(N, B, H, dtype=torch.bfloat16):
    """(qkv [B][N][3 * 64 H] in `dtype`, cnt [B][H][64] int64): every query row of unit (b, h) must be cnt[b, h] / N."""
    qkv = torch.empty(B, N, 3, H, HD, dtype=torch.float32)
    qkv[:, :, 0] = 2.0
    qkv[:, :, 1] = -2.0
    u = torch.arange(B * H).reshape(B, 1, H)
    j = torch.arange(N).reshape(1, N, 1)
    qkv[:, :, 2] = torch.nn.functional.one_hot((j + u) % HD, HD).float()
    return qkv.reshape(B, N, 3 * HD * H).to(dtype), census_counts(N, B, H)


def census_expected(cnt, N):
    """cnt [B][H][64] -> the exact outputs [B][N][64 H] in float64."""
    B, H, _ = cnt.shape
    return (cnt.double() / N).reshape(B, 1, H * HD).expand(B, N, H * HD)


# ---- the bars, with messages that name the fault --------------------------------------------------------------------

def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def selection_errors(out, qkv, expected, pi, rows=None, limit=4):
    """[] when out[:, :rows] holds the bits of `expected`; otherwise one line per mismatching (b, h, i) (the first
    `limit`), with pi(i) and the V row of that unit whose bits the output does equal, if any."""
    B, N, D = expected.shape
    H = D // HD
    rows = N if rows is None else rows
    out = out.cpu()
    bad = (_bits(out[:, :rows]) != _bits(expected[:, :rows])).reshape(B, rows, H, HD).any(-1)
    if not bool(bad.any()):
        return []
    msgs = [f"selection: {int(bad.sum())} of {bad.numel()} (b, i, h) rows differ from V[pi(i)] (N={N}, rows={rows})"]
    for b, i, h in bad.nonzero()[:limit].tolist():
        got = _bits(out[b, i, h * HD:(h + 1) * HD])
        v = _bits(qkv[b, :, 2 * D + h * HD: 2 * D + (h + 1) * HD])
        hit = (v == got[None, :]).all(-1).nonzero().flatten().tolist()
        what = f"equals V row {hit[0]}" if hit else \
            f"equals no V row of the unit (got[:4] = {out[b, i, h * HD: h * HD + 4].float().tolist()})"
        msgs.append(f"  b={b} h={h} i={i}: pi(i) = {int(pi[b, h, i])}, output {what}")
    return msgs


def ulp_bf16(x):
    """The spacing of bf16 values around x > 0 (float64 tensor): 2^(floor(log2 x) - 7)."""
    _, e = torch.frexp(x)            # x = m 2^e, m in [0.5, 1)
    return torch.exp2((e - 8).double())


def census_errors(out, cnt, N, rows=None, limit=4):
    """[] when every out[b, i < rows, h, d] meets the bar for its type against cnt[b, h, d] / N: bf16 one of the two
    neighbouring bf16 values (|diff| < ulp_bf16), fp32 |diff| <= 2^-22 cnt / N; exactly 0 where cnt = 0. Otherwise one
    line per failing element (the first `limit`): (b, h, i, d), the expected count, and round(out N)."""
    B, H, _ = cnt.shape
    rows = N if rows is None else rows
    out = out.cpu()
    got = out[:, :rows].double().reshape(B, rows, H, HD)
    exact = (cnt.double() / N)[:, None].expand(B, rows, H, HD)
    diff = (got - exact).abs()
    if out.dtype == torch.bfloat16:
        ok = diff < ulp_bf16(exact.clamp_min(2.0 ** -100))
    else:
        ok = diff <= 2.0 ** -22 * exact
    ok = torch.where(exact == 0, got == 0, ok) & torch.isfinite(got)
    if bool(ok.all()):
        return []
    bad = ~ok
    msgs = [f"census: {int(bad.sum())} of {bad.numel()} outputs off cnt / N (N={N}, rows={rows})"]
    # the elements whose rounded count is wrong first: they name the key (a wrong l alone moves every element a little)
    seen = torch.nan_to_num(got * N, nan=-1.0, posinf=-1.0, neginf=-1.0).round()
    miscounted = bad & (seen != cnt[:, None].expand(B, rows, H, HD))
    first = torch.cat([miscounted.nonzero()[:limit], (bad & ~miscounted).nonzero()[:limit]])[:limit]
    for b, i, h, d in first.tolist():
        g = got[b, i, h, d].item()
        msgs.append(f"  b={b} h={h} i={i} d={d} (keys j = {(d - b * H - h) % HD} mod 64): expected cnt "
                    f"{int(cnt[b, h, d])} of {N}, round(out N) = {int(seen[b, i, h, d])} (out = {g!r})")
    return msgs


# ---- fp64 attention, optionally with one defect ---------------------------------------------------------------------

FAULTS = ["drop_last", "double_last", "swap_v", "l_not_o", "q_xor1"]


def model_attention(qkv, H, fault=None):
    """out [B][N][64 H] float64 of the fp64 softmax attention; `fault` plants one defect a kernel could have:
      drop_last    key N - 1 is never visited
      double_last  key N - 1 is visited twice (a pad copy let through the mask)
      swap_v       keys j = (N - 1) // 2 and j + 1 swapped in V only (a wrong PV slot map)
      l_not_o      key N - 1 counted in l but not in O
      q_xor1       query i reads the Q row of query i ^ 1 (the last query of an odd N keeps its own)"""
    B, N, _ = qkv.shape
    q, k, v = qkv.double().reshape(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)   # [B][H][N][64]
    if fault == "q_xor1":
        i = torch.arange(N) ^ 1
        q = q[:, :, torch.where(i < N, i, torch.arange(N))]
    if fault == "swap_v":
        j = (N - 1) // 2
        order = torch.arange(N)
        order[j], order[j + 1] = j + 1, j
        v = v[:, :, order]
    if fault == "drop_last":
        k, v = k[:, :, :N - 1], v[:, :, :N - 1]
    if fault == "double_last":
        k, v = torch.cat([k, k[:, :, N - 1:]], 2), torch.cat([v, v[:, :, N - 1:]], 2)
    p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1)
    if fault == "l_not_o":
        p = p.clone()
        p[..., N - 1] = 0.0
    return (p @ v).transpose(1, 2).reshape(B, N, H * HD)


# ---- tests ----------------------------------------------------------------------------------------------------------

B0, H0 = 3, 3    # the units of the GPU tests


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("N", ALL_N)
def test_selection_probe_is_exact(N, dtype):
    """The fp64 softmax of the selection probe, rounded to the compute type, is V[pi(i)] bit for bit, for the three
    permutation kinds; every key is selected once per unit; the builder is deterministic."""
    for kind in PERMS:
        qkv, expected, pi = selection_probe(N, B0, H0, kind, 0, dtype)
        assert qkv.shape == (B0, N, 3 * HD * H0) and qkv.dtype == dtype and expected.dtype == dtype
        assert torch.equal(pi.sort(-1).values, torch.arange(N).expand(B0, H0, N))
        out = model_attention(qkv, H0).to(dtype)
        assert selection_errors(out, qkv, expected, pi) == []
        again = selection_probe.__wrapped__(N, B0, H0, kind, 0, dtype)
        assert torch.equal(again[0], qkv) and torch.equal(again[2], pi)
    if N > 2:   # units differ, seeds differ
        qkv, _, pi = selection_probe(N, B0, H0, "random", 0, dtype)
        assert not torch.equal(qkv[0, :, :HD], qkv[0, :, HD:2 * HD]) and not torch.equal(pi[0, 0], pi[0, 1])
        assert not torch.equal(selection_probe(N, B0, H0, "random", 1, dtype)[0], qkv)


@pytest.mark.parametrize("N", ALL_N)
def test_census_probe_is_exact(N):
    """The fp64 softmax of the census probe is cnt / N to 1e-14; the counts add up to N per unit; both output types
    rounded from the exact value meet their bar."""
    for dtype in (torch.bfloat16, torch.float32):
        qkv, cnt = census_probe(N, B0, H0, dtype)
        assert qkv.shape == (B0, N, 3 * HD * H0) and qkv.dtype == dtype
        assert bool((cnt.sum(-1) == N).all())
        assert bool((cnt.max(-1).values - cnt.min(-1).values <= 1).all())
        out = model_attention(qkv, H0)
        assert float((out - census_expected(cnt, N)).abs().max()) <= 1e-14
        assert census_errors(out.to(dtype), cnt, N) == []
    if N % HD:   # the units' counts are rotations of each other, not copies
        assert not torch.equal(cnt[0, 0], cnt[0, 1])


def test_ulp_bf16():
    x = torch.tensor([1.0, 1.5, 0.5, 0.75, 10 / 640, 1 / 3], dtype=torch.float64)
    nxt = (x.to(torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16).double() - x.to(torch.bfloat16).double()
    assert torch.equal(ulp_bf16(x), nxt)


# which probe's bar rejects which defect (test_fault_models_are_rejected asserts this table at every N > 1)
DETECTED_BY = {
    "drop_last": {"selection", "census"},
    "double_last": {"census"},           # the selected key's weight is renormalised: selection cannot see it
    "swap_v": {"selection"},             # the multiset of V rows is unchanged: the census cannot see it
    "l_not_o": {"selection", "census"},
    "q_xor1": {"selection"},             # every census query is the same row
}
fault_record = {}    # (fault, N) -> the set of probes that rejected it, as observed


@pytest.mark.parametrize("fault", FAULTS)
def test_fault_models_are_rejected(fault):
    """An fp64 attention with one defect, its output rounded to bf16 as a kernel would store it, fails the bars of
    tests/test_gpu_attention_exact.py at every tested N > 1: each defect is caught by at least one probe, and by the
    probes DETECTED_BY names (the selection probe with every permutation kind)."""
    assert set(DETECTED_BY) == set(FAULTS)
    for N in ALL_N:
        if N == 1:
            continue
        seen = set()
        by_kind = []
        for kind in PERMS:
            qkv, expected, pi = selection_probe(N, B0, H0, kind)
            out = model_attention(qkv, H0, fault).to(torch.bfloat16)
            by_kind.append(bool(selection_errors(out, qkv, expected, pi)))
        if any(by_kind):
            assert all(by_kind), (fault, N, by_kind)
            seen.add("selection")
        qkv, cnt = census_probe(N, B0, H0)
        if census_errors(model_attention(qkv, H0, fault).to(torch.bfloat16), cnt, N):
            seen.add("census")
        fault_record[(fault, N)] = seen
        assert seen, f"{fault} at N={N} passes both probes"
        assert seen == DETECTED_BY[fault], (fault, N, seen)


def test_failure_messages_name_the_fault():
    """The messages of the two bars: the selection message names pi(i) and the V row actually delivered, the census
    message the residue class and the count seen."""
    N = 41
    qkv, expected, pi = selection_probe(N, B0, H0, "identity")
    msgs = selection_errors(model_attention(qkv, H0, "swap_v").to(torch.bfloat16), qkv, expected, pi)
    assert msgs[1].strip() == "b=0 h=0 i=20: pi(i) = 20, output equals V row 21"
    qkv, cnt = census_probe(N, B0, H0)
    out = model_attention(qkv, H0, "l_not_o").to(torch.bfloat16)
    msgs = census_errors(out, cnt, N)
    assert msgs[1].strip().startswith("b=0 h=0 i=0 d=40 (keys j = 40 mod 64): expected cnt 1 of 41, round(out N) = 0")
    # a pad copy of key N - 1: l is off for every element, the miscounted residue class is named first
    msgs = census_errors(model_attention(qkv, H0, "double_last").to(torch.bfloat16), cnt, N)
    assert msgs[1].strip().startswith("b=0 h=0 i=0 d=40 (keys j = 40 mod 64): expected cnt 1 of 41, round(out N) = 2")
    out[1, 5, 2 * HD + 3] = float("nan")
    assert any("b=1 h=2 i=5 d=3" in m for m in census_errors(out, cnt, N, limit=10 ** 6))
