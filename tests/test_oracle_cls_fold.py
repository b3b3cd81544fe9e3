"""CPU: exactly computable inputs for the folded CLS attention k_cls_attn_fold (csrc/cls_attn.hip; shared with
tests/test_gpu_cls_fold_exact.py, which imports this module), the proof that the bars set on them are fair, and the
proof that those bars reject a wrong kernel.

The kernel computes, per particle b and head h over the N token rows x_t (bf16, D = 64 H columns), with the row
statistics taken from H planes of {sum, sumsq} (mean_t = s1 / D, rstd_t = rsq(s2 / D - mean_t^2 + eps)):
  s_t = (rstd_t (x_t . G_h - mean_t sum(G_h)) + c0_h) / 8,  c0_h = q_h . bk_h,   p = softmax_t(s),
  out[b][h][:] = sum_t p_t (x_t - mean_t) rstd_t
in chunks of 16 rows: the score dot split over four waves (a quarter of the columns each), an online softmax with a
lazy rescale (the reference maximum m moves only when a chunk's maximum exceeds it by more than 8 in the exp2
domain), weights w_t = bf16(p_t rstd_t), corr = sum_t w_t mean_t from the same rounded weights, and one reciprocal
of l = sum_t p_t at the end. The planes are an input of their own: a probe chooses every row's mean and rstd
exactly, whatever the row holds.

Selection probe (bit equality). In the LN domain the rows are small integers z[t][i]; the stored row is
m_t + z_t 2^k_t with the planes saying mean = m_t, rstd = 2^-k_t (s1 = D m_t, s2 = D (4^k_t + m_t^2), spread unevenly
over the H planes: plane j holds the share (64 + 2 j - (H - 1)) / D, so a dropped or doubled plane moves the
statistic). Head h owns four score columns, one in each wave's quarter (score_cols), G_h = 2^12 there and 0 elsewhere.
On them z = 0 for the selected token pi[b][h]; every other token t has z = -1 on exactly one of the four, the one of
wave (t + h) % 4: its score is 2^12 lower, 739 in the exp2 domain, and every wave's partial is needed to see it.
Elsewhere z is an odd integer in [-99, 99]. Expected: out[b][h][:] holds the bits of z[pi[b][h]][:]. Why equality is
fair: every product and sum of the score is an integer below 2^24 (exact in fp32 in any order); the selected token's
score equals the chunk maximum, so its p = exp2(0) = 1 (to the 2 ulps of v_exp_f32) and w = bf16(2^-k (1 +- 1e-6)) =
2^-k; every other p is exp2(<= -200) = 0 once the selected token has been seen, and the rescale that its chunk
triggers has alpha = exp2(<= -200) = 0, which wipes the finite l, corr and u of the chunks before; then u - corr =
2^-k (m + z 2^k) - 2^-k m = z exactly, l = 1 +- 2 ulps, and z (1 +- 4 ulps) rounds back to the bf16 value z.
Statistics kinds: `unit` (m = 0, k = 0) and `varied` (m an even integer in [-4, 4], nonzero at every selected token,
or an omitted corr would be invisible there; k in {0, 1, 2}). Selection kinds: `first` (pi = 0), `last` (pi = N - 1:
the partial tail chunk; every head sees an alpha = 0 wipe of finite state), `spread` (pi differs per (b, h); for
N >= 16 every row-in-chunk position 0..15 is selected for every H: the LDS swizzle r & 15 and the transposed read).
The bias variant gives q, bk with an exact c0_h of 2, 4 or 6: the same for every token, so the output bits must not
move.

Census probe (one bf16 ulp). G = 0: every token ties, every p = 1. z[t][d] = 1 if (t + b) % 64 == d % 64 else 0, so
out[b][h][d] = cnt / N with cnt <= 10; l = N, u - corr = cnt exactly in fp32 in any order (w = 2^-k, and the sums of
m 2^-k are small dyadic numbers), what remains is one reciprocal, one multiply and one bf16 rounding: |out - cnt / N|
< ulp_bf16(cnt / N), and exactly 0 where cnt = 0. A token dropped at a chunk edge, counted twice, or a pad row let
through (the next particle's row 0) moves a count by at least 10 %. The varied kind checks corr.

Staircase probe (fractional rescales, derived tolerance). Integer rows with statistics planes that are consistent
with them, eps = 1e-6, G = 80 on the score columns. Per head the chunk maxima rise in steps of more than 8 (exp2
domain) at a set of chunks of its own, with spikes of less than 8 in between (no rescale; p reaches about 2^6
against the stale m) and, for every other head, a rise in the last chunk. The builder replays the lazy rule in fp64
on the LN-domain scores and asserts that every head rescales at least twice with 0 < alpha < 1, at the chunks
planned, that no comparison cm > m + 8 is closer than 1 to its threshold, and that no other head shares the set of
chunks (where the chunk count allows fewer distinct sets than heads, N = 49: four sets, no neighbouring head).
Reference: fp64 U = sum_t p_t LNraw_t. Bar: |out - U| <= 2^-7 sum_t p_t |LNraw_t[d]| + 2^-126: each w_t = bf16(p_t
rstd_t) carries at most 2^-8 relative error, l is summed from the unrounded p, and the output rounding adds at most
2^-8 |U| <= 2^-8 sum p |LNraw|.

model_fold restates the kernel in fp32 in its own order (chunks of 16, four score partials, lazy rescale, bf16
weights, corr, reciprocal), with rsq, exp2 and the reciprocal moved by a chosen number of fp32 ulps (what v_rsq_f32,
v_exp_f32 and v_rcp_f32 document), and optionally with one defect. test_bars_are_fair_* show that it meets the three
bars at every (H, N, kind) with those ulps at -2, 0, +2; test_fault_models_are_rejected shows that every defect in
FAULTS fails the bars named in DETECTED_BY at every N > 1 of that probe's list, outside the exceptions named there."""
import functools
import itertools
import math
import types

import pytest
import torch

HD = 64
CH = 16
LOG2E = 1.4426950408889634
B0 = 3
HEADS = [6, 12, 16]
N_LIST = [1, 15, 16, 17, 31, 32, 33, 48, 49, 197, 256, 257, 512, 513, 577, 640]
STAIR_N = [49, 197, 257, 577, 640]
STATS = ["unit", "varied"]
SELS = ["first", "last", "spread"]
MIN_GAP = 200.0
G_SEL = 4096.0      # 2^12: the selection probe's G on the score columns
G_STAIR = 80.0      # the staircase probe's
_OFF = (1, 6, 11, 12)


# ---- builders -------------------------------------------------------------------------------------------------------

def _gen(tag, N, H, seed=0):
    return torch.Generator().manual_seed(((seed * 7919 + tag) * 4099 + N) * 1009 + H)


def score_cols(H):
    """[H][4] int64: head h's score column in wave w's quarter of D, QD w + 16 h + off, the offset rotated with
    h >> 1 so that over the heads every wave sees all four 8-wide slots of its 32-wide k-steps."""
    QD = 16 * H
    return torch.tensor([[QD * w + 16 * h + _OFF[(w + (h >> 1)) & 3] for w in range(4)] for h in range(H)])


def plane_share(H):
    """[H] float64: the numerators 64 + 2 j - (H - 1) of plane j's share of a row's {sum, sumsq}; they add up to D."""
    s = 64.0 + 2.0 * torch.arange(H, dtype=torch.float64) - (H - 1)
    assert float(s.sum()) == 64.0 * H and len(set(s.tolist())) == H
    return s


def planes_from(m, k, H):
    """Statistics planes f32 [H][B N][2] that say mean = m, rstd = 2^-k (m, k [B][N]) for D = 64 H columns."""
    m, k = m.double().reshape(-1), k.double().reshape(-1)
    sh = plane_share(H)[:, None]
    pl = torch.stack([sh * m[None, :], sh * (4.0 ** k + m * m)[None, :]], -1)
    out = pl.float()
    assert torch.equal(out.double(), pl)
    return out


def _stats(kind, B, N, g, pi=None):
    """(m, k) int64 [B][N]; `varied` makes m nonzero at every selected token."""
    assert kind in STATS
    if kind == "unit":
        return torch.zeros(B, N, dtype=torch.int64), torch.zeros(B, N, dtype=torch.int64)
    m = 2 * torch.randint(-2, 3, (B, N), generator=g)
    k = torch.randint(0, 3, (B, N), generator=g)
    if pi is not None:
        for b in range(B):
            for t in pi[b].tolist():
                if m[b, t] == 0:
                    m[b, t] = 2 if (t + b) % 2 else -4
        assert bool((m.gather(1, pi) != 0).all())
    return m, k


def _spread(B, N, H, g):
    """pi [B][H]: unit u = b H + h selects row-in-chunk position u % 16 (u % N below 16 rows) of a seeded chunk, a
    token not yet taken while one is free."""
    pi = torch.empty(B, H, dtype=torch.int64)
    used = set()
    for u in range(B * H):
        r = u % CH if N >= CH else u % N
        cand = list(range(r, N, CH))
        start = int(torch.randint(0, len(cand), (1,), generator=g))
        cand = cand[start:] + cand[:start]
        free = [t for t in cand if t not in used]
        t = (free or cand)[0]
        used.add(t)
        pi[u // H, u % H] = t
    if N >= CH:
        assert set((pi % CH).flatten().tolist()) == set(range(CH))
    if N >= CH * ((B * H + CH - 1) // CH):
        assert len(used) == B * H
    return pi


def _exact_bf16(x):
    y = x.to(torch.bfloat16)
    assert torch.equal(y.double(), x.double()), "an input is not exact in bf16"
    return y


def _bias_pair(B, H):
    """(q bf16 [B][D], bk f32 [D]) with c0_h = q_h . bk_h = 2, 4, 6 for h % 3 = 0, 1, 2, exactly."""
    j = torch.arange(HD)
    qh = torch.where(j < 4, torch.ones(HD), ((j % 5) - 2).float())
    q = (qh[None, None, :] + torch.zeros(B, H, 1)).clone()
    q[:, :, 4:] += (torch.arange(B)[:, None, None] % 2).float()
    bk = torch.zeros(H, HD)
    bk[:, :4] = 0.5 * (torch.arange(H) % 3 + 1)[:, None].float()
    c0 = (q.double() * bk.double()[None]).sum(-1)
    assert torch.equal(c0, (2.0 * (torch.arange(H) % 3 + 1).double())[None].expand(B, H))
    return _exact_bf16(q.reshape(B, H * HD)), bk.reshape(H * HD)


@functools.lru_cache(maxsize=48)
def selection_probe(N, H, sel="spread", stat="unit", bias=False, B=B0, seed=0):
    """Namespace of tok bf16 [B][N][D], planes f32 [H][B N][2], G bf16 [B][H][D], q bf16 [B][D], bk f32 [D], eps,
    z int16 [B][N][D], pi [B][H], expected bf16 [B][H][D] = z[b, pi[b, h]]. Deterministic from the arguments; the
    tensors are shared, do not write them. `bias` changes q and bk only."""
    assert sel in SELS and stat in STATS
    D = HD * H
    g = _gen(1, N, H, seed)
    pi = {"first": torch.zeros(B, H, dtype=torch.int64), "last": torch.full((B, H), N - 1),
          "spread": _spread(B, N, H, g)}[sel]
    m, k = _stats(stat, B, N, g, pi)
    z = 2 * torch.randint(-50, 50, (B, N, D), generator=g) + 1
    cols = score_cols(H)
    t = torch.arange(N)
    for h in range(H):
        z[:, :, cols[h]] = 0
        z[:, t, cols[h][(t + h) % 4]] = -1
    for b in range(B):
        for h in range(H):
            z[b, pi[b, h], cols[h]] = 0
    tok = _exact_bf16(m[..., None].double() + z.double() * (2.0 ** k.double())[..., None])
    G = torch.zeros(B, H, D)
    for h in range(H):
        G[:, h, cols[h]] = G_SEL
    if bias:
        q, bk = _bias_pair(B, H)
    else:
        q, bk = _bias_pair(B, H)[0], torch.zeros(D)
    # fp64: the selected token scores 0 in the LN domain, every other token MIN_GAP lower in the exp2 domain
    s = torch.einsum("bnd,bhd->bhn", z.double(), G.double()) * 0.125 * LOG2E
    selected = s.gather(-1, pi[..., None])
    assert bool((selected == 0).all())
    if N > 1:
        gap = -s.scatter(-1, pi[..., None], -math.inf).amax(-1).max().item()
        assert gap >= MIN_GAP, f"selection probe N={N} H={H} {sel} {stat}: gap {gap:.1f} < {MIN_GAP}"
    expected = _exact_bf16(torch.stack([z[b, pi[b]] for b in range(B)]).double())
    return types.SimpleNamespace(tok=tok, planes=planes_from(m, k, H), G=_exact_bf16(G), q=q, bk=bk, eps=0.0,
                                 z=z.to(torch.int16), pi=pi, expected=expected, N=N, H=H, m=m, k=k)


def census_counts(N, B, H):
    """cnt [B][D] int64: cnt[b, d] = #{t < N : (t + b) % 64 == d % 64}."""
    t = torch.arange(N)[None, :] + torch.arange(B)[:, None]
    return torch.nn.functional.one_hot(t % HD, HD).sum(1).repeat(1, H)


@functools.lru_cache(maxsize=48)
def census_probe(N, H, stat="unit", B=B0, seed=0):
    """As selection_probe with G = 0, bk = 0 and z the residue indicator; cnt [B][D]: every head's output row of
    particle b must be cnt[b] / N."""
    D = HD * H
    g = _gen(2, N, H, seed)
    m, k = _stats(stat, B, N, g)
    t = torch.arange(N)[None, :, None] + torch.arange(B)[:, None, None]
    z = (t % HD == (torch.arange(D) % HD)[None, None, :]).long()
    tok = _exact_bf16(m[..., None].double() + z.double() * (2.0 ** k.double())[..., None])
    cnt = census_counts(N, B, H)
    assert int(cnt.max()) <= 10 and bool((cnt.view(B, H, HD).sum(-1) == N).all())
    return types.SimpleNamespace(tok=tok, planes=planes_from(m, k, H), G=torch.zeros(B, H, D, dtype=torch.bfloat16),
                                 q=_bias_pair(B, H)[0], bk=torch.zeros(D), eps=0.0, z=z.to(torch.int16), cnt=cnt,
                                 N=N, H=H, m=m, k=k)


def consistent_planes(tok, H):
    """The producers' planes of the rows themselves: plane j = {sum, sumsq} of columns 64 j .. 64 j + 63."""
    B, N, D = tok.shape
    x = tok.double().reshape(B * N, H, HD)
    pl = torch.stack([x.sum(-1), (x * x).sum(-1)], -1).transpose(0, 1).contiguous()   # [H][B N][2]
    out = pl.float()
    assert torch.equal(out.double(), pl)
    return out


STEP, SPIKE = 4, 2      # the staircase's rise and spike in units of the summed score columns


def _rise_sets(nc, H, g):
    """H sorted tuples of chunk indices in 1 .. nc - 1 (two, and for every other head a third: the last chunk)."""
    if nc <= 6:
        cand = [c for r in (2, 3) for c in itertools.combinations(range(1, nc), r)]
        cand.sort(key=lambda c: (nc - 1 not in c, c))
        return [cand[h % len(cand)] for h in range(H)]
    sets = []
    while len(sets) < H:
        a = tuple(sorted((torch.randperm(nc - 2, generator=g)[:2] + 1).tolist()))
        s = a + (nc - 1,) if len(sets) % 2 == 0 else a
        if s not in sets:
            sets.append(s)
    return sets


@functools.lru_cache(maxsize=48)
def staircase_probe(N, H, B=B0, seed=0):
    """Namespace as selection_probe (eps = 1e-6, consistent planes) with U float64 [B][H][D] the fp64 reference, bar
    [B][H][D] its tolerance, and rises[b][h] the chunks at which the kernel's lazy rule rescales with 0 < alpha < 1."""
    D = HD * H
    g = _gen(3, N, H, seed)
    nc = (N + CH - 1) // CH
    sets = _rise_sets(nc, H, g)
    cols = score_cols(H)
    x = torch.zeros(B, N, D, dtype=torch.int64)
    t = torch.arange(N)
    c = t // CH
    rows_in = torch.clamp(N - c * CH, max=CH)                           # valid rows of the token's chunk
    for b in range(B):
        for h in range(H):
            rs = sets[(h + b) % H]
            lev = sum((c >= r).long() for r in rs)
            e = -(1 + (t * 7 + h * 3) % 5)
            rise = (c == 0) | sum((c == r) for r in rs).bool()
            top = (t % CH) == (h * 3 + c + b) % rows_in
            e = torch.where(rise & top, torch.zeros_like(e), e)
            spike = ~rise & ((c + h) % 2 == 0) & ((t % CH) == (h + 5 * c) % rows_in)
            e = torch.where(spike, torch.full_like(e, SPIKE), e)
            S = STEP * lev + e
            for w in range(4):
                x[b, :, cols[h, w]] = S // 4 + ((w + t + h) % 4 < S % 4).long()
    # the other columns: +-v pairs, v a per-row shuffle of one multiset of [-8, 8], then the score columns' sum taken
    # off one by one: every row sums to 0 and has nearly the same sum of squares, so mean = 0 and the LN-domain score
    # is rstd G S with rstd within a few percent of one value
    fill = torch.ones(D, dtype=torch.bool)
    fill[cols.flatten()] = False
    fill = fill.nonzero().flatten()
    F = fill.numel()
    f1, f2 = fill[torch.randperm(F, generator=g)], fill[torch.randperm(F, generator=g)]
    v = (torch.arange(F // 2) % 17 - 8)[torch.rand(B, N, F // 2, generator=g).argsort(-1)]   # one multiset per row
    x[..., f1[:F // 2]] = v
    x[..., f1[F // 2:]] = -v
    r = x.sum(-1, keepdim=True)
    assert int(r.abs().max()) <= F
    x[..., f2] -= (torch.arange(F)[None, None, :] < r.abs()).long() * torch.sign(r)
    assert not bool(x.sum(-1).any())
    tok = _exact_bf16(x.double())
    G = torch.zeros(B, H, D)
    for h in range(H):
        G[:, h, cols[h]] = G_STAIR
    eps = 1e-6
    xd = tok.double()
    mean = xd.mean(-1, keepdim=True)
    ln = (xd - mean) / torch.sqrt((xd * xd).mean(-1, keepdim=True) - mean * mean + eps)
    s = torch.einsum("bnd,bhd->bhn", ln, G.double()) * 0.125 * LOG2E              # exp2 domain, LN-domain scores
    # the kernel's lazy rule, replayed in fp64
    rises = [[[] for _ in range(H)] for _ in range(B)]
    top_pr = -math.inf
    for b in range(B):
        for h in range(H):
            mref = -math.inf
            for ci in range(nc):
                sc = s[b, h, ci * CH:(ci + 1) * CH]
                cm = sc.max().item()
                if mref != -math.inf:
                    assert abs(cm - (mref + 8.0)) >= 1.0, f"staircase N={N} H={H}: chunk {ci} of (b={b}, h={h}) is " \
                        f"{cm - mref - 8.0:+.2f} from the rescale threshold"
                if cm > mref + 8.0:
                    if mref != -math.inf:
                        assert 2.0 ** -100 < 2.0 ** (mref - cm) < 1.0
                        rises[b][h].append(ci)
                    mref = cm
                top_pr = max(top_pr, (sc - mref).max().item())
            assert tuple(rises[b][h]) == sets[(h + b) % H], \
                f"staircase N={N} H={H} (b={b}, h={h}): rescales at {rises[b][h]}, planned {sets[(h + b) % H]}"
            assert len(rises[b][h]) >= 2
    assert 5.0 <= top_pr < 7.5, f"staircase N={N} H={H}: the largest p is 2^{top_pr:.2f}"
    distinct = len(set(sets))
    if distinct == H:
        pass                                    # no other head shares a head's set of rescale chunks
    else:                                       # fewer sets exist than heads (nc = 4): no neighbouring head does
        assert nc <= 6 and all(sets[h] != sets[(h + 1) % H] for h in range(H))
    assert any(nc - 1 in r for r in sets)       # a rise in the (partial) tail chunk
    p = torch.softmax(s * math.log(2.0), -1)
    U = torch.einsum("bhn,bnd->bhd", p, ln)
    bar = 2.0 ** -7 * torch.einsum("bhn,bnd->bhd", p, ln.abs()) + 2.0 ** -126
    return types.SimpleNamespace(tok=tok, planes=consistent_planes(tok, H), G=_exact_bf16(G), q=_bias_pair(B, H)[0],
                                 bk=torch.zeros(D), eps=eps, U=U, bar=bar, rises=rises, sets=sets, N=N, H=H)


# ---- the bars, with messages that name the fault --------------------------------------------------------------------

def _bits(t):
    return t.contiguous().view(torch.int16)


def selection_errors(out, p, limit=4):
    """[] when out [B][H][D] (bf16) holds the bits of p.expected; otherwise one line per mismatching (b, h) (the first
    `limit`) with pi[b][h] and the token row of that particle whose z bits the output does equal, if any."""
    out = out.cpu()
    assert out.dtype == torch.bfloat16 and out.shape == p.expected.shape
    bad = (_bits(out) != _bits(p.expected)).any(-1)
    if not bool(bad.any()):
        return []
    msgs = [f"selection: {int(bad.sum())} of {bad.numel()} (b, h) rows differ from z[pi[b][h]] (N={p.N}, H={p.H})"]
    for b, h in bad.nonzero()[:limit].tolist():
        zb = _bits(p.z[b].to(torch.bfloat16))
        hit = (zb == _bits(out[b, h])[None, :]).all(-1).nonzero().flatten().tolist()
        wrong = (_bits(out[b, h]) != _bits(p.expected[b, h])).nonzero().flatten()
        what = f"equals token row {hit[0]}" if hit else \
            f"equals no token row of the particle ({wrong.numel()} columns differ, first d = {int(wrong[0])}: got " \
            f"{out[b, h, wrong[0]].item()!r}, expected {p.expected[b, h, wrong[0]].item()!r})"
        msgs.append(f"  b={b} h={h}: pi = {int(p.pi[b, h])} (chunk {int(p.pi[b, h]) // CH}, row "
                    f"{int(p.pi[b, h]) % CH}), output {what}")
    return msgs


def ulp_bf16(x):
    """The spacing of bf16 values around x > 0 (float64 tensor): 2^(floor(log2 x) - 7)."""
    _, e = torch.frexp(x)
    return torch.exp2((e - 8).double())


def census_errors(out, p, limit=4):
    """[] when every out[b][h][d] is one of the two bf16 neighbours of cnt[b][d] / N (|diff| < ulp_bf16) and exactly 0
    where cnt = 0; otherwise one line per failing element (the first `limit`), the miscounted ones first."""
    out = out.cpu()
    B, H, D = out.shape
    N = p.N
    got = out.double()
    cnt = p.cnt[:, None, :].expand(B, H, D)
    exact = cnt.double() / N
    ok = (got - exact).abs() < ulp_bf16(exact.clamp_min(2.0 ** -100))
    ok = torch.where(exact == 0, got == 0, ok) & torch.isfinite(got)
    if bool(ok.all()):
        return []
    bad = ~ok
    msgs = [f"census: {int(bad.sum())} of {bad.numel()} outputs off cnt / N (N={N}, H={H})"]
    seen = torch.nan_to_num(got * N, nan=-1.0, posinf=-1.0, neginf=-1.0).round()
    miscounted = bad & (seen != cnt)
    first = torch.cat([miscounted.nonzero()[:limit], (bad & ~miscounted).nonzero()[:limit]])[:limit]
    for b, h, d in first.tolist():
        msgs.append(f"  b={b} h={h} d={d} (tokens t = {(d - b) % HD} mod 64): expected cnt {int(cnt[b, h, d])} of {N}, "
                    f"round(out N) = {int(seen[b, h, d])} (out = {got[b, h, d].item()!r})")
    return msgs


def staircase_errors(out, p, limit=4):
    """[] when |out - U| <= bar everywhere; otherwise the worst (b, h) rows with their ratio to the bar and the chunks
    at which that head rescales. Also returns nothing for a NaN-free pass only: a non-finite output fails."""
    out = out.cpu().double()
    ratio = (out - p.U).abs() / p.bar
    ratio = torch.where(torch.isfinite(out), ratio, torch.full_like(ratio, math.inf))
    if bool((ratio <= 1.0).all()):
        return []
    worst = ratio.amax(-1)
    msgs = [f"staircase: {int((ratio > 1).sum())} of {ratio.numel()} outputs beyond 2^-7 sum p |LNraw| "
            f"(N={p.N}, H={p.H})"]
    for b, h in (worst > 1).nonzero()[:limit].tolist():
        d = int(ratio[b, h].argmax())
        msgs.append(f"  b={b} h={h}: {worst[b, h].item():.3g} x the bar at d={d} (got {out[b, h, d].item()!r}, fp64 "
                    f"{p.U[b, h, d].item()!r}); the head rescales at chunks {p.rises[b][h]}")
    return msgs


def staircase_ratio(out, p):
    """max |out - U| / bar (for the record of how far inside the bar a run sits)."""
    return ((out.cpu().double() - p.U).abs() / p.bar).max().item()


# ---- the kernel restated in fp32, optionally with one defect --------------------------------------------------------

FAULTS = ["drop_wave", "drop_last", "pad_row", "plane_omitted", "corr_omitted", "corr_not_rescaled",
          "l_not_rescaled", "u_not_rescaled", "alpha_neighbour", "g_neighbour"]


def _nudge(x, k):
    """x (fp32, >= 0) moved by k fp32 ulps where it is a normal number."""
    if k == 0:
        return x
    i = x.view(torch.int32)
    return torch.where(torch.isfinite(x) & (i >= 0x00800000), (i + k).view(torch.float32), x)


def model_fold(p, fault=None, ulps=(0, 0, 0)):
    """out bf16 [B][H][D] of k_cls_attn_fold restated in fp32 in the kernel's order; ulps = (rsq, exp2, reciprocal)
    moves those three results by that many fp32 ulps. `fault` plants one defect:
      drop_wave          wave 1's score partial is not summed
      drop_last          token N - 1 is masked as a pad row
      pad_row            row N of a partial tail chunk is taken for a token: the next particle's row 0 and statistics
                         (zeros and the planes' pad after the last particle)
      plane_omitted      plane 1 is left out of the statistics
      corr_omitted       corr is not subtracted
      corr_not_rescaled / l_not_rescaled / u_not_rescaled   that accumulator ignores alpha
      alpha_neighbour    u of head h is rescaled by head h + 1's alpha
      g_neighbour        the score dot of head h reads G of head h + 1"""
    assert fault is None or fault in FAULTS
    f32 = torch.float32
    x = p.tok.float()
    B, N, D = x.shape
    H = D // HD
    nc = (N + CH - 1) // CH
    NP = nc * CH
    pl = torch.cat([p.planes.float(), torch.full((H, 1, 2), math.nan)], 1)       # the planes' pad behind the rows
    n_seen = N
    if fault == "pad_row" and N % CH:
        n_seen = N + 1
    if fault == "drop_last":
        n_seen = N - 1
    xp = torch.zeros(B, NP, D, dtype=f32)
    xp[:, :N] = x
    idx = torch.arange(B)[:, None] * N + torch.arange(NP)[None, :]
    idx = torch.where(torch.arange(NP)[None, :] < max(n_seen, N), idx, torch.full_like(idx, 0)).clamp_max(B * N)
    if n_seen > N:
        xp[:B - 1, N] = x[1:, 0]
    s1 = torch.zeros(B, NP, dtype=f32)
    s2 = torch.zeros(B, NP, dtype=f32)
    for j in range(H):
        if fault == "plane_omitted" and j == 1:
            continue
        s1 = s1 + pl[j, idx, 0]
        s2 = s2 + pl[j, idx, 1]
    inv_d = torch.tensor(1.0, dtype=f32) / D
    mean = s1 * inv_d
    rstd = _nudge(torch.rsqrt(torch.clamp_min(s2 * inv_d - mean * mean, 0.0) + torch.tensor(p.eps, dtype=f32)), ulps[0])
    valid = (torch.arange(NP) < n_seen)[None, :]
    mean = torch.where(valid, mean, torch.zeros_like(mean))
    rstd = torch.where(valid, rstd, torch.zeros_like(rstd))
    Gf = p.G.float()
    gsum = Gf.sum(-1)
    c0 = (p.q.float().view(B, H, HD) * p.bk.float().view(1, H, HD)).sum(-1)
    Gs = Gf.roll(-1, 1) if fault == "g_neighbour" else Gf
    sl2 = torch.tensor(0.125, dtype=f32) * torch.tensor(1.44269504088896341, dtype=f32)
    ninf = torch.tensor(-math.inf, dtype=f32)
    m = torch.full((B, H), -math.inf, dtype=f32)
    l = torch.zeros(B, H, dtype=f32)
    corr = torch.zeros(B, H, dtype=f32)
    u = torch.zeros(B, H, D, dtype=f32)
    for c in range(nc):
        sl = slice(c * CH, (c + 1) * CH)
        xc = xp[:, sl]
        parts = torch.einsum("btwd,bhwd->bhtw", xc.reshape(B, CH, 4, D // 4), Gs.reshape(B, H, 4, D // 4))
        if fault == "drop_wave":
            parts[..., 1] = 0.0
        dot = ((parts[..., 0] + parts[..., 1]) + parts[..., 2]) + parts[..., 3]
        mc, rc, vc = mean[:, None, sl], rstd[:, None, sl], valid[:, None, sl]
        sc = torch.where(vc, (rc * (dot - mc * gsum[..., None]) + c0[..., None]) * sl2, ninf)
        cm = sc.amax(-1)
        fire = cm > m + 8.0
        alpha = torch.where(fire, torch.where(m == ninf, torch.zeros_like(m), _nudge(torch.exp2(m - cm), ulps[1])),
                            torch.ones_like(m))
        m = torch.where(fire, cm, m)
        pr = torch.where(sc == ninf, torch.zeros_like(sc), _nudge(torch.exp2(sc - m[..., None]), ulps[1]))
        wb = (pr * rc).to(torch.bfloat16).float()
        one = torch.ones_like(alpha)
        l = l * (one if fault == "l_not_rescaled" else alpha) + pr.sum(-1)
        corr = corr * (one if fault == "corr_not_rescaled" else alpha) + (wb * mc).sum(-1)
        au = one if fault == "u_not_rescaled" else alpha.roll(-1, 1) if fault == "alpha_neighbour" else alpha
        u = u * au[..., None] + torch.einsum("bht,btd->bhd", wb, xc)
    inv = _nudge(1.0 / l, ulps[2])
    cr = torch.zeros_like(corr) if fault == "corr_omitted" else corr
    return ((u - cr[..., None]) * inv[..., None]).to(torch.bfloat16)


# ---- tests ----------------------------------------------------------------------------------------------------------

ULPS = [(0, 0, 0), (2, 2, 2), (-2, -2, -2), (2, -2, 2), (-2, 2, -2), (2, 2, -2), (-2, -2, 2)]


def _fail(msgs, *ctx):
    assert not msgs, "\n".join([repr(ctx)] + msgs)


@pytest.mark.parametrize("N", N_LIST)
@pytest.mark.parametrize("H", HEADS)
def test_bars_are_fair_selection(H, N):
    """The fp32 restatement, its rsq / exp2 / reciprocal at -2, 0, +2 ulps, delivers z[pi] bit for bit for every
    selection and statistics kind, with and without the bias c0; the builder is deterministic."""
    for sel, stat in itertools.product(SELS, STATS):
        p = selection_probe(N, H, sel, stat)
        assert p.tok.shape == (B0, N, HD * H) and p.planes.shape == (H, B0 * N, 2)
        pb = selection_probe(N, H, sel, stat, True)
        assert torch.equal(pb.tok, p.tok) and torch.equal(pb.expected, p.expected) and bool(pb.bk.any())
        for ulps in ULPS:
            _fail(selection_errors(model_fold(p, None, ulps), p), sel, stat, ulps)
        _fail(selection_errors(model_fold(pb, None, ULPS[3]), pb), sel, stat, "bias")
    again = selection_probe.__wrapped__(N, H, "spread", "varied")
    p = selection_probe(N, H, "spread", "varied")
    assert torch.equal(again.tok, p.tok) and torch.equal(again.pi, p.pi) and torch.equal(again.planes, p.planes)
    if N > 1:
        assert bool((p.m != 0).any()) and bool((p.k != 0).any())


@pytest.mark.parametrize("N", N_LIST)
@pytest.mark.parametrize("H", HEADS)
def test_bars_are_fair_census(H, N):
    """The fp32 restatement meets the strict one-bf16-ulp census bar for both statistics kinds at every ulp setting;
    cnt / N rounded from the exact value does too."""
    for stat in STATS:
        p = census_probe(N, H, stat)
        exact = (p.cnt.double() / N)[:, None, :].expand(B0, H, HD * H)
        _fail(census_errors(exact.to(torch.bfloat16), p), stat, "exact")
        for ulps in ULPS:
            _fail(census_errors(model_fold(p, None, ulps), p), stat, ulps)


stair_record = {}    # (H, N, ulps) -> max |out - U| / bar of the restatement


@pytest.mark.parametrize("N", STAIR_N)
@pytest.mark.parametrize("H", HEADS)
def test_bars_are_fair_staircase(H, N):
    """The fp32 restatement sits inside the derived staircase bar at every ulp setting (the builder has asserted the
    rescale pattern); the fp64 reference rounded to bf16 sits inside half of it."""
    p = staircase_probe(N, H)
    assert staircase_ratio(p.U.to(torch.bfloat16), p) <= 0.5
    for ulps in ULPS:
        out = model_fold(p, None, ulps)
        stair_record[(H, N, ulps)] = staircase_ratio(out, p)
        _fail(staircase_errors(out, p), ulps)


def test_ulp_bf16():
    x = torch.tensor([1.0, 1.5, 0.5, 0.75, 10 / 640, 1 / 3], dtype=torch.float64)
    nxt = (x.to(torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16).double() - x.to(torch.bfloat16).double()
    assert torch.equal(ulp_bf16(x), nxt)


def test_score_columns_reach_every_slot():
    """Per H: the score columns are distinct, one per (head, wave) in that wave's quarter; together they reach every
    32-wide k-step of every wave, and every wave sees all four 8-wide slots."""
    for H in HEADS:
        cols = score_cols(H)
        QD = 16 * H
        assert cols.unique().numel() == 4 * H
        assert torch.equal(cols // QD, torch.arange(4).expand(H, 4))
        for w in range(4):
            within = cols[:, w] - QD * w
            assert set((within // 32).tolist()) == set(range(H // 2))
            assert set(((within % 32) // 8).tolist()) == {0, 1, 2, 3}


# Which probe (and kinds) must reject which defect at every N > 1 of its list, for every H. A probe named here is
# asserted; the exceptions name the (fault, probe) cells that cannot see the defect at some N, and why.
DETECTED_BY = {
    "drop_wave": [("selection", "first", "unit"), ("selection", "spread", "varied"), ("staircase",)],
    "drop_last": [("selection", "last", "unit"), ("census", "unit")],
    "pad_row": [("census", "unit"), ("census", "varied")],
    "plane_omitted": [("selection", "spread", "unit"), ("census", "unit"), ("census", "varied")],
    "corr_omitted": [("selection", "first", "varied"), ("selection", "spread", "varied"), ("census", "varied")],
    "corr_not_rescaled": [("selection", "last", "varied")],
    "l_not_rescaled": [("selection", "last", "unit"), ("staircase",)],
    "u_not_rescaled": [("selection", "last", "unit"), ("staircase",)],
    "alpha_neighbour": [("staircase",)],
    "g_neighbour": [("selection", "spread", "unit"), ("staircase",)],
}
EXCEPTIONS = {
    # a whole number of chunks has no pad row in any chunk the kernel visits
    ("pad_row", "census"): lambda N: N % CH == 0,
    # the last token is in chunk 0: no state exists to rescale
    ("corr_not_rescaled", "selection"): lambda N: N <= CH,
    ("l_not_rescaled", "selection"): lambda N: N <= CH,
    ("u_not_rescaled", "selection"): lambda N: N <= CH,
}


def _rejects(case, N, H, fault):
    if case[0] == "selection":
        p = selection_probe(N, H, case[1], case[2])
        return bool(selection_errors(model_fold(p, fault), p))
    if case[0] == "census":
        p = census_probe(N, H, case[1])
        return bool(census_errors(model_fold(p, fault), p))
    p = staircase_probe(N, H)
    return bool(staircase_errors(model_fold(p, fault), p))


@pytest.mark.parametrize("fault", FAULTS)
def test_fault_models_are_rejected(fault):
    """The restatement with one defect fails every bar DETECTED_BY names for it, at every N > 1 of that probe's list
    and every H, except where EXCEPTIONS says the defect cannot show."""
    assert set(DETECTED_BY) == set(FAULTS)
    for case in DETECTED_BY[fault]:
        skip = EXCEPTIONS.get((fault, case[0]), lambda N: False)
        for H in HEADS:
            for N in (STAIR_N if case[0] == "staircase" else N_LIST):
                if N == 1 or skip(N):
                    continue
                assert _rejects(case, N, H, fault), f"{fault} passes {case} at N={N} H={H}"


def test_blind_spots_that_the_kinds_exist_for():
    """Why the varied statistics and the staircase are there: with m = 0 everywhere an omitted corr changes nothing,
    and when every head selects the same token all heads share one alpha, so the neighbour's is as good as its own."""
    for H in HEADS:
        for N in (17, 197):
            for sel in SELS:
                assert not _rejects(("selection", sel, "unit"), N, H, "corr_omitted")
            assert not _rejects(("census", "unit"), N, H, "corr_omitted")
            for sel in ("first", "last"):
                assert not _rejects(("selection", sel, "varied"), N, H, "alpha_neighbour")


def test_rescale_faults_are_gross_on_the_staircase():
    """The rescale defects miss the staircase bar by orders of magnitude, the correct restatement sits well inside."""
    for H in HEADS:
        p = staircase_probe(197, H)
        assert staircase_ratio(model_fold(p), p) <= 1.0
        for fault in ("l_not_rescaled", "u_not_rescaled", "alpha_neighbour"):
            assert staircase_ratio(model_fold(p, fault), p) > 100.0, (fault, H)


def test_failure_messages_name_the_fault():
    """The selection message names (b, h), pi and the token row delivered; the census message the residue class and
    the count seen; the staircase message the head's rescale chunks."""
    p = selection_probe(49, 6, "spread", "unit")
    msgs = selection_errors(model_fold(p, "g_neighbour"), p)
    assert msgs[1].strip() == f"b=0 h=0: pi = {int(p.pi[0, 0])} (chunk {int(p.pi[0, 0]) // 16}, row " \
        f"{int(p.pi[0, 0]) % 16}), output equals token row {int(p.pi[0, 1])}"
    p = census_probe(49, 6, "unit")
    msgs = census_errors(model_fold(p, "drop_last"), p)
    assert msgs[1].strip().startswith("b=0 h=0 d=48 (tokens t = 48 mod 64): expected cnt 1 of 49, round(out N) = 0")
    msgs = census_errors(model_fold(p, "pad_row"), p)
    assert "b=0 h=0 d=1 (tokens t = 1 mod 64): expected cnt 1 of 49, round(out N) = 2" in msgs[1]
    p = staircase_probe(49, 6)
    msgs = staircase_errors(model_fold(p, "u_not_rescaled"), p)
    assert "the head rescales at chunks" in msgs[1] and msgs[1].strip().startswith("b=0 h=0:")


# ---- cls_g_weight ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", HEADS)
def test_cls_g_weight(H):
    """vit.cls_g_weight(Wk, H) is the block-diagonal [H D][D] weight with q W_G^T = einsum("bhd,hdi->bhi", q, Wk) on
    integer weights, exactly; it keeps Wk's dtype, is contiguous, and is zero off the blocks."""
    from vitparticlefiltertracker_amd.vit import cls_g_weight
    D = HD * H
    g = _gen(4, 0, H)
    Wk = torch.randint(-8, 9, (D, D), generator=g).to(torch.bfloat16)
    q = torch.randint(-8, 9, (B0, D), generator=g).double()
    wg = cls_g_weight(Wk, H)
    assert wg.shape == (H * D, D) and wg.dtype == torch.bfloat16 and wg.is_contiguous()
    ref = torch.einsum("bhd,hdi->bhi", q.view(B0, H, HD), Wk.double().view(H, HD, D))
    assert torch.equal((q @ wg.double().t()).view(B0, H, D), ref)
    blocks = wg.view(H, D, H, HD)
    for h in range(H):
        assert torch.equal(blocks[h, :, h], Wk[HD * h:HD * h + HD].t())
        assert not bool(blocks[h, :, torch.arange(H) != h].any())
    assert cls_g_weight(Wk.float(), H).dtype == torch.float32
