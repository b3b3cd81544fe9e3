"""CPU: pin the MX-fp8 oracle (oracle/mx8.py) — e4m3 encoding against the OCP value table and torch's own
float8_e4m3fn cast, the block-exponent rule on known answers, and the scale-plane layout."""
import numpy as np
import pytest
import torch

from oracle import mx8


def test_e4m3_table_known_values():
    t = mx8.e4m3_value_table()
    assert t[0x38] == 1.0 and t[0x7E] == 448.0 and t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6
    assert t[0xB8] == -1.0 and t[0x00] == 0.0 and np.isnan(t[0x7F]) and np.isnan(t[0xFF])
    assert t[0x3C] == 1.5 and t[0x30] == 0.5 and t[0x07] == 7 * 2.0 ** -9


def test_e4m3_encode_round_trips_every_finite_code():
    t = mx8.e4m3_value_table()
    codes = np.array([b for b in range(256) if np.isfinite(t[b]) and b != 0x80])   # -0 encodes as +0's sign bit
    assert np.array_equal(mx8.e4m3_encode(t[codes]), codes.astype(np.uint8))


def test_e4m3_encode_matches_torch_cast():
    rng = np.random.default_rng(0)
    t = mx8.e4m3_value_table()
    pos = np.sort(t[np.isfinite(t) & (t >= 0)])
    ties = (pos[:-1] + pos[1:]) / 2                  # exactly half-way between neighbouring codes: to even
    x = np.concatenate([rng.uniform(-448, 448, 20000), rng.normal(0, 1e-2, 20000), rng.normal(0, 1e-3, 5000),
                        ties, -ties, [448.0, -448.0, 0.0]])
    x = x[np.abs(x) <= 448].astype(np.float32)
    ref = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = mx8.e4m3_encode(x)
    assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:10]


@pytest.mark.parametrize("amax,E", [(1.0, -8), (1.75, -8), (1.7578125, -7), (448.0, 0), (450.0, 1), (3e38, 120),
                                    (0.0, -127), (1e-39, -127)])
def test_block_exponent_known_answers(amax, E):
    bits = (np.array([amax], np.float32).view(np.uint32) >> 16).astype(np.int64) & 0x7FFF
    assert int(mx8.block_exponent(bits)[0]) == E
    if amax > 0:   # no element saturates, and the top of the block uses the top binade
        assert amax * 2.0 ** -E <= 448.0


def test_quantize_dequantize_error_bound():
    rng = np.random.default_rng(1)
    x = (rng.normal(size=(37, 256)) * np.exp2(rng.integers(-30, 30, (37, 1)))).astype(np.float32)
    bits = (x.view(np.uint32) >> 16).astype(np.uint16)              # truncate to bf16 (any bf16 will do)
    xb = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    codes, sc = mx8.quantize(bits)
    d = mx8.dequantize(codes, sc)
    ulp_floor = np.repeat(np.exp2(sc - 127.0 - 9), 32, axis=1)      # subnormal step of the block
    assert np.all(np.abs(d - xb) <= np.abs(xb) * 2.0 ** -4 + ulp_floor)


def test_scale_planes_layout():
    rows, K, lds = 130, 256, 192
    sb = np.arange(rows * (K // 32)).reshape(rows, K // 32) % 251
    planes = mx8.pack_scales(sb, lds).view(np.uint8).reshape(-1)
    for r in (0, 15, 16, 63, 64, 129):
        for kb in range(K // 32):
            assert planes[mx8.scale_byte_index(r, kb * 32, lds)] == sb[r, kb]
    # a GEMM lane (brick row r16, K-block fq) finds its 4 fragments' scales in one word
    w = planes.view(np.uint32)
    r16, fq = 5, 2
    word = int(w[0 * lds + 64 + fq * 16 + r16])     # brick 1 (rows 64..127), plane 0
    assert [(word >> (8 * f)) & 0xFF for f in range(4)] == [sb[64 + 16 * f + r16, fq] for f in range(4)]


# ---- exact-routing operands (shared with tests/test_gpu_mx8.py, which imports this module) -------------------------
# Every dequantised value is a signed power of two and one operand has a single nonzero per row, so every output of
# the GEMM is exactly one product +-2^(g + e): exact in fp32 and in bf16, whatever the accumulation order. A scale byte
# or an element taken from the wrong fragment, K-block, brick or K-tile then changes bits, not a tolerance.

ROUTING_SHAPES = [(300, 320, 512), (300, 320, 128), (394, 64, 384), (5, 128, 256)]   # (M, N, K)


def _pow2_bits(exp, neg):
    """bf16 bit patterns of +-2^exp (normal range)."""
    exp = np.asarray(exp, dtype=np.int64)
    return (((exp + 127) << 7) | (np.asarray(neg, dtype=np.int64) << 15)).astype(np.uint16)


def routing_dense(rows, K, seed):
    """(bf16 bits, float64 values) [rows][K]: per (row, 32-block) an exponent uniform in [-8, 8], per element a
    further offset in [-3, 0] and a random sign."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-8, 9, (rows, K // 32))
    ex = np.repeat(e, 32, axis=1) + rng.integers(-3, 1, (rows, K))
    neg = rng.integers(0, 2, (rows, K)).astype(bool)
    return _pow2_bits(ex, neg), np.where(neg, -1.0, 1.0) * np.exp2(ex.astype(np.float64))


def routing_onehot(rows, K, c, seed):
    """(bf16 bits, float64 values, k) : row m holds the single value 2^g(m), g in [-8, 8], at k(m) = (37 m + c) % K."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-8, 9, rows)
    k = (37 * np.arange(rows) + c) % K
    bits = np.zeros((rows, K), dtype=np.uint16)
    val = np.zeros((rows, K))
    bits[np.arange(rows), k] = _pow2_bits(g, False)
    val[np.arange(rows), k] = np.exp2(g.astype(np.float64))
    return bits, val, k


def routing_offsets(rows, K):
    """Offsets c of the repeated one-hot operands: repetition j selects k = 37 (m + j rows) % K, so ceil(K / rows)
    repetitions select every k in [0, K) (37 is coprime to K = 2^a 3^b)."""
    return [37 * rows * j for j in range(-(-K // rows))]


def routing_pairs(M, N, K, onehot):
    """The operand pairs of one shape: `onehot` = "a" (one-hot A x dense W: every W element and W scale byte is the
    factor of some output) or "w" (dense A x one-hot W). Yields (a_bits, a_val, w_bits, w_val, k) per repetition."""
    if onehot == "a":
        w_bits, w_val = routing_dense(N, K, 1000 + N + K)
        for j, c in enumerate(routing_offsets(M, K)):
            a_bits, a_val, k = routing_onehot(M, K, c, 2000 + j)
            yield a_bits, a_val, w_bits, w_val, k
    else:
        a_bits, a_val = routing_dense(M, K, 3000 + M + K)
        for j, c in enumerate(routing_offsets(N, K)):
            w_bits, w_val, k = routing_onehot(N, K, c, 4000 + j)
            yield a_bits, a_val, w_bits, w_val, k


@pytest.mark.parametrize("M,N,K", ROUTING_SHAPES)
@pytest.mark.parametrize("onehot", ["a", "w"])
def test_routing_operands_make_bit_equality_fair(M, N, K, onehot):
    """The bar tests/test_gpu_mx8.py sets for the kernel (bf16 bits equal to oracle gemm) is exact arithmetic: the
    oracle's MX8 form of the operands holds the intended powers of two, every output is one product that is its own
    bf16 rounding, the scale bytes are heterogeneous, and the one-hot positions cover every k."""
    seen = np.zeros(K, dtype=bool)
    for a_bits, a_val, w_bits, w_val, k in routing_pairs(M, N, K, onehot):
        seen[k] = True
        ac, asc = mx8.quantize(a_bits)
        wc, wsc = mx8.quantize(w_bits)
        assert np.array_equal(mx8.dequantize(ac, asc), a_val)
        assert np.array_equal(mx8.dequantize(wc, wsc), w_val)
        dense_sc, hot_sc, hot_val = (wsc, asc, a_val) if onehot == "a" else (asc, wsc, w_val)
        assert len(np.unique(dense_sc)) >= 12
        zero_block = ~(hot_val.reshape(hot_val.shape[0], K // 32, 32) != 0).any(axis=2)
        assert zero_block.sum() == hot_val.shape[0] * (K // 32 - 1) and np.all(hot_sc[zero_block] == 0)
        ref = mx8.gemm(ac, asc, wc, wsc)
        assert np.all(ref != 0) and np.all(np.abs(ref) == np.exp2(np.round(np.log2(np.abs(ref)))))
        rounded = torch.from_numpy(ref).to(torch.bfloat16).double().numpy()
        assert np.array_equal(rounded, ref)
    assert seen.all()
