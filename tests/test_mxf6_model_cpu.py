"""The numpy model of the MXFP6 (e2m3) format, quantizer rule and W4A6 reference (tests/_mxf6_model.py) against the properties the contract states -- CPU only.
The GPU tests hold the kernels to this model byte for byte, so what is pinned here is what the kernels are held to."""
import numpy as np
import torch

import _mxf6_model as m
import _mxf8_quant_model as m8


def test_table_and_every_e2m3_value_is_an_e4m3_value():
    assert m.E2M3.shape == (64,) and m.E2M3[0] == 0 and np.signbit(m.E2M3[32]) and m.E2M3[32] == 0
    assert m.E2M3[1] == 0.125 and m.E2M3[7] == 0.875 and m.E2M3[8] == 1.0 and m.E2M3[15] == 1.875 and m.E2M3[16] == 2.0 and m.E2M3[24] == 4.0 and m.E2M3[31] == 7.5
    assert np.array_equal(m.E2M3[32:], -m.E2M3[:32]) and (np.diff(m.E2M3[:32]) > 0).all() and np.isfinite(m.E2M3).all()   # no NaN, no infinity
    assert m.E2M3[m.HOT_CODE] == -1.625
    e4 = m8.decode(np.arange(256, dtype=np.uint8), "e4m3")
    assert np.isin(m.E2M3, e4).all()
    assert np.array_equal(m.e4m3_bytes(m.E2M3[:32]).astype(np.int64) & 0x7f, torch.from_numpy(m.E2M3[:32].astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy())


def test_pack_unpack_round_trip_and_the_bit_layout():
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 64, (5, 7, 128)).astype(np.uint8)
    packed = m.pack_e2m3(codes)
    assert packed.shape == (5, 7, 96) and packed.dtype == np.uint8 and np.array_equal(m.unpack_e2m3(packed), codes)
    # element k occupies bits 6 k .. 6 k + 5 of the row read as one little-endian bit string
    row = codes[2, 3]
    bits = np.unpackbits(packed[2, 3], bitorder="little")
    for k in (0, 1, 2, 3, 4, 31, 32, 77, 127):
        assert int(np.packbits(bits[6 * k:6 * k + 6], bitorder="little")[0]) == row[k], k
    # a 32-element scale block is the 24 bytes 24 j .. 24 j + 23
    assert np.array_equal(m.unpack_e2m3(packed[..., 24:48]), codes[..., 32:64])
    one = np.zeros(128, np.uint8)
    one[5] = 0x3F
    assert np.flatnonzero(m.pack_e2m3(one)).tolist() == [3, 4] and m.pack_e2m3(one)[3] == 0xC0 and m.pack_e2m3(one)[4] == 0x0F


def _group(vals, top=4.0):
    g = np.zeros(32, np.float32)
    g[:len(vals)] = vals
    g[31] = top
    return g


def test_every_tie_goes_to_the_even_code_and_saturation():
    mags = m.E2M3[:32]
    mids = (mags[:-1] + mags[1:]) / 2
    for sign in (1.0, -1.0):
        for lo in range(0, 31, 16):
            part = mids[lo:lo + 16]
            codes, e8 = m.quantize(_group(sign * part))
            assert e8.tolist() == [127]
            c = codes[:len(part)].astype(np.int64)
            assert ((c & 1) == 0).all(), "a tie that went to an odd code"
            assert ((c >> 5) == (sign < 0)).all()
            below, above = np.arange(lo, lo + len(part)), np.arange(lo, lo + len(part)) + 1
            assert np.array_equal(c & 31, np.where(below % 2 == 0, below, above))
    # just off a tie: to the nearer neighbour
    codes, _ = m.quantize(_group([0.0625 + 2.0 ** -10, 0.0625 - 2.0 ** -10, 7.25 + 2.0 ** -6, 7.25 - 2.0 ** -6]))
    assert codes[:4].tolist() == [1, 0, 31, 30]
    # (7.5, 8) -> 7.5, both signs; the scaled maximum lies in [4, 8)
    codes, e8 = m.quantize(_group([7.5, 7.51, 7.75, 7.999, -7.999, -7.5], top=7.9999))
    assert e8.tolist() == [127] and codes[:6].tolist() == [31, 31, 31, 31, 63, 63] and codes[31] == 31
    for amax in (1e-30, 0.37, 1.0, 5.0, 3e38):
        y = _group([], top=amax)
        _, e8 = m.quantize(y)
        assert 4.0 <= np.float64(np.float32(amax)) * 2.0 ** (127 - int(e8[0])) < 8.0


def test_signed_zero_nan_inf_zero_and_denormal_groups():
    y = _group([-0.0, 0.0, -2.0 ** -30, 2.0 ** -30], top=1.0)
    codes, e8 = m.quantize(y)
    assert e8.tolist() == [125] and codes[:4].tolist() == [32, 0, 32, 0] and codes[31] == 24    # -0 and negatives that round to zero keep their sign
    z = np.zeros(32, np.float32)
    z[3] = -0.0
    codes, e8 = m.quantize(z)
    assert e8.tolist() == [127] and codes[3] == 32 and not np.delete(codes, 3).any()           # amax == 0 -> 127
    for bad in (np.nan, np.inf, -np.inf):
        y = np.concatenate([_group([1.0, -2.0, bad]), _group([1.0, -2.0, 3.0])]).astype(np.float32)
        codes, e8 = m.quantize(y)
        assert e8.tolist() == [255, 127] and not codes[:32].any() and codes[32:35].tolist() == [8, 48, 20]   # the NaN travels in the scale byte; the next group is untouched
        assert np.isnan(m.dequantize(codes, e8)[:32]).all() and np.isfinite(m.dequantize(codes, e8)[32:]).all()
    allnan = np.full(32, np.nan, np.float32)
    assert m.quantize(allnan)[1].tolist() == [255]
    den = np.zeros(32, np.float32)
    den[:3] = [2.0 ** -130, -2.0 ** -140, 2.0 ** -149]
    codes, e8 = m.quantize(den)
    assert e8.tolist() == [0] and codes[:3].tolist() == [1, 32, 0]                              # E - 2 < 0 clamps to 0: 2^-130 x 2^127 = 1/8
    big = np.zeros(32, np.float32)
    big[0] = np.float32(3.4e38)
    assert m.quantize(big)[1].tolist() == [252]


def test_round_trip_of_every_code_and_scale():
    rng = np.random.default_rng(1)
    codes = rng.integers(0, 64, (64, 64)).astype(np.uint8)
    codes[:, 31::32] = 31                       # the group's maximum at 7.5: the scale byte comes back
    codes[codes == 32] = 0
    e8 = rng.integers(3, 250, (64, 2)).astype(np.uint8)
    y = m.dequantize(codes, e8)
    c2, e2 = m.quantize(y.astype(np.float32))
    assert np.array_equal(e2, e8) and np.array_equal(c2, codes)


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _sim(x, wd):
    """relative Frobenius errors of x_q @ wd^T against x @ wd^T for e2m3 (this rule), e4m3 (fusedQuantizeMxf8's rule), e2m1 (abs-max scale, RNE on the e2m1 grid) and
    the saturation share of the e2m3 rule"""
    x32 = x.astype(np.float32)
    ref = x @ wd.T
    c6, s6 = m.quantize(x32)
    x6 = m.dequantize(c6, s6.reshape(x.shape[0], -1))
    c8, s8 = m8.quantize(x32, "e4m3")
    x8 = m8.dequantize(c8, s8, "e4m3")
    g = x.reshape(x.shape[0], -1, 32)
    amax = np.abs(g).max(-1, keepdims=True)
    sc = 2.0 ** (np.floor(np.log2(amax)) - 2)                       # the OCP MX rule for e2m1: the scaled maximum in [4, 8), saturating at 6
    grid = m.E2M1[:8]
    t = np.minimum(np.abs(g) / sc, 6.0)
    idx = np.abs(t[..., None] - grid).argmin(-1)                     # (ties: the error's size does not depend on the side)
    x4 = (np.sign(g) * grid[idx] * sc).reshape(x.shape)
    scaled = np.abs(x) * 2.0 ** (127 - np.repeat(s6.reshape(x.shape[0], -1).astype(np.int64), 32, axis=-1))
    return _rel(x6 @ wd.T, ref), _rel(x8 @ wd.T, ref), _rel(x4 @ wd.T, ref), float((scaled > 7.5).mean())


def _mxfp4_weights(w):
    g = w.reshape(w.shape[0], -1, 32)
    amax = np.abs(g).max(-1, keepdims=True)
    sc = 2.0 ** (np.floor(np.log2(amax)) - 2)
    grid = m.E2M1[:8]
    t = np.minimum(np.abs(g) / sc, 6.0)
    return (np.sign(g) * grid[np.abs(t[..., None] - grid).argmin(-1)] * sc).reshape(w.shape)


def test_simulation_e2m3_tokens_lose_less_than_half_of_what_e2m1_tokens_lose():
    rng = np.random.default_rng(2026)
    x = torch.from_numpy(rng.standard_normal((64, 512)).astype(np.float32)).to(torch.bfloat16).double().numpy()
    wd = _mxfp4_weights(rng.standard_normal((256, 512)))
    e6, e8, e4, sat = _sim(x, wd)
    print(f"simulation: e2m3 {e6:.4f}, e4m3 {e8:.4f}, e2m1 {e4:.4f}; {100 * sat:.2f} % of the e2m3 elements saturate")
    assert e6 < e4 / 2, (e6, e4)
    assert 0.02 < e6 < 0.04 and 0.02 < e8 < 0.04 and 0.08 < e4 < 0.16 and sat < 0.01


def test_the_gpu_point_tests_own_data_keeps_the_margin():
    """tests/test_gpu_grouped_w4a6.py's 64 tokens and weights (CPU-generated, fixed seed) through the CPU model: the factor the GPU test asserts (2) is met with room"""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("_w4a6_gpu_point", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_grouped_w4a6.py"))
    src = open(spec.origin).read()
    ns = {"torch": torch}
    exec(src[src.index("def point_inputs"):src.index("def test_w4a6_is_far_closer")], ns)   # the generator alone: the module's imports need the lab library
    x, w = ns["point_inputs"]()
    e6, e8, e4, _ = _sim(x.double().numpy(), _mxfp4_weights(3.0 * w.double().numpy()))        # (fusedQuantizeMx's abs-max codes sit at three times the value)
    print(f"the GPU test's data on the CPU model: e6 {e6:.4f}, e8 {e8:.4f}, e4 {e4:.4f}")
    assert e6 < e4 / 3, (e6, e4)


def test_exact_problems_are_exact_at_every_k_the_gpu_tests_use():
    for K in (128, 512, 640, 1024, 1152, 1536, 1664, 2048, 2176, 3584, 3712, 7296):
        p = m.exact_problem(3, 40, K, 64, seed=K, a_vals="both" if K <= 2176 else "e2m1")
        m.assert_exact(p, [33, 0, 31])
        assert np.array_equal(m.unpack_e2m3(p.a).shape, (64, K))
    counts = [0, 1, 31, 32, 33, 0, 65, 64, 2]
    for N in (8, 24, 40, 72):
        m.assert_exact(m.exact_problem(9, N, 640, sum(counts), seed=N), counts)
    p = m.exact_problem(9, 72, 640, sum(counts), seed=4)
    assert np.array_equal(m8.decode(p.a_as_e4m3(), "e4m3"), p.a_vals())                       # the re-encoding the W4A8 cross-check uses is value for value
    p2 = m.exact_problem(9, 72, 640, sum(counts), seed=5, a_vals="e2m1")
    assert np.array_equal(m.E2M1[m.unpack_e2m1(p2.a_as_e2m1())], p2.a_vals())
    for K, shift in ((128, 0), (256, 0), (256, 128)):
        p = m.one_hot_problem(K, shift)
        m.assert_exact(p, [p.M])
        assert (m.unpack_e2m3(p.a) != 0).sum() == p.M and set(np.unique(m.unpack_e2m3(p.a))) == {0, m.HOT_CODE}
