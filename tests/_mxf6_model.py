"""The MXFP6 (e2m3) operand format, the contract of the MXFP6 rotate-and-quantize ops (fusedQuantizeMxf6, fusedGatherQuantizeMxf6) and the fp64 reference of the W4A6
grouped GEMM (grouped_matmul_mxf6_mxf4_bf16_tn) in numpy -- a plain module, CPU only.

Format: a row of K elements is 3 K / 4 bytes; element k occupies bits 6 k .. 6 k + 5 of the row read as one little-endian bit string (a 32-element scale block is the
24 bytes 24 j .. 24 j + 23).  A code is sign (bit 5), 2 exponent bits (bias 1), 3 mantissa bits: m / 8 for exponent 0, (1 + m / 8) 2^(e - 1) otherwise, up to 7.5.

Quantizer, per 32 consecutive y = x_group @ h (fp32 values; `rotate` of _mxf8_quant_model gives them where the products are exact):
    amax = max |y|, NaNs ignored;  E = biased exponent field of the fp32 amax
    e8   = 255 if any y is NaN or infinite (all 32 codes 0), 127 if amax == 0, else clamp(E - 2, 0, 254)
    q    = min(RNE(|y| 2^(127 - e8)) on the e2m3 grid, 7.5) with the sign of y: ties to the even code, -0 and negatives that round to zero keep their sign

GEMM, the exact regime: as tests/_w4a8_model.py -- every product a multiple of one quantum q and sum |terms| < 2^24 q per output, so fp32 sums in any order equal the
fp64 reference bit for bit.  The e2m3 quantum is 1/8; the value sets are those of the W4A8 model (every one an e2m3 value), so the same K bounds hold."""
import numpy as np
import torch

from _mxf8_quant_model import bf16_to_f64, rotate  # noqa: F401  (re-exported for the tests)
from _w4a8_model import (E2M1, E4M3_ONLY, E8M0, EXACT_VALS, POS7, SF_HI, SF_LO, e2m1_codes, e4m3_bytes, groups, pack_e2m1, scale_f64, to_bf16_bits,  # noqa: F401
                         unpack_e2m1)


def _e2m3_table():
    t = np.empty(64, np.float64)
    for c in range(64):
        e, m = (c >> 3) & 3, c & 7
        mag = m / 8.0 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1)
        t[c] = -mag if c & 32 else mag
    return t


E2M3 = _e2m3_table()        # code -> value; code 32 is -0
E2M3_MAX = 7.5
HOT_CODE = 0x2D             # 1 01 101: -(1 + 5/8) = -1.625, all three fields mixed


def pack_e2m3(codes):
    """(.., K) 6-bit codes -> (.., 3 K / 4) bytes: four codes c0 .. c3 are the 24-bit little-endian word c0 | c1 << 6 | c2 << 12 | c3 << 18"""
    c = np.asarray(codes, np.uint32)
    assert c.shape[-1] % 4 == 0 and (c < 64).all()
    c = c.reshape(*c.shape[:-1], c.shape[-1] // 4, 4)
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    out = np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], axis=-1).astype(np.uint8)
    return out.reshape(*out.shape[:-2], -1)


def unpack_e2m3(packed):
    p = np.asarray(packed, np.uint8).astype(np.uint32)
    assert p.shape[-1] % 3 == 0
    p = p.reshape(*p.shape[:-1], p.shape[-1] // 3, 3)
    w = p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)
    out = np.stack([(w >> (6 * i)) & 63 for i in range(4)], axis=-1).astype(np.uint8)
    return out.reshape(*out.shape[:-2], -1)


def e2m3_codes(vals):
    """values exactly in the e2m3 table (-0 never produced) -> codes"""
    vals = np.asarray(vals, np.float64)
    codes = np.zeros(vals.shape, np.uint8)
    hit = np.zeros(vals.shape, bool)
    for c in range(64):
        if c == 32:
            continue
        m = vals == E2M3[c]
        codes[m] = c
        hit |= m
    assert hit.all(), "a value outside the e2m3 table"
    return codes


def round_e2m3(scaled):
    """fp64 magnitudes-with-sign -> codes: RNE on the e2m3 grid (ties to the even code), saturating at 7.5, the sign bit of the input kept (also on zero)"""
    s = np.asarray(scaled, np.float64)
    a = np.minimum(np.abs(s), E2M3_MAX)
    ex = np.floor(np.log2(np.maximum(a, 1.0)))                 # 0 below 2, 1 below 4, 2 below 8
    step = np.ldexp(1.0, ex.astype(np.int64) - 3)
    n = np.rint(a / step)                                      # numpy rounds half to even; a / step is exact (a power-of-two divisor)
    code = (n + 8 * ex).astype(np.int64)                       # n = 16 carries into the next exponent as it should
    assert (code >= 0).all() and (code <= 31).all()
    return (code | (np.signbit(s).astype(np.int64) << 5)).astype(np.uint8)


def scale_bytes(y):
    """y (.., 32 n) fp32 values -> e8 (.., n) uint8"""
    y32 = np.ascontiguousarray(y, dtype=np.float32)
    assert np.array_equal(y32.astype(np.float64), np.asarray(y, dtype=np.float64), equal_nan=True), "y must hold fp32 values"
    g = y32.reshape(*y32.shape[:-1], y32.shape[-1] // 32, 32)
    amax = np.fmax.reduce(np.abs(g), axis=-1, initial=np.float32(0))   # fmax: NaNs ignored
    E = (amax.view(np.uint32) >> 23).astype(np.int64) & 0xff
    e8 = np.where(amax == 0, 127, np.clip(E - 2, 0, 254))
    return np.where(~np.isfinite(g).all(axis=-1), 255, e8).astype(np.uint8)


def quantize(y):
    """y (.., 32 n) fp32 values -> (codes (.., 32 n) uint8 6-bit, e8 (.., n) uint8)"""
    e8 = scale_bytes(y)
    e8r = np.repeat(e8.astype(np.int64), 32, axis=-1)
    poison = e8r == 255
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = np.where(poison, 0.0, np.asarray(y, np.float64)) * np.ldexp(1.0, 127 - np.where(poison, 127, e8r))
        # the kernel's multiply is fp32: exact unless the product falls below 2^-126, far under half the smallest step, where both round to a signed zero
        scaled = scaled.astype(np.float32).astype(np.float64)
    codes = round_e2m3(scaled)
    return np.where(poison, 0, codes).astype(np.uint8), e8


def dequantize(codes, e8):
    """fp64 values of the quantized operand: code value * 2^(e8 - 127), NaN under scale byte 255"""
    return E2M3[codes] * np.repeat(scale_f64(np.asarray(e8, np.uint8)), 32, axis=-1)


class W4A6:
    """host copies of one problem: a (M, 3 K / 4) packed e2m3, b (E, N, K / 2) packed e2m1, sfa (M, K / 32), sfb (E, N, K / 32) e8m0 bytes"""

    def __init__(self, a, b, sfa, sfb):
        self.a, self.b, self.sfa, self.sfb = (np.ascontiguousarray(x, np.uint8) for x in (a, b, sfa, sfb))
        self.M = self.a.shape[0]
        self.K = self.a.shape[1] * 4 // 3
        self.E, self.N = self.b.shape[:2]
        assert self.a.shape[1] * 4 == self.K * 3 and self.b.shape[2] * 2 == self.K
        assert self.sfa.shape == (self.M, self.K // 32) and self.sfb.shape == (self.E, self.N, self.K // 32)

    def a_vals(self):
        return E2M3[unpack_e2m3(self.a)]

    def a_f64(self):
        return self.a_vals() * np.repeat(scale_f64(self.sfa), 32, axis=-1)

    def b_f64(self):
        return E2M1[unpack_e2m1(self.b)] * np.repeat(scale_f64(self.sfb), 32, axis=-1)

    def device(self, dev):
        t = lambda x, dt: torch.from_numpy(x).to(dev).view(dt)
        return torch.from_numpy(self.a).to(dev), torch.from_numpy(self.b).to(dev), t(self.sfa.reshape(-1), E8M0), t(self.sfb.reshape(-1), E8M0)

    def a_as_e4m3(self):
        """the tokens re-encoded as e4m3 bytes (M, K): exact, every e2m3 value is an e4m3 value"""
        return e4m3_bytes(self.a_vals())

    def a_as_e2m1(self):
        """the tokens re-encoded as packed e2m1 (M, K / 2): only when every A value is in the e2m1 table"""
        return pack_e2m1(e2m1_codes(self.a_vals()))


def reference_f64(p, counts, alpha=None):
    """(M, N) fp64: alpha[g] (A_r . SFA_r)(B_g . SFB_g)^T for the rows of group g; rows past sum(counts) stay 0"""
    A, B = p.a_f64(), p.b_f64()
    out = np.zeros((p.M, p.N), np.float64)
    al = np.ones(p.E) if alpha is None else np.broadcast_to(np.asarray(alpha, np.float64), (p.E,))
    with np.errstate(invalid="ignore"):
        for g, s, e in groups(counts):
            if e > s:
                out[s:e] = (A[s:e] @ B[g].T) * al[g]
    return out


def assert_exact(p, counts):
    """every product a multiple of one quantum q, sum |terms| < 2^24 q per output: fp32 sums in any order are exact"""
    A, B = p.a_f64(), p.b_f64()
    av = p.a_vals()
    qa = (2.0 ** -1 if np.array_equal(av * 2, np.round(av * 2)) else 2.0 ** -3) * 2.0 ** (int(p.sfa.min()) - 127)   # e2m3 values are multiples of 1/8 ...
    qb = 2.0 ** -1 * 2.0 ** (int(p.sfb.min()) - 127)                                                                  # ... e2m1 values multiples of 1/2
    assert np.array_equal(A / qa, np.round(A / qa)) and np.array_equal(B / qb, np.round(B / qb))
    q = qa * qb
    for g, s, e in groups(counts):
        if e > s:
            assert (np.abs(A[s:e]) @ np.abs(B[g]).T).max() < 2.0 ** 24 * q, (g, "the exact regime needs sum |terms| < 2^24 q")


def exact_problem(E, N, K, M, seed, a_vals="both", p_only=0.25):
    """exact-regime operands: B from EXACT_VALS, A from EXACT_VALS with the multiples of 1/8 of E4M3_ONLY (all e2m3 values) mixed in (a_vals = "both") or EXACT_VALS
    alone ("e2m1": multiples of 1/2, for the longer K); scale bytes 125 ... 129 drawn independently per 32-block"""
    rng = np.random.default_rng(seed)
    av = EXACT_VALS[rng.integers(0, len(EXACT_VALS), (M, K))]
    if a_vals == "both":
        only = rng.random((M, K)) < p_only
        av = np.where(only, E4M3_ONLY[rng.integers(0, len(E4M3_ONLY), (M, K))], av)
    bv = EXACT_VALS[rng.integers(0, len(EXACT_VALS), (E, N, K))]
    sfa = rng.integers(SF_LO, SF_HI + 1, (M, K // 32)).astype(np.uint8)
    sfb = rng.integers(SF_LO, SF_HI + 1, (E, N, K // 32)).astype(np.uint8)
    return W4A6(pack_e2m3(e2m3_codes(av)), pack_e2m1(e2m1_codes(bv)), sfa, sfb)


def one_hot_problem(K, shift, M=128, N=32, hot=HOT_CODE):
    """token row j is zero except code `hot` at K index shift + j; b[n, k] = POS7[(n + k) % 7]; every (row, block) has its own scale byte"""
    codes = np.zeros((M, K), np.uint8)
    codes[np.arange(M), shift + np.arange(M)] = hot
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    bv = POS7[(n + k) % 7][None]
    r, blk = np.meshgrid(np.arange(M), np.arange(K // 32), indexing="ij")
    sfa = (SF_LO + (r + 2 * blk) % 5).astype(np.uint8)
    n2, blk2 = np.meshgrid(np.arange(N), np.arange(K // 32), indexing="ij")
    sfb = (SF_LO + (3 * n2 + blk2) % 5).astype(np.uint8)[None]
    return W4A6(pack_e2m3(codes), pack_e2m1(e2m1_codes(bv)), sfa, sfb)
