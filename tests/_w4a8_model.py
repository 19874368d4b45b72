"""Operands and the fp64 reference of the W4A8 grouped GEMM (grouped_matmul_mxf8_mxf4_bf16_tn), built on the CPU with numpy / torch: the CPU oracle has no mixed
kind, so the tests of that op dequantise A (e4m3 x e8m0) and B (e2m1 x e8m0) in fp64, multiply in fp64, scale by alpha and round once to bf16.

The exact regime: every operand value is a multiple of a known quantum, so every product is a multiple of one quantum q, and while sum |terms| < 2^24 q per output
every partial sum in any order is an integer multiple of q below 2^24 q -- exact in fp32.  Then the fp32 result of ANY summation order equals the fp64 reference bit
for bit, and so does its bf16 rounding.  assert_exact() checks that on the operands themselves."""
import numpy as np
import torch

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], np.float64)   # code -> value
POS7 = np.array([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], np.float64)                                                           # the seven positive e2m1 values
EXACT_VALS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0], np.float64)                 # in e2m1 and in e4m3
E4M3_ONLY = np.array([1.25, 1.75, 0.875, 2.5, 3.5, -1.25, -1.75, -0.875, -2.5, -3.5], np.float64)                         # in e4m3, not in e2m1
E4, E8M0 = torch.float8_e4m3fn, torch.float8_e8m0fnu
SF_LO, SF_HI = 125, 129   # scale bytes of the exact regime


def e2m1_codes(vals):
    """values (all in the e2m1 table, -0 never produced) -> 4-bit codes"""
    vals = np.asarray(vals, np.float64)
    codes = np.zeros(vals.shape, np.uint8)
    hit = np.zeros(vals.shape, bool)
    for c in (0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15):
        m = vals == E2M1[c]
        codes[m] = c
        hit |= m
    assert hit.all(), "a value outside the e2m1 table"
    return codes


def pack_e2m1(codes):
    """(.., K) codes -> (.., K/2) bytes: element 2 j in the low nibble, 2 j + 1 in the high nibble of byte j"""
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).astype(np.uint8)


def unpack_e2m1(packed):
    out = np.empty(packed.shape[:-1] + (packed.shape[-1] * 2,), np.uint8)
    out[..., 0::2] = packed & 0xF
    out[..., 1::2] = packed >> 4
    return out


def e4m3_bytes(vals):
    """values exactly representable in e4m3 -> their bytes"""
    t = torch.from_numpy(np.asarray(vals, np.float32)).to(E4)
    assert np.array_equal(t.float().numpy().astype(np.float64), np.asarray(vals, np.float64)), "a value outside e4m3"
    return t.view(torch.uint8).numpy()


def scale_f64(sf):
    """e8m0 bytes -> 2^(b - 127) in fp64, byte 255 -> NaN"""
    s = np.ldexp(1.0, sf.astype(np.int64) - 127)
    return np.where(sf == 255, np.nan, s)


class W4A8:
    """host copies of one problem: a (M, K) e4m3 bytes, b (E, N, K/2) packed e2m1, sfa (M, K/32), sfb (E, N, K/32) e8m0 bytes"""

    def __init__(self, a, b, sfa, sfb):
        self.a, self.b, self.sfa, self.sfb = (np.ascontiguousarray(x, np.uint8) for x in (a, b, sfa, sfb))
        self.M, self.K = self.a.shape
        self.E, self.N = self.b.shape[:2]
        assert self.b.shape[2] * 2 == self.K and self.sfa.shape == (self.M, self.K // 32) and self.sfb.shape == (self.E, self.N, self.K // 32)

    def a_f64(self):
        v = torch.from_numpy(self.a).view(E4).float().numpy().astype(np.float64)
        return v * np.repeat(scale_f64(self.sfa), 32, axis=-1)

    def b_f64(self):
        return E2M1[unpack_e2m1(self.b)] * np.repeat(scale_f64(self.sfb), 32, axis=-1)

    def device(self, dev):
        t = lambda x, dt: torch.from_numpy(x).to(dev).view(dt)
        return t(self.a, E4), torch.from_numpy(self.b).to(dev), t(self.sfa.reshape(-1), E8M0), t(self.sfb.reshape(-1), E8M0)

    def b_as_e4m3(self):
        """the weights upcast to e4m3 bytes (E, N, K): exact, every e2m1 value is an e4m3 value"""
        return e4m3_bytes(E2M1[unpack_e2m1(self.b)])

    def a_as_e2m1(self):
        """the tokens re-encoded as packed e2m1 (M, K/2): only when every A value is in the e2m1 table"""
        return pack_e2m1(e2m1_codes(torch.from_numpy(self.a).view(E4).float().numpy()))


def groups(counts):
    o = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [(g, int(o[g]), int(o[g + 1])) for g in range(len(counts))]


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


def to_bf16_bits(ref64):
    """one rounding to bf16 (fp64 -> fp32 is exact in the exact regime); int16 view of the bits"""
    return torch.from_numpy(ref64).to(torch.float32).to(torch.bfloat16).view(torch.int16)


def assert_exact(p, counts):
    """every product a multiple of one quantum q, sum |terms| < 2^24 q per output: fp32 sums in any order are exact"""
    A, B = p.a_f64(), p.b_f64()
    av = torch.from_numpy(p.a).view(E4).float().numpy()
    qa = (2.0 ** -1 if np.array_equal(av * 2, np.round(av * 2)) else 2.0 ** -3) * 2.0 ** (int(p.sfa.min()) - 127)   # the e4m3-only values used here are multiples of 1/8 ...
    qb = 2.0 ** -1 * 2.0 ** (int(p.sfb.min()) - 127)                                                                  # ... e2m1 values multiples of 1/2
    assert np.array_equal(A / qa, np.round(A / qa)) and np.array_equal(B / qb, np.round(B / qb))
    q = qa * qb
    for g, s, e in groups(counts):
        if e > s:
            assert (np.abs(A[s:e]) @ np.abs(B[g]).T).max() < 2.0 ** 24 * q, (g, "the exact regime needs sum |terms| < 2^24 q")


def exact_problem(E, N, K, M, seed, a_vals="both", p_only=0.25):
    """exact-regime operands: B from EXACT_VALS, A from EXACT_VALS with E4M3_ONLY mixed in (a_vals = "both") or EXACT_VALS alone ("e2m1"); scale bytes 125 ... 129
    drawn independently per 32-block"""
    rng = np.random.default_rng(seed)
    av = EXACT_VALS[rng.integers(0, len(EXACT_VALS), (M, K))]
    if a_vals == "both":
        only = rng.random((M, K)) < p_only
        av = np.where(only, E4M3_ONLY[rng.integers(0, len(E4M3_ONLY), (M, K))], av)
    bv = EXACT_VALS[rng.integers(0, len(EXACT_VALS), (E, N, K))]
    sfa = rng.integers(SF_LO, SF_HI + 1, (M, K // 32)).astype(np.uint8)
    sfb = rng.integers(SF_LO, SF_HI + 1, (E, N, K // 32)).astype(np.uint8)
    return W4A8(e4m3_bytes(av), pack_e2m1(e2m1_codes(bv)), sfa, sfb)


def one_hot_problem(K, shift, M=128, N=32):
    """token row j is zero except a[j, shift + j] = 1; b[n, k] = POS7[(n + k) % 7]; every (row, block) has its own scale byte"""
    a = np.zeros((M, K), np.float64)
    a[np.arange(M), shift + np.arange(M)] = 1.0
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    bv = POS7[(n + k) % 7][None]
    r, blk = np.meshgrid(np.arange(M), np.arange(K // 32), indexing="ij")
    sfa = (SF_LO + (r + 2 * blk) % 5).astype(np.uint8)
    n2, blk2 = np.meshgrid(np.arange(N), np.arange(K // 32), indexing="ij")
    sfb = (SF_LO + (3 * n2 + blk2) % 5).astype(np.uint8)[None]
    return W4A8(e4m3_bytes(a), pack_e2m1(e2m1_codes(bv)), sfa, sfb)
