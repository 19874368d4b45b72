"""Operands and the fp64 reference of the W4A16 grouped GEMM (grouped_matmul_bf16_mxf4_bf16_tn: bf16 tokens against MXFP4 expert weights), built on the CPU with
numpy / torch.  The reference dequantises B (e2m1 x e8m0) in fp64, multiplies in fp64, scales by alpha and rounds once to bf16; the tables and the packing are
tests/_w4a8_model.py's.

The exact regime, as there: every token value is a multiple of qa and every weight value a multiple of qb, so every product is a multiple of one quantum q = qa qb,
and while sum |terms| < 2^24 q per output every partial sum in any order is an integer multiple of q below 2^24 q -- exact in fp32.  Then the fp32 result of ANY
summation order equals the fp64 reference bit for bit, and so does its bf16 rounding.  assert_exact() checks that on the operands themselves.  Tokens are multiples of
1/8 that bf16 holds exactly (|v| <= amax, 8 significant bits), weights e2m1 values under scale bytes 125 ... 129; exact_problem() narrows the tokens' range as K
grows so that the assert holds."""
import numpy as np
import torch

from _w4a8_model import E2M1, EXACT_VALS, POS7, SF_HI, SF_LO, e2m1_codes, groups, pack_e2m1, scale_f64, to_bf16_bits, unpack_e2m1  # noqa: F401

E8M0 = torch.float8_e8m0fnu
# the cases of tests/test_gpu_grouped_w4a16.py whose operands tests/test_grouped_w4a16_cpu.py asserts exact.  A stage is 128 K elements; the 32-row forms (606, 607) run
# one shot with 1, 2, 3 slots per wave (K <= 512, 1024, 1536) and rings of 3 slots beyond, the 64-row form (608) one shot up to K = 1024 and rings of 2 slots beyond:
# the K on either side of every rung, the first ring K of either ladder (1152, 1664) and 3200 (25 stages: a ring of 3 slots wraps twice, one of 2 slots three times)
LADDER_K = (128, 512, 640, 1024, 1152, 1536, 1664, 3200)
LADDER_COUNTS = [33, 0, 31]
RAGGED_N = (8, 24, 40, 72)
RAGGED_COUNTS = [0, 1, 31, 32, 33, 0, 65, 64, 2]
ONE_HOT = ((128, 0), (256, 0), (256, 128))


def bf16_bits(vals):
    """values bf16 holds exactly -> their bits (uint16)"""
    t = torch.from_numpy(np.asarray(vals, np.float32)).to(torch.bfloat16)
    assert np.array_equal(t.float().numpy().astype(np.float64), np.asarray(vals, np.float64)), "a value outside bf16"
    return t.view(torch.int16).numpy().view(np.uint16)


class W4A16:
    """host copies of one problem: x (M, K) bf16 bits (uint16), b (E, N, K/2) packed e2m1, sfb (E, N, K/32) e8m0 bytes"""

    def __init__(self, x, b, sfb):
        self.x = np.ascontiguousarray(x, np.uint16)
        self.b, self.sfb = np.ascontiguousarray(b, np.uint8), np.ascontiguousarray(sfb, np.uint8)
        self.M, self.K = self.x.shape
        self.E, self.N = self.b.shape[:2]
        assert self.b.shape[2] * 2 == self.K and self.sfb.shape == (self.E, self.N, self.K // 32)

    def x_f64(self):
        return torch.from_numpy(self.x.view(np.int16)).view(torch.bfloat16).float().numpy().astype(np.float64)

    def b_f64(self):
        return E2M1[unpack_e2m1(self.b)] * np.repeat(scale_f64(self.sfb), 32, axis=-1)

    def device(self, dev):
        return (torch.from_numpy(self.x.view(np.int16)).to(dev).view(torch.bfloat16), torch.from_numpy(self.b).to(dev),
                torch.from_numpy(self.sfb.reshape(-1)).to(dev).view(E8M0))


def reference_f64(p, counts, alpha=None, x=None):
    """(M, N) fp64: alpha[g] x_r (B_g . SFB_g)^T for the rows of group g; rows past sum(counts) stay 0.  x: the sorted tokens where they are not p's own (gather)"""
    X, B = p.x_f64() if x is None else x, p.b_f64()
    out = np.zeros((X.shape[0], p.N), np.float64)
    al = np.ones(p.E) if alpha is None else np.broadcast_to(np.asarray(alpha, np.float64), (p.E,))
    with np.errstate(invalid="ignore", over="ignore"):
        for g, s, e in groups(counts):
            if e > s:
                out[s:e] = (X[s:e] @ B[g].T) * al[g]
    return out


def assert_exact(p, counts, qa=2.0 ** -3, x=None):
    """every product a multiple of one quantum q = qa qb, sum |terms| < 2^24 q per output: fp32 sums in any order are exact.  Non-finite weights (scale byte 255)
    are left out: their outputs are NaN in any order"""
    X, B = p.x_f64() if x is None else x, p.b_f64()
    fin = np.where(np.isfinite(B), B, 0.0)
    qb = 2.0 ** -1 * 2.0 ** (int(p.sfb[p.sfb != 255].min()) - 127)   # e2m1 values are multiples of 1/2
    assert np.array_equal(X / qa, np.round(X / qa)) and np.array_equal(fin / qb, np.round(fin / qb))
    q = qa * qb
    for g, s, e in groups(counts):
        if e > s:
            assert (np.abs(X[s:e]) @ np.abs(fin[g]).T).max() < 2.0 ** 24 * q, (g, "the exact regime needs sum |terms| < 2^24 q")


def token_amax(K):
    """the tokens' range for an inner dimension K: multiples of 1/8 up to amax, all exact in bf16 (amax <= 16: at most 8 significant bits).  The worst sum of
    |terms| is K amax x 4 x 2^2 (|e2m1 value| <= 4 here, scale bytes <= 129) against 2^24 q = 2^24 x 2^-3 x 2^-3 = 2^18: amax <= 2^14 / K"""
    return float(min(16.0, 2.0 ** 14 / K))


def exact_tokens(rng, M, K):
    amax = token_amax(K)
    return rng.integers(-int(amax * 8), int(amax * 8) + 1, (M, K)).astype(np.float64) / 8.0


def exact_problem(E, N, K, M, seed):
    """exact-regime operands: tokens multiples of 1/8 in [-amax(K), amax(K)], B from EXACT_VALS, scale bytes 125 ... 129 drawn independently per 32-block"""
    rng = np.random.default_rng(seed)
    bv = EXACT_VALS[rng.integers(0, len(EXACT_VALS), (E, N, K))]
    sfb = rng.integers(SF_LO, SF_HI + 1, (E, N, K // 32)).astype(np.uint8)
    return W4A16(bf16_bits(exact_tokens(rng, M, K)), pack_e2m1(e2m1_codes(bv)), sfb)


def one_hot_problem(K, shift, M=128, N=32):
    """token row j is zero except x[j, shift + j] = 1; b[n, k] = POS7[(n + k) % 7]: neighbouring k never share a value; every (column, block) has its own scale byte"""
    x = np.zeros((M, K), np.float64)
    x[np.arange(M), shift + np.arange(M)] = 1.0
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    bv = POS7[(n + k) % 7][None]
    n2, blk2 = np.meshgrid(np.arange(N), np.arange(K // 32), indexing="ij")
    sfb = (SF_LO + (3 * n2 + blk2) % 5).astype(np.uint8)[None]
    return W4A16(bf16_bits(x), pack_e2m1(e2m1_codes(bv)), sfb)
