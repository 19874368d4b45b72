"""Operands and the fp64 reference of grouped_matmul_bf16_nvf4_bf16_tn: weights dequantised in fp64 (e2m1 x e4m3, one scale per 16 elements), fp64 matmul, alpha, one
rounding to bf16; tables, packing and the reference loop are tests/_w4a16_model.py's.  The exact regime: tokens multiples of 1/8, codes of 1/2, EXACT_SCALES of 1/8, so
every product is a multiple of q = 2^-7; while sum |terms| < 2^24 q = 2^17 per output any fp32 summation order is exact.  With |w| <= 6 x 2.5 = 15 that needs
amax <= 2^17 / (15 K), at most 16: exact_problem().  assert_exact() checks the condition on the operands themselves."""
import numpy as np
import torch

from _w4a16_model import E2M1, W4A16, bf16_bits, groups, pack_e2m1, reference_f64, to_bf16_bits, unpack_e2m1  # noqa: F401

E4M3 = torch.float8_e4m3fn
FINITE = np.array([b for b in range(256) if b & 0x7F != 0x7F], np.uint8)   # the 254 finite e4m3 bytes, both zeros among them
EXACT_SCALES = np.array([0.75, 1.0, 1.125, 1.5, 1.875, 2.5, -1.25])        # e4m3 values that use the mantissa and both signs, multiples of 1/8
COUNTS = [0, 1, 31, 32, 33, 0, 65, 64, 2]
# (K, N): both forms run one slot per wave up to K = 512, two up to 1024, rings of two beyond -- either side of every rung, 3200 (every ring wraps three times); ragged N
LADDER = [(K, 40) for K in (128, 512, 640, 1024, 1152, 3200)] + [(640, N) for N in (8, 24, 72)]


class NvW4A16(W4A16):
    """host copies of one problem: x (M, K) bf16 bits, b (E, N, K/2) packed e2m1, sfb (E, N, K/16) e4m3 bytes; x_f64() is the MXFP4 problem's"""
    def __init__(self, x, b, sfb):
        self.x, self.b, self.sfb = np.ascontiguousarray(x, np.uint16), np.ascontiguousarray(b, np.uint8), np.ascontiguousarray(sfb, np.uint8)
        (self.M, self.K), (self.E, self.N) = self.x.shape, self.b.shape[:2]
        assert self.b.shape[2] * 2 == self.K and self.sfb.shape == (self.E, self.N, self.K // 16)

    def b_f64(self):
        return E2M1[unpack_e2m1(self.b)] * np.repeat(torch.from_numpy(self.sfb).view(E4M3).float().numpy().astype(np.float64), 16, axis=-1)   # 0x7f / 0xff: NaN

    def device(self, dev):
        x, b, sf = super().device(dev)
        return x, b, sf.view(torch.uint8).view(E4M3)


def assert_exact(p, counts, x=None):
    X, B = p.x_f64() if x is None else x, p.b_f64()
    assert np.array_equal(X * 8, np.round(X * 8)) and np.array_equal(B * 16, np.round(B * 16)) and np.abs(B).max() <= 15
    assert all((np.abs(X[s:e]) @ np.abs(B[g]).T).max() < 2.0 ** 17 for g, s, e in groups(counts) if e > s), "sum |terms| < 2^24 quanta of 2^-7"


def exact_problem(E, N, K, M, seed):
    """tokens multiples of 1/8 in [-amax(K), amax(K)], any of the 16 codes, scales from EXACT_SCALES drawn per 16-group"""
    rng = np.random.default_rng(seed)
    a8 = int(min(16.0, 2.0 ** 17 / (15 * K)) * 8)   # amax in eighths
    x = rng.integers(-a8, a8 + 1, (M, K)) / 8.0
    sfb = torch.from_numpy(EXACT_SCALES[rng.integers(0, len(EXACT_SCALES), (E, N, K // 16))]).to(E4M3).view(torch.uint8).numpy()
    return NvW4A16(bf16_bits(x), pack_e2m1(rng.integers(0, 16, (E, N, K)).astype(np.uint8)), sfb)


def ladder_case(K, N):
    """-> the problem (5 rows past offs[E-1]), alpha (powers of two), the unsorted tokens, src_row (a permutation, two indices outside [0, T)), the sorted tokens as seen"""
    p = exact_problem(len(COUNTS), N, K, sum(COUNTS) + 5, seed=K + N)
    src = np.random.default_rng(K).permutation(p.M).astype(np.int32)
    unsorted, seen = np.empty_like(p.x), p.x_f64()
    unsorted[src] = p.x
    src[[3, p.M // 2]] = (-1, p.M + 3)
    seen[[3, p.M // 2]] = 0.0
    return p, np.ldexp(1.0, np.arange(p.E) % 5 - 2), unsorted, src, seen


def every_byte_problem(E, M=256, N=32, K=256):
    """one-hot tokens (x[j, j] = 1) in E equal groups against weights whose (N, K/16) scale table carries all 254 finite bytes -- the same table in every expert, so the
    groups the E experts' rows read out (columns j / 16 of expert j / (M / E)) are together the whole table --, every group all 16 codes in its own permutation"""
    codes = np.random.default_rng(E).permuted(np.tile(np.arange(16, dtype=np.uint8), (E, N, K // 16, 1)), axis=-1).reshape(E, N, K)
    return NvW4A16(bf16_bits(np.eye(M, K)), pack_e2m1(codes), np.tile(np.resize(FINITE, N * K // 16).reshape(N, K // 16), (E, 1, 1)))
