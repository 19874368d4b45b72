"""The numpy model of the gpt-oss ops (swiglu_oai_and_mul, moe_combine with a bias) on bf16 BIT PATTERNS (uint16): the judge of tests/test_gpu_swiglu_oai.py and
tests/test_gpu_moe_combine_bias.py.  No torch ops.  s, the one transcendental, is evaluated in fp64 and rounded to bf16 ONCE; every other step is the np.float32
operation the contract names (one add, one multiply, no fma), rounded to bf16 to nearest-even where the contract rounds."""
import numpy as np


def bf16_to_f32(bits) -> np.ndarray:
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def bf16_to_f64(bits) -> np.ndarray:
    with np.errstate(invalid="ignore"):   # (a signalling NaN among the bit patterns)
        return bf16_to_f32(bits).astype(np.float64)


def f32_to_bf16(v) -> np.ndarray:
    """np.float32 -> bf16 bits, round-to-nearest-even (finite values; inf stays inf)"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def f64_to_bf16(v) -> np.ndarray:
    """fp64 (or longdouble) -> bf16 bits, round-to-nearest-even in ONE rounding: the 8-bit significand at v's own exponent, the subnormal quantum 2^-133 below 2^-126"""
    v = np.asarray(v)
    sign = np.signbit(v).astype(np.uint16) << 15
    a = np.abs(v)
    fin = np.isfinite(a) & (a > 0)
    m, e = np.frexp(np.where(fin, a, 1.0))                       # a = m * 2^e, m in [0.5, 1)
    e = np.maximum(e, -125)
    quant = np.ldexp(np.ones_like(a), e - 8)
    r = np.rint(np.where(fin, a, 0.0) / quant) * quant           # ties to even; the division is by a power of two (exact)
    with np.errstate(over="ignore"):
        r32 = r.astype(np.float32)                               # exactly representable, or inf as bf16 overflows
    out = np.where(fin, (r32.view(np.uint32) >> 16).astype(np.uint16), np.uint16(0))
    out = np.where(np.isinf(a), np.uint16(0x7f80), out)
    out = np.where(np.isnan(a), np.uint16(0x7fc0), out)
    return (out | sign).astype(np.uint16)


def group_of_rows(offs, rows) -> np.ndarray:
    """g(r) = min(E - 1, #{g : offs[g] <= r}) for non-decreasing offs"""
    offs = np.asarray(offs)
    return np.minimum(np.searchsorted(offs, np.asarray(rows), side="right"), len(offs) - 1)


def sigmoid_gate(gc_bits, alpha, dtype=np.float64) -> np.ndarray:
    """the real number gc / (1 + exp(-alpha * gc)) evaluated in `dtype` (fp64 or longdouble); alpha is the fp32 value, the product is exact in either"""
    g = bf16_to_f32(gc_bits).astype(dtype)
    a = dtype(np.float32(alpha))
    with np.errstate(over="ignore"):
        return g / (dtype(1) + np.exp(-a * g))


def swiglu_oai(x_bits, alpha=1.702, limit=7.0, bias_bits=None, offs=None) -> np.ndarray:
    """x (.., 2 I) bf16 bits [gate | up] -> act (.., I) bf16 bits; bias (E, 2 I) bits with offs (E,) (None: one expert)"""
    x_bits = np.asarray(x_bits, dtype=np.uint16)
    inter = x_bits.shape[-1] // 2
    x2 = x_bits.reshape(-1, 2 * inter)
    g, u = x2[:, :inter], x2[:, inter:]
    if bias_bits is not None:
        bias_bits = np.asarray(bias_bits, dtype=np.uint16)
        e = np.zeros(x2.shape[0], dtype=np.int64) if offs is None else group_of_rows(offs, np.arange(x2.shape[0]))
        b = bias_bits[e]
        g = f32_to_bf16(bf16_to_f32(g) + bf16_to_f32(b[:, :inter]))
        u = f32_to_bf16(bf16_to_f32(u) + bf16_to_f32(b[:, inter:]))
    lim = np.float32(limit)
    gc = f32_to_bf16(np.minimum(bf16_to_f32(g), lim))                                  # exact: bf16 values
    uc = np.minimum(np.maximum(bf16_to_f32(u), -lim), lim)
    s = f64_to_bf16(sigmoid_gate(gc, alpha))
    act = f32_to_bf16(bf16_to_f32(s) * (uc + np.float32(1.0)))
    return act.reshape(*x_bits.shape[:-1], inter)


def exact_f64(x_bits, alpha=1.702, limit=7.0) -> np.ndarray:
    """the exact function of the bf16 inputs in fp64, nothing rounded: (min(max(u, -l), l) + 1) * gc / (1 + exp(-alpha * gc))"""
    x_bits = np.asarray(x_bits, dtype=np.uint16)
    inter = x_bits.shape[-1] // 2
    g, u = bf16_to_f64(x_bits[..., :inter]), bf16_to_f64(x_bits[..., inter:])
    gc, uc = np.minimum(g, limit), np.clip(u, -limit, limit)
    with np.errstate(over="ignore"):
        return (uc + 1.0) * gc / (1.0 + np.exp(-float(np.float32(alpha)) * gc))


def moe_combine_bias(y_bits, pos, weights, bias_bits, offs) -> np.ndarray:
    """y (M, H) bits, pos (T, topk) int, weights (T, topk) float32, bias (E, H) bits, offs (E,) or None -> out (T, H) bits"""
    y_bits, bias_bits = np.asarray(y_bits, dtype=np.uint16), np.asarray(bias_bits, dtype=np.uint16)
    pos, w = np.asarray(pos).astype(np.int64), np.asarray(weights, dtype=np.float32)
    M, T = y_bits.shape[0], pos.shape[0]
    acc = np.zeros((T, y_bits.shape[1]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(pos.shape[1]):
            p = pos[:, k]
            ok = (p >= 0) & (p < M)
            pp = np.where(ok, p, 0)
            e = np.zeros(T, dtype=np.int64) if offs is None else group_of_rows(offs, pp)
            v = bf16_to_f32(f32_to_bf16(bf16_to_f32(y_bits[pp]) + bf16_to_f32(bias_bits[e])))
            acc = np.where(ok[:, None], acc + w[:, k, None] * v, acc)
    return f32_to_bf16(acc)


def finite_gates(lo_exp=-120) -> np.ndarray:
    """every finite bf16 gate with |g| >= 2^lo_exp, and +-0: 63 490 bit patterns for -120"""
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    a = np.abs(bf16_to_f64(bits))
    return bits[np.isfinite(a) & ((a >= 2.0 ** lo_exp) | (a == 0))]


def tiny_gates(lo_exp=-120) -> np.ndarray:
    """the excluded gates: 0 < |g| < 2^lo_exp"""
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    a = np.abs(bf16_to_f64(bits))
    return bits[(a > 0) & (a < 2.0 ** lo_exp)]


def bf16_line(bits) -> np.ndarray:
    """bf16 bit patterns on a monotone integer line (+0 and -0 coincide): distances in bf16 steps"""
    v = np.asarray(bits).astype(np.int32)
    return np.where(v & 0x8000, -(v & 0x7fff), v)
