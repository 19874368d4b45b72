"""The contract of the MXFP8 rotate-and-quantize ops (fusedQuantizeMxf8 and its blocked, gathering and gated forms) in numpy -- a plain module, CPU only.

    y     = x_group @ h                       handed in by the caller: fp32 (or fp64 holding fp32 values); `rotate` below gives it where the products are exact
    amax  = max |y| over 32 consecutive y     NaNs ignored (a group that is all NaN has amax 0)
    E     = biased exponent field of the FP32 amax (not rounded to bf16 first)
    e8    = 127 if amax == 0 else clamp(E - SH, 0, 254),  SH = 7 for e4m3, 14 for e5m2
    q     = RNE(y * 2^(127 - e8)) to e4m3fn / e5m2; the power-of-two scaling is exact, -0 keeps its sign

The roundings are the oracle's orc_e4m3_encode / orc_e5m2_encode, called once per distinct scaled value."""
import numpy as np

import oracle

SH = {"e4m3": 7, "e5m2": 14}


def _encode(scaled: np.ndarray, fmt: str) -> np.ndarray:
    enc = oracle.e4m3_encode if fmt == "e4m3" else oracle.e5m2_encode
    bits = np.ascontiguousarray(scaled, dtype=np.float32).view(np.uint32)   # by bit pattern: -0 and +0 stay apart, every NaN goes through the encoder
    uniq, inv = np.unique(bits.reshape(-1), return_inverse=True)
    table = np.array([enc(float(v)) for v in uniq.view(np.float32)], dtype=np.uint8)
    return table[inv].reshape(scaled.shape)


def scale_bytes(y: np.ndarray, fmt: str) -> np.ndarray:
    """y (.., 32 n) -> e8 (.., n) uint8"""
    y32 = np.ascontiguousarray(y, dtype=np.float32)
    assert np.array_equal(y32.astype(np.float64), np.asarray(y, dtype=np.float64), equal_nan=True), "y must hold fp32 values"
    g = np.abs(y32).reshape(*y32.shape[:-1], y32.shape[-1] // 32, 32)
    amax = np.fmax.reduce(g, axis=-1, initial=np.float32(0))   # fmax: NaNs ignored
    E = (amax.view(np.uint32) >> 23).astype(np.int64) & 0xff
    return np.where(amax == 0, 127, np.clip(E - SH[fmt], 0, 254)).astype(np.uint8)


def quantize(y: np.ndarray, fmt: str):
    """y (.., 32 n) fp32 values -> (codes (.., 32 n) uint8, e8 (.., n) uint8)"""
    e8 = scale_bytes(y, fmt)
    mult = np.ldexp(1.0, 127 - np.repeat(e8.astype(np.int64), 32, axis=-1))   # fp64: 2^-127 .. 2^127, and the product with an fp32 is exact
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = np.asarray(y, dtype=np.float64) * mult
        # |scaled| < 2^16 for finite y; what falls below fp32's normal range is far under half the smallest fp8 subnormal and encodes to a signed zero
        return _encode(scaled.astype(np.float32), fmt), e8


def decode(codes: np.ndarray, fmt: str) -> np.ndarray:
    dec = oracle.e4m3_decode if fmt == "e4m3" else oracle.e5m2_decode
    table = np.array([dec(b) for b in range(256)], dtype=np.float64)
    return table[codes]


def dequantize(codes: np.ndarray, e8: np.ndarray, fmt: str) -> np.ndarray:
    """fp64 values of the quantized operand: code value * 2^(e8 - 127)"""
    return decode(codes, fmt) * np.ldexp(1.0, np.repeat(e8.astype(np.int64), 32, axis=-1) - 127)


def bf16_to_f64(bits: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(bits).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def rotate(x_bits: np.ndarray, h_bits: np.ndarray) -> np.ndarray:
    """y = x_group @ h in fp64 from bf16 bit patterns: x (.., K) viewed as rows of R, h (R, R).  Exact -- and therefore what any fp32 accumulation gives -- for
    the inputs of tests/_rotations.exact_input with a rotation of one magnitude, or for the identity.  The sum starts from +0 (the MFMA's accumulator), so a sum
    that is zero is +0 whatever the signs of its zero products: `+ 0.0`."""
    R = h_bits.shape[0]
    x = bf16_to_f64(x_bits)
    return (x.reshape(-1, R) @ bf16_to_f64(h_bits)).reshape(x.shape) + 0.0
