"""Four more layers for tests/_moe_model.py (which imports this module and dispatches to it): the MXFP8 SiLU layer, gpt-oss on MXFP4, gpt-oss W4A8 from checkpoint
bytes, and that W4A8 layer split over two expert-parallel ranks.  As there: numpy, the oracle and the CPU models of tests/ -- nothing of qutlass_amd but
utils.split_interleaved_gate_up, the load-time rule itself (plain torch, on the CPU).

    mxf8_silu    out[t] = sum_k w[t, k] * W2 (silu(g) * u)                                     [g; u] = W13 x_t, W13 = [W_g; W_u] in halves
    oai_*        out[t] = sum_k w[t, k] * (W2 ((clip(u, -7, 7) + 1) * gc * sigmoid(1.702 gc)) + b2)     gc = min(g, 7), g = (W13 x_t + b1)[0::2], u = (W13 x_t + b1)[1::2]:
                 the checkpoint stores gate and up INTERLEAVED, even rows the gate; every bias belongs to the slot's expert e = ids[t, k]

  * layer_fp64:       that formula in fp64 on the unquantized weights -- for oai_w4a8 the fp64 dequantization of the checkpoint's e2m1 codes and e8m0 scale bytes.  With
                      `rank` only the slots whose expert lives on that rank are summed: the partial an expert-parallel rank contributes.
  * quantize_weights: what a deployment uploads, in the [gate | up] halves the ops take: w13, its scales and b1 through split_interleaved_gate_up; mxf8_silu rotates
                      w @ h and quantizes with _mxf8_quant_model, oai_mx with the oracle, oai_w4a8 uploads the checkpoint's bytes.
  * layer_quantized:  the device chain step by step: the routed rows sorted by LOCAL expert (moe_sort's definition, an expert of another rank dropped: pos -1, its row
                      past offs[-1]), the activation quantizer (_mxf8_quant_model.quantize of the fp32 rotation, or the oracle's MXFP4), _moe_model._gemm_dq,
                      _swiglu_oai_model.swiglu_oai with the expert's b1 (or _ref_act), the second quantizer and GEMM, _swiglu_oai_model.moe_combine_bias (or the
                      plain combine).  Its keyword arguments, and those of quantize_weights, build the deliberately WRONG layers of tests/test_moe_model_cpu.py.

The data is chosen so that every convention is visible above the quantization noise (tests/test_moe_model_cpu.py asserts the properties): the gpt-oss layers take
gate/up weights large enough that a good share of gate and up values pass the limit of 7, and biases of the size of what they are added to."""
from typing import NamedTuple, Optional

import numpy as np

import _moe_model as mm
import _mxf8_quant_model as m8
import _swiglu_oai_model as oai
import _w4a8_model as w4
from _rotations import bits, signed_permuted_hadamard
from test_gpu_gated_quantize import _ref_act

T, E, TOPK, H, I = mm.T, mm.E, mm.TOPK, mm.H, mm.I
RANKS = 2                         # oai_w4a8_ep: global experts 0 .. 3 on rank 0, 4 .. 7 on rank 1
ALPHA, LIMIT = 1.702, 7.0         # gpt-oss
NO_LIMIT = float(2.0 ** 126)      # a bf16 value no gate or up reaches: the "no clamp" mutation


class Layer2(NamedTuple):
    name: str
    kind: str                     # "silu" | "oai"
    fmt: str                      # "mxf8": e4m3 tokens and weights | "mx": MXFP4 both (the oracle's) | "w4a8": e4m3 tokens, checkpoint MXFP4 weights
    method: str                   # "abs_max" (MXFP8 has no other)
    rot: int
    router: str                   # "softmax" -- what route_fp64 reads
    route_op: str                 # "moe_route" | "moe_route_fused": the device op (the same five results)
    ranks: int                    # 1, or RANKS for the expert-parallel layer
    tok: np.ndarray               # (T, H) bf16 bits
    logits: np.ndarray            # (T, E) float32
    bias: None                    # (no router bias: route_fp64 reads the field)
    h: np.ndarray                 # (R, R) bf16 bits: not symmetric, or the identity (w4a8)
    w13: Optional[np.ndarray]     # (E, 2 I, H) bf16 bits: [gate; up] halves (silu), INTERLEAVED rows (oai_mx), None (w4a8)
    w2: Optional[np.ndarray]      # (E, H, I) bf16 bits
    b1: Optional[np.ndarray]      # (E, 2 I) bf16 bits, interleaved like w13's rows (oai)
    b2: Optional[np.ndarray]      # (E, H) bf16 bits (oai)
    ck: Optional[dict]            # w4a8, the checkpoint: w13c (E, 2 I, H / 2) packed e2m1 (_w4a8_model.pack_e2m1's order), w13s (E, 2 I, H / 32) e8m0 bytes, w2c, w2s
    alpha13: np.ndarray           # (1,) float32
    alpha2: np.ndarray


class Upload(NamedTuple):
    """what goes to the device: code bytes (E, N, K or K / 2), scale bytes (E, N, K / 32), biases as bf16 bits in [gate | up] halves"""
    w13q: np.ndarray
    w13s: np.ndarray
    w2q: np.ndarray
    w2s: np.ndarray
    b1: Optional[np.ndarray]
    b2: Optional[np.ndarray]


#            kind    fmt     rot  route_op           ranks seed  w13 x (gate rows, up rows)  w2 x  b1 x  b2 x
LAYERS = {"mxf8_silu": ("silu", "mxf8", 32, "moe_route", 1, 48, (0.2, 0.2), 0.2, None, None),
          "oai_mx": ("oai", "mx", 64, "moe_route_fused", 1, 32, (0.35, 0.2), 0.2, 2.0, 24.0),
          "oai_w4a8": ("oai", "w4a8", 32, "moe_route", 1, 36, None, None, 2.0, 16.0),
          "oai_w4a8_ep": ("oai", "w4a8", 32, "moe_route", RANKS, 36, None, None, 2.0, 16.0)}   # the same data as oai_w4a8: the ranks' partials sum to that layer
# the W4A8 checkpoint: code bytes uniform (e2m1 values of rms 2.93), scale bytes drawn per 32-block from these ranges -- w13 of rms about 0.35, w2 about 0.2
W13_SF, W2_SF = (122, 126), (121, 125)


def _bf16(a) -> np.ndarray:
    import torch

    return bits(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16))


def make_layer(name: str) -> Layer2:
    kind, fmt, rot, route_op, ranks, seed, s13, s2, sb1, sb2 = LAYERS[name]
    rng = np.random.default_rng(seed)
    tok = _bf16(rng.standard_normal((T, H)))
    logits = rng.standard_normal((T, E)).astype(np.float32)
    logits[:, mm.EMPTY] = -30.0
    w13 = w2 = b1 = b2 = ck = None
    if fmt == "w4a8":
        ck = {"w13c": rng.integers(0, 256, (E, 2 * I, H // 2), dtype=np.uint8), "w13s": rng.integers(*W13_SF, (E, 2 * I, H // 32)).astype(np.uint8),
              "w2c": rng.integers(0, 256, (E, H, I // 2), dtype=np.uint8), "w2s": rng.integers(*W2_SF, (E, H, I // 32)).astype(np.uint8)}
        h = _bf16(np.eye(rot))
    else:
        rows = np.repeat(s13, I) if kind == "silu" else np.tile(s13, I)   # halves, or interleaved: even = gate
        w13 = _bf16(rng.standard_normal((E, 2 * I, H)) * rows[None, :, None])
        w2 = _bf16(rng.standard_normal((E, H, I)) * s2)
        h = bits(signed_permuted_hadamard(rot, seed=seed))
    if kind == "oai":
        b1, b2 = _bf16(rng.standard_normal((E, 2 * I)) * sb1), _bf16(rng.standard_normal((E, H)) * sb2)
    a = np.float32(1.0 / 9.0) if fmt == "mx" else np.float32(1.0)   # MX abs_max stores codes at 3 x the value; MXFP8 and the checkpoint's scales need no alpha
    alpha = np.array([a], dtype=np.float32)
    return Layer2(name, kind, fmt, "abs_max", rot, "softmax", route_op, ranks, tok, logits, None, h, w13, w2, b1, b2, ck, alpha, alpha)


# ---- the weights ---------------------------------------------------------------------------------------------------------------------------------------------------
def dequant_e2m1(codes, sf) -> np.ndarray:
    """(.., K / 2) packed e2m1, (.., K / 32) e8m0 bytes -> (.., K) fp64: _w4a8_model's tables (element 2 j in the low nibble of byte j)"""
    return w4.E2M1[w4.unpack_e2m1(codes)] * np.repeat(w4.scale_f64(sf), 32, axis=-1)


def weights_fp64(layer: Layer2):
    """-> W13 (E, 2 I, H), W2 (E, H, I) in fp64 as the layer stores them (oai: rows interleaved)"""
    if layer.fmt == "w4a8":
        return dequant_e2m1(layer.ck["w13c"], layer.ck["w13s"]), dequant_e2m1(layer.ck["w2c"], layer.ck["w2s"])
    return oai.bf16_to_f64(layer.w13), oai.bf16_to_f64(layer.w2)


def _split(a, dim, no_split=False, odd_gate=False) -> np.ndarray:
    """utils.split_interleaved_gate_up on a numpy array -- or one of the two load-time mistakes"""
    import torch

    from qutlass_amd.utils import split_interleaved_gate_up

    if no_split:
        return np.ascontiguousarray(a)
    if odd_gate:
        sl = [slice(None)] * a.ndim
        ev, od = list(sl), list(sl)
        ev[dim], od[dim] = slice(0, None, 2), slice(1, None, 2)
        return np.concatenate([a[tuple(od)], a[tuple(ev)]], axis=dim)
    if a.dtype == np.uint16:
        return split_interleaved_gate_up(torch.from_numpy(a.view(np.int16).copy()), dim).numpy().view(np.uint16)
    return split_interleaved_gate_up(torch.from_numpy(np.ascontiguousarray(a)), dim).numpy()


def rotate_f32(x_bits, h_bits, acc_model: int = 1) -> np.ndarray:
    """y = x_group @ h as fp32 values.  acc_model 1: the exact sum (fp64: the products of bf16 values and their sums over at most 128 terms of this size are exact
    there) rounded once to fp32; acc_model 0: a sequential fp32 accumulation from +0, every product exact.  Any fp32 summation order lies as close to either."""
    if acc_model == 1:
        return m8.rotate(x_bits, h_bits).astype(np.float32)
    R = h_bits.shape[0]
    x, h = oai.bf16_to_f32(x_bits).reshape(-1, R), oai.bf16_to_f32(h_bits)
    acc = np.zeros((x.shape[0], R), dtype=np.float32)
    for i in range(R):
        acc = acc + x[:, i: i + 1] * h[i][None, :]
    return acc.reshape(x_bits.shape)


def quantize_weights(layer: Layer2, acc_model: int = 1, no_split: bool = False, odd_gate: bool = False, swap_nibbles: bool = False,
                     scales_kn: bool = False) -> Upload:
    """The wrong variants: no_split -- gate/up weight, scales and b1 uploaded interleaved as stored; odd_gate -- split with the odd rows as the gate; swap_nibbles --
    the two e2m1 codes of every weight byte exchanged (w4a8); scales_kn -- the weight scale bytes laid out (E, K / 32, N) where the GEMM reads (E, N, K / 32) (w4a8)."""
    sp = lambda a, dim: _split(a, dim, no_split, odd_gate)
    b1 = None if layer.b1 is None else sp(layer.b1, 1)
    if layer.fmt == "w4a8":
        ck = layer.ck
        w13q, w13s, w2q, w2s = sp(ck["w13c"], 1), sp(ck["w13s"], 1), ck["w2c"], ck["w2s"]
        if swap_nibbles:
            w13q, w2q = ((w >> 4) | ((w & 0xF) << 4) for w in (w13q, w2q))
        if scales_kn:
            w13s, w2s = (np.ascontiguousarray(s.transpose(0, 2, 1)).reshape(s.shape) for s in (w13s, w2s))
        return Upload(np.ascontiguousarray(w13q), np.ascontiguousarray(w13s), w2q, w2s, b1, layer.b2)
    w13 = layer.w13 if layer.kind == "silu" else sp(layer.w13, 1)   # (the SiLU layer's weight is in halves already)
    out = []
    for w in (w13, layer.w2):
        if layer.fmt == "mx":
            qs = [mm._quantize(layer, w[e], layer.h, None, acc_model) for e in range(E)]
        else:
            qs = [m8.quantize(rotate_f32(w[e], layer.h, acc_model), "e4m3") for e in range(E)]
        out += [np.stack([q for q, _ in qs]), np.stack([s for _, s in qs])]
    return Upload(out[0], out[1], out[2], out[3], b1, layer.b2)


def rank_stacks(wq: Upload, rank: int) -> Upload:
    """the stacks rank `rank` holds: its E / RANKS experts"""
    n = E // RANKS
    return Upload(*(None if a is None else np.ascontiguousarray(a[rank * n: (rank + 1) * n]) for a in wq))


def expert_map(rank: int) -> np.ndarray:
    """(E,) int32: the local index of every global expert on `rank`, -1 for the other rank's"""
    n = E // RANKS
    g = np.arange(E)
    return np.where(g // n == rank, g - rank * n, -1).astype(np.int32)


def sort_slots(local_ids, n_local: int):
    """moe_sort's definition -> src_row (T topk,), offs (n_local,), pos (T, topk): rows ordered by local expert, then (token, slot); an id outside [0, n_local) is
    dropped -- its row behind every expert's, pos -1, not counted in offs"""
    flat = local_ids.reshape(-1)
    key = np.where((flat >= 0) & (flat < n_local), flat, n_local)
    order = np.argsort(key, kind="stable")
    pos = np.empty(flat.size, dtype=np.int64)
    pos[order] = np.arange(flat.size)
    pos = np.where(key < n_local, pos, -1).reshape(local_ids.shape)
    return order // local_ids.shape[1], np.cumsum(np.bincount(key, minlength=n_local + 1)[:n_local]), pos


# ---- the two models --------------------------------------------------------------------------------------------------------------------------------------------------
def layer_fp64(layer: Layer2, ids, weights, rank: Optional[int] = None) -> np.ndarray:
    x = oai.bf16_to_f64(layer.tok)
    w13, w2 = weights_fp64(layer)
    a = float(np.float32(ALPHA))
    out = np.zeros((T, H))
    for t in range(T):
        for k in range(TOPK):
            e = ids[t, k]
            if rank is not None and e // (E // RANKS) != rank:
                continue
            gu = w13[e] @ x[t]
            if layer.kind == "silu":
                g, u = gu[:I], gu[I:]
                y = w2[e] @ (g / (1.0 + np.exp(-g)) * u)
            else:
                gu = gu + oai.bf16_to_f64(layer.b1[e])
                gc, uc = np.minimum(gu[0::2], LIMIT), np.clip(gu[1::2], -LIMIT, LIMIT)   # even = gate
                y = w2[e] @ ((uc + 1.0) * gc / (1.0 + np.exp(-a * gc))) + oai.bf16_to_f64(layer.b2[e])
            out[t] += weights[t, k] * y
    return out


def _quant_act(layer: Layer2, x_bits, ha, acc_model, e5m2_shift=False) -> np.ndarray:
    """the activation quantizer and its dequantization: x (rows, K) bf16 bits -> (rows, K) fp64"""
    if layer.fmt == "mx":
        return mm._dequant(layer, *mm._quantize(layer, x_bits, ha, None, acc_model))
    y = rotate_f32(x_bits, ha, acc_model)
    if not e5m2_shift:
        return m8.dequantize(*m8.quantize(y, "e4m3"), "e4m3")
    e8 = m8.scale_bytes(y, "e5m2")     # the wrong shift: the block maximum scaled to [2^14, 2^15), which e4m3 saturates at 448
    scaled = y.astype(np.float64) * np.ldexp(1.0, 127 - np.repeat(e8.astype(np.int64), 32, axis=-1))
    return m8.dequantize(m8._encode(scaled.astype(np.float32), "e4m3"), e8, "e4m3")


def _dequant_w(layer: Layer2, codes, sf) -> np.ndarray:
    if layer.fmt == "mx":
        return mm._dequant(layer, codes, sf)
    if layer.fmt == "w4a8":
        return dequant_e2m1(codes, sf)
    return m8.dequantize(codes, sf, "e4m3")


def _act_oai(gate_up, b1_row, no_clamp, no_plus_one, alpha_one) -> np.ndarray:
    """swiglu_oai_and_mul's contract for the rows of ONE expert, (rows, 2 I) bits -> (rows, I) bits"""
    limit = NO_LIMIT if no_clamp else LIMIT
    if not no_plus_one:
        return oai.swiglu_oai(gate_up, 1.0 if alpha_one else ALPHA, limit, bias_bits=b1_row[None, :])
    # the wrong variant restates the model's steps without the + 1
    g = oai.f32_to_bf16(oai.bf16_to_f32(gate_up[:, :I]) + oai.bf16_to_f32(b1_row[None, :I]))
    u = oai.f32_to_bf16(oai.bf16_to_f32(gate_up[:, I:]) + oai.bf16_to_f32(b1_row[None, I:]))
    gc = oai.f32_to_bf16(np.minimum(oai.bf16_to_f32(g), np.float32(limit)))
    uc = np.minimum(np.maximum(oai.bf16_to_f32(u), -np.float32(limit)), np.float32(limit))
    return oai.f32_to_bf16(oai.bf16_to_f32(oai.f64_to_bf16(oai.sigmoid_gate(gc, ALPHA))) * uc)


def layer_quantized(layer: Layer2, ids, weights, wq: Upload, acc_model: int = 1, rank: Optional[int] = None, ha=None, swap_weights: bool = False,
                    swap_gate_up: bool = False, neighbour_b1: bool = False, neighbour_b2: bool = False, unweighted_b2: bool = False, no_clamp: bool = False,
                    no_plus_one: bool = False, alpha_one: bool = False, global_bias_index: bool = False, e5m2_shift: bool = False) -> np.ndarray:
    """The layer as the device chain defines it, (T, H) fp64 holding bf16 values.  wq = quantize_weights(layer), with `rank` its rank_stacks(wq, rank): the partial of
    that rank.  The wrong variants: ha -- the activations' rotation (pass layer.h.T); swap_weights -- a token's two routing weights exchanged; swap_gate_up -- the
    halves of the GEMM output exchanged before the activation; neighbour_b1 / neighbour_b2 -- the next local expert's bias; unweighted_b2 -- sum(w y) + sum(b2)
    instead of sum(w (y + b2)); no_clamp; no_plus_one; alpha_one -- the sigmoid's alpha 1.0 instead of 1.702; global_bias_index -- b1 / b2 addressed by the global expert index, held inside the rank's stack as g(r) is;
    e5m2_shift -- the scale shift 14 of e5m2 in the e4m3 activation quantizers."""
    ha = layer.h if ha is None else np.ascontiguousarray(ha)
    n_local = E if rank is None else E // RANKS
    first = 0 if rank is None else rank * n_local
    local = np.where((ids >= first) & (ids < first + n_local), ids - first, -1)
    src_row, offs, pos = sort_slots(local, n_local)
    assert wq.w13q.shape[0] == n_local

    def bias_row(b, e, neighbour):
        e = (e + 1) % n_local if neighbour else e
        return b[min(e + first, n_local - 1) if global_bias_index else e]

    y = np.zeros((T * TOPK, H), dtype=np.uint16)   # the down projection's sorted rows; those past offs[-1] are never read
    start = 0
    for e in range(n_local):
        rows, start = slice(start, int(offs[e])), int(offs[e])
        if rows.stop == rows.start:
            continue
        a_dq = _quant_act(layer, layer.tok[src_row[rows]], ha, acc_model, e5m2_shift)
        gate_up = mm._gemm_dq(a_dq, _dequant_w(layer, wq.w13q[e], wq.w13s[e]), layer.alpha13[0])
        if swap_gate_up:
            gate_up = np.concatenate([gate_up[:, I:], gate_up[:, :I]], axis=1)
        act = _ref_act(gate_up) if layer.kind == "silu" else _act_oai(gate_up, bias_row(wq.b1, e, neighbour_b1), no_clamp, no_plus_one, alpha_one)
        y[rows] = mm._gemm_dq(_quant_act(layer, act, ha, acc_model, e5m2_shift), _dequant_w(layer, wq.w2q[e], wq.w2s[e]), layer.alpha2[0])
    w32 = (weights[:, ::-1] if swap_weights else weights).astype(np.float32)
    if layer.kind == "oai" and not unweighted_b2:
        b2 = np.stack([bias_row(wq.b2, e, neighbour_b2) for e in range(n_local)])
        return oai.bf16_to_f64(oai.moe_combine_bias(y, pos, w32, b2, offs))
    acc = np.zeros((T, H), dtype=np.float32)
    for k in range(TOPK):   # moe_combine: a slot with pos -1 is skipped; the product and the sum each rounded to fp32
        ok = pos[:, k] >= 0
        acc = np.where(ok[:, None], acc + w32[:, k: k + 1] * oai.bf16_to_f32(y[np.where(ok, pos[:, k], 0)]), acc)
    if unweighted_b2:       # the wrong combine: the biases of the token's (local) experts added once each, behind the weighted sum
        for k in range(TOPK):
            ok = local[:, k] >= 0
            acc = np.where(ok[:, None], acc + oai.bf16_to_f32(wq.b2[np.where(ok, local[:, k], 0)]), acc)
    return oai.bf16_to_f64(oai.f32_to_bf16(acc))
