"""Two CPU models of one quantized mixture-of-experts layer -- numpy and the pinned oracle, nothing of qutlass_amd -- for tests that compare a whole layer with the
MATHEMATICS instead of with another sequence of this library's ops (tests/test_gpu_moe_layer_vs_fp64.py, tests/test_moe_model_cpu.py):

    out[t] = sum_k w[t, k] * (silu(x_t W_g^T) * (x_t W_u^T)) W_2^T      over the topk experts e = ids[t, k], W13[e] = [W_g; W_u] (2 I, H), W2[e] (H, I)

  * layer_fp64:       the fp64 router, the expert MLP and the weighted sum in fp64 on the unquantized bf16 values: no rotation, no fp4.
  * layer_quantized:  the same layer as the device chain computes it, step by step from the oracle: per expert oracle.fused_quantize_* of the routed tokens,
                      oracle.dequant_fp4 and an fp64 matmul times alpha (fp32), bf16 rounding of the GEMM output, the two-rounding activation of `_ref_act`,
                      a second quantize and GEMM, and moe_combine's definition (an fp32 multiply and add per slot, then bf16).
The expert weights are quantized HERE by the oracle, as w @ h over the input dimension with the activations' h, and a test uploads their bytes: how a deployment gets
its weights -- a transposition common to the device quantizers cannot cancel itself out.  The keyword arguments of layer_quantized build deliberately WRONG layers
(the mutation checks of tests/test_moe_model_cpu.py): the distance a convention error moves the result, in units of the quantization noise |L_q - L_fp64|.

Four more layers -- MXFP8 with SiLU, gpt-oss (clamped SwiGLU, per-expert biases, interleaved gate/up) on MXFP4 and as W4A8 from checkpoint bytes, and the latter over two
expert-parallel ranks -- live in tests/_moe_model_more.py, with formulas and wrong variants of their own; make_layer, quantize_weights, layer_fp64 and layer_quantized
here take their names and layers and hand them on."""
from typing import NamedTuple, Optional

import numpy as np

import oracle
from _rotations import bits, signed_permuted_hadamard
from test_gpu_gated_quantize import _bf16_to_f64, _f64_to_bf16, _ref_act  # the fp64 reference of the activation and its bf16 rounding

T, E, TOPK, H, I = 33, 8, 2, 256, 256
EMPTY = 6          # the expert that no token is routed to
MIN_GAP = 1e-3     # between neighbouring selection scores in fp64: no fp32 router can legitimately choose differently


class Layer(NamedTuple):
    name: str
    fmt: str                    # "mx" | "nv"
    method: str                 # "abs_max" | "quest"
    rot: int
    router: str                 # "softmax" (moe_route) | "grouped" (moe_route_grouped: sigmoid, bias, n_group 4, topk_group 2)
    tok: np.ndarray             # (T, H) bf16 bits
    logits: np.ndarray          # (T, E) float32
    bias: Optional[np.ndarray]  # (E,) float32, grouped router only
    w13: np.ndarray             # (E, 2 I, H) bf16 bits
    w2: np.ndarray              # (E, H, I) bf16 bits
    h: np.ndarray               # (R, R) bf16 bits, not symmetric
    a13_gs: Optional[np.ndarray]   # (E,) float32 each, NV only
    a2_gs: Optional[np.ndarray]
    w13_gs: Optional[np.ndarray]
    w2_gs: Optional[np.ndarray]
    alpha13: np.ndarray         # (1,) or (E,) float32
    alpha2: np.ndarray


N_GROUP, TOPK_GROUP = 4, 2
LAYERS = {"mx_abs_max": ("mx", "abs_max", 32, "softmax", 11), "mx_quest": ("mx", "quest", 64, "softmax", 22), "nv_grouped": ("nv", "abs_max", 32, "grouped", 13)}


def _nv_scales():
    """32 global scales between 0.5 and 13, pairwise different, none a power of two, dealt to a13_gs / a2_gs / w13_gs / w2_gs in a fixed shuffle"""
    i = np.arange(4 * E)
    s = (0.53 * 1.105 ** i + 0.0137 * i).astype(np.float32)
    assert len(np.unique(s)) == 4 * E and ((s.view(np.uint32) & 0x7fffff) != 0).all()
    return s[np.random.default_rng(5).permutation(4 * E)].reshape(4, E)


def make_layer(name: str):
    if name in MORE_LAYERS:
        return _more.make_layer(name)
    fmt, method, rot, router, seed = LAYERS[name]
    rng = np.random.default_rng(seed)
    import torch

    def bf16(a):
        return bits(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16))

    tok = bf16(rng.standard_normal((T, H)))
    w13 = bf16(rng.standard_normal((E, 2 * I, H)) * 0.2)
    w2 = bf16(rng.standard_normal((E, H, I)) * 0.2)
    logits = rng.standard_normal((T, E)).astype(np.float32)
    logits[:, EMPTY] = -30.0
    bias = None
    if router == "grouped":
        bias = (rng.uniform(0.0, 0.2, E)).astype(np.float32)
        bias[EMPTY] = 0.0
        bias[EMPTY ^ 1] = 0.9   # the empty expert's group mate carries the group's score alone
    h = bits(signed_permuted_hadamard(rot, seed=seed))
    gs = [None] * 4
    if fmt == "nv":
        gs = list(_nv_scales())
        alpha13, alpha2 = (1.0 / (gs[0] * gs[2])).astype(np.float32), (1.0 / (gs[1] * gs[3])).astype(np.float32)
    else:
        a = np.float32(1.0 / 9.0) if method == "abs_max" else np.float32(1.0)   # MX abs_max stores codes at 3 x the value: two operands, 9
        alpha13 = alpha2 = np.array([a], dtype=np.float32)
    return Layer(name, fmt, method, rot, router, tok, logits, bias, w13, w2, h, gs[0], gs[1], gs[2], gs[3], alpha13, alpha2)


# ---- routing in fp64 ---------------------------------------------------------------------------------------------------------------------------------------------
def _top(score, k):
    """(indices of the k + 1 largest in (score descending, index ascending), the smallest gap between neighbours among them)"""
    order = np.lexsort((np.arange(score.size), -score))[: k + 1]
    return order[:k], float(np.min(-np.diff(score[order]))) if order.size > 1 else np.inf


def route_fp64(layer: Layer):
    """-> ids (T, topk) int64 in selection order, weights (T, topk) fp64 (renormalized), the smallest gap between two neighbouring selection scores (group scores
    included) over all tokens.  "softmax": moe_topk_softmax -- selection on the logits, weights softmax probabilities over the selected sum.  "grouped":
    moe_topk_grouped -- s = sigmoid(x), c = s + bias selects; a group's score is the sum of its two largest c; the topk_group best groups survive; w = s / sum."""
    x = layer.logits.astype(np.float64)
    ids, w, gap = np.zeros((T, TOPK), np.int64), np.zeros((T, TOPK)), np.inf
    for t in range(T):
        if layer.router == "softmax":
            sel, g = _top(x[t], TOPK)
            p = np.exp(x[t] - x[t].max())
            p /= p.sum()
        else:
            p = 1.0 / (1.0 + np.exp(-x[t]))
            c = p + layer.bias.astype(np.float64)
            gscore = np.sort(c.reshape(N_GROUP, E // N_GROUP), axis=1)[:, -2:].sum(axis=1)
            groups, gg = _top(gscore, TOPK_GROUP)
            cand = np.full(E, -np.inf)
            for grp in groups:
                lo = grp * (E // N_GROUP)
                cand[lo: lo + E // N_GROUP] = c[lo: lo + E // N_GROUP]
            sel, g = _top(cand, TOPK)
            g = min(g, gg)
        ids[t], w[t], gap = sel, p[sel] / p[sel].sum(), min(gap, g)
    return ids, w, gap


# ---- the quantized operands ----------------------------------------------------------------------------------------------------------------------------------------
def _quantize(layer: Layer, x_bits, h, gs, acc_model):
    """x (rows, K) bf16 bits -> (codes (rows, K / 2), scale bytes (rows, K / group)) by the oracle"""
    rows, k = x_bits.shape
    m = oracle.QUEST if layer.method == "quest" else oracle.ABS_MAX
    if layer.fmt == "mx":
        q, s, _ = oracle.fused_quantize_mx(x_bits, h, m, acc_model=acc_model)
        return q.reshape(rows, k // 2), s.reshape(rows, k // 32)
    q, s = oracle.fused_quantize_nv(x_bits, h, float(gs), m, acc_model=acc_model)
    return q.reshape(rows, k // 2), s.reshape(rows, k // 16)


def _dequant(layer: Layer, codes, sf):
    rows = codes.shape[0]
    nv = layer.fmt == "nv"
    return oracle.dequant_fp4(codes, sf, 16 if nv else 32, nv).reshape(rows, -1)


def quantize_weights(layer, acc_model: int = 1, **wrong):
    """-> w13q (E, 2 I, H / 2), w13s (E, 2 I, H / group), w2q (E, H, I / 2), w2s (E, H, I / group): every expert's weight rotated as w @ h with the layer's h over its
    input dimension and quantized (NV: under its own global scale) by the oracle"""
    if isinstance(layer, _more.Layer2):
        return _more.quantize_weights(layer, acc_model, **wrong)
    out = []
    for w, gs in ((layer.w13, layer.w13_gs), (layer.w2, layer.w2_gs)):
        qs = [_quantize(layer, w[e], layer.h, None if gs is None else gs[e], acc_model) for e in range(E)]
        out += [np.stack([q for q, _ in qs]), np.stack([s for _, s in qs])]
    return tuple(out)


def _gemm(layer: Layer, a_dq, wq, ws, alpha):
    """bf16(fp32(a_dq @ dequant(w)^T) * alpha) as bf16 bits: the block-scaled GEMMs' contract (oracle.gemm_blockscaled: exact sum, one fp32 multiply, bf16 RNE)"""
    return _gemm_dq(a_dq, _dequant(layer, wq, ws), alpha)


def _gemm_dq(a_dq, w_dq, alpha):
    """the same contract on dequantized operands (rows, K) and (N, K) in fp64, whatever their formats"""
    acc = (a_dq @ w_dq.T).astype(np.float32) * np.float32(alpha)
    return _f64_to_bf16(acc.astype(np.float64))


# ---- the two models --------------------------------------------------------------------------------------------------------------------------------------------------
def layer_fp64(layer, ids, weights, **rank) -> np.ndarray:
    if isinstance(layer, _more.Layer2):
        return _more.layer_fp64(layer, ids, weights, **rank)
    x = _bf16_to_f64(layer.tok)
    out = np.zeros((T, H))
    for t in range(T):
        for k in range(TOPK):
            e = ids[t, k]
            gu = _bf16_to_f64(layer.w13[e]) @ x[t]
            g, u = gu[:I], gu[I:]
            out[t] += weights[t, k] * (_bf16_to_f64(layer.w2[e]) @ (g / (1.0 + np.exp(-g)) * u))
    return out


def layer_quantized(layer, ids, weights, wq, acc_model: int = 1, ha=None, swap_weights: bool = False, swap_gate_up: bool = False,
                    neighbour_a2: bool = False, **more) -> np.ndarray:
    """The layer as the device chain defines it, (T, H) fp64 holding bf16 values.  wq = quantize_weights(layer).  The wrong variants: ha -- the activations' rotation
    (default layer.h; pass its transpose); swap_weights -- the two routing weights of every token exchanged; swap_gate_up -- the halves of the (rows, 2 I) GEMM
    output exchanged before the activation; neighbour_a2 -- the second quantizer takes the next expert's a2 global scale while alpha2 stays (NV only).
    The layers of tests/_moe_model_more.py have flags of their own (**more: see its layer_quantized)."""
    if isinstance(layer, _more.Layer2):
        return _more.layer_quantized(layer, ids, weights, wq, acc_model, ha=ha, swap_weights=swap_weights, swap_gate_up=swap_gate_up, **more)
    assert not more, more
    ha = layer.h if ha is None else np.ascontiguousarray(ha)
    w13q, w13s, w2q, w2s = wq
    y = np.zeros((T, TOPK, H))   # the down projection's rows, by slot
    for e in range(E):
        tt, kk = np.nonzero(ids == e)
        if tt.size == 0:
            continue
        per = lambda a: a[e] if a is not None and a.size > 1 else (None if a is None else a[0])
        aq, asf = _quantize(layer, layer.tok[tt], ha, per(layer.a13_gs), acc_model)
        gate_up = _gemm(layer, _dequant(layer, aq, asf), w13q[e], w13s[e], per(layer.alpha13))
        if swap_gate_up:
            gate_up = np.concatenate([gate_up[:, I:], gate_up[:, :I]], axis=1)
        a2 = None if layer.a2_gs is None else layer.a2_gs[(e + 1) % E if neighbour_a2 else e]
        bq, bsf = _quantize(layer, _ref_act(gate_up), ha, a2, acc_model)
        y[tt, kk] = _bf16_to_f64(_gemm(layer, _dequant(layer, bq, bsf), w2q[e], w2s[e], per(layer.alpha2)))
    w = weights[:, ::-1] if swap_weights else weights
    w32, y32 = w.astype(np.float32), y.astype(np.float32)
    acc = np.zeros((T, H), dtype=np.float32)
    for k in range(TOPK):   # moe_combine: acc = acc + w * y, the product and the sum each rounded to fp32
        acc = acc + w32[:, k: k + 1] * y32[:, k]
    return _bf16_to_f64(_f64_to_bf16(acc.astype(np.float64)))


def fro(a) -> float:
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


# ---- the MXFP8, gpt-oss and W4A8 layers: tests/_moe_model_more.py, reached through make_layer / quantize_weights / layer_fp64 / layer_quantized above ------------------
MORE_LAYERS = ("mxf8_silu", "oai_mx", "oai_w4a8", "oai_w4a8_ep")
import _moe_model_more as _more  # noqa: E402  (it imports this module: at the end, where everything it uses is defined)
