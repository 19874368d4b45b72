"""GPU: whole mixture-of-experts layers against the MATHEMATICS.  Every other whole-layer test compares the chain with another sequence of this library's own ops,
which pins fusion and grouping but not meaning: which alpha undoes which quantizer (MX abs_max stores codes at 3 x the value: 1 / 9 for two operands), that
activations and offline-quantized weights are rotated the same way round, which half of the (rows, 2 I) GEMM output is the gate, which routing weight belongs to
which slot.  Here tokens, router logits and bf16 expert weights go in, and the result is held against the two CPU models of tests/_moe_model.py:

    |L_gpu - L_q| <= 0.25 x |L_q - L_fp64|      L_q: the layer with oracle quantization, L_fp64: the unquantized fp64 layer; both norms from the CPU models

The expert weights are quantized on the CPU by the oracle (w @ h) and uploaded as bytes.  The 0.25: the suite accepts up to 2e-3 of an operand's codes flipping with the
accumulation order -- at most sqrt(2e-3) ~ 0.05 of the quantization-noise norm per operand -- and the bf16 rounding of gate_up adds about 2^-9 relative against about
0.1 of fp4 noise; the bound leaves a few times headroom over that, and tests/test_moe_model_cpu.py shows every convention error at 1.2 ... 20 x the noise.
Measured on an MI355X (|L_gpu - L_q| / noise): 0 for all three layers -- the device output is bit-equal to L_q."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _moe_model as mm  # noqa: E402
from _rotations import bits  # noqa: E402

DEV = "cuda:0"
BOUND = 0.25


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _bf16(bits_u16):
    return torch.from_numpy(bits_u16.view(np.int16).copy()).view(torch.bfloat16).to(DEV)


def _run(q, layer, dev):
    """router -> gathering quantizer -> grouped GEMM -> gated quantizer -> grouped GEMM -> moe_combine"""
    tok, h, logits, w13q, w13s, w2q, w2s, alpha13, alpha2 = (dev[k] for k in ("tok", "h", "logits", "w13q", "w13s", "w2q", "w2s", "alpha13", "alpha2"))
    if layer.router == "softmax":
        weights, ids, src_row, offs, pos = q.moe_route(logits, mm.TOPK)
    else:
        weights, ids, src_row, offs, pos = q.moe_route_grouped(logits, mm.TOPK, n_group=mm.N_GROUP, topk_group=mm.TOPK_GROUP, bias=dev["bias"], scoring="sigmoid")
    if layer.fmt == "mx":
        aq, asf = q.fusedGatherQuantizeMx(tok, h, src_row, method=layer.method)
        gate_up = q.grouped_matmul_mxf4_bf16_tn(aq, w13q, asf, w13s, alpha13, offs)
        bq, bsf = q.fusedSiluMulQuantizeMx(gate_up, h, method=layer.method)
        y = q.grouped_matmul_mxf4_bf16_tn(bq, w2q, bsf, w2s, alpha2, offs)
    else:
        aq, asf = q.fusedGatherQuantizeNvGrouped(tok, h, dev["a13_gs"], src_row, offs)
        gate_up = q.grouped_matmul_nvf4_bf16_tn(aq, w13q, asf, w13s, alpha13, offs)
        bq, bsf = q.fusedSiluMulQuantizeNvGrouped(gate_up, h, dev["a2_gs"], offs)
        y = q.grouped_matmul_nvf4_bf16_tn(bq, w2q, bsf, w2s, alpha2, offs)
    assert gate_up.shape == (mm.T * mm.TOPK, 2 * mm.I) and y.shape == (mm.T * mm.TOPK, mm.H)
    out = q.moe_combine(y, pos, weights)
    torch.cuda.synchronize()
    return weights, ids, offs, out


@pytest.mark.parametrize("name", list(mm.LAYERS))
def test_moe_layer_against_the_fp64_model(q, name):
    layer = mm.make_layer(name)
    ids, weights, gap = mm.route_fp64(layer)
    assert gap > mm.MIN_GAP, gap                      # the precondition of comparing ids exactly: no fp32 router can legitimately choose differently
    wq = mm.quantize_weights(layer)                   # by the oracle, on the CPU
    l_fp64 = mm.layer_fp64(layer, ids, weights)
    l_q = mm.layer_quantized(layer, ids, weights, wq)
    noise = mm.fro(l_q - l_fp64)

    sf_dtype = torch.float8_e8m0fnu if layer.fmt == "mx" else torch.float8_e4m3fn
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    dev = {"tok": _bf16(layer.tok), "h": _bf16(layer.h), "logits": up(layer.logits), "alpha13": up(layer.alpha13), "alpha2": up(layer.alpha2),
           "w13q": up(wq[0]), "w13s": up(wq[1].reshape(-1)).view(sf_dtype), "w2q": up(wq[2]), "w2s": up(wq[3].reshape(-1)).view(sf_dtype)}
    if layer.router == "grouped":
        dev["bias"] = up(layer.bias)
    if layer.fmt == "nv":
        dev["a13_gs"], dev["a2_gs"] = up(layer.a13_gs), up(layer.a2_gs)

    g_w, g_ids, g_offs, out = _run(q, layer, dev)
    assert np.array_equal(g_ids.cpu().numpy(), ids), np.nonzero((g_ids.cpu().numpy() != ids).any(axis=1))[0]
    assert np.abs(g_w.cpu().numpy().astype(np.float64) - weights).max() <= 1e-5                    # fp32 softmax / sigmoid against fp64
    ends = np.concatenate([[0], g_offs.cpu().numpy()])
    assert np.array_equal(np.diff(ends), np.bincount(ids.reshape(-1), minlength=mm.E)) and ends[mm.EMPTY + 1] == ends[mm.EMPTY]

    assert out.shape == (mm.T, mm.H) and out.dtype == torch.bfloat16
    l_gpu = out.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(l_gpu).all()
    ratio = mm.fro(l_gpu - l_q) / noise
    print(f"{name}: |L_gpu - L_q| / |L_q - L_fp64| = {ratio:.3e}   (noise / |L_fp64| = {noise / mm.fro(l_fp64):.4f}, "
          f"|L_gpu - L_fp64| / |L_fp64| = {mm.fro(l_gpu - l_fp64) / mm.fro(l_fp64):.4f})")
    assert ratio <= BOUND, ratio

    # the empty expert contributes nothing: its weights replaced by other bytes (every code 6, the model's scale bytes kept), the layer's bytes stay
    for k in ("w13q", "w2q"):
        dev[k] = dev[k].clone()
        dev[k][mm.EMPTY] = 0x77
    again = _run(q, layer, dev)[3]
    assert np.array_equal(bits(again), bits(out))
