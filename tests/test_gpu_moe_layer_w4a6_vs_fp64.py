"""GPU: the gpt-oss expert layer on 6-bit tokens against MXFP4 checkpoint bytes (W4A6) held against the MATHEMATICS:

    moe_route -> fusedGatherQuantizeMxf6 -> grouped_matmul_mxf6_mxf4_bf16_tn(w13) -> swiglu_oai_and_mul(bias=b1, offs) -> fusedQuantizeMxf6
              -> grouped_matmul_mxf6_mxf4_bf16_tn(w2) -> moe_combine(bias=b2, offs)

on the layer `oai_w4a8` of tests/_moe_model_more.py (the size tests/test_gpu_moe_layer_vs_fp64.py holds the W4A8 layer at, the same seed): the weights are a
checkpoint's e2m1 and e8m0 bytes, whose fp64 dequantization IS the fp64 layer's weight, so L_fp64 is fp64 mathematics on the dequantised weights and the error left
is that of the two token quantizations and the bf16 roundings between the ops.  The W4A4 chain (fusedGatherQuantizeMx / fusedSwigluOaiQuantizeMx with abs-max
scales, whose codes sit at three times the value: alpha = 1/3) and the W4A8 chain run beside it on the same operands; the 6-bit chain's error must be below half
the 4-bit chain's.  The three errors are recorded in DESIGN.md section 10."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _moe_model as mm  # noqa: E402
import _moe_model_more as more  # noqa: E402,F401  (registers the layer)
from _rotations import bits  # noqa: E402

DEV = "cuda:0"
E8M0 = torch.float8_e8m0fnu


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _bf16(bits_u16):
    return torch.from_numpy(bits_u16.view(np.int16).copy()).view(torch.bfloat16).to(DEV)


def _w4a6(q, dev):
    weights, ids, src_row, offs, pos = q.moe_route(dev["logits"], mm.TOPK)
    aq, asf = q.fusedGatherQuantizeMxf6(dev["tok"], dev["h"], src_row)
    gate_up = q.grouped_matmul_mxf6_mxf4_bf16_tn(aq, dev["w13q"], asf, dev["w13s"], dev["alpha"], offs)
    act = q.swiglu_oai_and_mul(gate_up, bias=dev["b1"], offs=offs)
    bq, bsf = q.fusedQuantizeMxf6(act, dev["h"])
    y = q.grouped_matmul_mxf6_mxf4_bf16_tn(bq, dev["w2q"], bsf, dev["w2s"], dev["alpha"], offs)
    assert aq.shape == (mm.T * mm.TOPK, mm.H * 3 // 4) and gate_up.shape == (mm.T * mm.TOPK, 2 * mm.I) and y.shape == (mm.T * mm.TOPK, mm.H)
    out = q.moe_combine(y, pos, weights, bias=dev["b2"], offs=offs)
    torch.cuda.synchronize()
    return weights, ids, offs, out


def _w4a8(q, dev):
    weights, ids, src_row, offs, pos = q.moe_route(dev["logits"], mm.TOPK)
    aq, asf = q.fusedGatherQuantizeMxf8(dev["tok"], dev["h"], src_row)
    gate_up = q.grouped_matmul_mxf8_mxf4_bf16_tn(aq, dev["w13q"], asf, dev["w13s"], dev["alpha"], offs)
    bq, bsf = q.fusedSwigluOaiQuantizeMxf8(gate_up, dev["h"], bias=dev["b1"], offs=offs)
    y = q.grouped_matmul_mxf8_mxf4_bf16_tn(bq, dev["w2q"], bsf, dev["w2s"], dev["alpha"], offs)
    out = q.moe_combine(y, pos, weights, bias=dev["b2"], offs=offs)
    torch.cuda.synchronize()
    return out


def _w4a4(q, dev):
    weights, ids, src_row, offs, pos = q.moe_route(dev["logits"], mm.TOPK)
    third = dev["alpha"] / 3.0        # fusedQuantizeMx's abs-max codes sit at three times the value
    aq, asf = q.fusedGatherQuantizeMx(dev["tok"], dev["h"], src_row, method="abs_max")
    gate_up = q.grouped_matmul_mxf4_bf16_tn(aq, dev["w13q"], asf, dev["w13s"], third, offs)
    bq, bsf = q.fusedSwigluOaiQuantizeMx(gate_up, dev["h"], method="abs_max", bias=dev["b1"], offs=offs)
    y = q.grouped_matmul_mxf4_bf16_tn(bq, dev["w2q"], bsf, dev["w2s"], third, offs)
    out = q.moe_combine(y, pos, weights, bias=dev["b2"], offs=offs)
    torch.cuda.synchronize()
    return out


def test_gpt_oss_w4a6_layer_against_the_fp64_model(q):
    layer = mm.make_layer("oai_w4a8")
    ids, weights, gap = mm.route_fp64(layer)
    assert gap > mm.MIN_GAP, gap
    wq = mm.quantize_weights(layer)                   # the checkpoint's own bytes, biases in [gate | up] halves
    l_fp64 = mm.layer_fp64(layer, ids, weights)       # fp64 mathematics on the fp64 dequantization of those bytes
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    assert float(layer.alpha13[0]) == 1.0 and float(layer.alpha2[0]) == 1.0
    dev = {"tok": _bf16(layer.tok), "h": _bf16(layer.h), "logits": up(layer.logits), "alpha": up(layer.alpha13), "w13q": up(wq.w13q),
           "w13s": up(wq.w13s.reshape(-1)).view(E8M0), "w2q": up(wq.w2q), "w2s": up(wq.w2s.reshape(-1)).view(E8M0), "b1": _bf16(wq.b1), "b2": _bf16(wq.b2)}

    g_w, g_ids, g_offs, out = _w4a6(q, dev)
    assert np.array_equal(g_ids.cpu().numpy(), ids)
    assert np.abs(g_w.cpu().numpy().astype(np.float64) - weights).max() <= 1e-5
    ends = np.concatenate([[0], g_offs.cpu().numpy()])
    assert np.array_equal(np.diff(ends), np.bincount(ids.reshape(-1), minlength=mm.E)) and ends[mm.EMPTY + 1] == ends[mm.EMPTY]
    assert out.shape == (mm.T, mm.H) and out.dtype == torch.bfloat16
    l6 = out.float().cpu().numpy().astype(np.float64)
    l8 = _w4a8(q, dev).float().cpu().numpy().astype(np.float64)
    l4 = _w4a4(q, dev).float().cpu().numpy().astype(np.float64)
    assert np.isfinite(l6).all() and np.isfinite(l8).all() and np.isfinite(l4).all()
    e6, e8, e4 = (mm.fro(l - l_fp64) / mm.fro(l_fp64) for l in (l6, l8, l4))
    print(f"oai layer on checkpoint MXFP4 weights, |L_gpu - L_fp64| / |L_fp64|: W4A6 {e6:.5f}, W4A8 {e8:.5f}, W4A4 {e4:.5f}")
    assert e6 < e4 / 2, (e6, e4)

    # the empty expert contributes nothing: its weight bytes replaced, the layer's bytes stay
    for k in ("w13q", "w2q"):
        dev[k] = dev[k].clone()
        dev[k][mm.EMPTY] = 0x77
    assert np.array_equal(bits(_w4a6(q, dev)[3]), bits(out))
