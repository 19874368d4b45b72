"""GPU: the gpt-oss expert layer on bf16 tokens against MXFP4 checkpoint bytes (W4A16) held against the MATHEMATICS:

    moe_route -> grouped_matmul_bf16_mxf4_bf16_tn(tok, w13, src_row=src_row) -> swiglu_oai_and_mul(bias=b1, offs) -> grouped_matmul_bf16_mxf4_bf16_tn(w2)
              -> moe_combine(bias=b2, offs)

on the layer `oai_w4a8` of tests/_moe_model_more.py (the smallest shapes of tests/test_gpu_moe_layer_vs_fp64.py, the same seed): the weights are a checkpoint's e2m1
and e8m0 bytes, whose fp64 dequantization IS the fp64 layer's weight, so L_fp64 is fp64 mathematics on the dequantised weights and the only error left on this path
is the bf16 rounding of gate_up, of the activation and of the down projection's output.  The bound is the W4A8 layer's own figure on that seed: tests/
test_gpu_moe_layer_vs_fp64.py measures |L_q - L_fp64| / |L_fp64| = 0.0479 for `oai_w4a8` -- the new path must not exceed it -- and the W4A8
chain is run beside it here on the same operands: the bf16 tokens must come out closer to L_fp64 than the e4m3 ones."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _moe_model as mm  # noqa: E402
import _moe_model_more as more  # noqa: E402
from _rotations import bits  # noqa: E402

DEV = "cuda:0"
W4A8_FIGURE = 0.0479   # |L_q - L_fp64| / |L_fp64| of oai_w4a8 (tests/test_gpu_moe_layer_vs_fp64.py)
E8M0 = torch.float8_e8m0fnu


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _bf16(bits_u16):
    return torch.from_numpy(bits_u16.view(np.int16).copy()).view(torch.bfloat16).to(DEV)


def _w4a16(q, dev):
    weights, ids, src_row, offs, pos = q.moe_route(dev["logits"], mm.TOPK)
    gate_up = q.grouped_matmul_bf16_mxf4_bf16_tn(dev["tok"], dev["w13q"], dev["w13s"], dev["alpha"], offs, src_row=src_row)   # the gather in the GEMM
    act = q.swiglu_oai_and_mul(gate_up, bias=dev["b1"], offs=offs)
    y = q.grouped_matmul_bf16_mxf4_bf16_tn(act, dev["w2q"], dev["w2s"], dev["alpha"], offs)
    assert gate_up.shape == (mm.T * mm.TOPK, 2 * mm.I) and y.shape == (mm.T * mm.TOPK, mm.H)
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


def test_gpt_oss_w4a16_layer_against_the_fp64_model(q):
    layer = mm.make_layer("oai_w4a8")
    ids, weights, gap = mm.route_fp64(layer)
    assert gap > mm.MIN_GAP, gap
    wq = mm.quantize_weights(layer)                   # the checkpoint's own bytes, biases in [gate | up] halves
    l_fp64 = mm.layer_fp64(layer, ids, weights)       # fp64 mathematics on the fp64 dequantization of those bytes
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    assert float(layer.alpha13[0]) == 1.0 and float(layer.alpha2[0]) == 1.0
    dev = {"tok": _bf16(layer.tok), "h": _bf16(layer.h), "logits": up(layer.logits), "alpha": up(layer.alpha13), "w13q": up(wq.w13q),
           "w13s": up(wq.w13s.reshape(-1)).view(E8M0), "w2q": up(wq.w2q), "w2s": up(wq.w2s.reshape(-1)).view(E8M0), "b1": _bf16(wq.b1), "b2": _bf16(wq.b2)}

    g_w, g_ids, g_offs, out = _w4a16(q, dev)
    assert np.array_equal(g_ids.cpu().numpy(), ids)
    assert np.abs(g_w.cpu().numpy().astype(np.float64) - weights).max() <= 1e-5
    ends = np.concatenate([[0], g_offs.cpu().numpy()])
    assert np.array_equal(np.diff(ends), np.bincount(ids.reshape(-1), minlength=mm.E)) and ends[mm.EMPTY + 1] == ends[mm.EMPTY]
    assert out.shape == (mm.T, mm.H) and out.dtype == torch.bfloat16
    l16 = out.float().cpu().numpy().astype(np.float64)
    l8 = _w4a8(q, dev).float().cpu().numpy().astype(np.float64)
    assert np.isfinite(l16).all() and np.isfinite(l8).all()
    e16, e8 = mm.fro(l16 - l_fp64) / mm.fro(l_fp64), mm.fro(l8 - l_fp64) / mm.fro(l_fp64)
    print(f"oai layer on checkpoint MXFP4 weights, |L_gpu - L_fp64| / |L_fp64|: W4A16 {e16:.5f}, W4A8 {e8:.5f} (the W4A8 figure: {W4A8_FIGURE})")
    assert e16 < e8, (e16, e8)
    assert e16 <= W4A8_FIGURE, e16

    # the gather in the GEMM is the gather in front of it: the same bits from the routed copy of the tokens
    weights_d, _, src_row, offs, pos = q.moe_route(dev["logits"], mm.TOPK)
    routed = dev["tok"].index_select(0, src_row.long())
    a = q.grouped_matmul_bf16_mxf4_bf16_tn(routed, dev["w13q"], dev["w13s"], dev["alpha"], offs)
    b = q.grouped_matmul_bf16_mxf4_bf16_tn(dev["tok"], dev["w13q"], dev["w13s"], dev["alpha"], offs, src_row=src_row)
    assert np.array_equal(bits(a), bits(b))

    # the empty expert contributes nothing: its weight bytes replaced, the layer's bytes stay
    for k in ("w13q", "w2q"):
        dev[k] = dev[k].clone()
        dev[k][mm.EMPTY] = 0x77
    assert np.array_equal(bits(_w4a16(q, dev)[3]), bits(out))
