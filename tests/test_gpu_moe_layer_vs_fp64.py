"""GPU: whole mixture-of-experts layers against the MATHEMATICS.  Every other whole-layer test compares the chain with another sequence of this library's own ops,
which pins fusion and grouping but not meaning: which alpha undoes which quantizer (MX abs_max stores codes at 3 x the value: 1 / 9 for two operands), that
activations and offline-quantized weights are rotated the same way round, which half of the (rows, 2 I) GEMM output is the gate, which routing weight belongs to
which slot.  Here tokens, router logits and bf16 expert weights go in, and the result is held against the two CPU models of tests/_moe_model.py:

    |L_gpu - L_q| <= 0.25 x |L_q - L_fp64|      L_q: the layer with oracle quantization, L_fp64: the unquantized fp64 layer; both norms from the CPU models

The expert weights are quantized on the CPU by the oracle (w @ h) and uploaded as bytes.  The 0.25: the suite accepts up to 2e-3 of an operand's codes flipping with the
accumulation order -- at most sqrt(2e-3) ~ 0.05 of the quantization-noise norm per operand -- and the bf16 rounding of gate_up adds about 2^-9 relative against about
0.1 of fp4 noise; the bound leaves a few times headroom over that, and tests/test_moe_model_cpu.py shows every convention error at 1.2 ... 20 x the noise.
Measured on an MI355X (|L_gpu - L_q| / noise): 0 for all three layers -- the device output is bit-equal to L_q.

Four more layers (tests/_moe_model_more.py) under the same bound: MXFP8 with SiLU, its weights quantized on the CPU by tests/_mxf8_quant_model.py; gpt-oss on MXFP4
through the one-launch router, gate/up weight and b1 de-interleaved once by utils.split_interleaved_gate_up; gpt-oss W4A8 whose weights are a checkpoint's e2m1 and
e8m0 bytes; and that layer over two expert-parallel ranks (expert_map, four local experts, each rank with its own stacks), every rank judged against its own partial.
They pin what the first three cannot: the [gate | up] halves after de-interleaving, bias[g(r)] in the activation and w_k (y + b2[g(p)]) in the combine, the clamp and
the + 1, nibble order and scale layout of uploaded MXFP4 bytes against e4m3 tokens, and which rank's stack a local expert index addresses.  The e4m3 layers' noise is
0.05 ... 0.07 of |L_fp64|, so their 0.25 is a quarter of that: a flipped e4m3 code moves one element by 2^-3 of itself at most, and the models' exact GEMM sum differs
from an fp32 accumulation only where a bf16 rounding sits within 2^-24 of a tie.  Measured on an MI355X: mxf8_silu 0.043, oai_mx 3.3e-7, oai_w4a8 0.0095,
oai_w4a8_ep 0.0064 (rank 0) and 0.0106 (rank 1)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _moe_model as mm  # noqa: E402
import _moe_model_more as more  # noqa: E402
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


# ---- the MXFP8, gpt-oss and W4A8 layers of tests/_moe_model_more.py ------------------------------------------------------------------------------------------------------
E8M0, E4M3 = torch.float8_e8m0fnu, torch.float8_e4m3fn


def _upload(layer, wq):
    """one rank's stacks as the ops take them: code bytes (e4m3 for the MXFP8 layer, packed e2m1 else), flat e8m0 scales, the biases in [gate | up] halves"""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    codes = (lambda a: up(a).view(E4M3)) if layer.fmt == "mxf8" else up
    dev = {"w13q": codes(wq.w13q), "w13s": up(wq.w13s.reshape(-1)).view(E8M0), "w2q": codes(wq.w2q), "w2s": up(wq.w2s.reshape(-1)).view(E8M0)}
    if layer.kind == "oai":
        dev["b1"], dev["b2"] = _bf16(wq.b1), _bf16(wq.b2)
    return dev


def _run_more(q, layer, dev, rank=None):
    """router (with the rank's expert_map) -> gathering quantizer -> grouped GEMM -> activation quantizer (gpt-oss: with b1) -> grouped GEMM -> moe_combine (with b2)"""
    tok, h, logits, alpha13, alpha2 = (dev[k] for k in ("tok", "h", "logits", "alpha13", "alpha2"))
    route = getattr(q, layer.route_op)
    if rank is None:
        weights, ids, src_row, offs, pos = route(logits, mm.TOPK)
    else:
        weights, ids, src_row, offs, pos = route(logits, mm.TOPK, mm.E // more.RANKS, expert_map=dev["expert_map"])
    if layer.fmt == "mx":
        gather, gemm, act = (lambda *a: q.fusedGatherQuantizeMx(*a, method=layer.method)), q.grouped_matmul_mxf4_bf16_tn, \
            (lambda x, **kw: q.fusedSwigluOaiQuantizeMx(x, h, method=layer.method, **kw))
    elif layer.fmt == "w4a8":
        gather, gemm, act = q.fusedGatherQuantizeMxf8, q.grouped_matmul_mxf8_mxf4_bf16_tn, (lambda x, **kw: q.fusedSwigluOaiQuantizeMxf8(x, h, **kw))
    else:
        gather, gemm, act = q.fusedGatherQuantizeMxf8, q.grouped_matmul_mxf8_bf16_tn, (lambda x: q.fusedSiluMulQuantizeMxf8(x, h))
    aq, asf = gather(tok, h, src_row)
    gate_up = gemm(aq, dev["w13q"], asf, dev["w13s"], alpha13, offs)
    bq, bsf = act(gate_up, bias=dev["b1"], offs=offs) if layer.kind == "oai" else act(gate_up)
    y = gemm(bq, dev["w2q"], bsf, dev["w2s"], alpha2, offs)
    assert gate_up.shape == (mm.T * mm.TOPK, 2 * mm.I) and y.shape == (mm.T * mm.TOPK, mm.H)
    out = q.moe_combine(y, pos, weights, bias=dev["b2"], offs=offs) if layer.kind == "oai" else q.moe_combine(y, pos, weights)
    torch.cuda.synchronize()
    return weights, ids, offs, pos, out


@pytest.mark.parametrize("name", list(mm.MORE_LAYERS))
def test_more_moe_layers_against_the_fp64_model(q, name):
    layer = mm.make_layer(name)
    ids, weights, gap = mm.route_fp64(layer)
    assert gap > mm.MIN_GAP, gap
    wq_all = mm.quantize_weights(layer)               # on the CPU: the oracle, tests/_mxf8_quant_model.py, or the checkpoint's own bytes
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    shared = {"tok": _bf16(layer.tok), "h": _bf16(layer.h), "logits": up(layer.logits), "alpha13": up(layer.alpha13), "alpha2": up(layer.alpha2)}
    n_local = mm.E // layer.ranks
    partials = []
    for rank in ([None] if layer.ranks == 1 else range(layer.ranks)):
        kw = {} if rank is None else {"rank": rank}
        wq = wq_all if rank is None else more.rank_stacks(wq_all, rank)   # every rank holds its own weight and bias stacks
        l_fp64 = mm.layer_fp64(layer, ids, weights, **kw)
        l_q = mm.layer_quantized(layer, ids, weights, wq, **kw)
        noise = mm.fro(l_q - l_fp64)
        dev = dict(shared, **_upload(layer, wq))
        first = 0
        if rank is not None:
            dev["expert_map"], first = up(more.expert_map(rank)), rank * n_local
        mine = (ids >= first) & (ids < first + n_local)

        g_w, g_ids, g_offs, g_pos, out = _run_more(q, layer, dev, rank)
        assert np.array_equal(g_ids.cpu().numpy(), ids), np.nonzero((g_ids.cpu().numpy() != ids).any(axis=1))[0]   # the GLOBAL ids, on every rank
        assert np.abs(g_w.cpu().numpy().astype(np.float64) - weights).max() <= 1e-5
        ends = np.concatenate([[0], g_offs.cpu().numpy()])
        assert np.array_equal(np.diff(ends), np.bincount(ids[mine] - first, minlength=n_local))   # the bincount of the LOCAL experts
        g_pos = g_pos.cpu().numpy()
        assert np.array_equal(g_pos == -1, ~mine) and (g_pos[mine] < ends[-1]).all()              # -1 exactly on the other rank's slots
        if rank is None:
            assert mine.all()

        assert out.shape == (mm.T, mm.H) and out.dtype == torch.bfloat16
        l_gpu = out.float().cpu().numpy().astype(np.float64)
        assert np.isfinite(l_gpu).all()
        ratio = mm.fro(l_gpu - l_q) / noise
        print(f"{name} {kw}: |L_gpu - L_q| / |L_q - L_fp64| = {ratio:.3e}   (noise / |L_fp64| = {noise / mm.fro(l_fp64):.4f}, "
              f"|L_gpu - L_fp64| / |L_fp64| = {mm.fro(l_gpu - l_fp64) / mm.fro(l_fp64):.4f})")
        assert ratio <= BOUND, ratio
        partials.append(l_fp64)

        # the empty expert contributes nothing: its weight bytes replaced on the rank that holds it, the layer's bytes stay
        if first <= mm.EMPTY < first + n_local:
            assert ends[mm.EMPTY - first + 1] == ends[mm.EMPTY - first]
            for k in ("w13q", "w2q"):
                dev[k] = dev[k].clone()
                dev[k].view(torch.uint8)[mm.EMPTY - first] = 0x77
            again = _run_more(q, layer, dev, rank)[4]
            assert np.array_equal(bits(again), bits(out))
    if layer.ranks > 1:   # what the ranks are judged against adds up to the unsplit layer
        full = mm.layer_fp64(layer, ids, weights)
        assert np.abs(sum(partials) - full).max() <= 1e-12 * np.abs(full).max()
