"""fusedSwigluOaiQuantizeMxf8 on the GPU: the clamped SwiGLU of gpt-oss fused into the MXFP8 (e4m3) quantizer, the A operand of the W4A8 grouped GEMM.  Every
comparison is byte for byte: against the two-launch composition fusedQuantizeMxf8(swiglu_oai_and_mul(x, ...), h) (the contract), against the numpy models of the
activation and of the MXFP8 scale rule with a rotation that is not its own transpose (independent of both library ops), over a second round of the capped grid, on
the footprint arena, with malformed offs, under graph replay, and in a gpt-oss-shaped W4A8 layer.  The CPU half is tests/test_swiglu_oai_mxf8_cpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _footprint as fp  # noqa: E402
import _mxf8_quant_model as m8  # noqa: E402
import _rotations as rot  # noqa: E402
import _swiglu_oai_model as oai  # noqa: E402
from _rotations import bits as _np  # noqa: E402
from test_gpu_op_footprint import _groups, _int_bias  # noqa: E402
from test_gpu_swiglu_oai import MALFORMED, _bias, _experts, _hadamard, _offs, _offs_patterns  # noqa: E402

DEV = "cuda:0"
ALPHA, LIMIT = 1.702, 7.0      # gpt-oss
BF16, I32, E4M3, E8M0 = torch.bfloat16, torch.int32, torch.float8_e4m3fn, torch.float8_e8m0fnu


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    qutlass_amd.ops.register_torch_ops()
    return qutlass_amd


def _flat(sf: torch.Tensor, n: int) -> torch.Tensor:
    """the first n bytes of a scale buffer: the flat scales (the rest is the caller's)"""
    return sf.view(torch.uint8).reshape(-1)[:n]


# ------------------------------------------------------------------------------------------------
# 1. fused equals composition: codes and the first rows * I / 32 scale bytes
# ------------------------------------------------------------------------------------------------
def _assert_fused_equals_composition(q, x, h, bias, offs, ctx, alpha=ALPHA, limit=LIMIT):
    fc, fs = q.fusedSwigluOaiQuantizeMxf8(x, h, alpha=alpha, limit=limit, bias=bias, offs=offs)
    cc, cs = q.fusedQuantizeMxf8(q.swiglu_oai_and_mul(x, alpha=alpha, limit=limit, bias=bias, offs=offs), h)
    n = x.numel() // 2 // 32
    assert fc.shape == cc.shape == (*x.shape[:-1], x.size(-1) // 2) and fc.dtype == cc.dtype == E4M3, ctx
    assert fs.shape == cs.shape and fs.dtype == cs.dtype == E8M0, ctx
    a, b = fc.view(torch.uint8), cc.view(torch.uint8)
    assert torch.equal(a, b), (ctx, "codes", int((a != b).sum()))
    a, b = _flat(fs, n), _flat(cs, n)
    assert torch.equal(a, b), (ctx, "scales", int((a != b).sum()))


@pytest.mark.parametrize("R", [32, 64])
def test_fused_equals_composition(q, R):
    h = _hadamard(R)
    gen = torch.Generator(device="cpu").manual_seed(R * 7 + 8)
    shapes = [(rows, 2 * k * R) for rows in (1, 31, 33, 70) for k in (1, 3, 5)] + [(2, 35, 2 * 3 * R)]
    for shape in shapes:
        x = (torch.randn(*shape, generator=gen) * 4.0).to(BF16).to(DEV)
        M = x.numel() // shape[-1]
        _assert_fused_equals_composition(q, x, h, None, None, (R, shape, "no bias"))
        # one expert (with and without offs), boundaries at rows 31 / 32 / 33 (inside a 32-row tile for I > R), empty groups, one-row groups, 65 and 1024 experts, a tail
        for name, E, counts in _offs_patterns(M):
            bias = _bias(E, shape[-1], gen, 2.0)
            _assert_fused_equals_composition(q, x, h, bias, _offs(counts), (R, shape, name))
            if E == 1:
                _assert_fused_equals_composition(q, x, h, bias, None, (R, shape, "E1 without offs"))
    x = (torch.randn(33, 2 * 3 * R, generator=gen) * 4.0).to(BF16).to(DEV)
    _assert_fused_equals_composition(q, x, h, None, None, (R, "alpha 1, limit 2.5"), alpha=1.0, limit=2.5)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 2. independent of the composition: the numpy models, a rotation that differs from its transpose
# ------------------------------------------------------------------------------------------------
def _exact_case(R, rows, counts, seed):
    """-> (x (rows, 2 I) bf16, h, bias or None, offs or None, want codes (rows, I), want scales (rows * I / 32)), all on the CPU.  The exact regime of
    tests/test_gpu_op_footprint.py: gate = 100 (clamped to 7, where s = 7 in bf16), ups small integers, integer biases that keep both there -- the activation is
    7 * (-2 .. 4), every rotated sum is exact in fp32 in any order, so the models and the kernel must agree to the bit."""
    k = 3 * R
    h = rot.signed_permuted_hadamard(R, seed=1)
    up = rot.exact_input((rows, k), seed=seed, scale=1.0)
    x = torch.cat([torch.full((rows, k), 100.0, dtype=BF16), up], dim=1)
    bias = offs = None
    if counts is not None:
        assert int(np.sum(counts)) == rows
        bias, offs = _int_bias(len(counts), k, seed), np.cumsum(counts).astype(np.int32)
    act = oai.swiglu_oai(_np(x), ALPHA, LIMIT, None if bias is None else _np(bias), offs)
    assert set(np.unique(oai.bf16_to_f32(act))) <= {7.0 * i for i in range(-2, 5)}
    wq, ws = m8.quantize(m8.rotate(act, _np(h)), "e4m3")
    return x, h, bias, offs, np.ascontiguousarray(wq), np.ascontiguousarray(ws).reshape(-1)


@pytest.mark.parametrize("R", [32, 64])
@pytest.mark.parametrize("with_bias", [False, True])
def test_equals_the_numpy_models(q, R, with_bias):
    rows = 70
    x, h, bias, offs, wq, ws = _exact_case(R, rows, [25, 0, 1, 30, 14] if with_bias else None, seed=7 * R + rows)
    kw = dict(bias=bias.to(DEV), offs=torch.from_numpy(offs).to(DEV)) if with_bias else {}
    codes, sf = q.fusedSwigluOaiQuantizeMxf8(x.to(DEV), h.to(DEV), alpha=ALPHA, limit=LIMIT, **kw)
    got_q, got_s = _np(codes), _np(_flat(sf, ws.size))
    assert np.array_equal(got_s, ws), ("scales", int((got_s != ws).sum()), ws.size)
    assert np.array_equal(got_q, wq), ("codes", int((got_q != wq).sum()), wq.size)
    # the precondition of "pins orientation": h.T gives other bytes
    tq, _ = m8.quantize(m8.rotate(oai.swiglu_oai(_np(x), ALPHA, LIMIT, None if bias is None else _np(bias), offs), _np(h.T.contiguous())), "e4m3")
    assert not np.array_equal(tq, wq)
    if with_bias:   # ... and of "pins the expert lookup": expert 0's bias for every row gives other bytes
        zq, _ = m8.quantize(m8.rotate(oai.swiglu_oai(_np(x), ALPHA, LIMIT, _np(bias[:1]), None), _np(h)), "e4m3")
        assert not np.array_equal(zq, wq)


# ------------------------------------------------------------------------------------------------
# 3. a second, partial round of the capped grid
# ------------------------------------------------------------------------------------------------
def test_fused_equals_composition_second_grid_round(q):
    """The grid cap belongs to quant_fill / quant_grid and depends on the rotation size alone, not on the code format: it is the MXFP4 form's, 8 workgroups of 4
    waves per CU at R = 32, 8192 waves on 256 CUs.  2051 x 4608 outputs are 9230 tiles of 32 x 32, the last one half full: 1038 waves walk a second tile (and the
    look-ahead of the expert lookup runs a second, partial round) -- the shape of tests/test_gpu_swiglu_oai.py's MXFP4 test."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    launch = fp.quant_launch(2051 * 4608, 32, cus)
    assert 0 < launch.second_trip < 4 * launch.grid and launch.last_rows < 32, launch
    h = _hadamard(32)
    gen = torch.Generator(device="cpu").manual_seed(32)
    x = (torch.randn(2051, 2 * 4608, generator=gen) * 4.0).to(BF16).to(DEV)
    _assert_fused_equals_composition(q, x, h, None, None, "no bias")
    name, E, counts = _offs_patterns(2051)[2]
    _assert_fused_equals_composition(q, x, h, _bias(E, 2 * 4608, gen, 2.0), _offs(counts), name)


# ------------------------------------------------------------------------------------------------
# 4. footprint: nothing outside rows * I code bytes and rows * I / 32 scale bytes is written
# ------------------------------------------------------------------------------------------------
def _footprint_cases():
    return [dict(rows=r) for r in fp.ROWS] + [dict(rows=fp.M_ROWS, e65=False), dict(rows=fp.M_ROWS, e65=True)]


@pytest.mark.parametrize("R", [32, 64])
def test_footprint(q, R):
    for v in _footprint_cases():
        rows, k = v["rows"], 3 * R
        counts = _groups(v["e65"])[0] if "e65" in v else None
        x, h, bias, offs, wq, ws = _exact_case(R, rows, counts, seed=7 * R + rows)
        lay = fp.Layout().input("A", x).input("R", h)
        if bias is not None:
            lay.input("bias", bias).input("offs", torch.from_numpy(offs))
        ext = fp.quant_extents("mxf8", (rows, k), False, True)
        assert ext["OUT"] == (rows * k, rows * k) and ext["OUT_sf"][1] == rows * k // 32 < ext["OUT_sf"][0]   # a caller-owned tail behind the flat scales
        for nm, (nbytes, extent) in ext.items():
            lay.output(nm, nbytes, extent)

        def call(a):
            b = a.t("bias", BF16, len(counts), 2 * k) if bias is not None else torch.empty(0, dtype=BF16, device=DEV)
            o = a.t("offs", I32) if bias is not None else torch.empty(0, dtype=I32, device=DEV)
            torch.ops.qutlass_amd.fusedSwigluOaiQuantizeMxf8_(a.t("A", BF16, rows, 2 * k), a.t("R", BF16, R, R), a.t("OUT", E4M3), a.t("OUT_sf", E8M0), ALPHA, LIMIT, b, o)

        res = fp.run_twice(lay, call, DEV)
        ctx = (R, tuple(sorted(v.items())))
        assert np.array_equal(res["OUT_sf"], ws), (ctx, "scales", int((res["OUT_sf"] != ws).sum()))
        assert np.array_equal(res["OUT"], wq.reshape(-1)), (ctx, "codes", int((res["OUT"] != wq.reshape(-1)).sum()))


@pytest.mark.parametrize("R", [32, 64])
def test_scale_padding_keeps_its_fill(q, R):
    gen = torch.Generator(device="cpu").manual_seed(5)
    h = _hadamard(R)
    M, inter = 33, 3 * R
    x = (torch.randn(M, 2 * inter, generator=gen) * 4.0).to(BF16).to(DEV)
    bias, offs = _bias(3, 2 * inter, gen), torch.tensor([10, 20, 33], dtype=I32, device=DEV)
    codes, sf = q.ops.alloc_quant(q.ops.QUANT_OPS["swiglu_oai_quantize_mxf8"], x, h)
    n = M * inter // 32
    assert sf.numel() > n and codes.dtype == E4M3 and codes.shape == (M, inter)
    sf.view(torch.uint8).fill_(0xAB)
    torch.ops.qutlass_amd.fusedSwigluOaiQuantizeMxf8_(x, h, codes, sf, ALPHA, LIMIT, bias, offs)
    want = q.fusedSwigluOaiQuantizeMxf8(x, h, bias=bias, offs=offs)
    flat = sf.view(torch.uint8).reshape(-1)
    assert torch.equal(codes.view(torch.uint8), want[0].view(torch.uint8)) and torch.equal(flat[:n], _flat(want[1], n))
    assert bool((flat[n:] == 0xAB).all())


# ------------------------------------------------------------------------------------------------
# 5. malformed offs: the call completes, every row is some single expert's
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [32, 64])
@pytest.mark.parametrize("offs", MALFORMED)
def test_malformed_offs_select_some_expert(q, R, offs):
    gen = torch.Generator(device="cpu").manual_seed(sum(o % 97 for o in offs) + R)
    M, inter, E = 70, 2 * R, 3
    n = inter // 32
    x = (torch.randn(M, 2 * inter, generator=gen) * 3.0).to(BF16).to(DEV)
    bias, o = _bias(E, 2 * inter, gen, 2.0), torch.tensor(offs, dtype=I32, device=DEV)
    h = _hadamard(R)
    fc, fs = q.fusedSwigluOaiQuantizeMxf8(x, h, bias=bias, offs=o)
    fc, fs = fc.view(torch.uint8), _flat(fs, M * n).view(M, n)
    ok = torch.zeros(M, dtype=torch.bool, device=DEV)
    for e in range(E):
        wc, ws = q.fusedSwigluOaiQuantizeMxf8(x, h, bias=bias[e:e + 1].contiguous())      # the op with that single expert's bias
        ok |= (fc == wc.view(torch.uint8)).all(dim=1) & (fs == _flat(ws, M * n).view(M, n)).all(dim=1)
    torch.cuda.synchronize()
    assert bool(ok.all()), (offs, (~ok).nonzero().flatten().tolist())


# ------------------------------------------------------------------------------------------------
# 6. graph capture: offs, bias and x are read on the device
# ------------------------------------------------------------------------------------------------
def test_graph_replay_follows_offs_bias_and_x(q):
    h = _hadamard(64)
    gen = torch.Generator(device="cpu").manual_seed(78)
    M, inter, E = 70, 192, 5
    n = M * inter // 32
    cases = []
    for counts in ([70, 0, 0, 0, 0], [10, 0, 25, 5, 30], [1, 1, 1, 1, 2]):      # all rows in one expert; empty groups; one-row groups and a tail
        cases.append(((torch.randn(M, 2 * inter, generator=gen) * 4.0).to(BF16).to(DEV), _bias(E, 2 * inter, gen, 2.0), _offs(np.array(counts))))
    eager = []
    for x, b, o in cases:
        c, s = q.fusedSwigluOaiQuantizeMxf8(x, h, bias=b, offs=o)
        eager.append((c.view(torch.uint8).clone(), _flat(s, n).clone()))
    assert not torch.equal(eager[0][0], eager[1][0])
    sx, sb, so = (t.clone() for t in cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        q.fusedSwigluOaiQuantizeMxf8(sx, h, bias=sb, offs=so)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = q.fusedSwigluOaiQuantizeMxf8(sx, h, bias=sb, offs=so)
    for (x, b, o), (wc, ws) in zip(cases[::-1], eager[::-1]):
        sx.copy_(x)
        sb.copy_(b)
        so.copy_(o)
        cap[0].view(torch.uint8).zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap[0].view(torch.uint8), wc) and torch.equal(_flat(cap[1], n), ws)


# ------------------------------------------------------------------------------------------------
# 7. a gpt-oss-shaped W4A8 layer: MXFP4 expert weights as stored, 8-bit tokens
# ------------------------------------------------------------------------------------------------
def test_gpt_oss_w4a8_layer_equals_the_torch_bias_composition(q):
    T, E, topk, H, I, R = 40, 4, 2, 128, 128, 32
    h = _hadamard(R)
    gen = torch.Generator(device="cpu").manual_seed(12)
    tok = torch.randn(T, H, generator=gen).to(BF16).to(DEV)
    w13 = (torch.randn(E, 2 * I, H, generator=gen) * 0.2).to(BF16).to(DEV)
    w2 = (torch.randn(E, H, I, generator=gen) * 0.2).to(BF16).to(DEV)
    b1, b2 = _bias(E, 2 * I, gen), _bias(E, H, gen)
    alpha = torch.ones(1, device=DEV)
    logits = torch.randn(T, E, generator=gen)
    logits[:, 2] = -float("inf")                                          # expert 2 is never chosen: one empty group
    logits = logits.to(DEV)

    def quant_w(w):   # (E, N, K) -> e2m1 codes (E, N, K/2), row-major e8m0 scales (E * N * K / 32): quantized once
        c, s = q.fusedQuantizeMx(w.view(-1, w.size(-1)), h, method="abs_max")
        return c.view(w.size(0), w.size(1), -1), _flat(s, w.numel() // 32).clone().view(E8M0)

    w13q, w13s = quant_w(w13)
    w2q, w2s = quant_w(w2)
    weights, ids, src_row, offs, pos = q.moe_route(logits, topk)
    counts = np.diff(np.concatenate([[0], _np(offs)]))
    assert counts[2] == 0 and (counts[[0, 1, 3]] > 0).all() and counts.sum() == T * topk
    aq, asf = q.fusedGatherQuantizeMxf8(tok, h, src_row)
    assert aq.dtype == E4M3
    gate_up = q.grouped_matmul_mxf8_mxf4_bf16_tn(aq, w13q, asf, w13s, alpha, offs)

    def tail(bias2):
        bq, bsf = q.fusedSwigluOaiQuantizeMxf8(gate_up, h, bias=b1, offs=offs)
        return q.moe_combine(q.grouped_matmul_mxf8_mxf4_bf16_tn(bq, w2q, bsf, w2s, alpha, offs), pos, weights, bias=bias2, offs=offs)

    out = tail(b2)
    e = _experts(offs, T * topk)
    cq, csf = q.fusedQuantizeMxf8(q.swiglu_oai_and_mul(gate_up + b1[e]), h)      # the biases added by torch, the activation by the two launches
    ref = q.moe_combine(q.grouped_matmul_mxf8_mxf4_bf16_tn(cq, w2q, csf, w2s, alpha, offs) + b2[e], pos, weights)
    torch.cuda.synchronize()
    assert out.shape == (T, H) and out.dtype == BF16
    assert np.array_equal(_np(out), _np(ref)), int((_np(out) != _np(ref)).sum())
    assert np.isfinite(out.float().cpu().numpy()).all() and float(out.float().abs().max()) > 0
    # changing expert 3's down bias changes exactly the tokens routed to it
    b2x = b2.clone()
    b2x[3] += 1.0
    changed = (tail(b2x).view(torch.int16) != out.view(torch.int16)).any(dim=1)
    assert torch.equal(changed, (ids == 3).any(dim=1)) and bool(changed.any()) and not bool(changed.all())
