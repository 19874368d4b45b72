"""The gate/up W4A16 grouped GEMM on NVFP4 weights with fused activation (grouped_matmul_bf16_nvf4_silu_bf16_tn / ..._swiglu_oai_bf16_tn) on the MI355X: its bits
against the two launches it replaces -- grouped_matmul_bf16_nvf4_bf16_tn, then silu_and_mul / swiglu_oai_and_mul -- and against fp64 mathematics.

K values (a stage is 128 elements): both forms run one shot with 1 and 2 slots per wave (K <= 512, 1024) and rings of 2 beyond -- 128, the K on either side of
both rungs, and 2688 (21 stages: the ring of 2 wraps twice, waves 1 ... 3 end on a zero-filled slot).  fp64_case() needs no GPU: tests/test_grouped_bf16_nvf4_act_cpu.py
asserts its operands exact and its gates' range."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _benchlib as lab  # noqa: E402  (the LAB build: forced forms)
import _bf16_nvf4_model as W  # noqa: E402
import _swiglu_oai_model as S  # noqa: E402
import qutlass_amd as q  # noqa: E402

DEV, E4M3 = "cuda:0", torch.float8_e4m3fn
KS, K_NAN = (128, 512, 640, 1024, 1152, 2688), 640
COUNTS, TRAIL, INTER = (0, 1, 33, 70), 5, 96   # an empty group, one row, crossings of 32 and 64 rows; three column tiles, the up half starts inside the gate range
ACTS, ACT_ALPHA, LIMIT, SENTINEL = ("silu", "oai", "oai_bias"), 1.702, 7.0, 0x5A5A
FP64_COUNTS, FP64_ALPHA = (33, 70), np.array([2.0 ** -7, 2.0 ** -8])

_offs = lambda counts: torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)   # noqa: E731
_bits = lambda t: t.view(torch.int16)   # noqa: E731
_spans = lambda g: g.min() < -LIMIT and g.max() > LIMIT and ((g > 0) & (g < LIMIT)).any() and ((g < 0) & (g > -LIMIT)).any()   # noqa: E731


def _operands(E, inter, K, M, seed, gate_big=None, nan_rows=None):
    """device operands from a seeded generator: Gaussian bf16 tokens, random e2m1 code bytes, e4m3 scale bytes of either sign with magnitudes in [0.125, 0.9375] (all
    eight mantissas), which put the outputs around the activation's knee and clamp; gate_big: that expert's gate-row scale exponents raised by 8 (x 256, the largest byte 0x77 / 0xf7: finite);
    nan_rows (expert, gate row, up row): a scale byte 0x7f in the gate row and 0xff in the up row"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    b = torch.randint(0, 256, (E, 2 * inter, K // 2), generator=g, dtype=torch.uint8)
    bsf = torch.randint(0x20, 0x38, (E, 2 * inter, K // 16), generator=g, dtype=torch.uint8) | (torch.randint(0, 2, (E, 2 * inter, K // 16), generator=g, dtype=torch.uint8) << 7)
    if gate_big is not None:
        bsf[gate_big, :inter] += 8 << 3
    if nan_rows is not None:
        bsf[nan_rows[0], nan_rows[1], 0] = 0x7F
        bsf[nan_rows[0], inter + nan_rows[2], -1] = 0xFF
    bias = (torch.randn(E, 2 * inter, generator=g) * 2).to(torch.bfloat16)
    return a.to(DEV), b.to(DEV), bsf.to(DEV).view(E4M3), bias.to(DEV)


def _chain(act, ops, alpha, offs, bias, src_row=None):
    """the two launches: (y (M, 2 I), act (M, I))"""
    y = q.grouped_matmul_bf16_nvf4_bf16_tn(*ops, alpha, offs, src_row=src_row)
    if act == "silu":
        return y, q.silu_and_mul(y)
    return y, q.swiglu_oai_and_mul(y, alpha=ACT_ALPHA, limit=LIMIT, bias=bias if act == "oai_bias" else None, offs=offs if act == "oai_bias" else None)


def _op(act, ops, alpha, offs, bias, src_row=None):
    if act == "silu":
        return q.grouped_matmul_bf16_nvf4_silu_bf16_tn(*ops, alpha, offs, src_row=src_row)
    return q.grouped_matmul_bf16_nvf4_swiglu_oai_bf16_tn(*ops, alpha, offs, act_alpha=ACT_ALPHA, limit=LIMIT, bias=bias if act == "oai_bias" else None, src_row=src_row)


@functools.lru_cache(maxsize=None)
def _problem(K, act):
    """operands of one K and the chain's bits on them: computed once, shared by the forms"""
    E, M = len(COUNTS), sum(COUNTS) + TRAIL
    *ops, bias = _operands(E, INTER, K, M, seed=K, nan_rows=(3, 37, 5) if K == K_NAN else None)   # gate row 37 and up row 5 of expert 3: two column tiles
    alpha = torch.tensor([0.5, 0.25, 0.125, 0.375], device=DEV)
    offs = _offs(COUNTS)
    y, want = _chain(act, ops, alpha, offs, bias)
    gate = y[:sum(COUNTS), :INTER].float()
    assert _spans(gate[~gate.isnan()]), "the gates do not straddle 0 and +-limit"
    return ops, bias, alpha, offs, want


def _entry(form, act, ops, alpha, offs, bias, out, shape, src_row=None, T=0):
    """the C entry on a caller's buffer: the lab library under a forced form, the product library and its rule for form 0"""
    lib = lab.load() if form else q._lib.load()
    f = lib.qutlass_amd_grouped_matmul_bf16_nvf4_act_bf16_tn
    f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_void_p] * 2 + [ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 2 + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    args = (*(t.data_ptr() for t in ops), alpha.data_ptr(), alpha.numel(), offs.data_ptr(), None if src_row is None else src_row.data_ptr(), T, 0 if act == "silu" else 1,
            ACT_ALPHA, LIMIT, bias.data_ptr() if act == "oai_bias" else None, out.data_ptr(), *shape, torch.cuda.current_stream().cuda_stream)
    if form:
        with lab.forced(gemm_variant=form):
            rc = f(*args)
    else:
        rc = f(*args)
    assert rc == 0, lib.qutlass_amd_last_error().decode()
    torch.cuda.synchronize()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("form", (0, 622, 623))
def test_bits_equal_the_chain(form, K, act):
    ops, bias, alpha, offs, want = _problem(K, act)
    E, end, M = len(COUNTS), sum(COUNTS), sum(COUNTS) + TRAIL
    out = torch.full((M, INTER), SENTINEL, dtype=torch.int16, device=DEV)
    _entry(form, act, ops, alpha, offs, bias, out, (M, 2 * INTER, K, E))
    if K == K_NAN:
        nan = want[:end].isnan()
        assert bool(nan[34:, 37].all()) and bool(nan[34:, 5].all()) and int(nan.sum()) == 2 * COUNTS[3], "the chain's NaN are not the two poisoned columns of expert 3"
    bad = (out[:end] != _bits(want)[:end]).nonzero()
    assert bad.numel() == 0, f"{bad.size(0)} elements differ, first at (row, column) {bad[0].tolist()}"
    assert bool((out[end:] == SENTINEL).all()), "rows at or past offs[E-1] were written"


@pytest.mark.parametrize("form", (622, 623))
def test_gather(form):
    K, act, E, end, M, T = 640, "oai_bias", len(COUNTS), sum(COUNTS), sum(COUNTS) + TRAIL, 40
    (_, *wops), bias, alpha, offs, _ = _problem(K, act)
    g = torch.Generator(device="cpu").manual_seed(form)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16).to(DEV)
    src = torch.randint(0, T, (M,), generator=g, dtype=torch.int32)   # M > T: duplicates
    src[2], src[40], src[100] = -1, T, -1
    src = src.to(DEV)
    oor = (src < 0) | (src >= T)
    xs = x.index_select(0, src.clamp(0, T - 1).long())
    xs[oor] = 0
    got = torch.full((M, INTER), SENTINEL, dtype=torch.int16, device=DEV)
    _entry(form, act, (x, *wops), alpha, offs, bias, got, (M, 2 * INTER, K, E), src_row=src, T=T)
    sorted_ = torch.full((M, INTER), SENTINEL, dtype=torch.int16, device=DEV)
    _entry(form, act, (xs, *wops), alpha, offs, bias, sorted_, (M, 2 * INTER, K, E))
    want = _chain(act, (x, *wops), alpha, offs, bias, src_row=src)[1]
    assert torch.equal(got[:end], _bits(want)[:end]) and torch.equal(got, sorted_)


@functools.lru_cache(maxsize=None)
def fp64_case(K):
    """numpy only: the exact-regime problem, its bias bits and the fp64 GEMM rounded once to bf16 (M, 2 I) -- nothing of the GPU code"""
    p = W.exact_problem(len(FP64_COUNTS), 2 * INTER, K, sum(FP64_COUNTS), seed=K)
    bias_bits = S.f32_to_bf16(np.random.default_rng(K).standard_normal((p.E, 2 * INTER)).astype(np.float32))
    return p, bias_bits, W.to_bf16_bits(W.reference_f64(p, FP64_COUNTS, FP64_ALPHA)).numpy().view(np.uint16)


def fp64_gates(K, biased):
    p, bias_bits, y_bits = fp64_case(K)
    rows = S.group_of_rows(np.cumsum(FP64_COUNTS), np.arange(p.M))
    return S.bf16_to_f64(y_bits)[:, :INTER] + (S.bf16_to_f64(bias_bits)[rows][:, :INTER] if biased else 0.0)


@pytest.mark.parametrize("act", ("silu", "oai_bias"))
@pytest.mark.parametrize("K", (512, 1152))
@pytest.mark.parametrize("form", (622, 623))
def test_against_fp64_mathematics(form, K, act):
    """oai_bias: bit for bit the numpy model; silu: silu_and_mul's definition bf16(bf16(g / (1 + exp(-g))) u) in fp64 on the bf16 GEMM values, held as
    tests/test_gpu_gated_quantize.py holds silu_and_mul -- every output within one bf16 ulp, at least 99 % bit-equal (the kernel's exp and division are fp32)"""
    p, bias_bits, y_bits = fp64_case(K)
    assert _spans(fp64_gates(K, act == "oai_bias")), "the gates do not span the clamp and zero"
    out = torch.empty(p.M, INTER, dtype=torch.int16, device=DEV)
    _entry(form, act, p.device(DEV), torch.from_numpy(FP64_ALPHA).float().to(DEV), _offs(FP64_COUNTS), torch.from_numpy(bias_bits.view(np.int16)).view(torch.bfloat16).to(DEV),
           out, (p.M, 2 * INTER, K, p.E))
    got = out.cpu().numpy().view(np.uint16)
    if act == "oai_bias":
        bad = np.argwhere(got != S.swiglu_oai(y_bits, ACT_ALPHA, LIMIT, bias_bits, np.cumsum(FP64_COUNTS)))
        assert bad.size == 0, f"{len(bad)} elements differ from fp64 mathematics, first at {bad[0].tolist()}"
    else:
        gate, up = S.bf16_to_f64(y_bits[:, :INTER]), S.bf16_to_f64(y_bits[:, INTER:])
        with np.errstate(over="ignore"):
            want = S.f64_to_bf16(S.bf16_to_f64(S.f64_to_bf16(gate / (1.0 + np.exp(-gate)))) * up)
        d = np.abs(S.bf16_line(got) - S.bf16_line(want))
        print(f"silu form {form} K {K}: bit-equal {float((d == 0).mean()):.5f}, max distance {int(d.max())} bf16 ulp")
        assert int(d.max()) <= 1 and float((d == 0).mean()) >= 0.99


@pytest.mark.parametrize("act", ACTS)
def test_signed_zero_and_clamp_edges(act):
    E, M, K, inter = 2, 64, 256, 64
    *ops, bias = _operands(E, inter, K, M, seed=5, gate_big=1)   # expert 1's gate outputs x 256; its up outputs stay ordinary
    alpha, offs = torch.ones(1, device=DEV), _offs([32, 32])
    y, want = _chain(act, ops, alpha, offs, bias)
    gate = y[32:, :inter].float()
    assert float(gate.min()) < -200 and float(gate.max()) > LIMIT, "the operands do not reach the cases this test is about"
    assert int((_bits(want) == -0x8000).sum()) > 0, "no activation of -0 among the operands"
    assert torch.equal(_bits(_op(act, ops, alpha, offs, bias)), _bits(want))


def test_graph_capture_and_compile():
    E, M, K, inter = 8, 101, 256, 64
    *ops, bias = _operands(E, inter, K, M, seed=9)
    alpha, offs = torch.linspace(0.125, 0.5, E, device=DEV), _offs([12] * 8)
    run = lambda: _op("oai_bias", ops, alpha, offs, bias)   # noqa: E731
    eager = run()        # (also the warm-up off the capture)
    assert eager.dtype == torch.bfloat16 and tuple(eager.shape) == (M, inter)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for counts in ([12] * 8, [0, 40, 1, 7, 20, 3, 9, 16], [101, 0, 0, 0, 0, 0, 0, 0]):
        offs.copy_(_offs(counts))
        want = _chain("oai_bias", ops, alpha, offs, bias)[1]
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out)[:sum(counts)], _bits(want)[:sum(counts)]) and torch.equal(_bits(run())[:sum(counts)], _bits(want)[:sum(counts)])
    compiled = torch.compile(lambda *t: q.grouped_matmul_bf16_nvf4_swiglu_oai_bf16_tn(*t[:5], bias=t[5]), backend="eager", fullgraph=True)(*ops, alpha, offs, bias)
    assert torch.equal(_bits(compiled), _bits(run()))
