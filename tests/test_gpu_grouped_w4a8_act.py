"""The gate/up W4A8 grouped GEMM with fused activation and MXFP8 output (grouped_matmul_mxf8_mxf4_silu_mxf8_tn / ..._swiglu_oai_mxf8_tn) on the MI355X: its bytes
against the two launches it replaces -- grouped_matmul_mxf8_mxf4_bf16_tn, then fusedSiluMulQuantizeMxf8 / fusedSwigluOaiQuantizeMxf8 with the identity of 32 --
and once against fp64 mathematics.

K values (a stage is 128 elements): form 614 runs one shot with 1 ... 4 slots per wave (K <= 512, 1024, 1536, 2048) and rings of 4 beyond, form 615 one shot up to
K = 1536 and rings of 3 beyond -- 128, the K on either side of every rung, and a ring that wraps twice (5120: 10 stages per wave on 4 slots; 3584: 7 on 3)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _benchlib as lab  # noqa: E402  (the LAB build: forced forms)
import _mxf8_quant_model as Q  # noqa: E402
import _swiglu_oai_model as S  # noqa: E402
import _w4a8_model as W  # noqa: E402
import qutlass_amd as q  # noqa: E402

DEV, E4, E8M0 = "cuda:0", torch.float8_e4m3fn, torch.float8_e8m0fnu
K614, K615 = (128, 512, 640, 1024, 1152, 1536, 1664, 2048, 2176, 5120), (128, 512, 640, 1024, 1152, 1536, 1664, 3584)
CASES = [(f, k) for f, ks in ((0, K614), (614, K614), (615, K615)) for k in ks]   # 0: the product library and its rule (614 at these group sizes)
COUNTS, TRAIL, INTER = (0, 1, 33, 70), 5, 96   # an empty group, one row, crossings of 32 and 64 rows; three column tiles, the up half starts inside the gate range
ACTS, ACT_ALPHA, LIMIT, SENTINEL = ("silu", "oai", "oai_bias"), 1.702, 7.0, 0xA5


_offs = lambda counts: torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)   # noqa: E731


def _operands(E, inter, K, M, seed, gate_shift=None):
    """device operands from a seeded generator: e4m3 tokens, packed e2m1 weights, scale bytes that put the outputs around the activation's knee;
    gate_shift (expert, bytes): that expert's gate-row scale bytes raised"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = (torch.randn(M, K, generator=g) * 1.5).to(E4)
    b = torch.randint(0, 256, (E, 2 * inter, K // 2), generator=g, dtype=torch.uint8)
    asf = torch.randint(125, 130, (M, K // 32), generator=g, dtype=torch.uint8)
    bsf = torch.randint(121, 126, (E, 2 * inter, K // 32), generator=g, dtype=torch.uint8)
    if gate_shift is not None:
        bsf[gate_shift[0], :inter] += gate_shift[1]
    bias = (torch.randn(E, 2 * inter, generator=g) * 2).to(torch.bfloat16)
    return a.to(DEV), b.to(DEV), asf.reshape(-1).to(DEV).view(E8M0), bsf.reshape(-1).to(DEV).view(E8M0), bias.to(DEV)


def _chain(act, ops, alpha, offs, bias):
    """the two launches: (codes (M, I) uint8, flat scale bytes)"""
    y = q.grouped_matmul_mxf8_mxf4_bf16_tn(*ops, alpha, offs)
    eye = torch.eye(32, dtype=torch.bfloat16, device=DEV)
    if act == "silu":
        c, s = q.fusedSiluMulQuantizeMxf8(y, eye)
    else:
        c, s = q.fusedSwigluOaiQuantizeMxf8(y, eye, alpha=ACT_ALPHA, limit=LIMIT, bias=bias if act == "oai_bias" else None, offs=offs if act == "oai_bias" else None)
    return y, c.view(torch.uint8), s.view(torch.uint8).reshape(-1)


@functools.lru_cache(maxsize=None)
def _problem(K, act):
    """operands of one K and the chain's bytes on them: computed once, shared by the forms"""
    E, M = len(COUNTS), sum(COUNTS) + TRAIL
    *ops, bias = _operands(E, INTER, K, M, seed=K)
    alpha = torch.tensor([0.5, 0.25, 0.125, 0.375], device=DEV)
    offs = _offs(COUNTS)
    _, codes, scales = _chain(act, ops, alpha, offs, bias)
    return ops, bias, alpha, offs, codes, scales


def _entry(lib, act, ops, alpha, offs, bias, codes, scales, shape):
    """the C entry of `lib` (the product or the lab library) on caller buffers"""
    f = lib.qutlass_amd_grouped_matmul_mxf8_mxf4_act_mxf8_tn
    f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 3 + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    rc = f(*(t.data_ptr() for t in ops), alpha.data_ptr(), alpha.numel(), offs.data_ptr(), 0 if act == "silu" else 1, ACT_ALPHA, LIMIT,
           bias.data_ptr() if act == "oai_bias" else None, codes.data_ptr(), scales.data_ptr(), *shape, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.qutlass_amd_last_error().decode()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("form,K", CASES)
def test_bytes_equal_the_chain(form, K, act):
    ops, bias, alpha, offs, want_c, want_s = _problem(K, act)
    E, end, M, G = len(COUNTS), sum(COUNTS), sum(COUNTS) + TRAIL, INTER // 32
    codes = torch.full((M, INTER), SENTINEL, dtype=torch.uint8, device=DEV)
    scales = torch.full((M * G,), SENTINEL, dtype=torch.uint8, device=DEV)
    if form:
        with lab.forced(gemm_variant=form):
            _entry(lab.load(), act, ops, alpha, offs, bias, codes, scales, (M, 2 * INTER, K, E))
    else:
        _entry(q._lib.load(), act, ops, alpha, offs, bias, codes, scales, (M, 2 * INTER, K, E))
    torch.cuda.synchronize()
    bad = (codes[:end] != want_c[:end]).nonzero()
    assert bad.numel() == 0, f"{bad.size(0)} code bytes differ, first at (row, column) {bad[0].tolist()}"
    bad = (scales[:end * G] != want_s[:end * G]).nonzero()
    assert bad.numel() == 0, f"{bad.size(0)} scale bytes differ, first at (row, group) {divmod(int(bad[0]), G)}"
    assert bool((codes[end:] == SENTINEL).all()) and bool((scales[end * G:] == SENTINEL).all()), "rows at or past offs[E-1] were written"


@pytest.mark.parametrize("act", ACTS)
def test_dense_case_shared_alpha(act):
    M, K, inter = 70, 640, 32
    *ops, bias = _operands(1, inter, K, M, seed=3)
    alpha, offs = torch.full((1,), 0.25, device=DEV), _offs([M])
    _, want_c, want_s = _chain(act, ops, alpha, offs, bias)
    if act == "silu":
        c, s = q.grouped_matmul_mxf8_mxf4_silu_mxf8_tn(*ops, alpha, offs)
    else:
        c, s = q.grouped_matmul_mxf8_mxf4_swiglu_oai_mxf8_tn(*ops, alpha, offs, act_alpha=ACT_ALPHA, limit=LIMIT, bias=bias if act == "oai_bias" else None)
    assert c.dtype == E4 and tuple(c.shape) == (M, inter) and s.dtype == E8M0 and tuple(s.shape) == (128, 4)
    assert torch.equal(c.view(torch.uint8), want_c) and torch.equal(s.view(torch.uint8).reshape(-1)[:M], want_s[:M])


@pytest.mark.parametrize("act", ("silu", "oai"))
def test_signed_zero_and_saturation(act):
    E, M, K, inter = 2, 64, 256, 64
    *ops, bias = _operands(E, inter, K, M, seed=5, gate_shift=(1, 12))   # expert 1's gate outputs x 4096; its up outputs stay ordinary
    alpha, offs = torch.ones(1, device=DEV), _offs([32, 32])
    y, want_c, want_s = _chain(act, ops, alpha, offs, bias)
    gate = y[32:, :inter].float()
    assert float(gate.min()) < -200 and float(gate.max()) > LIMIT, "the operands do not reach the cases this test is about"
    f = q.grouped_matmul_mxf8_mxf4_silu_mxf8_tn if act == "silu" else q.grouped_matmul_mxf8_mxf4_swiglu_oai_mxf8_tn
    c, s = f(*ops, alpha, offs)
    assert torch.equal(c.view(torch.uint8), want_c) and torch.equal(s.view(torch.uint8).reshape(-1)[:M * inter // 32], want_s[:M * inter // 32])
    # what the chain makes of an activation that is -0: its identity rotation accumulates onto +0, so the code is +0 (0x00), not -0 (0x80)
    neg0 = (q.silu_and_mul(y) if act == "silu" else q.swiglu_oai_and_mul(y, alpha=ACT_ALPHA, limit=LIMIT)).view(torch.int16) == -0x8000
    assert int(neg0.sum()) > 0, "no activation of -0 among the operands"
    assert bool((want_c[neg0] == 0).all()), "the chain stores an activation of -0 as something other than the +0 code"


def test_against_fp64():
    """Measured on an MI355X: the op 0.026094, the CPU models' own chain 0.026094."""
    E, inter, K, counts = 2, 64, 512, (16, 48)
    M, alpha, offs_np = sum(counts), np.array([2.0 ** -6, 2.0 ** -7]), np.cumsum(counts)
    p = W.exact_problem(E, 2 * inter, K, M, seed=17)
    bias_bits = S.f32_to_bf16(np.random.default_rng(17).standard_normal((E, 2 * inter)).astype(np.float32))
    x = W.reference_f64(p, counts, alpha) + S.bf16_to_f64(bias_bits)[S.group_of_rows(offs_np, np.arange(M))]
    gc, uc = np.minimum(x[:, :inter], LIMIT), np.clip(x[:, inter:], -LIMIT, LIMIT)
    ref = (uc + 1.0) * gc / (1.0 + np.exp(-float(np.float32(ACT_ALPHA)) * gc))
    # ref: fp64 mathematics, nothing rounded after the operands.  The CPU models' own chain on them: bf16 GEMM output, activation, identity rotation, e4m3 quantizer
    y_bits = W.to_bf16_bits(W.reference_f64(p, counts, alpha)).numpy().view(np.uint16)
    act_bits = S.swiglu_oai(y_bits, ACT_ALPHA, LIMIT, bias_bits, offs_np)
    mc, ms = Q.quantize(Q.rotate(act_bits, S.f32_to_bf16(np.eye(32, dtype=np.float32))), "e4m3")
    err_model = np.linalg.norm(Q.dequantize(mc, ms, "e4m3") - ref) / np.linalg.norm(ref)
    c, s = q.grouped_matmul_mxf8_mxf4_swiglu_oai_mxf8_tn(*p.device(DEV), torch.from_numpy(alpha).float().to(DEV), _offs(counts), act_alpha=ACT_ALPHA, limit=LIMIT,
                                                         bias=torch.from_numpy(bias_bits.view(np.int16)).view(torch.bfloat16).to(DEV))
    got = Q.dequantize(c.view(torch.uint8).cpu().numpy(), s.view(torch.uint8).reshape(-1)[:M * inter // 32].cpu().numpy().reshape(M, inter // 32), "e4m3")
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"relative Frobenius error against fp64: op {err:.6f}, CPU models' chain {err_model:.6f}")
    assert err <= 1.05 * err_model, (err, err_model)


def test_graph_capture():
    ops, bias, alpha, offs, want_c, want_s = _problem(1152, "oai_bias")
    end, G = sum(COUNTS), INTER // 32
    op = lambda: q.grouped_matmul_mxf8_mxf4_swiglu_oai_mxf8_tn(*ops, alpha, offs, act_alpha=ACT_ALPHA, limit=LIMIT, bias=bias)
    eager_c, eager_s = op()        # (also the warm-up off the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c, sc = op()
    for _ in range(2):
        c.view(torch.uint8).fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c.view(torch.uint8)[:end], eager_c.view(torch.uint8)[:end]) and torch.equal(c.view(torch.uint8)[:end], want_c[:end])
        assert torch.equal(sc.view(torch.uint8).reshape(-1)[:end * G], eager_s.view(torch.uint8).reshape(-1)[:end * G])
