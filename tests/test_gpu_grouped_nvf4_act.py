"""The gate/up NVFP4 (W4A4) grouped GEMM with fused activation, rotation and NVFP4 output (grouped_matmul_nvf4_silu_nvf4_tn / ..._swiglu_oai_nvf4_tn) on the MI355X: its
bytes against the launches it replaces -- grouped_matmul_nvf4_bf16_tn, then fusedSiluMulQuantizeNvGrouped, or swiglu_oai_and_mul and fusedGatherQuantizeNvGrouped --
and once against fp64 mathematics.

The byte comparisons of the forced forms use GENERIC operands (inexact fp32 sums): forms 624 / 625 share the MFMA order of the chain GEMM's forms 600 / 601.
exact_operands() needs no GPU: tests/test_grouped_nvf4_act_cpu.py asserts its sums exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _benchlib as lab  # noqa: E402  (the LAB build: forced forms)
import _rotations as R  # noqa: E402
import qutlass_amd as q  # noqa: E402

DEV, E4M3 = "cuda:0", torch.float8_e4m3fn
COUNTS = {624: (1, 0, 37, 70), 625: (1, 0, 37, 150)}   # an empty group, a partial tile, a group that crosses a tile of 64 / 128 rows
TRAIL, INTER = 4, 128                                  # rows past offs[E-1]; four / two column tiles, the up rows start at I
ACT_ALPHA, LIMIT, SENTINEL = 1.702, 7.0, 0xA5
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])
GEMM_ARGS = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p]
ACT_ARGS = GEMM_ARGS + [ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + \
    [ctypes.c_void_p] * 2 + [ctypes.c_int64] * 4 + [ctypes.c_void_p]

_offs = lambda counts: torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)   # noqa: E731
_flat = lambda s: s.view(torch.uint8).reshape(-1)   # noqa: E731


def _ring_k():
    """the smallest K that fills the K loop's ring once, from the kernel's own constants"""
    out = (ctypes.c_int64 * 2)()
    plan = q._lib.load().qutlass_amd_debug_grouped_nvf4_act_plan
    plan.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
    assert plan(64, 128, 256, 1, out) == 625
    return int(out[1])


def _operands(counts, inter, K, seed):
    """device operands from a seeded generator: random codes, e4m3 scale bytes over three binades with every mantissa (0.5 ... 3.75), a per-expert alpha that is no power
    of two and puts the gates' standard deviation near 3 (a product's is 8.56 x 3.76), distinct global scales"""
    E, M = len(counts), sum(counts) + TRAIL
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randint(0, 256, (M, K // 2), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (E, 2 * inter, K // 2), generator=g, dtype=torch.uint8)
    asf = torch.randint(0x30, 0x48, (M * K // 16,), generator=g, dtype=torch.uint8)
    bsf = torch.randint(0x30, 0x48, (E * 2 * inter * K // 16,), generator=g, dtype=torch.uint8)
    bias = (torch.randn(E, 2 * inter, generator=g) * 2).to(torch.bfloat16)
    alpha = torch.tensor([1.0, 1.1, 0.9, 1.05][:E]) * 3.0 / (32.2 * K ** 0.5)
    gs = torch.tensor([0.9, 1.3, 0.7, 1.1][:E])
    return (a.to(DEV), b.to(DEV), asf.to(DEV).view(E4M3), bsf.to(DEV).view(E4M3)), alpha.to(DEV), bias.to(DEV), gs.to(DEV)


def _quantize(y, act, method, offs, h, bias, gs):
    """the chain behind its GEMM: (codes (M, I/2) uint8, flat scale bytes)"""
    if act == "silu":
        c, s = q.fusedSiluMulQuantizeNvGrouped(y, h, gs, offs, method=method)
    else:
        x = q.swiglu_oai_and_mul(y, alpha=ACT_ALPHA, limit=LIMIT, bias=bias, offs=offs if bias is not None else None)
        c, s = q.fusedGatherQuantizeNvGrouped(x, h, gs, torch.arange(y.size(0), dtype=torch.int32, device=DEV), offs, method=method)
    return c.view(torch.uint8), _flat(s)


@functools.lru_cache(maxsize=None)
def _problem(form, K):
    """operands of one form and K and the chain GEMM's output on them, that GEMM forced to the form this op mirrors: computed once"""
    counts = COUNTS[form]
    ops, alpha, bias, gs = _operands(counts, INTER, K, seed=K + form)
    offs, M, E = _offs(counts), sum(counts) + TRAIL, len(counts)
    y = torch.zeros(M, 2 * INTER, dtype=torch.bfloat16, device=DEV)
    f = lab.load().qutlass_amd_grouped_matmul_nvf4_bf16_tn
    f.argtypes = GEMM_ARGS + [ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    with lab.forced(gemm_variant=form - 24):
        rc = f(*(t.data_ptr() for t in ops), alpha.data_ptr(), E, offs.data_ptr(), y.data_ptr(), M, 2 * INTER, K, E, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lab.load().qutlass_amd_last_error().decode()
    gate = y[:sum(counts), :INTER].float()
    assert float(gate.min()) < -4 and float(gate.max()) > LIMIT, "the operands do not reach the activation's curved range and its clamp"
    return ops, alpha, bias, gs, offs, R.signed_permuted_hadamard(32, seed=1).to(DEV), y


@pytest.mark.parametrize("which", (128, "ring", "ring+128"))   # one stage; the ring filled once; one stage past it, with a wrap
@pytest.mark.parametrize("form", (624, 625))
def test_bytes_equal_the_chain(form, which):
    """every activation {silu, swiglu_oai with bias} x method {quest, abs_max} of a form and K, on the one chain GEMM output of that form and K"""
    K = which if isinstance(which, int) else _ring_k() + (128 if which == "ring+128" else 0)
    ops, alpha, bias, gs, offs, h, y = _problem(form, K)
    counts = COUNTS[form]
    E, end, M = len(counts), sum(counts), sum(counts) + TRAIL
    f = lab.load().qutlass_amd_grouped_matmul_nvf4_act_nvf4_tn
    f.argtypes = ACT_ARGS
    for act in ("silu", "oai_bias"):
        for method in ("quest", "abs_max"):
            want_c, want_s = _quantize(y, act, method, offs, h, bias if act == "oai_bias" else None, gs)
            codes = torch.full((M, INTER // 2), SENTINEL, dtype=torch.uint8, device=DEV)
            scales = torch.full((M * INTER // 16,), SENTINEL, dtype=torch.uint8, device=DEV)
            with lab.forced(gemm_variant=form):
                rc = f(*(t.data_ptr() for t in ops), alpha.data_ptr(), E, offs.data_ptr(), 0 if act == "silu" else 1, ACT_ALPHA, LIMIT,
                       bias.data_ptr() if act == "oai_bias" else None, h.data_ptr(), 32, gs.data_ptr(), q._METHOD_CODE[method], codes.data_ptr(), scales.data_ptr(),
                       M, 2 * INTER, K, E, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lab.load().qutlass_amd_last_error().decode()
            torch.cuda.synchronize()
            bad = (scales[:end * INTER // 16] != want_s[:end * INTER // 16]).nonzero()
            assert bad.numel() == 0, f"{act} {method}: {bad.size(0)} scale bytes differ, first at group {bad[0].item()}"
            bad = (codes[:end] != want_c[:end]).nonzero()
            assert bad.numel() == 0, f"{act} {method}: {bad.size(0)} code bytes differ, first at (row, byte) {bad[0].tolist()}"
            assert bool((codes[end:] == SENTINEL).all()) and bool((scales[end * INTER // 16:] == SENTINEL).all()), f"{act} {method}: rows at or past offs[E-1] were written"


def exact_operands(counts, inter=64, K=256, seed=3):
    """CPU tensors in the exact-sum regime: scale bytes 0x30 / 0x38 / 0x40 (0.5, 1, 2), so every product is a multiple of 2^-4 and a sum of K stays below 2^24 of them"""
    E, M = len(counts), sum(counts)
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randint(0, 256, (M, K // 2), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (E, 2 * inter, K // 2), generator=g, dtype=torch.uint8)
    asf = torch.randint(6, 9, (M * K // 16,), generator=g, dtype=torch.uint8) << 3
    bsf = torch.randint(6, 9, (E * 2 * inter * K // 16,), generator=g, dtype=torch.uint8) << 3
    return a, b, asf, bsf


def assert_exact(a, b, asf, bsf):
    K, sa, sb = 2 * a.size(1), asf.view(E4M3).float(), bsf.view(E4M3).float()
    assert bool(((sa.log2() % 1) == 0).all()) and bool(((sb.log2() % 1) == 0).all()), "a scale is no power of two"
    quantum = 0.25 * float(sa.min()) * float(sb.min())   # (the e2m1 grid is multiples of 0.5)
    assert K * 36.0 * float(sa.max()) * float(sb.max()) / quantum < 2 ** 24


@pytest.mark.parametrize("counts", ((20, 30), (60, 70)))   # at most 48 and more than 48 rows per expert: forms 624 / 625, the chain's GEMM on 600 / 601
def test_product_rule_and_python_ops(counts):
    inter, E, M = 64, len(counts), sum(counts)
    cpu = exact_operands(counts)
    assert_exact(*cpu)
    a, b, asf, bsf = (t.to(DEV) for t in cpu)
    ops, offs = (a, b, asf.view(E4M3), bsf.view(E4M3)), _offs(counts)
    alpha, gs = torch.tensor([0.013], device=DEV), torch.tensor([0.9, 1.3], device=DEV)
    h = torch.eye(32, dtype=torch.bfloat16, device=DEV) if M < 96 else R.signed_permuted_hadamard(32, seed=2).to(DEV)
    bias = (torch.randn(E, 2 * inter, generator=torch.Generator().manual_seed(1)) * 2).to(torch.bfloat16).to(DEV)
    y = q.grouped_matmul_nvf4_bf16_tn(*ops, alpha, offs)
    for method in ("quest", "abs_max"):
        for act, got in (("silu", q.grouped_matmul_nvf4_silu_nvf4_tn(*ops, alpha, offs, h, gs, method=method)),
                         ("oai", q.grouped_matmul_nvf4_swiglu_oai_nvf4_tn(*ops, alpha, offs, h, gs, method=method, act_alpha=ACT_ALPHA, limit=LIMIT, bias=bias))):
            want_c, want_s = _quantize(y, act, method, offs, h, bias if act == "oai" else None, gs)
            assert got[0].dtype == torch.uint8 and tuple(got[0].shape) == (M, inter // 2)
            assert got[1].dtype == E4M3 and tuple(got[1].shape) == q.utils.padded_scale_shape(M, inter, 16)
            assert torch.equal(_flat(got[1])[:M * inter // 16], want_s[:M * inter // 16]) and torch.equal(got[0], want_c), (act, method)


def test_graph_replay():
    counts, K = (5, 0, 40, 19), 256
    ops, alpha, bias, gs = _operands(counts, 64, K, seed=11)
    offs, h, end = _offs(counts), R.signed_permuted_hadamard(32, seed=3).to(DEV), sum(counts)
    run = lambda: q.grouped_matmul_nvf4_swiglu_oai_nvf4_tn(*ops, alpha, offs, h, gs, act_alpha=ACT_ALPHA, limit=LIMIT, bias=bias)   # noqa: E731
    eager = run()   # (also the warm-up off the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0][:end], eager[0][:end]) and torch.equal(_flat(out[1])[:end * 4], _flat(eager[1])[:end * 4])


def test_against_fp64_mathematics():
    """E = 2, I = 64, K = 512, counts (16, 48), silu, abs_max: relative Frobenius error of codes x scales / global scale against the dequantised operands multiplied, activated
    and rotated in fp64.  The bound is the error of the chain's launches on the same operands, measured here.  Measured on the MI355X: 0.100587 through the op, 0.100587
    through the chain's launches (equal bits)."""
    counts, inter, K = (16, 48), 64, 512
    ops, alpha, _, gs = _operands(counts, inter, K, seed=7)
    offs, h, M = _offs(counts), R.signed_permuted_hadamard(32, seed=4).to(DEV), sum(counts)
    a, b, asf, bsf = (t[:M].cpu() if i == 0 else t.cpu() for i, t in enumerate(ops))
    deq = lambda c, s: (torch.from_numpy(E2M1)[torch.stack((c & 15, c >> 4), -1).long()].reshape(*c.shape[:-1], -1, 16) * s.float().double().reshape(*c.shape[:-1], -1, 1)).flatten(-2)   # noqa: E731
    A, B = deq(a, asf[:M * K // 16]), deq(b, bsf)
    row_e = torch.repeat_interleave(torch.arange(2), torch.tensor(counts))
    yy = torch.einsum("mk,mnk->mn", A, B[row_e]) * alpha.cpu().double()[row_e, None]
    ref = ((yy[:, :inter] / (1 + torch.exp(-yy[:, :inter])) * yy[:, inter:]).reshape(M, -1, 32) @ h.cpu().double()).reshape(M, inter)

    def err(codes, scales):
        got = deq(codes[:M].cpu(), _flat(scales)[:M * inter // 16].cpu().view(E4M3)) / gs.cpu().double()[row_e, None]
        return float((got - ref).norm() / ref.norm())

    e_op = err(*q.grouped_matmul_nvf4_silu_nvf4_tn(*ops, alpha, offs, h, gs))
    e_chain = err(*q.fusedSiluMulQuantizeNvGrouped(q.grouped_matmul_nvf4_bf16_tn(*ops, alpha, offs), h, gs, offs))
    print(f"relative Frobenius error against fp64: op {e_op:.6f}, the chain's launches {e_chain:.6f}")
    assert e_op <= e_chain
