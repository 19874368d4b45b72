"""The gate/up MXFP4 (W4A4) grouped GEMM with fused activation, rotation and MXFP4 output (grouped_matmul_mxf4_silu_mxf4_tn / ..._swiglu_oai_mxf4_tn) on the MI355X:
its bytes against the two launches it replaces -- grouped_matmul_mxf4_bf16_tn, then fusedSiluMulQuantizeMx / fusedSwigluOaiQuantizeMx with the same h and method --
and once against fp64 mathematics.

All byte comparisons run in the regime where the GEMM's fp32 sums are exact in any order (the chain's GEMM sums K in another order than this kernel): e2m1 codes
uniform over all 16 values, scale bytes of both operands in {126, 127, 128}, K <= 4096 -- every product is a multiple of 2^-4 below 2^8, every partial sum below 2^20."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _benchlib as lab  # noqa: E402  (the LAB build: forced forms)
import _rotations as R  # noqa: E402
import qutlass_amd as q  # noqa: E402

DEV, E8M0 = "cuda:0", torch.float8_e8m0fnu
COUNTS, TRAIL, INTER = (1, 0, 37, 70), 4, 64   # an empty group, a partial m-tile, a group that crosses a 64-row tile; two column tiles, the up rows start at I
ACT_ALPHA, LIMIT, SENTINEL = 1.702, 7.0, 0xA5
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])

_offs = lambda counts: torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)   # noqa: E731


def _k_of(form, which):
    """128: a half-stage tail; 1280: five stages over four waves; the largest K the form runs in one shot and the smallest on its ring, from the kernel's own ladder"""
    if isinstance(which, int):
        return which
    out = (ctypes.c_int64 * 3)()
    plan = q._lib.load().qutlass_amd_debug_grouped_mxf4_act_plan
    plan.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
    assert plan(64, 128, 256, 1, out) in (616, 617)
    return int(out[form - 615]) + (128 if which == "ring" else 0)


def _operands(E, inter, K, M, seed, sf=(126, 129)):
    """device operands from a seeded generator; alpha per expert, no power of two, sized so that gate values spread over about +-8 (a sum of K products of variance
    ~224 at the default scale bytes): the activation's curved range and the clamp at 7 are both met"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randint(0, 256, (M, K // 2), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (E, 2 * inter, K // 2), generator=g, dtype=torch.uint8)
    asf = torch.randint(*sf, (M, K // 32), generator=g, dtype=torch.uint8)
    bsf = torch.randint(*sf, (E, 2 * inter, K // 32), generator=g, dtype=torch.uint8)
    bias = (torch.randn(E, 2 * inter, generator=g) * 2).to(torch.bfloat16)
    alpha = torch.tensor([0.17, 0.23, 0.21, 0.19][:E]) / (K ** 0.5)
    return (a.to(DEV), b.to(DEV), asf.reshape(-1).to(DEV).view(E8M0), bsf.reshape(-1).to(DEV).view(E8M0)), alpha.to(DEV), bias.to(DEV)


def _chain(act, method, ops, alpha, offs, h, bias):
    """the two launches: (gate/up bf16, codes (M, I/2) uint8, flat scale bytes)"""
    y = q.grouped_matmul_mxf4_bf16_tn(*ops, alpha, offs)
    if act == "silu":
        c, s = q.fusedSiluMulQuantizeMx(y, h, method=method)
    else:
        c, s = q.fusedSwigluOaiQuantizeMx(y, h, method=method, alpha=ACT_ALPHA, limit=LIMIT, bias=bias, offs=offs if bias is not None else None)
    return y, c.view(torch.uint8), s.view(torch.uint8).reshape(-1)


@functools.lru_cache(maxsize=None)
def _problem(K, act, method):
    """operands of one K and the chain's bytes on them: computed once, shared by the forms"""
    ops, alpha, bias = _operands(len(COUNTS), INTER, K, sum(COUNTS) + TRAIL, seed=K)
    h = R.signed_permuted_hadamard(32, seed=1).to(DEV)
    offs = _offs(COUNTS)
    y, codes, scales = _chain(act, method, ops, alpha, offs, h, bias if act == "oai_bias" else None)
    return ops, bias, alpha, offs, h, y, codes, scales


@pytest.mark.parametrize("method", ("quest", "abs_max"))
@pytest.mark.parametrize("act", ("silu", "oai_bias"))
@pytest.mark.parametrize("which", (128, 256, 1280, "one_shot", "ring"))
@pytest.mark.parametrize("form", (616, 617))
def test_bytes_equal_the_chain(form, which, act, method):
    K = _k_of(form, which)
    assert K <= 4096, "the exact-sum regime of this file"
    ops, bias, alpha, offs, h, y, want_c, want_s = _problem(K, act, method)
    gate = y[:sum(COUNTS), :INTER].float()
    assert float(gate.min()) < -4 and float(gate.max()) > LIMIT, "the operands do not reach the activation's curved range and its clamp"
    E, end, M, G = len(COUNTS), sum(COUNTS), sum(COUNTS) + TRAIL, INTER // 32
    codes = torch.full((M, INTER // 2), SENTINEL, dtype=torch.uint8, device=DEV)
    scales = torch.full((M * G,), SENTINEL, dtype=torch.uint8, device=DEV)
    f = lab.load().qutlass_amd_grouped_matmul_mxf4_act_mxf4_tn
    f.argtypes = ([ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2
                  + [ctypes.c_void_p] * 2 + [ctypes.c_int64] * 4 + [ctypes.c_void_p])
    with lab.forced(gemm_variant=form):
        rc = f(*(t.data_ptr() for t in ops), alpha.data_ptr(), alpha.numel(), offs.data_ptr(), 0 if act == "silu" else 1, ACT_ALPHA, LIMIT,
               bias.data_ptr() if act == "oai_bias" else None, h.data_ptr(), 32, 0 if method == "quest" else 1, codes.data_ptr(), scales.data_ptr(), M, 2 * INTER, K, E,
               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lab.load().qutlass_amd_last_error().decode()
    torch.cuda.synchronize()
    bad = (scales[:end * G] != want_s[:end * G]).nonzero()
    assert bad.numel() == 0, f"{bad.size(0)} scale bytes differ, first at (row, group) {divmod(int(bad[0]), G)}"
    bad = (codes[:end] != want_c[:end]).nonzero()
    assert bad.numel() == 0, f"{bad.size(0)} code bytes differ, first at (row, byte) {bad[0].tolist()}"
    assert bool((codes[end:] == SENTINEL).all()) and bool((scales[end * G:] == SENTINEL).all()), "rows at or past offs[E-1] were written"


def test_product_rule_and_shared_alpha():
    M, K, inter = 70, 640, 64
    ops, _, _ = _operands(1, inter, K, M, seed=3)
    alpha, offs, h = torch.full((1,), 0.2 / K ** 0.5, device=DEV), _offs([M]), torch.eye(32, dtype=torch.bfloat16, device=DEV)
    _, want_c, want_s = _chain("oai", "quest", ops, alpha, offs, h, None)
    c, s = q.grouped_matmul_mxf4_swiglu_oai_mxf4_tn(*ops, alpha, offs, h, act_alpha=ACT_ALPHA, limit=LIMIT)
    assert c.dtype == torch.uint8 and tuple(c.shape) == (M, inter // 2) and s.dtype == E8M0 and tuple(s.shape) == (128, 4)
    G = inter // 32
    assert torch.equal(c, want_c) and torch.equal(s.view(torch.uint8).reshape(-1)[:M * G], want_s[:M * G])


def test_against_fp64():
    """Scale bytes 120 ... 134: the GEMM's sums are no longer exact and the two may break a bf16 tie differently.  Measured on an MI355X: the op 0.103744, the two launches 0.103744."""
    E, inter, K, counts = 2, 64, 512, (16, 48)
    M, G = sum(counts), inter // 32
    ops, _, _ = _operands(E, inter, K, M, seed=17, sf=(120, 135))
    alpha, offs, h = torch.tensor([1.1e-5, 0.9e-5], device=DEV), _offs(counts), R.signed_permuted_hadamard(32, seed=2).to(DEV)

    def values(codes, sf, k):   # packed e2m1 (rows, k / 2) with e8m0 (rows, k / 32) -> fp64 (rows, k)
        c = codes.cpu().numpy()
        v = np.stack([E2M1[c & 15], E2M1[c >> 4]], axis=-1).reshape(c.shape[0], k)
        return v * np.repeat(np.exp2(sf.view(torch.uint8).cpu().numpy().reshape(c.shape[0], k // 32).astype(np.float64) - 127), 32, axis=1)

    a = values(ops[0], ops[2], K)
    w = values(ops[1].reshape(E * 2 * inter, K // 2), ops[3], K).reshape(E, 2 * inter, K)
    grp = np.repeat(np.arange(E), counts)
    x = np.einsum("mk,mnk->mn", a, w[grp]) * alpha.double().cpu().numpy()[grp][:, None]
    act = x[:, :inter] / (1.0 + np.exp(-x[:, :inter])) * x[:, inter:]
    ref = (act.reshape(M, G, 32) @ h.double().cpu().numpy()).reshape(M, inter)   # real arithmetic, nothing rounded after the operands

    def err(c, s):
        got = values(c.view(torch.uint8), s.view(torch.uint8).reshape(-1)[:M * G], inter)
        return np.linalg.norm(got - ref) / np.linalg.norm(ref)

    _, cc, cs = _chain("silu", "quest", ops, alpha, offs, h, None)
    e_chain, e_op = err(cc, cs), err(*q.grouped_matmul_mxf4_silu_mxf4_tn(*ops, alpha, offs, h))
    print(f"relative Frobenius error against fp64: op {e_op:.6f}, the two launches {e_chain:.6f}")
    assert e_op <= 1.01 * e_chain, (e_op, e_chain)


def test_graph_capture():
    ops, bias, alpha, offs, h, _, _, _ = _problem(1280, "oai_bias", "quest")
    G, offs = INTER // 32, offs.clone()
    op = lambda: q.grouped_matmul_mxf4_swiglu_oai_mxf4_tn(*ops, alpha, offs, h, act_alpha=ACT_ALPHA, limit=LIMIT, bias=bias)   # noqa: E731
    eager = []
    for counts in (COUNTS, (20, 30, 10, 40)):
        offs.copy_(_offs(counts))
        eager.append((sum(counts),) + tuple(t.view(torch.uint8).clone() for t in op()))   # (the first call is also the warm-up off the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c, sc = op()
    for counts, (end, want_c, want_s) in zip((COUNTS, (20, 30, 10, 40)), eager):
        offs.copy_(_offs(counts))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c[:end], want_c[:end]) and torch.equal(sc.view(torch.uint8).reshape(-1)[:end * G], want_s.reshape(-1)[:end * G])
