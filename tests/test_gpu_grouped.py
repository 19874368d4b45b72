"""Grouped MXFP4 GEMM for mixture-of-experts layers (qutlass_amd.grouped_matmul_mxf4_bf16_tn) on the MI355X: every group against the CPU oracle's dequantise-matmul
(bit-exact, the regime of tests/test_gpu_parity.py::_pipeline), against per-group matmul_ada_mxf4_bf16_tn, every form forced through the lab library, a stacked weight
above 2 GiB, per-expert alpha, rows past offs[-1] left untouched, graph capture with offsets rewritten between replays, and torch.compile."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)
import _benchlib as lab  # noqa: E402  (the LAB build: forced forms)

DEV = "cuda:0"
QWEN_UP, QWEN_DOWN = (128, 1536, 2048), (128, 2048, 768)          # Qwen3-30B-A3B (E, N, K)
MIXTRAL_UP, MIXTRAL_DOWN = (8, 28672, 4096), (8, 4096, 14336)     # Mixtral-8x7B
FORMS = (590, 591, 592, 593)                                       # 32x32, 32x16, 64x32 tiles of the wave-owned kernel; 64x64 ring kernel


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _hadamard(n):
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h * n ** -0.5).to(torch.bfloat16).to(DEV)


def _np(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint16).numpy() if t.dtype == torch.bfloat16 else t.view(torch.uint8).numpy() if t.element_size() == 1 else t.numpy()


def _counts(M, E, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        c = np.bincount(rng.integers(0, E, M), minlength=E)
    elif kind == "skewed":       # half of the rows in one expert
        c = np.bincount(rng.integers(0, E, M - M // 2), minlength=E)
        c[rng.integers(0, E)] += M // 2
    elif kind == "empty":        # an eighth of the experts get every row
        live = rng.choice(E, size=max(1, E // 8), replace=False)
        c = np.zeros(E, dtype=np.int64)
        c[live] = np.bincount(rng.integers(0, len(live), M), minlength=len(live))
    return c


class Moe:
    """Expert-sorted tokens and stacked expert weights, quantised on the GPU by fusedQuantizeMx (Hadamard 32); row-major scales as the op reads them."""

    def __init__(self, q, E, N, K, M, method="abs_max", seed=0):
        torch.manual_seed(seed)
        h = _hadamard(32)
        self.E, self.N, self.K, self.M = E, N, K, M
        self.x = torch.randn(M, K, dtype=torch.bfloat16, device=DEV) * 25.0
        self.aq, a_s = q.fusedQuantizeMx(self.x, h, method=method)
        self.asf = a_s.view(-1)[: M * K // 32]                         # the flat row-major (M, K/32) prefix
        wq, wsf = [], []
        for g in range(E):                                                 # (per expert: keeps the bf16 staging small)
            w = torch.randn(N, K, dtype=torch.bfloat16, device=DEV) * 25.0
            bq, b_s = q.fusedQuantizeMx(w, h, method=method)
            wq.append(bq)
            wsf.append(b_s.view(-1)[: N * K // 32])
            del w
        self.bq = torch.stack(wq)                                          # (E, N, K/2)
        self.bsf = torch.cat(wsf)                                          # (E * N * K/32)
        self.h, self.method = h, method

    def offs(self, counts):
        return torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)

    def bsf_of(self, g):
        n = self.N * self.K // 32
        return self.bsf[g * n:(g + 1) * n]


def _ada_groups(q, m, offs, alpha=None):
    """per-group matmul_ada_mxf4_bf16_tn (host offsets): the loop the grouped op replaces"""
    o = [0] + offs.cpu().tolist()
    kb = m.K // 32
    outs = {}
    for g in range(m.E):
        s, e = o[g], o[g + 1]
        if e <= s:
            continue
        al = alpha[g:g + 1] if alpha is not None and alpha.numel() > 1 else (alpha if alpha is not None else torch.ones(1, device=DEV))
        outs[g] = q.matmul_ada_mxf4_bf16_tn(m.aq[s:e], m.bq[g], m.asf[s * kb:e * kb], m.bsf_of(g), al)
    return outs


def _check_vs_ada(q, m, offs, out, alpha=None):
    o = [0] + offs.cpu().tolist()
    for g, ref in _ada_groups(q, m, offs, alpha).items():
        got = out[o[g]:o[g + 1]]
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), f"group {g}: {(got != ref).sum().item()} outputs differ from matmul_ada"


def _check_vs_oracle(m, offs, out, groups=None, ncols=256, nrows=48):
    """each checked group against oracle.gemm_blockscaled on oracle.to_blocked of that group's row-major scales (sampled rows / columns: CPU time)"""
    o = [0] + offs.cpu().tolist()
    kb = m.K // 32
    live = [g for g in range(m.E) if o[g + 1] > o[g]]
    if groups is None:
        sizes = {g: o[g + 1] - o[g] for g in live}
        groups = sorted({live[0], live[-1], max(live, key=sizes.get)} | set(live[:: max(1, len(live) // 4)]))
    cols = np.unique(np.r_[np.arange(min(ncols // 2, m.N)), np.arange(max(0, m.N - ncols // 2), m.N)])
    aq, asf, outn = _np(m.aq), _np(m.asf).reshape(m.M, kb), _np(out)
    for g in groups:
        s, e = o[g], o[g + 1]
        rows = np.arange(s, e) if e - s <= nrows else np.r_[np.arange(s, s + nrows // 2), np.arange(e - nrows // 2, e)]
        bq = _np(m.bq[g][torch.from_numpy(cols).to(DEV)])
        bsf = _np(m.bsf_of(g)).reshape(m.N, kb)[cols]
        ref = oracle.gemm_blockscaled(oracle.KIND_MXFP4, aq[rows], bq, oracle.to_blocked(asf[rows]), oracle.to_blocked(bsf), 1.0, len(rows), len(cols), m.K)
        got = outn[rows][:, cols]
        assert np.array_equal(got, ref), f"group {g}: {(got != ref).sum()} of {got.size} sampled outputs differ from the oracle"


def _lab_grouped(m, offs, alpha, D):
    lib = lab.load()
    f = lib.qutlass_amd_grouped_matmul_mxf4_bf16_tn
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    rc = f(m.aq.data_ptr(), m.bq.data_ptr(), m.asf.data_ptr(), m.bsf.data_ptr(), alpha.data_ptr(), alpha.numel(), offs.data_ptr(), D.data_ptr(),
           m.M, m.N, m.K, m.E, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.qutlass_amd_last_error().decode()
    return D


@pytest.mark.parametrize("shape,M,kind,method", [
    (QWEN_UP, 512, "uniform", "abs_max"),      # decode: batch 64 x top-8
    (QWEN_UP, 512, "skewed", "quest"),
    (QWEN_DOWN, 512, "empty", "abs_max"),
    (QWEN_DOWN, 4096, "uniform", "quest"),     # mean 32 rows per expert
    (MIXTRAL_UP, 128, "uniform", "abs_max"),   # decode: batch 64 x top-2
    (MIXTRAL_UP, 1024, "skewed", "abs_max"),   # prefill-like: the 64x64 ring form
    (MIXTRAL_DOWN, 128, "empty", "quest"),
])
def test_grouped_vs_oracle_and_ada(q, shape, M, kind, method):
    E, N, K = shape
    m = Moe(q, E, N, K, M, method)
    offs = m.offs(_counts(M, E, kind, seed=M + E))
    alpha = torch.ones(1, device=DEV)
    out = q.grouped_matmul_mxf4_bf16_tn(m.aq, m.bq, m.asf, m.bsf, alpha, offs)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    _check_vs_ada(q, m, offs, out)
    _check_vs_oracle(m, offs, out)


def test_e1_and_activation_path(q):
    """E = 1 is matmul_ada_mxf4_bf16_tn; one fusedQuantizeMx over the sorted tokens + the grouped op == per-group quantise + matmul_ada"""
    E, N, K = MIXTRAL_DOWN
    m = Moe(q, 1, N, K, 200)
    offs = m.offs([200])
    one = torch.ones(1, device=DEV)
    out = q.grouped_matmul_mxf4_bf16_tn(m.aq, m.bq, m.asf, m.bsf, one, offs)
    ref = q.matmul_ada_mxf4_bf16_tn(m.aq, m.bq[0], m.asf, m.bsf, one)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    _check_vs_oracle(m, offs, out, groups=[0])

    E, N, K = QWEN_UP
    m = Moe(q, E, N, K, 512, "quest", seed=5)
    offs = m.offs(_counts(512, E, "uniform", 9))
    out = q.grouped_matmul_mxf4_bf16_tn(m.aq, m.bq, m.asf, m.bsf, one, offs)
    o = [0] + offs.cpu().tolist()
    for g in range(E):
        s, e = o[g], o[g + 1]
        if e > s:
            xq, xs = q.fusedQuantizeMx(m.x[s:e], m.h, method="quest")   # this group's tokens quantised on their own
            ref = q.matmul_ada_mxf4_bf16_tn(xq, m.bq[g], xs, m.bsf_of(g), one)
            assert torch.equal(out[s:e].view(torch.int16), ref.view(torch.int16)), g


def test_per_expert_alpha(q):
    E, N, K = QWEN_DOWN
    m = Moe(q, E, N, K, 1024, seed=2)
    offs = m.offs(_counts(1024, E, "uniform", 4))
    one = torch.ones(1, device=DEV)
    alpha = torch.tensor([2.0 ** ((g % 7) - 3) for g in range(E)], device=DEV)
    base = q.grouped_matmul_mxf4_bf16_tn(m.aq, m.bq, m.asf, m.bsf, one, offs)
    out = q.grouped_matmul_mxf4_bf16_tn(m.aq, m.bq, m.asf, m.bsf, alpha, offs)
    o = [0] + offs.cpu().tolist()
    for g in range(E):
        s, e = o[g], o[g + 1]
        assert torch.equal(out[s:e].float(), base[s:e].float() * alpha[g]), g
    _check_vs_ada(q, m, offs, out, alpha)


def test_rows_past_the_last_offset_are_untouched(q):
    """offs[-1] < M through the C entry into a sentinel-filled D: the rows past the end keep the sentinel"""
    from qutlass_amd import _lib

    E, N, K = QWEN_DOWN
    M = 600
    m = Moe(q, E, N, K, M, seed=3)
    offs = torch.tensor(np.minimum(np.cumsum(_counts(M, E, "uniform", 8)), 451), dtype=torch.int32, device=DEV)
    assert offs[-1].item() == 451
    D = torch.full((M, N), -12345, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    one = torch.ones(1, device=DEV)
    rc = _lib.load().qutlass_amd_grouped_matmul_mxf4_bf16_tn(m.aq.data_ptr(), m.bq.data_ptr(), m.asf.data_ptr(), m.bsf.data_ptr(), one.data_ptr(), 1, offs.data_ptr(),
                                                            D.data_ptr(), M, N, K, E, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.load().qutlass_amd_last_error().decode()
    torch.cuda.synchronize()
    assert (D[451:].view(torch.int16) == -12345).all()
    _check_vs_ada(q, m, offs, D)
    _check_vs_oracle(m, offs, D)


@pytest.mark.parametrize("shape,M", [((16, 512, 2048), 700), ((8, 256, 7168), 900), ((4, 256, 14336), 300)])
def test_every_form_through_the_lab_library(q, shape, M):
    """590 / 591 / 592 / 593 forced: one-shot K (2048) and ring K (7168, 14336) -- each bit-equal to the product library and to the oracle"""
    E, N, K = shape
    m = Moe(q, E, N, K, M, seed=K)
    offs = m.offs(_counts(M, E, "skewed", K))
    one = torch.ones(1, device=DEV)
    prod = q.grouped_matmul_mxf4_bf16_tn(m.aq, m.bq, m.asf, m.bsf, one, offs)
    _check_vs_oracle(m, offs, prod, groups=list(range(E)), nrows=32)
    for v in FORMS:
        with lab.forced(gemm_variant=v):
            out = _lab_grouped(m, offs, one, torch.empty(M, N, dtype=torch.bfloat16, device=DEV))
        assert torch.equal(out.view(torch.int16), prod.view(torch.int16)), (v, (out != prod).sum().item())


def test_stacked_weight_above_2gib(q):
    """DeepSeek-V3 gate/up (E = 256, N = 4096, K = 7168: 3.76 GB of e2m1): random codes, every scale byte 127 -- products are multiples of 1/4 below 36,
    so every fp32 partial sum is exact for any K <= 16384"""
    E, N, K, M = 256, 4096, 7168, 512
    g = torch.Generator(device=DEV).manual_seed(11)
    m = Moe.__new__(Moe)
    m.E, m.N, m.K, m.M = E, N, K, M
    m.aq = torch.randint(0, 256, (M, K // 2), dtype=torch.uint8, device=DEV, generator=g)
    m.bq = torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=DEV, generator=g)
    assert m.bq.numel() > 2 ** 31
    m.asf = torch.full((M * K // 32,), 127, dtype=torch.uint8, device=DEV).view(torch.float8_e8m0fnu)
    m.bsf = torch.full((E * N * K // 32,), 127, dtype=torch.uint8, device=DEV).view(torch.float8_e8m0fnu)
    offs = m.offs(np.full(E, M // E))                 # decode: two rows per expert, the first and the last expert included
    one = torch.ones(1, device=DEV)
    out = q.grouped_matmul_mxf4_bf16_tn(m.aq, m.bq, m.asf, m.bsf, one, offs)
    _check_vs_ada(q, m, offs, out)
    _check_vs_oracle(m, offs, out, groups=[0, E - 1], ncols=128)
    del m.bq
    torch.cuda.empty_cache()


def test_graph_capture_and_compile(q):
    """one capture, offsets rewritten in place between replays: each replay equals a fresh eager call; torch.compile (inductor) equals eager"""
    E, N, K = QWEN_UP
    M = 512
    m = Moe(q, E, N, K, M, seed=7)
    offs = m.offs(_counts(M, E, "uniform", 0))
    one = torch.ones(1, device=DEV)
    op = lambda: q.grouped_matmul_mxf4_bf16_tn(m.aq, m.bq, m.asf, m.bsf, one, offs)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op()                       # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = op()
    for kind, seed in (("uniform", 1), ("skewed", 2), ("empty", 3)):
        offs.copy_(m.offs(_counts(M, E, kind, seed)))
        graph.replay()
        torch.cuda.synchronize()
        end = offs[-1].item()
        eager = op()
        assert torch.equal(static_out[:end].view(torch.int16), eager[:end].view(torch.int16)), kind

    def layer(a, b, a_sf, b_sf, alpha, offs):
        return q.grouped_matmul_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs)

    torch._dynamo.reset()
    compiled = torch.compile(layer, backend="inductor", fullgraph=True)
    got = compiled(m.aq, m.bq, m.asf, m.bsf, one, offs)
    assert torch.equal(got.view(torch.int16), op().view(torch.int16))
