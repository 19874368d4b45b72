"""Grouped MXFP8 GEMM for mixture-of-experts layers (qutlass_amd.grouped_matmul_mxf8_bf16_tn) on the MI355X: exact-regime operands bit-equal to the CPU oracle
(on oracle.to_blocked of each group's row-major scales) and to the dense matmul_mxf8_bf16_tn per group, e4m3 and e5m2 A; quantised Gaussians within the MXFP8
tolerance; every form forced through the lab library; per-expert alpha, rows past offs[-1] left untouched, E = 1, a stacked weight above 2 GiB, graph capture with
offsets rewritten between replays, and torch.compile."""
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
FORMS = (594, 595, 596, 597)                                       # 32x32, 32x16, 64x32 tiles of the wave-owned kernel; 64x64 ring kernel
E4, E5, E8M0 = torch.float8_e4m3fn, torch.float8_e5m2, torch.float8_e8m0fnu
# the exact regime (tests/test_gpu_round6.py): every product and partial sum is exact in fp32, so any K order gives the same bits
EXACT_VALS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0], np.float32)


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


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


def _codes(dtype):
    return torch.from_numpy(EXACT_VALS).to(dtype).view(torch.uint8).to(DEV)


class Moe8:
    """Expert-sorted fp8 tokens (M, K) and stacked e4m3 expert weights (E, N, K) with row-major e8m0 scales, as the op reads them.
    exact: codes from EXACT_VALS and scale bytes 125 ... 129; otherwise quantised Gaussians (oracle.pseudoquant_mxfp8)."""

    def __init__(self, E, N, K, M, a5=False, exact=True, seed=0):
        self.E, self.N, self.K, self.M, self.a5 = E, N, K, M, a5
        kb = K // 32
        if exact:
            g = torch.Generator(device=DEV).manual_seed(seed)
            ta, tb = _codes(E5 if a5 else E4), _codes(E4)
            self.a = ta[torch.randint(0, len(EXACT_VALS), (M, K), device=DEV, generator=g)].view(E5 if a5 else E4)
            self.b = torch.empty(E, N, K, dtype=torch.uint8, device=DEV)
            for e in range(E):                                            # (per expert: keeps the index tensor small)
                self.b[e] = tb[torch.randint(0, len(EXACT_VALS), (N, K), device=DEV, generator=g)]
            self.b = self.b.view(E4)
            self.asf = torch.randint(125, 130, (M * kb,), dtype=torch.uint8, device=DEV, generator=g).view(E8M0)
            self.bsf = torch.randint(125, 130, (E * N * kb,), dtype=torch.uint8, device=DEV, generator=g).view(E8M0)
        else:
            assert not a5
            torch.manual_seed(seed)
            aq, asf = oracle.pseudoquant_mxfp8(_np(torch.randn(M, K, dtype=torch.bfloat16) * 25.0))
            bq, bsf = oracle.pseudoquant_mxfp8(_np(torch.randn(E * N, K, dtype=torch.bfloat16) * 25.0))
            self.a = torch.from_numpy(aq).to(DEV).view(E4)
            self.b = torch.from_numpy(bq).to(DEV).view(E, N, K).view(E4)
            self.asf = torch.from_numpy(asf.reshape(-1)).to(DEV).view(E8M0)
            self.bsf = torch.from_numpy(bsf.reshape(-1)).to(DEV).view(E8M0)

    def offs(self, counts):
        return torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)

    def bsf_of(self, g):
        n = self.N * self.K // 32
        return self.bsf[g * n:(g + 1) * n]


def _dense_groups(q, m, offs, alpha=None):
    """per-group matmul_mxf8_bf16_tn with to_blocked scales (host offsets): the loop the grouped op replaces"""
    from qutlass_amd.utils import to_blocked

    o = [0] + offs.cpu().tolist()
    kb = m.K // 32
    outs = {}
    for g in range(m.E):
        s, e = o[g], o[g + 1]
        if e <= s:
            continue
        al = alpha[g:g + 1] if alpha is not None and alpha.numel() > 1 else (alpha if alpha is not None else torch.ones(1, device=DEV))
        outs[g] = q.matmul_mxf8_bf16_tn(m.a[s:e], m.b[g], to_blocked(m.asf[s * kb:e * kb].view(e - s, kb)), to_blocked(m.bsf_of(g).view(m.N, kb)), al)
    return outs


def _check_vs_dense(q, m, offs, out, alpha=None):
    o = [0] + offs.cpu().tolist()
    for g, ref in _dense_groups(q, m, offs, alpha).items():
        got = out[o[g]:o[g + 1]]
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), f"group {g}: {(got != ref).sum().item()} outputs differ from matmul_mxf8_bf16_tn"


def _mxfp8_close(got_bits, want_bits):
    got = oracle.bf16_bits_to_f32(got_bits).astype(np.float64)
    want = oracle.bf16_bits_to_f32(want_bits).astype(np.float64)
    tol = np.abs(want) / 128.0 + 2e-5 * np.abs(want).max()
    return np.abs(got - want) <= tol


def _check_vs_oracle(m, offs, out, groups=None, ncols=256, nrows=48, exact=True):
    """each checked group against oracle.gemm_blockscaled on oracle.to_blocked of that group's row-major scales (sampled rows / columns: CPU time)"""
    o = [0] + offs.cpu().tolist()
    kb = m.K // 32
    live = [g for g in range(m.E) if o[g + 1] > o[g]]
    if groups is None:
        sizes = {g: o[g + 1] - o[g] for g in live}
        groups = sorted({live[0], live[-1], max(live, key=sizes.get)} | set(live[:: max(1, len(live) // 4)]))
    cols = np.unique(np.r_[np.arange(min(ncols // 2, m.N)), np.arange(max(0, m.N - ncols // 2), m.N)])
    aq, asf, outn = _np(m.a), _np(m.asf).reshape(m.M, kb), _np(out)
    kind = oracle.KIND_MXFP8_TN_A5 if m.a5 else oracle.KIND_MXFP8_TN
    for g in groups:
        s, e = o[g], o[g + 1]
        rows = np.arange(s, e) if e - s <= nrows else np.r_[np.arange(s, s + nrows // 2), np.arange(e - nrows // 2, e)]
        bq = _np(m.b[g][torch.from_numpy(cols).to(DEV)])
        bsf = _np(m.bsf_of(g)).reshape(m.N, kb)[cols]
        ref = oracle.gemm_blockscaled(kind, aq[rows], bq, oracle.to_blocked(asf[rows]), oracle.to_blocked(bsf), 1.0, len(rows), len(cols), m.K)
        got = outn[rows][:, cols]
        if exact:
            assert np.array_equal(got, ref), f"group {g}: {(got != ref).sum()} of {got.size} sampled outputs differ from the oracle"
        else:
            assert _mxfp8_close(got, ref).all(), f"group {g}: {(~_mxfp8_close(got, ref)).sum()} sampled outputs outside the MXFP8 tolerance"


def _entry(lib):
    f = lib.qutlass_amd_grouped_matmul_mxf8_bf16_tn
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_int, ctypes.c_void_p]
    return f


def _call(lib, m, offs, alpha, D):
    rc = _entry(lib)(m.a.data_ptr(), m.b.data_ptr(), m.asf.data_ptr(), m.bsf.data_ptr(), alpha.data_ptr(), alpha.numel(), offs.data_ptr(), D.data_ptr(),
                     m.M, m.N, m.K, m.E, 1 if m.a5 else 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.qutlass_amd_last_error().decode()
    return D


@pytest.mark.parametrize("shape,M,kind,a5", [
    (QWEN_UP, 512, "uniform", False),      # decode: batch 64 x top-8
    (QWEN_UP, 512, "skewed", True),
    (QWEN_DOWN, 512, "empty", False),
    (QWEN_DOWN, 4096, "uniform", True),    # mean 32 rows per expert
    (MIXTRAL_UP, 128, "uniform", False),   # decode: batch 64 x top-2
    (MIXTRAL_UP, 1024, "skewed", True),    # prefill-like: the 64x64 ring form
    (MIXTRAL_DOWN, 128, "empty", False),
    (MIXTRAL_DOWN, 1024, "uniform", True),
])
def test_grouped_exact_vs_oracle_and_dense(q, shape, M, kind, a5):
    E, N, K = shape
    m = Moe8(E, N, K, M, a5=a5, seed=M + E)
    offs = m.offs(_counts(M, E, kind, seed=M + E))
    alpha = torch.ones(1, device=DEV)
    out = q.grouped_matmul_mxf8_bf16_tn(m.a, m.b, m.asf, m.bsf, alpha, offs)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    _check_vs_dense(q, m, offs, out)
    _check_vs_oracle(m, offs, out)


@pytest.mark.parametrize("shape,M,kind", [((16, 512, 2048), 700, "skewed"), ((8, 1024, 4096), 300, "uniform"), ((32, 256, 768), 96, "empty")])
def test_grouped_on_quantised_gaussians(q, shape, M, kind):
    E, N, K = shape
    m = Moe8(E, N, K, M, exact=False, seed=K + M)
    offs = m.offs(_counts(M, E, kind, seed=M))
    out = q.grouped_matmul_mxf8_bf16_tn(m.a, m.b, m.asf, m.bsf, torch.ones(1, device=DEV), offs)
    _check_vs_oracle(m, offs, out, exact=False)


@pytest.mark.parametrize("a5", [False, True])
@pytest.mark.parametrize("shape,M", [((16, 512, 1024), 700), ((16, 512, 2048), 700), ((8, 256, 7168), 900), ((4, 256, 14336), 300)])
def test_every_form_through_the_lab_library(q, shape, M, a5):
    """594 / 595 / 596 / 597 forced: one-shot K (1024, 2048 for the 32-row tiles) and ring K (7168, 14336) -- each bit-equal to the product library and to the oracle"""
    E, N, K = shape
    m = Moe8(E, N, K, M, a5=a5, seed=K + a5)
    offs = m.offs(_counts(M, E, "skewed", K))
    one = torch.ones(1, device=DEV)
    prod = q.grouped_matmul_mxf8_bf16_tn(m.a, m.b, m.asf, m.bsf, one, offs)
    _check_vs_oracle(m, offs, prod, groups=list(range(E)), nrows=32)
    lib = lab.load()
    for v in FORMS:
        with lab.forced(gemm_variant=v):
            out = _call(lib, m, offs, one, torch.empty(M, N, dtype=torch.bfloat16, device=DEV))
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), prod.view(torch.int16)), (v, (out != prod).sum().item())


def test_per_expert_alpha(q):
    E, N, K = QWEN_DOWN
    m = Moe8(E, N, K, 1024, seed=2)
    offs = m.offs(_counts(1024, E, "uniform", 4))
    one = torch.ones(1, device=DEV)
    alpha = torch.tensor([2.0 ** ((g % 7) - 3) for g in range(E)], device=DEV)
    base = q.grouped_matmul_mxf8_bf16_tn(m.a, m.b, m.asf, m.bsf, one, offs)
    out = q.grouped_matmul_mxf8_bf16_tn(m.a, m.b, m.asf, m.bsf, alpha, offs)
    o = [0] + offs.cpu().tolist()
    for g in range(E):
        s, e = o[g], o[g + 1]
        assert torch.equal(out[s:e].float(), base[s:e].float() * alpha[g]), g
    _check_vs_dense(q, m, offs, out, alpha)


def test_rows_past_the_last_offset_are_untouched(q):
    """offs[-1] < M through the C entry into a sentinel-filled D: the rows past the end keep the sentinel"""
    from qutlass_amd import _lib

    E, N, K = QWEN_DOWN
    M = 600
    m = Moe8(E, N, K, M, seed=3)
    offs = torch.tensor(np.minimum(np.cumsum(_counts(M, E, "uniform", 8)), 451), dtype=torch.int32, device=DEV)
    assert offs[-1].item() == 451
    D = torch.full((M, N), -12345, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    _call(_lib.load(), m, offs, torch.ones(1, device=DEV), D)
    torch.cuda.synchronize()
    assert (D[451:].view(torch.int16) == -12345).all()
    _check_vs_dense(q, m, offs, D)
    _check_vs_oracle(m, offs, D)


@pytest.mark.parametrize("a5", [False, True])
def test_e1_equals_the_dense_op(q, a5):
    from qutlass_amd.utils import to_blocked

    E, N, K = MIXTRAL_DOWN
    M = 200
    m = Moe8(1, N, K, M, a5=a5, seed=9)
    offs = m.offs([M])
    one = torch.ones(1, device=DEV)
    out = q.grouped_matmul_mxf8_bf16_tn(m.a, m.b, m.asf, m.bsf, one, offs)
    kb = K // 32
    ref = q.matmul_mxf8_bf16_tn(m.a, m.b[0], to_blocked(m.asf.view(M, kb)), to_blocked(m.bsf.view(N, kb)), one)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    _check_vs_oracle(m, offs, out, groups=[0])


def test_stacked_weight_above_2gib(q):
    """E = 160, N = 2048, K = 7168: 2.35 GB of e4m3 -- exact-regime codes; decode routing with the first and the last expert checked"""
    E, N, K, M = 160, 2048, 7168, 320
    m = Moe8(E, N, K, M, seed=11)
    assert m.b.numel() > 2 ** 31
    offs = m.offs(np.full(E, M // E))
    one = torch.ones(1, device=DEV)
    out = q.grouped_matmul_mxf8_bf16_tn(m.a, m.b, m.asf, m.bsf, one, offs)
    o = [0] + offs.cpu().tolist()
    dense = _dense_groups(q, m, offs)
    for g in (0, E - 1):
        assert torch.equal(out[o[g]:o[g + 1]].view(torch.int16), dense[g].view(torch.int16)), g
    _check_vs_oracle(m, offs, out, groups=[0, E - 1], ncols=128)
    del m.b
    torch.cuda.empty_cache()


def test_graph_capture_and_compile(q):
    """one capture, offsets rewritten in place between replays: each replay equals a fresh eager call; torch.compile (inductor) equals eager"""
    E, N, K = QWEN_UP
    M = 512
    m = Moe8(E, N, K, M, seed=7)
    offs = m.offs(_counts(M, E, "uniform", 0))
    one = torch.ones(1, device=DEV)
    op = lambda: q.grouped_matmul_mxf8_bf16_tn(m.a, m.b, m.asf, m.bsf, one, offs)
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
        return q.grouped_matmul_mxf8_bf16_tn(a, b, a_sf, b_sf, alpha, offs)

    torch._dynamo.reset()
    compiled = torch.compile(layer, backend="inductor", fullgraph=True)
    got = compiled(m.a, m.b, m.asf, m.bsf, one, offs)
    assert torch.equal(got.view(torch.int16), op().view(torch.int16))
