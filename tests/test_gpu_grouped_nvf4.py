"""Grouped NVFP4 GEMM for mixture-of-experts layers (qutlass_amd.grouped_matmul_nvf4_bf16_tn) on the MI355X: exact-regime operands bit-equal to the CPU oracle
(on oracle.to_blocked of each group's row-major scales) and to the dense matmul_nvf4_bf16_tn per group, for the product rule and for every form forced through the
lab library; quantised Gaussians through fusedQuantizeNv with per-expert global scales; scale bytes past K and NaN scale bytes; per-expert alpha, rows past
offs[-1] left untouched, E = 1 and E = 1024, malformed offsets, a stacked weight above 2 GiB, graph capture with offsets rewritten between replays, and
torch.compile."""
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
FORMS = (598, 599, 600, 601)                                       # 32x32, 64x32 tiles of the wave-owned kernel; 64x64, 128x128 tiles of the tile kernel
E4 = torch.float8_e4m3fn


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


class MoeNv:
    """Expert-sorted e2m1 tokens (M, K/2) and stacked expert weights (E, N, K/2) with ROW-MAJOR e4m3 scales (one per 16 elements), as the op reads them.
    The exact regime of tests/test_gpu_round6.py::test_nvf4_wave_owned_kernel_against_the_oracle: any e2m1 code, scale bytes 0x30 ... 0x47 (2^-1 ... 2^1 x 1.0 ... 1.875):
    every product and every partial sum is exact in fp32, so any K order gives the same bits."""

    def __init__(self, E, N, K, M, seed=0):
        self.E, self.N, self.K, self.M = E, N, K, M
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.a = torch.randint(0, 256, (M, K // 2), dtype=torch.uint8, device=DEV, generator=g)
        self.b = torch.empty(E, N, K // 2, dtype=torch.uint8, device=DEV)
        for e in range(E):                                            # (per expert: keeps the temporaries small)
            self.b[e] = torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device=DEV, generator=g)
        self.asf = torch.randint(0x30, 0x48, (M * (K // 16),), dtype=torch.uint8, device=DEV, generator=g).view(E4)
        self.bsf = torch.randint(0x30, 0x48, (E * N * (K // 16),), dtype=torch.uint8, device=DEV, generator=g).view(E4)

    def offs(self, counts):
        return torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)

    def bsf_of(self, g):
        n = self.N * self.K // 16
        return self.bsf[g * n:(g + 1) * n]


def _dense_groups(q, m, offs, alpha=None, only=None):
    """per-group matmul_nvf4_bf16_tn with to_blocked scales (host offsets): the loop the grouped op replaces"""
    from qutlass_amd.utils import to_blocked

    o = [0] + offs.cpu().tolist()
    kb = m.K // 16
    outs = {}
    for g in range(m.E) if only is None else only:
        s, e = o[g], o[g + 1]
        if e <= s:
            continue
        al = alpha[g:g + 1] if alpha is not None and alpha.numel() > 1 else (alpha if alpha is not None else torch.ones(1, device=DEV))
        outs[g] = q.matmul_nvf4_bf16_tn(m.a[s:e], m.b[g], to_blocked(m.asf[s * kb:e * kb].view(e - s, kb)), to_blocked(m.bsf_of(g).view(m.N, kb)), al)
    return outs


def _same(got, ref):
    """bit-equal, NaNs in the same places (a NaN's payload is not compared)"""
    gn, rn = got.isnan(), ref.isnan()
    return torch.equal(gn, rn) and torch.equal(got.view(torch.int16)[~gn], ref.view(torch.int16)[~rn])


def _check_vs_dense(q, m, offs, out, alpha=None, only=None):
    o = [0] + offs.cpu().tolist()
    for g, ref in _dense_groups(q, m, offs, alpha, only).items():
        got = out[o[g]:o[g + 1]]
        assert _same(got, ref), f"group {g}: {(got.view(torch.int16) != ref.view(torch.int16)).sum().item()} outputs differ from matmul_nvf4_bf16_tn"


def _check_vs_oracle(m, offs, out, groups=None, ncols=256, nrows=48, alpha=None):
    """each checked group against oracle.gemm_blockscaled on oracle.to_blocked of that group's row-major scales (sampled rows / columns: CPU time)"""
    o = [0] + offs.cpu().tolist()
    kb = m.K // 16
    live = [g for g in range(m.E) if o[g + 1] > o[g]]
    if groups is None:
        sizes = {g: o[g + 1] - o[g] for g in live}
        groups = sorted({live[0], live[-1], max(live, key=sizes.get)} | set(live[:: max(1, len(live) // 4)]))
    cols = np.unique(np.r_[np.arange(min(ncols // 2, m.N)), np.arange(max(0, m.N - ncols // 2), m.N)])
    aq, asf, outn = _np(m.a), _np(m.asf).reshape(-1)[: m.M * kb].reshape(m.M, kb), _np(out)
    al = None if alpha is None else alpha.cpu().numpy()
    for g in groups:
        s, e = o[g], o[g + 1]
        if e <= s:
            continue
        rows = np.arange(s, e) if e - s <= nrows else np.r_[np.arange(s, s + nrows // 2), np.arange(e - nrows // 2, e)]
        bq = _np(m.b[g][torch.from_numpy(cols).to(DEV)])
        bsf = _np(m.bsf_of(g)).reshape(m.N, kb)[cols]
        a_g = 1.0 if al is None else float(al[g if al.size > 1 else 0])
        ref = oracle.gemm_blockscaled(oracle.KIND_NVFP4, np.ascontiguousarray(aq[rows]), bq, oracle.to_blocked(np.ascontiguousarray(asf[rows])), oracle.to_blocked(bsf),
                                      a_g, len(rows), len(cols), m.K)
        got = outn[rows][:, cols]
        assert np.array_equal(got, ref), f"group {g}: {(got != ref).sum()} of {got.size} sampled outputs differ from the oracle"


def _entry(lib):
    f = lib.qutlass_amd_grouped_matmul_nvf4_bf16_tn
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    return f


def _call(lib, m, offs, alpha, D):
    rc = _entry(lib)(m.a.data_ptr(), m.b.data_ptr(), m.asf.data_ptr(), m.bsf.data_ptr(), alpha.data_ptr(), alpha.numel(), offs.data_ptr(), D.data_ptr(),
                     m.M, m.N, m.K, m.E, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.qutlass_amd_last_error().decode()
    return D


def _forced(m, offs, alpha, v):
    with lab.forced(gemm_variant=v):
        out = _call(lab.load(), m, offs, alpha, torch.empty(m.M, m.N, dtype=torch.bfloat16, device=DEV))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape,M,kind", [
    (QWEN_UP, 512, "uniform"),        # decode: batch 64 x top-8
    (QWEN_UP, 512, "skewed"),
    (QWEN_DOWN, 512, "empty"),
    (QWEN_DOWN, 4096, "uniform"),     # mean 32 rows per expert
    (QWEN_UP, 20000, "skewed"),       # reduced prefill: mean 156 rows per expert, one of 10000
    (MIXTRAL_UP, 128, "uniform"),     # decode: batch 64 x top-2
    (MIXTRAL_UP, 1024, "skewed"),     # mean 128 rows per expert
    (MIXTRAL_DOWN, 128, "empty"),     # K = 14336: the wave-owned kernel's refilled slots
    (MIXTRAL_DOWN, 2048, "uniform"),  # reduced prefill: 256 rows per expert
])
def test_grouped_exact_vs_oracle_and_dense(q, shape, M, kind):
    E, N, K = shape
    m = MoeNv(E, N, K, M, seed=M + E)
    offs = m.offs(_counts(M, E, kind, seed=M + E))
    alpha = torch.ones(1, device=DEV)
    out = q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, alpha, offs)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    _check_vs_dense(q, m, offs, out)
    _check_vs_oracle(m, offs, out)


# group sizes that are not multiples of 32, N not a multiple of any tile width, K = 128, K % 256 == 128, one-shot K (1024, 2048 for the 32-row tiles) and K long enough
# for the refilled slots (4608: 18 stages; 14336)
RAGGED = [((16, 512, 1024), 700, "skewed"), ((6, 328, 384), 333, "uniform"), ((5, 200, 128), 150, "skewed"), ((16, 264, 2048), 500, "empty"), ((8, 256, 4608), 900, "uniform"),
          ((4, 264, 14336), 300, "skewed"), ((3, 136, 2432), 420, "uniform")]


@pytest.mark.parametrize("shape,M,kind", RAGGED)
def test_every_form_through_the_lab_library(q, shape, M, kind):
    """598 ... 601 forced: each bit-equal to the oracle (every group), to the dense op per group and to the product rule's output"""
    E, N, K = shape
    m = MoeNv(E, N, K, M, seed=K + M)
    offs = m.offs(_counts(M, E, kind, K))
    half = torch.tensor([0.5], device=DEV)
    prod = q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, half, offs)
    _check_vs_oracle(m, offs, prod, groups=list(range(E)), nrows=32, alpha=half)
    _check_vs_dense(q, m, offs, prod, half)
    for v in FORMS:
        out = _forced(m, offs, half, v)
        assert torch.equal(out.view(torch.int16), prod.view(torch.int16)), (v, (out != prod).sum().item())


def _hadamard(n):
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h * n ** -0.5).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("shape,M,kind", [((16, 512, 2048), 700, "skewed"), ((8, 1024, 4096), 300, "uniform"), ((32, 256, 768), 96, "empty"), ((4, 384, 1408), 1500, "uniform")])
def test_grouped_on_quantised_gaussians(q, shape, M, kind):
    """fusedQuantizeNv's operands, its scale buffer passed as it is, every expert's weight with a global scale of its own (alpha[g] = 1 / (gs_a gs_b[g])).
    Which case of the two applies: the grouped forms and the dense plan may walk K in different orders (the dense op picks split-K, 16x16x32-MFMA and persistent
    kernels by shape), but on such data every fp32 partial sum is still exact -- the dense NVFP4 tests assert EXACT equality with the fp64 oracle for quantised
    Gaussians (tests/test_gpu_parity.py, tests/test_gpu_baseline_configs.py::test_c4_nvfp4_8192_cubed_vs_oracle; the reference asserts out.equal(out_ref)) -- so
    both bars hold here: bit-equal to the dense op per group, and bit-equal to the oracle, for the product rule and every forced form."""
    E, N, K = shape
    torch.manual_seed(K + M)
    h = _hadamard(16)
    gs_a = 3.0
    gs_b = [1.5 * (1 + g % 5) for g in range(E)]
    x = torch.randn(M, K, dtype=torch.bfloat16, device=DEV) * 3.0
    a_q, a_s = q.fusedQuantizeNv(x, h, torch.tensor([gs_a], device=DEV))
    m = MoeNv.__new__(MoeNv)
    m.E, m.N, m.K, m.M = E, N, K, M
    m.a, m.asf = a_q, a_s                                           # (padded_rows, K / 16) buffer, written flat: passed as it is
    bq, bs = [], []
    for g in range(E):
        w = torch.randn(N, K, dtype=torch.bfloat16, device=DEV) * 3.0
        wq, ws = q.fusedQuantizeNv(w, h, torch.tensor([gs_b[g]], device=DEV))
        bq.append(wq)
        bs.append(ws.reshape(-1)[: N * K // 16])
    m.b, m.bsf = torch.stack(bq), torch.cat(bs)
    alpha = torch.tensor([1.0 / (gs_a * gs_b[g]) for g in range(E)], device=DEV)
    offs = m.offs(_counts(M, E, kind, seed=M))
    out = q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, alpha, offs)
    flat = MoeNv.__new__(MoeNv)                                     # the same operands with the A scales cut to their M K / 16 written bytes (the per-group loop slices them)
    flat.__dict__.update(m.__dict__)
    flat.asf = a_s.reshape(-1)[: M * K // 16]
    _check_vs_dense(q, flat, offs, out, alpha)
    _check_vs_oracle(flat, offs, out, groups=list(range(E)), nrows=24, ncols=128, alpha=alpha)
    for v in FORMS:
        got = _forced(m, offs, alpha, v)
        assert torch.equal(got.view(torch.int16), out.view(torch.int16)), (v, (got != out).sum().item())


@pytest.mark.parametrize("K", [384, 128, 2432, 4736])   # K % 256 == 128: one shot (384, 128, 2432) and the refilled slots (4736 = 18.5 stages)
def test_scales_past_k_and_nan_scale_bytes(q, K):
    """K % 256 == 128: the last stage's upper two scale dwords lie past the row -- in the row-major layout they are the NEXT row's first scales.  A NaN byte (0x7f / 0xff)
    planted as the first scale of row r + 1 (A) / column c + 1 (B, one expert) makes exactly that row / that expert's column NaN, never row r / column c, and the
    result equals the dense op; the same for a NaN byte in the middle of a row."""
    from qutlass_amd.utils import to_blocked  # noqa: F401

    E, N, M = 3, 136, 300
    counts = [90, 0, 210]
    kb = K // 16
    one = torch.ones(1, device=DEV)
    for where in ("first", "middle"):
        m = MoeNv(E, N, K, M, seed=K)
        offs = m.offs(counts)
        col = 0 if where == "first" else kb // 2
        arows = [13, 89, 150, 299]                        # group 0 (one its last row), group 2 (one the last row of all)
        bcols = {0: [1, 135], 2: [64]}
        asf, bsf = m.asf.view(torch.uint8).view(M, kb), m.bsf.view(torch.uint8).view(E, N, kb)
        for i, r in enumerate(arows):
            asf[r, col] = 0x7F if i % 2 == 0 else 0xFF
        for g, cs in bcols.items():
            for c in cs:
                bsf[g, c, col] = 0x7F
        bsf[1, 7, col] = 0xFF                             # the empty group's weight: no effect
        want = torch.zeros(M, N, dtype=torch.bool, device=DEV)
        want[arows] = True
        want[0:90, bcols[0]] = True
        want[90:300, bcols[2]] = True
        outs = [q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, one, offs)] + [_forced(m, offs, one, v) for v in FORMS]
        for i, out in enumerate(outs):
            assert torch.equal(out.isnan(), want), (K, where, i, (out.isnan() != want).sum().item())
            _check_vs_dense(q, m, offs, out)


def test_per_expert_alpha(q):
    E, N, K = QWEN_DOWN
    m = MoeNv(E, N, K, 1024, seed=2)
    offs = m.offs(_counts(1024, E, "uniform", 4))
    one = torch.ones(1, device=DEV)
    alpha = torch.tensor([2.0 ** ((g % 7) - 3) for g in range(E)], device=DEV)
    base = q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, one, offs)
    out = q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, alpha, offs)
    o = [0] + offs.cpu().tolist()
    for g in range(E):
        s, e = o[g], o[g + 1]
        assert torch.equal(out[s:e].float(), base[s:e].float() * alpha[g]), g
    third = torch.tensor([1.0 / (3 + g) for g in range(E)], device=DEV)           # not powers of two: alpha[g] is applied in fp32 before the rounding, as in the dense op
    out3 = q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, third, offs)
    _check_vs_dense(q, m, offs, out3, third)
    _check_vs_oracle(m, offs, out3, alpha=third)
    for v in FORMS:
        assert torch.equal(_forced(m, offs, third, v).view(torch.int16), out3.view(torch.int16)), v


def test_rows_past_the_last_offset_are_untouched(q):
    """offs[-1] < M through the C entry into a sentinel-filled D: the rows past the end keep the sentinel (every form)"""
    from qutlass_amd import _lib

    E, N, K = QWEN_DOWN
    M = 600
    m = MoeNv(E, N, K, M, seed=3)
    offs = torch.tensor(np.minimum(np.cumsum(_counts(M, E, "uniform", 8)), 451), dtype=torch.int32, device=DEV)
    assert offs[-1].item() == 451
    D = torch.full((M, N), -12345, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    _call(_lib.load(), m, offs, torch.ones(1, device=DEV), D)
    torch.cuda.synchronize()
    assert (D[451:].view(torch.int16) == -12345).all()
    _check_vs_dense(q, m, offs, D)
    _check_vs_oracle(m, offs, D)
    for v in FORMS:
        D2 = torch.full((M, N), -12345, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        with lab.forced(gemm_variant=v):
            _call(lab.load(), m, offs, torch.ones(1, device=DEV), D2)
        torch.cuda.synchronize()
        assert torch.equal(D2.view(torch.int16), D.view(torch.int16)), v


def test_e1_equals_the_dense_op(q):
    from qutlass_amd.utils import to_blocked

    E, N, K = MIXTRAL_DOWN
    M = 200
    m = MoeNv(1, N, K, M, seed=9)
    offs = m.offs([M])
    one = torch.ones(1, device=DEV)
    out = q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, one, offs)
    kb = K // 16
    ref = q.matmul_nvf4_bf16_tn(m.a, m.b[0], to_blocked(m.asf.view(M, kb)), to_blocked(m.bsf.view(N, kb)), one)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    _check_vs_oracle(m, offs, out, groups=[0])


def test_e1024_with_most_groups_empty(q):
    E, N, K, M = 1024, 264, 640, 700
    m = MoeNv(E, N, K, M, seed=10)
    rng = np.random.default_rng(10)
    counts = np.zeros(E, dtype=np.int64)
    live = np.sort(rng.choice(E, size=20, replace=False))
    live[0], live[-1] = 0, E - 1
    counts[live] = np.bincount(rng.integers(0, 20, M), minlength=20)
    offs = m.offs(counts)
    alpha = torch.tensor([2.0 ** (g % 3) for g in range(E)], device=DEV)
    out = q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, alpha, offs)
    _check_vs_dense(q, m, offs, out, alpha)
    _check_vs_oracle(m, offs, out, groups=[int(g) for g in live], nrows=16, alpha=alpha)
    for v in FORMS:
        assert torch.equal(_forced(m, offs, alpha, v).view(torch.int16), out.view(torch.int16)), v


def test_malformed_offsets_write_nothing_outside_and_agree_with_the_clamped_reading(q):
    """negative, decreasing and past-M offsets: the output lies in the middle of a sentinel-filled buffer whose guard rows stay untouched, and the rows written are those
    of the clamped running maximum of the offsets"""
    from qutlass_amd import _lib

    E, N, K, M, G = 6, 264, 896, 517, 256
    m = MoeNv(E, N, K, M, seed=12)
    one = torch.ones(1, device=DEV)
    for bad in ([600, 10, 20, 700, 5, 1 << 30], [-5, 140, 130, -(1 << 31), 300, 280], [M + 1] * 6, [100, 90, 80, 70, 60, 50], [-1] * 6, [0, 0, 200, 2 ** 31 - 1, 3, 400]):
        ends = np.maximum.accumulate(np.clip(np.asarray(bad, dtype=np.int64), 0, M))
        good = torch.tensor(ends, dtype=torch.int32, device=DEV)
        badt = torch.tensor(np.asarray(bad, dtype=np.int64).astype(np.int32), dtype=torch.int32, device=DEV)
        want = torch.full((M, N), -12345, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        _call(_lib.load(), m, good, one, want)
        if ends[-1] > 0:
            _check_vs_dense(q, m, good, want)
        libs = [(_lib.load(), 0)] + [(lab.load(), v) for v in FORMS]
        for L, v in libs:
            buf = torch.full((M + 2 * G, N), -12345, dtype=torch.int16, device=DEV)
            D = buf[G:G + M].view(torch.bfloat16)
            with lab.forced(gemm_variant=v):
                _call(L, m, badt, one, D)
            torch.cuda.synchronize()
            assert (buf[:G] == -12345).all() and (buf[G + M:] == -12345).all(), (bad, v)
            assert torch.equal(D.view(torch.int16), want.view(torch.int16)), (bad, v)


def test_stacked_weight_above_2gib(q):
    """E = 160, N = 2048, K = 14336: 2.35 GB of packed e2m1 -- decode routing with the first and the last expert checked"""
    E, N, K, M = 160, 2048, 14336, 320
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 2 ** 30:
        pytest.skip(f"a 2.35 GB stacked weight and its scales need 6 GiB of free device memory ({free >> 20} MiB free)")
    m = MoeNv(E, N, K, M, seed=11)
    assert m.b.numel() > 2 ** 31
    offs = m.offs(np.full(E, M // E))
    one = torch.ones(1, device=DEV)
    out = q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, one, offs)
    _check_vs_dense(q, m, offs, out, only=[0, 1, E // 2, E - 1])
    _check_vs_oracle(m, offs, out, groups=[0, E - 1], ncols=128)
    for v in (600, 601):     # (the forms the rule does not pick here rebase B in the same 64-bit arithmetic: one each of the two kernels is enough)
        assert torch.equal(_forced(m, offs, one, v).view(torch.int16), out.view(torch.int16)), v
    del m.b
    torch.cuda.empty_cache()


def test_graph_capture_and_compile(q):
    """one capture, offsets rewritten in place between replays: each replay equals a fresh eager call; torch.compile (inductor, fullgraph) of a small layer equals eager"""
    E, N, K = QWEN_UP
    M = 512
    m = MoeNv(E, N, K, M, seed=7)
    offs = m.offs(_counts(M, E, "uniform", 0))
    one = torch.ones(1, device=DEV)
    op = lambda: q.grouped_matmul_nvf4_bf16_tn(m.a, m.b, m.asf, m.bsf, one, offs)
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
        _check_vs_oracle(m, offs, static_out, nrows=16, ncols=64)

    def layer(a, b, a_sf, b_sf, alpha, offs):
        return q.grouped_matmul_nvf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs).float() * 2

    torch._dynamo.reset()
    compiled = torch.compile(layer, backend="inductor", fullgraph=True)
    got = compiled(m.a, m.b, m.asf, m.bsf, one, offs)
    end = offs[-1].item()
    assert torch.equal(got[:end], layer(m.a, m.b, m.asf, m.bsf, one, offs)[:end])
