"""W4A16 grouped GEMM (qutlass_amd.grouped_matmul_bf16_mxf4_bf16_tn: bf16 tokens against MXFP4 expert weights) on the MI355X: the product op and each form (606, 607,
608) forced through the lab library.  The reference is fp64 dequantise + matmul + one rounding to bf16 (tests/_w4a16_model.py).  In the exact regime (operands
asserted exact on the CPU, here and in tests/test_grouped_w4a16_cpu.py: every product a multiple of one quantum, sum |terms| < 2^24 quanta) any summation order
gives the same fp32 bits, so every such comparison is bit for bit.  The K of the ladder: tests/_w4a16_model.py LADDER_K."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (bf16 helpers)
import _benchlib as lab  # noqa: E402  (the LAB build: forced forms)
import _w4a8_model as W8  # noqa: E402
import _w4a16_model as W  # noqa: E402

DEV = "cuda:0"
FORMS = (606, 607, 608)   # 32x32, 32x16, 64x32 tiles of the bf16-token wave-owned kernel
E4, E8M0 = torch.float8_e4m3fn, torch.float8_e8m0fnu
LADDER_K, LADDER_COUNTS, RAGGED_N, RAGGED_COUNTS, ONE_HOT = W.LADDER_K, W.LADDER_COUNTS, W.RAGGED_N, W.RAGGED_COUNTS, W.ONE_HOT


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _offs(counts):
    return torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)


def _entry(lib):
    f = lib.qutlass_amd_grouped_matmul_bf16_mxf4_bf16_tn
    f.restype = ctypes.c_int
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    f.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, vp, i64, i64, i64, i64, vp]
    return f


def _call(lib, ops, shape, offs, alpha, D=None, src_row=None):
    """the C entry of `lib` (the product or the lab library) on device operands; with src_row the tokens are the unsorted (T, K) ones"""
    x, b, bsf = ops
    M, N, K, E = shape
    if D is None:
        D = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    rc = _entry(lib)(x.data_ptr(), b.data_ptr(), bsf.data_ptr(), alpha.data_ptr(), alpha.numel(), offs.data_ptr(), src_row.data_ptr() if src_row is not None else None,
                     x.size(0) if src_row is not None else 0, D.data_ptr(), M, N, K, E, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.qutlass_amd_last_error().decode()
    return D


def _every_form(q, ops, shape, counts, alpha=None, src_row=None):
    """the product op and each forced form: {name: (M, N) int16 bits on the CPU}"""
    offs = _offs(counts)
    al = torch.ones(1, device=DEV) if alpha is None else alpha
    outs = {"product": q.grouped_matmul_bf16_mxf4_bf16_tn(*ops, al, offs, src_row=src_row)}
    assert tuple(outs["product"].shape) == shape[:2] and outs["product"].dtype == torch.bfloat16
    lib = lab.load()
    for v in FORMS:
        with lab.forced(gemm_variant=v):
            outs[v] = _call(lib, ops, shape, offs, al, src_row=src_row)
    torch.cuda.synchronize()
    return {k: o.view(torch.int16).cpu() for k, o in outs.items()}


def _assert_bits(got, want, end, what):
    bad = (got[:end] != want[:end])
    if bad.any():
        r, c = np.argwhere(bad.numpy())[0]
        g = oracle.bf16_bits_to_f32(got.numpy().view(np.uint16))
        w = oracle.bf16_bits_to_f32(want.numpy().view(np.uint16))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ from the reference, first at ({r}, {c}): got {g[r, c]}, want {w[r, c]}")


def _check_exact(q, p, counts, what):
    W.assert_exact(p, counts)
    want = W.to_bf16_bits(W.reference_f64(p, counts))
    end = int(np.sum(counts))
    for name, got in _every_form(q, p.device(DEV), (p.M, p.N, p.K, p.E), counts).items():
        _assert_bits(got, want, end, f"{what}, {name}")


# ---- 1. K-index pairing ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,shift", ONE_HOT)
def test_one_hot_k_pairing(q, K, shift):
    """token row j holds a single 1 at K index shift + j: out[j, n] must be b[n, shift + j] 2^(sfb[n, blk] - 127) exactly, in every form -- a wrong nibble order in the
    convert, a wrong K assignment in the bf16 fragment or a scale from the wrong block moves the value (neighbouring k never share a weight value)"""
    p = W.one_hot_problem(K, shift)
    k = shift + np.arange(p.M)
    bv = W.E2M1[W.unpack_e2m1(p.b)][0]                                           # (N, K)
    want64 = bv[:, k].T * np.ldexp(1.0, p.sfb[0][:, k // 32].T.astype(np.int64) - 127)
    assert np.array_equal(want64, W.reference_f64(p, [p.M]))
    want = W.to_bf16_bits(want64)
    for name, got in _every_form(q, p.device(DEV), (p.M, p.N, p.K, p.E), [p.M]).items():
        _assert_bits(got, want, p.M, f"one-hot K={K} shift={shift}, {name}")


# ---- 2. the K ladder ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", LADDER_K)
def test_k_ladder_every_form(q, K):
    _check_exact(q, W.exact_problem(3, 40, K, 64, seed=K), LADDER_COUNTS, f"K={K}")


# ---- 3. rows and columns -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", RAGGED_N)
def test_ragged_rows_and_columns(q, N):
    _check_exact(q, W.exact_problem(9, N, 640, int(np.sum(RAGGED_COUNTS)), seed=N), RAGGED_COUNTS, f"N={N}")


def test_two_groups_per_decode_lane(q):
    rng = np.random.default_rng(65)
    counts = rng.integers(0, 2, 65)
    counts[37] = 40
    _check_exact(q, W.exact_problem(65, 40, 640, int(counts.sum()), seed=65), counts, "E=65")


# ---- 4. the dense wrapper ----------------------------------------------------------------------------------------------------------------------------------

def test_e1_equals_the_dense_wrapper(q):
    p = W.exact_problem(1, 72, 640, 70, seed=1)
    W.assert_exact(p, [70])
    x, b, bsf = p.device(DEV)
    one = torch.ones(1, device=DEV)
    grouped = q.grouped_matmul_bf16_mxf4_bf16_tn(x, b, bsf, one, _offs([70]))
    dense = q.matmul_bf16_mxf4_bf16_tn(x, b[0], bsf, one)
    assert dense.shape == (70, 72) and torch.equal(dense.view(torch.int16), grouped.view(torch.int16))
    _assert_bits(dense.view(torch.int16).cpu(), W.to_bf16_bits(W.reference_f64(p, [70])), 70, "dense wrapper")


# ---- 5. cross-check against W4A8 ----------------------------------------------------------------------------------------------------------------------------

def test_equals_w4a8_on_tokens_that_are_e4m3_values(q):
    """tokens whose values are also e4m3 values, once as bf16 and once as e4m3 codes with every token scale byte 127 (2^0): the same weights, the same bits"""
    counts = RAGGED_COUNTS
    M = int(np.sum(counts))
    p8 = W8.exact_problem(9, 72, 640, M, seed=4)
    p8.sfa[:] = 127
    W8.assert_exact(p8, counts)
    a8, b, asf, bsf = p8.device(DEV)
    p = W.W4A16(W.bf16_bits(torch.from_numpy(p8.a).view(E4).float().numpy().astype(np.float64)), p8.b, p8.sfb)
    W.assert_exact(p, counts)
    one, offs = torch.ones(1, device=DEV), _offs(counts)
    ref8 = q.grouped_matmul_mxf8_mxf4_bf16_tn(a8, b, asf, bsf, one, offs).view(torch.int16).cpu()
    for name, got in _every_form(q, p.device(DEV), (M, 72, 640, 9), counts).items():
        assert torch.equal(got, ref8), f"{name}: differs from grouped_matmul_mxf8_mxf4_bf16_tn on the same values"
    _assert_bits(ref8, W.to_bf16_bits(W.reference_f64(p, counts)), M, "the W4A8 op against this op's reference")


# ---- 6. gather ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [640, 1664])   # one shot and ring
def test_gather_equals_index_select(q, K):
    """with src_row the op equals itself on x.index_select(0, src_row), bit for bit; src_row repeats tokens, T != M; the indices -1 and T give the rows of an all-zero
    token and never read the NaN-filled tensors x lies between"""
    counts = [33, 0, 70, 5]
    M, T, N, E, G = int(np.sum(counts)), 37, 40, 4, 8
    p = W.exact_problem(E, N, K, T, seed=6 + K)
    rng = np.random.default_rng(6)
    src = rng.integers(0, T, M).astype(np.int32)
    src[[0, 40, 107]] = -1
    src[[5, 32, 33, 100]] = T
    src[[7, 64]] = [-(2 ** 31), 2 ** 31 - 1]
    ok = (src >= 0) & (src < T)
    assert len(set(src[ok].tolist())) < ok.sum(), "repeats"
    xs = np.where(ok[:, None], p.x_f64()[np.where(ok, src, 0)], 0.0)        # the sorted tokens, zero rows for the indices outside [0, T)
    W.assert_exact(p, counts, x=xs)
    x, b, bsf = p.device(DEV)
    arena = torch.full((G + T + G, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    arena[G:G + T] = x
    x = arena[G:G + T]
    assert x.is_contiguous() and torch.isnan(arena[G - 1]).all() and torch.isnan(arena[G + T]).all()
    src_d = torch.from_numpy(src).to(DEV)
    sorted_x = torch.from_numpy(W.bf16_bits(xs).view(np.int16)).to(DEV).view(torch.bfloat16)
    plain = q.grouped_matmul_bf16_mxf4_bf16_tn(sorted_x, b, bsf, torch.ones(1, device=DEV), _offs(counts)).view(torch.int16).cpu()
    want = W.to_bf16_bits(W.reference_f64(p, counts, x=xs))
    _assert_bits(plain, want, M, "the op on the gathered copy")
    for name, got in _every_form(q, (x, b, bsf), (M, N, K, E), counts, src_row=src_d).items():
        assert not torch.isnan(got.view(torch.bfloat16).float()).any(), f"{name}: a guard value reached an output"
        assert torch.equal(got, plain), f"{name}: differs from the op on x.index_select(0, src_row)"
    assert (got[[0, 40, 107, 5, 32, 33, 100, 7, 64]] == 0).all(), "an index outside [0, T) is an all-zero token"


# ---- 7. per-expert alpha ------------------------------------------------------------------------------------------------------------------------------------

def test_per_expert_alpha(q):
    counts = [5, 0, 40, 19]
    p = W.exact_problem(4, 40, 640, 64, seed=7)
    W.assert_exact(p, counts)
    x, b, bsf = p.device(DEV)
    offs = _offs(counts)
    alpha = torch.tensor([0.25, 8.0, 2.0, 0.5], device=DEV)
    base = q.grouped_matmul_bf16_mxf4_bf16_tn(x, b, bsf, torch.ones(1, device=DEV), offs)
    out = q.grouped_matmul_bf16_mxf4_bf16_tn(x, b, bsf, alpha, offs)
    for g, s, e in W.groups(counts):
        assert torch.equal(out[s:e].float(), base[s:e].float() * alpha[g]), g
    want = W.to_bf16_bits(W.reference_f64(p, counts, alpha.cpu().numpy()))
    for name, got in _every_form(q, (x, b, bsf), (64, 40, 640, 4), counts, alpha=alpha).items():
        _assert_bits(got, want, 64, f"per-expert alpha, {name}")


# ---- 8. masked rows and malformed offs ------------------------------------------------------------------------------------------------------------------------

def test_rows_past_the_last_offset_keep_the_sentinel(q):
    from qutlass_amd import _lib

    counts = [10, 0, 33, 2]          # 45 of M = 70 rows
    p = W.exact_problem(4, 40, 640, 70, seed=8)
    W.assert_exact(p, counts)
    want = W.to_bf16_bits(W.reference_f64(p, counts))
    for lib, v in [(_lib.load(), 0)] + [(lab.load(), v) for v in FORMS]:
        D = torch.full((70, 40), -12345, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        with lab.forced(gemm_variant=v):
            _call(lib, p.device(DEV), (70, 40, 640, 4), _offs(counts), torch.ones(1, device=DEV), D)
        torch.cuda.synchronize()
        assert (D[45:].view(torch.int16) == -12345).all(), v
        _assert_bits(D.view(torch.int16).cpu(), want, 45, f"offs[-1] < M, form {v}")


def test_decreasing_offset_is_an_empty_group(q):
    from qutlass_amd import _lib

    M = 64
    p = W.exact_problem(4, 40, 640, M, seed=9)
    W.assert_exact(p, [20, 0, 44, 0])
    offs = torch.tensor([20, 12, 200, -3], dtype=torch.int32, device=DEV)   # -> ends 20, 20, 64 (clamped), 64: groups of 20, 0, 44, 0 rows
    want = W.to_bf16_bits(W.reference_f64(p, [20, 0, 44, 0]))
    for lib, v in [(_lib.load(), 0)] + [(lab.load(), v) for v in FORMS]:
        guard = torch.full((M + 16, 40), -12345, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        D = guard[8:8 + M]
        with lab.forced(gemm_variant=v):
            _call(lib, p.device(DEV), (M, 40, 640, 4), offs, torch.ones(1, device=DEV), D)
        torch.cuda.synchronize()
        assert (guard[:8].view(torch.int16) == -12345).all() and (guard[8 + M:].view(torch.int16) == -12345).all(), "a write outside [0, M)"
        _assert_bits(D.view(torch.int16).cpu(), want, M, f"decreasing offset, form {v}")


# ---- 9. scale bytes ------------------------------------------------------------------------------------------------------------------------------------------

def test_scale_bytes_2_and_252(q):
    """the ends of the exact scale range, 2^-125 and 2^125, each against tokens moved the other way by a power of two (block 2: x 2^123 against byte 2, block 3:
    x 2^-123 against byte 252; bf16 holds both exactly, the smallest nonzero token is 2^-126, the largest 15.875 x 2^123) so that every product stays a multiple of
    the regime's quantum -- a byte decoded one off doubles or halves those blocks' share of every output"""
    counts = [33]
    p = W.exact_problem(1, 40, 640, 33, seed=11)
    x64 = p.x_f64()
    x64[:, 64:96] *= 2.0 ** 123
    x64[:, 96:128] *= 2.0 ** -123
    p = W.W4A16(W.bf16_bits(x64), p.b, p.sfb)
    p.sfb[0, :, 2], p.sfb[0, :, 3] = 2, 252
    wmag = np.abs(p.b_f64()[0][:, 64:128])
    assert wmag[wmag > 0].min() == 2.0 ** -126 and wmag.max() == 4.0 * 2.0 ** 125    # (EXACT_VALS: 0.5 ... 4)
    terms = p.x_f64()[:, None, :] * p.b_f64()[0][None, :, :]
    quantum = 2.0 ** -6          # (1/8) x (1/2 x 2^-2) with scale bytes 125 ... 129; blocks 2 and 3: (1/8 x 2^+-123) x (1/2 x 2^-+125)
    assert np.array_equal(terms / quantum, np.round(terms / quantum)) and np.abs(terms).sum(-1).max() < 2.0 ** 24 * quantum
    want = W.to_bf16_bits(W.reference_f64(p, counts))
    for name, got in _every_form(q, p.device(DEV), (33, 40, 640, 1), counts).items():
        _assert_bits(got, want, 33, f"scale bytes 2 and 252, {name}")


def test_scale_byte_255_and_non_finite_tokens(q):
    """byte 255: NaN in every output of that weight row for the rows of that expert -- also where the token is 0 over the whole block (0 x NaN) -- and nowhere else;
    inf and NaN tokens propagate as in fp64: the NaN positions equal the reference's exactly, the rest (the infinities included) is bit-equal"""
    counts = [33, 0, 31]
    p = W.exact_problem(3, 40, 640, 64, seed=12)
    x64 = p.x_f64()
    x64[44, 352:384] = 0.0          # row 44 (expert 2) is zero over block 11
    x64[3, 7] = np.inf              # row 3 (expert 0): +-inf, NaN where the weight is 0
    x64[50, 300] = np.nan           # row 50: every output
    p = W.W4A16(W.bf16_bits(np.where(np.isfinite(x64), x64, 0.0)), p.b, p.sfb)
    p.x[3, 7], p.x[50, 300] = 0x7F80, 0x7FC0
    p.sfb[2, 5, 11] = 255           # expert 2, column 5: rows 33 .. 63
    fin_x = np.where(np.isfinite(p.x_f64()), p.x_f64(), 0.0)
    W.assert_exact(p, counts, x=fin_x)
    with np.errstate(invalid="ignore"):
        want64 = W.reference_f64(p, counts)
    nan = np.isnan(want64)
    expect = np.zeros((64, 40), bool)
    expect[33:, 5] = True
    expect[50, :] = True
    expect[3, :] = p.b_f64()[0][:, 7] == 0
    assert np.array_equal(nan, expect) and np.isinf(want64[3]).sum() == 40 - expect[3].sum() > 0
    want = W.to_bf16_bits(np.where(nan, 0.0, want64))
    for name, got in _every_form(q, p.device(DEV), (64, 40, 640, 3), counts).items():
        got_nan = torch.isnan(got.view(torch.bfloat16).float()).numpy()
        assert np.array_equal(got_nan, expect), f"{name}: NaN positions differ in {int((got_nan != expect).sum())} outputs"
        _assert_bits(torch.where(torch.from_numpy(expect), torch.zeros((), dtype=torch.int16), got), want, 64, f"the outputs that are not NaN, {name}")


# ---- 10. quantised Gaussians -----------------------------------------------------------------------------------------------------------------------------------

def _dequant(b, bsf, E, N, K):
    return W.E2M1[W.unpack_e2m1(b.view(torch.uint8).cpu().numpy())] * np.repeat(W.scale_f64(bsf.view(torch.uint8).cpu().numpy().reshape(E, N, K // 32)), 32, axis=-1)


def test_quantised_gaussians_within_the_derived_bound(q):
    """every output within |want| 2^-8 + K 2^-24 (|x| @ |w|^T) of the fp64 reference: the final rounding to bf16 (2^-9 relative, a factor 2 of margin) plus the
    worst case of K fp32 additions in any order (each at most 2^-24 of the running sum of magnitudes)"""
    E, N, K, M = 4, 72, 2176, 150
    counts = [90, 0, 7, 53]
    torch.manual_seed(5)
    eye = torch.eye(32, dtype=torch.bfloat16, device=DEV)
    x = torch.randn(M, K, dtype=torch.bfloat16, device=DEV) * 25.0
    w = torch.randn(E * N, K, dtype=torch.bfloat16, device=DEV)
    b, bsf = q.fusedQuantizeMx(w, eye, method="abs_max")
    b, bsf = b.view(E, N, K // 2), bsf.view(-1)[:E * N * (K // 32)].contiguous()
    wd = _dequant(b, bsf, E, N, K)
    x64 = x.float().cpu().numpy().astype(np.float64)
    want = np.concatenate([x64[s:e] @ wd[g].T for g, s, e in W.groups(counts)])
    mag = np.concatenate([np.abs(x64[s:e]) @ np.abs(wd[g]).T for g, s, e in W.groups(counts)])
    tol = np.abs(want) * 2.0 ** -8 + K * 2.0 ** -24 * mag
    shape = (M, N, K, E)
    for name, got in _every_form(q, (x, b, bsf), shape, counts).items():
        err = np.abs(got.view(torch.bfloat16).float().numpy().astype(np.float64) - want)
        print(f"quantised Gaussians, {name}: max err / tol = {(err / tol).max():.4f}, max |want| = {np.abs(want).max():.4g}")
        assert (err <= tol).all(), f"{name}: {int((err > tol).sum())} of {err.size} outputs outside |want| 2^-8 + K 2^-24 |x| @ |w|^T"   # every output


# ---- 11. graph capture and torch.compile ------------------------------------------------------------------------------------------------------------------------

def test_graph_capture_and_compile(q):
    E, N, K, M, T = 8, 64, 512, 96, 40
    p = W.exact_problem(E, N, K, M, seed=10)
    x, b, bsf = p.device(DEV)
    one = torch.ones(1, device=DEV)
    offs = _offs([12] * 8)
    src = torch.from_numpy(np.random.default_rng(10).integers(0, T, M).astype(np.int32)).to(DEV)
    op = lambda: q.grouped_matmul_bf16_mxf4_bf16_tn(x, b, bsf, one, offs)
    gop = lambda: q.grouped_matmul_bf16_mxf4_bf16_tn(x[:T], b, bsf, one, offs, src_row=src)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op(), gop()                # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out, static_gout = op(), gop()
    xs = x[:T].index_select(0, src.long())
    for counts in ([12] * 8, [0, 40, 0, 1, 33, 0, 0, 10], [96, 0, 0, 0, 0, 0, 0, 0]):
        W.assert_exact(p, counts)
        offs.copy_(_offs(counts))
        graph.replay()
        torch.cuda.synchronize()
        end = int(np.sum(counts))
        eager = op()
        assert torch.equal(static_out[:end].view(torch.int16), eager[:end].view(torch.int16)), counts
        _assert_bits(eager.view(torch.int16).cpu(), W.to_bf16_bits(W.reference_f64(p, counts)), end, f"counts {counts}")
        assert torch.equal(static_gout[:end].view(torch.int16), q.grouped_matmul_bf16_mxf4_bf16_tn(xs, b, bsf, one, offs)[:end].view(torch.int16)), ("gather", counts)

    def layer(x, b, b_sf, alpha, offs, src_row):
        return q.grouped_matmul_bf16_mxf4_bf16_tn(x, b, b_sf, alpha, offs), q.grouped_matmul_bf16_mxf4_bf16_tn(x[:T], b, b_sf, alpha, offs, src_row=src_row)

    torch._dynamo.reset()
    compiled = torch.compile(layer, backend="inductor", fullgraph=True)
    got, ggot = compiled(x, b, bsf, one, offs, src)
    assert torch.equal(got.view(torch.int16), op().view(torch.int16)) and torch.equal(ggot.view(torch.int16), gop().view(torch.int16))


# ---- 12. the point of the feature -------------------------------------------------------------------------------------------------------------------------------

def test_w4a16_is_closer_than_w4a8_on_the_same_weights(q):
    """the operands of tests/test_gpu_grouped_w4a8.py test_w4a8_is_closer_than_w4a4_on_the_same_weights: 64 Gaussian tokens against fixed MXFP4 weights, reference
    fp64 x @ dequant(W)^T.  Unquantised tokens must lose less than 8-bit tokens, and no more than the final rounding to bf16 allows (2^-8)"""
    E, N, K, M = 4, 64, 512, 64
    counts = [16, 16, 16, 16]
    torch.manual_seed(8)
    eye = torch.eye(32, dtype=torch.bfloat16, device=DEV)
    x = torch.randn(M, K, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(E * N, K, dtype=torch.bfloat16, device=DEV)
    kb = K // 32
    b, bsf = q.fusedQuantizeMx(w, eye, method="abs_max")
    b, bsf = b.view(E, N, K // 2), bsf.view(-1)[:E * N * kb].contiguous()
    a8, a8sf = q.fusedQuantizeMxf8(x, eye)
    one, offs = torch.ones(1, device=DEV), _offs(counts)
    y8 = q.grouped_matmul_mxf8_mxf4_bf16_tn(a8, b, a8sf.view(-1)[:M * kb].contiguous(), bsf, one, offs)
    y16 = q.grouped_matmul_bf16_mxf4_bf16_tn(x, b, bsf, one, offs)
    wd = _dequant(b, bsf, E, N, K)
    x64 = x.float().cpu().numpy().astype(np.float64)
    ref = np.concatenate([x64[s:e] @ wd[g].T for g, s, e in W.groups(counts)])
    rel = lambda y: np.linalg.norm(y.float().cpu().numpy().astype(np.float64) - ref) / np.linalg.norm(ref)
    e16, e8 = rel(y16), rel(y8)
    print(f"relative Frobenius error vs fp64 x @ dequant(W)^T: W4A16 {e16:.6f}, W4A8 {e8:.5f}")
    assert e16 < e8, (e16, e8)
    assert e16 < 2.0 ** -8, e16
