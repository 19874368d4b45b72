"""W4A6 grouped GEMM (qutlass_amd.grouped_matmul_mxf6_mxf4_bf16_tn: MXFP6 e2m3 tokens against MXFP4 expert weights) on the MI355X -- tests/test_gpu_grouped_w4a8.py
section by section, on the product op and on each forced form 610-612.  The reference is fp64 dequantise + matmul + one rounding to bf16 (tests/_mxf6_model.py); in
the exact regime (operands asserted exact on the CPU) any summation order gives the same fp32 bits, so equality with the reference is bit for bit.

K values of the ladder: a stage is 128 K elements; the 32-row forms (610, 611) run one shot with 1, 2, 3, 4 and 7 slots per wave (K <= 512, 1024, 1536, 2048, 3584)
and rings of 7 slots beyond; the 64-row form (612) one shot with 1, 2, 3, 4 slots (K <= 2048) and rings of 4 slots beyond.  The list holds the K on either side of
every rung and 7296 (57 stages: a ring of 7 slots that wraps twice, a ring of 4 that wraps three times)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (bf16 helpers)
import _benchlib as lab  # noqa: E402  (the LAB build: forced forms)
import _mxf6_model as W  # noqa: E402

DEV = "cuda:0"
FORMS = (610, 611, 612)   # 32x32, 32x16, 64x32 tiles of the 6-bit-token wave-owned kernel
E4, E8M0 = torch.float8_e4m3fn, torch.float8_e8m0fnu
LADDER_K = (128, 512, 640, 1024, 1152, 1536, 1664, 2048, 2176, 3584, 3712, 7296)


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _offs(counts):
    return torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)


def _entry(lib):
    f = lib.qutlass_amd_grouped_matmul_mxf6_mxf4_bf16_tn
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    return f


def _call(lib, ops, shape, offs, alpha, D=None):
    """the C entry of `lib` (the product or the lab library) on device operands"""
    a, b, asf, bsf = ops
    M, N, K, E = shape
    if D is None:
        D = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    rc = _entry(lib)(a.data_ptr(), b.data_ptr(), asf.data_ptr(), bsf.data_ptr(), alpha.data_ptr(), alpha.numel(), offs.data_ptr(), D.data_ptr(), M, N, K, E,
                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.qutlass_amd_last_error().decode()
    return D


def _every_form(q, p, counts, alpha=None):
    """the product op and each forced form: {name: (M, N) int16 bits on the CPU}"""
    ops = p.device(DEV)
    offs = _offs(counts)
    al = torch.ones(1, device=DEV) if alpha is None else alpha
    outs = {"product": q.grouped_matmul_mxf6_mxf4_bf16_tn(*ops, al, offs)}
    lib = lab.load()
    for v in FORMS:
        with lab.forced(gemm_variant=v):
            outs[v] = _call(lib, ops, (p.M, p.N, p.K, p.E), offs, al)
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
    for name, got in _every_form(q, p, counts).items():
        _assert_bits(got, want, end, f"{what}, {name}")


# ---- 1. K-index pairing ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,shift", [(128, 0), (256, 0), (256, 128)])
def test_one_hot_k_pairing(q, K, shift):
    """token row j holds the single code 0x2D (-1.625: sign, exponent and mantissa bits all mixed) at K index shift + j: out[j, n] must be
    -1.625 b[n, shift + j] 2^(sfa[j, blk] + sfb[n, blk] - 254) exactly, in every form -- a wrong bit layout of the 6-bit fragment, a wrong pairing of A's and B's K
    indices inside the mixed MFMA fragment, or of a block with its scale byte, moves the value"""
    p = W.one_hot_problem(K, shift)
    k = shift + np.arange(p.M)
    bv = W.E2M1[W.unpack_e2m1(p.b)][0]                                           # (N, K)
    hot = W.E2M3[W.HOT_CODE]
    assert hot == -1.625
    want64 = hot * bv[:, k].T * np.ldexp(1.0, p.sfa[np.arange(p.M), k // 32].astype(np.int64)[:, None] + p.sfb[0][:, k // 32].T.astype(np.int64) - 254)
    assert np.array_equal(want64, W.reference_f64(p, [p.M]))
    want = W.to_bf16_bits(want64)
    for name, got in _every_form(q, p, [p.M]).items():
        _assert_bits(got, want, p.M, f"one-hot K={K} shift={shift}, {name}")


# ---- 2. the K ladder ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", LADDER_K)
def test_k_ladder_every_form(q, K):
    counts = [33, 0, 31]
    p = W.exact_problem(3, 40, K, 64, seed=K, a_vals="both" if K <= 2176 else "e2m1")   # (the multiples of 1/8 have a finer quantum: kept to the K where the sums stay exact)
    _check_exact(q, p, counts, f"K={K}")


# ---- 3. rows and columns -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [8, 24, 40, 72])
def test_ragged_rows_and_columns(q, N):
    counts = [0, 1, 31, 32, 33, 0, 65, 64, 2]
    p = W.exact_problem(9, N, 640, int(np.sum(counts)), seed=N)
    _check_exact(q, p, counts, f"N={N}")


def test_two_groups_per_decode_lane(q):
    rng = np.random.default_rng(65)
    counts = rng.integers(0, 2, 65)
    counts[37] = 40
    p = W.exact_problem(65, 40, 640, int(counts.sum()), seed=65)
    _check_exact(q, p, counts, "E=65")


def test_e1_equals_the_dense_wrapper(q):
    p = W.exact_problem(1, 72, 640, 70, seed=1)
    W.assert_exact(p, [70])
    a, b, asf, bsf = p.device(DEV)
    one = torch.ones(1, device=DEV)
    grouped = q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, asf, bsf, one, _offs([70]))
    dense = q.matmul_mxf6_mxf4_bf16_tn(a, b[0], asf, bsf, one)
    assert dense.shape == (70, 72) and torch.equal(dense.view(torch.int16), grouped.view(torch.int16))
    _assert_bits(dense.view(torch.int16).cpu(), W.to_bf16_bits(W.reference_f64(p, [70])), 70, "dense wrapper")


# ---- 4. cross-checks against the existing grouped ops --------------------------------------------------------------------------------------------------------

def test_equals_w4a8_on_recoded_tokens_and_mxf4_on_e2m1_tokens(q):
    counts = [0, 1, 31, 32, 33, 0, 65, 64, 2]
    M = int(np.sum(counts))
    offs, one = _offs(counts), torch.ones(1, device=DEV)
    p = W.exact_problem(9, 72, 640, M, seed=4)
    W.assert_exact(p, counts)
    a, b, asf, bsf = p.device(DEV)
    out = q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, asf, bsf, one, offs)
    a8 = torch.from_numpy(p.a_as_e4m3()).to(DEV).view(E4)
    ref8 = q.grouped_matmul_mxf8_mxf4_bf16_tn(a8, b, asf, bsf, one, offs)
    assert torch.equal(out[:M].view(torch.int16), ref8[:M].view(torch.int16)), "differs from grouped_matmul_mxf8_mxf4_bf16_tn on the tokens re-encoded as e4m3"
    p2 = W.exact_problem(9, 72, 640, M, seed=5, a_vals="e2m1")
    W.assert_exact(p2, counts)
    a, b, asf, bsf = p2.device(DEV)
    out = q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, asf, bsf, one, offs)
    a4 = torch.from_numpy(p2.a_as_e2m1()).to(DEV)
    ref4 = q.grouped_matmul_mxf4_bf16_tn(a4, b, asf, bsf, one, offs)
    assert torch.equal(out[:M].view(torch.int16), ref4[:M].view(torch.int16)), "differs from grouped_matmul_mxf4_bf16_tn on the tokens re-encoded as e2m1"


# ---- 5. quantised Gaussians ----------------------------------------------------------------------------------------------------------------------------------

def _mxfp8_tol(want):
    return np.abs(want) / 128.0 + 2e-5 * np.abs(want).max()   # the project's own bound (tests/test_gpu_grouped_mxf8.py _mxfp8_close)


def _host_problem(a, asf, b, bsf, M, E, N, K):
    kb = K // 32
    return W.W4A6(a.view(torch.uint8).cpu().numpy(), b.view(torch.uint8).cpu().numpy(), asf.view(torch.uint8).cpu().numpy().reshape(M, kb),
                  bsf.view(torch.uint8).cpu().numpy().reshape(E, N, kb))


def test_quantised_gaussians_within_the_project_bound(q):
    E, N, K, M = 4, 72, 2176, 150
    counts = [90, 0, 7, 53]
    torch.manual_seed(5)
    eye = torch.eye(32, dtype=torch.bfloat16, device=DEV)
    x = torch.randn(M, K, dtype=torch.bfloat16, device=DEV) * 25.0
    w = torch.randn(E * N, K, dtype=torch.bfloat16, device=DEV)
    a, asf = q.fusedQuantizeMxf6(x, eye)
    b, bsf = q.fusedQuantizeMx(w, eye, method="abs_max")
    kb = K // 32
    assert a.shape == (M, K * 3 // 4) and a.dtype == torch.uint8
    asf, bsf = asf.view(-1)[:M * kb].contiguous(), bsf.view(-1)[:E * N * kb].contiguous()
    b = b.view(E, N, K // 2)
    out = q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, asf, bsf, torch.ones(1, device=DEV), _offs(counts))
    want = W.reference_f64(_host_problem(a, asf, b, bsf, M, E, N, K), counts)
    got = out.float().cpu().numpy().astype(np.float64)
    err, tol = np.abs(got - want), _mxfp8_tol(want)
    print(f"quantised Gaussians: max |err| / tol = {(err / tol).max():.4f}, max |want| = {np.abs(want).max():.4g}")
    assert (err <= tol).all(), f"{int((err > tol).sum())} of {err.size} outputs outside |want| / 128 + 2e-5 max |want|"   # every output


# ---- 6. contract edges ---------------------------------------------------------------------------------------------------------------------------------------

def test_per_expert_alpha(q):
    counts = [5, 0, 40, 19]
    p = W.exact_problem(4, 40, 640, 64, seed=6)
    a, b, asf, bsf = p.device(DEV)
    offs = _offs(counts)
    alpha = torch.tensor([0.25, 8.0, 2.0, 0.5], device=DEV)
    base = q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, asf, bsf, torch.ones(1, device=DEV), offs)
    out = q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, asf, bsf, alpha, offs)
    for g, s, e in W.groups(counts):
        assert torch.equal(out[s:e].float(), base[s:e].float() * alpha[g]), g
    _assert_bits(out.view(torch.int16).cpu(), W.to_bf16_bits(W.reference_f64(p, counts, alpha.cpu().numpy())), 64, "per-expert alpha")


def test_rows_past_the_last_offset_keep_the_sentinel(q):
    from qutlass_amd import _lib

    counts = [10, 0, 33, 2]          # 45 of M = 70 rows
    p = W.exact_problem(4, 40, 640, 70, seed=7)
    D = torch.full((70, 40), -12345, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    _call(_lib.load(), p.device(DEV), (70, 40, 640, 4), _offs(counts), torch.ones(1, device=DEV), D)
    torch.cuda.synchronize()
    assert (D[45:].view(torch.int16) == -12345).all()
    _assert_bits(D.view(torch.int16).cpu(), W.to_bf16_bits(W.reference_f64(p, counts)), 45, "offs[-1] < M")


def test_decreasing_offset_is_an_empty_group(q):
    from qutlass_amd import _lib

    M = 64
    p = W.exact_problem(4, 40, 640, M, seed=8)
    offs = torch.tensor([20, 12, 200, -3], dtype=torch.int32, device=DEV)   # -> ends 20, 20, 64 (clamped), 64: groups of 20, 0, 44, 0 rows
    guard = torch.full((M + 16, 40), -12345, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    D = guard[8:8 + M]
    _call(_lib.load(), p.device(DEV), (M, 40, 640, 4), offs, torch.ones(1, device=DEV), D)
    torch.cuda.synchronize()
    assert (guard[:8].view(torch.int16) == -12345).all() and (guard[8 + M:].view(torch.int16) == -12345).all(), "a write outside [0, M)"
    _assert_bits(D.view(torch.int16).cpu(), W.to_bf16_bits(W.reference_f64(p, [20, 0, 44, 0])), M, "decreasing offset")


def test_scale_byte_255_on_each_side(q):
    counts = [33, 0, 31]
    p = W.exact_problem(3, 40, 640, 64, seed=9)
    p.sfa[3, 7] = 255            # row 3 (group 0): every output of the row
    p.sfa[40, 0] = 255           # row 40 (group 2)
    p.sfb[2, 5, 11] = 255        # expert 2, column 5: rows 33 .. 63
    want64 = W.reference_f64(p, counts)
    nan = np.isnan(want64)
    expect = np.zeros((64, 40), bool)
    expect[3, :] = True
    expect[40, :] = True
    expect[33:, 5] = True
    assert np.array_equal(nan, expect)
    a, b, asf, bsf = p.device(DEV)
    one, offs = torch.ones(1, device=DEV), _offs(counts)
    fin = ~expect
    want = torch.from_numpy(np.where(fin, want64, 0.0)).to(torch.float32).to(torch.bfloat16)
    ref8 = q.grouped_matmul_mxf8_mxf4_bf16_tn(torch.from_numpy(p.a_as_e4m3()).to(DEV).view(E4), b, asf, bsf, one, offs)
    assert np.array_equal(torch.isnan(ref8).cpu().numpy(), expect), "the W4A8 op's NaN positions"
    outs = {"product": q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, asf, bsf, one, offs)}
    lib = lab.load()
    for v in FORMS:
        with lab.forced(gemm_variant=v):
            outs[v] = _call(lib, (a, b, asf, bsf), (64, 40, 640, 3), offs, one)
    torch.cuda.synchronize()
    for name, out in outs.items():
        got_nan = torch.isnan(out).cpu().numpy()
        assert np.array_equal(got_nan, expect), f"{name}: NaN positions differ in {int((got_nan != expect).sum())} outputs"
        kept = torch.where(torch.from_numpy(fin), out.cpu(), torch.zeros((), dtype=torch.bfloat16))
        assert torch.equal(kept.view(torch.int16), want.view(torch.int16)), f"{name}: the finite outputs"


def test_scale_bytes_0_and_254(q):
    """the ends of the finite scale range, 2^-127 and 2^127, each against the other end on the other operand (block 2: A 0 x B 254, block 3: A 254 x B 0) so that
    every product stays a multiple of the regime's quantum -- a byte decoded one off doubles or halves those blocks' share of every output"""
    counts = [33]
    p = W.exact_problem(1, 40, 640, 33, seed=11)
    p.sfa[:, 2], p.sfb[0, :, 2] = 0, 254
    p.sfa[:, 3], p.sfb[0, :, 3] = 254, 0
    terms = p.a_f64()[:, None, :] * p.b_f64()[0][None, :, :]
    quantum = 2.0 ** -8          # (1/8 x 2^-2) x (1/2 x 2^-2) with scale bytes 125 ... 129; blocks 2 and 3: (1/8) x (1/2) x 2^0
    assert np.array_equal(terms / quantum, np.round(terms / quantum)) and np.abs(terms).sum(-1).max() < 2.0 ** 24 * quantum
    want = W.to_bf16_bits(W.reference_f64(p, counts))
    for name, got in _every_form(q, p, counts).items():
        _assert_bits(got, want, 33, f"scale bytes 0 and 254, {name}")


# ---- 7. graph capture and torch.compile ------------------------------------------------------------------------------------------------------------------------

def test_graph_capture_and_compile(q):
    E, N, K, M = 8, 64, 512, 96
    p = W.exact_problem(E, N, K, M, seed=10)
    a, b, asf, bsf = p.device(DEV)
    one = torch.ones(1, device=DEV)
    offs = _offs([12] * 8)
    op = lambda: q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, asf, bsf, one, offs)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op()                       # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = op()
    for counts in ([12] * 8, [0, 40, 0, 1, 33, 0, 0, 10], [96, 0, 0, 0, 0, 0, 0, 0]):
        offs.copy_(_offs(counts))
        graph.replay()
        torch.cuda.synchronize()
        end = int(np.sum(counts))
        eager = op()
        assert torch.equal(static_out[:end].view(torch.int16), eager[:end].view(torch.int16)), counts
        _assert_bits(eager.view(torch.int16).cpu(), W.to_bf16_bits(W.reference_f64(p, counts)), end, f"counts {counts}")

    def layer(a, b, a_sf, b_sf, alpha, offs):
        return q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs)

    torch._dynamo.reset()
    compiled = torch.compile(layer, backend="inductor", fullgraph=True)
    got = compiled(a, b, asf, bsf, one, offs)
    assert torch.equal(got.view(torch.int16), op().view(torch.int16))


# ---- 8. the point of the feature -------------------------------------------------------------------------------------------------------------------------------

def point_inputs():
    """the 64 x 512 tokens and the (4 x 64) x 512 weights of the test below, generated on the CPU with a fixed seed (tests/test_mxf6_model_cpu.py runs the CPU model
    on the same data)"""
    gen = torch.Generator(device="cpu").manual_seed(8)
    x = torch.randn(64, 512, generator=gen).to(torch.bfloat16)
    w = torch.randn(4 * 64, 512, generator=gen).to(torch.bfloat16)
    return x, w


def test_w4a6_is_far_closer_than_w4a4_on_the_same_weights(q):
    """64 Gaussian tokens against fixed MXFP4 weights, reference fp64 x @ dequant(W)^T: 6-bit tokens must lose less than half of what 4-bit tokens lose (the CPU model
    on the same data: e6 = 0.0280, e4 = 0.1145, a factor of 4; measured on the MI355X: e6 = 0.02836, e8 = 0.02649, e4 = 0.11877).  No order is asserted between e6 and e8: they are within 10 % of each other."""
    E, N, K, M = 4, 64, 512, 64
    counts = [16, 16, 16, 16]
    xc, wc = point_inputs()
    x, w = xc.to(DEV), wc.to(DEV)
    eye = torch.eye(32, dtype=torch.bfloat16, device=DEV)
    kb = K // 32
    b, bsf = q.fusedQuantizeMx(w, eye, method="abs_max")
    b, bsf = b.view(E, N, K // 2), bsf.view(-1)[:E * N * kb].contiguous()
    a6, a6sf = q.fusedQuantizeMxf6(x, eye)
    a8, a8sf = q.fusedQuantizeMxf8(x, eye)
    a4, a4sf = q.fusedQuantizeMx(x, eye, method="abs_max")
    one, offs = torch.ones(1, device=DEV), _offs(counts)
    flat = lambda sf: sf.view(-1)[:M * kb].contiguous()
    y6 = q.grouped_matmul_mxf6_mxf4_bf16_tn(a6, b, flat(a6sf), bsf, one, offs)
    y8 = q.grouped_matmul_mxf8_mxf4_bf16_tn(a8, b, flat(a8sf), bsf, one, offs)
    third = torch.full((1,), 1.0 / 3.0, device=DEV)   # fusedQuantizeMx's abs_max codes sit at three times the value; the MXFP6 / MXFP8 quantizers' at the value
    y4 = q.grouped_matmul_mxf4_bf16_tn(a4, b, flat(a4sf), bsf, third, offs)
    wd = W.E2M1[W.unpack_e2m1(b.view(torch.uint8).cpu().numpy())] * np.repeat(W.scale_f64(bsf.view(torch.uint8).cpu().numpy().reshape(E, N, kb)), 32, axis=-1)
    x64 = xc.float().numpy().astype(np.float64)
    ref = np.concatenate([x64[s:e] @ wd[g].T for g, s, e in W.groups(counts)])
    rel = lambda y: np.linalg.norm(y.float().cpu().numpy().astype(np.float64) - ref) / np.linalg.norm(ref)
    e6, e8, e4 = rel(y6), rel(y8), rel(y4)
    print(f"relative Frobenius error vs fp64 x @ dequant(W)^T: W4A6 e6 = {e6:.5f}, W4A8 e8 = {e8:.5f}, W4A4 e4 = {e4:.5f}")
    assert e6 < e4 / 2, (e6, e4)


# ---- 9. the torch op's own rejections ------------------------------------------------------------------------------------------------------------------------------

def test_the_torch_op_turns_bad_arguments_away(q):
    """the op is registered for no particular device (the list of ops under the CUDA key is walked by tests/test_gpu_ext_rejections.py), so its checks are held here:
    a CPU tensor, a non-contiguous one, wrong dtypes and shapes, and the C entry's own K and alignment checks behind them"""
    op = torch.ops.qutlass_amd.grouped_matmul_mxf6_mxf4
    M, N, K, E = 64, 40, 256, 2

    def args(**over):
        d = dict(a=torch.zeros(M, K * 3 // 4, dtype=torch.uint8, device=DEV), b=torch.zeros(E, N, K // 2, dtype=torch.uint8, device=DEV),
                 a_sf=torch.full((M * K // 32,), 127, dtype=torch.uint8, device=DEV).view(E8M0), b_sf=torch.full((E * N * K // 32,), 127, dtype=torch.uint8, device=DEV).view(E8M0),
                 alpha=torch.ones(1, device=DEV), offs=torch.tensor([30, 64], dtype=torch.int32, device=DEV))
        d.update(over)
        return tuple(d.values())

    ok = args()
    assert op(*ok).shape == (M, N)
    for over, msg in ((dict(a=ok[0].cpu()), "Expected tensor to have cuda DeviceType"),
                      (dict(a=torch.zeros(K * 3 // 4, M, dtype=torch.uint8, device=DEV).T), "Expected contiguous tensor"),
                      (dict(a=ok[0].view(E4)), "A must be uint8"),
                      (dict(b=ok[1].view(E4)), "B must be uint8 or float4_e2m1fn_x2"),
                      (dict(a_sf=ok[2].view(torch.uint8)), "A_sf must be float8_e8m0fnu"),
                      (dict(a=torch.zeros(M, K, dtype=torch.uint8, device=DEV)), "Inner dimensions must match"),
                      (dict(b=ok[1][0]), "A must be 2D (M, 3K/4) and B 3D (E, N, K/2)"),
                      (dict(offs=ok[5].long()), "offs must be an int32 tensor of E = 2 elements"),
                      (dict(alpha=torch.ones(3, device=DEV)), "alpha must be a float32 tensor of 1 or E = 2 elements"),
                      (dict(a_sf=ok[2][:-1]), "the row-major scale layout of A needs"),
                      (dict(a=torch.zeros(M, 144, dtype=torch.uint8, device=DEV), b=torch.zeros(E, N, 96, dtype=torch.uint8, device=DEV)), "K must be a positive multiple of 128"),
                      (dict(a=torch.zeros(M * K * 3 // 4 + 8, dtype=torch.uint8, device=DEV)[8:].view(M, K * 3 // 4)), "A must be 16-byte aligned")):
        with pytest.raises(RuntimeError) as e:
            op(*args(**over))
        assert msg in str(e.value), (msg, str(e.value))
