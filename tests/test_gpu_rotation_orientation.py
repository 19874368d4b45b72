"""GPU: every rotate-and-quantize entry point against the pinned CPU oracle with a rotation that is NOT its own transpose.

The Sylvester matrix of the `_hadamard(n)` helpers equals its transpose, and fused_quantize_body (csrc/quantize.hip.h) stages h in three different ways -- R = 16 as a
block-diagonal image padded to 32, RP = 32 as a transposed image built from two-byte stores, RP >= 64 as it lies in memory, read back with transposing LDS reads -- so
a kernel applying h.T on any one path would pass every test built on that matrix, the "fused equals the composition" tests included (both sides share the staging).
Here h = (P H D) R^-0.5 (tests/_rotations.py: orthogonal, every entry one magnitude, about half of its entries change under transposition) and x holds integers in
-2 .. 2 times 100: every product and sum of the rotation is exact in fp32 in any order, so scale bytes must EQUAL the oracle's and codes must equal them modulo the
sign of zero -- tolerance zero -- while h.T changes 90 % of the codes (tests/test_rotations_cpu.py).  Rows 1 / 33 / 70 and K = 3 max(R, 32) as in the existing exact
tests.  The one-launch decode GEMM and the NV fuzz (general random h every second draw) use the suite's existing bounds for non-exact operands."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)
import _rotations as rot  # noqa: E402
from _rotations import bits as _np  # noqa: E402
from test_gpu_gated_quantize import _ref_act  # noqa: E402  (the fp64 reference of the activation)

DEV = "cuda:0"
ROWS = (1, 33, 70)
MX, NV = (32, 64, 128), (16, 32, 64, 128)
CASES = [("mx", r) for r in MX] + [("nv", r) for r in NV]
METHODS = [("quest", oracle.QUEST), ("abs_max", oracle.ABS_MAX)]
GS = 2.3            # an NV global scale that is no power of two
GROUP = {"mx": 32, "nv": 16}


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _h(R):
    h = rot.signed_permuted_hadamard(R, seed=1)
    return h.to(DEV), _np(h)


def _oracle(fmt, x_bits, h_bits, om, gs=GS, with_mask=False):
    """-> (codes flat, scale bytes flat[, mask bytes flat]) of the oracle under acc_model 1"""
    if fmt == "mx":
        rq, rs, rm = oracle.fused_quantize_mx(x_bits, h_bits, om, with_mask=with_mask, acc_model=1)
        return (rq, rs, rm) if with_mask else (rq, rs)
    return oracle.fused_quantize_nv(x_bits, h_bits, float(gs), om, acc_model=1)


def _assert_flat(got, want, ctx):
    """got = (codes, scale buffer) of a flat-scale op: the first numel / group scale bytes equal the oracle's, codes equal modulo the sign of zero"""
    rq, rs = want[:2]
    assert np.array_equal(_np(got[1]).reshape(-1)[: rs.size], rs.reshape(-1)), (ctx, "scales", int((_np(got[1]).reshape(-1)[: rs.size] != rs.reshape(-1)).sum()))
    eq = oracle.codes_equal_mod_zero_sign(_np(got[0]).reshape(-1), rq.reshape(-1))
    assert eq.all(), (ctx, "codes", int((~eq).sum()), eq.size)


def _assert_blocked(got, want, rows, k, fmt, ctx):
    """got of a Blocked op: the codes as above, the scales oracle.to_blocked of the oracle's flat scales"""
    rq, rs = want[:2]
    eq = oracle.codes_equal_mod_zero_sign(_np(got[0]).reshape(-1), rq.reshape(-1))
    assert eq.all(), (ctx, "codes", int((~eq).sum()), eq.size)
    assert np.array_equal(_np(got[1]).reshape(-1), oracle.to_blocked(rs.reshape(rows, k // GROUP[fmt]))), (ctx, "blocked scales")


# ------------------------------------------------------------------------------------------------
# 1. the plain quantizers, flat and blocked
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", MX)
@pytest.mark.parametrize("method,om", METHODS)
def test_fused_quantize_mx(q, R, method, om):
    h, hb = _h(R)
    k = 3 * max(R, 32)
    for rows in ROWS:
        x = rot.exact_input((rows, k), seed=R + rows)
        mask = method == "quest" and R == 32
        want = _oracle("mx", _np(x), hb, om, with_mask=mask)
        got = q.fusedQuantizeMx(x.to(DEV), h, method=method, return_mask=mask)
        _assert_flat(got, want, ("mx", R, method, rows))
        if mask:
            assert np.array_equal(_np(got[2]).reshape(-1), want[2]), ("mx", R, rows, "clip mask")
        _assert_blocked(q.fusedQuantizeMxBlocked(x.to(DEV), h, method=method), want, rows, k, "mx", ("mx blocked", R, method, rows))


@pytest.mark.parametrize("R", NV)
@pytest.mark.parametrize("method,om", METHODS)
def test_fused_quantize_nv(q, R, method, om):
    h, hb = _h(R)
    k = 3 * max(R, 32)
    gs = torch.tensor([GS], device=DEV)
    for rows in ROWS:
        x = rot.exact_input((rows, k), seed=R + rows)
        want = _oracle("nv", _np(x), hb, om)
        _assert_flat(q.fusedQuantizeNv(x.to(DEV), h, gs, method=method), want, ("nv", R, method, rows))
        _assert_blocked(q.fusedQuantizeNvBlocked(x.to(DEV), h, gs, method=method), want, rows, k, "nv", ("nv blocked", R, method, rows))


# ------------------------------------------------------------------------------------------------
# 2. the four gated quantizers: gate = 100 (silu(100) == 100 in bf16), up = integers in -2 .. 2 -- the activation stays in the exact regime
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,R", CASES)
@pytest.mark.parametrize("method,om", METHODS)
def test_fused_silu_mul_quantize(q, fmt, R, method, om):
    h, hb = _h(R)
    inter = 3 * max(R, 32)
    gs = torch.tensor([GS], device=DEV)
    for rows in ROWS:
        up = rot.exact_input((rows, inter), seed=2 * R + rows, scale=1.0)
        x = torch.cat([torch.full((rows, inter), 100.0, dtype=torch.bfloat16), up], dim=1)
        act = _ref_act(_np(x))                                   # fp64, two bf16 roundings
        assert np.array_equal(act, _np((up.float() * 100.0).to(torch.bfloat16)))
        want = _oracle(fmt, act, hb, om)
        xd = x.to(DEV)
        if fmt == "mx":
            flat, blocked = q.fusedSiluMulQuantizeMx(xd, h, method=method), q.fusedSiluMulQuantizeMxBlocked(xd, h, method=method)
        else:
            flat, blocked = q.fusedSiluMulQuantizeNv(xd, h, gs, method=method), q.fusedSiluMulQuantizeNvBlocked(xd, h, gs, method=method)
        _assert_flat(flat, want, ("gated", fmt, R, method, rows))
        _assert_blocked(blocked, want, rows, inter, fmt, ("gated blocked", fmt, R, method, rows))


# ------------------------------------------------------------------------------------------------
# 3. the gathering quantizers: M = 53 rows (with repeats) out of T = 37
# ------------------------------------------------------------------------------------------------
T_TOK, M_ROWS = 37, 53


def _gather_input(R):
    k = 3 * max(R, 32)
    x = rot.exact_input((T_TOK, k), seed=3 * R)
    src = torch.randint(0, T_TOK, (M_ROWS,), generator=torch.Generator(device="cpu").manual_seed(R), dtype=torch.int32)
    assert len(set(src.tolist())) < M_ROWS   # repeats
    return k, x, src, _np(x)[src.numpy()]


@pytest.mark.parametrize("fmt,R", CASES)
@pytest.mark.parametrize("method,om", METHODS)
def test_fused_gather_quantize(q, fmt, R, method, om):
    h, hb = _h(R)
    k, x, src, xg_bits = _gather_input(R)
    want = _oracle(fmt, xg_bits, hb, om)
    if fmt == "mx":
        got = q.fusedGatherQuantizeMx(x.to(DEV), h, src.to(DEV), method=method)
    else:
        got = q.fusedGatherQuantizeNv(x.to(DEV), h, torch.tensor([GS], device=DEV), src.to(DEV), method=method)
    _assert_flat(got, want, ("gather", fmt, R, method))


# ------------------------------------------------------------------------------------------------
# 4. one global scale per expert: group by group against the oracle under that group's scale
# ------------------------------------------------------------------------------------------------
COUNTS = np.array([20, 0, 1, 25, 7])                                         # an empty group, a one-row group, boundaries off the 32-row tiles
SCALES = np.array([0.37, 1.4137, 2.6951, 5.1182, 9.7211], dtype=np.float32)  # pairwise different, none a power of two


def _assert_per_group(got, x_bits, hb, om, k, ctx):
    assert COUNTS.sum() == M_ROWS and len(np.unique(SCALES)) == len(SCALES) and ((SCALES.view(np.uint32) & 0x7fffff) != 0).all()
    codes = _np(got[0]).reshape(M_ROWS, k // 2)
    sf = _np(got[1]).reshape(-1)[: M_ROWS * k // 16].reshape(M_ROWS, k // 16)
    ends = np.cumsum(COUNTS)
    for g in range(len(COUNTS)):
        lo, hi = int(ends[g] - COUNTS[g]), int(ends[g])
        if hi > lo:
            rq, rs = _oracle("nv", x_bits[lo:hi], hb, om, gs=SCALES[g])
            assert np.array_equal(sf[lo:hi].reshape(-1), rs), (ctx, "scales of group", g)
            assert oracle.codes_equal_mod_zero_sign(codes[lo:hi].reshape(-1), rq).all(), (ctx, "codes of group", g)


@pytest.mark.parametrize("R", NV)
@pytest.mark.parametrize("method,om", METHODS)
def test_grouped_scale_quantizers(q, R, method, om):
    h, hb = _h(R)
    gs = torch.from_numpy(SCALES).to(DEV)
    offs = torch.tensor(np.cumsum(COUNTS), dtype=torch.int32, device=DEV)
    k, x, src, xg_bits = _gather_input(R)
    got = q.fusedGatherQuantizeNvGrouped(x.to(DEV), h, gs, src.to(DEV), offs, method=method)
    _assert_per_group(got, xg_bits, hb, om, k, ("gather grouped", R, method))
    up = rot.exact_input((M_ROWS, k), seed=5 * R, scale=1.0)
    xg = torch.cat([torch.full((M_ROWS, k), 100.0, dtype=torch.bfloat16), up], dim=1)
    got = q.fusedSiluMulQuantizeNvGrouped(xg.to(DEV), h, gs, offs, method=method)
    _assert_per_group(got, _ref_act(_np(xg)), hb, om, k, ("gated grouped", R, method))


# ------------------------------------------------------------------------------------------------
# 5. backward_t_bf16: x^T rotated per 32 along N
# ------------------------------------------------------------------------------------------------
def test_backward_t_bf16(q):
    B, N, M = 2, 96, 72
    h, hb = _h(32)
    x = rot.exact_input((B, N, M), seed=9)
    e2m1, e8m0 = q.backward_t_bf16(x.to(DEV), h)
    rq, rs = oracle.backward_t_bf16(_np(x), hb, acc_model=1)
    assert e2m1.shape == (B, M, N // 2) and e8m0.shape == (B, M, N // 32)
    assert np.array_equal(_np(e8m0), rs)
    eq = oracle.codes_equal_mod_zero_sign(_np(e2m1).reshape(-1), rq.reshape(-1))
    assert eq.all(), (int((~eq).sum()), eq.size)
    rq_t, _ = oracle.backward_t_bf16(_np(x), np.ascontiguousarray(hb.T), acc_model=1)     # (the comparison can tell: h.T gives other codes)
    assert (~oracle.codes_equal_mod_zero_sign(rq_t.reshape(-1), rq.reshape(-1))).mean() > 0.5


# ------------------------------------------------------------------------------------------------
# 6. the activation path of one linear layer: decode batches (one launch, the GEMM rotates and quantizes its own A operand) and a larger one (two launches)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,one_launch", [(1, True), (8, True), (40, False)])
@pytest.mark.parametrize("method,om", METHODS)
def test_fused_quantize_matmul(q, m, one_launch, method, om):
    """against oracle.fused_quantize_mx followed by oracle.gemm_blockscaled, the weight quantized by the oracle (w @ h); bound: the suite's for non-exact GEMM
    operands (tests/test_gpu_fuzz.py), max |got - want| <= 1e-2 max |want| -- a transposed rotation misses it by two orders of magnitude"""
    n, k = 264, 384
    assert q._decode_single_launch_wins(m, n, k, 32, torch.device(DEV)) == one_launch
    h, hb = _h(32)
    gen = torch.Generator(device="cpu").manual_seed(17 + m)
    x = (torch.randn(m, k, generator=gen) * 25.0).to(torch.bfloat16)
    w = (torch.randn(n, k, generator=gen) * 25.0).to(torch.bfloat16)
    wq, ws, _ = oracle.fused_quantize_mx(_np(w), hb, oracle.ABS_MAX, acc_model=1)
    xq, xs, _ = oracle.fused_quantize_mx(_np(x), hb, om, acc_model=1)
    alpha = (1.0 / 9.0) if method == "abs_max" else (1.0 / 3.0)   # abs_max codes sit at 3 x the value, quest codes at the value
    alpha = float(np.float32(alpha))
    w_sf = oracle.to_blocked(ws.reshape(n, k // 32))
    ref = oracle.gemm_blockscaled(oracle.KIND_MXFP4, xq.reshape(m, k // 2), wq.reshape(n, k // 2), oracle.to_blocked(xs.reshape(m, k // 32)), w_sf, alpha, m, n, k)
    want = oracle.bf16_bits_to_f32(ref).astype(np.float64)
    got = q.fused_quantize_matmul_mxf4_bf16_tn(x.to(DEV), h, torch.from_numpy(wq.reshape(n, k // 2)).to(DEV), torch.from_numpy(w_sf).to(DEV).view(torch.float8_e8m0fnu),
                                               torch.tensor([alpha], device=DEV), method=method)
    assert got.shape == (m, n) and got.dtype == torch.bfloat16
    err = np.abs(got.float().cpu().numpy().astype(np.float64) - want).max()
    print(f"m={m} {method}: max |got - want| = {err / np.abs(want).max():.2e} max |want|")
    assert err <= 1e-2 * np.abs(want).max(), (m, method, err, np.abs(want).max())
    # the layer means x w^T: the unquantized product is within fp4's noise of it (a wrong alpha or a weight rotated the other way round is not)
    exact = x.double().numpy() @ w.double().numpy().T
    assert np.linalg.norm(want - exact) <= 0.35 * np.linalg.norm(exact)


# ------------------------------------------------------------------------------------------------
# 7. NV fuzz: random shapes, magnitudes and global scales, a general random h every second draw
# ------------------------------------------------------------------------------------------------
def test_fuzz_quantize_nv(q):
    """test_fuzz_quantizers_and_swizzle's caps; tests/test_rotations_cpu.py shows for the same draws that the oracle's two accumulation models stay within half of them"""
    for it, R, x, h, gs, method in rot.nv_fuzz_draws():
        got = q.fusedQuantizeNv(x.to(DEV), h.to(DEV), torch.tensor([gs], device=DEV), method=method)
        rq, rs = oracle.fused_quantize_nv(_np(x), _np(h), gs, oracle.QUEST if method == "quest" else oracle.ABS_MAX, acc_model=1)
        got_s = _np(got[1]).reshape(-1)[: rs.size]
        cap_s, cap_c = rot.nv_fuzz_caps(rs.size, 2 * rq.size)
        sbad = int((got_s != rs).sum())
        same_grp = got_s == rs
        eq = oracle.codes_equal_mod_zero_sign(_np(got[0]).reshape(-1), rq)
        cbad = int((~eq & same_grp.repeat(16)).sum())
        print(f"it {it}: R={R} {method} {tuple(x.shape)} gs={gs:.3f}: {sbad} of {rs.size} scale bytes, {cbad} of {eq.size} codes differ")
        assert sbad <= cap_s, (it, R, method, tuple(x.shape), sbad, cap_s)
        assert cbad <= cap_c, (it, R, method, tuple(x.shape), cbad, cap_c)
