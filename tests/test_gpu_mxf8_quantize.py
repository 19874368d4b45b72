"""The MXFP8 rotate-and-quantize ops on the GPU -- fusedQuantizeMxf8[Blocked], fusedGatherQuantizeMxf8, fusedSiluMulQuantizeMxf8[Blocked] -- against the numpy model of
their contract (tests/_mxf8_quant_model.py, itself pinned to the oracle by tests/test_mxf8_quantize_cpu.py): byte for byte wherever y = x_group @ h is exact, against
the device's own MX quantizer for the scale bytes and against fp64 with a derived bound for the codes on arbitrary rotations; then the layouts, the three fused
forms against their compositions, non-finite inputs, the GEMMs taking the operands as they are, and graph capture.

A wave owns a tile of 32 rows x max(R, 32) elements and a workgroup has 4 waves: the shapes cover less than a tile, a tile's tail and more than one workgroup."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
import _mxf8_quant_model as model  # noqa: E402
import _rotations as rot  # noqa: E402
from _rotations import bits as _np  # noqa: E402

DEV = "cuda:0"
ROTS = (32, 64, 128)
DTYPES = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
FMTS = tuple(DTYPES)


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _identity(R):
    return torch.eye(R, dtype=torch.bfloat16)


def _flat(sf, n):
    return _np(sf).reshape(-1)[:n]


def _run(q, x, h, fmt):
    """the plain op on CPU tensors -> (codes uint8 of x's shape, the numel / 32 flat scale bytes)"""
    codes, sf = q.fusedQuantizeMxf8(x.to(DEV), h.to(DEV), dtype=DTYPES[fmt])
    assert codes.dtype == DTYPES[fmt] and codes.shape == x.shape and sf.dtype == torch.float8_e8m0fnu
    return _np(codes), _flat(sf, x.numel() // 32)


def _want(x, h, fmt):
    """the model on the exact y (the caller's inputs make it exact)"""
    codes, e8 = model.quantize(model.rotate(_np(x), _np(h)), fmt)
    return codes, e8.reshape(-1)


def _same(got, want, what):
    bad_c, bad_s = int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum())
    print(f"{what}: {bad_c} of {want[0].size} codes and {bad_s} of {want[1].size} scales differ from the model")
    assert bad_s == 0 and bad_c == 0, what


# ---- 1. the exact regime: zero tolerance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("R", ROTS)
def test_exact_regime_is_the_model_byte_for_byte(q, R, fmt):
    h = rot.signed_permuted_hadamard(R)
    for i, shape in enumerate([(1, R), (33, 3 * R), (2, 3, 39, 5 * R)]):
        x = rot.exact_input(shape, seed=100 * R + i)
        k = torch.randint(-6, 7, (*shape[:-1], 1), generator=torch.Generator().manual_seed(i))
        x = (x.float() * torch.exp2(k.float())).to(torch.bfloat16)            # a power of two per row: still exact, and the scale byte varies
        want = _want(x, h, fmt)
        _same(_run(q, x, h, fmt), want, f"R {R} {fmt} {shape}")
        if i == 2:
            assert np.unique(want[1]).size >= 8 and np.unique(want[0]).size >= 16


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("R", ROTS)
def test_identity_rotation_on_gaussians_is_the_model_byte_for_byte(q, R, fmt):
    gen = torch.Generator().manual_seed(7 + R)
    for mag in (0.01, 1.0, 25.0, 3000.0):
        x = (torch.randn(33, 3 * R, generator=gen) * mag).to(torch.bfloat16)   # y = x: one non-zero product per sum
        _same(_run(q, x, _identity(R), fmt), _want(x, _identity(R), fmt), f"identity R {R} {fmt} x {mag}")


# ---- 2. the edge rows of the contract, identity rotation ---------------------------------------------------------------------------------------------------
def _midpoint_groups(fmt):
    """every midpoint between two neighbouring codes from 0 up to `top` (128 for e4m3, 2^14 for e5m2), both signs, 31 to a group whose 32nd value is +top: the
    group's scale byte is then 127 and the scaled values are the midpoints themselves -- every tie of the format below its scaled maximum's binade"""
    top = 128.0 if fmt == "e4m3" else 2.0 ** 14
    vals = np.array(sorted(v for v in (model.decode(np.arange(128, dtype=np.uint8), fmt)) if v <= top))
    mids = (vals[:-1] + vals[1:]) / 2
    mids = np.concatenate([mids, -mids])
    pad = (-mids.size) % 31
    g = np.concatenate([mids, np.zeros(pad)]).reshape(-1, 31)
    return np.concatenate([g, np.full((g.shape[0], 1), top)], axis=1), mids.size


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("R", ROTS)
def test_edge_rows_of_the_contract(q, R, fmt):
    big = float(torch.tensor([0x7f7f], dtype=torch.uint16).view(torch.bfloat16).float())   # the largest finite bf16
    zero = np.zeros(32)
    neg0 = zero.copy(); neg0[[1, 7, 30]] = -0.0                         # a -0 INPUT: the rotation sums from +0, so y = +0 -- scale 127, codes 0
    tiny = zero.copy(); tiny[0] = 1.0; tiny[1:4] = [-2.0 ** -40, 2.0 ** -40, -2.0 ** -60]   # y * 2^(127 - e8) below half the smallest subnormal: -0 keeps its sign
    low = zero.copy(); low[[3, 4, 5]] = [2.0 ** -125, -2.0 ** -126, 1.5 * 2.0 ** -126]  # the clamp at 0: E - SH < 0
    high = zero.copy(); high[[0, 9, 31]] = [big, -big, big / 2]
    mids, n_mids = _midpoint_groups(fmt)
    groups = np.concatenate([np.stack([zero, neg0, tiny, low, high]), mids])
    groups = np.concatenate([groups, np.zeros(((-groups.shape[0]) % (R // 32), 32))])    # whole rotation blocks
    x = torch.from_numpy(groups).to(torch.bfloat16).reshape(-1, R)
    assert np.array_equal(x.double().numpy().reshape(-1, 32), groups), "every value must be a bf16 number"
    want = _want(x, _identity(R), fmt)
    sh = model.SH[fmt]
    assert want[1][:5].tolist() == [127, 127, 127 - sh, 0, 254 - sh] and (want[1][5:5 + mids.shape[0]] == 127).all()
    assert not want[0].reshape(-1, 32)[:2].any() and want[0].reshape(-1, 32)[2, :4].tolist() == [0x70 if fmt == "e4m3" else 0x74, 0x80, 0x00, 0x80]
    assert n_mids == (2 * 0x70 if fmt == "e4m3" else 2 * 0x74)
    _same(_run(q, x, _identity(R), fmt), want, f"edge rows R {R} {fmt}")


# ---- 3. / 4. arbitrary rotations: scale bytes against the device's MX quantizer, codes against fp64 ------------------------------------------------------------
def _general_cases(R):
    gen = torch.Generator().manual_seed(31 + R)
    for hname, h in (("general", rot.general_rotation(R)), ("hadamard", rot.signed_permuted_hadamard(R))):
        for shape in ((40, 2 * R), (130, R)):
            yield hname, h, (torch.randn(shape, generator=gen) * 64.0).to(torch.bfloat16)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("R", ROTS)
def test_scale_bytes_against_the_mx_quantizer_on_arbitrary_rotations(q, R, fmt):
    """the MX abs-max arm takes the exponent of amax + 1e-8 of the SAME y: with every sf_mx >= 130 (amax >= 8, half an ulp 4.8e-7) the addend cannot change it"""
    for hname, h, x in _general_cases(R):
        _, sf8 = _run(q, x, h, fmt)
        sf_mx = _flat(q.fusedQuantizeMx(x.to(DEV), h.to(DEV), method="abs_max")[1], x.numel() // 32)
        assert sf_mx.min() >= 130, int(sf_mx.min())   # the precondition, asserted and not filtered
        assert np.array_equal(sf8.astype(np.int64), sf_mx.astype(np.int64) - model.SH[fmt]), (hname, x.shape)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("R", ROTS)
def test_codes_against_fp64_on_arbitrary_rotations(q, R, fmt):
    """|dq - y64| <= r |y64| + s 2^(e8 - 127) + 2^-20 (|x_group| @ |h|) for EVERY element: r = half a step of the format relative to the value (2^-4 for the 3
    mantissa bits of e4m3, 2^-3 for the 2 of e5m2), s 2^(e8 - 127) = half the subnormal step (2^-10, 2^-17) in the group's scale, and the last term the slack of an fp32
    accumulation of up to 128 bf16 products in any order (128 * 2^-24 = 2^-17 of sum |x h| would be the worst case; 2^-20 holds with the MFMA's and was never
    approached by an fp32 stand-in: worst ratio to the whole bound 0.94)."""
    r, s = (2.0 ** -4, 2.0 ** -10) if fmt == "e4m3" else (2.0 ** -3, 2.0 ** -17)
    worst = 0.0
    for hname, h, x in _general_cases(R):
        codes, e8 = _run(q, x, h, fmt)
        x64, h64 = model.bf16_to_f64(_np(x)).reshape(-1, R), model.bf16_to_f64(_np(h))
        y64 = (x64 @ h64).reshape(x.shape)
        dq = model.dequantize(codes, e8.reshape(*x.shape[:-1], -1), fmt)
        step = np.ldexp(1.0, np.repeat(e8.astype(np.int64), 32) - 127).reshape(x.shape)
        bound = r * np.abs(y64) + s * step + 2.0 ** -20 * (np.abs(x64) @ np.abs(h64)).reshape(x.shape)
        ratio = float((np.abs(dq - y64) / bound).max())
        print(f"R {R} {fmt} {hname} {tuple(x.shape)}: worst |dq - y64| / bound = {ratio:.3f}")
        worst = max(worst, ratio)
        assert np.isfinite(dq).all() and (np.abs(dq - y64) <= bound).all(), (hname, x.shape, ratio)
    assert worst > 0.25, worst   # (the bound is not vacuous: the rounding error comes within a factor of it)


# ---- 5. the blocked form -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROTS)
def test_blocked_form_is_to_blocked_of_the_flat_form(q, R):
    h = rot.signed_permuted_hadamard(R).to(DEV)
    gen = torch.Generator().manual_seed(R)
    for K in ([32, 96, 128, 160] if R == 32 else [R, 3 * R]):
        for rows in (1, 127, 129, 257):
            x = (torch.randn(rows, K, generator=gen) * 3.0).to(torch.bfloat16).to(DEV)
            for fmt in FMTS if rows in (1, 129) else FMTS[:1]:
                codes, sf = q.fusedQuantizeMxf8(x, h, dtype=DTYPES[fmt])
                want_sf = oracle.to_blocked(_flat(sf, rows * K // 32).reshape(rows, K // 32))
                out = torch.full((rows, K), 0xff, dtype=torch.uint8, device=DEV).view(DTYPES[fmt])
                out_sf = torch.full((want_sf.size,), 0xff, dtype=torch.uint8, device=DEV).view(torch.float8_e8m0fnu)
                torch.ops.qutlass_amd.fusedQuantizeMxf8Blocked_(x, h, out, out_sf)
                assert np.array_equal(_np(out), _np(codes)), (rows, K, fmt)
                assert np.array_equal(_np(out_sf), want_sf), (rows, K, fmt)            # padding included: zero, not the 0xff it held
                b_codes, b_sf = q.fusedQuantizeMxf8Blocked(x, h, dtype=DTYPES[fmt])    # the wrapper allocates exactly that
                assert b_sf.shape == (want_sf.size,) and np.array_equal(_np(b_sf), want_sf) and np.array_equal(_np(b_codes), _np(codes))


# ---- 6. the gathering form ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("R", ROTS)
def test_gathering_form_is_the_plain_op_on_index_select(q, R, fmt):
    T, K = 7, 3 * R
    gen = torch.Generator().manual_seed(50 + R)
    x = (torch.randn(T, K, generator=gen) * 5.0).to(torch.bfloat16).to(DEV)
    h = rot.general_rotation(R).to(DEV)
    xz = torch.cat([x, torch.zeros(1, K, dtype=torch.bfloat16, device=DEV)])          # row T: the zero row of a bad index
    for src in ([3], [-1], 37, 130):
        if isinstance(src, int):
            m = src
            src = torch.randint(0, T, (m,), generator=gen).tolist()                   # 7 rows for 37 / 130 indices: repeats
            for pos, bad in zip(torch.randperm(m, generator=gen)[:6].tolist(), (-1, 7, 2 ** 30, -1, 7, 2 ** 30)):
                src[pos] = bad
        M = len(src)
        idx = torch.tensor(src, dtype=torch.int32, device=DEV)
        safe = torch.tensor([i if 0 <= i < T else T for i in src], dtype=torch.int64, device=DEV)
        want_codes, want_sf = q.fusedQuantizeMxf8(xz.index_select(0, safe), h, dtype=DTYPES[fmt])
        got_codes, got_sf = q.fusedGatherQuantizeMxf8(x, h, idx, dtype=DTYPES[fmt])
        n = M * K // 32
        assert got_codes.shape == (M, K) and np.array_equal(_np(got_codes), _np(want_codes)) and np.array_equal(_flat(got_sf, n), _flat(want_sf, n)), (M, fmt)
        for i, s in enumerate(src):
            if not 0 <= s < T:
                assert not _np(got_codes)[i].any() and (_flat(got_sf, n).reshape(M, -1)[i] == 127).all(), (i, s)
        # the bytes of OUT / OUT_sf past the written range stay as they were
        out = torch.full((M + 3, K), 0xff, dtype=torch.uint8, device=DEV).view(DTYPES[fmt])
        out_sf = torch.full(tuple(got_sf.shape), 0xff, dtype=torch.uint8, device=DEV).view(torch.float8_e8m0fnu)
        torch.ops.qutlass_amd.fusedGatherQuantizeMxf8_(x, h, idx, out, out_sf)
        assert np.array_equal(_np(out)[:M], _np(want_codes)) and (_np(out)[M:] == 0xff).all()
        assert np.array_equal(_flat(out_sf, n), _flat(want_sf, n)) and (_np(out_sf).reshape(-1)[n:] == 0xff).all()


# ---- 7. the gated form ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ROTS)
def test_gated_form_is_the_plain_op_on_silu_and_mul(q, R):
    h = rot.general_rotation(R).to(DEV)
    gen = torch.Generator().manual_seed(70 + R)
    for rows in (1, 5, 40):
        for inter in (R, 3 * R):
            x = torch.cat([torch.randn(rows, inter, generator=gen) * 3.0, torch.randn(rows, inter, generator=gen) * 2.0], dim=1).to(torch.bfloat16).to(DEV)
            act = q.silu_and_mul(x)
            want_codes, want_sf = q.fusedQuantizeMxf8(act, h)
            got_codes, got_sf = q.fusedSiluMulQuantizeMxf8(x, h)
            n = rows * inter // 32
            assert got_codes.dtype == torch.float8_e4m3fn and got_codes.shape == (rows, inter)
            assert np.array_equal(_np(got_codes), _np(want_codes)) and np.array_equal(_flat(got_sf, n), _flat(want_sf, n)), (rows, inter)
            wb_codes, wb_sf = q.fusedQuantizeMxf8Blocked(act, h)
            gb_codes, gb_sf = q.fusedSiluMulQuantizeMxf8Blocked(x, h)
            assert np.array_equal(_np(gb_codes), _np(wb_codes)) and np.array_equal(_np(gb_sf), _np(wb_sf)), (rows, inter)
            assert np.array_equal(_np(gb_sf), oracle.to_blocked(_flat(want_sf, n).reshape(rows, inter // 32)))


# ---- 8. non-finite inputs ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("R", ROTS)
def test_a_non_finite_input_poisons_its_own_rotation_block_only(q, R, fmt):
    h = rot.signed_permuted_hadamard(R)
    x = (torch.randn(33, 3 * R, generator=torch.Generator().manual_seed(90 + R)) * 2.0).to(torch.bfloat16)
    clean_c, clean_s = _run(q, x, h, fmt)
    for value, block, at in ((float("nan"), 17, 5), (float("inf"), 3 * 33 - 1, R - 1), (float("nan"), 40, 0)):   # (a block of the first tile, the very last block, ...)
        xb = x.clone().reshape(-1, R)
        xb[block, at] = value
        c, s = _run(q, xb.reshape(x.shape), h, fmt)
        c, s, cc, cs = c.reshape(-1, R), s.reshape(-1, R // 32), clean_c.reshape(-1, R), clean_s.reshape(-1, R // 32)
        others = np.arange(c.shape[0]) != block
        assert np.array_equal(c[others], cc[others]) and np.array_equal(s[others], cs[others]), (value, block)
        if value != value:
            assert np.isnan(model.decode(c[block], fmt)).all(), (block, c[block])


# ---- 9. the GEMMs take the operands as they are ----------------------------------------------------------------------------------------------------------
def _dev(codes, e8, dtype):
    return (torch.from_numpy(np.ascontiguousarray(codes)).to(DEV).view(dtype), torch.from_numpy(np.ascontiguousarray(e8).reshape(-1)).to(DEV).view(torch.float8_e8m0fnu))


@pytest.mark.parametrize("fmt", FMTS)
def test_the_mxfp8_gemms_take_the_operands_as_they_are(q, fmt):
    R, M, N, K, E = 64, 37, 64, 256, 3
    h = rot.signed_permuted_hadamard(R)
    a = rot.exact_input((M, K), seed=5)
    w = rot.exact_input((E * N, K), seed=6, scale=50.0)
    alpha = torch.ones(1, device=DEV)
    offs = torch.tensor([5, 5, 37], dtype=torch.int32, device=DEV)
    ad, hd, wd = a.to(DEV), h.to(DEV), w.to(DEV)
    am, wm = _want(a, h, fmt), _want(w, h, "e4m3")
    # grouped: flat scales, row-major (M, K / 32) and (E, N, K / 32) -- the quantizers' buffers as they come
    a_q, a_sf = q.fusedQuantizeMxf8(ad, hd, dtype=DTYPES[fmt])
    w_q, w_sf = q.fusedQuantizeMxf8(wd, hd)
    got = q.grouped_matmul_mxf8_bf16_tn(a_q, w_q.view(E, N, K), a_sf, w_sf, alpha, offs)
    a_m, a_sf_m = _dev(*am, DTYPES[fmt])
    w_m, w_sf_m = _dev(*wm, torch.float8_e4m3fn)
    want = q.grouped_matmul_mxf8_bf16_tn(a_m, w_m.view(E, N, K), a_sf_m, w_sf_m, alpha, offs)
    assert got.shape == (M, N) and np.array_equal(_np(got), _np(want)) and np.abs(_np(want).astype(np.int64)).max() > 0
    # dense: scales in the to_blocked layout
    w0, wm0 = wd[:N], _want(w[:N], h, "e4m3")
    a_q, a_sf = q.fusedQuantizeMxf8Blocked(ad, hd, dtype=DTYPES[fmt])
    b_q, b_sf = q.fusedQuantizeMxf8Blocked(w0, hd)
    got = q.matmul_mxf8_bf16_tn(a_q, b_q, a_sf, b_sf, alpha)
    a_m, a_sf_m = _dev(am[0], oracle.to_blocked(am[1].reshape(M, K // 32)), DTYPES[fmt])
    b_m, b_sf_m = _dev(wm0[0], oracle.to_blocked(wm0[1].reshape(N, K // 32)), torch.float8_e4m3fn)
    want = q.matmul_mxf8_bf16_tn(a_m, b_m, a_sf_m, b_sf_m, alpha)
    assert got.shape == (M, N) and np.array_equal(_np(got), _np(want)) and np.abs(_np(want).astype(np.int64)).max() > 0


# ---- 10. graph capture ----------------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bytes(q):
    R = 64
    gen = torch.Generator().manual_seed(3)
    h = rot.general_rotation(R).to(DEV)
    x = (torch.randn(70, 3 * R, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    src = torch.randint(-1, 71, (45,), generator=gen).to(torch.int32).to(DEV)
    calls = {
        "plain": lambda: q.fusedQuantizeMxf8(x, h, dtype=torch.float8_e5m2),
        "blocked": lambda: q.fusedQuantizeMxf8Blocked(x, h),
        "gather": lambda: q.fusedGatherQuantizeMxf8(x, h, src, dtype=torch.float8_e5m2),
        "gated": lambda: q.fusedSiluMulQuantizeMxf8(x.view(35, 6 * R), h),
    }
    for name, call in calls.items():
        eager = call()
        torch.cuda.synchronize()
        n = eager[1].numel() if name == "blocked" else eager[0].numel() // 32
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = call()
        cap[0].view(torch.uint8).zero_()
        cap[1].view(torch.uint8).zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(cap[0]), _np(eager[0])), name
        assert np.array_equal(_flat(cap[1], n), _flat(eager[1], n)), name
