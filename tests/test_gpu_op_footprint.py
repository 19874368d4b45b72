"""GPU: the write and read footprint, and the content, of every op outside the GEMMs (include/qutlass_amd.h states a footprint contract for each; the GEMMs' is pinned
by tests/test_gpu_gemm_footprint.py).  Harness: tests/_footprint.py -- every operand and result is a view of one arena with 64 KiB bands, every case runs twice on
identical inputs under two different fills; inside a result's contractual extent the runs must agree byte for byte and equal the op's model, everywhere else the fill
must survive, and the inputs must be unchanged.  The CPU half (the checker can fail, the extents, the shapes) is tests/test_op_footprint_cpu.py.

Ops of the README table outside the GEMMs, and the test that holds each:
  fusedQuantizeMx / Nv [+ clip mask], fusedQuantizeMxBlocked / NvBlocked, fusedSiluMulQuantizeMx / Nv [Blocked], fusedGatherQuantizeMx / Nv,
  fusedGatherQuantizeNvGrouped, fusedSiluMulQuantizeNvGrouped, fusedQuantizeMxf8 [Blocked], fusedGatherQuantizeMxf8, fusedSiluMulQuantizeMxf8 [Blocked],
  fusedSwigluOaiQuantizeMx                                   test_quantizer_family (the 16 rows of QUANT_OPS + fusedQuantizeMxMask_), test_grid_stride_trip
  silu_and_mul, swiglu_oai_and_mul                           test_streaming_activations
  moe_combine, moe_combine(bias=, offs=)                     test_moe_combine
  moe_topk_softmax, moe_topk_grouped                         test_moe_topk_softmax, test_moe_topk_grouped
  moe_sort_fused                                             test_moe_sort
  to_blocked                                                 test_to_blocked
  backward_t_bf16, backward_qt_bf16, backward_bf16_square_double_mxfp8, mxfp4_transpose_mxfp8      test_backward_t_qt, test_backward_rows
  fused_quantize_matmul_mxf4_bf16_tn (one launch)            test_one_launch_decode_layer
moe_route / moe_route_grouped are compositions of the routing ops above, moe_sort is torch, utils.split_interleaved_gate_up is torch: no kernel of their own.

Models (each the one of the op's existing GPU test, tolerance zero in the exact regime): oracle.fused_quantize_mx / _nv under acc_model = 1 with
codes_equal_mod_zero_sign on rot.exact_input and rot.signed_permuted_hadamard, gate = 100 for the SiLU forms (tests/test_gpu_rotation_orientation.py); the clamped SwiGLU
on gate = 100, integer ups and integer biases through tests/_swiglu_oai_model.py; tests/_mxf8_quant_model.py; oracle.to_blocked, oracle.backward_*; the numpy selection
models of the two routing tests; _sort_ref and _combine_ref of tests/test_gpu_moe_route.py / test_gpu_moe_dispatch.py.  Bounds that are not zero are the existing tests'
own: the routers' weights and scores (tests/test_gpu_moe_route.py: (E + 64) 2^-24; tests/test_gpu_moe_route_grouped.py: (topk + 4) 2^-24, 8 2^-24),
backward_qt_bf16's codes (tests/test_gpu_round4.py: 1e-4 of them modulo the sign of zero), the decode layer (tests/test_gpu_rotation_orientation.py: 1e-2 max |want|).

Left out, with the reason: backward_qt_bf16 takes M % 32 == 0, so its second shape is (2, 96, 96) where backward_t_bf16 runs (2, 96, 72).  The lab switch of the two
`_rows` ops is "transpose_nc" (tests/test_gpu_round4.py forces their kernels with it; "bwd_variant" selects among the backward_t / backward_qt kernels only); its
1024-column form of square_double needs n % 1024 == 0 and takes none of the shapes here.  The grid-stride cases keep R = 128 for all four kinds (the oracle takes
about a second per case).

Wall time of this file on an MI355X: 220 tests in 4.2 s (the whole file, oracle included; the slowest case is the MXFP8 grid-stride trip at R = 128 with 0.28 s).
"""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
import _footprint as fp  # noqa: E402
import _mxf8_quant_model as m8  # noqa: E402
import _rotations as rot  # noqa: E402
import _swiglu_oai_model as oai  # noqa: E402
from _rotations import bits as _np  # noqa: E402
from test_gpu_gated_quantize import _ref_act  # noqa: E402
from test_gpu_moe_dispatch import _combine_ref  # noqa: E402
from test_gpu_moe_route import _sort_ref  # noqa: E402
from test_moe_route_grouped_cpu import grouped_topk_ref  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
GS = 2.3                       # an NV global scale that is no power of two
ALPHA, LIMIT = 1.702, 7.0      # gpt-oss
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
BF16, I32, F32, U8 = torch.bfloat16, torch.int32, torch.float32, torch.uint8


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    qutlass_amd.ops.register_torch_ops()
    return qutlass_amd


def _empty(dtype):
    """the in-place ops' "no tensor" """
    return torch.empty(0, dtype=dtype, device=DEV)


def _codes_equal(got, want, fp8, ctx):
    if fp8:
        assert np.array_equal(got, want.reshape(-1)), (ctx, "codes", int((got != want.reshape(-1)).sum()), got.size)
    else:
        eq = oracle.codes_equal_mod_zero_sign(got, want.reshape(-1))
        assert eq.all(), (ctx, "codes", int((~eq).sum()), eq.size)


# ------------------------------------------------------------------------------------------------
# 1. the rotate-and-quantize family
# ------------------------------------------------------------------------------------------------
ROTS = {"mx": (32, 64, 128), "nv": (16, 32, 64, 128), "mxf8": (32, 64, 128)}
MXF8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def _family():
    from qutlass_amd.ops import QUANT_OPS

    out = []
    for name, row in QUANT_OPS.items():
        if name == "swiglu_oai_quantize_mxf8":   # its footprint test is tests/test_gpu_swiglu_oai_mxf8.py::test_footprint
            continue
        rots = (32, 64) if name == "swiglu_oai_quantize_mx" else ROTS[row.fmt]
        hows = (("e4m3",) if name == "silu_mul_quantize_mxf8" else tuple(MXF8)) if row.fmt == "mxf8" else (0, 1)   # the MXFP8 code dtype, or the method
        out += [(name, R, how) for R in rots for how in hows]
    return out + [("quantize_mx_mask", 32, 0)]


def _variants(name):
    """the inner cases of one (op, R, how): dicts of rows / blocked / bad (out-of-range indices) / e65 (the 65-expert offs)"""
    from qutlass_amd.ops import QUANT_OPS, _gathered

    row = QUANT_OPS.get(name)
    if row is not None and row.operand is _gathered:
        if "grouped" in name:
            return [dict(e65=False), dict(e65=True)]
        return [dict(bad=False), dict(bad=True)]
    if name == "silu_mul_quantize_nv_grouped":
        return [dict(rows=fp.M_ROWS, e65=False), dict(rows=fp.M_ROWS, e65=True)]
    if name == "swiglu_oai_quantize_mx":
        return [dict(rows=r) for r in fp.ROWS] + [dict(rows=fp.M_ROWS, bias=True, e65=False), dict(rows=fp.M_ROWS, bias=True, e65=True)]
    blocked = [False, True] if row is not None and row.blocked is None else [bool(row is not None and row.blocked)]
    return [dict(rows=r, blocked=b) for b in blocked for r in (fp.BLOCKED_ROWS if b else fp.ROWS)]


def _groups(e65: bool):
    counts = fp.counts_e65() if e65 else np.array(fp.COUNTS)
    assert counts.sum() == fp.M_ROWS
    scales = (0.37 + 0.1371 * np.arange(len(counts))).astype(np.float32)      # pairwise different, none a power of two
    assert len(np.unique(scales)) == len(scales) and ((scales.view(np.uint32) & 0x7fffff) != 0).all()
    return counts, np.cumsum(counts).astype(np.int32), scales


def _int_bias(E, inter, seed):
    """per-expert gate / up biases that keep the clamped SwiGLU in the exact regime: gate + 0 .. 3 stays above the limit, up + (-1 .. 1) stays a small integer; rows
    pairwise different"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    b = torch.cat([torch.randint(0, 4, (E, inter), generator=gen), torch.randint(-1, 2, (E, inter), generator=gen)], dim=1).to(BF16)
    assert len({r.numpy().tobytes() for r in b.view(torch.int16)}) == E
    return b


def _quant_case(name, R, how, v, lab_call=None, shape=None):
    """-> (layout, call(arena), verify(results)) of one case of the family.  lab_call / shape: the grid-stride cases (section 2)."""
    from qutlass_amd.ops import QUANT_FORMATS, QUANT_OPS, _act, _gathered

    mask = name == "quantize_mx_mask"
    row = QUANT_OPS["quantize_mx" if mask else name]
    fmt, fp8 = row.fmt, row.fmt == "mxf8"
    group, sf_dtype = QUANT_FORMATS[fmt]
    k = 3 * fp.rp(R) if shape is None else shape[1]
    rows = v.get("rows", fp.M_ROWS) if shape is None else shape[0]
    blocked = bool(v.get("blocked", False))
    method = 0 if fp8 else how
    h = rot.signed_permuted_hadamard(R, seed=1)
    hb = _np(h)
    seed = 7 * R + rows + 1000 * blocked
    lay = fp.Layout()
    ctx = (name, R, how, tuple(sorted(v.items())))
    counts = offs = scales = bias = None
    if v.get("e65") is not None:
        counts, offs, scales = _groups(v["e65"])
    if row.operand is _gathered:
        T = fp.T_TOK if shape is None else 4099
        x = rot.exact_input((T, k), seed=seed)
        src = torch.randint(0, T, (rows,), generator=torch.Generator(device="cpu").manual_seed(R), dtype=I32)
        assert len(set(src.tolist())) < rows   # repeats
        if v.get("bad"):
            src[3], src[40] = -1, T            # the header: an index outside [0, t) gives the bytes of an all-zero row
        ok = (src >= 0) & (src < T)
        bits = np.where(ok.numpy()[:, None], _np(x)[src.clamp(0, T - 1).numpy()], np.uint16(0))
        lay.input("A", x).input("R", h).input("src_row", src)
        a_shape = (T, k)
    elif row.operand is _act:
        up = rot.exact_input((rows, k), seed=seed, scale=1.0)
        x = torch.cat([torch.full((rows, k), 100.0, dtype=BF16), up], dim=1)      # silu(100) == 100 in bf16; the clamped gate is 7
        if name == "swiglu_oai_quantize_mx":
            if v.get("bias"):
                bias = _int_bias(len(counts), k, seed)
            bits = oai.swiglu_oai(_np(x), ALPHA, LIMIT, None if bias is None else _np(bias), offs if bias is not None else None)
            assert set(np.unique(oai.bf16_to_f32(bits))) <= {7.0 * i for i in range(-2, 5)}
        else:
            bits = _ref_act(_np(x))
            assert np.array_equal(bits, _np((up.float() * 100.0).to(BF16)))
        lay.input("A", x).input("R", h)
        a_shape = (rows, 2 * k)
    else:
        x = rot.exact_input((rows, k), seed=seed)
        bits = _np(x)
        lay.input("A", x).input("R", h)
        a_shape = (rows, k)
    if fmt == "nv":
        lay.input("gscale", torch.from_numpy(scales) if scales is not None else torch.tensor([GS]))
    if bias is not None:
        lay.input("bias", bias)
    if offs is not None and (fmt == "nv" or bias is not None):
        lay.input("offs", torch.from_numpy(offs))
    ext = fp.quant_extents(fmt, (rows, k), blocked, fp8)
    for nm, (nbytes, extent) in ext.items():
        lay.output(nm, nbytes, extent)
    if mask:
        lay.output("OUT_mask", fp.mask_bytes(rows * k))

    def call(a):
        if lab_call is not None:
            return lab_call(a, rows, k, R, method if not fp8 else list(MXF8).index(how))
        lead = [a.t("A", BF16, *a_shape), a.t("R", BF16, R, R)] + ([a.t("src_row", I32)] if row.operand is _gathered else [])
        out = [a.t("OUT", MXF8[how] if fp8 else U8), a.t("OUT_sf", sf_dtype)]
        if mask:
            rest = [a.t("OUT_mask", U8)]
        elif name == "swiglu_oai_quantize_mx":
            rest = [ALPHA, LIMIT, a.t("bias", BF16, len(counts), 2 * k) if bias is not None else _empty(BF16), a.t("offs", I32) if bias is not None else _empty(I32), method]
        else:
            rest = ([a.t("gscale", F32)] if fmt == "nv" else []) + ([a.t("offs", I32)] if "grouped" in name else []) + ([] if fp8 else [method])
            rest += [blocked] if row.blocked is None else []
        getattr(torch.ops.qutlass_amd, "fusedQuantizeMxMask_" if mask else row.twin)(*lead, *out, *rest)

    def verify(res):
        om = oracle.QUEST if method == 0 else oracle.ABS_MAX
        want_mask = None
        if fp8:
            wq, ws = m8.quantize(m8.rotate(bits, hb), how)
        elif fmt == "mx":
            wq, ws, want_mask = oracle.fused_quantize_mx(bits, hb, om, with_mask=mask, acc_model=1)
        elif scales is None:
            wq, ws = oracle.fused_quantize_nv(bits, hb, GS, om, acc_model=1)
        else:   # the bytes of row r are those of the single-scale entry called with global_scales[g(r)]
            g = oai.group_of_rows(offs, np.arange(rows))
            wq, ws = np.empty((rows, k // 2), np.uint8), np.empty((rows, k // 16), np.uint8)
            for e in np.unique(g):
                cq, cs = oracle.fused_quantize_nv(bits[g == e], hb, float(scales[e]), om, acc_model=1)
                wq[g == e], ws[g == e] = cq.reshape(-1, k // 2), cs.reshape(-1, k // 16)
        ws = np.ascontiguousarray(ws).reshape(-1)
        if blocked:
            ws = oracle.to_blocked(ws.reshape(rows, k // group))          # padding: zero
        assert np.array_equal(res["OUT_sf"], ws), (ctx, "scales", int((res["OUT_sf"] != ws).sum()), ws.size)
        _codes_equal(res["OUT"], np.ascontiguousarray(wq), fp8, ctx)
        if mask:
            assert np.array_equal(res["OUT_mask"], want_mask), (ctx, "clip mask")

    return lay, call, verify


@pytest.mark.parametrize("name,R,how", _family(), ids=lambda p: str(p))
def test_quantizer_family(q, name, R, how):
    """every row of QUANT_OPS and the clip-mask form, through the in-place twins on arena views: rows 1 / 33 / 70 (a last tile of 3 or 18 RP-rows, idle waves in the last
    workgroup) with K = 3 max(R, 32) (scale columns no multiple of 4), 130 rows for the blocked forms, 53 gathered rows with repeats and with a -1 and a T entry, the
    per-expert forms with 5 and with 65 experts"""
    for v in _variants(name):
        lay, call, verify = _quant_case(name, R, how, v)
        verify(fp.run_twice(lay, call, DEV))


@pytest.mark.parametrize("oai_form,inter", [(o, i) for o in (False, True) for i in (96, 104, 192, 384)], ids=str)
def test_streaming_activations(q, oai_form, inter):
    """siluAndMul_ (gate = 100: the exact regime of tests/test_gpu_gated_quantize.py) and swigluOaiAndMul_ (random data: tests/test_gpu_swiglu_oai.py holds it to the
    model bit for bit), without a bias at rows 1 / 33 / 70 and, the clamped form, with the bias of 5 and of 65 experts at 53 rows"""
    cases = [dict(rows=r) for r in fp.ROWS] + ([dict(rows=fp.M_ROWS, e65=False), dict(rows=fp.M_ROWS, e65=True)] if oai_form else [])
    for v in cases:
        rows = v["rows"]
        gen = torch.Generator(device="cpu").manual_seed(rows * 31 + inter)
        lay = fp.Layout()
        bias = offs = None
        if oai_form:
            x = torch.cat([torch.randn(rows, inter, generator=gen) * 3.0, torch.randn(rows, inter, generator=gen) * 2.0], dim=1).to(BF16)
            if "e65" in v:
                counts, offs, _ = _groups(v["e65"])
                bias = (torch.randn(len(counts), 2 * inter, generator=gen) * 2.0).to(BF16)
            want = oai.swiglu_oai(_np(x), ALPHA, LIMIT, None if bias is None else _np(bias), offs)
        else:
            x = torch.cat([torch.full((rows, inter), 100.0, dtype=BF16), rot.exact_input((rows, inter), seed=rows + inter, scale=1.0)], dim=1)
            want = _ref_act(_np(x))
        lay.input("X", x)
        if bias is not None:
            lay.input("bias", bias).input("offs", torch.from_numpy(offs))
        lay.output("OUT", rows * inter * 2)

        def call(a):
            X, OUT = a.t("X", BF16, rows, 2 * inter), a.t("OUT", BF16, rows, inter)
            if not oai_form:
                torch.ops.qutlass_amd.siluAndMul_(X, OUT)
            elif bias is None:
                torch.ops.qutlass_amd.swigluOaiAndMul_(X, OUT, ALPHA, LIMIT, _empty(BF16), _empty(I32))
            else:
                torch.ops.qutlass_amd.swigluOaiAndMul_(X, OUT, ALPHA, LIMIT, a.t("bias", BF16, bias.size(0), 2 * inter), a.t("offs", I32))

        got = fp.run_twice(lay, call, DEV)["OUT"].view(np.uint16).reshape(rows, inter)
        assert np.array_equal(got, want), (oai_form, inter, v, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------
# 2. the grid-stride trip: more tiles than waves, through the lab library with one workgroup per CU
# ------------------------------------------------------------------------------------------------
def _lab_quant(kind):
    lib = fp.cabi(lab=True)

    def call(a, rows, k, R, how):
        s = fp.stream()
        if kind == "plain":
            rc = lib.qutlass_amd_fused_quantize_mx(a.ptr("A"), a.ptr("R"), R, rows * k, how, a.ptr("OUT"), a.ptr("OUT_sf"), None, s)
        elif kind == "gated":
            rc = lib.qutlass_amd_fused_silu_mul_quantize_mx(a.ptr("A"), a.ptr("R"), R, rows, k, how, 0, a.ptr("OUT"), a.ptr("OUT_sf"), s)
        elif kind == "gather":
            t = a.layout.views["A"].nbytes // (2 * k)
            rc = lib.qutlass_amd_fused_gather_quantize_mx(a.ptr("A"), a.ptr("R"), R, t, k, a.ptr("src_row"), rows, how, a.ptr("OUT"), a.ptr("OUT_sf"), s)
        else:
            rc = lib.qutlass_amd_fused_quantize_mxf8(a.ptr("A"), a.ptr("R"), R, rows * k, how, a.ptr("OUT"), a.ptr("OUT_sf"), s)
        fp.ok(lib, rc)
    return call


GRID_KINDS = {"plain": ("quantize_mx", 1), "gated": ("silu_mul_quantize_mx", 0), "gather": ("gather_quantize_mx", 1), "mxf8": ("quantize_mxf8", "e4m3")}


@pytest.mark.parametrize("R", [32, 128])
@pytest.mark.parametrize("kind", list(GRID_KINDS))
def test_grid_stride_trip(q, kind, R):
    """ntiles = 4 CUs + 5 under lab.forced(quant_wg_per_cu=1): a grid of one workgroup per CU, every wave walks a tile and five of them a second one, the last tile
    partial (tests/test_op_footprint_cpu.py checks the arithmetic).  Inputs of about 8 MiB at R = 128 (16 MiB for the gated kind: [gate | up])."""
    import _benchlib as lab

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows, k = fp.grid_stride_shape(R, cus)
    launch = fp.quant_launch(rows * k, R, cus, wg_per_cu=1)
    assert launch.ntiles == 4 * cus + 5 and launch.grid == cus and launch.second_trip == 5 and launch.last_rows < 32
    name, how = GRID_KINDS[kind]
    lay, call, verify = _quant_case(name, R, how, dict(), lab_call=_lab_quant(kind), shape=(rows, k))
    with lab.forced(quant_wg_per_cu=1):
        res = fp.run_twice(lay, call, DEV)
    verify(res)


# ------------------------------------------------------------------------------------------------
# 3. moe_combine, with and without the down bias
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("H", [64, 2944])
@pytest.mark.parametrize("topk", [1, 4])
@pytest.mark.parametrize("T", [1, 33])
def test_moe_combine(q, T, topk, H, with_bias):
    """pos holds -1 and M entries (both skipped: M would be the first row behind y), y has 5 rows no pos names; bit-equal to the spelled-out fp32 arithmetic
    (_combine_ref of tests/test_gpu_moe_dispatch.py, tests/_swiglu_oai_model.moe_combine_bias)"""
    gen = torch.Generator(device="cpu").manual_seed(T * 1009 + H * 13 + topk)
    M = T * topk + 5
    y = torch.randn(M, H, generator=gen).to(BF16)
    w = (torch.rand(T, topk, generator=gen) * 1.9 + 0.02).float()
    pos = (torch.randperm(M - 1, generator=gen)[: T * topk] + 1).view(T, topk).to(I32)
    if T * topk >= 4:                      # (a single slot stays a real row)
        pos.view(-1)[0::3] = -1
        pos.view(-1)[1::5] = M
        assert (pos == -1).any() and (pos == M).any() and ((pos >= 0) & (pos < M)).any()
    lay = fp.Layout().input("Y", y).input("pos", pos).input("weights", w)
    E = 5
    if with_bias:
        bias = (torch.randn(E, H, generator=gen) * 2.0).to(BF16)
        offs = np.cumsum([M // 2, 0, 1, M - M // 2 - 3, 1]).astype(np.int32)      # one row behind offs[-1]: expert E - 1's
        lay.input("bias", bias).input("offs", torch.from_numpy(offs))
        want = oai.moe_combine_bias(_np(y), pos.numpy(), w.numpy(), _np(bias), offs)
    else:
        want = _combine_ref(_np(y), pos.numpy(), w.numpy())
    lay.output("OUT", T * H * 2)

    def call(a):
        args = [a.t("Y", BF16, M, H), a.t("pos", I32, T, topk), a.t("weights", F32, T, topk)]
        if with_bias:
            torch.ops.qutlass_amd.moeCombineBias_(*args, a.t("bias", BF16, E, H), a.t("offs", I32), a.t("OUT", BF16, T, H))
        else:
            torch.ops.qutlass_amd.moeCombine_(*args, a.t("OUT", BF16, T, H))

    got = fp.run_twice(lay, call, DEV)["OUT"].view(np.uint16).reshape(T, H)
    assert np.array_equal(got, want), (int((got != want).sum()), want.size)


# ------------------------------------------------------------------------------------------------
# 4. the routers
# ------------------------------------------------------------------------------------------------
TOKENS = (1, 5, 67)
EXPERTS = (1, 63, 64, 65, 384, 1024)


def _logits(T, E, dtype, seed):
    """randn * 3, every second row on a grid of quarters (exact ties)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(T, E, generator=gen) * 3.0
    x[1::2] = torch.round(x[1::2] * 4.0) / 4.0
    return x.to(dtype)


def _f64(x):
    return x.float().numpy().astype(np.float64)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("E", EXPERTS)
def test_moe_topk_softmax(q, E, dtype):
    """ids: a stable argsort of the logits, exactly; weights within (E + 64) 2^-24 of the float64 softmax (the bound derived in tests/test_gpu_moe_route.py)"""
    for T in TOKENS:
        x = _logits(T, E, dtype, seed=E * 100 + T)
        x64 = _f64(x)
        e = np.exp(x64 - x64.max(axis=1, keepdims=True))
        p64 = e / e.sum(axis=1, keepdims=True)
        for topk in (k for k in (1, 8, 32) if k <= E):
            renorm = topk != 8
            lay = fp.Layout().input("logits", x).output("weights", T * topk * 4).output("ids", T * topk * 4)

            def call(a):
                torch.ops.qutlass_amd.moeTopkSoftmax_(a.t("logits", dtype, T, E), a.t("weights", F32, T, topk), a.t("ids", I32, T, topk), renorm)

            res = fp.run_twice(lay, call, DEV)
            ids, w = res["ids"].view(np.int32).reshape(T, topk), res["weights"].view(np.float32).reshape(T, topk).astype(np.float64)
            assert np.array_equal(ids, np.argsort(-x64, axis=1, kind="stable")[:, :topk]), (E, T, topk)
            w64 = np.take_along_axis(p64, ids.astype(np.int64), axis=1)
            w64 = w64 / w64.sum(axis=1, keepdims=True) if renorm else w64
            assert (np.abs(w - w64) <= (E + 64) * U * w64).all(), (E, T, topk, (np.abs(w - w64) / w64).max() / U)


def _grouped_configs(E):
    """(n_group, topk_group, scoring, bias, renormalize, scale, topks)"""
    G, tg = {64: (4, 2), 384: (8, 4), 1024: (64, 16)}.get(E, (1, 1))
    top = min(32, tg * (E // G), E)
    topks = [k for k in (1, 8, 32) if k <= top]
    return [(G, tg, "sigmoid", True, True, 2.5, topks), (G, tg, "softmax", False, False, 1.0, topks)]


PUBLISHED = [(256, 8, 4, 8, "sigmoid", True, True, 2.5), (384, 1, 1, 8, "sigmoid", True, True, 2.827), (160, 8, 3, 6, "softmax", False, False, 16.0)]   # DeepSeek-V3, Kimi-K2, DeepSeek-V2


def _run_grouped(T, E, dtype, topk, G, tg, scoring, with_bias, renorm, scale, seed):
    x = _logits(T, E, dtype, seed)
    bias = (torch.randint(-3, 4, (E,), generator=torch.Generator(device="cpu").manual_seed(seed + 1)).float() / 8.0) if with_bias else None
    got = {}
    for scores in (True, False):
        lay = fp.Layout().input("logits", x)
        if bias is not None:
            lay.input("bias", bias)
        lay.output("weights", T * topk * 4).output("ids", T * topk * 4)
        if scores:
            lay.output("scores", T * E * 4)

        def call(a):
            torch.ops.qutlass_amd.moeTopkGrouped_(a.t("logits", dtype, T, E), a.t("bias", F32) if bias is not None else _empty(F32), a.t("weights", F32, T, topk),
                                                  a.t("ids", I32, T, topk), a.t("scores", F32, T, E) if scores else _empty(F32), G, tg,
                                                  {"sigmoid": 0, "softmax": 1}[scoring], renorm, scale)

        got[scores] = fp.run_twice(lay, call, DEV)
    ctx = (T, E, topk, G, tg, scoring, with_bias, renorm)
    res = got[True]
    assert np.array_equal(res["ids"], got[False]["ids"]) and np.array_equal(res["weights"], got[False]["weights"]), (ctx, "asking for the scores changed ids or weights")
    s = res["scores"].view(np.float32).reshape(T, E)
    ids, w = res["ids"].view(np.int32).reshape(T, topk), res["weights"].view(np.float32).reshape(T, topk)
    x64 = _f64(x)
    if scoring == "sigmoid":
        s64, bound = 1.0 / (1.0 + np.exp(-x64)), 8 * U
    else:
        e = np.exp(x64 - x64.max(axis=1, keepdims=True))
        s64, bound = e / e.sum(axis=1, keepdims=True), (E + 64) * U
    assert (np.abs(s.astype(np.float64) - s64) <= bound * s64).all(), (ctx, "scores")
    want_ids, want_w = grouped_topk_ref(s, topk, n_group=G, topk_group=tg, bias=None if bias is None else bias.numpy(), renormalize=renorm, routed_scaling_factor=scale)
    assert np.array_equal(ids, want_ids), (ctx, "ids")
    if renorm:
        assert (np.abs(w - want_w) <= (topk + 4) * U * want_w).all(), (ctx, "weights")
    else:
        assert np.array_equal(w.view(np.int32), want_w.view(np.int32)), (ctx, "weights")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("E", EXPERTS)
def test_moe_topk_grouped(q, E, dtype):
    """with and without the scores (the same bits); ids equal grouped_topk_ref on the returned scores, the scores within the bounds of
    tests/test_gpu_moe_route_grouped.py (sigmoid 8 2^-24, softmax (E + 64) 2^-24), plain weights bit for bit, renormalised ones within (topk + 4) 2^-24"""
    for T in TOKENS:
        for G, tg, scoring, with_bias, renorm, scale, topks in _grouped_configs(E):
            for topk in topks:
                _run_grouped(T, E, dtype, topk, G, tg, scoring, with_bias, renorm, scale, seed=E * 100 + T * 7 + topk)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("cfg", PUBLISHED, ids=["deepseek_v3", "kimi_k2", "deepseek_v2"])
def test_moe_topk_grouped_published_configurations(q, cfg, dtype):
    E, G, tg, topk, scoring, with_bias, renorm, scale = cfg
    _run_grouped(5, E, dtype, topk, G, tg, scoring, with_bias, renorm, scale, seed=E)


# ------------------------------------------------------------------------------------------------
# 5. the expert sort
# ------------------------------------------------------------------------------------------------
def _sort_bound():
    ws = fp.cabi().qutlass_amd_moe_sort_workspace_bytes
    lo, hi = 1, 1 << 30
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ws(mid, 8) == 0 else (lo, mid)
    return lo


def _sort_ids(n, E, rng):
    ids = rng.integers(0, E, n).astype(np.int64)
    if n >= 8:   # dropped ids, as in tests/test_gpu_moe_route.py
        where = rng.permutation(n)[: max(4, n // 16)]
        ids[where] = np.array([-1, E, I32_MIN, I32_MAX])[np.arange(where.size) % 4]
    return ids


def _sort_case(n, E, dtype, with_map, forced):
    """one call of moeSort_ (the product library) or, forced, of the lab library's C entry under moe_sort_one_launch_max"""
    import _benchlib as lab

    rng = np.random.default_rng(n * 31 + E + with_map)
    topk = next(k for k in (8, 5, 3, 2, 1) if n % k == 0)
    T = n // topk
    lib = fp.cabi(lab=forced is not None)
    if with_map:                       # E local experts out of G = 2 E global ones: the second half maps to 0 .. E - 1, the first is another rank's
        Gn = 2 * E
        emap = np.full(Gn, -1, dtype=np.int32)
        emap[E:] = np.arange(E)
        flat = _sort_ids(n, Gn, rng)
        key = np.where((flat >= 0) & (flat < Gn), emap[np.clip(flat, 0, Gn - 1)], -1).astype(np.int64)
    else:
        flat = key = _sort_ids(n, E, rng)
    ids = torch.from_numpy(flat.reshape(T, topk)).to(dtype)   # (int32: the out-of-range values are int32's own extremes)
    with lab.forced(moe_sort_one_launch_max=forced) if forced is not None else contextlib.nullcontext():
        ws_bytes = lib.qutlass_amd_moe_sort_workspace_bytes(n, E)
        lay = fp.Layout().input("topk_ids", ids)
        if with_map:
            lay.input("expert_map", torch.from_numpy(emap))
        lay.output("src_row", n * 4).output("offs", E * 4).output("pos", n * 4)
        if ws_bytes:
            lay.scratch("workspace", ws_bytes + fp.SORT_WS_TAIL, ws_bytes)

        def call(a):
            if forced is None:
                torch.ops.qutlass_amd.moeSort_(a.t("topk_ids", dtype, T, topk), a.t("expert_map", I32) if with_map else _empty(I32), E, a.t("src_row", I32), a.t("offs", I32),
                                               a.t("pos", I32, T, topk), a.t("workspace", U8)[:ws_bytes] if ws_bytes else _empty(U8))
            else:
                fp.ok(lib, lib.qutlass_amd_moe_sort(a.ptr("topk_ids"), ids.element_size(), T, topk, E, a.ptr("expert_map") if with_map else None, 2 * E if with_map else 0,
                                                    a.ptr("src_row"), a.ptr("offs"), a.ptr("pos"), a.ptr("workspace") if ws_bytes else None, ws_bytes, fp.stream()))

        res = fp.run_twice(lay, call, DEV)
    want = _sort_ref(key, E, topk)
    for name, w in zip(("src_row", "offs", "pos"), want):
        g = res[name].view(np.int32)
        assert np.array_equal(g, w), (n, E, with_map, forced, name, int((g != w).sum()))
    return ws_bytes


@pytest.mark.parametrize("with_map", [False, True], ids=["nomap", "map"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("E", [1, 8, 128])
def test_moe_sort(q, E, dtype, with_map):
    """1 and 63 slots, the one-launch bound - 1 / + 0 / + 1, 8192 and 8193 slots (two workgroups of the three-launch form), and 130 slots forced into the
    three-launch form; results equal the numpy stable sort, the workspace is written inside the queried size only (a 1 MiB tail keeps the fill)"""
    bound = _sort_bound()
    for n in (1, 63, bound - 1, bound, bound + 1, 8192, 8193):
        ws = _sort_case(n, E, dtype, with_map, None)
        assert (ws > 0) == (n > bound)
    assert _sort_case(130, E, dtype, with_map, 129) > 0


# ------------------------------------------------------------------------------------------------
# 6. to_blocked
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 3), (128, 4), (129, 5), (130, 6), (257, 9)])
def test_to_blocked(q, rows, cols):
    lib = fp.cabi()
    src = np.random.default_rng(rows * 16 + cols).integers(1, 256, size=(rows, cols), dtype=np.uint8)   # no zero byte: padding is told from data
    lay = fp.Layout().input("in", src).output("out", fp.blocked_scale_bytes(rows, cols * 32, 32))

    def call(a):
        fp.ok(lib, lib.qutlass_amd_to_blocked(a.ptr("in"), rows, cols, a.ptr("out"), fp.stream()))

    got = fp.run_twice(lay, call, DEV)["out"]
    assert np.array_equal(got, oracle.to_blocked(src))


# ------------------------------------------------------------------------------------------------
# 7. QAT backward
# ------------------------------------------------------------------------------------------------
def _h32():
    h = rot.signed_permuted_hadamard(32, seed=1)
    return h, _np(h)


@pytest.mark.parametrize("variant", [0, 1, 2, 3], ids=lambda v: f"bwd_variant{v}")
@pytest.mark.parametrize("op,B,N,M", [("t", 1, 96, 64), ("t", 2, 96, 72), ("qt", 1, 96, 64), ("qt", 2, 96, 96)])
def test_backward_t_qt(q, op, B, N, M, variant):
    """variant 0: backward_t_bf16_ / backward_qt_bf16_ (the product library's rule); 1 / 2 / 3: the three kernels tests/test_gpu_round4.py forces, through the lab
    library's C entries.  backward_t: rot.exact_input, scales and codes equal the oracle (tests/test_gpu_rotation_orientation.py).  backward_qt: random codes with
    scale bytes 126 .. 128, one all-zero group row; scales exact, codes within tests/test_gpu_round4.py's bound (1e-4 of them modulo the sign of zero: none, here)."""
    import _benchlib as lab

    h, hb = _h32()
    lib = fp.cabi(lab=True)
    lay = fp.Layout()
    if op == "t":
        x = rot.exact_input((B, N, M), seed=9 + M)
        lay.input("x", x).input("h", h)
        wq, ws = oracle.backward_t_bf16(_np(x), hb, acc_model=1)
    else:
        rng = np.random.default_rng(B * 100 + M)
        codes = rng.integers(0, 256, size=(B, N, M // 2), dtype=np.uint8)
        scales = rng.integers(126, 129, size=(B, N, M // 32), dtype=np.uint8)
        codes[:, -32:, : M // 4] = 0
        lay.input("xq", codes).input("xs", scales).input("h", h).input("alpha", torch.tensor([3.0]))
        wq, ws = oracle.backward_qt_bf16(codes, scales, hb, 3.0, acc_model=1)
    lay.output("out", B * M * N // 2).output("out_sf", B * M * N // 32)

    def call(a):
        if variant == 0 and op == "t":
            torch.ops.qutlass_amd.backward_t_bf16_(a.t("x", BF16, B, N, M), a.t("h", BF16, 32, 32), a.t("out", U8, B, M, N // 2), a.t("out_sf", torch.float8_e8m0fnu, B, M, N // 32))
        elif variant == 0:
            torch.ops.qutlass_amd.backward_qt_bf16_(a.t("xq", U8, B, N, M // 2), a.t("xs", torch.float8_e8m0fnu, B, N, M // 32), a.t("h", BF16, 32, 32), a.t("alpha", F32),
                                                    a.t("out", U8, B, M, N // 2), a.t("out_sf", torch.float8_e8m0fnu, B, M, N // 32))
        elif op == "t":
            fp.ok(lib, lib.qutlass_amd_backward_t_bf16(a.ptr("x"), a.ptr("h"), B, N, M, a.ptr("out"), a.ptr("out_sf"), fp.stream()))
        else:
            fp.ok(lib, lib.qutlass_amd_backward_qt_bf16(a.ptr("xq"), a.ptr("xs"), a.ptr("h"), a.ptr("alpha"), B, N, M, a.ptr("out"), a.ptr("out_sf"), fp.stream()))

    with lab.forced(bwd_variant=variant):
        res = fp.run_twice(lay, call, DEV)
    assert np.array_equal(res["out_sf"], ws.reshape(-1)), (op, variant, "scales", int((res["out_sf"] != ws.reshape(-1)).sum()))
    eq = oracle.codes_equal_mod_zero_sign(res["out"], wq.reshape(-1))
    assert int((~eq).sum()) <= (0 if op == "t" else 1e-4 * eq.size), (op, variant, "codes", int((~eq).sum()), eq.size)


ROWS_SHAPES = [(1, 128, 256), (129, 256, 256), (200, 256, 512)]


@pytest.mark.parametrize("m,m_pad,n,nc", [(*s, nc) for s in ROWS_SHAPES for nc in (0, 1, 4) if nc != 4 or s[2] % 512 == 0])   # (512-column workgroups: n % 512 == 0)
def test_backward_rows_square_double(q, m, m_pad, n, nc):
    """qutlass_amd_backward_bf16_square_double_mxfp8_rows: the input view holds exactly m rows; rows m .. m_pad - 1 count as zeros, so the whole m_pad extent is written
    and equals the oracle on the zero-padded input.  nc 0: the product library; 1 / 4: the 128- and 512-column workgroups through the lab library."""
    import _benchlib as lab

    lib = fp.cabi(lab=nc != 0)
    rng = np.random.default_rng(m + n)
    x = torch.from_numpy(rng.standard_normal((m, n)).astype(np.float32) * 3.0).to(BF16)
    if m >= 64:
        x[32:64, 128:256] = 0          # an all-zero 32 x 32 block: shared exponent 127
    xp = np.zeros((m_pad, n), np.uint16)
    xp[:m] = _np(x)
    wy, wrs, wcs = oracle.backward_bf16_square_double_mxfp8(xp)
    lay = fp.Layout().input("x", x).output("y", m_pad * n).output("row_sf", m_pad * n // 32).output("col_sf", n * m_pad // 32)

    def call(a):
        fp.ok(lib, lib.qutlass_amd_backward_bf16_square_double_mxfp8_rows(a.ptr("x"), m, m_pad, n, a.ptr("y"), a.ptr("row_sf"), a.ptr("col_sf"), fp.stream()))

    with lab.forced(transpose_nc=nc) if nc else contextlib.nullcontext():
        res = fp.run_twice(lay, call, DEV)
    for name, w in (("y", wy), ("row_sf", wrs), ("col_sf", wcs)):
        assert np.array_equal(res[name], np.asarray(w).reshape(-1)), (name, int((res[name] != np.asarray(w).reshape(-1)).sum()))


@pytest.mark.parametrize("nc", [0, 4, 2, 128, 3], ids=lambda v: f"transpose_nc{v}")
@pytest.mark.parametrize("m,m_pad,n", ROWS_SHAPES)
def test_backward_rows_transpose(q, m, m_pad, n, nc):
    """qutlass_amd_mxfp4_transpose_mxfp8_rows: x_fp4 and scales hold exactly m rows (read-only); rows m .. m_pad - 1 count as zero codes with unit scales.  nc 0: the
    product library; the others: the forms tests/test_gpu_round4.py forces through the lab library."""
    import _benchlib as lab

    lib = fp.cabi(lab=nc != 0)
    rng = np.random.default_rng(m * 7 + n)
    codes = rng.integers(0, 256, size=(m, n // 2), dtype=np.uint8)
    scales = rng.integers(117, 137, size=(m, n // 32), dtype=np.uint8)
    if m >= 64:
        codes[32:64, : n // 4] = 0
    pc = np.zeros((m_pad, n // 2), np.uint8)
    pc[:m] = codes
    ps = np.full((m_pad, n // 32), 127, np.uint8)
    ps[:m] = scales
    wy, ws = oracle.mxfp4_transpose_mxfp8(pc, ps)
    lay = fp.Layout().input("x_fp4", codes).input("scales", scales).output("y", n * m_pad).output("out_sf", n * m_pad // 32)

    def call(a):
        fp.ok(lib, lib.qutlass_amd_mxfp4_transpose_mxfp8_rows(a.ptr("x_fp4"), a.ptr("scales"), m, m_pad, n, a.ptr("y"), a.ptr("out_sf"), fp.stream()))

    with lab.forced(transpose_nc=nc) if nc else contextlib.nullcontext():
        res = fp.run_twice(lay, call, DEV)
    assert np.array_equal(res["out_sf"], np.asarray(ws).reshape(-1)), int((res["out_sf"] != np.asarray(ws).reshape(-1)).sum())
    assert np.array_equal(res["y"], np.asarray(wy).reshape(-1)), int((res["y"] != np.asarray(wy).reshape(-1)).sum())


# ------------------------------------------------------------------------------------------------
# 8. the one-launch decode layer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,om", [(0, oracle.QUEST), (1, oracle.ABS_MAX)], ids=["quest", "abs_max"])
@pytest.mark.parametrize("m", [1, 8])
def test_one_launch_decode_layer(q, m, method, om):
    """qutlass_amd_fused_quantize_matmul_mxf4_bf16_tn, n = 264, k = 384: D between bands, every operand banded; against oracle.fused_quantize_mx followed by
    oracle.gemm_blockscaled within tests/test_gpu_rotation_orientation.py's bound for non-exact GEMM operands, max |got - want| <= 1e-2 max |want|"""
    n, k = 264, 384
    lib = fp.cabi()
    h, hb = _h32()
    gen = torch.Generator(device="cpu").manual_seed(17 + m)
    x = (torch.randn(m, k, generator=gen) * 25.0).to(BF16)
    w = (torch.randn(n, k, generator=gen) * 25.0).to(BF16)
    wq, wsf, _ = oracle.fused_quantize_mx(_np(w), hb, oracle.ABS_MAX, acc_model=1)
    xq, xs, _ = oracle.fused_quantize_mx(_np(x), hb, om, acc_model=1)
    alpha = float(np.float32((1.0 / 9.0) if method == 1 else (1.0 / 3.0)))
    w_sf = oracle.to_blocked(wsf.reshape(n, k // 32))
    ref = oracle.gemm_blockscaled(oracle.KIND_MXFP4, xq.reshape(m, k // 2), wq.reshape(n, k // 2), oracle.to_blocked(xs.reshape(m, k // 32)), w_sf, alpha, m, n, k)
    want = oracle.bf16_bits_to_f32(ref).astype(np.float64)
    lay = fp.Layout().input("x", x).input("h", h).input("B", wq).input("B_sf", w_sf).input("alpha", torch.tensor([alpha])).output("D", m * n * 2)

    def call(a):
        fp.ok(lib, lib.qutlass_amd_fused_quantize_matmul_mxf4_bf16_tn(a.ptr("x"), a.ptr("h"), 32, method, a.ptr("B"), a.ptr("B_sf"), a.ptr("alpha"), a.ptr("D"), m, n, k, fp.stream()))

    got = oracle.bf16_bits_to_f32(fp.run_twice(lay, call, DEV)["D"].view(np.uint16).reshape(m, n)).astype(np.float64)
    err = np.abs(got - want).max()
    print(f"m={m} method={method}: max |got - want| = {err / np.abs(want).max():.2e} max |want|")
    assert err <= 1e-2 * np.abs(want).max(), (m, method, err, np.abs(want).max())
