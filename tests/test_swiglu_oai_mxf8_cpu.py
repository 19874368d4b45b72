"""fusedSwigluOaiQuantizeMxf8 (the clamped SwiGLU of gpt-oss fused into the MXFP8 quantizer: the A operand of the W4A8 grouped GEMM) without a GPU: the exported
symbol, every argument check of the C entry (all of them happen before any HIP call, so null / dummy pointers are enough), the schemas of the in-place twin and of
the functional op, the shape-only kernel, a traced W4A8 layer, the Python wrapper's errors, and the quantizer table left as it was.  The GPU half is
tests/test_gpu_swiglu_oai_mxf8.py."""
import ctypes
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import _footprint as fp
import qutlass_amd as q
from qutlass_amd import _lib

OK, INVALID = _lib.QAMD_OK, _lib.QAMD_ERR_INVALID
E4M3, E5M2 = 0, 1   # QAMD_FP8_E4M3, QAMD_FP8_E5M2 (include/qutlass_amd.h)
X = 0x10000   # a 16-byte aligned dummy address: nothing below dereferences it
NAME = "qutlass_amd_fused_swiglu_oai_quantize_mxf8"


def _err():
    return _lib.load().qutlass_amd_last_error().decode()


def _fq(rot, rows, inter, fmt=E4M3, alpha=1.702, limit=7.0, bias=None, offs=None, e=0, x=X, h=X, out=X, sf=X):
    return _lib.load().qutlass_amd_fused_swiglu_oai_quantize_mxf8(x, h, rot, rows, inter, fmt, alpha, limit, bias, offs, e, out, sf, None)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_declared_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, NAME) and NAME in _lib.SYMBOLS
    header = open(fp.HEADER).read()
    decl = re.search(NAME + r"\(([^;]*)\);", header)
    assert decl is not None and len(decl.group(1).split(",")) == 14 == len(_lib.SYMBOLS[NAME][1])
    # the same argument list as the MXFP4 entry, fmt standing where method does
    assert _lib.SYMBOLS[NAME] == _lib.SYMBOLS["qutlass_amd_fused_swiglu_oai_quantize_mx"]
    for words in ("byte for byte", "first rows * inter / 32 bytes of out_e8m0", "rest of the caller's buffer untouched", "rows * inter bytes of e4m3 codes",
                  "rows * inter, e * inter < 2^29", "unspecified bytes for their own rotation group"):
        assert words in header, words


def test_rotation_sizes():
    assert _fq(128, 4, 128) == INVALID
    msg = _err()
    assert "fusedSwigluOaiQuantizeMxf8" in msg and "128 is not supported" in msg
    assert "swiglu_oai_and_mul followed by fusedQuantizeMxf8" in msg                  # names the two-call composition, with the right quantizer
    assert _fq(128, 0, 128) == INVALID                                                # before the empty-input return
    assert _fq(128, 4, 128, fmt=E5M2) == INVALID and "128 is not supported" in _err()   # and before the fmt check
    for rot in (16, 0, 48, 256):
        assert _fq(rot, 4, 256) == INVALID and "Unsupported rotation size" in _err() and "expected 32 or 64" in _err(), rot


@pytest.mark.parametrize("rot", [32, 64])
def test_fmt_is_e4m3_only(rot):
    for fmt in (E5M2, -1, 2):
        assert _fq(rot, 4, 64, fmt=fmt) == INVALID
        assert "invalid fmt" in _err() and "a forward activation is e4m3 only" in _err(), fmt
    assert _fq(rot, 0, 64, fmt=E5M2) == INVALID                                       # before the empty-input return
    assert _fq(rot, -1, 64, fmt=E5M2) == INVALID and "invalid fmt" in _err()         # and before the shape checks, where the MXFP4 entry checks its method


@pytest.mark.parametrize("rot", [32, 64])
def test_argument_checks(rot):
    assert _fq(rot, 4, rot + 16) == INVALID and f"multiple of {rot}" in _err()        # I % R
    assert _fq(rot, 4, 8) == INVALID and f"multiple of {rot}" in _err()
    assert _fq(rot, -1, 64) == INVALID and "bad shape" in _err()
    assert _fq(rot, 4, 0) == INVALID and _fq(rot, 4, -64) == INVALID and _fq(rot, 1 << 31, 64) == INVALID
    assert _fq(rot, 4, 64, x=X + 4) == INVALID and "x must be 16-byte aligned" in _err()
    assert _fq(rot, 4, 64, bias=X + 8, offs=X, e=2) == INVALID and "bias must be 16-byte aligned" in _err()
    assert _fq(rot, 4, 64, bias=X, offs=X + 2, e=2) == INVALID and "offs must be 4-byte aligned" in _err()
    assert _fq(rot, 4, 64, bias=X, offs=None, e=2) == INVALID and "needs offs" in _err()                  # e > 1 without offs
    for e in (0, -1, 1025):
        assert _fq(rot, 4, 64, bias=X, offs=X, e=e) == INVALID and "E must be in [1, 1024]" in _err(), e
    for alpha in (0.0, -1.0, float("inf"), float("nan")):
        assert _fq(rot, 4, 64, alpha=alpha) == INVALID and "alpha must be finite and > 0" in _err(), alpha
    for limit in (0.0, -7.0, float("inf"), float("nan"), 7.01, 1.0 + 2.0 ** -8):
        assert _fq(rot, 4, 64, limit=limit) == INVALID and "exactly representable in bf16" in _err(), limit
    for null in ("x", "h", "out", "sf"):
        assert _fq(rot, 4, 64, **{null: None}) == INVALID and "null pointer" in _err(), null
    if rot == 64:
        assert _fq(64, 4, 64, h=X + 2) == INVALID and "rotation matrix must be 16-byte aligned" in _err()
    # every message carries the entry's own name
    assert _fq(rot, 4, 8) == INVALID and _err().startswith("fusedSwigluOaiQuantizeMxf8:")


def test_empty_input_launches_nothing():
    for rot in (32, 64):
        assert _fq(rot, 0, 64) == OK and _fq(rot, 0, 2944) == OK
        assert _fq(rot, 0, 64, x=None, h=None, out=None, sf=None) == OK                                   # rows == 0 with null pointers
        assert _fq(rot, 0, 64, bias=X, offs=None, e=1) == OK                                              # one expert: offs is optional
        assert _fq(rot, 0, 64, bias=X, offs=X, e=1024) == OK
        assert _fq(rot, 0, 64, limit=0.5) == OK and _fq(rot, 0, 64, alpha=1.0, limit=2.5) == OK


def test_size_limits_are_checked_not_wrapped():
    rows, inter = 1 << 15, 1 << 14            # rows * inter = 2^29: exactly 2 GiB of input
    assert _fq(32, rows, inter) == INVALID and "x (rows * 2 * inter * 2" in _err() and "below 2 GiB" in _err()
    assert _fq(64, rows, inter) == INVALID and "below 2 GiB" in _err()
    assert _fq(32, 4, 1 << 19, bias=X, offs=X, e=1024) == INVALID and "bias (E * 2 * inter * 2" in _err() and "below 2 GiB" in _err()
    assert _fq(32, 0, 1 << 18, bias=X, offs=X, e=1024) == OK                                               # 2^28: fits


def test_the_checks_come_in_the_mxfp4_entry_s_order():
    """one call that breaks several rules names the first: rotation, fmt, shape, x's size, alpha / limit, the bias's checks, the bias's size"""
    assert _fq(32, 4, 8, fmt=E5M2) == INVALID and "invalid fmt" in _err()
    assert _fq(32, 1 << 15, 1 << 14, x=X + 4) == INVALID and "16-byte aligned" in _err()
    assert _fq(32, 1 << 15, 1 << 14, alpha=0.0) == INVALID and "below 2 GiB" in _err()
    assert _fq(32, 4, 64, alpha=0.0, bias=X, offs=X, e=0) == INVALID and "alpha must be" in _err()
    assert _fq(32, 4, 1 << 19, bias=X + 8, offs=X, e=1024) == INVALID and "bias must be 16-byte aligned" in _err()


# ---- the torch ops --------------------------------------------------------------------------------------------------------------------
def _meta(*shape, dtype=torch.bfloat16):
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_schema_of_the_twin():
    schema = torch.ops.qutlass_amd.fusedSwigluOaiQuantizeMxf8_.default._schema
    written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
    assert written == ["OUT", "OUT_sf"] and len(schema.returns) == 0, str(schema)
    assert [a.name for a in schema.arguments] == ["A", "R", "OUT", "OUT_sf", "alpha", "limit", "bias", "offs"], str(schema)    # no method: abs-max only
    assert torch._library.simple_registry.singleton.find("qutlass_amd::fusedSwigluOaiQuantizeMxf8_").fake_impl.kernel is not None
    row = q.ops.QUANT_OPS["swiglu_oai_quantize_mxf8"]
    assert row.twin == "fusedSwigluOaiQuantizeMxf8_" and row.fmt == "mxf8"


def test_schema_of_the_functional_op():
    schema = torch.ops.qutlass_amd.swiglu_oai_quantize_mxf8.default._schema
    assert not any(a.alias_info is not None for a in schema.arguments) and not any(r.alias_info is not None for r in schema.returns), str(schema)
    assert len(schema.returns) == 2 and [a.name for a in schema.arguments] == ["A", "R", "alpha", "limit", "bias", "offs"], str(schema)


def test_fake_kernel_allocates_what_fusedQuantizeMxf8_does():
    with FakeTensorMode():
        dev = "cuda"
        x, h = torch.empty(2, 35, 192, dtype=torch.bfloat16, device=dev), torch.empty(32, 32, dtype=torch.bfloat16, device=dev)
        want = q.ops.alloc_quant(q.ops.QUANT_OPS["quantize_mxf8"], torch.empty(2, 35, 96, dtype=torch.bfloat16, device=dev), h, torch.float8_e4m3fn)
        assert want[0].shape == (2, 35, 96) and want[0].dtype == torch.float8_e4m3fn and want[1].dtype == torch.float8_e8m0fnu
        bias, offs = torch.empty(4, 192, dtype=torch.bfloat16, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
        for b, o in ((None, None), (bias, offs), (bias[:1], None)):
            got = torch.ops.qutlass_amd.swiglu_oai_quantize_mxf8(x, h, 1.702, 7.0, b, o)
            for g, w in zip(got, want):
                assert g.shape == w.shape and g.dtype == w.dtype and g.device == w.device
            got = torch.compile(lambda x, h, b, o: q.fusedSwigluOaiQuantizeMxf8(x, h, bias=b, offs=o), backend="eager", fullgraph=True)(x, h, b, o)
            for g, w in zip(got, want):
                assert g.shape == w.shape and g.dtype == w.dtype


def test_a_w4a8_layer_traces_with_fullgraph():
    with FakeTensorMode():
        dev = "cuda"
        M, I, N, E = 35, 128, 64, 4
        x, h = torch.empty(M, 2 * I, dtype=torch.bfloat16, device=dev), torch.empty(64, 64, dtype=torch.bfloat16, device=dev)
        b1, offs = torch.empty(E, 2 * I, dtype=torch.bfloat16, device=dev), torch.empty(E, dtype=torch.int32, device=dev)
        w = torch.empty(E, N, I // 2, dtype=torch.uint8, device=dev)
        w_sf = torch.empty(E * N * I // 32, dtype=torch.float8_e8m0fnu, device=dev)
        alpha = torch.empty(1, device=dev)

        def layer(x, h, b1, offs, w, w_sf, alpha):
            c, s = q.fusedSwigluOaiQuantizeMxf8(x, h, bias=b1, offs=offs)
            return q.grouped_matmul_mxf8_mxf4_bf16_tn(c, w, s, w_sf, alpha, offs)

        out = torch.compile(layer, backend="eager", fullgraph=True)(x, h, b1, offs, w, w_sf, alpha)
        assert out.shape == (M, N) and out.dtype == torch.bfloat16


# ---- the Python wrapper -------------------------------------------------------------------------------------------------------------------
def test_wrapper_value_errors():
    x, h = _meta(4, 128), _meta(32, 32)
    with pytest.raises(ValueError, match="not supported by fusedSwigluOaiQuantizeMxf8.*swiglu_oai_and_mul followed by fusedQuantizeMxf8"):
        q.fusedSwigluOaiQuantizeMxf8(_meta(4, 256), _meta(128, 128))
    with pytest.raises(ValueError, match=r"2 \* I"):
        q.fusedSwigluOaiQuantizeMxf8(_meta(4, 127), h)                                 # an odd last dimension
    with pytest.raises(ValueError, match=r"bias must be \(E, 2 \* I\)"):
        q.fusedSwigluOaiQuantizeMxf8(x, h, bias=_meta(1, 64))                           # a bias of the wrong width
    with pytest.raises(ValueError, match="needs offs"):
        q.fusedSwigluOaiQuantizeMxf8(x, h, bias=_meta(2, 128))
    with pytest.raises(ValueError, match="offs without a bias"):
        q.fusedSwigluOaiQuantizeMxf8(x, h, offs=_meta(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="limit must be"):
        q.fusedSwigluOaiQuantizeMxf8(x, h, limit=7.01)
    with pytest.raises(ValueError, match="alpha must be"):
        q.fusedSwigluOaiQuantizeMxf8(x, h, alpha=0.0)
    # the MXFP4 op's message is its own still
    with pytest.raises(ValueError, match="not supported by fusedSwigluOaiQuantizeMx .*followed by fusedQuantizeMx$"):
        q.fusedSwigluOaiQuantizeMx(_meta(4, 256), _meta(128, 128))


def test_eager_calls_take_the_twin_through_the_shared_runner(monkeypatch):
    seen = []
    monkeypatch.setattr(q.ops, "run_quant", lambda row, *a: seen.append((row.twin, a[2:])) or "ran")
    x, h = _meta(4, 128), _meta(32, 32)
    assert q.fusedSwigluOaiQuantizeMxf8(x, h) == "ran"
    assert q.fusedSwigluOaiQuantizeMx(x, h, method="abs_max") == "ran"
    assert seen == [("fusedSwigluOaiQuantizeMxf8_", (1.702, 7.0, None, None)), ("fusedSwigluOaiQuantizeMx_", (1.702, 7.0, None, None, 1))]


def test_exported_and_documented():
    import qutlass

    assert qutlass.fusedSwigluOaiQuantizeMxf8 is q.fusedSwigluOaiQuantizeMxf8
    assert "fusedSwigluOaiQuantizeMxf8" in q.__doc__


def test_the_op_is_the_last_row_of_the_quantizer_table():
    """the op's record stands IN the table, behind the fifteen rows that were there before it: a row may fix its code dtype, as it may fix `blocked`"""
    assert list(q.ops.QUANT_OPS) == [
        "quantize_mx", "quantize_nv", "quantize_mx_blocked", "quantize_nv_blocked", "silu_mul_quantize_mx", "silu_mul_quantize_nv", "swiglu_oai_quantize_mx",
        "gather_quantize_mx", "gather_quantize_nv", "gather_quantize_nv_grouped", "silu_mul_quantize_nv_grouped", "quantize_mxf8", "quantize_mxf8_blocked",
        "silu_mul_quantize_mxf8", "gather_quantize_mxf8", "swiglu_oai_quantize_mxf8"]
    row = q.ops.QUANT_OPS["swiglu_oai_quantize_mxf8"]
    assert row.twin == "fusedSwigluOaiQuantizeMxf8_" and row.fmt == "mxf8" and row.dtype == torch.float8_e4m3fn and row.blocked is False
    assert not hasattr(q.ops, "SWIGLU_OAI_MXF8")
