"""gpt-oss ops (swiglu_oai_and_mul, fusedSwigluOaiQuantizeMx, moe_combine with a bias) without a GPU: the numpy model is a valid judge (its rounding helper, and
fp64 against longdouble over every gate it is asked about), every argument check of the three C entries (all of them happen before any HIP call, so null / dummy
pointers are enough), the Python wrappers' errors, the shape-only kernels of the functional ops, and utils.split_interleaved_gate_up.  The GPU half is
tests/test_gpu_swiglu_oai.py and tests/test_gpu_moe_combine_bias.py."""
import ctypes

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import _swiglu_oai_model as model
import qutlass_amd as q
from qutlass_amd import _lib
from qutlass_amd.utils import split_interleaved_gate_up

OK, INVALID = _lib.QAMD_OK, _lib.QAMD_ERR_INVALID
X = 0x10000   # a 16-byte aligned dummy address: nothing below dereferences it


def _err():
    return _lib.load().qutlass_amd_last_error().decode()


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def test_model_rounding_helpers():
    bits = np.arange(0, 0x7f80, dtype=np.uint16)
    assert np.array_equal(model.f64_to_bf16(model.bf16_to_f64(bits)), bits)
    assert np.array_equal(model.f64_to_bf16(-model.bf16_to_f64(bits)), bits | 0x8000)
    mid = (model.bf16_to_f64(bits[:-1]) + model.bf16_to_f64(bits[1:])) / 2
    even = np.where(bits[:-1] & 1, bits[1:], bits[:-1])
    assert np.array_equal(model.f64_to_bf16(mid), even)
    assert model.f64_to_bf16(np.array([-0.0]))[0] == 0x8000
    # the fp32 -> bf16 helper: the same two properties (the midpoints of normal neighbours are fp32 numbers)
    assert np.array_equal(model.f32_to_bf16(model.bf16_to_f32(bits)), bits)
    assert np.array_equal(model.f32_to_bf16(mid.astype(np.float32)), even)


@pytest.mark.parametrize("alpha", [1.702, 1.0])
def test_model_fp64_is_a_valid_judge(alpha):
    """over the 63 490 finite gates with |g| >= 2^-120 or g = +-0: fp64 and longdouble give the same bf16 s, and no true value lies closer to a bf16 tie than
    fp64's error could decide wrongly"""
    assert np.finfo(np.longdouble).nmant > 52, "the second opinion needs a longdouble wider than fp64 (x86: 64-bit significand)"
    gates = model.finite_gates()
    assert gates.size == 63490
    gc = model.f32_to_bf16(np.minimum(model.bf16_to_f32(gates), np.float32(7.0)))
    v64, vld = model.sigmoid_gate(gc, alpha, np.float64), model.sigmoid_gate(gc, alpha, np.longdouble)
    s64, sld = model.f64_to_bf16(v64), model.f64_to_bf16(vld)
    assert int((s64 != sld).sum()) == 0
    # distance of the longdouble value from the nearest tie (the midpoint of s and its neighbour on the value's side), in bf16 ulp of s
    nz = (vld != 0) & np.isfinite(vld)
    a = np.abs(vld[nz])
    _, e = np.frexp(a)
    ulp = np.ldexp(np.ones_like(a), np.maximum(e, -125) - 8)
    frac = a / ulp - np.floor(a / ulp)
    dist = np.abs(frac - 0.5)
    inexact = frac != 0
    print(f"alpha {alpha}: nearest tie {float(dist[inexact].min()):.3g} bf16 ulp away")
    # fp64: exp within 1 ulp, a product, a sum and a quotient -- under 4 * 2^-53 relative, i.e. under 2^-43 = 1.2e-13 bf16 ulp (an ulp is at least 2^-8 of the value)
    assert float(dist[inexact].min()) > 1e-9


def test_model_zero_and_clamp():
    one, z = 0x3f80, 0x0000
    x = np.array([[z, z]], dtype=np.uint16)
    assert model.swiglu_oai(x)[0, 0] == 0                                   # zero gate, zero up -> +0
    big = model.f32_to_bf16(np.array([100.0, 117.0], dtype=np.float32))
    assert model.swiglu_oai(np.array([[big[0], one]], dtype=np.uint16))[0, 0] == model.f32_to_bf16(np.array([14.0], np.float32))[0]   # s = 7, up + 1 = 2
    assert model.swiglu_oai(np.array([[one, big[1]]], dtype=np.uint16))[0, 0] == model.swiglu_oai(np.array([[one, model.f32_to_bf16(np.array([7.0], np.float32))[0]]], np.uint16))[0, 0]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("qutlass_amd_swiglu_oai_mul_bf16", "qutlass_amd_fused_swiglu_oai_quantize_mx", "qutlass_amd_moe_combine_bias_bf16"):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS


def _act(rows, inter, alpha=1.702, limit=7.0, bias=None, offs=None, e=0, x=X, out=X):
    return _lib.load().qutlass_amd_swiglu_oai_mul_bf16(x, rows, inter, alpha, limit, bias, offs, e, out, None)


def _fq(rot, rows, inter, method=0, alpha=1.702, limit=7.0, bias=None, offs=None, e=0, x=X, h=X, out=X, sf=X):
    return _lib.load().qutlass_amd_fused_swiglu_oai_quantize_mx(x, h, rot, rows, inter, method, alpha, limit, bias, offs, e, out, sf, None)


def _cb(m, hdim, t, topk, bias=X, offs=X, e=4, y=X, pos=X, w=X, out=X):
    return _lib.load().qutlass_amd_moe_combine_bias_bf16(y, m, hdim, pos, w, t, topk, bias, offs, e, out, None)


BAD_LIMITS = [0.0, -7.0, float("inf"), float("nan"), 7.01, 1.0 + 2.0 ** -8]
BAD_ALPHAS = [0.0, -1.0, float("inf"), float("nan")]


def _activation_checks(call):
    """the checks the two activation entries share; call(rows, inter, **kw) with inter a legal width"""
    for limit in BAD_LIMITS:
        assert call(4, 64, limit=limit) == INVALID and "limit must be > 0, finite and exactly representable in bf16" in _err(), limit
    for alpha in BAD_ALPHAS:
        assert call(4, 64, alpha=alpha) == INVALID and "alpha must be finite and > 0" in _err(), alpha
    for limit in (7.0, 0.5, 2.0 ** -130, 3.3895313892515355e38):   # bf16 values, the smallest subnormals and the largest finite among them
        assert call(0, 64, limit=limit) == OK, limit
    for e in (0, -1, 1025):
        assert call(4, 64, bias=X, offs=X, e=e) == INVALID and "E must be in [1, 1024]" in _err(), e
    assert call(4, 64, bias=X, offs=None, e=2) == INVALID and "needs offs" in _err()
    assert call(0, 64, bias=X, offs=None, e=1) == OK                                          # one expert: offs is optional
    assert call(0, 64, bias=X, offs=X, e=1024) == OK
    assert call(4, 64, bias=X + 8, offs=X, e=2) == INVALID and "bias must be 16-byte aligned" in _err()
    assert call(4, 64, bias=X, offs=X + 2, e=2) == INVALID and "offs must be 4-byte aligned" in _err()
    assert call(4, 64, x=X + 4) == INVALID and "16-byte aligned" in _err()
    assert call(-1, 64) == INVALID and "bad shape" in _err()
    assert call(4, 0) == INVALID and call(4, -64) == INVALID and call(1 << 31, 64) == INVALID
    assert call(0, 64) == OK and call(0, 64, x=None, out=None) == OK                             # rows == 0: nothing to do, nothing launched
    assert call(4, 64, x=None) == INVALID and "null pointer" in _err()
    assert call(4, 64, out=None) == INVALID and "null pointer" in _err()


def test_swiglu_oai_mul_argument_checks():
    _activation_checks(_act)
    assert _act(4, 12) == INVALID and "multiple of 8" in _err()
    assert _act(4, 64, out=X + 8) == INVALID and "out must be 16-byte aligned" in _err()
    assert _act(0, 8) == OK and _act(0, 2880) == OK


@pytest.mark.parametrize("rot", [32, 64])
def test_fused_swiglu_oai_argument_checks(rot):
    _activation_checks(lambda rows, inter, **kw: _fq(rot, rows, inter, **kw))
    assert _fq(rot, 4, rot + 16) == INVALID and f"multiple of {rot}" in _err()                      # I % R
    assert _fq(rot, 4, 8) == INVALID and f"multiple of {rot}" in _err()
    for method in (-1, 2):
        assert _fq(rot, 4, 64, method=method) == INVALID and "invalid method" in _err()
    for null in ("h", "sf"):
        assert _fq(rot, 4, 64, **{null: None}) == INVALID and "null pointer" in _err(), null
    assert _fq(rot, 0, 2944) == OK
    if rot == 64:
        assert _fq(64, 4, 64, h=X + 2) == INVALID and "rotation matrix must be 16-byte aligned" in _err()


def test_fused_swiglu_oai_rotation_sizes():
    assert _fq(128, 4, 128) == INVALID
    msg = _err()
    assert "128 is not supported" in msg and "swiglu_oai_and_mul" in msg and "fusedQuantizeMx" in msg      # names the two-call composition
    assert _fq(128, 0, 128) == INVALID                                                                   # before the empty-input return
    for rot in (16, 0, 48, 256):
        assert _fq(rot, 4, 256) == INVALID and "Unsupported rotation size" in _err(), rot


def test_fused_swiglu_oai_size_limits_are_checked_not_wrapped():
    rows, inter = 1 << 15, 1 << 14            # rows * inter = 2^29: exactly 2 GiB of input
    assert _fq(32, rows, inter) == INVALID and "x (rows * 2 * inter * 2" in _err() and "below 2 GiB" in _err()
    assert _fq(64, rows, inter) == INVALID and "below 2 GiB" in _err()
    assert _fq(32, 4, 1 << 19, bias=X, offs=X, e=1024) == INVALID and "bias (E * 2 * inter * 2" in _err() and "below 2 GiB" in _err()
    assert _fq(32, 0, 1 << 18, bias=X, offs=X, e=1024) == OK                                               # 2^28: fits
    assert _act(0, 1 << 20, bias=X, offs=X, e=1024) == OK                                                  # the streaming op has no such limit


def test_moe_combine_bias_argument_checks():
    assert _cb(8, 64, 0, 2) == OK and _cb(8, 64, 0, 2, y=None, pos=None, w=None, out=None) == OK           # t == 0: nothing to do
    assert _cb(8, 12, 4, 2) == INVALID and "multiple of 8" in _err()
    for topk in (0, 33):
        assert _cb(8, 64, 4, topk) == INVALID and "topk must be in [1, 32]" in _err()
    assert _cb(-1, 64, 4, 2) == INVALID and "bad shape" in _err()
    assert _cb(8, 0, 4, 2) == INVALID and _cb(8, 64, -1, 2) == INVALID and _cb(1 << 31, 64, 4, 2) == INVALID
    assert _cb(8, 64, 4, 2, y=X + 2) == INVALID and "y and out must be 16-byte aligned" in _err()
    assert _cb(8, 64, 4, 2, out=X + 8) == INVALID and "y and out must be 16-byte aligned" in _err()
    for e in (0, -3, 1025):
        assert _cb(8, 64, 4, 2, e=e) == INVALID and "E must be in [1, 1024]" in _err(), e
    assert _cb(8, 64, 4, 2, offs=None, e=2) == INVALID and "needs offs" in _err()
    assert _cb(8, 64, 0, 2, offs=None, e=1) == OK
    assert _cb(8, 64, 4, 2, bias=X + 4) == INVALID and "bias must be 16-byte aligned" in _err()
    assert _cb(8, 64, 4, 2, offs=X + 1) == INVALID and "offs must be 4-byte aligned" in _err()
    for null in ("y", "pos", "w", "out", "bias"):
        assert _cb(8, 64, 4, 2, **{null: None}) == INVALID and "null pointer" in _err(), null


# ---- the Python wrappers ----------------------------------------------------------------------------------------------------------------
def _meta(*shape, dtype=torch.bfloat16):
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_wrapper_value_errors():
    x, h = _meta(4, 128), _meta(32, 32)
    for f in (lambda **kw: q.swiglu_oai_and_mul(x, **kw), lambda **kw: q.fusedSwigluOaiQuantizeMx(x, h, **kw)):
        for limit in BAD_LIMITS:
            with pytest.raises(ValueError, match="limit must be"):
                f(limit=limit)
        for alpha in BAD_ALPHAS:
            with pytest.raises(ValueError, match="alpha must be"):
                f(alpha=alpha)
        with pytest.raises(ValueError, match="needs offs"):
            f(bias=_meta(2, 128))
        with pytest.raises(ValueError, match="offs without a bias"):
            f(offs=_meta(2, dtype=torch.int32))
        with pytest.raises(ValueError, match=r"bias must be \(E, 2 \* I\)"):
            f(bias=_meta(1, 64))
        with pytest.raises(ValueError, match="offs must be an int32 tensor"):
            f(bias=_meta(2, 128), offs=_meta(3, dtype=torch.int32))
        with pytest.raises(ValueError, match="offs must be an int32 tensor"):
            f(bias=_meta(2, 128), offs=_meta(2, dtype=torch.int64))
        with pytest.raises(ValueError, match=r"\[1, 1024\]"):
            f(bias=_meta(1025, 128), offs=_meta(1025, dtype=torch.int32))
    with pytest.raises(ValueError, match="2 \\* I"):
        q.swiglu_oai_and_mul(_meta(4, 127))
    with pytest.raises(ValueError, match="swiglu_oai_and_mul followed by fusedQuantizeMx"):
        q.fusedSwigluOaiQuantizeMx(_meta(4, 256), _meta(128, 128))
    with pytest.raises(ValueError, match="invalid method"):
        q.fusedSwigluOaiQuantizeMx(x, h, method="max")
    y, pos, w = _meta(8, 64), _meta(4, 2, dtype=torch.int32), _meta(4, 2, dtype=torch.float32)
    with pytest.raises(ValueError, match=r"bias must be \(E, H\)"):
        q.moe_combine(y, pos, w, bias=_meta(2, 32), offs=_meta(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="needs offs"):
        q.moe_combine(y, pos, w, bias=_meta(2, 64))
    with pytest.raises(ValueError, match="offs without a bias"):
        q.moe_combine(y, pos, w, offs=_meta(2, dtype=torch.int32))


def test_fake_kernels_of_the_functional_ops():
    """shapes and dtypes of the three functional ops on meta tensors"""
    amd = torch.ops.qutlass_amd
    x, h = _meta(3, 35, 192), _meta(32, 32)
    bias, offs = _meta(4, 192), _meta(4, dtype=torch.int32)
    ref = q.ops.alloc_quant(q.ops.QUANT_OPS["quantize_mx"], _meta(3, 35, 96))
    for b, o in ((None, None), (bias, offs), (_meta(1, 192), None)):
        act = amd.swiglu_oai_and_mul(x, 1.702, 7.0, b, o)
        assert act.shape == (3, 35, 96) and act.dtype == torch.bfloat16 and act.device.type == "meta"
        codes, sf = amd.swiglu_oai_quantize_mx(x, h, 1.702, 7.0, b, o, 0)
        assert codes.shape == (3, 35, 48) and codes.dtype == torch.uint8
        assert sf.shape == ref[1].shape and sf.dtype == torch.float8_e8m0fnu
    y, pos, w = _meta(70, 136), _meta(33, 5, dtype=torch.int32), _meta(33, 5, dtype=torch.float32)
    out = amd.moe_combine_bias(y, pos, w, _meta(4, 136), offs)
    assert out.shape == (33, 136) and out.dtype == torch.bfloat16
    assert amd.moe_combine_bias(y, pos, w, _meta(1, 136), None).shape == (33, 136)


def test_schemas_and_registration():
    for n in ("swigluOaiAndMul_", "fusedSwigluOaiQuantizeMx_", "moeCombineBias_"):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
        assert written and len(schema.returns) == 0, str(schema)
        assert torch._library.simple_registry.singleton.find(f"qutlass_amd::{n}").fake_impl.kernel is not None
    assert q.ops.QUANT_OPS["swiglu_oai_quantize_mx"].twin == "fusedSwigluOaiQuantizeMx_"
    for n in ("swiglu_oai_and_mul", "swiglu_oai_quantize_mx", "moe_combine_bias"):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        assert not any(a.alias_info is not None for a in schema.arguments), str(schema)


def test_the_ops_trace_with_fullgraph():
    with FakeTensorMode():
        x, h = torch.empty(35, 256, dtype=torch.bfloat16, device="cuda"), torch.empty(64, 64, dtype=torch.bfloat16, device="cuda")
        b1, offs = torch.empty(4, 256, dtype=torch.bfloat16, device="cuda"), torch.empty(4, dtype=torch.int32, device="cuda")
        y, pos, w = torch.empty(35, 128, dtype=torch.bfloat16, device="cuda"), torch.empty(9, 4, dtype=torch.int32, device="cuda"), torch.empty(9, 4, device="cuda")
        b2 = torch.empty(4, 128, dtype=torch.bfloat16, device="cuda")

        def layer(x, h, b1, offs, y, pos, w, b2):
            c, s = q.fusedSwigluOaiQuantizeMx(x, h, bias=b1, offs=offs, method="abs_max")
            a = q.swiglu_oai_and_mul(x, bias=b1, offs=offs)
            return c, s, a, q.moe_combine(y, pos, w, bias=b2, offs=offs)

        c, s, a, o = torch.compile(layer, backend="eager", fullgraph=True)(x, h, b1, offs, y, pos, w, b2)
        assert c.shape == (35, 64) and a.shape == (35, 128) and o.shape == (9, 128)


def test_moe_combine_without_a_bias_is_the_old_op(monkeypatch):
    calls = []
    monkeypatch.setattr(q.ops, "run_output", lambda row, *a: calls.append(row.twin) or row.alloc(*a))   # the one runner of the eager wrappers: which twin, on what results
    y, pos, w = _meta(8, 64), _meta(4, 2, dtype=torch.int32), _meta(4, 2, dtype=torch.float32)
    out = q.moe_combine(y, pos, w)
    assert calls == ["moeCombine_"] and out.shape == (4, 64)
    out = q.moe_combine(y, pos, w, bias=None, offs=None)
    assert calls == ["moeCombine_", "moeCombine_"]


def test_eager_quantizer_sends_empty_tensors_for_a_missing_bias(monkeypatch):
    """the in-place twin takes tensors only: the eager wrapper goes through the runner that turns None into an empty tensor"""
    seen = []
    monkeypatch.setattr(q.ops, "run_quant", lambda row, *a: seen.append((row.twin, a[2:])) or "ran")
    x, h = _meta(4, 128), _meta(32, 32)
    assert q.fusedSwigluOaiQuantizeMx(x, h, method="abs_max") == "ran"
    assert seen == [("fusedSwigluOaiQuantizeMx_", (1.702, 7.0, None, None, 1))]
    e = q.ops._optional(x, None, torch.int32)
    assert e.numel() == 0 and e.dtype == torch.int32 and e.device == x.device and q.ops._optional(x, h, torch.int32) is h


# ---- the checkpoint layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [0, 1, -1])
def test_split_interleaved_gate_up(dim):
    t = torch.arange(4 * 6 * 8, dtype=torch.float32).reshape(4, 6, 8)
    got = split_interleaved_gate_up(t, dim)
    d = dim % 3
    idx = [slice(None)] * 3
    idx[d] = slice(0, None, 2)
    gate = t[tuple(idx)]
    idx[d] = slice(1, None, 2)
    up = t[tuple(idx)]
    assert got.shape == t.shape and torch.equal(got, torch.cat([gate, up], dim=d))
    half = t.size(d) // 2
    assert torch.equal(got.narrow(d, 0, half), gate) and torch.equal(got.narrow(d, half, half), up)
    with pytest.raises(ValueError, match="even"):
        split_interleaved_gate_up(torch.zeros(3, 5), 1)
    b = torch.tensor([[1, 2, 3, 4]], dtype=torch.uint8)      # a scale / bias row: even = gate, odd = up
    assert split_interleaved_gate_up(b, 1).tolist() == [[1, 3, 2, 4]]
