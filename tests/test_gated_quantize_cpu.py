"""Gated-MLP ops (silu_and_mul, fusedSiluMulQuantize{Mx,Nv}[Blocked]) without a GPU: the C ABI's argument checks (every one of them happens before any HIP call,
so null / dummy pointers are enough), the shape-only kernels of the torch ops, and the Python wrappers' own errors.  The GPU half is tests/test_gpu_gated_quantize.py."""
import ctypes

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import qutlass_amd as q
from qutlass_amd import _lib

DEV = "cuda"
OK, INVALID = _lib.QAMD_OK, _lib.QAMD_ERR_INVALID
X = 0x10000   # a 16-byte aligned dummy address: nothing below dereferences it


def _err():
    return _lib.load().qutlass_amd_last_error().decode()


def test_the_three_symbols_are_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("qutlass_amd_silu_mul_bf16", "qutlass_amd_fused_silu_mul_quantize_mx", "qutlass_amd_fused_silu_mul_quantize_nv"):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS


def test_silu_mul_argument_checks():
    f = _lib.load().qutlass_amd_silu_mul_bf16
    assert f(X, 0, 64, X, None) == OK                          # rows == 0: nothing to do
    assert f(None, 0, 64, None, None) == OK
    assert f(X, 4, 12, X, None) == INVALID and "multiple of 8" in _err()
    assert f(X, 4, 0, X, None) == INVALID
    assert f(X, -1, 64, X, None) == INVALID and "bad shape" in _err()
    assert f(X, 4, -8, X, None) == INVALID
    assert f(X, 1 << 31, 64, X, None) == INVALID
    assert f(X + 2, 4, 64, X, None) == INVALID and "16-byte aligned" in _err()
    assert f(X, 4, 64, X + 8, None) == INVALID and "16-byte aligned" in _err()
    assert f(None, 4, 64, X, None) == INVALID and "null pointer" in _err()
    assert f(X, 4, 64, None, None) == INVALID and "null pointer" in _err()


def _mx(rot, rows, inter, method=0, blocked=0, x=X, h=X, out=X, sf=X):
    return _lib.load().qutlass_amd_fused_silu_mul_quantize_mx(x, h, rot, rows, inter, method, blocked, out, sf, None)


def _nv(rot, rows, inter, method=1, blocked=0, x=X, h=X, gs=X, out=X, sf=X):
    return _lib.load().qutlass_amd_fused_silu_mul_quantize_nv(x, h, rot, rows, inter, method, gs, blocked, out, sf, None)


@pytest.mark.parametrize("blocked", [0, 1])
def test_fused_argument_checks(blocked):
    for call, rots, bad_rots in ((_mx, (32, 64, 128), (16, 0, 48, 256)), (_nv, (16, 32, 64, 128), (8, 0, 48, 256))):
        for rot in rots:
            rp = max(rot, 32)
            assert call(rot, 0, rp, blocked=blocked) == OK                                     # rows == 0 returns before any launch
            assert call(rot, 0, rp, blocked=blocked, x=None, h=None, out=None, sf=None) == OK
            assert call(rot, 4, rp + 16, blocked=blocked) == INVALID and f"multiple of {rp}" in _err()   # inter % max(rot, 32)
            assert call(rot, 4, 0, blocked=blocked) == INVALID
            assert call(rot, -1, rp, blocked=blocked) == INVALID and "bad shape" in _err()
            assert call(rot, 4, -rp, blocked=blocked) == INVALID
            for method in (-1, 2):
                assert call(rot, 4, rp, method=method, blocked=blocked) == INVALID and "invalid method" in _err()
            assert call(rot, 4, rp, blocked=blocked, x=X + 4) == INVALID and "16-byte aligned" in _err()
            for null in ("x", "h", "out", "sf"):
                assert call(rot, 4, rp, blocked=blocked, **{null: None}) == INVALID and "null pointer" in _err(), null
        for rot in bad_rots:
            assert call(rot, 4, 256, blocked=blocked) == INVALID and "Unsupported rotation size" in _err()
    assert _nv(32, 4, 64, blocked=blocked, gs=None) == INVALID and "null pointer" in _err()
    assert _mx(64, 4, 64, blocked=blocked, h=X + 2) == INVALID and "rotation matrix must be 16-byte aligned" in _err()


def test_fused_size_limit_is_checked_not_wrapped():
    """x = rows * 2 * inter * 2 bytes must stay below 2 GiB (32-bit offsets from one buffer descriptor): the first size beyond it is refused, for every form."""
    rows, inter = 1 << 15, 1 << 14        # rows * inter = 2^29: exactly 2 GiB of input
    for blocked in (0, 1):
        assert _mx(32, rows, inter, blocked=blocked) == INVALID and "below 2 GiB" in _err()
        assert _nv(16, rows, inter, blocked=blocked) == INVALID and "below 2 GiB" in _err()
        assert _mx(128, (1 << 29) // 128, 128, blocked=blocked) == INVALID and "below 2 GiB" in _err()
    assert _lib.load().qutlass_amd_silu_mul_bf16(X, 0, inter, X, None) == OK


@pytest.mark.parametrize("shape", [(70, 768), (2, 35, 768)])
def test_functional_ops_give_the_plain_quantizers_shapes_under_fake_tensors(shape):
    q.ops.register_torch_ops()
    amd = torch.ops.qutlass_amd
    inter, rows = shape[-1] // 2, 70
    with FakeTensorMode():
        x = torch.empty(*shape, dtype=torch.bfloat16, device=DEV)
        h = torch.empty(32, 32, dtype=torch.bfloat16, device=DEV)
        gs = torch.empty(1, device=DEV)
        act = amd.silu_and_mul(x)
        assert act.shape == (*shape[:-1], inter) and act.dtype == torch.bfloat16 and act.device.type == "cuda"
        for blocked in (False, True):
            c, s = amd.silu_mul_quantize_mx(x, h, 0, blocked)
            pc, ps = amd.quantize_mx_blocked(act, h, 0) if blocked else amd.quantize_mx(act, h, 0)
            assert c.shape == pc.shape == (*shape[:-1], inter // 2) and c.dtype == torch.uint8
            assert s.shape == ps.shape == ((128 * 12,) if blocked else (128, 12)) and s.dtype == torch.float8_e8m0fnu
            c, s = amd.silu_mul_quantize_nv(x, h, gs, 1, blocked)
            pc, ps = amd.quantize_nv_blocked(act, h, gs, 1) if blocked else amd.quantize_nv(act, h, gs, 1)
            assert c.shape == pc.shape == (*shape[:-1], inter // 2) and c.dtype == torch.uint8
            assert s.shape == ps.shape == ((128 * 24,) if blocked else (128, 24)) and s.dtype == torch.float8_e4m3fn
        # the eager wrappers (in-place twins on tensors they allocate) agree
        assert q.silu_and_mul(x).shape == act.shape
        for fn, pfn, extra in ((q.fusedSiluMulQuantizeMx, q.fusedQuantizeMx, ()), (q.fusedSiluMulQuantizeMxBlocked, q.fusedQuantizeMxBlocked, ()),
                               (q.fusedSiluMulQuantizeNv, q.fusedQuantizeNv, (gs,)), (q.fusedSiluMulQuantizeNvBlocked, q.fusedQuantizeNvBlocked, (gs,))):
            got, want = fn(x, h, *extra), pfn(act, h, *extra)
            assert [(t.shape, t.dtype) for t in got] == [(t.shape, t.dtype) for t in want], fn.__name__
    assert rows * inter // 32 <= 128 * 12


def test_in_place_twins_declare_their_writes():
    q.ops.register_torch_ops()
    for n, nwritten in (("siluAndMul_", 1), ("fusedSiluMulQuantizeMx_", 2), ("fusedSiluMulQuantizeNv_", 2)):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
        assert len(written) == nwritten and len(schema.returns) == 0, str(schema)
        assert torch._library.simple_registry.singleton.find(f"qutlass_amd::{n}").fake_impl.kernel is not None
    for n in ("silu_and_mul", "silu_mul_quantize_mx", "silu_mul_quantize_nv"):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        assert not any(a.alias_info is not None for a in schema.arguments), str(schema)


def test_gated_mlp_traces_with_fullgraph():
    def mlp(x, h, w2q, w2sf, alpha):      # the second half of a gated MLP: Q(silu(gate) * up . h) W2^T
        aq, asf = q.fusedSiluMulQuantizeMx(x, h, method="abs_max")
        return q.matmul_ada_mxf4_bf16_tn(aq.view(-1, aq.size(-1)), w2q, asf, w2sf, alpha)

    with FakeTensorMode():
        x = torch.empty(2, 35, 768, dtype=torch.bfloat16, device=DEV)
        h = torch.empty(32, 32, dtype=torch.bfloat16, device=DEV)
        w2q = torch.empty(256, 192, dtype=torch.uint8, device=DEV)
        w2sf = torch.empty(256, 12, dtype=torch.float8_e8m0fnu, device=DEV)
        out = torch.compile(mlp, backend="eager", fullgraph=True)(x, h, w2q, w2sf, torch.empty(1, device=DEV))
        assert out.shape == (70, 256) and out.dtype == torch.bfloat16
        c, s = torch.compile(lambda x, h: q.fusedSiluMulQuantizeMx(x, h), backend="eager", fullgraph=True)(x, h)
        assert c.shape == (2, 35, 192) and s.shape == (128, 12)
        act = torch.compile(q.silu_and_mul, backend="eager", fullgraph=True)(x)
        assert act.shape == (2, 35, 384)


def test_bad_method_raises_value_error():
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    h = torch.zeros(32, 32, dtype=torch.bfloat16)
    gs = torch.ones(1)
    for fn, extra in ((q.fusedSiluMulQuantizeMx, ()), (q.fusedSiluMulQuantizeMxBlocked, ()), (q.fusedSiluMulQuantizeNv, (gs,)), (q.fusedSiluMulQuantizeNvBlocked, (gs,))):
        with pytest.raises(ValueError, match="invalid method 'nope', must be 'quest' or 'abs_max'"):
            fn(x, h, *extra, method="nope")


def test_alias_package_exposes_the_new_functions():
    import qutlass

    for n in ("silu_and_mul", "fusedSiluMulQuantizeMx", "fusedSiluMulQuantizeNv", "fusedSiluMulQuantizeMxBlocked", "fusedSiluMulQuantizeNvBlocked"):
        assert getattr(qutlass, n) is getattr(q, n)
