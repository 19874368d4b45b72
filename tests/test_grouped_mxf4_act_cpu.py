"""The gate/up MXFP4 (W4A4) grouped GEMM with fused activation, rotation and MXFP4 output (grouped_matmul_mxf4_silu_mxf4_tn / ..._swiglu_oai_mxf4_tn) on the host: the
form rule and grid of the debug plan entry, the rejections of the C entry and of the Python ops, the fake kernel.  No GPU needed; the GPU half is
tests/test_gpu_grouped_mxf4_act.py."""
import ctypes
import re

import pytest
import torch

DEV = "cuda"
ENTRY = "qutlass_amd_grouped_matmul_mxf4_act_mxf4_tn"
PLAN = "qutlass_amd_debug_grouped_mxf4_act_plan"
E8M0 = torch.float8_e8m0fnu


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    L = _lib.load()
    getattr(L, PLAN).argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]   # (restype: ctypes' default, int)
    return L


@pytest.mark.parametrize("change,message", [(dict(N=96), "multiple of 64"), (dict(K=192), "K must be a positive multiple of 128"), (dict(E=1025), r"E must be in \[1, 1024\]"),
                                            (dict(rot=64), "rotation size 64 is not supported; expected 32 .*grouped_matmul_mxf4_bf16_tn"), (dict(method=2), "invalid method 2"),
                                            (dict(act=2), "invalid act 2"), (dict(limit=7.01), "exactly representable in bf16"), (dict(bias=0x1008), "bias must be 16-byte aligned"),
                                            (dict(act=0, bias=0x1000), "takes no bias"), (dict(), None)])
def test_c_entry_rejections(lib, change, message):
    a = {**dict(act=1, limit=7.0, bias=None, rot=32, method=0, M=0, N=128, K=256, E=4), **change}
    d = ctypes.c_void_p(0x1000)   # never dereferenced: every call here returns before a launch (the accepted one through M == 0)
    rc = getattr(lib, ENTRY)(d, d, d, d, d, 1, d, a["act"], 1.702, a["limit"], a["bias"], d, a["rot"], a["method"], d, d, a["M"], a["N"], a["K"], a["E"], None)
    assert (rc == 0) if message is None else (rc == 1 and re.search(message, lib.qutlass_amd_last_error().decode())), lib.qutlass_amd_last_error().decode()


@pytest.mark.parametrize("M,inter,K,E", [(16, 2944, 2944, 32), (64, 768, 2048, 128), (4096, 768, 2048, 128), (8192, 14336, 4096, 8), (128, 32, 1024, 4), (128, 32, 1152, 4),
                                         (127, 32, 1152, 4), (0, 64, 128, 1)])
def test_plan_is_pure_and_its_grid_is_grouped_workgroups(lib, M, inter, K, E):
    """only 616 (32 rows) and 617 (64 rows); the same answer every time; the grid is grouped_workgroups over tiles of 32 ACTIVATION columns"""
    out = (ctypes.c_int64 * 3)(-1, -1, -1)
    v = getattr(lib, PLAN)(M, 2 * inter, K, E, out)
    assert v in (616, 617) and all(getattr(lib, PLAN)(M, 2 * inter, K, E, None) == v for _ in range(3))
    tm = 32 * (v - 615)
    assert out[0] == (0 if M == 0 else ((M + tm - 1) // tm + E) * (inter // 32))
    assert (out[1], out[2]) == (3072, 2048), "the one-shot ladders of gemm_mx_os_mxf4_act.hip.h"
    assert getattr(lib, PLAN)(M, 2 * inter + 32, K, E, out) == -1, "N % 64"


def _operands(M=48, inter=64, K=256, E=4, adtype=torch.uint8, hshape=(32, 32), hdtype=torch.bfloat16):
    return [torch.zeros(M, K // 2, dtype=adtype), torch.zeros(E, 2 * inter, K // 2, dtype=torch.uint8), torch.zeros(M * K // 32, dtype=torch.uint8).view(E8M0),
            torch.zeros(E * 2 * inter * K // 32, dtype=torch.uint8).view(E8M0), torch.ones(1), torch.full((E,), M, dtype=torch.int32), torch.zeros(hshape, dtype=hdtype)]


def test_python_rejections_come_before_any_device_work():
    """CPU tensors on a machine that may have no GPU: each call raises its own message, so nothing was dispatched"""
    import qutlass
    import qutlass_amd as q

    silu, oai = q.grouped_matmul_mxf4_silu_mxf4_tn, q.grouped_matmul_mxf4_swiglu_oai_mxf4_tn
    assert qutlass.grouped_matmul_mxf4_silu_mxf4_tn is silu and qutlass.grouped_matmul_mxf4_swiglu_oai_mxf4_tn is oai
    for f in (silu, oai):
        assert f.__doc__.startswith("EXTENSION") and "one fp32 rounding" in " ".join(f.__doc__.split()) and f.__name__ in q.__doc__
        for kw, message in ((dict(hshape=(64, 64)), r"h must be a 32 x 32 rotation \(got \(64, 64\)\).*grouped_matmul_mxf4_bf16_tn followed by"),
                            (dict(hdtype=torch.float16), "h must be bfloat16"), (dict(adtype=torch.int8), "a must be uint8 or float4_e2m1fn_x2"),
                            (dict(inter=48), "I a multiple of 32"), (dict(K=192), r"K must be a multiple of 128 \(got 192\)"),
                            (dict(M=1, inter=32, K=128, E=1025), r"experts must be in \[1, 1024\] \(got 1025\)")):
            with pytest.raises(ValueError, match=message):
                f(*_operands(**kw))
        with pytest.raises(ValueError, match="invalid method 'rtn'"):
            f(*_operands(), method="rtn")
    for kw, message in ((dict(bias=torch.zeros(4, 64, dtype=torch.bfloat16)), r"bias must be \(E, 2 \* I\) = \(4, 128\)"), (dict(bias=torch.zeros(4, 128)), "bias must be bfloat16"),
                        (dict(limit=7.01), "limit must be > 0, finite and exactly representable in bf16"), (dict(act_alpha=float("nan")), "act_alpha must be finite and > 0")):
        with pytest.raises(ValueError, match=message):
            oai(*_operands(), **kw)


def test_fake_kernel_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import qutlass_amd as q

    q.ops.register_torch_ops()
    assert torch._library.simple_registry.singleton.find("qutlass_amd::grouped_matmul_mxf4_act_mxf4").fake_impl.kernel is not None
    M, inter, K, E = 160, 96, 256, 4
    with FakeTensorMode():
        args = (torch.empty(M, K // 2, dtype=torch.uint8, device=DEV), torch.empty(E, 2 * inter, K // 2, dtype=torch.uint8, device=DEV), torch.empty(M * K // 32, dtype=E8M0, device=DEV),
                torch.empty(E * 2 * inter * K // 32, dtype=E8M0, device=DEV), torch.empty(E, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV),
                torch.empty(32, 32, dtype=torch.bfloat16, device=DEV))
        for c, s in (q.grouped_matmul_mxf4_silu_mxf4_tn(*args, method="abs_max"),
                     q.grouped_matmul_mxf4_swiglu_oai_mxf4_tn(*args, bias=torch.empty(E, 2 * inter, dtype=torch.bfloat16, device=DEV))):
            assert tuple(c.shape) == (M, inter // 2) and c.dtype == torch.uint8 and tuple(s.shape) == (256, 4) and s.dtype == E8M0
