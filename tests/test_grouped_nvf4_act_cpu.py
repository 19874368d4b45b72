"""The gate/up NVFP4 (W4A4) grouped GEMM with fused activation, rotation and NVFP4 output (grouped_matmul_nvf4_silu_nvf4_tn / ..._swiglu_oai_nvf4_tn) on the host: the C
entry's declaration and binding, its own rejections and the Python ops', the form rule and grid of the debug plan entry, the fake kernel, and the exact-regime operands
of the GPU half.  No GPU needed; the GPU half is tests/test_gpu_grouped_nvf4_act.py."""
import ctypes
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import qutlass
import qutlass_amd as q
import test_gpu_grouped_nvf4_act as G   # (its numpy / CPU-only exact_operands and assert_exact)
from qutlass_amd import build

TORCH_OP = "grouped_matmul_nvf4_act_nvf4"
ENTRY, PLAN = "qutlass_amd_grouped_matmul_nvf4_act_nvf4_tn", "qutlass_amd_debug_grouped_nvf4_act_plan"
E4M3 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def lib():
    build.build()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    L = q._lib.load()
    getattr(L, PLAN).argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]   # (restype: ctypes' default, int)
    return L


def test_entry_is_declared_exported_and_bound(lib):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")).read()
    decl = re.search(r"\b" + ENTRY + r"\s*\(([^)]*)\)", hdr)
    assert decl is not None and len(decl.group(1).split(",")) == 22 == len(q._lib.SYMBOLS[ENTRY][1]) and PLAN not in hdr
    assert q._lib.SYMBOLS[ENTRY][1] == G.ACT_ARGS, "the binding's argument list is the one the GPU half calls the entry with"
    assert all(hasattr(L, n) for L in (lib, ctypes.CDLL(build.BENCH_OUT)) for n in (ENTRY, PLAN)), "the product and the lab library export both"


@pytest.mark.parametrize("change,message", [(dict(h=None), "null pointer"), (dict(gs=None), "null pointer"), (dict(out_sf=None), "null pointer"), (dict(A=None), "null pointer"),
                                            (dict(K=192), "K must be a positive multiple of 128"), (dict(N=96), "multiple of 64"), (dict(E=0), r"E must be in \[1, 1024\]"),
                                            (dict(E=1025), r"E must be in \[1, 1024\]"), (dict(n_alpha=3), "alpha must have 1 or E"), (dict(h_size=64), "rotation size 64 is not supported"),
                                            (dict(method=2), "method"), (dict(act=2), "invalid act 2"), (dict(act_alpha=0.0), "alpha must be finite and > 0"),
                                            (dict(limit=7.01), "exactly representable in bf16"), (dict(act=0, bias=0x1000), "takes no bias"),
                                            (dict(M=1 << 22, K=1024), r"token matrix \(M \* K/2 bytes"), (dict(N=1 << 22, K=1024), "one expert's weight"),
                                            (dict(act=1, bias=None), None), (dict(), None)])
def test_c_entry_boundaries(lib, change, message):
    """every call here returns before a launch (the accepted ones through M == 0); the pointers are never dereferenced"""
    a = {**dict(A=0x1000, h=0x1000, gs=0x1000, out_sf=0x1000, act=1, act_alpha=1.702, limit=7.0, bias=0x1000, h_size=32, method=1, n_alpha=1, M=0, N=128, K=256, E=4), **change}
    f, d = getattr(lib, ENTRY), ctypes.c_void_p(0x1000)
    f.argtypes = G.ACT_ARGS
    rc = f(a["A"], d, d, d, d, a["n_alpha"], d, a["act"], a["act_alpha"], a["limit"], a["bias"], a["h"], a["h_size"], a["gs"], a["method"], d, a["out_sf"],
           a["M"], a["N"], a["K"], a["E"], None)
    err = lib.qutlass_amd_last_error().decode()
    assert (rc == 0) if message is None else (rc == 1 and re.search(message, err) and "grouped_matmul_nvf4_act_nvf4_tn" in err), err


@pytest.mark.parametrize("M,inter,K,E,form", [(48 * 32, 2944, 2944, 32, 624), (48 * 32 + 1, 2944, 2944, 32, 625), (16, 1024, 8192, 8, 624), (8192, 14336, 4096, 8, 625),
                                              (49, 96, 128, 1, 625), (0, 64, 128, 1, 624)])
def test_plan_rule_and_grid(lib, M, inter, K, E, form):
    """the committed rule (capi.hip grouped_nvf4_act_plan: a mean of at most 48 rows per group -> 624, else 625; no wave-owned corner), pinned on either side of its
    threshold; the grid counts tiles of 32 / 64 ACTIVATION columns, (cdiv(M, TM) + E) * (I / TN) with a last partial tile counted whole"""
    out = (ctypes.c_int64 * 2)(-1, -1)
    assert getattr(lib, PLAN)(M, 2 * inter, K, E, out) == form
    TM, TN = (64, 32) if form == 624 else (128, 64)
    assert out[0] == (0 if M == 0 else ((M + TM - 1) // TM + E) * ((inter + TN - 1) // TN)) and out[1] == 512
    assert getattr(lib, PLAN)(M, 2 * inter + 32, K, E, out) == -1 and getattr(lib, PLAN)(M, 2 * inter, K + 64, E, out) == -1, "N % 64, K % 128"


def _operands(M=48, inter=64, K=256, E=4, cdtype=torch.uint8, sdtype=E4M3, hshape=(32, 32), hdtype=torch.bfloat16, gdtype=torch.float32, brank=3):
    b = torch.zeros(E, 2 * inter, K // 2, dtype=torch.uint8)
    return [torch.zeros(M, K // 2, dtype=cdtype), b if brank == 3 else b[0], torch.zeros(M * K // 16, dtype=torch.uint8).view(sdtype),
            torch.zeros(E * 2 * inter * K // 16, dtype=torch.uint8).view(E4M3), torch.ones(1), torch.full((E,), M, dtype=torch.int32), torch.zeros(hshape, dtype=hdtype),
            torch.ones(E, dtype=gdtype)]


def test_python_rejections_come_before_any_device_work():
    """CPU tensors on a machine that may have no GPU: each call raises its own message, so nothing was dispatched"""
    silu, oai = q.grouped_matmul_nvf4_silu_nvf4_tn, q.grouped_matmul_nvf4_swiglu_oai_nvf4_tn
    assert qutlass.grouped_matmul_nvf4_silu_nvf4_tn is silu and qutlass.grouped_matmul_nvf4_swiglu_oai_nvf4_tn is oai
    for f in (silu, oai):
        assert f.__doc__.startswith("EXTENSION") and "grouped_matmul_nvf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs)" in f.__doc__ and f.__name__ in q.__doc__
        for kw, message in ((dict(cdtype=torch.int8), f.__name__ + ": a must be uint8 or float4_e2m1fn_x2"), (dict(sdtype=torch.float8_e8m0fnu), "a_sf must be float8_e4m3fn"),
                            (dict(hdtype=torch.float16), "h must be bfloat16"), (dict(gdtype=torch.float64), "global_scales must be a 1D float32 tensor of E = 4"),
                            (dict(brank=2), "a must be 2D .* and b 3D"), (dict(hshape=(64, 64)), r"h must be a 32 x 32 rotation \(got \(64, 64\)\)"),
                            (dict(hshape=(32,)), "h must be a 32 x 32 rotation"), (dict(inter=48), "I a multiple of 32"), (dict(K=192), r"K must be a multiple of 128 \(got 192\)")):
            with pytest.raises(ValueError, match=message):
                f(*_operands(**kw))
        with pytest.raises(ValueError, match="invalid method 'max'"):
            f(*_operands(), method="max")
    for kw, message in ((dict(bias=torch.zeros(4, 64, dtype=torch.bfloat16)), r"bias must be \(E, 2 \* I\) = \(4, 128\)"), (dict(bias=torch.zeros(4, 128)), "bias must be bfloat16"),
                        (dict(limit=7.01), "limit must be > 0, finite and exactly representable in bf16"), (dict(act_alpha=float("nan")), "act_alpha must be finite and > 0")):
        with pytest.raises(ValueError, match=message):
            oai(*_operands(), **kw)


def test_schema_and_fake_kernel():
    q.ops.register_torch_ops()
    schema = str(getattr(torch.ops.qutlass_amd, TORCH_OP).default._schema)
    assert schema == (f"qutlass_amd::{TORCH_OP}(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha, Tensor offs, int act, float act_alpha, float limit, Tensor? bias, "
                      "Tensor h, Tensor global_scales, int method) -> (Tensor, Tensor)") and "!" not in schema
    assert [torch._C._dispatch_has_kernel_for_dispatch_key("qutlass_amd::" + TORCH_OP, k) for k in ("CompositeExplicitAutograd", "CUDA")] == [True, False]
    M, inter, K, E = 160, 96, 256, 4
    with FakeTensorMode():
        e = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="cuda")   # noqa: E731
        ops = (e(M, K // 2, dtype=torch.uint8), e(E, 2 * inter, K // 2, dtype=torch.uint8), e(M * K // 16, dtype=E4M3), e(E * 2 * inter * K // 16, dtype=E4M3), e(E),
               e(E, dtype=torch.int32), e(32, 32, dtype=torch.bfloat16), e(E))
        for codes, scales in (q.grouped_matmul_nvf4_silu_nvf4_tn(*ops), q.grouped_matmul_nvf4_swiglu_oai_nvf4_tn(*ops, method="quest", bias=e(E, 2 * inter, dtype=torch.bfloat16))):
            assert tuple(codes.shape) == (M, inter // 2) and codes.dtype == torch.uint8 and codes.device.type == "cuda"
            assert tuple(scales.shape) == (256, 8) == q.utils.padded_scale_shape(M, inter, 16) and scales.dtype == E4M3


@pytest.mark.parametrize("counts", ((20, 30), (60, 70)))
def test_exact_operands_of_the_gpu_half(counts):
    G.assert_exact(*G.exact_operands(counts))
