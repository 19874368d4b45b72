"""The gate/up W4A16 grouped GEMM on NVFP4 weights with fused activation (grouped_matmul_bf16_nvf4_silu_bf16_tn / ..._swiglu_oai_bf16_tn) on the host: the C entry's
declaration and binding, its own rejections and the Python ops', the form rule and grid of the debug plan entry, the fake kernel, and the operands of the GPU half's
fp64 cases (exact, and their gates span the clamp and zero).  No GPU needed; the GPU half is tests/test_gpu_grouped_bf16_nvf4_act.py."""
import ctypes
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import _bf16_nvf4_model as W
import qutlass
import qutlass_amd as q
import test_gpu_grouped_bf16_nvf4_act as G   # (its constants and the numpy-only fp64_case)
from qutlass_amd import build

TORCH_OP = "grouped_matmul_bf16_nvf4_act_bf16"
ENTRY, PLAN = "qutlass_amd_grouped_matmul_bf16_nvf4_act_bf16_tn", "qutlass_amd_debug_grouped_bf16_nvf4_act_plan"
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
    assert decl is not None and len(decl.group(1).split(",")) == 18 == len(q._lib.SYMBOLS[ENTRY][1])
    assert q._lib.SYMBOLS[ENTRY] == q._lib.SYMBOLS["qutlass_amd_grouped_matmul_bf16_mxf4_act_bf16_tn"] and PLAN not in hdr
    assert all(hasattr(L, n) for L in (lib, ctypes.CDLL(build.BENCH_OUT)) for n in (ENTRY, PLAN)), "the product and the lab library export both"


@pytest.mark.parametrize("change,message", [(dict(N=96), "multiple of 64"), (dict(act=1, bias=None, M=0), None), (dict(act=2), "invalid act 2"),
                                            (dict(act=0, bias=0x1000), "takes no bias"), (dict(bias=0x1008), "bias must be 16-byte aligned"),
                                            (dict(B_sf=0x1004), "B_sf must be 8-byte aligned"), (dict(B_sf=None), "null pointer"), (dict(D=0x1008), "D must be 16-byte aligned"),
                                            (dict(K=192), "K must be a positive multiple of 128"), (dict(E=1025), r"E must be in \[1, 1024\]"),
                                            (dict(n_alpha=3), "alpha must have 1 or E"), (dict(limit=7.01), "exactly representable in bf16"),
                                            (dict(src=0x1000, T=1 << 22, K=256), "gathered token matrix"), (dict(src=0x1000, T=-1), "T must be >= 0"), (dict(), None)])
def test_c_entry_boundaries(lib, change, message):
    """(the entry's act is 0 / 1 and the biased kernel is chosen by the bias pointer, so the biased kernel with a null bias cannot be asked for: act 1 with a null bias
    is the unbiased SwiGLU, accepted; a bias with act 0 is rejected)"""
    a = {**dict(act=1, limit=7.0, bias=0x1000, src=None, T=0, n_alpha=1, B_sf=0x1000, D=0x1000, M=0, N=128, K=256, E=4), **change}
    d = ctypes.c_void_p(0x1000)   # never dereferenced: every call here returns before a launch (the accepted ones through M == 0)
    rc = getattr(lib, ENTRY)(d, d, a["B_sf"], d, a["n_alpha"], d, a["src"], a["T"], a["act"], 1.702, a["limit"], a["bias"], a["D"], a["M"], a["N"], a["K"], a["E"], None)
    err = lib.qutlass_amd_last_error().decode()
    assert (rc == 0) if message is None else (rc == 1 and re.search(message, err) and "grouped_matmul_bf16_nvf4_act_bf16_tn" in err), err


@pytest.mark.parametrize("M,inter,K,E,form", [(16, 2944, 2944, 32, 622), (16384, 2944, 2944, 32, 622), (8192, 14336, 4096, 8, 623), (4096, 32, 512, 4, 622),
                                              (4096, 32, 640, 4, 623), (4095, 32, 640, 4, 622), (0, 64, 128, 1, 622)])
def test_plan_rule_and_grid(lib, M, inter, K, E, form):
    """the committed rule (capi.hip grouped_bf16_nvf4_act_plan: mean rows per group >= 1024 and K > 512 -> 623, else 622), pinned on either side of both
    thresholds; the grid counts tiles of 32 ACTIVATION columns"""
    out = (ctypes.c_int64 * 1)(-1)
    v = getattr(lib, PLAN)(M, 2 * inter, K, E, out)
    assert v == form
    TM = 32 * (v - 621)
    assert out[0] == (0 if M == 0 else ((M + TM - 1) // TM + E) * (inter // 32))
    assert getattr(lib, PLAN)(M, 2 * inter + 32, K, E, out) == -1 and getattr(lib, PLAN)(M, 2 * inter, K + 64, E, out) == -1, "N % 64, K % 128"


def _operands(M=48, inter=64, K=256, E=4, adtype=torch.bfloat16, sdtype=E4M3):
    return [torch.zeros(M, K, dtype=adtype), torch.zeros(E, 2 * inter, K // 2, dtype=torch.uint8), torch.zeros(E * 2 * inter * K // 16, dtype=torch.uint8).view(sdtype),
            torch.ones(1), torch.full((E,), M, dtype=torch.int32)]


def test_python_rejections_come_before_any_device_work():
    """CPU tensors on a machine that may have no GPU: each call raises its own message, so nothing was dispatched"""
    silu, oai = q.grouped_matmul_bf16_nvf4_silu_bf16_tn, q.grouped_matmul_bf16_nvf4_swiglu_oai_bf16_tn
    assert qutlass.grouped_matmul_bf16_nvf4_silu_bf16_tn is silu and qutlass.grouped_matmul_bf16_nvf4_swiglu_oai_bf16_tn is oai
    for f in (silu, oai):
        assert f.__doc__.startswith("EXTENSION") and "grouped_matmul_bf16_nvf4_bf16_tn(a, b, b_sf, alpha, offs, src_row=src_row)" in f.__doc__ and f.__name__ in q.__doc__
        for kw, message in ((dict(adtype=torch.float16), f.__name__ + ": a must be bfloat16"), (dict(sdtype=torch.float8_e8m0fnu), "b_sf must be float8_e4m3fn"),
                            (dict(inter=48), "I a multiple of 32"), (dict(K=192), r"K must be a multiple of 128 \(got 192\)"),
                            (dict(M=1, inter=32, K=128, E=1025), r"experts must be in \[1, 1024\] \(got 1025\)"),
                            (dict(src_row=torch.zeros(48, dtype=torch.int64)), "src_row must be a 1D int32 tensor")):
            with pytest.raises(ValueError, match=message):
                f(*_operands(**{k: v for k, v in kw.items() if k != "src_row"}), **{k: v for k, v in kw.items() if k == "src_row"})
    for kw, message in ((dict(bias=torch.zeros(4, 64, dtype=torch.bfloat16)), r"bias must be \(E, 2 \* I\) = \(4, 128\)"), (dict(bias=torch.zeros(4, 128)), "bias must be bfloat16"),
                        (dict(limit=7.01), "limit must be > 0, finite and exactly representable in bf16"), (dict(limit=0.0), "limit must be > 0"),
                        (dict(act_alpha=float("nan")), "act_alpha must be finite and > 0"), (dict(act_alpha=0.0), "act_alpha must be finite and > 0")):
        with pytest.raises(ValueError, match=message):
            oai(*_operands(), **kw)


def test_schema_and_fake_kernel():
    q.ops.register_torch_ops()
    assert str(getattr(torch.ops.qutlass_amd, TORCH_OP).default._schema) == (
        f"qutlass_amd::{TORCH_OP}(Tensor A, Tensor B, Tensor B_sf, Tensor alpha, Tensor offs, int act, float act_alpha, float limit, Tensor? bias, Tensor? src_row) -> Tensor")
    assert [torch._C._dispatch_has_kernel_for_dispatch_key("qutlass_amd::" + TORCH_OP, k) for k in ("CompositeExplicitAutograd", "CUDA")] == [True, False]
    T, M, inter, K, E = 40, 160, 96, 256, 4
    with FakeTensorMode():
        e = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="cuda")   # noqa: E731
        w = (e(E, 2 * inter, K // 2, dtype=torch.uint8), e(E * 2 * inter * K // 16, dtype=E4M3), e(E), e(E, dtype=torch.int32))
        for out in (q.grouped_matmul_bf16_nvf4_silu_bf16_tn(e(M, K, dtype=torch.bfloat16), *w),
                    q.grouped_matmul_bf16_nvf4_swiglu_oai_bf16_tn(e(T, K, dtype=torch.bfloat16), *w, bias=e(E, 2 * inter, dtype=torch.bfloat16), src_row=e(M, dtype=torch.int32))):
            assert tuple(out.shape) == (M, inter) and out.dtype == torch.bfloat16 and out.device.type == "cuda"


@pytest.mark.parametrize("K", (512, 1152))
def test_fp64_cases_of_the_gpu_half_are_exact_and_their_gates_span_the_clamp(K):
    """the reference alone: exact-regime operands, and gates below -limit, above +limit and of both signs in between, with the bias (oai_bias) and without (silu)"""
    W.assert_exact(G.fp64_case(K)[0], G.FP64_COUNTS)
    assert G._spans(G.fp64_gates(K, True)) and G._spans(G.fp64_gates(K, False))
