"""grouped_matmul_bf16_nvf4_bf16_tn on the host: the C entry's declaration and binding, the rejections that are its own (the shared ones are the other grouped ops'
files') and the Python wrappers', the plan rule and workgroup count, the torch op's schema and fake kernel, the exactness of the GPU half's operands.  No GPU needed."""
import ctypes
import os

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import _bf16_nvf4_model as W
import qutlass
import qutlass_amd as q
from qutlass_amd import build

OP = "grouped_matmul_bf16_nvf4_bf16_tn"
ENTRY, PLAN = "qutlass_amd_" + OP, "qutlass_amd_debug_grouped_bf16_nvf4_plan"
E4M3, I64 = torch.float8_e4m3fn, ctypes.c_int64
OK = dict(M=64, N=64, K=512, E=4, n_alpha=1, A=0x1000, B=0x1000, B_sf=0x1000, alpha=0x1000, offs=0x1000, D=0x1000, src_row=0, T=0)
CASES = [(dict(B_sf=0), "null pointer"), (dict(K=448), "K must be a positive multiple of 128"), (dict(D=0x1008), "D must be 16-byte aligned"),
         (dict(B_sf=0x1004), "B_sf must be 8-byte aligned"), (dict(K=4096, src_row=0x1000, T=(1 << 31) // 8192), "gathered token matrix"),
         (dict(src_row=0x1000, T=-1), "T must be >= 0"),   # below: accepted -- no rows, nothing launched; T unread without src_row
         (dict(M=0, n_alpha=4), None), (dict(M=0, K=4096, src_row=0x1000, T=(1 << 31) // 8192 - 1), None), (dict(M=0, T=-1), None)]


@pytest.fixture(scope="module")
def lib():
    build.build()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    return q._lib.load()


@pytest.mark.parametrize("over,words", CASES, ids=str)
def test_entry_rejections_name_the_op_and_come_before_any_launch(lib, over, words):
    a = dict(OK, **over)   # the pointers are never dereferenced: every call here returns before a launch
    p = lambda k: ctypes.c_void_p(a[k]) if a[k] else None
    rc = getattr(lib, ENTRY)(p("A"), p("B"), p("B_sf"), p("alpha"), a["n_alpha"], p("offs"), p("src_row"), a["T"], p("D"), a["M"], a["N"], a["K"], a["E"], None)
    msg = lib.qutlass_amd_last_error().decode()
    assert rc == 0 if words is None else (rc == 1 and words in msg and OP in msg), (rc, msg)


def test_plan_rule_at_its_threshold_and_workgroups(lib):
    grid = I64(-1)
    plan = lambda M, N, K, E: getattr(lib, PLAN)(I64(M), I64(N), I64(K), I64(E), ctypes.byref(grid))
    for M, want, TM in ((0, 620, 32), (8 * 1024 - 1, 620, 32), (8 * 1024, 621, 64)):   # capi.hip grouped_bf16_nvf4_plan: mean rows per group, 8 experts
        assert plan(M, 40, 2944, 8) == want and grid.value == (((M + TM - 1) // TM + 8) * 2 if M else 0), (M, grid.value)
    assert plan(64, 2048, 4000, 8) == -1 and plan(64, 2044, 4096, 8) == -1 and plan(64, 2048, 4096, 1025) == -1 and plan(8192, 64, 131072, 8) == -1


def _operands(M=96, N=64, K=512, E=4, adtype=torch.bfloat16, bdtype=torch.uint8, sdtype=E4M3):
    return [torch.zeros(M, K, dtype=adtype), torch.zeros(E, N, K // 2, dtype=torch.uint8).view(bdtype), torch.zeros(E * N * K // 16, dtype=torch.uint8).view(sdtype),
            torch.ones(1), torch.full((E,), M, dtype=torch.int32)]


def test_wrapper_rejections_come_before_any_device_work():
    o, i64, col = _operands(), torch.zeros(96, dtype=torch.int64), torch.zeros(96, 1, dtype=torch.int32)
    for args, kw, words in ((_operands(adtype=torch.float16), {}, OP + r": a must be bfloat16 \(got torch.float16"),
                            (_operands(bdtype=torch.float8_e4m3fn), {}, r"b must be uint8 or float4_e2m1fn_x2"),
                            (o[:1] + [torch.zeros(4, 64, 512, dtype=torch.uint8)] + o[2:], {}, r"inner dimensions must match"),
                            (o[:1] + [o[1][0]] + o[2:], {}, r"a must be 2D \(M, K\) and b 3D \(E, N, K/2\)"),
                            (o[:2] + [o[2][:-1]] + o[3:], {}, r"b_sf has 8191 elements, the row-major scale layout needs 8192"),
                            (_operands(sdtype=torch.float8_e8m0fnu), {}, r"b_sf must be float8_e4m3fn"),
                            (o, dict(src_row=i64), r"src_row must be a 1D int32 tensor \(got torch.int64"), (o, dict(src_row=col), r"src_row must be a 1D int32 tensor")):
        with pytest.raises(ValueError, match=words):
            q.grouped_matmul_bf16_nvf4_bf16_tn(*args, **kw)
    a, b, bsf, alpha, _ = _operands(E=1)
    with pytest.raises(ValueError, match=r"matmul_bf16_nvf4_bf16_tn: a must be bfloat16"):
        q.matmul_bf16_nvf4_bf16_tn(a.float(), b[0], bsf, alpha)
    with pytest.raises(ValueError, match=r"b 2D \(N, K/2\)"):
        q.matmul_bf16_nvf4_bf16_tn(a, b, bsf, alpha)


def test_declared_bound_schema_and_fake_kernel(lib):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")).read()
    assert ENTRY + "(" in hdr and PLAN not in hdr and q._lib.SYMBOLS[ENTRY] == q._lib.SYMBOLS["qutlass_amd_grouped_matmul_bf16_mxf4_bf16_tn"] and all(
        hasattr(L, n) for L in (lib, ctypes.CDLL(build.BENCH_OUT)) for n in (ENTRY, PLAN)) and qutlass.matmul_bf16_nvf4_bf16_tn is q.matmul_bf16_nvf4_bf16_tn
    q.ops.register_torch_ops()
    assert str(getattr(torch.ops.qutlass_amd, OP).default._schema) == f"qutlass_amd::{OP}(Tensor A, Tensor B, Tensor B_sf, Tensor alpha, Tensor offs, Tensor? src_row) -> Tensor"
    assert [torch._C._dispatch_has_kernel_for_dispatch_key("qutlass_amd::" + OP, k) for k in ("CompositeExplicitAutograd", "CUDA")] == [True, False]
    M, N, K, E, T = 96, 256, 512, 4, 24
    with FakeTensorMode():
        e = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="cuda")
        b, b_sf, alpha, offs = e(E, N, K // 2, dtype=torch.float4_e2m1fn_x2), e(E * N * K // 16, dtype=E4M3), e(E), e(E, dtype=torch.int32)
        for out in (qutlass.grouped_matmul_bf16_nvf4_bf16_tn(e(M, K, dtype=torch.bfloat16), b, b_sf, alpha, offs),
                    q.grouped_matmul_bf16_nvf4_bf16_tn(e(T, K, dtype=torch.bfloat16), b, b_sf, alpha, offs, src_row=e(M, dtype=torch.int32)),   # the rows are src_row's
                    q.matmul_bf16_nvf4_bf16_tn(e(M, K, dtype=torch.bfloat16), b[0], b_sf, alpha[:1])):
            assert out.shape == (M, N) and out.dtype == torch.bfloat16 and out.device.type == "cuda"


def test_exact_regime_holds_for_every_case_the_gpu_half_uses():
    for K, N in W.LADDER:
        p, _, _, _, seen = W.ladder_case(K, N)
        W.assert_exact(p, W.COUNTS)
        W.assert_exact(p, W.COUNTS, x=seen)
    W.assert_exact(W.exact_problem(1, 24, 640, 45, seed=5), [45])
